"""CPU pins of the profile shapes the trainer writes (`seqToProfile -k 1..5 -B 10..L`; tests/profile_shapes.py): the
shapes of tests/test_gpu_profile_shapes.py, where the GPU is held to oracle(philox), are held here to the reference:
  * oracle(mt) = the unmodified reference simuReads, byte for byte, PE and SE (where oracle/_ref is not built, its
    recorded runs in golden/reference_runs.json; the key holds the md5 of the profile and of the genome);
  * the closed-form histograms G1 / G2 at k-mer 5 with bins = L, on both oracle modes, and their power: the same counts
    held against the table shifted by one bin or by one context fail;
  * the integer tables keep every count; the 32-bit bin arithmetic's limit in build_tables, at its exact boundary (the
    command line's refusal of such a profile comes after the engine's sg_create: tests/test_gpu_profile_shapes.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import histo_util as H
import profile_shapes as PS
import ref_runs
import simuscop_amd
import test_gpu_profile_shapes as GS
import test_integer_tables as TI
from profile_shapes import Shape

SHAPES = list(dict.fromkeys(s for s, *_ in GS.MATRIX))


@pytest.mark.parametrize("layout", ["PE", "SE"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s.tag for s in SHAPES])
def test_oracle_mt_equals_the_reference(shape, layout, oracle_lib, tmp_path):
    wd = str(tmp_path)
    cfg = PS.build_shape_case(shape, wd, layout)
    out = os.path.join(wd, "out")
    key = f"shape/{layout}/{PS.md5(os.path.join(wd, shape.tag + '.profile'))}/{PS.md5(os.path.join(wd, 'ref.fa'))}"
    rc, want = ref_runs.run(key, cfg, out, timeout=600)
    assert rc == 0 and len(want) == (2 if layout == "PE" else 1)
    assert oracle_lib.orc_simulate(cfg.encode(), 0, cases.FAKE_SEC, cases.FAKE_NSEC, b"", 1) == 0, oracle_lib.orc_last_error().decode()
    assert all(os.path.getsize(os.path.join(out, f)) > 100_000 for f in want)
    assert ref_runs.md5s(out) == want


K5_BINS_L = Shape(5, 151, indel_scale=0.0, edge_rows=False)   # (no sequencing indels: an insertion and a deletion of one size would blur G1)


@pytest.mark.parametrize("mode", [0, 1], ids=["mt", "philox"])
def test_histograms_at_k5_bins_eq_L(mode, oracle_lib, tmp_path):
    """G1-G4 of the oracle's bytes (mt: the reference's own, philox: the GPU's spec) on a k-mer 5 profile with one bin per
    read position: contexts of length 5, X-prefixed at read starts, bin = i * bins // L.  SE, both strands (see
    tests/test_gpu_profile_shapes.py: the mate-2 placement of the PE analysis is biased at these error rates)."""
    wd = str(tmp_path)
    prof = PS.write_profile(os.path.join(wd, "p.profile"), K5_BINS_L)
    cfg, fa = H.histogram_config(cases, wd, prof, "SE", 10, 350)
    assert oracle_lib.orc_simulate(cfg.encode(), mode, 1600000000, 11, b"", 8 if mode else 1) == 0, oracle_lib.orc_last_error().decode()
    rep = H.analyse_run(oracle_lib, cases, None, "SE", 350, fa, cases.output_files(cfg), f"k5 bins=L mode {mode}", want_gc=False,
                        profile_path=prof)
    assert rep["mate1"]["reads_used"] > 20_000 and rep["mate1"]["substitutions"] > 100_000, rep


def test_the_analysis_detects_a_shifted_bin_or_context(oracle_lib, tmp_path):
    """Power of G1 / G2 at such a shape: mate-1 counts pass against their own table and fail against it shifted by one bin
    (substitutions, qualities) or by one context."""
    wd = str(tmp_path)
    prof = PS.write_profile(os.path.join(wd, "p.profile"), Shape(5, 30, indel_scale=0.0, edge_rows=False))
    cfg, fa = H.histogram_config(cases, wd, prof, "PE", 10, 350)
    assert oracle_lib.orc_simulate(cfg.encode(), 1, 5, 5, b"", 8) == 0
    T = H.ProfileTables(oracle_lib, prof, True, 350)
    ref = H.read_fasta_one(fa)
    fq = H.Fastq(cases.output_files(cfg)[0])
    rows = np.flatnonzero((fq.len == T.L) & (fq.pos + 1000 <= len(ref)))
    sub, qual, used, _ = H.sub_and_quality_counts(T, fq, H.forward_source(ref, fq, T.L), rows, False)
    H.check_sub_and_quality(T, sub, qual, False, "mate 1 against its own table")
    good_sub, good_qual = T.sub[0].copy(), T.qual.copy()
    for what, sub_t, qual_t in (("substitutions one bin on", np.roll(good_sub, 1, axis=1), good_qual),
                                ("qualities one bin on", good_sub, np.roll(good_qual, 1, axis=1)),
                                ("one context on, same last base", np.roll(good_sub, 4, axis=0), good_qual)):
        T.sub, T.qual = [sub_t, sub_t], qual_t
        with pytest.raises(AssertionError):
            H.check_sub_and_quality(T, sub, qual, False, what)


COUNT_SHAPES = [Shape(5, 20, bases="ACGT"), Shape(3, 30, n_qual_mass=70), Shape(1, 50, n_qual_mass=1), Shape(3, 100, n_qual_mass=8),
                Shape(4, 25)]


@pytest.mark.parametrize("shape", COUNT_SHAPES, ids=[s.tag for s in COUNT_SHAPES])
def test_tables_keep_every_count(shape, oracle_lib, tmp_path):
    """test_integer_tables' check on generated shapes: five-base contexts in another base order, W 128, W 4 with one symbol a
    row, all-zero and single-symbol rows."""
    TI.check_tables_keep_every_count(oracle_lib, PS.write_profile(str(tmp_path / "p.profile"), shape), shape.tag)


def prepare(shape):
    """sg_profile_prepare (host only) on tables of `shape`'s size: (code, message)."""
    lib = simuscop_amd.load_engine()
    lib.sg_profile_prepare.argtypes = [C.POINTER(simuscop_amd.SgProfileCdf), C.POINTER(C.c_void_p)]
    lib.sg_profile_tables_error.argtypes = [C.c_void_p]
    lib.sg_profile_tables_error.restype = C.c_char_p
    lib.sg_profile_tables_free.argtypes = [C.c_void_p]
    kc = sum(4 ** m for m in range(1, shape.kmer + 1))
    sub = np.tile(np.array([0.97, 0.98, 0.99, 1.0]), kc * shape.bins)
    qual = np.tile(np.linspace(1.0 / PS.N_QUAL, 1.0, PS.N_QUAL), 16 * shape.bins)
    n_ins = PS.n_ins(shape)
    ins = np.linspace(1.0 / n_ins, 1.0, n_ins)
    p = simuscop_amd.SgProfileCdf(n_bases=4, bases=shape.bases.encode(), kmer=shape.kmer, bins=shape.bins, read_length=shape.read_length,
                                  n_qual=PS.N_QUAL, min_qual=33, insert_rate=1e-3, del_rate=1e-3, n_ins=n_ins, n_del=n_ins, insert_size=350)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    p.ins_cdf = p.del_cdf = dp(ins)
    p.subs_cdf1 = dp(sub)
    p.qual_cdf = dp(qual)
    t = C.c_void_p()
    rc = lib.sg_profile_prepare(C.byref(p), C.byref(t))
    msg = lib.sg_profile_tables_error(t).decode()
    lib.sg_profile_tables_free(t)
    return rc, msg


LIMIT_MSG = "sg_load_profile: read_length * bins too large for the 32-bit bin arithmetic"


def largest_bins(L, n_ins):
    """The bin arithmetic (bin = i * bins / n' with a 32-bit reciprocal) is exact while n'max^2 * bins < 2^32, n'max = L +
    SG_MAX_EVENTS (32) insertions of the longest length."""
    npmax = L + 32 * n_ins
    return ((1 << 32) - 1) // (npmax * npmax)


def test_bin_arithmetic_limit_at_its_exact_boundary():
    n_ins = PS.n_ins(Shape(1, 10))
    assert largest_bins(1000, n_ins) == 702     # (the GPU matrix samples this shape)
    assert prepare(Shape(1, 702, read_length=1000, n_qual_mass=4)) == (0, "")
    assert prepare(Shape(1, 703, read_length=1000, n_qual_mass=4)) == (3, LIMIT_MSG)     # SG_ERR_UNSUPPORTED
    # along bins = L: the largest read length accepted with one bin per position, the next one refused
    Lmax = max(x for x in range(100, 2000) if largest_bins(x, n_ins) >= x)
    assert prepare(Shape(1, Lmax, read_length=Lmax, n_qual_mass=4)) == (0, "")
    assert prepare(Shape(1, Lmax + 1, read_length=Lmax + 1, n_qual_mass=4)) == (3, LIMIT_MSG)
