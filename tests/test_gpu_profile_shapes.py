"""GPU sampling on every profile shape the trainer writes (`seqToProfile -k 1..5 -B 10..L`): simuReads FASTQ = oracle(philox)
byte for byte on profiles of tests/profile_shapes.py, whose rows all differ (an off-by-one context, bin or mate table
changes bytes), with all-zero / one-hot / identity-less substitution rows and all-zero / single-symbol quality rows.

The matrix holds a shape on each side of every boundary of the emit kernels' choice (sg_kernels.hip emit_lds /
emit_path, 160 KiB of LDS; EMIT_WAVES 16, META_ROW 32 and the straight-line kernel's layout, FastLds, in sg_emit.h):
substitution rows go to LDS while 32 KiB + contexts x bins x 16 B
fits; the straight-line kernel (k-mer 3 only) while its table image -- bins x (192 + 4 W) words, W the alias columns --
and its queues fit, its deferred items then go to emit_slow_kernel<3, rows in LDS or not>.  Each row states the path it
must take (the `--stats` line: sg_emit_path of the last pass), and straight-line rows must have queued items for
emit_slow_kernel (it returns at once on an empty queue) and give the same bytes with the generic kernel (SG_DIAG=0).
The CPU side of the same shapes: oracle(mt) = the unmodified reference in tests/test_profile_shapes_cpu.py."""
import os
import re
import subprocess
import time

import pytest

import cases
import histo_util as H
import profile_shapes as PS
from profile_shapes import Shape

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMU = os.path.join(ROOT, "simuscop_amd", "lib", "simuReads")
SEED = (cases.FAKE_SEC << 32) | cases.FAKE_NSEC

STRAIGHT, K3_LDS, ANY_LDS, GLOBAL = 1, 2, 3, 4     # SG_EMIT_* (include/simuscop_amd.h)

# (shape, layout, main kernel, emit_slow_kernel rows in LDS (1 / 0; -1 no slow kernel), clean_cap or None)
MATRIX = [
    (Shape(3, 53), "PE", STRAIGHT, 1, 0),                       # the largest straight-line image at W 64: no clean list
    (Shape(3, 52), "SE", STRAIGHT, 1, 64),                      # ... one bin less: a 64-entry list
    (Shape(3, 54), "PE", K3_LDS, -1, None),                     # image too large at W 64
    (Shape(3, 97), "SE", K3_LDS, -1, None),                     # the last rows that fit LDS at k 3
    (Shape(3, 98), "PE", GLOBAL, -1, None),
    (Shape(3, 151), "PE", GLOBAL, -1, None),                    # bins = L
    (Shape(3, 90, n_qual_mass=16), "PE", STRAIGHT, 1, 128),     # W 16: straight-line at a bin count the shipped files never had
    (Shape(3, 100, n_qual_mass=8), "PE", STRAIGHT, 0, 192),     # W 8: straight-line, emit_slow_kernel<3, false>
    (Shape(3, 30, n_qual_mass=70), "PE", STRAIGHT, 1, 256),     # W 128 (lgW 7) in the straight-line kernel
    (Shape(3, 60, n_qual_mass=70), "SE", K3_LDS, -1, None),     # W 128 in the generic kernel
    (Shape(4, 24), "PE", ANY_LDS, -1, None),
    (Shape(4, 25), "PE", GLOBAL, -1, None),
    (Shape(4, 30, mate2=False), "PE", GLOBAL, -1, None),        # PE without a mate-2 table: mate 2 from the mate-1 rows
    (Shape(2, 409, read_length=410), "PE", ANY_LDS, -1, None),
    (Shape(2, 410, read_length=410), "SE", GLOBAL, -1, None),
    (Shape(5, 10), "PE", GLOBAL, -1, None),
    (Shape(5, 151), "PE", GLOBAL, -1, None),
    (Shape(5, 250, read_length=250), "PE", GLOBAL, -1, None),
    (Shape(5, 20, bases="ACGT"), "PE", GLOBAL, -1, None),       # remapped base order, five-base contexts
    (Shape(1, 50, n_qual_mass=1), "SE", ANY_LDS, -1, None),     # one quality symbol per row: W 4
    (Shape(1, 702, read_length=1000, n_qual_mass=4), "PE", ANY_LDS, -1, None),   # the largest bins accepted at L 1000
]
IDS = [f"{s.tag}_{lay}" for s, lay, *_ in MATRIX]


def _files(d):
    return sorted(x for x in os.listdir(d) if ".fq" in x)


def _stat(stderr, key):
    return int(re.search(key + r"=(-?\d+)", stderr).group(1))


def first_difference(a, b, what):
    n = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    lo = a.rfind(b"\n@", 0, n) + 1
    return (f"{what}: first difference at byte {n} (sizes {len(a)} vs {len(b)})\n"
            f"oracle: {a[lo:lo + 400]!r}\ngpu:    {b[lo:lo + 400]!r}")


def run_gpu(cfg, out, env=None):
    r = subprocess.run([SIMU, cfg, "--seed", str(SEED), "--out", out, "--quiet", "--stats"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def assert_gpu_equals_oracle(oracle_lib, cfg, wd, what, env=None, oracle_dir=None):
    """simuReads (GPU) on `cfg` = oracle(philox) byte for byte; returns the --stats text of the GPU run."""
    odir, gdir = oracle_dir or os.path.join(wd, "oracle_out"), os.path.join(wd, "gpu_out" + ("_" + "_".join(env) if env else ""))
    if oracle_dir is None:
        rc = oracle_lib.orc_simulate(cfg.encode(), 1, cases.FAKE_SEC, cases.FAKE_NSEC, odir.encode(), 8)
        assert rc == 0, oracle_lib.orc_last_error().decode()
    err = run_gpu(cfg, gdir, env)
    assert _files(odir) == _files(gdir) and _files(odir)
    for f in _files(odir):
        a = open(os.path.join(odir, f), "rb").read()
        b = open(os.path.join(gdir, f), "rb").read()
        if a != b:
            pytest.fail(first_difference(a, b, f"{what}/{f}"))
    return err


_PATHS = {}


@pytest.mark.parametrize("shape,layout,main,slow_lds,clean_cap", MATRIX, ids=IDS)
def test_fastq_identical_to_oracle(shape, layout, main, slow_lds, clean_cap, oracle_lib, tmp_path):
    wd = str(tmp_path)
    cfg = PS.build_shape_case(shape, wd, layout)
    err = assert_gpu_equals_oracle(oracle_lib, cfg, wd, shape.tag)
    got = (_stat(err, "emit_kernel"), _stat(err, "slow_rows_lds"), _stat(err, "clean_cap"))
    _PATHS[(shape, layout)] = got
    assert got[:2] == (main, slow_lds), err
    if clean_cap is not None:
        assert got[2] == clean_cap, err
    if main == STRAIGHT:
        # emit_slow_kernel did work (N and X windows, reads of >= 2 sequencing indels), and the generic kernel alone agrees
        assert _stat(err, "queued_items") > 0 and _stat(err, "requeued_batches") == 0, err
        err0 = assert_gpu_equals_oracle(oracle_lib, cfg, wd, shape.tag + " SG_DIAG=0", env={"SG_DIAG": "0"},
                                        oracle_dir=os.path.join(wd, "oracle_out"))
        assert _stat(err0, "emit_kernel") != STRAIGHT and _stat(err0, "queued_items") == 0, err0


def test_matrix_reaches_every_path():
    """Every path of the emit kernels' choice is in the matrix, and every row took the path it states (rows run in this
    session; the whole file runs them all before this test)."""
    want = {(m, s) for _, _, m, s, _ in MATRIX}
    assert want == {(STRAIGHT, 1), (STRAIGHT, 0), (K3_LDS, -1), (ANY_LDS, -1), (GLOBAL, -1)}
    assert {c for *_, m, s, c in MATRIX if m == STRAIGHT} == {0, 64, 128, 192, 256}   # clean_cap shrunk to 0, to 64 and between
    assert {s.W for s, *_ in MATRIX} >= {4, 8, 16, 64, 128} and {s.kmer for s, *_ in MATRIX} == {1, 2, 3, 4, 5}
    assert len(_PATHS) == len(MATRIX), "run the whole file: the matrix rows record the paths they took"
    for shape, layout, m, s, _ in MATRIX:
        assert _PATHS[(shape, layout)][:2] == (m, s), (shape, layout)


@pytest.mark.parametrize("shape", [Shape(5, 30, indel_scale=0.0, edge_rows=False), Shape(3, 151, indel_scale=0.0, edge_rows=False)], ids=["k5_b30", "k3_bins_eq_L"])
def test_histograms_of_what_the_gpu_emitted(shape, oracle_lib, tmp_path):
    """G1 (substitutions by bin x context) and G2 (qualities by bin x reference x called base), with G3, of the GPU's own
    bytes against the closed form of the profile: no oracle in between (tests/test_histograms_closed_form.py).  SE runs,
    both strands: the mate-2 analysis of a PE run places each mate 2 by its mismatches, which at these shapes' error rates
    (up to 30 % a row) keeps the reads with fewer substitutions -- the reference's own bytes fail it there as well."""
    wd, layout = str(tmp_path), "SE"
    prof = PS.write_profile(os.path.join(wd, shape.tag + ".profile"), shape)
    cfg, fa = H.histogram_config(cases, wd, prof, layout, 12, 350)
    run_gpu(cfg, os.path.join(wd, "out"))
    rep = H.analyse_run(oracle_lib, cases, None, layout, 350, fa, cases.output_files(cfg), f"{shape.tag} {layout} GPU", want_gc=False,
                        profile_path=prof)
    assert rep["mate1"]["reads_used"] > 20_000 and rep["mate1"]["substitutions"] > 50_000, rep


def test_simureads_refuses_a_profile_past_the_bin_arithmetic_limit(tmp_path):
    """One bin more than the largest accepted at L 1000 (tests/test_profile_shapes_cpu.py pins the boundary in
    sg_profile_prepare): the command line exits non-zero with the message (after sg_create: hence a GPU test)."""
    cfg = PS.build_shape_case(Shape(1, 703, read_length=1000, n_qual_mass=4), str(tmp_path), "SE")
    r = subprocess.run([SIMU, cfg, "--quiet"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "read_length * bins too large for the 32-bit bin arithmetic" in r.stderr, r.stderr[-2000:]
