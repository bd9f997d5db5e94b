"""True allele counts on the MI355X through a Session (sg_variants.hip): after every sampling pass the device's counters
equal, row by row and exactly, what the label-level model (tests/variant_model.py) counts for the same reads -- their
templates from sg_truth_reads, the piece map from sg_truth_pieces, the chains' bases from sg_haplotype_codes.  Cases: the
suite's variant run, the four-clone mixture into one state, and a crowded two-contig case made here; add twice, reset,
begin again, and the calls that are refused."""
import ctypes as C

import numpy as np
import pytest

import cases
import simuscop_amd
import test_gpu_truth_bam as TB
import variant_util as VU
from variant_model import DEL, INS, SNV

pytestmark = pytest.mark.gpu


def run_passes(sess, L, paired, popus, reads_of):
    """Every (population, chromosome) pass into one state; the device's counts against the model's after each."""
    table = sess.variant_table()
    want = np.zeros((len(table), 2), dtype=np.int64)
    passes = expanded = hit_sum = 0
    for p in popus:
        sess.weighted_length(p)
        sess.set_reads(reads_of(p), p)
        for chrom in range(sess.n_chromosomes):
            if not sess.prepare_batch(chrom, p):
                continue
            if passes == 0:
                assert sess.variants_info() == (len(table), 0, 0)   # (the driver began the counts with its table)
            sess.sample()
            sess.result()
            step, n_exp = VU.model_counts(sess, L, table, paired)
            reads_hit, hits = sess.variants_add()
            want += step
            got = sess.variants_counts().astype(np.int64)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert not len(bad), (p, chrom, len(bad), table[bad[0]], got[bad[0]].tolist(), want[bad[0]].tolist())
            assert hits == int(step[:, 1].sum()) and reads_hit <= min(hits, n_exp) and (reads_hit > 0) == (hits > 0)
            passes += 1
            expanded += n_exp
            hit_sum += hits
    assert sess.variants_info()[0] == len(table) and sess.variants_info()[2] == hit_sum
    return table, want, passes, expanded


@pytest.fixture(scope="module")
def wgs(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("wgs"))
    cfg = cases.build_case("wgs_pe_variants", wd)
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=TB.SEED, truth_variants=1) as sess:
        L = VU.read_length(cfg)
        table, want, passes, expanded = run_passes(sess, L, True, [0], lambda p: sess.planned_reads)
        yield sess, L, table, want, passes, expanded


def test_wgs_pe_variants(wgs):
    sess, L, table, want, passes, expanded = wgs
    assert passes >= 2 and expanded > 1000
    kinds = {k: want[[i for i, r in enumerate(table) if r[1] == k]] for k in (SNV, INS, DEL)}
    for k in (SNV, INS, DEL):                                   # every kind of row is met, as reference and as allele
        assert kinds[k][:, 1].sum() > 0 and kinds[k][:, 0].sum() > 0, k
    assert (want[:, 0] <= want[:, 1]).all() and (want[:, 1] == 0).any()     # (at coverage 2 some rows are met by no read)


def test_add_again_reset_and_begin_again(wgs):
    """A second add of the same pass adds it again; reset zeroes counters and sums and keeps the table; a table of the
    caller's replaces the state; end frees it, and the calls are refused again."""
    sess, L, table, want, _, _ = wgs
    assert sess.prepare_batch(0)
    sess.sample()
    sess.result()
    before = sess.variants_counts().astype(np.int64)
    step, _ = VU.model_counts(sess, L, table, True)
    assert step[:, 1].sum() > 100
    sess.variants_add()
    assert np.array_equal(sess.variants_counts().astype(np.int64), before + step)
    before += step
    sess.variants_add()
    assert np.array_equal(sess.variants_counts().astype(np.int64), before + step)
    sess.variants_reset()
    assert not sess.variants_counts().any() and sess.variants_info() == (len(table), 0, 0)
    sess.variants_add()
    assert np.array_equal(sess.variants_counts().astype(np.int64), step)
    few = [r for r in table if step[table.index(r), 1] > 0][:5]
    sess.variants_begin(few)
    assert sess.variants_info() == (len(few), 0, 0) and not sess.variants_counts().any()
    sess.variants_add()
    assert np.array_equal(sess.variants_counts().astype(np.int64), np.array([step[table.index(r)] for r in few]))
    with pytest.raises(simuscop_amd.SimuError, match="out of order"):
        sess.variants_begin(few[::-1])
    assert sess.variants_info()[0] == len(few)                  # a refused table leaves the earlier one
    sess.variants_begin([])
    assert sess.variants_add() == (0, 0) and sess.variants_counts().shape == (0, 2)
    sess.variants_end()
    for call in (sess.variants_add, sess.variants_counts, sess.variants_reset, sess.variants_info, sess.variants_end):
        with pytest.raises(simuscop_amd.SimuError, match="sg_variants_begin first"):
            call()


def test_tumor_mixture_into_one_state(tmp_path):
    wd = str(tmp_path)
    cfg = cases.build_case("tumor_se_mixture", wd)
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=TB.SEED, truth_variants=1) as sess:
        L = VU.read_length(cfg)
        table, want, passes, expanded = run_passes(sess, L, False, [0, 1, 2, 3], lambda p: sess.planned_reads)
        assert passes == 4 and expanded > 400
        indels = want[[i for i, r in enumerate(table) if r[1] != SNV]]        # (clones differ: some reads carry a row, some do not)
        assert indels[:, 1].sum() > 0 and 0 < indels[:, 0].sum() < indels[:, 1].sum()
        sess.variants_reset()
        assert not sess.variants_counts().any()


def test_crowded_rows(tmp_path):
    cfg = VU.crowded_case(str(tmp_path))
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=TB.SEED, truth_variants=1) as sess:
        L = VU.read_length(cfg)
        assert L == 75
        table, want, passes, expanded = run_passes(sess, L, True, [0, 1], lambda p: sess.planned_reads)
        assert passes >= 2 and expanded > 1500
        at = {(r[0], r[1], r[2] + 1, r[3], chr(r[4]) if r[1] == SNV else 0): tuple(want[i]) for i, r in enumerate(table)}
        LN = VU.CROWDED_LEN[0]
        met = lambda key: at[key][1] > 0
        # the rows the case is about exist and are met by reads
        for key in ((0, DEL, 1000, 5, 0), (0, DEL, 2000, 10, 0), (0, INS, 3000, 5, 0), (0, INS, 3500, 3, 0), (0, INS, 3501, 2, 0),
                    (0, DEL, 6001, 4, 0), (0, INS, 6200, 3, 0), (0, DEL, 6300, 6, 0), (0, DEL, 9020, 2, 0), (0, INS, 9025, 1, 0),
                    (0, DEL, 14000, 3, 0), (0, DEL, 14000, 7, 0), (0, INS, 15000, 2, 0), (0, INS, 15000, 3, 0)):
            assert met(key), key
        assert (1, DEL, 100, 3, 0) in at and (1, INS, 200, 2, 0) in at
        snv_at = lambda c, pos: [k for k in at if k[:3] == (c, SNV, pos)]
        for c, pos in ((0, 999), (0, 1005), (0, 2004), (0, 3000), (0, 6100), (0, 9010), (0, 13000)):
            assert snv_at(c, pos) and all(met(k) for k in snv_at(c, pos)), (c, pos)
        for c, pos in ((0, 1), (0, LN), (1, 1), (1, 300)):       # (few templates reach a contig's outermost bases)
            assert snv_at(c, pos), (c, pos)
        assert (0, DEL, LN - 4, 5, 0) in at
        two = snv_at(0, 12000)                                  # one place, an allele per population and the SNP's
        assert len(two) >= 2 and all(0 < at[k][0] < at[k][1] for k in two[:2])
        (fasta_base,) = snv_at(0, 13000)                        # the SNP row whose allele is the FASTA's base: alt is total
        assert at[fasta_base][0] == at[fasta_base][1] > 0
        assert 0 < at[(0, DEL, 1000, 5, 0)][0] < at[(0, DEL, 1000, 5, 0)][1]    # het: some carry it, some do not


def test_calls_before_begin_and_without_a_map_are_refused(tmp_path):
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path))
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=TB.SEED) as sess:     # no truth option: no piece map
        sess.weighted_length()
        sess.set_reads(2000)
        assert sess.prepare_batch(0)
        sess.sample()
        sess.result()
        for call in (sess.variants_add, sess.variants_counts, sess.variants_reset, sess.variants_info, sess.variants_end):
            with pytest.raises(simuscop_amd.SimuError, match="sg_variants_begin first"):
                call()
        with pytest.raises(simuscop_amd.SimuError, match="truth_variants"):
            sess.variant_table()
        sess.variants_begin([(0, SNV, 1000, 0, "A")])
        with pytest.raises(simuscop_amd.SimuError, match="sg_truth_map first"):
            sess.variants_add()
        assert sess.variants_info() == (1, 0, 0) and not sess.variants_counts().any()
        for bad in ([(0, SNV, 5, 1, "A")], [(0, DEL, 5, 0, 0)], [(0, 7, 5, 1, 0)], [(0, SNV, 2 ** 32, 0, "A")]):
            with pytest.raises(simuscop_amd.SimuError, match="sg_variants_begin"):
                sess.variants_begin(bad)
        sess.variants_end()
    eng = simuscop_amd.load_engine()
    n = C.c_uint64()
    assert eng.sg_variants_counts(None, None, 0, C.byref(n)) != 0
