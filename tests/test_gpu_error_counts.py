"""True error counts on the MI355X through a Session (sg_errors.hip): after every sampling pass the device's table
equals, cell by cell and exactly, the model (tests/errors_model.py) applied to every read of the pass -- templates and
events from sg_truth_reads, the chains' codes from sg_haplotype_codes, the text from sg_fetch.  The cases are the suite's
small ones, each chosen for a boundary of the kernel (lane = cycle in chunks of 64, a workgroup's slab of win_cycles
cycles, waves that take 64 slots at a time); then passes of a few reads, add twice / reset / begin again / end, and the
passes that are refused."""
import os

import numpy as np
import pytest

import cases
import errors_model as EM
import errors_util as EU
import simuscop_amd
import test_gpu_truth_bam as TB
from simuscop_amd import synth

pytestmark = pytest.mark.gpu

MAX_READS = 4000   # per population: the model is Python


def _derived(read_length):
    def make(wd):
        fa = os.path.join(wd, "ref.fa")
        synth.write_fasta(fa, [("chr3", 60000)], seed=61)
        prof = os.path.join(wd, "derived.profile")
        cases.derive_profile("xten", prof, read_length=read_length, indel_scale=4.0)
        cfg = os.path.join(wd, "config.txt")
        cases._config(cfg, ref=fa, profile=prof, name="d", output=os.path.join(wd, "out"), layout="PE", threads=1, verbose=0, coverage=6,
                      insertSize=350)
        return cfg
    return make


# name -> (config maker, paired, populations)
CASES = {
    "short_reads_se": (lambda wd: cases.build_case("short_reads_se", wd), False, 1),                    # L = 52: one partial chunk
    "wgs_se_hs2000": (lambda wd: cases.build_case("wgs_se_hs2000", wd), False, 1),                      # L = 75
    "wgs_pe_xten": (lambda wd: cases.build_case("wgs_pe_xten", wd), True, 1),                           # L = 151, two mates
    "long_reads_pe": (lambda wd: cases.build_case("long_reads_pe", wd), True, 1),                       # L = 600: ten chunks, windows
    "indel_storm_se": (lambda wd: cases.build_case("indel_storm_se", wd), False, 1),                    # ~4.6 events a read
    "indel_rich_n_islands_pe": (lambda wd: cases.build_case("indel_rich_n_islands_pe", wd), True, 1),   # `other`; two contigs
    "wgs_pe_variants": (lambda wd: cases.build_case("wgs_pe_variants", wd), True, 1),                   # template = haplotype
    "tumor_se_mixture": (lambda wd: cases.build_case("tumor_se_mixture", wd), False, 4),                # four populations, one state
    "derived_L64": (_derived(64), True, 1),
    "derived_L65": (_derived(65), True, 1),
    "derived_L128": (_derived(128), True, 1),
}


def run_passes(sess, paired, popus, max_reads=MAX_READS):
    """Every (population, chromosome) pass into one state; the device's table against the model's after each."""
    want = None
    passes = counted = 0
    for p in range(popus):
        sess.weighted_length(p)
        sess.set_reads(min(sess.planned_reads, max_reads), p)
        for chrom in range(sess.n_chromosomes):
            if not sess.prepare_batch(chrom, p):
                continue
            info = sess.errors_info()
            if want is None:                                          # (the driver began the table with the profile's sizes)
                want = EM.Table(info.cycles, info.qual_lo, info.n_qual, info.tmpl_len)
                assert info.cells == want.cells and (info.bases, info.errors, info.skipped, info.reads) == (0, 0, 0, 0)
                assert info.win_cycles % 64 == 0 and 64 <= info.win_cycles and info.lds_bytes <= 72 * 1024
            sess.sample()
            sess.result()
            before = (int(want.Q[..., EM.BASES].sum()), int(want.Q[..., EM.ERRORS].sum()))
            n, _ = EU.model_of_pass(sess, want, paired)
            bases, errors = sess.errors_add()
            EU.assert_tables_equal(sess.errors_counts(), want, (p, chrom))
            assert (bases, errors) == (int(want.Q[..., EM.BASES].sum()) - before[0], int(want.Q[..., EM.ERRORS].sum()) - before[1])
            passes += 1
            counted += n
    info = sess.errors_info()
    assert (info.bases, info.errors, info.skipped, info.reads) == (int(want.Q[..., EM.BASES].sum()), int(want.Q[..., EM.ERRORS].sum()),
                                                                   want.skipped, counted)
    return want, passes, counted


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    done = {}   # every case runs once for the whole file

    def run(name):
        if name not in done:
            make, paired, popus = CASES[name]
            cfg = make(str(tmp_path_factory.mktemp(name)))
            with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=TB.SEED, truth_bam=1, truth_errors=1) as sess:
                done[name] = run_passes(sess, paired, popus)
        return done[name]
    return run


@pytest.mark.parametrize("name", sorted(CASES))
def test_table_equals_the_model(name, tables):
    want, passes, counted = tables(name)
    paired = CASES[name][1]
    assert passes >= CASES[name][2] and counted > 500
    assert want.Q[0, :, :, EM.BASES].sum() > 0 and want.Q[..., EM.ERRORS].sum() > 0
    assert bool(want.Q[1].any()) == paired and bool(want.S[1].any()) == paired
    assert want.S[:, :, :4].sum() + want.S[:, :, 4].sum() == want.Q[..., EM.BASES].sum()


def test_the_cases_meet_every_clause(tables):
    """Nothing above is vacuous: reads longer and shorter than L, insertions, deletions, `other`, chunks beyond the first,
    cycles beyond a workgroup's slab, and reads that are longer than the template."""
    storm, _, _ = tables("indel_storm_se")
    assert storm.I[..., 0].sum() > 1000 and storm.D[..., 0].sum() > 1000 and storm.Q[..., EM.INSERTED].sum() > 1000
    assert storm.Q[0, storm.L:, :, EM.BASES].sum() > 0                # read positions behind cycle L: paired bases pushed there
    assert storm.D[0, 0, 0] > 0 and storm.I[0, storm.L - 1, 0] + storm.D[0, storm.L - 1, 0] > 0      # events on the first and last base
    islands, _, _ = tables("indel_rich_n_islands_pe")
    assert islands.Q[..., EM.OTHER].sum() > 0
    long_reads, _, _ = tables("long_reads_pe")
    assert long_reads.L == 600 and long_reads.Q[:, 576:600, :, EM.BASES].sum() > 0
    short, _, _ = tables("short_reads_se")
    assert short.L == 52 and short.Q[0, 51, :, EM.BASES].sum() > 0


@pytest.fixture(scope="module")
def xten(tmp_path_factory):
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path_factory.mktemp("xten")))
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=TB.SEED, truth_bam=1, truth_errors=1) as sess:
        sess.weighted_length()
        yield sess


@pytest.fixture(scope="module")
def hs2000(tmp_path_factory):
    cfg = cases.build_case("wgs_se_hs2000", str(tmp_path_factory.mktemp("hs2000")))
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=TB.SEED, truth_bam=1, truth_errors=1) as sess:
        sess.weighted_length()
        yield sess


def _pass_of(sess, slots, paired):
    """A pass of exactly `slots` fragment slots against the model.  set_reads asks for reads and the planner makes slots
    of them (a window's reads, halved and rounded up for pairs), so the read count that gives the wanted number of slots
    is looked for; a size that no read count gives fails the test."""
    found = None
    for reads in range(max(1, slots - 2), 2 * slots + 8):
        sess.set_reads(reads)
        if sess.prepare_batch(0) and sess.batch_slots == slots:
            found = reads
            break
    assert found is not None, "no set_reads() value gives %d slots" % slots
    assert sess.batch_slots == slots
    sess.sample()
    sess.result()
    info = sess.errors_info()
    sess.errors_reset()
    want = EM.Table(info.cycles, info.qual_lo, info.n_qual, info.tmpl_len)
    n, skipped = EU.model_of_pass(sess, want, paired)
    sess.errors_add()
    EU.assert_tables_equal(sess.errors_counts(), want, slots)
    print("%d slots: set_reads(%d), %d reads counted, %d skipped" % (slots, found, n, skipped))
    assert 0 < n <= (2 if paired else 1) * slots and sess.errors_info().reads == n


@pytest.mark.parametrize("slots", [1, 63, 64, 65, 255, 256, 257])
def test_passes_of_a_few_reads(slots, hs2000):
    """Wave and workgroup boundaries: a wave takes 64 slots of one mate at a time, text_offset addresses the text in
    blocks of 256 reads.  In the SE layout one read is one slot, so every size is reached exactly: 256 is four full
    groups of 64 and one full block."""
    _pass_of(hs2000, slots, False)


@pytest.mark.parametrize("slots", [1, 63, 64, 65, 255, 257])
def test_passes_of_a_few_pairs(slots, xten):
    """The same boundaries with two mates a slot.  (The windows of this case's planner round pairs up one by one: no
    read count gives 256 slots, which the SE passes above cover.)"""
    _pass_of(xten, slots, True)


def test_add_again_reset_begin_again_and_end(xten):
    sess = xten
    sess.set_reads(2000)
    assert sess.prepare_batch(0)
    sess.sample()
    sess.result()
    info = sess.errors_info()
    sess.errors_reset()
    step = EM.Table(info.cycles, info.qual_lo, info.n_qual, info.tmpl_len)
    n, _ = EU.model_of_pass(sess, step, True)
    first = sess.errors_add()
    assert first[0] > 100000 and 0 < first[1] < first[0]
    EU.assert_tables_equal(sess.errors_counts(), step)
    assert sess.errors_add() == first                                # a second add of the same pass adds it again
    assert np.array_equal(sess.errors_counts().astype(np.int64), 2 * step.flat())
    assert sess.errors_info().bases == 2 * first[0] and sess.errors_info().reads == 2 * n
    sess.errors_reset()
    assert not sess.errors_counts().any() and sess.errors_info().bases == 0 and sess.errors_info().reads == 0
    # a table of the caller's: other cycles and another quality range replace the state
    sess.errors_begin(info.cycles + 7, 0, 60)
    again = sess.errors_info()
    assert (again.cycles, again.qual_lo, again.n_qual, again.bases) == (info.cycles + 7, 0, 60, 0) and not sess.errors_counts().any()
    wide = EM.Table(info.cycles + 7, 0, 60, info.tmpl_len)
    EU.model_of_pass(sess, wide, True)
    assert sess.errors_add() == first
    EU.assert_tables_equal(sess.errors_counts(), wide)
    for bad in ((info.tmpl_len - 1, 0, 60), (info.tmpl_len, 0, 0), (info.tmpl_len, 0, 129), (70000, 0, 41), (info.tmpl_len, 200, 41)):
        with pytest.raises(simuscop_amd.SimuError, match="sg_errtab_begin"):
            sess.errors_begin(*bad)
    assert sess.errors_info().cycles == info.cycles + 7              # a refused begin leaves the earlier state
    # a range the pass's qualities do not fit: the call fails, and says why
    sess.errors_begin(info.cycles, 0, 10)
    with pytest.raises(simuscop_amd.SimuError, match="quality"):
        sess.errors_add()
    sess.errors_end()
    for call in (sess.errors_add, sess.errors_counts, sess.errors_reset, sess.errors_info, sess.errors_end):
        with pytest.raises(simuscop_amd.SimuError, match="sg_errtab_begin first"):
            call()
    sess.errors_begin(info.cycles, info.qual_lo, info.n_qual)        # (the fixture's other tests go on with the driver's sizes)


def test_a_pass_under_sg_diag_is_refused(xten, monkeypatch):
    sess = xten
    sess.set_reads(500)
    assert sess.prepare_batch(0)
    monkeypatch.setenv("SG_DIAG", "4")                               # (the ablation that leaves the names unwritten)
    sess.sample()
    sess.result()
    sess.errors_reset()
    with pytest.raises(simuscop_amd.SimuError, match="SG_DIAG"):
        sess.errors_add()
    assert not sess.errors_counts().any()
    monkeypatch.delenv("SG_DIAG")
    sess.sample()
    sess.result()
    assert sess.errors_add()[0] > 0


def test_no_piece_map_is_needed_and_calls_before_begin_are_refused(tmp_path):
    cfg = cases.build_case("wgs_se_hs2000", str(tmp_path))
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=TB.SEED, host_haplotypes=1) as sess:     # uploaded chains: no map
        sess.weighted_length()
        sess.set_reads(3000)
        assert sess.prepare_batch(0)
        for call in (sess.errors_add, sess.errors_counts, sess.errors_reset, sess.errors_info, sess.errors_end):
            with pytest.raises(simuscop_amd.SimuError, match="sg_errtab_begin first"):
                call()
        sess.errors_begin(75 + 32 * 4, 0, 45)
        with pytest.raises(simuscop_amd.SimuError, match="sg_result first"):
            sess.errors_add()
        sess.sample()
        b1, _, nf = sess.result()
        bases, errors = sess.errors_add()
        flat = sess.errors_counts().astype(np.int64)
        t = EM.Table.of_flat(flat, 75 + 32 * 4, 0, 45, 75)
        info = sess.errors_info()
        # every base of every counted read is in exactly one column
        text = sess.fetch(b1, 0)[0].split(b"\n")
        read_bases = sum(len(text[i]) for i in range(1, len(text) - 1, 4))
        n_all = int(t.Q.sum() - t.Q[..., EM.ERRORS].sum())          # (an error is one of the bases)
        assert info.reads + info.skipped == nf and n_all <= read_bases and (info.skipped > 0 or n_all == read_bases)
        assert t.Q[..., EM.BASES].sum() == bases == t.S.sum() and t.Q[..., EM.ERRORS].sum() == errors > 0 and not t.Q[1].any()
