"""`simuReads --truth-depth` on the MI355X: the reads' true coverage as bedGraph (sg_depth.hip).

The model is the truth BAM of the same run: every record's POS and M operations, piled up with numpy.  The bedGraph is
expanded to per-base depths and compared base by base; its rows tile every contig of the @SQ list in order.  Further:
pieces (the same file however the run is cut), bins (the fixed grid, means of the per-base model), additivity (FASTQ and
BAM unchanged), the Session route against the host rule (sg_truth_reads through sg_truth_align), --no-write."""
import os
import re

import numpy as np
import pytest

import simuscop_amd
import test_gpu_truth_bam as TB
import truth_util as U
from profile_shapes import Shape

pytestmark = pytest.mark.gpu

SUFFIX = ".truth.depth.bedgraph"
CASES = ["k3_b53_PE_fast_kernel", "k3_b52_SE_fast_kernel", "k5_b10_PE", "wgs_pe_variants", "wes_pe_targets", "tumor_se_mixture"]


def read_bedgraph(path):
    """[(contig name, start, end, value as written)]; the file has no track line and nothing but four-column rows."""
    text = open(path, "rb").read()
    assert text.endswith(b"\n") and b"\r" not in text and b"track" not in text
    rows = []
    for ln in text[:-1].split(b"\n"):
        name, a, b, v = ln.split(b"\t")
        assert re.fullmatch(rb"\d+", a) and re.fullmatch(rb"\d+", b)
        rows.append((name, int(a), int(b), v))
    return rows


def rows_by_contig(rows, refs):
    """The rows of every contig of `refs`, in the order of `refs`: each contig's rows together, tiling [0, LN)."""
    names = []
    for r in rows:
        if not names or names[-1] != r[0]:
            names.append(r[0])
    assert names == [n for n, ln in refs if ln > 0], "the contigs are not the @SQ lines in order"
    out = {}
    for name, ln in refs:
        mine = [r for r in rows if r[0] == name]
        assert mine[0][1] == 0 and mine[-1][2] == ln
        assert all(a[2] == b[1] for a, b in zip(mine, mine[1:])) and all(r[1] < r[2] for r in mine)
        out[name] = mine
    return out


def depth_of_records(recs, refs):
    """Per contig the depth the records' M operations give (D, N, I, S and unmapped records add nothing)."""
    diff = [np.zeros(ln + 1, dtype=np.int64) for _, ln in refs]
    m_total = 0
    for rec in recs:
        p = rec["pos"]
        for n, o in rec["ops"]:
            if o == 0:
                diff[rec["rid"]][p] += 1
                diff[rec["rid"]][p + n] -= 1
                m_total += n
            if o in (0, 2, 3):
                p += n
    return [np.cumsum(d)[:-1] for d in diff], m_total


def expand_runs(mine, ln):
    d = np.zeros(ln, dtype=np.int64)
    for _, a, b, v in mine:
        assert re.fullmatch(rb"\d+", v), v
        d[a:b] = int(v)
    return d


def _run_case(name, wd):
    """One `--truth-bam --truth-depth 1` run of the case; per stem (refs, records, bedGraph rows), and the stats line."""
    cfg = TB.RUNS[name](wd)
    out = os.path.join(wd, "depth_out")
    err = TB.simu(cfg, out, "--truth-bam", "--truth-depth", "1").stderr
    per_stem = {}
    for stem in TB.stems(out):
        _, refs, recs, _ = U.read_truth_bam(os.path.join(out, stem + ".truth.bam"))
        per_stem[stem] = (refs, recs, read_bedgraph(os.path.join(out, stem + SUFFIX)))
    assert sorted(x[:-len(SUFFIX)] for x in os.listdir(out) if x.endswith(SUFFIX)) == sorted(per_stem)
    return cfg, out, err, per_stem


@pytest.fixture(scope="module")
def run_case(tmp_path_factory):
    done = {}   # every case runs once for the whole file

    def run(name):
        if name not in done:
            done[name] = _run_case(name, str(tmp_path_factory.mktemp(name)))
        return done[name]
    return run


@pytest.mark.parametrize("name", CASES)
def test_bedgraph_equals_the_pile_up_of_the_truth_bam(name, run_case):
    _, _, err, per_stem = run_case(name)
    assert per_stem
    m_all = lines = 0
    piles = []
    for stem, (refs, recs, rows) in per_stem.items():
        want, m_total = depth_of_records(recs, refs)
        by = rows_by_contig(rows, refs)
        for (cname, ln), w in zip(refs, want):
            mine = by[cname]
            assert all(a[3] != b[3] for a, b in zip(mine, mine[1:])), (stem, cname, "two equal rows in a row")
            got = expand_runs(mine, ln)
            bad = np.flatnonzero(got != w)
            assert not len(bad), (stem, cname, len(bad), int(bad[0]), int(got[bad[0]]), int(w[bad[0]]))
        # (nearly every base of a mapped read is an M base: I and S take a few, D and N are no read bases)
        read_bases = sum(len(rec["seq"]) for rec in recs if rec["ops"])
        assert read_bases // 2 < m_total <= read_bases and len(recs) > 1000
        m_all += m_total
        lines += len(rows)
        piles.append(np.concatenate(want))
    assert TB.stat(err, "depth_bases") == m_all and TB.stat(err, "depth_rows") == lines
    assert float(re.search(r"depth_s=([0-9.]+)", err).group(1)) >= 0
    if len(piles) > 1:   # the reset between stems: no stem's file is another's, or the sum of those before it
        assert not np.array_equal(piles[0], piles[1]) and not np.array_equal(piles[0] + piles[1], piles[1])


def test_the_suite_meets_every_shape(run_case):
    """Nothing above is vacuous: among the compared records are deletions, insertions, skips across targets and reverse
    reads, and one stem holds more than one population."""
    seen = set()
    for name in CASES:
        _, _, _, per_stem = run_case(name)
        for stem, (refs, recs, rows) in per_stem.items():
            # a mixture's stem is name_proportion+name_proportion...: more than one population has a share
            if sum(float(part.rsplit("_", 1)[1]) > 0 for part in stem.split("+") if "+" in stem) > 1:
                seen.add("mixture")
            for rec in recs:
                if rec["ops"]:
                    seen |= {"IDN"[o - 1] for _, o in rec["ops"] if o in (1, 2, 3)}
                    if rec["flag"] & 0x10:
                        seen.add("reverse")
            if any(r[3] == b"0" and r[2] - r[1] > 1000 for r in rows):
                seen.add("long zero row")
    assert seen >= {"D", "I", "N", "reverse", "mixture", "long zero row"}, seen


def test_pieces_give_the_same_file(run_case, tmp_path):
    cfg, out, err, per_stem = run_case("wgs_pe_variants")
    (stem,) = per_stem
    cut = str(tmp_path / "cut")
    r1 = TB.simu(cfg, str(tmp_path / "whole"), "--truth-depth", "1", env={"SIMU_TRACE_PIECES": "1"})
    r = TB.simu(cfg, cut, "--truth-depth", "1", env={"SIMU_PIECE_SLOTS": "1", "SIMU_TRACE_PIECES": "1"})
    n_whole, n_cut = r1.stderr.count("[piece]"), r.stderr.count("[piece]")
    assert n_cut >= 4 and n_cut > n_whole >= 1, (n_whole, n_cut)
    want = open(os.path.join(out, stem + SUFFIX), "rb").read()
    assert open(os.path.join(cut, stem + SUFFIX), "rb").read() == want
    assert open(os.path.join(str(tmp_path / "whole"), stem + SUFFIX), "rb").read() == want
    assert TB.stat(r.stderr, "depth_bases") == TB.stat(err, "depth_bases") and TB.stat(r.stderr, "depth_rows") == TB.stat(err, "depth_rows")


def test_reads_with_more_runs_than_the_stage_holds(run_case, tmp_path):
    """depth_add_kernel stages a read's M runs until the walk has told where they start; a read with more runs than the
    stage holds walks a second time.  With a stage of one run (SG_DEPTH_STAGE) every read with a D, an N or an I inside
    takes that path, with a stage of none every read: the file is the same."""
    cfg, out, err, per_stem = run_case("wgs_pe_variants")
    (stem,) = per_stem
    assert sum(1 for rec in per_stem[stem][1] if sum(o == 0 for _, o in rec["ops"]) > 1) > 100
    want = open(os.path.join(out, stem + SUFFIX), "rb").read()
    for stage in ("1", "0"):
        d = str(tmp_path / ("stage" + stage))
        r = TB.simu(cfg, d, "--truth-depth", "1", env={"SG_DEPTH_STAGE": stage})
        assert open(os.path.join(d, stem + SUFFIX), "rb").read() == want
        assert TB.stat(r.stderr, "depth_bases") == TB.stat(err, "depth_bases")


def test_bins_are_means_on_the_fixed_grid(tmp_path):
    wd = str(tmp_path)
    prof = U.write_identity_profile(os.path.join(wd, "identity.profile"), Shape(3, 53))
    cfg, _, _ = U.acgt_case(wd, prof, "PE")                      # 90,000 + 25,000 bases: 777 divides neither
    for bin_width in (777, 1000000):
        out = os.path.join(wd, "out%d" % bin_width)
        err = TB.simu(cfg, out, "--truth-bam", "--truth-depth", str(bin_width)).stderr
        (stem,) = TB.stems(out)
        _, refs, recs, _ = U.read_truth_bam(os.path.join(out, stem + ".truth.bam"))
        want, m_total = depth_of_records(recs, refs)
        rows = read_bedgraph(os.path.join(out, stem + SUFFIX))
        by = rows_by_contig(rows, refs)
        for (cname, ln), w in zip(refs, want):
            mine = by[cname]
            assert len(mine) == -(-ln // bin_width) and mine[-1][2] == ln
            for k, (_, a, b, v) in enumerate(mine):
                assert (a, b) == (k * bin_width, min(ln, (k + 1) * bin_width))
                assert v == ("%.4f" % (int(w[a:b].sum()) / (b - a))).encode(), (cname, k, v)
            assert any(r[3] != mine[0][3] for r in mine) or len(mine) == 1
        if bin_width == 1000000:
            assert len(rows) == len(refs) == 2
        assert TB.stat(err, "depth_rows") == len(rows) and TB.stat(err, "depth_bases") == m_total > 0


def test_the_option_only_adds(run_case, tmp_path):
    cfg, out, err, per_stem = run_case("k3_b53_PE_fast_kernel")
    plain = str(tmp_path / "plain")
    perr = TB.simu(cfg, plain, "--truth-bam").stderr
    files = sorted(os.listdir(plain))
    assert files and files == sorted(x for x in os.listdir(out) if not x.endswith(SUFFIX))
    assert any(x.endswith(".truth.bam") for x in files) and any(x.endswith(".fq") for x in files)
    for f in files:
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(out, f), "rb").read(), f
    assert not [x for x in files if "bedgraph" in x]
    assert TB.stat(perr, "depth_bases") == 0 and TB.stat(perr, "depth_rows") == 0 and re.search(r"depth_s=0\.000\b", perr)
    assert TB.stat(err, "depth_bases") > 0


def test_no_write_counts_and_writes_nothing(run_case, tmp_path):
    cfg, _, err, _ = run_case("k3_b53_PE_fast_kernel")
    out = str(tmp_path / "nowrite")
    r = TB.simu(cfg, out, "--no-write", "--truth-depth", "1")
    assert TB.stat(r.stderr, "depth_bases") == TB.stat(err, "depth_bases") > 0
    assert TB.stat(r.stderr, "depth_rows") == TB.stat(err, "depth_rows") > 0
    assert not os.path.exists(out) or not os.listdir(out)


def test_session_route_follows_the_host_rule(tmp_path):
    """prepare_batch / sample / depth_add() per chromosome; the model is sg_truth_reads through sg_truth_align, the host's
    statement of the rule: independent of the record kernels.  A second depth_add() of the same pass adds it again."""
    wd = str(tmp_path)
    cfg = TB.RUNS["k3_b53_PE_fast_kernel"](wd)
    text = open(cfg).read()
    refs = U.fasta_contigs(re.search(r"^ref = (\S+)", text, re.M).group(1))
    L = int(re.search(r"readLength: (\d+)", open(re.search(r"profile = (\S+)", text).group(1)).read()).group(1))
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=TB.SEED, truth_depth=1) as sess:
        sess.weighted_length()
        sess.set_reads(sess.planned_reads)
        have = [np.zeros(ln, dtype=np.int64) for _, ln in refs]
        reads = m_sum = 0
        for chrom in range(sess.n_chromosomes):
            if not sess.prepare_batch(chrom):
                continue
            sess.sample()
            sess.result()
            n = sess.batch_slots
            diff = [np.zeros(ln + 1, dtype=np.int64) for _, ln in refs]
            pieces, m_pass = {}, 0
            for m in range(2):
                rows = sess.truth_reads(m, 0, n)
                for t in range(n):
                    r = rows[t]
                    if not r.live or not r.inside:
                        continue
                    if r.chain not in pieces:
                        pieces[r.chain] = sess.truth_pieces(r.chain)
                    contig, pos, ops = simuscop_amd.truth_align(pieces[r.chain], r.tmpl_off, L, bool(r.reverse), [r.events[e] for e in range(r.n_events)])
                    for k, o in ops:
                        if o == 0:
                            diff[contig][pos] += 1
                            diff[contig][pos + k] -= 1
                            m_pass += k
                        if o in (0, 2, 3):
                            pos += k
                    reads += 1
            step = [np.cumsum(d)[:-1] for d in diff]
            for times in (1, 2):
                assert sess.depth_add() == m_pass
                for c, (_, ln) in enumerate(refs):
                    have[c] = have[c] + step[c]
                    assert np.array_equal(sess.depth_fetch(c, 0, ln), have[c].astype(np.uint32)), (chrom, times, c)
            m_sum += 2 * m_pass
        assert reads > 1000 and sess.depth_info() == (len(refs), m_sum, sess.depth_info()[2])
        sess.depth_reset()
        assert not any(sess.depth_fetch(c, 0, ln).any() for c, (_, ln) in enumerate(refs))
