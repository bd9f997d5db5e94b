"""`simuReads --truth-variants` on the MI355X, through the command line: the file's rows against the table the input
files give (read here, not by the simulator), one file per stem, the same file however the run is cut into pieces, FASTQ /
truth BAM / bedGraph unchanged by the option, --no-write, and what the counts mean, bounded by the pile-up of the same
run's truth BAM and met exactly by the records of reads without sequencing events."""
import bisect
import os
import re

import numpy as np
import pytest

import cases
import simuscop_amd
import test_gpu_truth_bam as TB
import test_truth_variants_cpu as TV
import truth_util as U
import variant_util as VU
from profile_shapes import Shape
from variant_model import DEL, INS, SNV

pytestmark = pytest.mark.gpu

SUFFIX = VU.SUFFIX


def expected_file(cfg, refs):
    """(text with zero counts, rows, dropped) of the table the config's input files give, under the BAM's @SQ names."""
    rows, popus = VU.input_rows(cfg)
    contigs = [(n.decode(), ln) for n, ln in refs]
    by_key = {}
    for n, _ in contigs:
        by_key.setdefault(VU.abbr(n), n)
    rows = [(k, by_key.get(c, "?" + c), p, q, t) for k, c, p, q, t in rows]
    return TV.model_file(contigs, popus, rows), popus


def descr(rows):
    return [(r[0], r[1], r[2], r[3], r[6]) for r in rows]


def descr_of_text(text):
    return [tuple(f[i] if i != 1 else int(f[i]) for i in (0, 1, 2, 3, 6)) for f in (ln.split("\t") for ln in text.decode().splitlines()[1:])]


@pytest.fixture(scope="module")
def run_case(tmp_path_factory):
    done = {}

    def run(name):
        if name not in done:
            wd = str(tmp_path_factory.mktemp(name))
            cfg = TB.RUNS[name](wd)
            out = os.path.join(wd, "variants_out")
            err = TB.simu(cfg, out, "--truth-bam", "--truth-depth", "1", "--truth-variants").stderr
            done[name] = (cfg, out, err)
        return done[name]
    return run


def test_file_rows_are_the_input_files_rows(run_case):
    cfg, out, err = run_case("wgs_pe_variants")
    (stem,) = TB.stems(out)
    _, refs, recs, _ = U.read_truth_bam(os.path.join(out, stem + ".truth.bam"))
    (text, n_rows, dropped), popus = expected_file(cfg, refs)
    rows = VU.read_file(os.path.join(out, stem + SUFFIX))
    assert descr(rows) == descr_of_text(text) and len(rows) == n_rows > 1000
    assert {r[0].encode() for r in rows} <= {n for n, _ in refs}
    ids = {n.decode(): i for i, (n, _) in enumerate(refs)}
    order = [(ids[r[0]], r[1], {"s": 0, "p": 0, "i": 1, "d": 2}[r[2]]) for r in rows]
    assert order == sorted(order)
    assert {r[2] for r in rows} == set("spid") and all(r[6] == "." for r in rows if r[2] == "p") and all(r[6] == "test" for r in rows if r[2] != "p")
    assert all(r[4] <= r[5] for r in rows) and any(r[5] == 0 for r in rows) and any(0 < r[4] < r[5] for r in rows)
    assert TB.stat(err, "variant_rows") == n_rows and TB.stat(err, "variant_dropped") == dropped
    assert TB.stat(err, "variant_hits") == sum(r[5] for r in rows) > 1000
    assert float(re.search(r"variants_s=([0-9.]+)", err).group(1)) >= 0


def test_the_option_only_adds(run_case, tmp_path):
    cfg, out, err = run_case("wgs_pe_variants")
    plain = str(tmp_path / "plain")
    perr = TB.simu(cfg, plain, "--truth-bam", "--truth-depth", "1").stderr
    files = sorted(os.listdir(plain))
    assert files and files == sorted(x for x in os.listdir(out) if not x.endswith(SUFFIX))
    assert any(x.endswith(".truth.bam") for x in files) and any(x.endswith(".fq") for x in files) and any(x.endswith(".bedgraph") for x in files)
    for f in files:
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(out, f), "rb").read(), f
    assert TB.stat(perr, "variant_rows") == 0 and TB.stat(perr, "variant_hits") == 0 and re.search(r"variants_s=0\.000\b", perr)


def test_one_file_per_stem(run_case):
    cfg, out, err = run_case("tumor_se_mixture")
    stems = TB.stems(out)
    assert len(stems) == 2 and sorted(x[:-len(SUFFIX)] for x in os.listdir(out) if x.endswith(SUFFIX)) == stems
    first = next(s for s in stems if s.startswith("clone1_1.000"))
    (second,) = [s for s in stems if s != first]
    a, b = VU.read_file(os.path.join(out, first + SUFFIX)), VU.read_file(os.path.join(out, second + SUFFIX))
    assert descr(a) == descr(b)                                              # one table, every row in every file
    others = [i for i, r in enumerate(a) if r[2] != "p" and "clone1" not in r[6].split(",")]
    only1 = [i for i, r in enumerate(a) if r[6] == "clone1"]
    assert only1 and {a[i][2] for i in only1} == set("sid")
    assert all(a[i][4] == 0 for i in others)                                 # only clone1's reads: no other clone's allele
    # rows that clone1 alone lists: its reads are all of the first stem and 30 % of the second
    alt1, tot1 = sum(a[i][4] for i in only1), sum(a[i][5] for i in only1)
    alt2, tot2 = sum(b[i][4] for i in only1), sum(b[i][5] for i in only1)
    assert 0 < alt1 <= tot1 and alt2 < tot2 and alt1 * tot2 > alt2 * tot1
    assert TB.stat(err, "variant_hits") == sum(r[5] for r in a) + sum(r[5] for r in b)
    # the reset between the stems: the second file is not the first, nor the first plus something everywhere
    assert [r[5] for r in a] != [r[5] for r in b] and any(y[5] < x[5] for x, y in zip(a, b))


def test_pieces_give_the_same_file(run_case, tmp_path):
    cfg, out, err = run_case("wgs_pe_variants")
    (stem,) = TB.stems(out)
    cut = str(tmp_path / "cut")
    r = TB.simu(cfg, cut, "--truth-variants", env={"SIMU_PIECE_SLOTS": "1", "SIMU_TRACE_PIECES": "1"})
    assert r.stderr.count("[piece]") >= 4
    assert open(os.path.join(cut, stem + SUFFIX), "rb").read() == open(os.path.join(out, stem + SUFFIX), "rb").read()
    assert TB.stat(r.stderr, "variant_hits") == TB.stat(err, "variant_hits")


def test_no_write_counts_and_writes_nothing(run_case, tmp_path):
    cfg, _, err = run_case("wgs_pe_variants")
    out = str(tmp_path / "nowrite")
    r = TB.simu(cfg, out, "--no-write", "--truth-variants")
    assert TB.stat(r.stderr, "variant_hits") == TB.stat(err, "variant_hits") > 0
    assert TB.stat(r.stderr, "variant_rows") == TB.stat(err, "variant_rows") > 0
    assert not os.path.exists(out) or not os.listdir(out)


# ---- what the counts mean ----
def record_hits(rec, keys, table):
    """[(row, is_alt)] the record itself shows: its CIGAR and bases against the rows (a read without sequencing events,
    sampled without substitutions: every I is a variant's literal, every D a joint's gap)."""
    hits = []
    if not rec["ops"]:
        return hits
    rid, ops = rec["rid"], rec["ops"]
    p, q = rec["pos"], 0
    for j, (n, o) in enumerate(ops):
        if o == 0:
            lo = bisect.bisect_left(keys, (rid << 32) | p)
            hi = bisect.bisect_right(keys, (rid << 32) | (p + n))
            nxt, after = (ops[j + 1] if j + 1 < len(ops) else None), (ops[j + 2] if j + 2 < len(ops) else None)
            for r in range(lo, hi):
                _, kind, x, k, allele = table[r]
                if kind == SNV:
                    if x < p + n:
                        hits.append((r, rec["seq"][q + x - p] == allele))
                elif kind == INS:
                    if x + 1 < p + n:
                        hits.append((r, False))
                    elif x == p + n - 1 and nxt and nxt[1] == 1 and nxt[0] == k and after:
                        hits.append((r, True))
                else:
                    if p < x < p + n:
                        hits.append((r, False))
                    elif x == p + n and x > 0 and nxt and nxt[1] == 2 and nxt[0] == k and after and after[1] == 0:
                        hits.append((r, True))
            p += n
            q += n
        elif o in (1, 4):
            q += n
        elif o in (2, 3):
            p += n
    return hits


def test_counts_against_the_truth_bam(tmp_path):
    wd = str(tmp_path)
    prof = U.write_identity_profile(os.path.join(wd, "identity.profile"), Shape(3, 53))
    cfg, fa, seqs = U.acgt_case(wd, prof, "PE", variants=True)
    vfile = os.path.join(wd, "variations.txt")
    kept = [ln for ln in open(vfile).read().splitlines() if not ln.startswith("c\t")]   # no CNV: no joint goes backwards
    cases._write(vfile, kept)
    assert {ln[0] for ln in kept} == set("sid")
    out = os.path.join(wd, "out")
    TB.simu(cfg, out, "--truth-bam", "--truth-variants")
    (stem,) = TB.stems(out)
    _, refs, recs, _ = U.read_truth_bam(os.path.join(out, stem + ".truth.bam"))
    rows = VU.read_file(os.path.join(out, stem + SUFFIX))
    ids = {n.decode(): i for i, (n, _) in enumerate(refs)}
    ins_seq = {(ids[r[0]], r[1] - 1, len(r[3])): r[3].upper().encode() for r in rows if r[2] == "i"}
    table = [(ids[r[0]], {"s": SNV, "p": SNV, "i": INS, "d": DEL}[r[2]], r[1] - 1, len(r[3]) if r[2] == "i" else int(r[3]) if r[2] == "d" else 0,
              ord(r[3]) if r[2] in "sp" else 0) for r in rows]
    assert table == sorted(table, key=lambda r: (r[0], r[2], r[1], r[4], r[3]))
    keys = [(r[0] << 32) | r[2] for r in table]
    pile = np.zeros((len(table), 2), dtype=np.int64)           # (alt, total) the records' M bases, I and D operations show
    busy = np.zeros(len(table), dtype=np.int64)                # records over [p - 1, p + 1] that carry an I, a D or an S
    for rec in recs:
        if not rec["ops"]:
            continue
        rid, a = rec["rid"], rec["pos"]
        b = a + U.ref_span(rec["ops"])
        if any(o in (1, 2, 4) for _, o in rec["ops"]):
            lo = bisect.bisect_left(keys, (rid << 32) | max(a - 1, 0))
            hi = bisect.bisect_right(keys, (rid << 32) | b)    # p - 1 <= b - 1
            busy[lo:hi] += 1
        for r, alt in record_hits(rec, keys, table):
            if alt and table[r][1] == INS:                     # the inserted bases are the row's sequence
                q = sum(n for n, o in rec["ops"][:[j for j, (n, o) in enumerate(rec["ops"]) if o == 1 and n == table[r][3]][0]] if o in (0, 1, 4))
                alt = rec["seq"][q:q + table[r][3]] == ins_seq[(table[r][0], table[r][2], table[r][3])]
            pile[r, 1] += 1
            pile[r, 0] += 1 if alt else 0
    got = np.array([(r[4], r[5]) for r in rows], dtype=np.int64)
    assert (pile[:, 0] <= got[:, 0]).all(), [rows[i] for i in np.flatnonzero(pile[:, 0] > got[:, 0])][:3]
    assert (pile[:, 1] <= got[:, 1]).all(), [rows[i] for i in np.flatnonzero(pile[:, 1] > got[:, 1])][:3]
    short = got[:, 1] - pile[:, 1]
    assert (short <= busy).all(), [(rows[i], int(short[i]), int(busy[i])) for i in np.flatnonzero(short > busy)][:3]
    for kind in (SNV, INS, DEL):                               # the bounds bite: most counts are the pile-up's own
        sel = np.array([r[1] == kind for r in table])
        assert pile[sel, 1].sum() > 0 and pile[sel, 0].sum() > 0 and pile[sel, 1].sum() * 10 >= got[sel, 1].sum() * 8, kind

    # reads without sequencing events, through a Session: what the rule counts is exactly what the record shows
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=TB.SEED, truth_bam=1, truth_variants=1) as sess:
        L = VU.read_length(cfg)
        stable = sess.variant_table()
        assert stable == table
        tab = simuscop_amd._variant_rows(stable)
        sess.weighted_length()
        sess.set_reads(sess.planned_reads)
        checked = with_hits = 0
        for chrom in range(sess.n_chromosomes):
            if not sess.prepare_batch(chrom):
                continue
            sess.sample()
            sess.result()
            rb, _ = sess.truth_bam()
            srecs = U.records_of_stream(sess.fetch_truth(False, rb))
            n = sess.batch_slots
            reads = [np.frombuffer(sess.truth_reads(m, 0, n), dtype=VU.READ_DT, count=n) for m in range(2)]
            live = [(t, m) for t in range(n) for m in range(2) if reads[m][t]["live"]]
            assert len(live) == len(srecs)
            chains = {}
            for (t, m), rec in zip(live, srecs):
                r = reads[m][t]
                if not r["inside"] or r["n_events"]:
                    continue
                ch, off = int(r["chain"]), int(r["tmpl_off"])
                if ch not in chains:
                    pieces = sess.truth_pieces(ch)
                    arr = (simuscop_amd.SgTruthPiece * len(pieces))(*[simuscop_amd.SgTruthPiece(*p) for p in pieces])
                    chains[ch] = (arr, sess.haplotype_codes(ch, 0, pieces[-1][0] + pieces[-1][2]))
                arr, codes = chains[ch]
                got_hits = simuscop_amd.variant_observe(arr, np.ascontiguousarray(codes[off:off + L]), off, L, tab)
                want_hits = record_hits(rec, keys, table)
                assert sorted(got_hits) == sorted(want_hits), (rec["name"], rec["pos"], rec["ops"], got_hits, want_hits)
                checked += 1
                with_hits += 1 if got_hits else 0
        assert checked > 2000 and with_hits > 300
