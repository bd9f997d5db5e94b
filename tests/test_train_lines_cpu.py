"""The generators of tests/train_lines.py on the restatement alone (oracle/train_oracle.cpp, no GPU): every one produces what
it is for -- the line numbers on the scan's edges, which reads are counted, turned away or open a window there, totals
that change when the line on the edge is removed or doubled, a cap that lands on the stated line, and the hand-written
numbers of the clause cases.  No generator is random: each condition holds or this file fails, not silently
tests/test_gpu_train_kernels.py."""
import os
import re

import numpy as np
import pytest

import train_lines as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPENS, COUNTED, TURNED_AWAY, OPENS_UNCOUNTED = (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1)


def _differs(a, b):
    return any(not np.array_equal(a.a[k], b.a[k]) for k in TL.ARRAYS) or any(a.scalar(k) != b.scalar(k) for k in TL.SCALARS) or a.pairs() != b.pairs()


def test_the_edges_are_the_kernels_own():
    src = open(os.path.join(ROOT, "simuscop_amd", "csrc", "sg_train.hip")).read()
    m = re.search(r"kScanThreads = (\d+), kScanItems = (\d+), kScanTile = kScanThreads \* kScanItems", src)
    assert m and int(m.group(2)) == TL.ITEMS and int(m.group(1)) * int(m.group(2)) == TL.TILE
    assert "b += kScanThreads" in src and TL.ROUND == TL.TILE * int(m.group(1))        # tiles a spine round
    assert "(J.bytes + 63) / 64" in src and TL.LINE_TILE == 131072 and TL.LINE_ROUND == 33554432
    assert TL.where_is(7) == "item 7 = thread 0 (its item 7), tile 0, spine round 0"
    assert TL.where_is(8) == "item 8 = thread 1 (its item 0), tile 0, spine round 0"
    assert TL.where_is(2047) == "item 2047 = thread 255 (its item 7), tile 0, spine round 0"
    assert TL.where_is(2048) == "item 2048 = thread 256 (its item 0), tile 1, spine round 0"
    assert TL.where_is(524287) == "item 524287 = thread 65535 (its item 7), tile 255, spine round 0"
    assert TL.where_is(524288) == "item 524288 = thread 65536 (its item 0), tile 256, spine round 1"


@pytest.mark.parametrize("drop", [0, 5])
@pytest.mark.parametrize("exome", [False, True])
def test_every_verdict_is_reached_on_every_edge_of_the_scan(exome, drop, oracle_lib, tmp_path):
    """Over the six variants of scan_lines the gated read on items 7 / 8 / 9, 15 / 16 / 17, 63 / 64 / 65 and 2,047 / 2,048 / 2,049
    opens a window, is counted in the open one and is turned away; with targets a read between two of them opens a window
    without being counted at every edge.  With dropped lines interleaved the gated-read number is not the line number.
    Removing or doubling the line changes the restatement's totals."""
    contigs, bed = TL.scan_contigs(exome)
    files = TL.write_inputs(str(tmp_path), contigs, (), bed)
    seen = {}
    for variant in range(6):
        lines, aims = TL.scan_lines(2600 if drop else 2060, exome, variant, drop_every=drop)
        by_d = {d: k for k, (_, d) in aims.items()}
        assert (by_d[2048] == 2048) == (drop == 0)
        whole = TL.restate(oracle_lib, TL.text_of(lines), files)
        assert whole.code == 0 and whole.st.lines == len(lines)
        for e in (8, 16, 64, TL.TILE):
            for o in (-1, 0, 1):
                k = by_d[e + o]
                seen.setdefault((e, o), set()).add(TL.what_the_line_does(oracle_lib, lines, k, files))
            k = by_d[e]
            assert _differs(whole, TL.restate(oracle_lib, TL.text_of(lines[:k] + lines[k + 1:]), files)), (variant, e, "removed")
            assert _differs(whole, TL.restate(oracle_lib, TL.text_of(lines[:k + 1] + lines[k:]), files)), (variant, e, "doubled")
    for key, verdicts in sorted(seen.items()):
        assert {OPENS, COUNTED, TURNED_AWAY} <= verdicts, (key, verdicts)
    if exome:
        for e in (8, 16, 64, TL.TILE):
            assert any(OPENS_UNCOUNTED in seen[(e, o)] for o in (-1, 0, 1)), e


ROUND_EDGE = {1: (("open", "contig", "same"), (OPENS, OPENS, COUNTED)),          # a contig run that begins exactly at item 524,288
              3: (("right", "left-1", "right+1"), (COUNTED, TURNED_AWAY, OPENS)),
              5: (("open", "same", "back"), (OPENS, COUNTED, TURNED_AWAY))}       # opened by the round's last item, counted from the next


@pytest.mark.parametrize("variant", [1, 3, 5])
def test_the_spine_rounds_edge_by_line_count(variant, oracle_lib, tmp_path):
    """524,488 lines without dropped ones: what items 524,287 (the first round's last), 524,288 (the second round's first) and
    524,289 do in the three variants the GPU file runs; the 200 items of the second round hold counted reads and more than 70
    openings; reads 8,300 to 12,500 lie in one window of several tiles."""
    contigs, bed = TL.scan_contigs(False)
    files = TL.write_inputs(str(tmp_path), contigs, (), bed)
    lines, aims = TL.scan_lines(TL.ROUND + 200, False, variant)
    events, verdicts = ROUND_EDGE[variant]
    assert len(lines) == 524488 and tuple(aims[TL.ROUND + o] for o in (-1, 0, 1)) == tuple((e, TL.ROUND + o) for e, o in zip(events, (-1, 0, 1)))
    text = TL.text_of(lines)
    ends = TL.line_ends(text)
    t = [TL.restate(oracle_lib, text[:int(ends[n - 1]) + 1], files).st for n in (TL.ROUND - 1, TL.ROUND, TL.ROUND + 1)]
    whole = TL.restate(oracle_lib, text, files).st
    verdict = lambda a, b: (b.gc_windows - a.gc_windows, b.reads_counted - a.reads_counted, b.gc_rejected - a.gc_rejected)   # noqa: E731
    assert tuple(verdict(t[i], t[i + 1]) for i in range(2)) == verdicts[:2]      # (item 524,289's is the aim alone)
    in_round_2 = verdict(t[1], whole)                                              # items 524,288 to 524,487
    assert in_round_2[0] > 70 and in_round_2[1] > 190 and in_round_2[1] + in_round_2[2] == 200
    if variant == 3:
        a, b = TL.restate(oracle_lib, TL.text_of(lines[:8300]), files), TL.restate(oracle_lib, TL.text_of(lines[:12500]), files)
        assert b.st.gc_windows == a.st.gc_windows and b.st.reads_counted == a.st.reads_counted + 4200


def test_exome_reads_reach_the_nested_and_the_swapped_targets():
    """In the 4,200-line exome texts of variants 3, 4 and 5 gated reads lie in the nested target and in both rows that are
    swapped in the file (every variant reaches the swapped rows)."""
    for variant in range(6):
        hit = set()
        for ln in TL.scan_lines(4200, True, variant)[0]:
            f = ln.split(b"\t")
            if f[4] == b"60" and f[2] in (b"chr1", b"chr2", b"chr3"):
                hit.update(name for name, (a, b) in TL.ODD_TARGETS.items() if a <= int(f[3]) - 1 <= b)
        assert hit >= {"row 105", "row 109"} and (variant < 3 or "nested" in hit), (variant, hit)


def test_the_short_contig_shrinks_the_window_at_the_stated_read(oracle_lib, tmp_path):
    contigs, bed = TL.scan_contigs(False)
    files = TL.write_inputs(str(tmp_path), contigs, (), bed)
    lines, aims = TL.scan_lines(2400, False, 0, short_at=TL.TILE)
    assert aims[TL.TILE][0] == "short" and b"chrS" in lines[TL.TILE] and not any(b"chrS" in x for x in lines[:TL.TILE])
    # windows of 1,000 bases before it, of 50 behind it: without that one line the reads behind it open far fewer windows
    a, b = TL.restate(oracle_lib, TL.text_of(lines[:TL.TILE]), files), TL.restate(oracle_lib, TL.text_of(lines), files)
    plain = TL.restate(oracle_lib, TL.text_of(lines[:TL.TILE] + lines[TL.TILE + 1:]), files)
    assert b.st.gc_windows - a.st.gc_windows > 2 * (plain.st.gc_windows - a.st.gc_windows) > 0


@pytest.mark.parametrize("k", [0, 7, 8, 2047, 2048, 2059])
def test_a_cap_lands_on_the_stated_line(k, oracle_lib, tmp_path):
    contigs, bed = TL.scan_contigs(False)
    files = TL.write_inputs(str(tmp_path), contigs, (), bed)
    lines, _ = TL.scan_lines(2060, False, 2)
    lines = lines + [TL.TEN_FIELDS]                          # behind every cap: never read
    cap = TL.cap_on_line(oracle_lib, lines, k, files)
    t = TL.restate(oracle_lib, TL.text_of(lines), files, max_reads=cap)
    assert t.code == 0 and t.st.capped == 1 and t.st.lines == k + 1 and t.st.reads_counted == cap
    assert TL.restate(oracle_lib, TL.text_of(lines), files).code == 1     # without a cap the ten-field line is the reference's error


@pytest.mark.parametrize("k", [1, 7, 8, 2047, 2048, 2059])
def test_a_cap_lands_on_the_stated_line_with_targets(k, oracle_lib, tmp_path):
    """With targets the run ends at twice max_reads counted reads (Profile.cpp:497-507): exome_cap makes the count at line k even."""
    contigs, bed = TL.scan_contigs(True)
    files = TL.write_inputs(str(tmp_path), contigs, (), bed)
    lines, cap = TL.exome_cap(oracle_lib, TL.scan_lines(2060, True, 2)[0], k, files)
    t = TL.restate(oracle_lib, TL.text_of(lines + [TL.TEN_FIELDS]), files, max_reads=cap)
    assert t.code == 0 and t.st.capped == 1 and t.st.lines == k + 1 and t.st.reads_counted == 2 * cap


def test_line_scan_texts():
    """break_text / text_of_length: a break at each residue of a 64-byte element, elements of 0, 1 and 64 breaks, the stated
    lengths, a break as the last byte of element 2,047 of a tile and of tile 255 of a round, no NUL byte."""
    t = TL.break_text([65] * 64)
    assert sorted(int(e) % 64 for e in TL.line_ends(t)) == list(range(64))
    t = TL.break_text([128] + [0] * 64 + [64])
    per_elem = np.bincount(TL.line_ends(t) // 64, minlength=4)
    assert list(per_elem) == [0, 1, 64, 1]
    for total in (63, 64, 65, TL.LINE_TILE - 1, TL.LINE_TILE, TL.LINE_TILE + 1):
        t = TL.text_of_length(total, 1 + total // 40000)
        assert len(t) == total and t[-1:] == b"\n" and 0 not in t
    t = TL.text_of_length(TL.LINE_TILE, 3) + TL.text_of_length(TL.LINE_TILE + 64, 3)
    assert TL.LINE_TILE - 1 in TL.line_ends(t)               # the last byte of element 2,047 of tile 0
    t = TL.text_of_length(TL.LINE_ROUND, 300)
    assert int(TL.line_ends(t)[-1]) == TL.LINE_ROUND - 1 and len(TL.line_ends(t)) == 300
    for text, where in TL.odd_byte_texts():
        assert 0 not in text and len(TL.line_ends(text)) == 40
        assert any(b in text for b in (b"\x0b\n", b"\n\x0b")) and b"\x8a" in text and b"\xff" in text and b"\t\n" in text, where


def test_fields_clauses(oracle_lib, tmp_path):
    """Each clause alone is counted or not as written beside it; the whole text counts the written number; ten fields are
    the reference's error."""
    files = TL.write_inputs(str(tmp_path), TL.fields_contigs())
    for what, line, counted in TL.fields_clauses():
        t = TL.restate(oracle_lib, line + b"\n", files, gc=False)
        assert t.code == 0 and t.st.lines == 1 and t.st.reads_counted == counted, what
    lines, counted = TL.fields_text(256, 0)
    assert counted == 256 + 22 and len(lines) == 256 + 31
    t = TL.restate(oracle_lib, TL.text_of(lines), files, gc=False)
    assert t.code == 0 and t.st.reads_counted == 278 and t.st.lines == 287
    assert t.a["isize"][1:257].sum() == 257 and t.a["isize"][77] == 2     # the numbered lines, and TLEN 77 of a clause beside line 76
    assert t.a["quality"].sum() == 4 * (278 - 3)                          # QUAL shorter, longer and empty count no quality cell
    assert t.a["subs2"].sum() == 4                                        # the one reverse read
    assert TL.restate(oracle_lib, TL.text_of(lines + [TL.TEN_FIELDS]), files, gc=False).code == 1


def test_verdict_case_counts_what_is_written(oracle_lib, tmp_path):
    contigs, vcf, lines, want = TL.verdict_case()
    files = TL.write_inputs(str(tmp_path), contigs, vcf)
    t = TL.restate(oracle_lib, TL.text_of(lines), files, n_isize=TL.VERDICT_N_ISIZE, n_indel_len=TL.VERDICT_N_INDEL)
    assert t.code == 0 and t.st.lines == len(lines) == 34
    for k, v in want.items():
        if isinstance(v, dict):
            assert {int(i): int(t.a[k][i]) for i in np.flatnonzero(t.a[k])} == v, k
        else:
            assert t.scalar(k) == v, (k, t.scalar(k), v)
    chars = sum(len(x.split(b"\t")[5]) for x in lines) - len(b"5H45M")
    assert t.st.cigar_chars == chars == (3 + 5 + 8 + 8 + 8 + 6 + 2 + 1 + 1 + 15) + 17 * 8 + 6 * 3
    assert t.st.gc_rejected == 0 and t.st.gc_windows == 4


def test_count_case_holds_what_it_is_for(oracle_lib, tmp_path):
    contigs, vcf, lines = TL.count_case(300)
    seqs = dict(contigs)
    reads = [(x.split(b"\t")[2], int(x.split(b"\t")[3]), x.split(b"\t")[9], int(x.split(b"\t")[8]), x.split(b"\t")[10]) for x in lines]
    assert {len(r[2]) for r in reads} == set(TL.COUNT_LENGTHS)
    for rev in (False, True):
        for o in range(6):     # an N at context place o in front of a base, forward and reverse; among the first K - 1 bases for o < 5
            assert any(seqs[c][p - 1 + i] == ord("N") and i + o < len(s) for c, p, s, t, _ in reads if (t < 0) == rev for i in range(len(s))), (rev, o)
    assert any(s != s.upper() for _, _, s, _, _ in reads) and all({32, 33, 126, 127} <= set(q) for *_, q in reads if len(q) >= 6)
    alts = {(r.split(b"\t")[0], int(r.split(b"\t")[1])): r.split(b"\t")[4] for r in vcf}
    assert {a for a in alts.values()} == {bytes([c]) for c in TL.PRINTABLE}
    shown = {(k % 2 == 0) for k, (c, p, s, _, _) in enumerate(reads) for i in range(len(s)) if (c, p + i) in alts}
    assert shown == {True, False}
    files = TL.write_inputs(str(tmp_path), contigs, vcf)
    for kmer, bases in ((3, b"ACTG"), (6, b"GTCA")):
        t = TL.restate(oracle_lib, TL.text_of(lines), files, kmer=kmer, bins=7, bases=bases)
        assert t.code == 0 and t.st.reads_counted == 300 and t.st.gc_rejected == 0          # ascending: countGC counts every read
        assert t.a["subs1"].sum() > 0 and t.a["subs2"].sum() > 0 and int(t.a["isize"].sum()) == 200
        q = t.a["quality"].sum(axis=(0, 1))
        assert q[0] > 0 and q[93] > 0 and q[70 - 33] > 0                                    # bytes 33 and 126 count, 32 and 127 have no cell
    # a literal X in the genome or in a shown allele counts as the trie's place holder: its twin with R there counts fewer contexts
    text = TL.text_of(lines)
    assert b"X" in text and any(r.split(b"\t")[4] == b"X" for r in vcf)
    twin = TL.write_inputs(str(tmp_path / "twin"), [(n, s.replace(b"X", b"R")) for n, s in contigs], [r.replace(b"X", b"R") for r in vcf])
    a, b = TL.restate(oracle_lib, text, files, kmer=3, bins=7), TL.restate(oracle_lib, text.replace(b"X", b"R"), twin, kmer=3, bins=7)
    assert a.st.reads_counted == b.st.reads_counted == 300 and a.a["subs1"].sum() > b.a["subs1"].sum() and a.a["subs2"].sum() == b.a["subs2"].sum()
    assert len(TL.tiny_reads(70000)) == 70000 and {len(x.split(b"\t")[9]) for x in TL.tiny_reads(64)} == {1, 2, 3}


def test_window_cases(oracle_lib, tmp_path):
    """window_case(64, 100): the short contig's window, 100 whole windows and the last one; the three with an N and the one
    without G or C are not pushed, nor is the last; the read counts are 1, 2, 3 in turn.  exome_window_case: every read
    counted, the read counts scaled."""
    contigs, lines = TL.window_case(64, 100, (1, 2, 3))
    files = TL.write_inputs(str(tmp_path / "w"), contigs)
    t = TL.restate(oracle_lib, TL.text_of(lines), files)
    assert t.code == 0 and t.st.gc_windows == 102 and t.st.gc_rejected == 0 and t.st.reads_counted == len(lines)
    pairs = t.pairs()
    assert len(pairs) == 1 + 100 - 4 and [rc for _, rc in pairs[1:8]] == [1.0, 2.0, 3.0, 2.0, 3.0, 1.0, 2.0] and all(0 < g <= 1 for g, _ in pairs)
    contigs, bed, lines = TL.exome_window_case()
    files = TL.write_inputs(str(tmp_path / "x"), contigs, (), bed)
    t = TL.restate(oracle_lib, TL.text_of(lines), files)
    assert t.code == 0 and t.st.reads_counted == len(lines) == 45 and t.st.gc_windows == 9
    sizes = [100, 113, 114, 115, 499, 1599, 100, 115, 499]       # rightPos - leftPos + 1 of the padded targets (1,599: one piece)
    reads = [1, 5, 9, 4, 8, 3, 7, 2, 6]
    want = [float(1000 * r // s) for s, r in zip(sizes, reads)][:-1]   # (the last window is never pushed)
    assert want == [10.0, 44.0, 78.0, 34.0, 16.0, 1.0, 70.0, 17.0]
    assert [rc for _, rc in t.pairs()] == want
