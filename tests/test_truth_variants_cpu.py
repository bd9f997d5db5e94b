"""`simuReads --truth-variants` without a GPU: sg_variant_observe -- the engine's piece-level scan, as host code -- against
the label-level model of the same rule (tests/variant_model.py), one hand-made piece table per clause with the counts it
must give written out, then seeded random tables; the file's formatter against a second writing of the format; the
command lines that are refused before the engine exists; the new names in the header and the ABI list."""
import os
import random
import re
import subprocess

import pytest

import cases
import simuscop_amd
import simuscop_amd.build as build
import variant_model as vm
from variant_model import DEL, INS, SNV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMU = os.path.join(build.LIBDIR, "simuReads")


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(SIMU):
        build.build_all()


def both(pieces, codes, off, L, rows):
    """{row: [alt, total]} of the engine's scan, checked against the model."""
    rows = vm.sort_rows(rows)
    got = {}
    for r, alt in simuscop_amd.variant_observe(pieces, codes, off, L, rows):
        c = got.setdefault(r, [0, 0])
        c[1] += 1
        c[0] += 1 if alt else 0
    exp = vm.observe(pieces, codes, off, L, rows)
    assert got == exp, (got, exp, pieces, off, L, rows)
    return {rows[r]: tuple(c) for r, c in got.items()}


REF = [(0, 1000, 500, 0, 0, 1)]            # one reference piece: chain offset x is contig position 1000 + x
A, C_, T, G = 0, 1, 2, 3


def codes_with(L, at=None, code=G, fill=A):
    c = [fill] * L
    if at is not None:
        c[at] = code
    return c


def test_snv_alt_ref_and_other_allele():
    L = 50
    g, t, c = (0, SNV, 1110, 0, "G"), (0, SNV, 1110, 0, "T"), (0, SNV, 1110, 0, "c")   # a lower-case allele counts as its letter
    assert both(REF, codes_with(L, 10, G), 100, L, [g, t, c]) == {g: (1, 1), t: (0, 1), c: (0, 1)}
    assert both(REF, codes_with(L, 10, C_), 100, L, [g, t, c]) == {g: (0, 1), t: (0, 1), c: (1, 1)}
    assert both(REF, codes_with(L), 100, L, [g]) == {g: (0, 1)}                        # the haplotype shows the reference base
    assert both(REF, codes_with(L), 100, L, [(1, SNV, 1110, 0, "A"), (0, SNV, 1150, 0, "A"), (0, SNV, 1099, 0, "A")]) == {}


def test_site_on_the_first_and_last_base():
    L = 50
    first, last = (0, SNV, 1100, 0, "A"), (0, SNV, 1149, 0, "A")
    assert both(REF, codes_with(L), 100, L, [first, last]) == {first: (1, 1), last: (1, 1)}
    # pairs need a base behind: an insertion or a deletion anchored on the last base counts nowhere, on the last but one it does
    i_last, d_last, i_prev, d_prev = (0, INS, 1149, 2, 0), (0, DEL, 1150, 2, 0), (0, INS, 1148, 2, 0), (0, DEL, 1149, 2, 0)
    assert both(REF, codes_with(L), 100, L, [i_last, d_last, i_prev, d_prev]) == {i_prev: (0, 1), d_prev: (0, 1)}
    # a deletion whose anchor lies in front of the template's first base counts nowhere; anchored on it, it does
    d_front, d_first = (0, DEL, 1100, 3, 0), (0, DEL, 1101, 3, 0)
    assert both(REF, codes_with(L), 100, L, [d_front, d_first]) == {d_first: (0, 1)}


def test_deletion_ref_alt_and_other_joints():
    L = 50
    gone = [(0, 1000, 120, 0, 0, 1), (120, 1125, 300, 0, 0, 0)]              # bases [1120, 1125) are deleted
    d5, d4, d_in = (0, DEL, 1120, 5, 0), (0, DEL, 1120, 4, 0), (0, DEL, 1122, 2, 0)
    assert both(gone, codes_with(L), 100, L, [d5, d4, d_in]) == {d5: (1, 1)}   # another gap length: neither ref nor alt
    assert both(REF, codes_with(L), 100, L, [d5, d4]) == {d5: (0, 1), d4: (0, 1)}
    seg = [(0, 1000, 120, 0, 0, 1), (120, 1125, 300, 0, 0, 1)]               # seg_first plays no part
    assert both(seg, codes_with(L), 100, L, [d5]) == {d5: (1, 1)}
    straight = [(0, 1000, 120, 0, 0, 1), (120, 1120, 300, 0, 0, 1)]          # a joint that goes straight on is reference
    assert both(straight, codes_with(L), 100, L, [d5]) == {d5: (0, 1)}
    other = [(0, 1000, 120, 0, 0, 1), (120, 1125, 300, 1, 0, 0)]             # the same position on another contig
    assert both(other, codes_with(L), 100, L, [d5]) == {}
    assert both(gone, codes_with(L), 70, L, [d5]) == {}                      # the template ends on the anchor
    assert both(gone, codes_with(L), 71, L, [d5]) == {d5: (1, 1)}


def test_deletion_at_position_0_counts_nothing():
    start = [(0, 0, 400, 0, 0, 1)]
    d0 = (0, DEL, 0, 3, 0)
    assert both(start, codes_with(50), 0, 50, [d0]) == {}
    cut = [(0, 3, 400, 0, 0, 1)]                                             # the haplotype lacks [0, 3)
    assert both(cut, codes_with(50), 0, 50, [d0]) == {}


def test_insertion_ref_and_alt():
    L = 50
    ins = [(0, 1000, 120, 0, 0, 1), (120, 7, 10, 0, 1, 0), (130, 1120, 300, 0, 0, 0)]     # 10 bases behind base 1119
    i10, i9, i_next = (0, INS, 1119, 10, 0), (0, INS, 1119, 9, 0), (0, INS, 1120, 10, 0)
    assert both(ins, codes_with(L), 100, L, [i10, i9, i_next]) == {i10: (1, 1), i_next: (0, 1)}    # a literal of another length
    assert both(REF, codes_with(L), 100, L, [i10, i9]) == {i10: (0, 1), i9: (0, 1)}


def test_insertion_literal_cut_or_last():
    L = 50
    ins = [(0, 1000, 120, 0, 0, 1), (120, 7, 10, 0, 1, 0), (130, 1120, 300, 0, 0, 0)]
    i10 = (0, INS, 1119, 10, 0)
    assert both(ins, codes_with(L), 119, L, [i10]) == {i10: (1, 1)}          # the anchor is the template's first base
    assert both(ins, codes_with(L), 120, L, [i10]) == {}                     # cut by the template's start: no anchor
    assert both(ins, codes_with(L), 125, L, [i10]) == {}
    assert both(ins, codes_with(L), 80, L, [i10]) == {}                      # the literal is the template's last bases
    assert both(ins, codes_with(L), 81, L, [i10]) == {i10: (1, 1)}           # one more template base behind it
    assert both(ins, codes_with(L), 79, L, [i10]) == {}                      # cut by the template's end
    assert both(ins, codes_with(L), 71, L, [i10]) == {}                      # ... down to its first base
    assert both(ins, codes_with(L), 70, L, [i10]) == {}                      # the template ends on the anchor


def test_two_literals_in_a_row():
    L = 50
    two = [(0, 1000, 120, 0, 0, 1), (120, 7, 4, 0, 1, 0), (124, 30, 6, 0, 1, 0), (130, 1120, 300, 0, 0, 0)]
    i4, i6, i10 = (0, INS, 1119, 4, 0), (0, INS, 1119, 6, 0), (0, INS, 1119, 10, 0)
    assert both(two, codes_with(L), 100, L, [i4, i6, i10]) == {i4: (1, 1)}   # the first literal is the one behind the anchor
    assert both(two, codes_with(L), 75, L, [i4]) == {i4: (1, 1)}             # followed by a literal base: still a template base
    assert both(two, codes_with(L), 74, L, [i4]) == {}


def test_a_site_present_twice():
    L = 60
    twice = [(0, 1000, 20, 0, 0, 1), (20, 1000, 20, 0, 0, 0), (40, 1000, 20, 0, 0, 0), (60, 1020, 200, 0, 0, 0)]   # three tandem copies
    s, d, i = (0, SNV, 1005, 0, "G"), (0, DEL, 1010, 2, 0), (0, INS, 1019, 3, 0)
    codes = codes_with(L)
    codes[5] = G
    codes[45] = G
    assert both(twice, codes, 0, L, [s, d, i]) == {s: (2, 3), d: (0, 3)}     # 1019 is followed by 1000 twice, then the template ends
    assert both(twice, codes[:41] + [A], 0, 42, [s, d, i]) == {s: (1, 2), d: (0, 2)}
    assert both(twice, codes + [A], 0, 61, [i]) == {i: (0, 1)}


@pytest.mark.parametrize("seed", range(10))
def test_random_tables_match_the_model(seed):
    rng = random.Random(8800 + seed)
    hits = alts = 0
    for _ in range(2000):
        pieces, codes, off, L, rows = vm.random_case(rng)
        got = both(pieces, codes, off, L, rows)
        hits += sum(c[1] for c in got.values())
        alts += sum(c[0] for c in got.values())
    assert hits > 2000 and alts > 200                                        # the tables do meet the templates


def test_bad_arguments_are_refused():
    ok = [(0, SNV, 1110, 0, "G")]
    with pytest.raises(simuscop_amd.SimuError):
        simuscop_amd.variant_observe(REF, codes_with(50), 480, 50, ok)                                  # runs off the pieces
    for rows in ([(0, SNV, 1110, 0, "G"), (0, SNV, 1110, 0, "G")],          # twice
                 [(0, SNV, 1111, 0, "G"), (0, SNV, 1110, 0, "G")],          # out of order
                 [(0, DEL, 1110, 0, 0)], [(0, INS, 1110, 0, 0)],            # no length
                 [(0, 3, 1110, 1, 0)], [(0, SNV, 2 ** 32, 0, "G")]):
        with pytest.raises(simuscop_amd.SimuError):
            simuscop_amd.variant_observe(REF, codes_with(50), 100, 50, rows)


# ---- the file ----
CONTIGS = [("chr1", 1000), ("chr2", 300), ("HLA-A*01:01", 50)]
POPUS = ["normal", "clone1", "clone2"]


def model_file(contigs, popus, rows, counts=None):
    """The file's definition, written a second time: (text, table rows, dropped)."""
    ids = {n: i for i, (n, _) in enumerate(contigs)}
    table, dropped = {}, 0
    for kind, contig, pos, popu, text in rows:
        p = pos - 1
        if contig not in ids or p < 0 or p >= contigs[ids[contig]][1]:
            dropped += 1
            continue
        if kind in "sp":
            key = (ids[contig], p, 0, ord(text[0].upper()))
        elif kind == "i":
            key = (ids[contig], p, 1, len(text))
        else:
            key = (ids[contig], p, 2, int(text))
        if (kind in "sp" and not text) or key[3] < 1:
            dropped += 1
            continue
        e = table.setdefault(key, {"listed": False, "popus": set(), "text": text})
        if kind != "p":
            e["listed"] = True
            e["popus"].add(popu)
    lines = ["#chrom\tpos\ttype\tallele\talt_reads\ttotal_reads\tpopulations\n"]
    for n, key in enumerate(sorted(table)):
        e = table[key]
        typ = ("s" if e["listed"] else "p") if key[2] == 0 else "id"[key[2] - 1]
        allele = chr(key[3]) if key[2] == 0 else e["text"] if key[2] == 1 else str(key[3])
        alt, total = counts[n] if counts is not None else (0, 0)
        pl = ",".join(popus[q] for q in sorted(e["popus"])) if typ != "p" and e["popus"] else "."
        lines.append("%s\t%d\t%s\t%s\t%d\t%d\t%s\n" % (contigs[key[0]][0], key[1] + 1, typ, allele, alt, total, pl))
    return "".join(lines).encode(), len(table), dropped


FILE_ROWS = [
    ("s", "chr2", 7, 1, "G"), ("s", "chr1", 500, 2, "t"), ("s", "chr1", 500, 1, "T"), ("s", "chr1", 500, 0, "C"),   # merge on the upper-case allele; config order
    ("p", "chr1", 500, -1, "T"), ("p", "chr1", 500, -1, "A"), ("p", "chr1", 20, -1, "g"),                             # s over p; a p row of its own
    ("i", "chr1", 500, 2, "ACG"), ("i", "chr1", 500, 1, "TTT"), ("i", "chr1", 500, 1, "TTTT"),                        # merge on the length: the first sequence met
    ("d", "chr1", 500, 1, "3"), ("d", "chr1", 500, 2, "3"), ("d", "chr1", 500, 2, "12"), ("d", "chr1", 1, 0, "2"),
    ("s", "chr1", 1000, 0, "A"), ("s", "chr1", 1, 0, "A"), ("s", "HLA-A*01:01", 50, 2, "N"),
    # dropped: behind the contig's end, position 0, a contig the reference does not hold, a deletion without a length
    ("s", "chr1", 1001, 0, "A"), ("i", "chr2", 301, 0, "AC"), ("d", "chr2", 0, 0, "4"), ("s", "chr9", 5, 0, "A"), ("p", "9", 5, -1, "A"),
    ("d", "chr1", 40, 0, "0"),
]


def test_format_matches_its_definition():
    text, n, dropped = simuscop_amd.variants_format(CONTIGS, POPUS, FILE_ROWS)
    exp = model_file(CONTIGS, POPUS, FILE_ROWS)
    assert (text, n, dropped) == exp
    assert dropped == 6 and n == 13
    lines = text.decode().splitlines()
    assert lines[0] == "#chrom\tpos\ttype\tallele\talt_reads\ttotal_reads\tpopulations"
    assert all(l.split("\t")[4:6] == ["0", "0"] for l in lines[1:])                        # every row is written, counts or not
    assert "chr1\t500\ts\tT\t0\t0\tclone1,clone2" in lines and "chr1\t500\tp\tA\t0\t0\t." in lines
    assert "chr1\t500\ti\tACG\t0\t0\tclone1,clone2" in lines and "chr1\t500\td\t3\t0\t0\tclone1,clone2" in lines
    at500 = [l.split("\t")[2:4] for l in lines if l.startswith("chr1\t500\t")]
    assert at500 == [["p", "A"], ["s", "C"], ["s", "T"], ["i", "ACG"], ["i", "TTTT"], ["d", "3"], ["d", "12"]]
    order = [l.split("\t")[0] for l in lines[1:]]
    assert order == sorted(order, key=[c[0] for c in CONTIGS].index)                       # refID order, not name order


def test_format_with_counts_and_the_table():
    counts = [(i, 2 * i + 1) for i in range(13)]
    counts[3] = (2 ** 32 - 1, 2 ** 32 - 1)
    text, n, dropped, table = simuscop_amd.variants_format(CONTIGS, POPUS, FILE_ROWS, counts, want_table=True)
    assert text == model_file(CONTIGS, POPUS, FILE_ROWS, counts)[0]
    # the table is the file's rows as the engine takes them: sorted, 0-based, the allele's letter for SNVs
    assert table == vm.sort_rows(table) and len(table) == n
    for row, line in zip(table, text.decode().splitlines()[1:]):
        f = line.split("\t")
        assert CONTIGS[row[0]][0] == f[0] and row[2] + 1 == int(f[1])
        assert {"s": SNV, "p": SNV, "i": INS, "d": DEL}[f[2]] == row[1]
        assert (chr(row[4]) == f[3] and row[3] == 0) if row[1] == SNV else (row[4] == 0 and row[3] == (len(f[3]) if row[1] == INS else int(f[3])))
    with pytest.raises(simuscop_amd.SimuError):
        simuscop_amd.variants_format(CONTIGS, POPUS, FILE_ROWS, counts[:-1])


def test_format_of_an_empty_table():
    text, n, dropped = simuscop_amd.variants_format(CONTIGS, POPUS, [])
    assert (n, dropped) == (0, 0) and text == b"#chrom\tpos\ttype\tallele\talt_reads\ttotal_reads\tpopulations\n"


# ---- refusals ----
REFUSED = {
    "world_2": ["--truth-variants", "--world", "2"],
    "gpus_2": ["--truth-variants", "--gpus", "2"],
    "host_haplotypes": ["--truth-variants", "--host-haplotypes"],
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_cli_refuses_before_the_engine_exists(name, tmp_path):
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path / "base"))
    out = str(tmp_path / "out")
    r = subprocess.run([SIMU, cfg, "--quiet", "--out", out, *REFUSED[name]], capture_output=True, text=True, timeout=120)
    assert r.returncode not in (0, None) and r.returncode > 0, (r.returncode, r.stderr[-300:])
    assert "--truth-variants" in r.stderr, r.stderr[-300:]
    assert "GPU engine error" not in r.stderr
    assert not os.path.exists(out) or not os.listdir(out)


def test_in_process_refusals(tmp_path):
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path / "base"))
    for kw in (dict(truth_variants=1, host_haplotypes=1), dict(truth_variants=1, shard_world=2)):
        out = str(tmp_path / "out")
        with pytest.raises(simuscop_amd.SimuError, match="--truth-variants"):
            simuscop_amd.run_config(cfg, seed=1, output_dir=out, quiet=1, **kw)
        assert not os.path.exists(out) or not os.listdir(out)


def test_new_names_are_in_the_header_and_the_abi_list():
    hdr = open(os.path.join(ROOT, "include", "simuscop_amd.h")).read()
    declared = set(re.findall(r"\b(sg_variants?_[a-z_0-9]+)\s*\(", hdr))
    assert declared == {"sg_variants_begin", "sg_variants_add", "sg_variants_counts", "sg_variants_reset", "sg_variants_info",
                        "sg_variants_end", "sg_variant_observe"}
    assert declared <= set(simuscop_amd.ENGINE_SYMBOLS)
    assert "typedef struct sg_variant {" in hdr
    opts = [f[0] for f in simuscop_amd.SimuOptions._fields_]
    assert opts[-2:] == ["truth_variants", "truth_depth"]
    assert [f[0] for f in simuscop_amd.SimuStats._fields_[-7:]] == ["variant_rows", "variant_dropped", "variant_hits", "t_variants",
                                                                    "depth_bases", "depth_rows", "t_depth"]
    shdr = open(os.path.join(ROOT, "simuscop_amd", "csrc", "host", "simulate.h")).read()
    assert re.search(r"int32_t truth_variants;.*?\n\s*int32_t truth_depth;", shdr, re.S)
    assert re.search(r"double t_variants;[^\n]*\n\s*uint64_t depth_bases;", shdr)
