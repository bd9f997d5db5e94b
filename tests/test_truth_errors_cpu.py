"""`simuReads --truth-errors` without a GPU: the counting rule as the engine states it for one read (sg_errtab_observe)
against the model written from its definition (tests/errors_model.py) -- one hand-made read per clause, then 20,000
seeded random reads --, the file's text (simu_errors_format) against a formatter written from the definition, the
command lines that are refused before the engine exists, and the new names' place in the ABI list."""
import os
import re
import subprocess

import numpy as np
import pytest

import cases
import errors_model as EM
import simuscop_amd
import simuscop_amd.build as build
from errors_model import ev_pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMU = os.path.join(build.LIBDIR, "simuReads")
A, C_, T, G, N, OTHER, X = 0, 1, 2, 3, 4, 5, 6


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(SIMU):
        build.build_all()


def both(codes, reverse, events, bases, quals, mate=0, cycles=None, qual_lo=2, n_qual=40):
    """The read through the engine's rule and through the model; both tables, or Refused by both."""
    L = len(codes)
    cycles = cycles if cycles is not None else L + 40
    want = EM.Table(cycles, qual_lo, n_qual, L)
    got = np.zeros(simuscop_amd.errors_cells(cycles, n_qual, L), dtype=np.uint64)
    try:
        want.add(codes, reverse, events, bases, quals, mate)
    except EM.Refused:
        with pytest.raises(simuscop_amd.SimuError):
            simuscop_amd.errors_observe(got, codes, reverse, events, bases, quals, mate, cycles, qual_lo, n_qual)
        assert not got.any()
        raise
    simuscop_amd.errors_observe(got, codes, reverse, events, bases, quals, mate, cycles, qual_lo, n_qual)
    assert np.array_equal(got.astype(np.int64), want.flat())
    return want


TMPL = [A, C_, G, T, T, G, C_, A, A, G]            # ACGTTGCAAG; reverse complement CTTGCAACGT
Q10 = b"5" * 10                                    # quality 20


def test_forward_read():
    t = both(TMPL, False, [], b"ACGTTGCAAG", b"#+5?I5555D")
    assert t.Q[0, :, :, EM.BASES].sum() == 10 and not t.Q[0, :, :, EM.ERRORS].sum() and not t.Q[1].any()
    assert t.Q[0, 0, 0, EM.BASES] == 1 and t.Q[0, 4, ord("I") - 35, EM.BASES] == 1 and t.Q[0, 9, ord("D") - 35, EM.BASES] == 1
    assert t.S[0, A, A] == 3 and t.S[0, G, G] == 3 and t.S[0].sum() == 10
    t = both(TMPL, False, [], b"ACGTTGCATG", Q10, mate=1)
    assert t.Q[1, 8, 18].tolist() == [1, 1, 0, 0] and t.S[1, A, T] == 1 and t.Q[1, :, :, EM.ERRORS].sum() == 1 and not t.Q[0].any()


def test_reverse_read_is_compared_with_the_complement_in_reverse_order():
    t = both(TMPL, True, [], b"CTTGCAACGT", Q10)
    assert t.Q[0, :, :, EM.BASES].sum() == 10 and not t.Q[0, :, :, EM.ERRORS].sum()
    t = both(TMPL, True, [], b"ACGTTGCAAG", Q10)                     # the forward text against a reverse template
    assert t.Q[0, :, :, EM.ERRORS].sum() == sum(x != y for x, y in zip(b"ACGTTGCAAG", b"CTTGCAACGT")) == 10
    t = both(TMPL, True, [ev_pack(0, 1, 1)], b"TTGCAACGT", Q10[:9])  # j counts from the read's start: the chain's last base goes
    assert t.D[0, 0].tolist() == [1, 1] and not t.Q[0, :, :, EM.ERRORS].sum()


def test_insertion_at_the_first_and_the_last_base():
    t = both(TMPL, False, [ev_pack(0, 2, 0)], b"ATTCGTTGCAAG", b"5" * 12)
    assert t.Q[0, 1, 18, EM.INSERTED] == 1 and t.Q[0, 2, 18, EM.INSERTED] == 1 and t.Q[0, :, :, EM.BASES].sum() == 10
    assert t.I[0, 0].tolist() == [1, 2] and t.I.sum() == 3 and not t.Q[0, :, :, EM.ERRORS].sum()
    t = both(TMPL, False, [ev_pack(9, 3, 0)], b"ACGTTGCAAGTTT", b"5" * 13)
    assert t.Q[0, 10:13, 18, EM.INSERTED].tolist() == [1, 1, 1] and t.I[0, 9].tolist() == [1, 3]
    assert t.S[0].sum() == 10                                        # an inserted base has no verdict and no S cell


def test_deletion_at_the_first_base_and_clipped_at_the_end():
    t = both(TMPL, False, [ev_pack(0, 3, 1)], b"TTGCAAG", Q10[:7])
    assert t.D[0, 0].tolist() == [1, 3] and t.Q[0, :7, 18, EM.BASES].tolist() == [1] * 7 and not t.Q[0, :, :, EM.ERRORS].sum()
    t = both(TMPL, False, [ev_pack(7, 9, 1)], b"ACGTTGC", Q10[:7])   # 9 asked, 3 left
    assert t.D[0, 7].tolist() == [1, 3] and t.Q[0, :, :, EM.BASES].sum() == 7
    t = both(TMPL, False, [ev_pack(9, 1, 1)], b"ACGTTGCAA", Q10[:9])
    assert t.D[0, 9].tolist() == [1, 1]


def test_adjacent_events():
    # insertion behind base 2, deletion of bases 3..4, insertion behind base 5, deletion of 6, deletion of 7
    ev = [ev_pack(2, 1, 0), ev_pack(3, 2, 1), ev_pack(5, 2, 0), ev_pack(6, 1, 1), ev_pack(7, 1, 1)]
    t = both(TMPL, False, ev, b"ACGAGCCAG", Q10[:9])
    assert t.Q[0, :, 18, EM.INSERTED].nonzero()[0].tolist() == [3, 5, 6] and t.Q[0, :, :, EM.BASES].sum() == 6
    assert not t.Q[0, :, :, EM.ERRORS].sum() and t.I[0, :, 0].sum() == 2 and t.D[0, :, 0].sum() == 3
    for bad in ([ev_pack(3, 2, 1), ev_pack(4, 1, 0)],               # an event inside what the one before deleted
                [ev_pack(3, 1, 0), ev_pack(3, 1, 1)],               # two events on one base
                [ev_pack(5, 1, 0), ev_pack(2, 1, 0)],               # descending
                [ev_pack(10, 1, 0)],                                # behind the template
                [ev_pack(4, 0, 0)],                                 # of no length
                [ev_pack(j, 1, 0) for j in range(10)] * 4):         # more than a pass keeps
        with pytest.raises(EM.Refused):
            both(TMPL, False, bad, b"ACGTTGCAAG", Q10)


def test_template_bases_that_are_no_letter():
    codes = [A, N, X, T, OTHER, G, C_, A, A, G]
    t = both(codes, False, [], b"ANGTNGCAAG", Q10)
    assert t.Q[0, [1, 2, 4], 18, EM.OTHER].tolist() == [1, 1, 1] and t.Q[0, :, :, EM.BASES].sum() == 7 and t.S[0].sum() == 7
    assert not t.Q[0, :, :, EM.ERRORS].sum()
    t = both(codes, True, [], b"CTTGCNANNT", Q10)                    # N, X and `other` stay what they are on the other strand
    assert t.Q[0, [5, 7, 8], 18, EM.OTHER].tolist() == [1, 1, 1] and not t.Q[0, :, :, EM.ERRORS].sum()


def test_an_n_in_the_read_is_an_error():
    t = both(TMPL, False, [], b"ACGNTGCAAG", Q10)
    assert t.Q[0, 3, 18].tolist() == [1, 1, 0, 0] and t.S[0, T, N] == 1 and t.S[0, T, T] == 1
    t = both(TMPL, False, [], b"ACGtTGCAAG", Q10)                    # anything that is no A, C, G, T counts as N does
    assert t.S[0, T, N] == 1


def test_refused_reads():
    with pytest.raises(EM.Refused):
        both(TMPL, False, [], b"ACGTTGCAA", Q10[:9])                 # the events give 10 bases
    with pytest.raises(EM.Refused):
        both(TMPL, False, [ev_pack(4, 1, 0)], b"ACGTTGCAAG", Q10)    # ... 11
    with pytest.raises(EM.Refused):
        both(TMPL, False, [], b"ACGTTGCAAG", b"55555 5555")          # a byte below 33
    with pytest.raises(EM.Refused):
        both(TMPL, False, [], b"ACGTTGCAAG", b'55555"5555')          # below the table's lowest quality (35)
    with pytest.raises(EM.Refused):
        both(TMPL, False, [], b"ACGTTGCAAG", b"55555K5555")          # above its highest (74)
    both(TMPL, False, [], b"ACGTTGCAAG", b"#5555J5555")
    with pytest.raises(EM.Refused):
        both(TMPL, False, [ev_pack(9, 1, 0)], b"ACGTTGCAAGT", b"5" * 11, cycles=10)   # longer than the table's cycles
    got = np.zeros(7, dtype=np.uint64)                               # a table of another size
    with pytest.raises(simuscop_amd.SimuError):
        simuscop_amd.errors_observe(got, TMPL, False, [], b"ACGTTGCAAG", Q10, 0, 50, 2, 40)
    ok = np.zeros(simuscop_amd.errors_cells(50, 40, 10), dtype=np.uint64)
    with pytest.raises(simuscop_amd.SimuError):
        simuscop_amd.errors_observe(ok, TMPL, False, [], b"ACGTTGCAAG", Q10, 2, 50, 2, 40)    # mate 2 of 0 / 1
    with pytest.raises(simuscop_amd.SimuError):
        simuscop_amd.errors_observe(np.zeros(simuscop_amd.errors_cells(5, 40, 10), dtype=np.uint64), TMPL, False, [], b"ACGTTGCAAG", Q10, 0, 5, 2, 40)


def test_random_reads():
    """20,000 seeded reads into one table: template lengths 50 .. 700 in turn (the table is as long as the longest), 0 .. 32
    events, both strands, both mates, islands of N / other / X, a twentieth of the bases changed."""
    rng = np.random.default_rng(20240611)
    qual_lo, n_qual, total = 2, 41, 0
    lengths = [50, 63, 64, 65, 127, 128, 151, 300, 699, 700]
    per = 20000 // len(lengths)
    seen_events = set()
    for L in lengths:
        cycles = L + 32 * 5
        want = EM.Table(cycles, qual_lo, n_qual, L)
        got = np.zeros(simuscop_amd.errors_cells(cycles, n_qual, L), dtype=np.uint64)
        for i in range(per):
            n_ev = int(rng.integers(0, 33)) if i % 3 else 0
            codes, reverse, events, bases, quals = EM.random_read(rng, L, n_ev, qual_lo, n_qual)
            mate = i & 1
            try:
                want.add(codes, reverse, events, bases, quals, mate)
            except EM.Refused:                                       # (a read that 32 long insertions push past the cycles)
                with pytest.raises(simuscop_amd.SimuError):
                    simuscop_amd.errors_observe(got, codes, reverse, events, bases, quals, mate, cycles, qual_lo, n_qual)
                continue
            simuscop_amd.errors_observe(got, codes, reverse, events, bases, quals, mate, cycles, qual_lo, n_qual)
            seen_events.add(len(events))
            total += 1
        bad = np.flatnonzero(got.astype(np.int64) != want.flat())
        assert not len(bad), (L, len(bad), int(bad[0]), int(got[bad[0]]), int(want.flat()[bad[0]]))
        assert want.Q[..., EM.ERRORS].sum() > 0 and want.Q[..., EM.OTHER].sum() > 0 and want.Q[..., EM.INSERTED].sum() > 0
        assert want.D[..., 0].sum() > 0 and want.Q[1].any() and want.S[:, :, 4].sum() > 0
    assert total > 19000 and {0, 1, 32} <= seen_events


# ---- the file ----
def table_of(cells, cycles=6, qual_lo=2, n_qual=5, L=4):
    t = EM.Table(cycles, qual_lo, n_qual, L)
    for where, v in cells.items():
        getattr(t, where[0])[where[1:]] = v
    return t


FORMAT_CASES = {
    "empty": ({}, 2),
    "empty_se": ({}, 1),
    "single_row": ({("Q", 0, 2, 3, EM.BASES): 7}, 1),
    "ordering": ({("Q", 1, 0, 4, EM.BASES): 1, ("Q", 0, 5, 0, EM.OTHER): 2, ("Q", 0, 5, 1, EM.INSERTED): 3, ("Q", 0, 0, 4, EM.ERRORS): 4,
                  ("Q", 0, 0, 4, EM.BASES): 9, ("Q", 1, 3, 2, EM.BASES): 2 ** 40 + 1,
                  ("I", 1, 3, 0): 2, ("I", 1, 3, 1): 5, ("I", 0, 0, 0): 1, ("I", 0, 0, 1): 1, ("D", 0, 2, 0): 3, ("D", 0, 2, 1): 2 ** 33,
                  ("I", 0, 1, 1): 9,                                  # bases without an event: no row
                  ("S", 0, 2, 3): 11, ("S", 1, 3, 4): 12, ("S", 0, 0, 0): 2 ** 50}, 2),
    "mate_2_left_out_of_an_se_file": ({("Q", 1, 0, 0, EM.BASES): 5, ("Q", 0, 1, 1, EM.BASES): 6, ("S", 1, 0, 0): 5}, 1),
}


@pytest.mark.parametrize("case", sorted(FORMAT_CASES))
def test_format(case):
    cells, mates = FORMAT_CASES[case]
    t = table_of(cells)
    flat = t.flat().astype(np.uint64)
    text, rows = simuscop_amd.errors_format(flat, t.cycles, t.qual_lo, t.n_qual, t.L, mates)
    assert (text, rows) == EM.format_table(t, mates)
    parsed = EM.parse_file(text)
    assert len(parsed["S"]) == 20 * mates                            # every cell of the matrix, zeros too
    assert set(k[1:] for k in parsed["S"]) == {(f, to) for f in "ACGT" for to in "ACGTN"}
    q_keys = [tuple(int(v) for v in l.split("\t")[1:4]) for l in text.decode().splitlines() if l.startswith("Q\t")]
    assert q_keys == sorted(q_keys) and all(any(parsed["Q"][k]) for k in parsed["Q"])
    if case == "empty":
        assert not parsed["Q"] and not parsed["I"] and not parsed["D"] and rows == 40 and not any(parsed["S"].values())
    if case == "single_row":
        assert parsed["Q"] == {(1, 3, 5): (7, 0, 0, 0)} and rows == 21
    if case == "ordering":
        assert parsed["Q"][(1, 1, 6)] == (9, 4, 0, 0) and parsed["Q"][(2, 4, 4)] == (2 ** 40 + 1, 0, 0, 0)
        assert parsed["I"] == {(1, 1): (1, 1), (2, 4): (2, 5)} and parsed["D"] == {(1, 3): (3, 2 ** 33)}
        assert parsed["S"][(1, "T", "G")] == 11 and parsed["S"][(2, "G", "N")] == 12 and parsed["S"][(1, "A", "A")] == 2 ** 50
    if case == "mate_2_left_out_of_an_se_file":
        assert parsed["Q"] == {(1, 2, 3): (6, 0, 0, 0)}


def test_format_refuses_a_table_of_another_size():
    t = table_of({})
    with pytest.raises(simuscop_amd.SimuError):
        simuscop_amd.errors_format(t.flat().astype(np.uint64)[:-1], t.cycles, t.qual_lo, t.n_qual, t.L, 2)
    with pytest.raises(simuscop_amd.SimuError):
        simuscop_amd.errors_format(t.flat().astype(np.uint64), t.cycles, t.qual_lo, t.n_qual, t.L, 3)


# ---- command lines ----
REFUSED = {
    "world_2": ["--truth-errors", "--world", "2"],
    "gpus_2": ["--truth-errors", "--gpus", "2"],
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_cli_refuses_before_the_engine_exists(name, tmp_path):
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path / "base"))
    out = str(tmp_path / "out")
    r = subprocess.run([SIMU, cfg, "--quiet", "--out", out, *REFUSED[name]], capture_output=True, text=True, timeout=120)
    assert r.returncode not in (0, None) and r.returncode > 0, (r.returncode, r.stderr[-300:])
    assert "--truth-errors" in r.stderr, r.stderr[-300:]
    assert "GPU engine error" not in r.stderr
    assert not os.path.exists(out) or not os.listdir(out)


def test_host_haplotypes_are_accepted(tmp_path):
    """No piece map is needed, so the option goes with --host-haplotypes: the command line gets as far as the engine (and,
    where there is a GPU, through)."""
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path / "base"))
    out = str(tmp_path / "out")
    r = subprocess.run([SIMU, cfg, "--quiet", "--out", out, "--truth-errors", "--host-haplotypes"], capture_output=True, text=True, timeout=300)
    assert "--truth-errors" not in r.stderr, r.stderr[-300:]
    assert r.returncode == 0 or "GPU engine error" in r.stderr, (r.returncode, r.stderr[-300:])
    if r.returncode == 0:
        assert [x for x in os.listdir(out) if x.endswith(".truth.errors.tsv")]


def test_in_process_refusals(tmp_path):
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path / "base"))
    out = str(tmp_path / "out")
    with pytest.raises(simuscop_amd.SimuError, match="--truth-errors"):
        simuscop_amd.run_config(cfg, seed=1, output_dir=out, quiet=1, truth_errors=1, shard_world=2)
    assert not os.path.exists(out) or not os.listdir(out)


def test_new_names_are_in_the_header_and_the_abi_list():
    hdr = open(os.path.join(ROOT, "include", "simuscop_amd.h")).read()
    declared = set(re.findall(r"\b(sg_errtab_[a-z_0-9]+)\s*\(", hdr))
    assert declared == {"sg_errtab_begin", "sg_errtab_add", "sg_errtab_counts", "sg_errtab_reset", "sg_errtab_info", "sg_errtab_end",
                        "sg_errtab_observe"}
    assert declared <= set(simuscop_amd.ENGINE_SYMBOLS)
    eng = simuscop_amd.load_engine()
    for name in declared:
        getattr(eng, name)
    assert "typedef struct sg_errtab_shape {" in hdr
    opts = [f[0] for f in simuscop_amd.SimuOptions._fields_]
    assert "truth_errors" in opts
    stats = [f[0] for f in simuscop_amd.SimuStats._fields_]
    i = stats.index("errors_bases")
    assert stats[i:i + 3] == ["errors_bases", "errors_subst", "t_errors"]
    # the structs of the host library and of the Python glue list their fields in one order
    shdr = open(os.path.join(ROOT, "simuscop_amd", "csrc", "host", "simulate.h")).read()
    c_opts = re.findall(r"^\s*(?:int32_t|uint64_t|const char\*|void\*)\s+(\w+);", shdr[shdr.index("typedef struct simu_options"):shdr.index("} simu_options;")], re.M)
    assert [o for o in opts if o.startswith("truth_")] == [o for o in c_opts if o.startswith("truth_")]
    flat = []
    for chunk in re.sub(r"//[^\n]*", "", shdr[shdr.index("typedef struct simu_stats {") + 27:shdr.index("} simu_stats;")]).split(";"):
        names = re.sub(r"^\s*(uint64_t|double|float|int32_t|uint32_t)\s+", "", chunk.strip())
        flat += [re.sub(r"\[\d+\]", "", n.strip()) for n in names.split(",") if n.strip()]
    assert flat == stats
    assert callable(simuscop_amd.errors_observe) and callable(simuscop_amd.errors_format)
    for name in ("errors_begin", "errors_add", "errors_counts", "errors_reset", "errors_info", "errors_end"):
        assert callable(getattr(simuscop_amd.Session, name))
