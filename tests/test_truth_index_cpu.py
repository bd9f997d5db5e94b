"""--truth-index without a GPU: simu_bai_build (host/truth_index.cpp) against bai_model's serialiser on hand-made and
seeded random tables -- also in a stand-alone program under the sanitizers -- the refusals, the struct layouts and the
ABI names."""
import os
import random
import re
import subprocess

import pytest

import bai_model as M
import bam_util
import cases
import simuscop_amd
import simuscop_amd.build as build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMU = os.path.join(build.LIBDIR, "simuReads")
EOF_VOFF = 1 << 40


def R(ref, beg, stop, unmapped=False):
    return dict(ref=ref, beg=beg, stop=stop, bin=bam_util.reg2bin(beg, stop) if ref >= 0 else None, unmapped=unmapped)


def place(recs, rng=None):
    """Ascending start offsets for records in file order, and each record's end: the next one's start."""
    v = 5 << 16
    for r in recs:
        r["voff"] = v
        v += (rng.randrange(1, 70000) if rng else 300) << (16 if rng and rng.random() < 0.3 else 0)
    for a, b in zip(recs, recs[1:]):
        a["end"] = b["voff"]
    if recs:
        recs[-1]["end"] = EOF_VOFF
    return recs


def device_tables(recs, ref_len, cuts):
    """What the driver hands simu_bai_build: the chunk rows of the calls [cuts[i], cuts[i + 1]) in call order, each open
    end closed with the next call's first record (the last with the end-of-file offset), linear cells, counts."""
    bounds = [0] + sorted(cuts) + [len(recs)]
    rows = []
    for a, b in zip(bounds, bounds[1:]):
        if a == b:
            continue
        nxt = recs[b]["voff"] if b < len(recs) else EOF_VOFF
        rows += [(k, beg, nxt if end == M.OPEN else end) for k, beg, end in M.chunk_rows(recs[a:b])]
    lin, counts = M.linear_and_counts(recs, ref_len)
    return rows, lin, counts


def both(recs, ref_len, cuts=()):
    rows, lin, counts = device_tables(recs, ref_len, cuts)
    bai, bins, chunks = simuscop_amd.bai_build(ref_len, rows, lin, counts)
    want = M.serialise(*M.index(recs, len(ref_len)))
    assert bai == want
    refs, no_coor = M.parse(bai)
    assert bins == sum(len(x["bins"]) for x in refs) and chunks == sum(len(c) for x in refs for c in x["bins"].values())
    assert all(v != M.OPEN for x in refs for v in x["linear"])                       # no entry is left at ~0
    return refs, no_coor


LENS = [1 << 20, 5000, 1 << 29]


def test_no_records_at_all():
    refs, no_coor = both([], LENS)
    assert no_coor == 0 and all(x == dict(bins={}, pseudo=None, linear=[]) for x in refs)
    assert both([], [])[0] == []
    assert len(simuscop_amd.bai_build(LENS, [], [M.OPEN] * (64 + 1 + 32768), [0, 0, M.OPEN] * 3 + [0])[0]) == 8 + 3 * 8 + 8


def test_one_record():
    refs, _ = both(place([R(0, 100, 250)]), LENS)
    assert refs[0]["bins"] == {4681: [[5 << 16, EOF_VOFF]]} and refs[0]["pseudo"] == [[5 << 16, EOF_VOFF], [1, 0]] and refs[0]["linear"] == [5 << 16]


def test_an_empty_reference_between_two_used_ones():
    refs, _ = both(place([R(0, 1, 9), R(2, 1, 9), R(2, 5, 9, True)]), LENS, cuts=(1,))
    assert refs[1] == dict(bins={}, pseudo=None, linear=[]) and refs[2]["pseudo"][1] == [1, 1]


def test_a_bin_met_twice_with_another_between():
    recs = place([R(0, 10, 20), R(0, 16380, 16390), R(0, 16381, 16382), R(0, 16382, 16383)])   # 4681, 585, 4681 4681
    for cuts in ((), (1,), (2,), (3,), (1, 2, 3)):
        refs, _ = both(recs, LENS, cuts)
        assert [len(refs[0]["bins"][b]) for b in (585, 4681)] == [1, 2]


def test_chunks_that_touch_across_a_call_boundary_are_joined_and_others_are_not():
    recs = place([R(0, 10 + i, 20 + i) for i in range(6)] + [R(0, 20000, 20001)] + [R(0, 40000 + i, 40001 + i) for i in range(4)])
    for cuts in ((3,), (1, 2, 3, 4, 5), (8,), (9, 10)):
        refs, _ = both(recs, LENS, cuts)
        assert [len(refs[0]["bins"][b]) for b in (4681, 4682, 4683)] == [1, 1, 1]
    # the same bin in two calls with a record of another bin between them: kept apart
    recs = place([R(0, 10, 20), R(0, 10, 20000), R(0, 11, 20)])
    refs, _ = both(recs, LENS, (1, 2))
    assert len(refs[0]["bins"][4681]) == 2


def test_only_records_without_a_reference():
    refs, no_coor = both(place([R(-1, -1, 0, True) for _ in range(5)]), LENS, (2,))
    assert no_coor == 5 and all(x["pseudo"] is None and not x["bins"] and not x["linear"] for x in refs)


def test_a_window_gap_is_filled_from_the_right_and_n_intv_ends_at_the_last_touched_window():
    recs = place([R(0, 5, 10), R(0, 5 << 14, (5 << 14) + 3), R(0, (7 << 14) - 10, 8 << 14)])
    refs, _ = both(recs, LENS)
    lin = refs[0]["linear"]
    assert len(lin) == 8                                             # the last record ends exactly on a window boundary
    assert lin[0] == recs[0]["voff"] and lin[1:6] == [recs[1]["voff"]] * 5 and lin[6:] == [recs[2]["voff"]] * 2
    assert len(both(place([R(0, 0, 1 << 14)]), LENS)[0][0]["linear"]) == 1
    assert len(both(place([R(0, 0, (1 << 14) + 1)]), LENS)[0][0]["linear"]) == 2
    assert len(both(place([R(2, (1 << 29) - 1, 1 << 29)]), LENS)[0][2]["linear"]) == 1 << 15


def random_records(rng):
    n = rng.choice((0, 1, 2, 5, 30, 200))
    ref_len = [rng.choice((1, 16384, 16385, 100000, 1 << 22)) for _ in range(rng.randrange(1, 5))]
    recs = []
    for _ in range(n):
        ref = rng.randrange(-1, len(ref_len))
        if ref < 0:
            recs.append((1 << 40, R(-1, -1, 0, True)))
            continue
        beg = rng.randrange(ref_len[ref])
        if rng.random() < 0.5:
            beg = min(beg, rng.randrange(1, 40000)) if ref_len[ref] > 1 else 0
        stop = min(ref_len[ref], beg + rng.choice((1, 2, 100, 16384, 50000)))
        unm = rng.random() < 0.15
        recs.append((ref << 32 | beg, R(ref, beg, beg + 1 if unm else stop, unm)))
    recs = [r for _, r in sorted(recs, key=lambda t: t[0])]
    return place(recs, rng), ref_len


def test_seeded_random_tables():
    rng = random.Random(20261019)
    joined = empty_refs = 0
    for _ in range(2000):
        recs, ref_len = random_records(rng)
        cuts = sorted(rng.randrange(len(recs) + 1) for _ in range(rng.choice((0, 1, 3, 8))))
        refs, _ = both(recs, ref_len, cuts)
        rows, _, _ = device_tables(recs, ref_len, cuts)
        joined += len(rows) > sum(len(c) for x in refs for c in x["bins"].values())
        empty_refs += any(x["pseudo"] is None for x in refs)
    assert joined > 200 and empty_refs > 200


def test_tables_that_describe_no_index_are_refused():
    recs = place([R(0, 1, 9), R(0, 20000, 20001)])
    rows, lin, counts = device_tables(recs, LENS, ())
    for bad in ([(rows[0][0], rows[0][1], M.OPEN)] + rows[1:], [(3 << 32 | 4681, 1, 2)] + rows, [(37450, 1, 2)] + rows, rows[:0]):
        with pytest.raises(simuscop_amd.SimuError, match="refused"):
            simuscop_amd.bai_build(LENS, bad, lin, counts)


def test_the_serialiser_under_the_sanitizers(tmp_path):
    """tools/bai_build_sanitized.sh: simu_bai_build in a stand-alone program with its own main, AddressSanitizer +
    UndefinedBehaviorSanitizer, against a serialiser written there.  CPU only, no Python in that process, nothing
    preloaded."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "bai_build_sanitized.sh"), "2000", "77"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    assert "all as the plain serialiser has them" in r.stdout


# ---- refusals: before anything is forked or written, no device is touched ----
TEXT = "Error: --truth-index needs --truth-sort: a BAI indexes a coordinate-sorted BAM"


@pytest.mark.parametrize("flags", [["--truth-index"], ["--truth-bam", "--truth-index"], ["--truth-bam", "--truth-tags", "--truth-index", "--gpus", "2"]])
def test_command_line_refusal(flags, tmp_path):
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path / "base"))
    out = str(tmp_path / "out")
    r = subprocess.run([SIMU, cfg, "--quiet", "--out", out, *flags], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stderr.strip() == TEXT, (r.returncode, r.stderr[-300:])
    assert not os.path.exists(out) or not os.listdir(out)


def test_in_process_refusal_and_the_refusals_in_front_of_it(tmp_path):
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path / "base"))
    out = str(tmp_path / "out")
    with pytest.raises(simuscop_amd.SimuError, match=re.escape(TEXT)):
        simuscop_amd.run_config(cfg, seed=1, output_dir=out, quiet=1, truth_bam=1, truth_index=1)
    with pytest.raises(simuscop_amd.SimuError, match="--truth-sort cannot be combined with --world"):
        simuscop_amd.run_config(cfg, seed=1, output_dir=out, quiet=1, truth_bam=1, truth_sort=1, truth_index=1, shard_world=2)
    assert not os.path.exists(out) or not os.listdir(out)
    for flags, text in ((["--truth-sort", "--truth-index"], "Error: --truth-sort needs --truth-bam: it is the truth BAM's records that are sorted"),
                        (["--truth-tags", "--truth-index"], "Error: --truth-tags needs --truth-bam: the tags go on the truth BAM's records")):
        r = subprocess.run([SIMU, cfg, "--quiet", "--out", out, *flags], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and r.stderr.strip() == text


# ---- struct order and the ABI list ----
def test_new_names_are_in_the_header_the_abi_list_and_the_structs():
    hdr = open(os.path.join(ROOT, "include", "simuscop_amd.h")).read()
    declared = set(re.findall(r"\b(sg_bamindex_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == {"sg_bamindex_begin", "sg_bamindex_add", "sg_bamindex_chunks", "sg_bamindex_finish", "sg_bamindex_end"}
    assert declared <= set(simuscop_amd.ENGINE_SYMBOLS)
    eng = simuscop_amd.load_engine()
    for name in declared:
        getattr(eng, name)
    assert re.search(r"#define SG_BAMINDEX_MERGE %d\b" % simuscop_amd.BAMINDEX_MERGE, hdr)
    assert re.search(r"#define SG_BAMINDEX_DEFLATE %d\b" % simuscop_amd.BAMINDEX_DEFLATE, hdr)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in integ for name in declared)
    # the option sits directly in front of truth_bam, the stats directly in front of truth_records
    opts = [f[0] for f in simuscop_amd.SimuOptions._fields_]
    i = opts.index("truth_bam")
    assert opts[i - 2:i + 1] == ["unique_contigs", "truth_index", "truth_bam"]
    stats = [f[0] for f in simuscop_amd.SimuStats._fields_]
    i = stats.index("truth_records")
    assert stats[i - 5:i + 1] == ["emit_clean_cap", "bai_bins", "bai_chunks", "bai_bytes", "t_bai", "truth_records"]
    # the structs of the host library and of the Python glue list their fields in one order
    shdr = open(os.path.join(ROOT, "simuscop_amd", "csrc", "host", "simulate.h")).read()
    c_opts = re.findall(r"^\s*(?:int32_t|uint64_t|const char\*|void\*)\s+(\w+);", shdr[shdr.index("typedef struct simu_options"):shdr.index("} simu_options;")], re.M)
    assert [o for o in opts if o.startswith("truth_")] == [o for o in c_opts if o.startswith("truth_")]
    assert c_opts[c_opts.index("truth_index") - 1] == "unique_contigs"
    flat = []
    for chunk in re.sub(r"//[^\n]*", "", shdr[shdr.index("typedef struct simu_stats {") + 27:shdr.index("} simu_stats;")]).split(";"):
        names = re.sub(r"^\s*(uint64_t|double|float|int32_t|uint32_t)\s+", "", chunk.strip())
        flat += [re.sub(r"\[\d+\]", "", n.strip()) for n in names.split(",") if n.strip()]
    assert flat == stats
    assert "simu_bai_build(" in shdr
    assert all(callable(getattr(simuscop_amd, n)) for n in ("bamindex_begin", "bamindex_add", "bamindex_chunks", "bamindex_finish", "bai_build"))
    assert simuscop_amd.default_options(truth_index=1).truth_index == 1 and simuscop_amd.default_options().truth_index == 0
    # the --stats line: the new group stands behind gz_bytes= and in front of truth_records=
    main = open(os.path.join(ROOT, "simuscop_amd", "csrc", "host", "main.cpp")).read()
    assert 'gz_bytes=%llu | "\n            "bai_bins=%llu bai_chunks=%llu bai_bytes=%llu bai_s=%.3f | "\n            "truth_records=%llu' in main
    assert "--truth-index" in main[:main.index("#include")]
    fmt = "".join(re.findall(r'"((?:[^"\\]|\\.)*)"', main[main.index('"stats: reads='):main.index("(unsigned long long)st.reads")]))
    keys = re.findall(r"(\w+)=%", fmt)
    new = ["bai_bins", "bai_chunks", "bai_bytes", "bai_s"]
    assert all(k in keys for k in new)
    assert all(len(re.findall(r"\b" + k + "=", fmt)) == 1 for k in keys)        # as the tests look a key up, each is found once
