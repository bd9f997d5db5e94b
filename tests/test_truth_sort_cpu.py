"""`simuReads --truth-sort` without a GPU: the tile cutter (simu_sort_tiles) against a brute-force model -- concatenate,
sort, cut -- on hand-made and seeded random run sets; the same function in a stand-alone program under the sanitizers;
the command line's refusals; the structs and the ABI list."""
import os
import random
import re
import subprocess

import pytest

import cases
import simuscop_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMU = os.path.join(ROOT, "simuscop_amd", "lib", "simuReads")
KMAX = 2 ** 64 - 1


def model_tiles(runs, budget):
    """Brute force: all (key, bytes) sorted by key, grouped by key value, then greedily cut -- a tile takes whole key
    values while they fit the budget; a key value that alone does not fit is a tile of its own, marked."""
    per_key = {}
    for keys, lens in runs:
        assert list(keys) == sorted(keys)
        for k, n in zip(keys, lens):
            per_key[k] = per_key.get(k, 0) + n
    tiles, cur, cur_bytes = [], None, 0
    for k in sorted(per_key):
        b = per_key[k]
        if b > budget:
            if cur is not None:
                tiles.append((cur, False))
            tiles.append((k, True))
            cur, cur_bytes = None, 0
        elif cur is None:
            cur, cur_bytes = k, b
        elif cur_bytes + b <= budget:
            cur_bytes += b
        else:
            tiles.append((cur, False))
            cur, cur_bytes = k, b
    if cur is not None:
        tiles.append((cur, False))
    return tiles


def check_properties(runs, budget, tiles):
    """Tiles partition every record exactly once, in key order; an unmarked tile is within the budget, a marked one has
    one key and exceeds it."""
    firsts = [f for f, _ in tiles]
    assert firsts == sorted(set(firsts))
    recs = sorted((k, n) for keys, lens in runs for k, n in zip(keys, lens))
    seen = 0
    for i, (first, single) in enumerate(tiles):
        hi = firsts[i + 1] if i + 1 < len(tiles) else KMAX + 1
        mine = [(k, n) for k, n in recs if first <= k < hi]
        assert mine and mine[0][0] == first, "an empty tile, or a splitter no record has"
        seen += len(mine)
        total = sum(n for _, n in mine)
        if single:
            assert len({k for k, _ in mine}) == 1 and total > budget
        else:
            assert total <= budget
    assert seen == len(recs)
    if recs:
        assert firsts[0] == recs[0][0]   # nothing in front of the first tile


def both(runs, budget):
    got = simuscop_amd.sort_tiles(runs, budget)
    assert got == model_tiles(runs, budget), (runs, budget)
    check_properties(runs, budget, got)
    return got


def test_hand_made_cases():
    assert both([], 100) == []
    assert both([([], [])], 100) == []
    assert both([([5, 7, 9], [10, 10, 10])], 100) == [(5, False)]                        # one run, everything fits
    assert both([([5, 7, 9], [10, 10, 10])], 20) == [(5, False), (9, False)]
    assert both([([5, 7, 9], [10, 10, 10]), ([], []), ([7, 7], [10, 10])], 30) == [(5, False), (7, False), (9, False)]   # an empty run
    assert both([([4, 4, 4], [10, 10, 10]), ([4], [10])], 100) == [(4, False)]           # all keys equal, light
    assert both([([4, 4, 4], [10, 10, 10]), ([4], [10])], 39) == [(4, True)]             # ... and heavier than the budget
    # a single key heavier than the budget, between lighter ones
    assert both([([1, 2, 6, 6, 6, 8], [10, 10, 40, 40, 40, 10]), ([6, 9], [40, 10])], 100) == [(1, False), (6, True), (8, False)]
    # a budget smaller than any record: every key value is a tile of its own
    assert both([([1, 2, 2, 3], [10, 10, 10, 10]), ([2, 5], [10, 10])], 9) == [(1, True), (2, True), (3, True), (5, True)]
    assert both([([1, 2, 2, 3], [10, 10, 10, 10]), ([2, 5], [10, 10])], 10 ** 15) == [(1, False)]   # larger than everything
    # keys at 0 and at 2^64 - 1
    assert both([([0, 0, KMAX], [10, 10, 10]), ([0, KMAX - 1, KMAX], [10, 10, 10])], 30) == [(0, False), (KMAX - 1, False)]
    assert both([([0, 0, KMAX], [10, 10, 10]), ([0, KMAX - 1, KMAX], [10, 10, 10])], 15) == [(0, True), (KMAX - 1, False), (KMAX, True)]
    assert both([([0, KMAX], [10, 10])], 10) == [(0, False), (KMAX, False)]
    assert both([([KMAX, KMAX], [10, 10])], 10) == [(KMAX, True)]
    assert both([([3, KMAX], [10, 10]), ([KMAX], [10])], 20) == [(3, False), (KMAX, False)]


def random_runs(rng):
    style = rng.randrange(4)
    span = (1, 8, 1000, KMAX)[style]
    base = rng.choice((0, 1 << 32, KMAX - span)) if span < KMAX else 0
    runs = []
    for _ in range(rng.randrange(1, 6)):
        n = rng.choice((0, 1, 2, 7, 40))
        keys = sorted(base + rng.randrange(span + 1) for _ in range(n))
        if n and rng.random() < 0.2:
            keys[-1] = KMAX
        runs.append((keys, [rng.randrange(1, 400) for _ in range(n)]))
    return runs


def test_seeded_random_run_sets():
    rng = random.Random(20261019)
    flagged = multi = 0
    for _ in range(3000):
        runs = random_runs(rng)
        total = sum(sum(lens) for _, lens in runs)
        budget = rng.choice((1, 50, 399, 400, 1000, max(1, total // 3), max(1, total - 1), total + 1, 10 ** 12))
        got = both(runs, budget)
        flagged += any(s for _, s in got)
        multi += len(got) > 2
    assert flagged > 300 and multi > 300   # the cases reach both kinds of tile


def test_the_cutter_under_the_sanitizers(tmp_path):
    """tools/sort_tiles_sanitized.sh: simu_sort_tiles in a stand-alone program with its own main, AddressSanitizer +
    UndefinedBehaviorSanitizer, against a brute-force cut.  CPU only, no Python in that process, nothing preloaded."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "sort_tiles_sanitized.sh"), "3000", "77"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    assert "all as the brute-force cut has them" in r.stdout


# ---- refusals: before anything is forked or written, no device is touched ----
@pytest.mark.parametrize("flags,words", [(["--truth-sort"], ["--truth-sort", "--truth-bam"]),
                                         (["--truth-bam", "--truth-sort", "--world", "2"], ["--truth-sort", "--world"]),
                                         (["--truth-bam", "--truth-sort", "--gpus", "2"], ["--truth-sort", "--gpus"])])
def test_command_line_refusals(flags, words, tmp_path):
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path / "base"))
    out = str(tmp_path / "out")
    r = subprocess.run([SIMU, cfg, "--quiet", "--out", out, *flags], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr[-300:])
    assert all(w in r.stderr for w in words) and "GPU engine error" not in r.stderr
    assert not os.path.exists(out) or not os.listdir(out)


def test_in_process_refusals(tmp_path):
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path / "base"))
    out = str(tmp_path / "out")
    with pytest.raises(simuscop_amd.SimuError, match="--truth-sort needs --truth-bam"):
        simuscop_amd.run_config(cfg, seed=1, output_dir=out, quiet=1, truth_sort=1)
    with pytest.raises(simuscop_amd.SimuError, match="--truth-sort cannot be combined with --world"):
        simuscop_amd.run_config(cfg, seed=1, output_dir=out, quiet=1, truth_bam=1, truth_sort=1, shard_world=2)
    assert not os.path.exists(out) or not os.listdir(out)


def test_existing_refusal_texts_are_unchanged(tmp_path):
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path / "base"))
    r = subprocess.run([SIMU, cfg, "--quiet", "--out", str(tmp_path / "out"), "--truth-tags"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and r.stderr.strip() == "Error: --truth-tags needs --truth-bam: the tags go on the truth BAM's records"


# ---- struct order and the ABI list ----
def test_new_names_are_in_the_header_the_abi_list_and_the_structs():
    hdr = open(os.path.join(ROOT, "include", "simuscop_amd.h")).read()
    declared = set(re.findall(r"\b(sg_bamsort_[a-z_0-9]+)\s*\(", hdr))
    assert declared == {"sg_bamsort_pass", "sg_bamsort_merge", "sg_bamsort_index", "sg_bamsort_fetch"}
    assert declared <= set(simuscop_amd.ENGINE_SYMBOLS)
    assert set(re.findall(r"\b(sg_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))) <= set(simuscop_amd.ENGINE_SYMBOLS)
    eng = simuscop_amd.load_engine()
    for name in declared:
        getattr(eng, name)
    assert re.search(r"#define SG_BAMSORT_TILE %d\b" % simuscop_amd.BAMSORT_TILE, hdr)
    # the option sits behind truth_tags, the stats behind truth_xe_sum; everything from errors_bases on stays
    opts = [f[0] for f in simuscop_amd.SimuOptions._fields_]
    i = opts.index("truth_bam")
    assert opts[i:] == ["truth_bam", "truth_tags", "truth_sort", "truth_errors", "truth_variants", "truth_depth"]
    stats = [f[0] for f in simuscop_amd.SimuStats._fields_]
    i = stats.index("truth_xe_sum")
    assert stats[i:i + 6] == ["truth_xe_sum", "truth_sort_runs", "truth_sort_tiles", "truth_spool_bytes", "t_truth_sort", "errors_bases"]
    assert stats[i + 5:] == ["errors_bases", "errors_subst", "t_errors", "variant_rows", "variant_dropped", "variant_hits", "t_variants",
                             "depth_bases", "depth_rows", "t_depth"]
    # the structs of the host library and of the Python glue list their fields in one order
    shdr = open(os.path.join(ROOT, "simuscop_amd", "csrc", "host", "simulate.h")).read()
    c_opts = re.findall(r"^\s*(?:int32_t|uint64_t|const char\*|void\*)\s+(\w+);", shdr[shdr.index("typedef struct simu_options"):shdr.index("} simu_options;")], re.M)
    assert [o for o in opts if o.startswith("truth_")] == [o for o in c_opts if o.startswith("truth_")]
    flat = []
    for chunk in re.sub(r"//[^\n]*", "", shdr[shdr.index("typedef struct simu_stats {") + 27:shdr.index("} simu_stats;")]).split(";"):
        names = re.sub(r"^\s*(uint64_t|double|float|int32_t|uint32_t)\s+", "", chunk.strip())
        flat += [re.sub(r"\[\d+\]", "", n.strip()) for n in names.split(",") if n.strip()]
    assert flat == stats
    assert "simu_sort_tiles(" in shdr
    assert callable(simuscop_amd.bamsort_merge) and callable(simuscop_amd.sort_tiles)
    assert all(callable(getattr(simuscop_amd.Session, n)) for n in ("bamsort_pass", "bamsort_index", "bamsort_fetch"))
    assert simuscop_amd.default_options(truth_sort=1).truth_sort == 1 and simuscop_amd.default_options().truth_sort == 0
    # the --stats line: the new keys form the last group
    main = open(os.path.join(ROOT, "simuscop_amd", "csrc", "host", "main.cpp")).read()
    assert 'errors_s=%.3f | "\n            "truth_sort_runs=%llu truth_sort_tiles=%llu truth_spool_bytes=%llu truth_sort_s=%.3f\\n"' in main
