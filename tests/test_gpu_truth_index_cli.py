"""`simuReads --truth-bam --truth-sort --truth-index` on the MI355X against bai_model: the .bai beside every sorted BAM is
byte for byte the model's index of that file's bytes, the BAM is the file the run without the option writes, the counts in
the index are the records', and a standard reader finds through the written index exactly the records a brute-force
filter finds -- with one run per piece or many (SIMU_PIECE_SLOTS), one tile, a handful, or one per key value
(SIMU_SORT_TILE_BYTES; the last goes through the pass-through path and its skipped fronts)."""
import os
import random
import re
import subprocess

import pytest

import bai_model as M
import cases
import simuscop_amd.build as build
import truth_util as U

pytestmark = pytest.mark.gpu

SIMU = os.path.join(build.LIBDIR, "simuReads")
SEED = (cases.FAKE_SEC << 32) | cases.FAKE_NSEC
MANY = {"SIMU_PIECE_SLOTS": "1500"}


def long_insertion_case(wd):
    """A homozygous insertion longer than a fragment: pairs inside it are unplaced (-1 / -1), pairs across its edge have
    one mate unmapped and placed at the other."""
    prof = os.path.join(cases.TESTDATA, cases.PROFILES["hs2000"])
    cfg, _, _ = U.acgt_case(wd, prof, "PE", variants=False, coverage=20, lengths=(40000, 5000))
    var = os.path.join(wd, "variations.txt")
    cases._write(var, ["i\tv\tchr3\t20000\t%s\thomo" % "".join(random.Random(7).choices("ACGT", k=1500))])
    with open(cfg, "a") as f:
        f.write("variation = %s\n" % var)
    return cfg


CASES = {
    "wgs_pe_variants": lambda wd: cases.build_case("wgs_pe_variants", wd),
    "wes_pe_targets": lambda wd: cases.build_case("wes_pe_targets", wd),
    "tumor_se_mixture": lambda wd: cases.build_case("tumor_se_mixture", wd),
    "long_insertion_pe": long_insertion_case,
}
VARIANTS = ("one_tile", "many_runs", "a_handful_of_tiles", "one_tile_per_key")


def simu(cfg, out, *flags, env=None, want=0):
    r = subprocess.run([SIMU, cfg, "--seed", str(SEED), "--out", out, "--quiet", "--stats", *flags], capture_output=True, text=True,
                       timeout=900, env=dict(os.environ, **(env or {})))
    assert r.returncode == want, r.stderr[-2000:]
    return r.stderr


def stat(stderr, key):
    return int(re.search(r"\b" + key + r"=(-?\d+)", stderr).group(1))


def files(d, suffix):
    return sorted(x for x in os.listdir(d) if x.endswith(suffix))


_base = {}


def base_of(name, tmp_path_factory):
    """Per case, once: its configuration and the budget that cuts its largest stem into a handful of tiles."""
    if name not in _base:
        wd = str(tmp_path_factory.mktemp(name))
        cfg = CASES[name](wd)
        tags = ["--truth-tags"] if name == "wgs_pe_variants" else []
        out = os.path.join(wd, "size")
        simu(cfg, out, "--truth-bam", "--truth-sort", *tags)
        largest = max(sum(len(r["raw"]) for r in M.file_records(open(os.path.join(out, f), "rb").read())[1]) for f in files(out, ".truth.bam"))
        _base[name] = dict(wd=wd, cfg=cfg, tags=tags, envs={"one_tile": None, "many_runs": MANY,
                                                            "a_handful_of_tiles": dict(MANY, SIMU_SORT_TILE_BYTES=str(largest // 4)),
                                                            "one_tile_per_key": dict(MANY, SIMU_SORT_TILE_BYTES="20")})
    return _base[name]


def regions(name, refs, recs, rng):
    """A dozen regions: per contig (two at most) its first base, its last base, all of it, a stretch across a 2^14
    boundary, the inside of a 2^14 window no read touches where there is one; where the reads are thickest; the places of
    the unmapped reads that lie at their mates."""
    out = []
    used = sorted({r["ref"] for r in recs if r["ref"] >= 0})
    for ref in used[:1] + used[-1:]:
        ln = refs[ref][1]
        out += [(ref, 0, 1), (ref, ln - 1, ln), (ref, 0, ln)]
        if ln > 16390:
            out.append((ref, 16380, 16390))
        touched = set()
        for r in recs:
            if r["ref"] == ref:
                touched.update(range(r["beg"] >> 14, ((r["stop"] - 1) >> 14) + 1))
        mine = [r for r in recs if r["ref"] == ref]
        if mine[0]["beg"] > 0:                                        # in front of the contig's first read: nothing
            out.append((ref, 0, mine[0]["beg"]))
        if max(r["stop"] for r in mine) < ln:                         # ... and behind its last
            out.append((ref, max(r["stop"] for r in mine), ln))
        free = [w for w in range((ln + 16383) >> 14) if w not in touched]
        if free:
            w = rng.choice(free)
            out.append((ref, (w << 14) + 5, min(ln, (w << 14) + 900)))
    mid = recs[len(recs) // 3]
    if mid["ref"] >= 0:
        out.append((mid["ref"], mid["beg"], mid["beg"] + 1))
    for r in [r for r in recs if r["unmapped"] and r["ref"] >= 0][:3]:
        out.append((r["ref"], r["beg"], r["beg"] + 1))
    if name == "long_insertion_pe":                                   # the insertion site
        out.append((max(used), 19990, 20010))
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CASES))
def test_index_of_a_sorted_truth_bam(name, variant, tmp_path_factory):
    b = base_of(name, tmp_path_factory)
    env = b["envs"][variant]
    without, out = os.path.join(b["wd"], variant + "_without"), os.path.join(b["wd"], variant)
    err0 = simu(b["cfg"], without, "--truth-bam", "--truth-sort", *b["tags"], env=env)
    err = simu(b["cfg"], out, "--truth-bam", "--truth-sort", "--truth-index", *b["tags"], env=env)
    bams = files(out, ".truth.bam")
    assert bams and bams == files(without, ".truth.bam") and files(out, ".bai") == [f + ".bai" for f in bams]
    assert not files(out, ".runs.tmp") and not files(without, ".bai")
    assert sorted(os.listdir(out)) == sorted(os.listdir(without) + files(out, ".bai"))
    for key in ("reads", "truth_records", "truth_unmapped", "truth_bytes", "truth_bgzf_bytes", "truth_sort_runs", "truth_sort_tiles", "truth_spool_bytes"):
        assert stat(err, key) == stat(err0, key), key
    assert stat(err0, "bai_bins") == stat(err0, "bai_chunks") == stat(err0, "bai_bytes") == 0
    if variant == "one_tile_per_key":
        assert stat(err, "truth_sort_tiles") > 20 * len(bams)
    elif variant == "a_handful_of_tiles":
        assert stat(err, "truth_sort_tiles") >= 4
    rng = random.Random(len(name))
    n_records = n_unmapped = bai_bytes = bins = chunks = hits = misses = placed_back = 0
    for f in bams:
        bam = open(os.path.join(out, f), "rb").read()
        assert bam == open(os.path.join(without, f), "rb").read(), f               # the index changes nothing about the BAM
        bai = open(os.path.join(out, f + ".bai"), "rb").read()
        refs, recs = M.file_records(bam)
        want = M.serialise(*M.index(recs, len(refs)))
        assert bai == want, (f, len(bai), len(want))
        bai_bytes += len(bai)
        parsed = M.parse(bai)
        bins += sum(len(R["bins"]) for R in parsed[0])
        chunks += sum(len(c) for R in parsed[0] for c in R["bins"].values())
        # the counts in the index against the records
        assert parsed[1] == sum(r["ref"] < 0 for r in recs)
        for ref, R in enumerate(parsed[0]):
            mine = [r for r in recs if r["ref"] == ref]
            assert (R["pseudo"] is None) == (not mine)
            if mine:
                assert R["pseudo"][1] == [sum(not r["unmapped"] for r in mine), sum(r["unmapped"] for r in mine)]
        n_records += len(recs)
        n_unmapped += sum(r["unmapped"] for r in recs)
        # the record's own bin field is the bin an indexer computes
        wrong = [(r["ref"], r["beg"], r["stop"], r["bin"], r["bin_field"]) for r in recs if r["ref"] >= 0 and r["bin"] != r["bin_field"]]
        assert not wrong, wrong[:5]
        # a reader's answers through the written index
        for ref, beg, end in regions(name, refs, recs, rng):
            brute = [r["raw"] for r in recs if r["ref"] == ref and r["beg"] < end and r["stop"] > beg]
            got = M.query(parsed, bam, ref, beg, end)
            assert got == brute, (f, ref, beg, end, len(got), len(brute))
            hits += bool(brute)
            misses += not brute
            placed_back += sum(1 for r in recs if r["ref"] == ref and r["unmapped"] and r["beg"] < end and r["stop"] > beg)
    assert hits > 0 and misses > 0, (hits, misses)
    assert (n_records, n_unmapped) == (stat(err, "truth_records"), stat(err, "truth_unmapped"))
    assert (bai_bytes, bins, chunks) == (stat(err, "bai_bytes"), stat(err, "bai_bins"), stat(err, "bai_chunks"))
    if name == "long_insertion_pe":
        assert placed_back > 0 and stat(err, "truth_unmapped") > placed_back                  # placed at the mate, and unplaced ones


def test_no_write_writes_no_index_and_a_refused_run_leaves_nothing(tmp_path):
    cfg = CASES["wgs_pe_variants"](str(tmp_path))
    out = str(tmp_path / "out")
    err = simu(cfg, out, "--truth-bam", "--truth-sort", "--truth-index", "--no-write")
    assert stat(err, "truth_records") > 1000 and stat(err, "bai_bytes") == stat(err, "bai_chunks") == 0
    assert not os.path.exists(out) or not os.listdir(out)
    err = simu(cfg, out, "--truth-bam", "--truth-index", want=1)
    assert "--truth-index needs --truth-sort" in err
    assert not os.path.exists(out) or not os.listdir(out)
