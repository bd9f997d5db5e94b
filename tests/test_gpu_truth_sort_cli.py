"""`simuReads --truth-bam --truth-sort` on the MI355X against a model made of the verified unsorted output: the records
of `--truth-bam`'s file in file order, `sorted` (stable) by (u32 refID, u32 POS), under the same header with
SO:coordinate.  Every variant of a case -- one run per piece or many (SIMU_PIECE_SLOTS), one tile, a handful or one per
key value (SIMU_SORT_TILE_BYTES) -- must give that file byte for byte once inflated, leave the FASTQ files and the counts
alone, report the runs and tiles it was forced into, and leave no spool behind."""
import os
import re
import struct
import subprocess

import pytest

import bam_util as B
import cases
import profile_shapes as PS
import simuscop_amd.build as build
import truth_util as U
from profile_shapes import Shape

pytestmark = pytest.mark.gpu

SIMU = os.path.join(build.LIBDIR, "simuReads")
SEED = (cases.FAKE_SEC << 32) | cases.FAKE_NSEC
MANY = {"SIMU_PIECE_SLOTS": "1500"}


def long_insertion_case(wd):
    """No shipped case has an unmapped read (a read without an M base).  A homozygous insertion longer than a fragment
    gives both kinds: pairs that lie inside it (unplaced, -1 / -1) and pairs across its edge (one mate unmapped, placed at
    the other)."""
    import random
    prof = os.path.join(cases.TESTDATA, cases.PROFILES["hs2000"])
    cfg, _, _ = U.acgt_case(wd, prof, "PE", variants=False, coverage=20, lengths=(40000, 5000))
    var = os.path.join(wd, "variations.txt")
    cases._write(var, ["i\tv\tchr3\t20000\t%s\thomo" % "".join(random.Random(7).choices("ACGT", k=1500))])
    with open(cfg, "a") as f:
        f.write("variation = %s\n" % var)
    return cfg


CASES = {
    "k3_b53_PE_fast_kernel": lambda wd: PS.build_shape_case(Shape(3, 53), wd, "PE"),
    "k3_b52_SE_fast_kernel": lambda wd: PS.build_shape_case(Shape(3, 52), wd, "SE"),
    "wgs_pe_variants": lambda wd: cases.build_case("wgs_pe_variants", wd),
    "wes_pe_targets": lambda wd: cases.build_case("wes_pe_targets", wd),
    "tumor_se_mixture": lambda wd: cases.build_case("tumor_se_mixture", wd),
    "long_insertion_pe": long_insertion_case,
}


def simu(cfg, out, *flags, env=None):
    r = subprocess.run([SIMU, cfg, "--seed", str(SEED), "--out", out, "--quiet", "--stats", *flags], capture_output=True, text=True,
                       timeout=900, env=dict(os.environ, SIMU_TRACE_PIECES="1", **(env or {})))
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def stat(stderr, key):
    return int(re.search(r"\b" + key + r"=(-?\d+)", stderr).group(1))


def pieces_with_reads(stderr):
    return sum(1 for n in re.findall(r"^\[piece\] .* (\d+) fragments$", stderr, re.M) if int(n))


def split_file(path):
    """(bytes in front of the records, [record bytes]) of an inflated BAM file."""
    d = U.inflate_members(open(path, "rb").read())
    _, recs = B.parse_stream(d)
    first = recs[0][0] if recs else len(d)
    assert b"".join(r for _, r in recs) == d[first:]
    return d[:first], [r for _, r in recs]


def key_of(rec):
    return struct.unpack_from("<I", rec, 4)[0] << 32 | struct.unpack_from("<I", rec, 8)[0]


def model_file(head, recs):
    """The sorted file's inflated bytes: the unsorted file's header with the sort order renamed, its records sorted stably."""
    l_text = struct.unpack_from("<i", head, 4)[0]
    text = head[8:8 + l_text]
    assert text.startswith(b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n")
    text2 = b"@HD\tVN:1.6\tSO:coordinate\n" + text[len(b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n"):]
    return head[:4] + struct.pack("<i", len(text2)) + text2 + head[8 + l_text:] + b"".join(sorted(recs, key=key_of))


def greedy_tiles(recs, budget):
    """Tiles of a stem under `budget`: whole key values while they fit; a key value that alone does not fit is one tile."""
    per_key = {}
    for r in recs:
        per_key[key_of(r)] = per_key.get(key_of(r), 0) + len(r)
    tiles, cur = 0, None
    for k in sorted(per_key):
        b = per_key[k]
        if b > budget:
            tiles += 1 + (cur is not None)
            cur = None
        elif cur is None or cur + b > budget:
            tiles += cur is not None
            cur = b
        else:
            cur += b
    return tiles + (cur is not None)


def stems(d):
    return sorted(x[:-len(".truth.bam")] for x in os.listdir(d) if x.endswith(".truth.bam"))


_base = {}


@pytest.fixture
def base(request, tmp_path_factory):
    """Per case, once: its configuration, the unsorted run (the model's source) and the same with many pieces."""
    name = request.param
    if name not in _base:
        wd = str(tmp_path_factory.mktemp(name))
        cfg = CASES[name](wd)
        tags = ["--truth-tags"] if name == "wgs_pe_variants" else []
        plain, many = os.path.join(wd, "unsorted"), os.path.join(wd, "unsorted_many")
        err = simu(cfg, plain, "--truth-bam", *tags)
        err_many = simu(cfg, many, "--truth-bam", *tags, env=MANY)
        files = {}
        for stem in stems(plain):
            files[stem] = split_file(os.path.join(plain, stem + ".truth.bam"))
            # many pieces make the same unsorted file: pass order then record order is one order for both
            assert split_file(os.path.join(many, stem + ".truth.bam")) == files[stem]
        # (the case made here has two short contigs, one segment each: its pieces cannot be cut smaller)
        assert files and pieces_with_reads(err_many) > pieces_with_reads(err) - (name == "long_insertion_pe") > 0
        _base[name] = dict(name=name, wd=wd, cfg=cfg, tags=tags, plain=plain, err=err, files=files, runs_many=pieces_with_reads(err_many),
                           runs_plain=pieces_with_reads(err))
    return _base[name]


def run_sorted(b, label, env, flags=()):
    out = os.path.join(b["wd"], label)
    err = simu(b["cfg"], out, "--truth-bam", "--truth-sort", *b["tags"], *flags, env=env)
    assert stems(out) == sorted(b["files"])
    for stem, (head, recs) in b["files"].items():
        path = os.path.join(out, stem + ".truth.bam")
        d = U.inflate_members(open(path, "rb").read())
        assert b"@HD\tVN:1.6\tSO:coordinate\n@SQ" in d[:200]
        assert d == model_file(head, recs), (label, stem)
    # the FASTQ files are those of the run without the option; no spool is left behind
    others = sorted(x for x in os.listdir(b["plain"]) if not x.endswith(".truth.bam"))
    assert others and others == sorted(x for x in os.listdir(out) if not x.endswith(".truth.bam"))
    for f in others:
        assert open(os.path.join(out, f), "rb").read() == open(os.path.join(b["plain"], f), "rb").read(), f
    assert not [x for x in os.listdir(out) if x.endswith(".runs.tmp")]
    for key in ("reads", "truth_records", "truth_unmapped", "truth_bytes", "truth_tag_bytes", "truth_nm_sum", "truth_xe_sum"):
        assert stat(err, key) == stat(b["err"], key), key
    assert stat(err, "truth_spool_bytes") == stat(err, "truth_bytes") == sum(len(r) for _, recs in b["files"].values() for r in recs)
    assert 0 < stat(err, "truth_bgzf_bytes") < stat(err, "truth_bytes")
    return err


ALL = list(CASES)


@pytest.mark.parametrize("base", ALL, indirect=True)
def test_one_run_per_piece_one_tile_per_stem(base):
    err = run_sorted(base, "sorted", None)
    assert stat(err, "truth_sort_runs") == base["runs_plain"] and stat(err, "truth_sort_tiles") == len(base["files"])
    assert stat(base["err"], "truth_sort_runs") == stat(base["err"], "truth_sort_tiles") == stat(base["err"], "truth_spool_bytes") == 0


@pytest.mark.parametrize("base", ALL, indirect=True)
def test_many_runs(base):
    err = run_sorted(base, "sorted_many", MANY)
    assert stat(err, "truth_sort_runs") == base["runs_many"] > 1 and stat(err, "truth_sort_tiles") == len(base["files"])


@pytest.mark.parametrize("base", ALL, indirect=True)
def test_many_runs_a_handful_of_tiles(base):
    budget = max(sum(len(r) for r in recs) for _, recs in base["files"].values()) // 4
    want = sum(greedy_tiles(recs, budget) for _, recs in base["files"].values())
    assert 4 <= want <= 8 * len(base["files"])
    err = run_sorted(base, "sorted_tiles", dict(MANY, SIMU_SORT_TILE_BYTES=str(budget)))
    assert stat(err, "truth_sort_runs") == base["runs_many"] and stat(err, "truth_sort_tiles") == want


@pytest.mark.parametrize("base", ALL, indirect=True)
def test_many_runs_a_budget_below_one_record(base):
    want = sum(len({key_of(r) for r in recs}) for _, recs in base["files"].values())   # every tile is a single key
    err = run_sorted(base, "sorted_single", dict(MANY, SIMU_SORT_TILE_BYTES="20"))
    assert stat(err, "truth_sort_runs") == base["runs_many"] and stat(err, "truth_sort_tiles") == want


@pytest.mark.parametrize("base", ALL, indirect=True)
def test_the_inputs_have_what_the_order_is_about(base):
    """Tied keys in every case; in the case made for it unmapped records placed at their mates and unplaced ones; several
    stems whose chromosomes recur per population in the mixture."""
    placed = unplaced = ties = 0
    for _, recs in base["files"].values():
        keys = [key_of(r) for r in recs]
        ties += len(keys) - len(set(keys))
        for r in recs:
            if struct.unpack_from("<H", r, 18)[0] & 4:
                unplaced += key_of(r) == 2 ** 64 - 1
                placed += key_of(r) != 2 ** 64 - 1
    print("ties", ties, "unmapped at the mate", placed, "unplaced", unplaced)
    assert ties > 0
    if base["name"] == "long_insertion_pe":
        assert placed > 0 and unplaced > 0, (placed, unplaced)
    if base["name"] == "tumor_se_mixture":
        assert len(base["files"]) > 1


def test_no_write_counts_only(tmp_path):
    cfg = CASES["k3_b53_PE_fast_kernel"](str(tmp_path))
    out = str(tmp_path / "out")
    plain = simu(cfg, out, "--truth-bam", "--no-write")
    err = simu(cfg, out, "--truth-bam", "--truth-sort", "--no-write")
    for key in ("truth_records", "truth_unmapped", "truth_bytes"):
        assert stat(err, key) == stat(plain, key), key
    assert stat(err, "truth_records") > 1000 and stat(err, "truth_bytes") > 100000
    assert stat(err, "truth_sort_runs") == stat(err, "truth_sort_tiles") == stat(err, "truth_spool_bytes") == stat(err, "truth_bgzf_bytes") == 0
    assert not os.path.exists(out) or not os.listdir(out)
