"""`simuReads --truth-depth` without a GPU: the bedGraph rows simu_depth_format makes of the device's runs and bin sums
against a formatter written here from the file's definition, the command lines that are refused before the engine
exists, and the new calls' place in the ABI list."""
import os
import re
import subprocess

import pytest

import cases
import simuscop_amd
import simuscop_amd.build as build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMU = os.path.join(build.LIBDIR, "simuReads")


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(SIMU):
        build.build_all()


def model_rows(name, ln, bin_width, data):
    """The file's definition: bin 1 -- runs (start, depth) reach to the next start, equal neighbours are one row, the value
    a decimal integer; bin > 1 -- the fixed grid, unmerged, '%.4f' of sum / the row's own width."""
    out = []
    if bin_width == 1:
        merged = []
        for start, depth in data:
            if not merged or merged[-1][1] != depth:
                merged.append((start, depth))
        for i, (start, depth) in enumerate(merged):
            end = merged[i + 1][0] if i + 1 < len(merged) else ln
            out.append("%s\t%d\t%d\t%d\n" % (name, start, end, depth))
    else:
        for k, s in enumerate(data):
            a, b = k * bin_width, min(ln, (k + 1) * bin_width)
            out.append("%s\t%d\t%d\t%s\n" % (name, a, b, "%.4f" % (s / (b - a))))
    return "".join(out).encode()


RUN_CASES = {
    "one_run_over_the_contig": ("chr1", 1000, [(0, 0)]),
    "one_base": ("c", 1, [(0, 7)]),
    "steps": ("chr20", 500, [(0, 0), (10, 1), (11, 2), (12, 1), (499, 0)]),
    "depth_above_2_31": ("chrX", 3000, [(0, 2 ** 31 + 5), (100, 2 ** 32 - 1), (2999, 3)]),
    "equal_neighbours_merge": ("m", 90, [(0, 4), (30, 4), (60, 5), (70, 5), (80, 4)]),
    "name_with_dots": ("HLA-A*01:01.v2", 20, [(0, 1), (5, 0)]),
}


@pytest.mark.parametrize("case", sorted(RUN_CASES))
def test_runs_format(case):
    name, ln, runs = RUN_CASES[case]
    got = simuscop_amd.depth_format(name, ln, 1, runs)
    assert got == model_rows(name, ln, 1, runs)
    rows = [r.split(b"\t") for r in got.splitlines()]
    assert int(rows[0][1]) == 0 and int(rows[-1][2]) == ln
    assert all(a[2] == b[1] and a[3] != b[3] for a, b in zip(rows, rows[1:]))     # tiling; no two equal neighbours


BIN_CASES = {
    "short_last_bin": ("chr3", 1000, 300, [300, 600, 1, 7]),                 # the last bin is 100 wide: 7 / 100
    "bin_larger_than_the_contig": ("chr8", 777, 1000000, [123456]),
    "bin_equal_to_the_contig": ("chr8", 777, 777, [777 * 3]),
    "bin_2_odd_length": ("o", 7, 2, [0, 1, 2, 1]),
    # means that need rounding at the fourth decimal: thirds, sevenths, .00005 ties as a double holds them, large sums
    "rounding": ("r", 7 * 12 + 3, 7, [1, 2, 3, 4, 5, 6, 10 ** 15 + 1, 22, 2 ** 40 + 3, 123457, 7 * 10000 + 3, 50, 2]),
    "rounding_ties": ("t", 8 * 20000, 20000, [1, 3, 5, 7, 9, 20001, 10 ** 12 + 1, 2 ** 52 + 12345]),
    "zeros": ("z", 40, 10, [0, 0, 0, 0]),
}


@pytest.mark.parametrize("case", sorted(BIN_CASES))
def test_bins_format(case):
    name, ln, bin_width, sums = BIN_CASES[case]
    assert len(sums) == -(-ln // bin_width)
    got = simuscop_amd.depth_format(name, ln, bin_width, sums)
    assert got == model_rows(name, ln, bin_width, sums)
    rows = [r.split(b"\t") for r in got.splitlines()]
    assert len(rows) == len(sums) and int(rows[-1][2]) == ln
    assert all(int(r[1]) == k * bin_width for k, r in enumerate(rows))             # on the grid, unmerged
    assert all(re.fullmatch(rb"\d+\.\d{4}", r[3]) for r in rows)


def test_a_contig_without_bases_gives_no_row():
    assert simuscop_amd.depth_format("empty", 0, 1, []) == b""
    assert simuscop_amd.depth_format("empty", 0, 50, []) == b""


def test_data_that_is_no_contig_is_refused():
    for ln, bin_width, data in ((100, 1, [(5, 1)]),            # the first run does not start at 0
                                (100, 1, [(0, 1), (100, 2)]),   # a run starts behind the last base
                                (100, 1, [(0, 1), (50, 2), (50, 3)]),
                                (100, 1, []),
                                (100, 10, [1] * 9),
                                (100, 10, [1] * 11)):
        with pytest.raises(simuscop_amd.SimuError):
            simuscop_amd.depth_format("x", ln, bin_width, data)


REFUSED = {
    "no_value": ["--truth-depth"],
    "zero": ["--truth-depth", "0"],
    "negative": ["--truth-depth", "-3"],
    "not_a_number": ["--truth-depth", "x"],
    "number_with_a_tail": ["--truth-depth", "5k"],
    "world_2": ["--truth-depth", "5", "--world", "2"],
    "gpus_2": ["--truth-depth", "5", "--gpus", "2"],
    "host_haplotypes": ["--truth-depth", "5", "--host-haplotypes"],
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_cli_refuses_before_the_engine_exists(name, tmp_path):
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path / "base"))
    out = str(tmp_path / "out")
    r = subprocess.run([SIMU, cfg, "--quiet", "--out", out, *REFUSED[name]], capture_output=True, text=True, timeout=120)
    assert r.returncode not in (0, None) and r.returncode > 0, (r.returncode, r.stderr[-300:])
    assert "--truth-depth" in r.stderr, r.stderr[-300:]
    assert "GPU engine error" not in r.stderr
    assert not os.path.exists(out) or not os.listdir(out)


def test_in_process_refusals(tmp_path):
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path / "base"))
    for kw in (dict(truth_depth=5, host_haplotypes=1), dict(truth_depth=5, shard_world=2), dict(truth_depth=-1)):
        out = str(tmp_path / "out")
        with pytest.raises(simuscop_amd.SimuError, match="--truth-depth"):
            simuscop_amd.run_config(cfg, seed=1, output_dir=out, quiet=1, **kw)
        assert not os.path.exists(out) or not os.listdir(out)


def test_new_calls_are_in_the_abi_list():
    hdr = open(os.path.join(ROOT, "include", "simuscop_amd.h")).read()
    declared = set(re.findall(r"\b(sg_depth_[a-z_0-9]+)\s*\(", hdr))
    assert declared == {"sg_depth_begin", "sg_depth_add", "sg_depth_add_spans", "sg_depth_bins", "sg_depth_runs", "sg_depth_fetch",
                        "sg_depth_reset", "sg_depth_info", "sg_depth_end"}
    assert declared <= set(simuscop_amd.ENGINE_SYMBOLS)
    assert simuscop_amd.SimuOptions._fields_[-1][0] == "truth_depth"
    assert [f[0] for f in simuscop_amd.SimuStats._fields_[-3:]] == ["depth_bases", "depth_rows", "t_depth"]
