"""The files of a stem as the driver opens and closes them: FASTQ, truth BAM, its spool, then the summed truth outputs.
Which "can not open" message a run ends with is that order, and what an error leaves behind is how each owner closes:
the truth BAM with its end-of-file block, the spool removed.  Every case is one command line on a genome of 25 kbp with a
few hundred reads; a path is made unopenable by putting a directory there."""
import os
import subprocess

import pytest

import bam_util as B
import cases
import simuscop_amd.build as build
import truth_util as U

pytestmark = pytest.mark.gpu

SIMU = os.path.join(build.LIBDIR, "simuReads")
SEED = (cases.FAKE_SEC << 32) | cases.FAKE_NSEC
FLAGS = ("--truth-bam", "--truth-sort", "--truth-depth", "1")
XTEN = os.path.join(cases.TESTDATA, cases.PROFILES["xten"])


def simu(cfg, out, *flags):
    return subprocess.run([SIMU, cfg, "--seed", str(SEED), "--out", out, "--quiet", *FLAGS, *flags], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def cfg(tmp_path_factory):
    return U.acgt_case(str(tmp_path_factory.mktemp("driver_files")), XTEN, "PE", coverage=3, lengths=(20000, 5000))[0]


def obstructed(cfg, tmp_path, name):
    """The run with a directory at out/<name>: its exit status, its stderr, the path, and a test of what else is there."""
    out = str(tmp_path / "out")
    os.makedirs(os.path.join(out, name))
    r = simu(cfg, out)
    rest = sorted(x for x in os.listdir(out) if x != name)
    return r.returncode, r.stderr, os.path.join(out, name), out, rest


def header_alone(path):
    """The truth BAM holds its header, no record, and the end-of-file block (once, at the end)."""
    _, refs, recs, _ = U.read_truth_bam(path)
    return [n for n, _ in refs] == [b"chr3", b"chr8"] and recs == []


def test_fastq_is_opened_first(cfg, tmp_path):
    rc, err, path, out, rest = obstructed(cfg, tmp_path, "v_2.fq")
    assert rc == 255 and err.rstrip("\n").endswith("Error: can not open fastq file to save results:\n" + path), (rc, err)
    assert rest == ["v_1.fq"]


def test_then_the_truth_bam(cfg, tmp_path):
    rc, err, path, out, rest = obstructed(cfg, tmp_path, "v.truth.bam")
    assert rc == 255 and err.rstrip("\n").endswith("Error: can not open BAM file to save the true alignments:\n" + path), (rc, err)
    assert rest == ["v_1.fq", "v_2.fq"]


def test_then_its_spool(cfg, tmp_path):
    rc, err, path, out, rest = obstructed(cfg, tmp_path, "v.truth.bam.runs.tmp")
    assert rc == 255 and err.rstrip("\n").endswith("Error: can not open the spool file of the sorted truth BAM:\n" + path), (rc, err)
    assert rest == ["v.truth.bam", "v_1.fq", "v_2.fq"] and header_alone(os.path.join(out, "v.truth.bam"))


def test_then_the_summed_outputs(cfg, tmp_path):
    rc, err, path, out, rest = obstructed(cfg, tmp_path, "v.truth.depth.bedgraph")
    assert rc == 255 and err.rstrip("\n").endswith("Error: can not open bedGraph file to save the true depth:\n" + path), (rc, err)
    assert rest == ["v.truth.bam", "v_1.fq", "v_2.fq"] and header_alone(os.path.join(out, "v.truth.bam"))   # (the spool is gone)


def test_nothing_obstructed(cfg, tmp_path):
    out = str(tmp_path / "out")
    r = simu(cfg, out)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["v.truth.bam", "v.truth.depth.bedgraph", "v_1.fq", "v_2.fq"]
    reads = len(U.read_fastq(os.path.join(out, "v_1.fq"))) + len(U.read_fastq(os.path.join(out, "v_2.fq")))
    assert 200 < reads < 2000 and len(U.read_truth_bam(os.path.join(out, "v.truth.bam"))[2]) == reads


def test_two_stems_each_file_closed_once(tmp_path):
    """Two abundance rows with --gzip: six BGZF files, each ending with the end-of-file block and holding no other empty
    member (inflate_members), each stem's files its own.  The first stem's are byte for byte those of a run of its row
    alone.  The second stem's batches are numbered behind the first's and the numbers address the draws, so a run of its
    row alone samples other reads: there the counts are compared, which follow from the weights alone."""
    wd = str(tmp_path)
    _, fa, _ = U.acgt_case(wd, XTEN, "PE", lengths=(20000, 5000))
    rows = ["1.0\t0", "0.4\t0.6"]
    stems = ["a_1.000+b_0.000", "a_0.400+b_0.600"]
    got = {}
    for tag, use in (("both", rows), ("first", rows[:1]), ("second", rows[1:])):
        cases._write(os.path.join(wd, tag + ".abundance.txt"), use)
        cfg = os.path.join(wd, tag + ".txt")
        cases._config(cfg, ref=fa, profile=XTEN, name="a, b", abundance=os.path.join(wd, tag + ".abundance.txt"), output=os.path.join(wd, "out"),
                      layout="PE", threads=1, verbose=0, coverage=3, insertSize=400)
        out = os.path.join(wd, tag)
        r = simu(cfg, out, "--gzip")
        assert r.returncode == 0, r.stderr[-2000:]
        got[tag] = {x: open(os.path.join(out, x), "rb").read() for x in sorted(os.listdir(out))}
    want = sorted(s + e for s in stems for e in ("_1.fq.gz", "_2.fq.gz", ".truth.bam", ".truth.depth.bedgraph"))
    assert sorted(got["both"]) == want and sorted(got["first"]) == want[4:] and sorted(got["second"]) == want[:4]
    text = {tag: {x: U.inflate_members(d) for x, d in files.items() if not x.endswith(".bedgraph")} for tag, files in got.items()}
    assert all(len(t) > 10000 for t in text["both"].values())
    for x in want[4:]:
        assert got["both"][x] == got["first"][x], x
    for x in want[:4]:
        if x.endswith(".fq.gz"):
            assert text["both"][x].count(b"\n") == text["second"][x].count(b"\n") > 400, x
        elif x.endswith(".bam"):
            assert len(B.parse_stream(text["both"][x])[1]) == len(B.parse_stream(text["second"][x])[1]) > 200, x
    assert text["both"][stems[0] + "_1.fq.gz"] != text["both"][stems[1] + "_1.fq.gz"]
