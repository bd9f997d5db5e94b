"""`simuReads --truth-bam --truth-tags` as a command line on the MI355X: the file's records are those of a --truth-bam run
with tags behind them, NM and MD as the model (tests/tags_model.py) has them from the record and the FASTA, XE adding up
to the true error counts of the same run (read by read XE is checked through a Session, test_gpu_truth_tag_records.py);
the FASTQ files do not change; pieces, ranks and --no-write; the refusal; and the project's trainer reads the tagged file."""
import hashlib
import os

import pytest

import bam_util as B
import cases
import errors_model as EM
import tags_model as TM
import tags_util as TU
import test_gpu_truth_bam as TB
import truth_util as U

pytestmark = pytest.mark.gpu


def raw_records_of_file(path, want_eof=True):
    d = U.inflate_members(open(path, "rb").read(), want_eof)
    return d, [r for _, r in B.parse_stream(d)[1]]


def md5s(d):
    return {f: hashlib.md5(open(os.path.join(d, f), "rb").read()).hexdigest() for f in sorted(os.listdir(d)) if f.endswith(".fq")}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One untagged and one tagged run of a case with variants (chains that differ from the reference), the tagged one
    with --truth-errors beside it."""
    wd = str(tmp_path_factory.mktemp("cli"))
    cfg = cases.build_case("wgs_pe_variants", wd)
    plain, tagged = os.path.join(wd, "plain"), os.path.join(wd, "tagged")
    rp = TB.simu(cfg, plain, "--truth-bam")
    rt = TB.simu(cfg, tagged, "--truth-bam", "--truth-tags", "--truth-errors")
    (stem,) = TB.stems(plain)
    return dict(wd=wd, cfg=cfg, plain=plain, tagged=tagged, stem=stem, err_plain=rp.stderr, err_tagged=rt.stderr)


def test_the_file_is_the_untagged_file_plus_the_tags(runs):
    stem = runs["stem"]
    d0, plain = raw_records_of_file(os.path.join(runs["plain"], stem + ".truth.bam"))
    d1, tagged = raw_records_of_file(os.path.join(runs["tagged"], stem + ".truth.bam"))
    hdr_end = B.parse_stream(d0)[1][0][0]
    assert d0[:hdr_end] == d1[:hdr_end] and len(plain) == len(tagged) > 1000
    assert md5s(runs["plain"]) == md5s(runs["tagged"]) and md5s(runs["plain"])
    fastas = TU.fasta_sequences(TU.config_value(runs["cfg"], "ref"))
    nm_sum = xe_sum = tag_bytes = with_caret = with_mismatch = 0
    for p, t in zip(plain, tagged):
        front, aux = TU.split_record(t)
        assert front == p                                              # the record but for block_size and the tags
        tags = TM.parse_tags(aux)
        rec = U.parse_record(p)
        if rec["ops"]:
            nm, md = TM.nm_md(rec["ops"], rec["seq"], fastas[rec["rid"]], rec["pos"])
            assert list(tags) == ["NM", "XE", "MD"] and (tags["NM"], tags["MD"]) == (nm, md), (rec, tags, nm, md)
            with_caret += b"^" in md
            with_mismatch += nm > 0
        else:
            assert list(tags) in (["XE"], [])
        nm_sum += tags.get("NM", 0)
        xe_sum += tags.get("XE", 0)
        tag_bytes += len(aux)
    assert with_caret > 0 and with_mismatch > 100
    err = runs["err_tagged"]
    assert TB.stat(err, "truth_nm_sum") == nm_sum and TB.stat(err, "truth_xe_sum") == xe_sum and TB.stat(err, "truth_md_dropped") == 0
    assert TB.stat(err, "truth_tag_bytes") == tag_bytes == TB.stat(err, "truth_bytes") - TB.stat(runs["err_plain"], "truth_bytes")
    assert TB.stat(err, "truth_records") == TB.stat(runs["err_plain"], "truth_records") == len(plain)
    for key in ("truth_tag_bytes", "truth_md_dropped", "truth_nm_sum", "truth_xe_sum"):
        assert TB.stat(runs["err_plain"], key) == 0
    # XE over the file = the true error counts of the same run
    table = EM.parse_file(open(os.path.join(runs["tagged"], stem + ".truth.errors.tsv"), "rb").read())
    assert xe_sum == sum(v[1] for v in table["Q"].values()) + sum(v[1] for v in table["I"].values()) + sum(v[1] for v in table["D"].values()) > 1000


def test_pieces_give_the_same_records(runs, tmp_path):
    out = str(tmp_path / "pieces")
    r = TB.simu(runs["cfg"], out, "--truth-bam", "--truth-tags", env={"SIMU_PIECE_SLOTS": "1", "SIMU_TRACE_PIECES": "1"})
    assert r.stderr.count("[piece]") >= 2                            # several pieces (a segment is never cut)
    stem = runs["stem"]
    assert raw_records_of_file(os.path.join(out, stem + ".truth.bam"))[1] == raw_records_of_file(os.path.join(runs["tagged"], stem + ".truth.bam"))[1]
    assert md5s(out) == md5s(runs["tagged"])


def test_two_ranks_give_the_same_records(runs, tmp_path):
    two = str(tmp_path / "two")
    for r in range(2):
        TB.simu(runs["cfg"], two, "--truth-bam", "--truth-tags", "--rank", str(r), "--world", "2")
    stem = runs["stem"]
    p0 = open(os.path.join(two, stem + ".truth.bam.part0"), "rb").read()
    p1 = open(os.path.join(two, stem + ".truth.bam.part1"), "rb").read()
    d2 = U.inflate_members(p0 + p1)
    one = raw_records_of_file(os.path.join(runs["tagged"], stem + ".truth.bam"))[1]
    assert sorted(r for _, r in B.parse_stream(d2)[1]) == sorted(one)


def test_no_write_and_the_refusal(runs, tmp_path):
    out = str(tmp_path / "nowrite")
    r = TB.simu(runs["cfg"], out, "--truth-bam", "--truth-tags", "--no-write")
    for key in ("truth_records", "truth_bytes", "truth_tag_bytes", "truth_nm_sum", "truth_xe_sum"):
        assert TB.stat(r.stderr, key) == TB.stat(runs["err_tagged"], key) > 0, key
    assert not os.path.exists(out) or not os.listdir(out)
    alone = str(tmp_path / "alone")
    r = TB.simu(runs["cfg"], alone, "--truth-tags", ok=False)
    assert r.returncode == 1 and "--truth-tags" in r.stderr and "--truth-bam" in r.stderr
    assert not os.path.exists(alone) or not os.listdir(alone)


def test_the_trainer_reads_the_tagged_file(tmp_path):
    """seqToProfile -b tagged.truth.bam --decode-bam writes the profile it writes from the untagged file of the same run."""
    wd = str(tmp_path)
    prof = os.path.join(cases.TESTDATA, cases.PROFILES["xten"])
    cfg, fa, _ = U.acgt_case(wd, prof, "PE", coverage=8, insert=350, lengths=(200000, 40000))
    vcf = os.path.join(wd, "empty.vcf")
    open(vcf, "w").write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n")
    got = {}
    for name, flags in (("plain", ()), ("tagged", ("--truth-tags",))):
        out = os.path.join(wd, name)
        TB.simu(cfg, out, "--truth-bam", *flags)
        (stem,) = TB.stems(out)
        dst = os.path.join(wd, name + ".profile")
        r, st = TB._train_cli(["-b", os.path.join(out, stem + ".truth.bam"), "--decode-bam", "-v", vcf, "-r", fa, "-o", dst])
        assert r.returncode == 0 and st["reads_counted"] > 0, r.stderr[-2000:]
        got[name] = open(dst, "rb").read().split(b"\n", 2)[2]           # (the first two lines carry the run's stamp)
    assert got["plain"] == got["tagged"] and len(got["plain"]) > 1000
