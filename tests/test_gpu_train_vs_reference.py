"""`seqToProfile` on the MI355X against the unmodified reference seqToProfile: `--sam` and `-b x.bam --decode-bam` write the
reference's .profile and .gc files byte for byte (behind the time-stamp line, which is the product's own clock) on the
whole-genome, exome, -k 1 / -k 5, non-base ALT and open-last-line inputs of tests/test_train_vs_reference.py.  The reference
runs from oracle/_ref/seqToProfile where it is built, from its recorded runs (tests/golden/reference_train_runs.json)
elsewhere."""
import hashlib
import os
import subprocess

import pytest

import bam_util as B
import ref_runs
import test_train_vs_reference as TR
from test_train_vs_reference import sim  # noqa: F401  (the module fixture: sampled read pairs)
import train_util as TU

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "simuscop_amd", "lib", "seqToProfile")


def _md5(b):
    return hashlib.md5(b).hexdigest()


def product(wd, args, kmer, bins, bed):
    """The product's files, as the reference would have named and stamped them: {"ref.profile": md5, "ref.profile.gc": md5}."""
    for f in ("got.profile", "got.profile.gc"):
        if os.path.exists(os.path.join(wd, f)):
            os.remove(os.path.join(wd, f))
    cmd = [EXE, *args, "-r", "train.fa", "-v", "known.vcf", "-o", "got.profile", "-k", str(kmer), "-B", str(bins), "--quiet"]
    r = subprocess.run(cmd + (["-t", os.path.basename(bed)] if bed else []), cwd=wd, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    head, body = open(os.path.join(wd, "got.profile"), "rb").read().split(b"\n", 1)
    assert head.startswith(b"#model created at ")
    out = {"ref.profile": _md5(b"#model created at " + TR.STAMP + body)}
    if os.path.exists(os.path.join(wd, "got.profile.gc")):
        out["ref.profile.gc"] = _md5(open(os.path.join(wd, "got.profile.gc"), "rb").read())
    return out, body


def reference(oracle_lib, wd, fa, vcf, bed, lines, kmer, bins, final_newline=True):
    sam = b"\n".join(lines) + (b"\n" if final_newline else b"")
    open(os.path.join(wd, "reads.sam"), "wb").write(sam)
    assert not TU.reference_undefined(oracle_lib, fa, vcf, bed, sam)
    rc, want = ref_runs.run_train(wd, "reads.sam", "train.fa", "known.vcf", bed and os.path.basename(bed), kmer, bins)
    assert rc == 0 and "ref.profile" in want
    return sam, want


@pytest.mark.parametrize("what,kmer,bins", [("wgs", 3, 50), ("exome", 3, 50), ("wgs", 1, 50), ("wgs", 5, 50), ("wgs", 3, 200)])
def test_sam_route_writes_the_reference_profile(what, kmer, bins, sim, oracle_lib, tmp_path):  # noqa: F811
    wd = str(tmp_path)
    fa, vcf, bed, lines = TR.whole_input(wd, sim, exome=(what == "exome"))
    _, want = reference(oracle_lib, wd, fa, vcf, bed, lines, kmer, bins)
    got, _ = product(wd, ["--sam", "reads.sam"], kmer, bins, bed)
    assert got == want


def test_sam_route_on_a_non_base_alt_and_an_open_last_line(sim, oracle_lib, tmp_path):  # noqa: F811
    """Known SNVs whose ALT is N, R, n or * with reads that show it, in position order among the sampled reads (the
    reference compares raw characters); then the same input without its final line break (:1459 chops a character)."""
    wd = str(tmp_path)
    fa, vcf, bed, lines = TR.whole_input(wd, sim)
    lines = TR.with_odd_alts(wd, sim, fa, vcf, lines)
    want = [reference(oracle_lib, wd, fa, vcf, bed, lines, 3, 50, final_newline)[1] for final_newline in (False, True)]
    got = [product(wd, ["--sam", "reads.sam"], 3, 50, bed)[0]]     # (reads.sam now ends in a line break)
    open(os.path.join(wd, "reads.sam"), "wb").write(b"\n".join(lines))
    got.insert(0, product(wd, ["--sam", "reads.sam"], 3, 50, bed)[0])
    assert got == want


@pytest.mark.parametrize("exome", [False, True])
def test_decode_bam_writes_the_reference_profile(exome, sim, oracle_lib, tmp_path):  # noqa: F811
    """A BAM of the same records (tests/bam_util.py), read with --decode-bam: `samtools view -F 0xD04 -q 20` of it prints
    exactly the SAM text the reference trained on, and the files are the reference's.  (The filter lines of
    train_util.filter_lines stay out: a BAM holds no lower-case base, no CIGAR without an operation, no short quality.)"""
    wd = str(tmp_path)
    fa, vcf, bed, lines = TR.whole_input(wd, sim, exome=exome)
    lines = [ln for ln in lines if not ln.startswith((b"x\t", b"extra\t"))]
    sam, want = reference(oracle_lib, wd, fa, vcf, bed, lines, 3, 50)
    refs = []
    for chunk in open(fa, "rb").read().split(b">")[1:]:
        name, seq = chunk.split(b"\n", 1)
        refs.append((name.split()[0], len(seq) - seq.count(b"\n")))
    text = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    d = B.bam_stream(lines, refs=refs, text=text)
    assert B.view(d) == sam
    open(os.path.join(wd, "reads.bam"), "wb").write(B.bgzf(d))
    got, body = product(wd, ["-b", "reads.bam", "--decode-bam"], 3, 50, bed)
    label = body.split(b"\n", 1)
    assert label[0] == b"#reads: reads.bam"
    got["ref.profile"] = _md5(b"#model created at " + TR.STAMP + b"#reads: reads.sam\n" + label[1])
    assert got == want
