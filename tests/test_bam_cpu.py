"""BAM input without the GPU: the tests' own BGZF / BAM writer (tests/bam_util.py) against Python's zlib and gzip, the
host-only member walk of the engine (sg_bgzf_members) against a Python walk, and the command line's refusals of
--decode-bam, which come before any device is touched."""
import ctypes as C
import gzip
import os
import random
import subprocess
import zlib

import bam_util as B
import simuscop_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "simuscop_amd", "lib", "seqToProfile")


def _payload(n, seed=1):
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n // 2)) + bytes(rng.randrange(256) for _ in range(n - n // 2))


def test_writer_inflates_with_zlib_and_ends_in_the_eof_member():
    data = _payload(300000)
    for level, strategy in ((0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (9, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)):
        buf = B.bgzf(data, member=50000, level=level, strategy=strategy)
        assert gzip.decompress(buf) == data
        assert B.inflate(buf) == data
    eof = C.create_string_buffer(28)
    assert simuscop_amd.load_engine().sg_bgzf_eof(eof) == 0
    assert eof.raw == B.EOF_MEMBER == buf[-28:]
    assert gzip.decompress(B.EOF_MEMBER) == b""


def test_record_layout_round_trips_through_the_renderer():
    lines = [b"r1\t99\tchr1\t100\t60\t10M2I5M3D2M\t=\t300\t250\tACGTACGTACGTACGTACG\tFFFFFFFFFFFFFFFFFFF",
             b"r2\t0\tchr2\t1\t20\t*\t*\t0\t0\t*\t*",
             b"r3\t16\tchr1\t5\t255\t4M\tchr2\t9\t-7\tNNAC\t*",
             b"r4\t0\tchr1\t50\t60\t3M1I3M\t=\t0\t0\tACGTACG\tIIIIIII"]
    d = B.bam_stream(lines, refs=[(b"chr1", 1000)], use_cg={3})
    assert B.view(d) == b"".join(ln + b"\n" for ln in lines)
    # the filter of `-F 0xD04 -q 20`
    drop = [b"d%d\t%d\tchr1\t1\t%d\t1M\t*\t0\t0\tA\tF" % (i, f, q) for i, (f, q) in enumerate(((4, 60), (0x100, 60), (0x400, 60), (0x800, 60), (0, 19)))]
    keep = [b"k%d\t%d\tchr1\t1\t%d\t1M\t*\t0\t0\tA\tF" % (i, f, q) for i, (f, q) in enumerate(((0x200, 60), (0, 20), (0, 255)))]
    assert B.view(B.bam_stream(drop + keep)) == b"".join(ln + b"\n" for ln in keep)
    assert B.reg2bin(0, 1) == 4681 and B.reg2bin(0, 1 << 14) == 4681 and B.reg2bin(0, (1 << 14) + 1) == 585 and B.reg2bin(0, 1 << 29) == 0


def test_optional_fields_of_every_type_leave_the_eleven_fields_alone():
    rng = random.Random(9)
    lines = [b"r%d\t0\tchr1\t%d\t60\t3M%dI4M\t=\t0\t0\tACGTACG%s\tIIIIIII%s" % (i, 50 + i, i + 1, b"A" * (i + 1), b"F" * (i + 1)) for i in range(6)]
    plain = B.bam_stream(lines, refs=[(b"chr1", 1000)], use_cg=set(range(6)))
    every = B.aux_every_type(rng)
    assert len(every) == 18 and sorted(t[2:3] for t in every) == sorted([bytes([c]) for c in b"AcCsSiIfdZH"] + [b"B"] * 7)
    assert sorted(t[3:4] for t in every if t[2:3] == b"B") == sorted(bytes([c]) for c in B.AUX_ARRAYS.encode())
    al = B.aligner_tags(rng, 7)
    assert [al.count(t) for t in (b"NM", b"MD", b"AS", b"XS", b"RG")] == [1] * 5
    aux = {0: (b"", b"".join(every) + al, b"I"), 1: (b"".join(every) + al, b"", b"I"), 2: (b"".join(every[:9]), b"".join(every[9:]), b"I"),
           3: (b"".join(every[::-1]), al, b"i"), 4: al, 5: (b"".join(every[11:]), b"".join(every[:11]), b"i")}
    d = B.bam_stream(lines, refs=[(b"chr1", 1000)], use_cg=set(range(6)), aux=aux)
    assert len(d) > len(plain) + 1000
    assert B.view(d) == B.view(plain) == b"".join(ln + b"\n" for ln in lines)   # CG:B:I and CG:B:i found behind, between and before them
    names, recs = B.parse_stream(d)
    for (_, r), ln in zip(recs, lines):
        cigar = ln.split(b"\t")[5]
        assert [(o >> 4, o & 15) for o in B._cigar_ops(r)] == B.parse_cigar(cigar)
        assert r.count(b"CGB") >= 1 and int.from_bytes(r[16:18], "little") == 2
    # an unknown type letter hides the CG behind it; a Z field that is not terminated runs to the record's end; a CG array
    # shorter than n_cigar is ignored (htslib's bam_tag2cigar)
    d = B.bam_stream(lines[:1], refs=[(b"chr1", 1000)], use_cg={0}, aux={0: (b"XQ?abcd", b"", b"I")})
    assert B.view(d).split(b"\t")[5] == b"8S7N"   # (l_seq 8, 7 reference bases: the placeholder itself)
    d = B.bam_stream([b"r\t0\tchr1\t5\t60\t7S9N\t=\t0\t0\tACGTACG\tIIIIIII"], refs=[(b"chr1", 1000)], aux={0: al + b"XZZnever ends"})
    assert B.view(d).split(b"\t")[5] == b"7S9N" and d.endswith(b"never ends")
    short = B.aux_tag(b"CG", "BI", [7 << 4])
    d = B.bam_stream([b"r\t0\tchr1\t5\t60\t7S9N\t=\t0\t0\tACGTACG\tIIIIIII"], refs=[(b"chr1", 1000)], aux={0: short})
    assert B.view(d).split(b"\t")[5] == b"7S9N"


def _members_c(buf, cap=1 << 20):
    lib = simuscop_amd.load_engine()
    off = (C.c_uint64 * cap)()
    bs, isz = (C.c_uint32 * cap)(), (C.c_uint32 * cap)()
    n, whole = C.c_uint64(), C.c_uint64()
    rc = lib.sg_bgzf_members(buf, len(buf), off, bs, isz, cap, C.byref(n), C.byref(whole))
    return rc, [(off[i], bs[i], isz[i]) for i in range(n.value)], whole.value


def test_member_walk_agrees_with_python():
    data = _payload(200000, 3)
    buf = B.bgzf(data, member=7000, level=6)
    want, wb = B.members(buf)
    rc, got, whole = _members_c(buf)
    assert rc == 0 and got == want and whole == wb == len(buf)
    for cut in (len(buf) - 1, len(buf) - 28, want[5][0] + 10, want[5][0] + 5, 3):   # a cut member at the end is left out
        w2, wb2 = B.members(buf[:cut])
        rc, got, whole = _members_c(buf[:cut])
        assert rc == 0 and got == w2 and whole == wb2 and whole <= cut, cut
    rc, got, whole = _members_c(buf, cap=4)   # a cap
    assert rc == 0 and got == want[:4] and whole == want[4][0]
    bad = bytearray(buf)
    bad[want[2][0] + 12] = ord("X")   # no BC subfield
    rc, got, whole = _members_c(bytes(bad))
    assert rc == 1 and whole == want[2][0] and len(got) == 2
    assert b"offset %d" % want[2][0] in simuscop_amd.load_engine().sg_last_error(None)


def test_decode_bam_refusals_touch_no_device(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    sam = os.path.join(str(tmp_path), "x.sam")
    open(sam, "w").write("")
    r = subprocess.run([EXE, "--decode-bam", "-v", "k.vcf", "-r", "r.fa"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 1 and "--decode-bam needs a BAM file" in r.stderr, r.stderr
    r = subprocess.run([EXE, "-b", "x.bam", "--decode-bam", "--sam", sam, "-v", "k.vcf", "-r", "r.fa"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 1 and "--decode-bam and --sam cannot be used together" in r.stderr, r.stderr
    assert "GPU engine" not in r.stderr
    r = subprocess.run([EXE, "-h"], capture_output=True, text=True, timeout=60)
    assert "--decode-bam" in r.stderr
