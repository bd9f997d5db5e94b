"""BGZF members inflated on the MI355X (sg_inflate_bgzf, simuscop_amd/csrc/sg_inflate.hip) against zlib, byte for byte:
stored, fixed- and dynamic-Huffman blocks (zlib levels 0, 1, 6, 9 and its strategies), members of 1 B to 65,280 B, empty
members, random bytes and FASTQ text, and this project's own device BGZF output (`simuReads --gzip`).  Members that are not
well formed -- CRC-32, ISIZE, BSIZE, block type 3, a truncated buffer -- are SG_ERR_INVALID with the member's offset named,
and the context keeps working."""
import ctypes as C
import os
import random
import struct
import subprocess
import zlib

import pytest

import bam_util as B
import cases
import simuscop_amd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMU = os.path.join(ROOT, "simuscop_amd", "lib", "simuReads")


@pytest.fixture(scope="module")
def eng():
    lib = simuscop_amd.load_engine()
    ctx = C.c_void_p()
    assert lib.sg_create(C.byref(ctx), 0, 1) == 0
    yield lib, ctx
    lib.sg_destroy(ctx)


def _inflate(eng, buf):
    lib, ctx = eng
    n = C.c_uint64()
    rc = lib.sg_inflate_bgzf(ctx, buf, len(buf), None, 0, C.byref(n))
    if rc == 4:   # SG_ERR_OVERFLOW: room for n bytes
        out = C.create_string_buffer(n.value + 1)
        rc = lib.sg_inflate_bgzf(ctx, buf, len(buf), out, n.value, C.byref(n))
        return rc, out.raw[:n.value]
    return rc, b""


def _fastq(n, seed):
    rng = random.Random(seed)
    out = []
    while sum(map(len, out)) < n:
        s = bytes(rng.choice(b"ACGT") for _ in range(150))
        q = bytes(rng.choice(b"#,-7<AFJ") for _ in range(150))
        out.append(b"@r%d/1\n%s\n+\n%s\n" % (rng.randrange(10 ** 9), s, q))
    return b"".join(out)[:n]


SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 1000, 4096, 32768, 40000, 65280)


@pytest.mark.parametrize("level,strategy", [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY),
                                            (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE),
                                            (9, zlib.Z_FILTERED)])
def test_inflate_matches_zlib(eng, level, strategy):
    rng = random.Random(level * 10 + strategy)
    pieces = []
    for i, n in enumerate(SIZES):
        pieces.append(bytes(rng.randrange(256) for _ in range(n)))                       # random bytes
        pieces.append(_fastq(n, i))                                                       # FASTQ text
        pieces.append(bytes(rng.choice(b"AC") for _ in range(n)))                         # long matches
        pieces.append(b"")                                                                # an empty member
    data = b"".join(pieces)
    cuts, at = [], 0
    for p in pieces:
        cuts.append(at)
        at += len(p)
    buf = b"".join(B.bgzf_member(p, level, strategy) for p in pieces) + B.EOF_MEMBER
    assert B.inflate(buf) == data
    rc, got = _inflate(eng, buf)
    assert rc == 0, eng[0].sg_last_error(eng[1])
    assert got == data


def test_several_blocks_per_member(eng):
    # a dynamic block, a stored block, a fixed block and a final empty block in one member (zlib's full flushes / params)
    rng = random.Random(4)
    parts = [_fastq(20000, 1), bytes(rng.randrange(256) for _ in range(9000)), b"ACGT" * 3000, b""]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = c.compress(parts[0]) + c.flush(zlib.Z_FULL_FLUSH)
    c2 = zlib.compressobj(0, zlib.DEFLATED, -15)
    raw2 = c2.compress(parts[1]) + c2.flush(zlib.Z_FULL_FLUSH)
    c3 = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    raw3 = c3.compress(parts[2]) + c3.flush()
    data = b"".join(parts)
    # raw and raw2 end with non-final blocks (the sync flush), raw3 ends with the final block
    deflate = raw + raw2 + raw3
    assert zlib.decompress(deflate, -15) == data
    bsize = 18 + len(deflate) + 8 - 1
    member = (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize) + deflate +
              struct.pack("<II", zlib.crc32(data), len(data)))
    rc, got = _inflate(eng, member + B.EOF_MEMBER)
    assert rc == 0 and got == data, eng[0].sg_last_error(eng[1])


def test_device_bgzf_output_round_trips(eng, tmp_path):
    cfg = cases.build_case("wgs_pe_variants", str(tmp_path))
    r = subprocess.run([SIMU, cfg, "--seed", "5", "--out", str(tmp_path / "gz"), "--quiet", "--gzip"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    files = sorted(os.listdir(tmp_path / "gz"))
    assert files
    for f in files:
        blob = open(tmp_path / "gz" / f, "rb").read()
        rc, got = _inflate(eng, blob)
        assert rc == 0, eng[0].sg_last_error(eng[1])
        assert got == B.inflate(blob), f


def test_malformed_members_are_refused(eng):
    lib, ctx = eng
    data = [_fastq(30000, 7), _fastq(20000, 8), _fastq(10000, 9)]
    ms = [B.bgzf_member(d, 6) for d in data]
    good = b"".join(ms) + B.EOF_MEMBER
    off2 = len(ms[0])
    cases_ = {}
    x = bytearray(good); x[off2 + len(ms[1]) - 8] ^= 1; cases_["crc"] = bytes(x)               # CRC-32
    x = bytearray(good); x[off2 + len(ms[1]) - 4] ^= 1; cases_["isize"] = bytes(x)             # ISIZE
    x = bytearray(ms[0] + ms[1]); struct.pack_into("<H", x, off2 + 16, len(ms[1]) - 1 + 40); cases_["bsize"] = bytes(x)   # BSIZE past the end
    t3 = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + 2 + 8 - 1) + b"\x07\x00" + struct.pack("<II", 0, 0)
    cases_["type3"] = ms[0] + t3 + ms[2]                                                       # block type 3
    cases_["truncated"] = good[:off2 + len(ms[1]) // 2]                                        # cut short
    x = bytearray(good); x[off2 + 18 + 10] ^= 0xFF; cases_["data"] = bytes(x)                   # the DEFLATE data itself
    x = bytearray(good); x[off2 + 12] = ord("X"); cases_["no_bc"] = bytes(x)                   # no BC subfield
    for name, buf in cases_.items():
        rc, _ = _inflate(eng, buf)
        msg = lib.sg_last_error(ctx).decode()
        assert rc == 1, (name, rc, msg)
        assert "offset %d" % off2 in msg, (name, msg)
    rc, got = _inflate(eng, good)   # the context is fine afterwards
    assert rc == 0 and got == b"".join(data)
