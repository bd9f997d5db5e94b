"""sg_inflate_bgzf (simuscop_amd/csrc/sg_inflate.hip) on DEFLATE streams that zlib's compressor never writes, against
zlib.decompressobj(-15) on the same raw stream (tests/deflate_craft.py; that writer is itself tested in
test_deflate_craft_cpu.py).

  legal     the directed corpus (codes of up to 15 bits, a distance code of one code and of none, runs that cross into the
            distance lengths, HLIT 286 / HDIST 30, length 258 as symbol 284 + 31, distance 32768 and distance == bytes written,
            output that ends at byte 65536, stored blocks of 0 bytes / behind every bit offset / that fill the member, bytes left
            before the trailer), the seeded generator's multi-block streams and the mutated streams zlib accepts: hundreds of
            members per launch, the output zlib's byte for byte
  sweep     ISIZE 0..2100, k * 1024 + {-1..4} and the sizes up to 65536: the CRC tree at every lane count and on the edge where
            the four bytes carrying the ~0 start straddle two lanes; a wrong first payload byte is a CRC-32 refusal
  illegal   each in a call of its own between two legal members: SG_ERR_INVALID naming the member's offset and, for the
            directed cases, the cause that belongs to zlib's message; for mutated streams the refusal

The order is legal, sweep, illegal; every call's return code is looked at, and after one that is neither 0 nor 1 nothing
more of this module runs.  SIMU_DEFLATE_SEEDS=a-b widens the generator's and the mutator's seeds."""
import ctypes as C
import struct
import zlib

import pytest

import bam_util as B
import deflate_craft as D
import simuscop_amd

pytestmark = pytest.mark.gpu

_STOP = []


@pytest.fixture(scope="module")
def eng():
    lib = simuscop_amd.load_engine()
    ctx = C.c_void_p()
    assert lib.sg_create(C.byref(ctx), 0, 1) == 0
    yield lib, ctx
    lib.sg_destroy(ctx)


@pytest.fixture(autouse=True)
def _stop_after_an_unexpected_return_code():
    if _STOP:
        pytest.fail("not run: an earlier call returned %s" % _STOP[0])


def _inflate(eng, buf, total):
    """one call with room for `total` bytes: (rc, output, message); rc is 0 or 1 or the module stops"""
    lib, ctx = eng
    out = C.create_string_buffer(total + 1)
    n = C.c_uint64()
    rc = lib.sg_inflate_bgzf(ctx, buf, len(buf), out, total, C.byref(n))
    msg = lib.sg_last_error(ctx).decode(errors="replace") if rc else ""
    if rc not in (0, 1):
        _STOP.append("%d (%s)" % (rc, msg))
        pytest.fail("sg_inflate_bgzf returned %d: %s" % (rc, msg))
    return rc, out.raw[:n.value] if rc == 0 else b"", msg


def _check_legal(eng, streams, per_call=400):
    """streams: (name, raw, expected output).  Members of `per_call` streams and the EOF member per launch."""
    for lo in range(0, len(streams), per_call):
        part = streams[lo:lo + per_call]
        ms = [D.member(raw, want) for _, raw, want in part]
        offs, at = [], 0
        for m in ms:
            offs.append(at)
            at += len(m)
        rc, got, msg = _inflate(eng, b"".join(ms) + B.EOF_MEMBER, sum(len(w) for _, _, w in part))
        if rc:
            named = [name for (name, _, _), o in zip(part, offs) if "offset %d:" % o in msg]
            pytest.fail("refused: %s (%s)" % (msg, named))
        at = 0
        for name, _, want in part:
            piece = got[at:at + len(want)]
            if piece != want:
                first = next(i for i in range(len(want)) if i >= len(piece) or piece[i] != want[i])
                pytest.fail("%s: output differs from zlib's at byte %d of %d" % (name, first, len(want)))
            at += len(want)
        assert at == len(got)


def _legal_directed():
    return [(c.name, c.raw, D.reference(c.raw)[1]) for c in D.directed() if c.legal and c.fits]


def _good_member(n, seed):
    data = D.crc_payload(n + seed)[:n]
    return B.bgzf_member(data, 6), data


# ---- legal streams -------------------------------------------------------------------------------------------------
def test_directed_legal_streams(eng):
    streams = _legal_directed()
    assert len(streams) >= 30 and all(D.reference(raw)[0] for _, raw, _ in streams)
    _check_legal(eng, streams)
    _check_legal(eng, streams[::-1] * 3)   # and in another order, so that a table left by one member meets another


def test_generated_streams(eng):
    streams = []
    for seed in D.seeds(D.GEN_SEEDS):
        raw = D.generate(seed).raw()
        legal, out, _ = D.reference(raw)
        assert legal, seed
        streams.append(("generate(%d)" % seed, raw, out))
    _check_legal(eng, streams)


def test_mutated_streams_that_zlib_accepts(eng):
    streams = []
    for label, _, raw in D.mutated(D.seeds(D.MUT_SEEDS)):
        legal, out, _ = D.reference(raw)
        if legal:
            streams.append((label, raw, out))
    assert len(streams) >= 100
    _check_legal(eng, streams)


# ---- the CRC-32 and size sweep ---------------------------------------------------------------------------------------
def test_crc_and_size_sweep(eng):
    sizes = D.CRC_SIZES
    half = len(sizes) // 2
    for part in (sizes[:half], sizes[half:]):
        datas = [D.crc_payload(n) for n in part]
        ms = [B.bgzf_member(d, 1) for d in datas]
        rc, got, msg = _inflate(eng, b"".join(ms) + B.EOF_MEMBER, sum(part))
        if rc:
            at = 0
            for n, m in zip(part, ms):
                assert "offset %d:" % at not in msg, "ISIZE %d refused: %s" % (n, msg)
                at += len(m)
            pytest.fail(msg)
        at = 0
        for n, d in zip(part, datas):
            assert got[at:at + n] == d, "ISIZE %d" % n
            at += n
        assert at == len(got)


@pytest.mark.parametrize("n", [5 * 1024 + 2, 5 * 1024 + 100, 63 * 1024 + 1, 4, 5])
def test_a_wrong_first_byte_is_a_crc_refusal(eng, n):
    # the neighbours inflate; the member in the middle holds, in a stored block, the payload with another first byte under
    # the trailer of the true payload.  5 KiB + 2 and 63 KiB + 1 are on the edge where the folded start straddles two lanes.
    a, _ = _good_member(3000, 1)
    z, _ = _good_member(1025, 2)
    data = D.crc_payload(n)
    s = D.Stream()
    s.stored(bytes([data[0] ^ 0x80]) + data[1:], final=True)
    bad = D.member(s.raw(), data)
    rc, _, msg = _inflate(eng, a + bad + z, 3000 + n + 1025)
    assert rc == 1 and "offset %d:" % len(a) in msg and "CRC-32 does not match" in msg, msg
    s = D.Stream()
    s.stored(data, final=True)
    rc, got, msg = _inflate(eng, a + D.member(s.raw(), data) + z, 3000 + n + 1025)
    assert rc == 0 and got[3000:3000 + n] == data, msg


# ---- the header walk -------------------------------------------------------------------------------------------------
def test_header_subfield_before_bc_and_flags_other_than_fextra(eng):
    data = D.crc_payload(700)
    raw = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = raw.compress(data) + raw.flush()
    a, da = _good_member(500, 3)
    m = D.member(raw, data, extra=b"XY" + struct.pack("<H", 2) + b"\x01\x02")
    assert struct.unpack_from("<H", m, 10)[0] == 12
    rc, got, msg = _inflate(eng, a + m + a, 500 + 700 + 500)
    assert rc == 0 and got == da + data + da, msg
    # gzip's FNAME beside FEXTRA: the name lies where the data would start; the member is refused by its header
    m = D.member(raw, data, flags=4 | 8, tail=b"reads.bam\0")
    assert zlib.decompress(m, 31) == data   # (a gzip member all right)
    rc, _, msg = _inflate(eng, a + m + a, 500 + 700 + 500)
    assert rc == 1 and "offset %d:" % len(a) in msg and "flags other than FEXTRA" in msg, msg
    for flags in (4 | 2, 4 | 16, 4 | 1):   # FHCRC, FCOMMENT, FTEXT
        rc, _, msg = _inflate(eng, a + D.member(raw, data, flags=flags) + a, 1700)
        assert rc == 1 and "offset %d:" % len(a) in msg and "flags other than FEXTRA" in msg, (flags, msg)


# ---- illegal streams -------------------------------------------------------------------------------------------------
# The verdict of sg_inflate.hip that belongs to each of zlib's messages.
CAUSE = {
    "invalid block type": "block type 3",
    "invalid stored block lengths": "stored block length does not match",
    "too many length or distance symbols": "Huffman code",
    "invalid code lengths set": "Huffman code",
    "invalid bit length repeat": "Huffman code",
    "invalid code -- missing end-of-block": "Huffman code",
    "invalid literal/lengths set": "Huffman code",
    "invalid distances set": "Huffman code",
    "invalid literal/length code": "Huffman code",
    "invalid distance code": "distance beyond the output",
    "invalid distance too far back": "distance beyond the output",
    D.TOO_LONG: "more than 64 KiB of output",
}
# zlib calls bits that match no code of the distance code "invalid distance code", as it calls the fixed code's distance codes
# 30 and 31.  The kernel tells the two apart: 30 and 31 are codes, of a distance that does not exist ("distance beyond the
# output"); bits that are no code at all -- the unused half of a code of one length-1 code, or any bit where the block has
# no distance code -- are "over-subscribed, incomplete or unused Huffman code", which says what is wrong with the stream.
CAUSE_BY_NAME = {"one_distance_code_of_length_1_other_bit": "unused Huffman code", "no_distance_code_but_a_match": "unused Huffman code"}


def _check_illegal(eng, name, raw, cause):
    a, z = _good_member(777, 5)[0], _good_member(64, 6)[0]   # (the call is refused as a whole: the neighbours' bytes are not seen)
    _, out, _ = D.reference(raw)
    m = D.member(raw, out)
    rc, _, msg = _inflate(eng, a + m + z, 777 + min(len(out), D.MAXI) + 64)
    assert rc == 1, "%s: accepted" % name
    assert "offset %d:" % len(a) in msg, (name, msg)
    if cause is not None:
        assert cause in msg, (name, msg)


def test_directed_illegal_streams(eng):
    corpus = [c for c in D.directed() if not c.legal]
    assert len(corpus) >= 30
    for c in corpus:
        assert c.fits
        # a stream that ends early makes the kernel read the trailer and the next member as data: which check stops it
        # depends on those bytes, so only the refusal and the offset are asserted
        cause = None if c.outcome == D.NO_EOF else CAUSE_BY_NAME.get(c.name, CAUSE[c.outcome])
        _check_illegal(eng, c.name, c.raw, cause)
    _check_legal(eng, _legal_directed())   # the context is as good as before


def test_mutated_streams_that_zlib_refuses(eng):
    n = 0
    for label, _, raw in D.mutated(D.seeds(D.MUT_SEEDS)):
        if not D.reference(raw)[0] and len(raw) <= D.MAX_RAW:
            _check_illegal(eng, label, raw, None)
            n += 1
    assert n >= 100
    _check_legal(eng, _legal_directed())
