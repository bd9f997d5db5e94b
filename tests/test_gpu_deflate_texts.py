"""The device BGZF compressor (simuscop_amd/csrc/sg_deflate.hip) on texts and lengths the sampler never gives it, through
sg_deflate_bgzf.  Every call is checked the same way (`check`): gzip returns the text; ceil(n / 32768) members whose BSIZE
walk ends at the blob's end; every member is one final dynamic block that zlib inflates, with nothing left over, to its own
32,768-byte slice, with that slice's CRC-32 and length behind it; sg_inflate_bgzf returns the text from the same blob; a
second call gives the same bytes.  On the members a test names, the tokens -- read by deflate_read.py -- are exactly those
the compressor's rules give (deflate_model.py), and where a closed form exists, that closed form.

The texts come from deflate_texts.py, which says what each is aimed at; tests/test_deflate_read_cpu.py runs the reader, the
model and the generators without a GPU.  Nothing here is meant to fault: every text is legal input, every call must return
SG_OK, and a test stops at its first other return."""
import ctypes as C
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

import cases
import deflate_craft as D
import deflate_model as M
import deflate_read as R
import deflate_texts as T
import profile_shapes as PS
import simuscop_amd
from profile_shapes import Shape
from test_gpu_bam_inflate import _fastq

pytestmark = pytest.mark.gpu

CHUNK = 32768
SG_OK, SG_ERR_OVERFLOW = 0, 4


def _create():
    lib = simuscop_amd.load_engine()
    ctx = C.c_void_p()
    assert lib.sg_create(C.byref(ctx), 0, 1) == 0
    return lib, ctx


@pytest.fixture(scope="module")
def eng():
    lib, ctx = _create()
    yield lib, ctx
    lib.sg_destroy(ctx)


def _deflate(eng, text):
    lib, ctx = eng
    cap = (len(text) + CHUNK - 1) // CHUNK * 65536      # BSIZE has 16 bits: no member is larger
    out = C.create_string_buffer(max(cap, 1))
    n = C.c_uint64(1 << 60)
    rc = lib.sg_deflate_bgzf(ctx, text, len(text), out, cap, C.byref(n))
    if rc != SG_OK:
        pytest.fail("sg_deflate_bgzf returned %d on %d bytes: %s" % (rc, len(text), lib.sg_last_error(ctx).decode()))
    assert n.value <= cap
    return out.raw[:n.value]


def _inflate(eng, blob):
    lib, ctx = eng
    n = C.c_uint64()
    rc = lib.sg_inflate_bgzf(ctx, blob, len(blob), None, 0, C.byref(n))
    if rc == SG_OK:
        assert n.value == 0
        return b""
    assert rc == SG_ERR_OVERFLOW, lib.sg_last_error(ctx).decode()
    out = C.create_string_buffer(n.value + 1)
    rc = lib.sg_inflate_bgzf(ctx, blob, len(blob), out, n.value, C.byref(n))
    if rc != SG_OK:
        pytest.fail("sg_inflate_bgzf returned %d: %s" % (rc, lib.sg_last_error(ctx).decode()))
    return out.raw[:n.value]


def _members(blob):
    """split by the BSIZE fields; the walk must end exactly at the blob's end"""
    out, p = [], 0
    while p < len(blob):
        assert blob[p:p + 4] == b"\x1f\x8b\x08\x04" and blob[p + 10:p + 12] == b"\x06\x00" and blob[p + 12:p + 16] == b"BC\x02\x00", p
        size = struct.unpack_from("<H", blob, p + 16)[0] + 1
        assert p + size <= len(blob), "BSIZE runs past the end"
        out.append(blob[p:p + size])
        p += size
    assert p == len(blob)
    return out


def check_blob(eng, text, blob, what, tokens=()):
    """everything `check` says about one blob; returns {member index: the reader's view} of the members in `tokens`"""
    assert gzip.decompress(blob) == text if blob else text == b"", what
    mem = _members(blob)
    assert len(mem) == (len(text) + CHUNK - 1) // CHUNK, what
    for i, m in enumerate(mem):
        want = text[i * CHUNK:(i + 1) * CHUNK]
        d = zlib.decompressobj(-15)
        body = d.decompress(m[18:-8])
        assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", (what, i)
        assert body == want, (what, i)
        assert struct.unpack("<II", m[-8:]) == (zlib.crc32(want) & 0xFFFFFFFF, len(want)), (what, i)
        assert m[18] & 7 == 5, (what, i)          # BFINAL = 1, BTYPE = 2: the first block is the last
    assert _inflate(eng, blob) == text, what
    seen = {}
    for i in tokens if mem else ():
        i = i % len(mem)
        if i in seen:
            continue
        s = R.read(mem[i][18:-8])
        want = text[i * CHUNK:(i + 1) * CHUNK]
        assert len(s.blocks) == 1 and s.blocks[0].kind == 2 and s.blocks[0].final and s.end == len(mem[i]) - 26, (what, i)
        assert s.out == want, (what, i)
        got, model = s.tokens(), M.member_tokens(want)
        if got != model:
            k = next(j for j in range(min(len(got), len(model))) if got[j] != model[j]) if got[:len(model)] != model[:len(got)] else min(len(got), len(model))
            at = M.positions(model)[k][0] if k < len(model) else len(want)
            pytest.fail("%s, member %d: tokens differ from the rules' at token %d (byte %d of the member, lane %d byte %d of the frame):\n device %r\n rules  %r" %
                        (what, i, k, at, (CHUNK - len(want) + at) // 64, (CHUNK - len(want) + at) % 64, got[max(0, k - 2):k + 4], model[max(0, k - 2):k + 4]))
        seen[i] = s
    return seen


ALL = object()


def check(eng, text, what, tokens=ALL):
    """one text through the compressor, twice; tokens: the members whose token lists are compared with the rules (ALL, or
    indexes; negative ones count from the end)"""
    blob = _deflate(eng, text)
    assert _deflate(eng, text) == blob, "%s: a second call gave other bytes" % what
    n_mem = (len(text) + CHUNK - 1) // CHUNK
    seen = check_blob(eng, text, blob, what, range(n_mem) if tokens is ALL else tokens)
    return blob, seen


# ---- the three kinds of text every length is run on -----------------------------------------------------------------
_BLOCK = {}


def kinds(n, seed=0):
    """FASTQ-like, all-equal and uniform random text of n bytes (long ones tile a block of 1 MiB: members are independent)"""
    if "fastq" not in _BLOCK:
        _BLOCK["fastq"] = _fastq(1 << 20, 1234)
        _BLOCK["random"] = np.random.default_rng(99).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    out = []
    for name in ("fastq", "random"):
        b = _BLOCK[name]
        off = (seed * 7919) % 4096
        out.append((name, (b[off:] + b * (n // len(b) + 1))[:n] if n > len(b) - off else b[off:off + n]))
    out.append(("equal", bytes([0x41 + seed % 50]) * n))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the entry point's contract
# ---------------------------------------------------------------------------------------------------------------------
def test_contract_of_the_entry_point(eng):
    lib, ctx = eng
    n = C.c_uint64(99)
    assert lib.sg_deflate_bgzf(ctx, None, 0, None, 0, C.byref(n)) == SG_OK and n.value == 0
    assert lib.sg_deflate_bgzf(ctx, b"", 0, None, 0, C.byref(n)) == SG_OK and n.value == 0
    text = _fastq(70000, 3)
    blob = _deflate(eng, text)
    for cap in (0, 1, len(blob) - 1):       # too small: the size is reported, nothing is written
        out = C.create_string_buffer(b"\xa5" * (cap + 8), cap + 8)
        n = C.c_uint64(0)
        assert lib.sg_deflate_bgzf(ctx, text, len(text), out, cap, C.byref(n)) == SG_ERR_OVERFLOW
        assert n.value == len(blob) and out.raw == b"\xa5" * (cap + 8)
    out = C.create_string_buffer(b"\xa5" * (len(blob) + 8), len(blob) + 8)
    assert lib.sg_deflate_bgzf(ctx, text, len(text), out, len(blob), C.byref(n)) == SG_OK      # exactly enough
    assert out.raw == blob + b"\xa5" * 8
    assert lib.sg_deflate_bgzf(ctx, text, len(text), out, len(blob), None) != SG_OK
    assert lib.sg_deflate_bgzf(ctx, None, 5, out, len(blob), C.byref(n)) != SG_OK
    eof = C.create_string_buffer(28)
    assert lib.sg_bgzf_eof(eof) == 0
    assert gzip.decompress(blob + eof.raw) == text


# ---------------------------------------------------------------------------------------------------------------------
# lengths
# ---------------------------------------------------------------------------------------------------------------------
def test_every_length_from_0_to_130(eng):
    for n in range(0, 131):
        for name, text in kinds(n, seed=n):
            check(eng, text, "%s of %d bytes" % (name, n))


def test_lengths_around_whole_members(eng):
    """32768 k + d: the last chunk holds 1, 63, 64, 65 bytes, or all but 65, 64, 63, 1, or is full"""
    for k in (1, 2, 3):
        for d in (-65, -64, -63, -1, 0, 1, 63, 64, 65):
            n = CHUNK * k + d
            for name, text in kinds(n, seed=k * 100 + d):
                check(eng, text, "%s of %d bytes" % (name, n), tokens=(-1,) if name != "equal" else ALL)


@pytest.mark.parametrize("members,extra", [(511, 0), (512, 0), (513, 0), (513, 1), (1025, 77)])
def test_lengths_where_the_histogram_starts_to_sample(eng, members, extra):
    """up to 512 members every member is in the histogram; 513 members: every second one; 1,025: every third"""
    n = CHUNK * members + extra
    assert M.sample_stride((n + CHUNK - 1) // CHUNK) == {511: 1, 512: 1, 513: 2, 514: 2, 1026: 3}[(n + CHUNK - 1) // CHUNK]
    for name, text in kinds(n, seed=members):
        check(eng, text, "%s of %d members + %d" % (name, members, extra), tokens=(0, 1, 2, 3, -2, -1) + tuple(range(4, members, 61)))


def test_a_context_that_went_large_then_small_then_large(eng):
    """the work buffer, the chunk counters, member sizes and offsets of an earlier, larger call must not show in a later one:
    the same calls on a context that has never compressed anything give the same bytes"""
    texts = [kinds(CHUNK * 40 + 1234, 5)[0][1], b"Z", kinds(CHUNK * 40 + 1234, 6)[1][1], b"", kinds(CHUNK * 3 - 1, 7)[0][1], kinds(7, 8)[2][1]]
    used = [_deflate(eng, t) for t in texts]
    for t, blob in zip(texts, used):
        check_blob(eng, t, blob, "used context, %d bytes" % len(t), tokens=(-1,))
    for i in (1, 5, 4, 2):       # each on a context of its own
        fresh = _create()
        try:
            assert _deflate(fresh, texts[i]) == used[i], "text %d" % i
        finally:
            fresh[0].sg_destroy(fresh[1])


# ---------------------------------------------------------------------------------------------------------------------
# all-equal text: closed-form tokens
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [0x00, 0x41, 0xFF])
def test_all_equal_member_has_the_closed_form_tokens(eng, b):
    """fails when gz_merge stops merging: 32,768 equal bytes are one literal, one match (255, 1), 127 matches (256, 1)"""
    _, seen = check(eng, bytes([b]) * CHUNK, "32768 x %02x" % b)
    assert seen[0].tokens() == [("lit", b), ("match", 255, 1)] + [("match", 256, 1)] * 127 + [("end",)]
    _, seen = check(eng, bytes([b]) * (3 * CHUNK), "3 x 32768 x %02x" % b)
    assert all(seen[i].tokens() == T.equal_tokens(CHUNK, b) for i in range(3))


@pytest.mark.parametrize("b", [0x00, 0x41, 0xFF])
def test_all_equal_short_last_chunk_has_the_closed_form_tokens(eng, b):
    """groups of four lanes are aligned to the frame, not to the data; the frame's bytes before the data are zeros and must
    not start a run of NULs (the `k > run_from` term)"""
    for j in (0, 1, 3, 4, 5):
        for r in (0, 1, 5, 63):
            n = 64 * j + r
            if n == 0:
                continue
            for lead in (0, CHUNK):      # the short chunk alone, and behind a full member
                _, seen = check(eng, bytes([b]) * (lead + n), "%d x %02x" % (lead + n, b))
                assert seen[len(seen) - 1].tokens() == T.equal_tokens(n, b), (j, r, lead)
    for n in range(1, 400):              # and every length up to six lanes, alone
        _, seen = check(eng, bytes([b]) * n, "%d x %02x" % (n, b))
        assert seen[0].tokens() == T.equal_tokens(n, b), n


# ---------------------------------------------------------------------------------------------------------------------
# runs, the six-match cap
# ---------------------------------------------------------------------------------------------------------------------
def test_runs_across_every_boundary(eng):
    """run bits from the masks (gz_tokens, "runs, where no copy went"), kGzMinRun on both sides, runs cut at the lane's end
    and put together again by gz_merge inside a group of four lanes, never across a group's or the member's edge"""
    name, text, facts = T.runs_text(1)
    _, seen = check(eng, text, name)
    toks = {i: dict(M.positions(s.tokens())) for i, s in seen.items()}
    for member, pos, length in T.runs_inside_a_lane(facts["runs"]):     # literal + (L - 1, 1) from six bytes on, literals below
        if length - 1 >= M.MIN_RUN:
            assert toks[member].get(pos) == ("lit", text[member * CHUNK + pos]) and toks[member].get(pos + 1) == ("match", length - 1, 1), (member, pos, length)
        else:
            assert all(toks[member].get(p, ("",))[0] == "lit" for p in range(pos, pos + length)), (member, pos, length)
    for i, s in seen.items():        # no match reaches over the member's edge (zlib enforces it too: a member is a stream of its own)
        for pos, t in M.positions(s.tokens()):
            assert t[0] != "match" or (t[2] <= pos and pos + t[1] <= len(s.out)), (i, pos, t)


def test_six_matches_per_lane_and_no_more(eng):
    """lanes of eight runs of six bytes in a text where no gram occurs twice: six leave as matches (5, 1), the seventh and
    eighth as literals -- in full members and in a short last chunk whose frame starts inside a lane"""
    name, text, facts = T.cap_text()
    _, seen = check(eng, text, name)
    for member, lane in facts["cap_lanes"]:
        base = lane * 64 - (facts["q0_last"] if member else 0)
        toks = [(p - base, t) for p, t in M.positions(seen[member].tokens()) if base <= p < base + 64 and t[0] != "end"]
        assert [(p, t[1:]) for p, t in toks if t[0] == "match"] == [(7 * i + 1, (5, 1)) for i in range(6)], (member, lane, toks)
        assert [p for p, t in toks if t[0] == "lit"] == sorted([7 * i for i in range(6)] + [7 * i + 6 for i in range(6)] + list(range(42, 64))), (member, lane)


# ---------------------------------------------------------------------------------------------------------------------
# copies
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", T.PERIODS)
def test_copies_at_odd_and_even_distances(eng, period):
    """only even positions are in the table: a copy at an odd distance is seen from the probes at odd positions"""
    name, text, facts = T.period_text(period, 1)
    _, seen = check(eng, text, name)
    for i, s in seen.items():
        ms = [t for t in s.tokens() if t[0] == "match"]
        assert all(t[2] % period == 0 for t in ms), name          # (the unit has no repeat inside)
        if period <= 152 and len(s.out) > 1000:
            assert ms and max(t[1] for t in ms) >= 64, name
    line = T.filler(151, 5) + b"\n"                              # a 152-byte line over and over, then with a byte changed now and then
    text = bytearray(line * 700)
    for at in range(1000, len(text), 1777):
        text[at] ^= 0x20
    check(eng, bytes(text), "a 152-byte line repeated")


@pytest.mark.parametrize("kind", T.COPY_KINDS + ("collision",))
def test_directed_copies(eng, kind):
    """overlapping copies; backward growth from the residues no probe falls on; the short-copy heuristic; tag collisions"""
    name, text, facts = T.tag_collision_text() if kind == "collision" else T.directed_copy_text(kind)
    _, seen = check(eng, text, name)
    at = dict(M.positions(seen[0].tokens()))
    for member, pos, length, dist in facts["matches"]:
        assert at.get(pos) == ("match", length, dist), (name, pos, length, dist)
    for member, a, b in facts["literal_spans"]:
        assert all(at.get(p, ("",))[0] == "lit" for p in range(a, b)), (name, a, b)
    if kind == "overlap":
        assert sum(1 for t in seen[0].tokens() if t[0] == "match" and t[2] < t[1]) >= 3


# ---------------------------------------------------------------------------------------------------------------------
# byte values
# ---------------------------------------------------------------------------------------------------------------------
def test_nul_ff_and_all_256_values(eng):
    """the frame's non-data bytes and the pad behind it are zeros: NULs at the start of the data and at the end of a short
    last chunk must never be matched against them"""
    for name, text, _ in T.byte_value_texts():
        check(eng, text, name)


# ---------------------------------------------------------------------------------------------------------------------
# codes the sample never saw
# ---------------------------------------------------------------------------------------------------------------------
def test_members_the_histogram_never_saw(eng):
    """1,026 members, every third in the histogram: the sampled ones make a literal code that the 15-bit limit shapes, the
    others hold only bytes it gave the longest codes to -- the largest members there are.  BSIZE still fits, the staging
    area (gz_stage_words: 15 bits a byte) and the 10-bit bit counts per lane hold."""
    name, text, facts = T.unseen_codes_text()
    blob, seen = check(eng, text, name, tokens=(0, 1, 2, 3, 4, -2, -1))
    lens = seen[1].blocks[0].lit_lens
    assert max(lens[:256]) == 15 and min(lens[b] for b in T.STEEP) <= 2
    assert all(seen[i].blocks[0].lit_lens == lens for i in seen)          # one pair of codes for the whole text
    sizes = [len(m) for m in _members(blob)]
    assert max(sizes) <= 65536 and max(sizes[1::3]) > 14 * CHUNK // 8     # (14 bits a byte at least: these bytes have 14- and 15-bit codes)
    unseen = [t for t in seen[1].tokens() if t[0] == "lit"]
    assert all(lens[t[1]] >= 14 for t in unseen) and len(unseen) > CHUNK - 200


# ---------------------------------------------------------------------------------------------------------------------
# seeded mixtures
# ---------------------------------------------------------------------------------------------------------------------
def test_seeded_mixtures(eng):
    seeds = D.seeds(range(1, 201))
    assert len(seeds) >= 200 or os.environ.get("SIMU_DEFLATE_SEEDS")
    for seed in seeds:
        check(eng, T.mixture(seed), "mixture of seed %d" % seed)


# ---------------------------------------------------------------------------------------------------------------------
# natural text from profile shapes the shipped profiles lack
# ---------------------------------------------------------------------------------------------------------------------
NATURAL = [Shape(1, 50, n_qual_mass=1), Shape(3, 30, n_qual_mass=70), Shape(1, 702, read_length=1000, n_qual_mass=4)]


@pytest.mark.parametrize("contig", ["homopolymer", "period2"])
@pytest.mark.parametrize("shape", NATURAL, ids=[s.tag for s in NATURAL])
def test_natural_text_of_other_profile_shapes(eng, shape, contig, tmp_path):
    """through Session and sg_compress, as test_gpu_gzip.py does: one quality symbol a row, 70 symbols, reads of 1,000
    bases, over a contig of one base and one of period 2"""
    wd = str(tmp_path)
    prof = PS.write_profile(os.path.join(wd, shape.tag + ".profile"), shape)
    fa = os.path.join(wd, "ref.fa")
    cases._fasta_of(fa, [(b"chr1", b"A" * 60000 if contig == "homopolymer" else b"AC" * 30000)])
    cfg = os.path.join(wd, "config.txt")
    L = shape.read_length
    cases._config(cfg, ref=fa, profile=prof, name="n", output=os.path.join(wd, "out"), layout="PE", threads=1, verbose=0,
                  coverage=max(2, round(1200.0 / L)), insertSize=max(350, 2 * L + 50))
    sess = simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=77)
    try:
        sess.weighted_length()
        sess.set_reads(sess.planned_reads)
        done = 0
        for chrom in range(sess.n_chromosomes):
            if not sess.prepare_batch(chrom):
                continue
            sess.sample()
            b1, b2, nf = sess.result()
            t1, t2 = sess.fetch(b1, b2)
            g1, g2 = sess.compress()
            for mate, text, gz in ((0, t1, g1), (1, t2, g2)):
                assert text and len(text) > 3 * CHUNK
                blob = sess.fetch_compressed(mate, gz)
                check_blob(eng, text, blob, "%s %s mate %d" % (shape.tag, contig, mate + 1), tokens=(0, 1, -1))
                assert _deflate(eng, text) == blob          # the buffer-in entry writes what sg_compress writes
            done += 1
        assert done
    finally:
        sess.close()
