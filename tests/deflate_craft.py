"""DEFLATE streams that zlib's compressor never writes (RFC 1951), for the tests of the device inflate (sg_inflate.hip).

  Stream            a bit-level writer: stored, fixed and dynamic blocks; the code lengths (literal/length, distance,
                    code-length code) are the caller's, the tokens are explicit, and the header fields HLIT / HDIST / HCLEN
                    and the run-length items of the length sequence can be overridden
  directed()        a named corpus: every shape the decoder has separate code for, each legal case beside its illegal neighbour
  generate(seed)    a legal multi-block stream of random complete codes up to 15 bits deep; its compressed size is bounded
                    while it is written, so that it always fits a BGZF member and no stream is ever dropped
  mutate(raw, rng)  1 to 3 bit flips biased to the block headers, or a cut
  reference(raw)    what zlib.decompressobj(-15) makes of a raw stream: the verdict every test compares with
  member(raw, ...)  the stream in a BGZF member whose CRC-32 and ISIZE are those of zlib's output

Tokens of a block: an int is a literal; (ls, lx, ds, dx) is a match of length symbol 257 + ls with extra bits lx at distance
symbol ds with extra bits dx; ("L", sym) is a bare literal/length symbol with nothing behind it; ("bits", v, n) are n raw bits."""
import os
import random
import struct
import zlib

MAXI = 65536                 # output bytes a BGZF member may hold
MAX_RAW = 65536 - 26         # raw DEFLATE bytes a member may hold: BSIZE + 1 <= 65536 with an 18-byte header and the trailer
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

# ISIZE of the CRC sweep: every lane count of the CRC tree's first level, every size on and beside the edge where the four
# bytes that carry the ~0 start straddle two lanes (ISIZE mod 1024 in 1..3), and the largest sizes a member may have
CRC_SIZES = sorted(set(range(0, 2101)) | {k * 1024 + d for k in range(1, 64) for d in (-1, 0, 1, 2, 3, 4)} | {65281, 65533, 65534, 65535, 65536})


def match_len(t):
    return LEN_BASE[t[0]] + t[1]


def match_dist(t):
    return DIST_BASE[t[2]] + t[3]


def canon(lens):
    """{symbol: (code, length)} of the canonical code of `lens` (RFC 1951 3.2.2); a set that is no prefix code still gets codes"""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for n in range(1, 17):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n] & ((1 << n) - 1), n)
            nxt[n] += 1
    return out


def chain(symbols):
    """lengths 1, 2, ..., n - 1, n - 1 of a complete code over n >= 2 symbols: the deepest tree they can make"""
    n = len(symbols)
    return {s: min(i + 1, n - 1) for i, s in enumerate(symbols)}


def balanced(symbols):
    """a complete code over the symbols with all lengths within one of each other (one symbol: a second one is added)"""
    symbols = list(symbols)
    if len(symbols) < 2:
        symbols.append(next(s for s in range(19) if s not in symbols))
    depth = [0]
    while len(depth) < len(symbols):
        d = depth.pop(depth.index(min(depth)))
        depth += [d + 1, d + 1]
    return dict(zip(symbols, sorted(depth)))


def random_complete(rng, symbols, maxlen):
    """a random complete code over the symbols that reaches depth maxlen where they are enough for it (n > maxlen); maxlen is
    raised to what the number of symbols needs"""
    symbols = list(symbols)
    n = len(symbols)
    assert n >= 2
    maxlen = max(maxlen, (n - 1).bit_length())
    spine = min(maxlen, n - 1)
    depth = list(range(1, spine + 1)) + [spine]
    while len(depth) < n:
        c = [i for i, d in enumerate(depth) if d < maxlen]
        i = max(c, key=lambda j: depth[j]) if rng.random() < 0.5 else rng.choice(c)
        d = depth.pop(i)
        depth += [d + 1, d + 1]
    rng.shuffle(depth)
    return dict(zip(symbols, depth))


def rle_items(seq, rng=None):
    """the length sequence as items (symbol, extra bits' value): runs of zeros as 17 / 18, runs of a length as 16 behind one
    copy of it.  The sequence is the literal/length lengths and the distance lengths together: runs cross between them."""
    items, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        plain = rng is not None and rng.random() < 0.1
        if v == 0 and run >= 3 and not plain:
            r = min(run, 138)
            items.append((18, r - 11) if r >= 11 else (17, r - 3))
            i += r
        elif v and run >= 4 and not plain:
            r = min(run - 1, 6)
            items += [(v, 0), (16, r - 3)]
            i += 1 + r
        else:
            items.append((v, 0))
            i += 1
    return items


class Stream:
    """One raw DEFLATE stream under construction.  `blocks` is what a decoder should make of it: ("stored", bytes) and
    ("tokens", [...]) in order; `used_lit` / `used_dist` are the longest codes the tokens written so far used."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()
        self.blocks = []
        self.used_lit = self.used_dist = 0

    # ---- bits ----
    def put(self, v, n):                 # LSB first: header fields, extra bits
        assert 0 <= v < 1 << n or n == 0 and v == 0, (v, n)
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, cl):                  # a Huffman code, most significant bit first
        c, n = cl
        for i in range(n - 1, -1, -1):
            self.put((c >> i) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bits(self):
        return len(self.out) * 8 + self.n

    def raw(self):
        self.align()
        return bytes(self.out)

    # ---- blocks ----
    def header(self, final, kind):
        self.put(1 if final else 0, 1)
        self.put(kind, 2)

    def stored(self, data, final=False, length=None, nlen=None):
        """a stored block; `length` / `nlen` override LEN and NLEN (nlen is the 16-bit value written, not its complement)"""
        self.header(final, 0)
        self.align()
        n = len(data) if length is None else length
        self.put(n, 16)
        self.put(n ^ 0xFFFF if nlen is None else nlen, 16)
        self.out += data
        self.blocks.append(("stored", bytes(data)))

    def token(self, t, lc, dc):
        if isinstance(t, int):
            self.code(lc[t])
            self.used_lit = max(self.used_lit, lc[t][1])
        elif t[0] == "L":
            self.code(lc[t[1]])
        elif t[0] == "bits":
            self.put(t[1], t[2])
        else:
            ls, lx, ds, dx = t
            self.code(lc[257 + ls])
            self.put(lx, LEN_EXTRA[ls])
            self.code(dc[ds])
            self.put(dx, DIST_EXTRA[ds] if ds < 30 else 0)
            self.used_lit = max(self.used_lit, lc[257 + ls][1])
            self.used_dist = max(self.used_dist, dc[ds][1])

    def fixed(self, tokens, final=False, end=True):
        self.header(final, 1)
        lc, dc = canon(FIXED_LIT), canon(FIXED_DIST)
        for t in tokens:
            self.token(t, lc, dc)
        if end:
            self.code(lc[256])
        self.blocks.append(("tokens", list(tokens)))

    def dynamic_header(self, ll, dl, final=False, cl=None, hlit=None, hdist=None, hclen=None, items=None, rng=None):
        """the header of a dynamic block for the literal/length lengths `ll` and distance lengths `dl` ({symbol: length});
        returns the two codes.  cl: lengths of the code-length code (default: a balanced complete code over the items'
        symbols); items: the run-length items (default: rle_items of the whole sequence); hlit / hdist / hclen: the counts
        written in the header and the number of lengths written, whatever the lengths say."""
        hlit = max(max(ll, default=0) + 1, 257) if hlit is None else hlit
        hdist = max(max(dl, default=0) + 1, 1) if hdist is None else hdist
        seq = [ll.get(i, 0) for i in range(hlit)] + [dl.get(i, 0) for i in range(hdist)]
        if items is None:
            items = rle_items(seq, rng)
        if cl is None:
            used = sorted({a for a, _ in items})
            cl = random_complete(rng, used, 7) if rng is not None and len(used) >= 2 else balanced(used)
        if hclen is None:
            hclen = max(4, max(CLEN_ORDER.index(s) for s in cl) + 1)
        self.header(final, 2)
        self.put(hlit - 257, 5)
        self.put(hdist - 1, 5)
        self.put(hclen - 4, 4)
        for k in range(hclen):
            self.put(cl.get(CLEN_ORDER[k], 0), 3)
        cc = canon([cl.get(i, 0) for i in range(19)])
        for a, x in items:
            self.code(cc[a])
            self.put(x, {16: 2, 17: 3, 18: 7}.get(a, 0))
        return canon([ll.get(i, 0) for i in range(max(hlit, 288))]), canon([dl.get(i, 0) for i in range(max(hdist, 32))])

    def dynamic(self, tokens, ll, dl, final=False, end=True, **header):
        lc, dc = self.dynamic_header(ll, dl, final, **header)
        for t in tokens:
            self.token(t, lc, dc)
        if end:
            self.code(lc[256])
        self.blocks.append(("tokens", list(tokens)))


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
NO_EOF, TOO_LONG = "stream does not reach eof", "output exceeds 65536 bytes"


def reference(raw):
    """(legal, output, outcome) of zlib.decompressobj(-15) on a raw stream: legal when zlib reaches eof with at most 65536
    bytes of output; otherwise the outcome is zlib's message (without its prefix), NO_EOF or TOO_LONG, and the output is
    what zlib had made of the stream until then."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(raw, MAXI + 1024)
    except zlib.error as e:
        msg = str(e).split(": ", 1)[1] if ": " in str(e) else str(e)
        d, out, step = zlib.decompressobj(-15), b"", max(16, len(raw) // 64)
        try:   # again in small steps, for the bytes made before the error
            for i in range(0, len(raw), step):
                out += d.decompress(raw[i:i + step], MAXI + 1024 - len(out))
        except zlib.error:
            pass
        return False, out, msg
    if len(out) > MAXI:
        return False, out, TOO_LONG
    if not d.eof:
        return False, out, NO_EOF
    return True, out, None


def member(raw, out=None, extra=b"", flags=4, tail=b""):
    """`raw` in a BGZF member: the BC subfield behind `extra` (other subfields), CRC-32 and ISIZE of `out` (default: what
    zlib makes of raw; of more than 64 KiB the first 64 KiB, so that ISIZE is one the member walk lets through and only the
    decoder can refuse it); `tail` goes between the header and the data (FNAME ...)"""
    if out is None:
        out = reference(raw)[1]
    out = out[:MAXI]
    xlen = len(extra) + 6
    bsize = 12 + xlen + len(tail) + len(raw) + 8 - 1
    assert bsize < 65536, "the stream does not fit a member"
    return (b"\x1f\x8b\x08" + bytes([flags]) + b"\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra + b"BC" + struct.pack("<HH", 2, bsize) + tail + raw +
            struct.pack("<II", zlib.crc32(out) & 0xFFFFFFFF, len(out)))


def crc_payload(n):
    """n bytes that compress well, differ in each of the first eight positions, and differ from size to size"""
    return (bytes([0x31, 0x7A, 0x05, 0xC4, 0x9B, 0x62, 0xE8, 0x1D]) + b"%d:" % n + b"GATTACA-CATTAG+" * (n // 15 + 1))[:n]


# ---------------------------------------------------------------------------------------------------------------------
# the directed corpus
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, stream, outcome=None, raw=None, note=""):
        self.name, self.outcome, self.note = name, outcome, note   # outcome: None = legal, else zlib's message / NO_EOF / TOO_LONG
        self.raw = stream.raw() if raw is None else raw
        self.blocks = stream.blocks if outcome is None else None
        self.legal = outcome is None
        self.fits = len(self.raw) <= MAX_RAW


def _fill(n, have=0):
    """tokens of a fixed block that make n bytes in few bits: matches of length 258 at distance 1 (behind one literal where
    nothing has been written yet), a shorter match, literals"""
    toks, left = [], n
    if left and not have:
        toks.append(0x41)
        left -= 1
    while left >= 258:
        toks.append((28, 0, 0, 0))
        left -= 258
    if left >= 3:
        ls = max(i for i in range(28) if LEN_BASE[i] <= left)
        lx = min(left - LEN_BASE[ls], (1 << LEN_EXTRA[ls]) - 1)
        toks.append((ls, lx, 0, 0))
        left -= LEN_BASE[ls] + lx
    return toks + [0x42] * left


def directed():
    """The corpus, in a fixed order.  Names are unique; a case found by these tests keeps its name for good."""
    out = []

    def add(name, build, outcome=None, tail=b"", cut=None, note=""):
        s = Stream()
        build(s)
        raw = s.raw() + tail
        if cut is not None:
            raw = raw[:cut] if cut >= 0 else raw[:len(raw) + cut]
        out.append(Case(name, s, outcome, raw, note))

    a, b, c = 0x61, 0x62, 0x63
    # ---- codes longer than the 10-bit look-up table ----
    lit16 = [a, b, c, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x6B, 0, 255, 257, 285, 256]     # lengths 1..15, 15
    dist16 = list(range(14)) + [28, 29]
    deep_tokens = lit16[:13] * 3 + [(0, 0, d, 0) for d in range(4)] + [(28, 0, 0, 0)] * 130 + [(28, 0, 28, 0), (28, 0, 29, 8191), (0, 0, 13, 31)] + lit16[:13]
    add("codes_of_1_to_15_bits", lambda s: s.dynamic(deep_tokens, chain(lit16), chain(dist16), final=True))
    rev = lit16[::-1]
    add("deepest_codes_for_the_commonest_literals", lambda s: s.dynamic([t for t in deep_tokens if isinstance(t, int)] * 4,
                                                                          chain(rev[:1] + rev[3:] + rev[1:3]), {}, final=True))
    # ---- distance codes of one code and of none ----
    add("one_distance_code_of_length_1_used", lambda s: s.dynamic([a, b, c, (0, 0, 2, 0), (5, 0, 2, 0)], balanced([a, b, c, 256, 257, 262]), {2: 1}, final=True))
    add("one_distance_code_of_length_1_other_bit", lambda s: s.dynamic([a, b, c, ("L", 257), ("bits", 1, 1), a], balanced([a, b, c, 256, 257, 262]), {2: 1}, final=True),
        "invalid distance code", note="the bit matches no code of the distance code")
    add("no_distance_code_literals_only", lambda s: s.dynamic([a, b, c] * 50, balanced([a, b, c, 256]), {}, final=True))
    add("no_distance_code_but_a_match", lambda s: s.dynamic([a, b, c, ("L", 257), ("bits", 0, 1), a], balanced([a, b, c, 256, 257]), {}, final=True),
        "invalid distance code", note="the bit matches no code of the distance code")
    add("one_literal_code_of_length_1_empty_block", lambda s: s.dynamic([], {256: 1}, {}, final=True))
    add("one_literal_code_of_length_1_other_bit", lambda s: s.dynamic([("bits", 1, 1)], {256: 1}, {}, final=True, end=False), "invalid literal/length code")
    # ---- runs of the length sequence ----
    ll4, dl4 = {a: 2, b: 2, 256: 2, 257: 2}, {0: 2, 1: 2, 2: 2, 3: 2}
    cross16 = [(18, 97 - 11), (2, 0), (2, 0), (18, 138 - 11), (18, 157 - 138 - 11), (2, 0), (16, 5 - 3)]
    add("run_of_16_crosses_into_the_distance_lengths", lambda s: s.dynamic([a, b, a, (0, 0, 2, 0), (0, 0, 3, 0)], ll4, dl4, final=True, items=cross16))
    ll3, dl3 = {a: 1, 256: 2, 257: 2}, {2: 1, 3: 1}
    cross17 = [(18, 97 - 11), (1, 0), (18, 138 - 11), (18, 158 - 138 - 11), (2, 0), (2, 0), (17, 4 - 3), (1, 0), (1, 0)]
    add("run_of_17_crosses_into_the_distance_lengths", lambda s: s.dynamic([a, a, a, (0, 0, 2, 0), (0, 0, 3, 0)], ll3, dl3, final=True, hlit=260, items=cross17))
    ll0 = {0: 3, 1: 3, 2: 3, 3: 3, 4: 3, 5: 3, 256: 3, 257: 3}
    add("run_of_16_as_second_item", lambda s: s.dynamic([0, 1, 2, (0, 0, 0, 0)], ll0, {0: 1}, final=True,
                                                        items=[(3, 0), (16, 2), (18, 127), (18, 250 - 138 - 11), (3, 0), (3, 0), (1, 0)]))
    add("run_of_16_as_first_item", lambda s: s.dynamic([0, 1, 2], ll0, {0: 1}, final=True, items=[(16, 3), (18, 127), (18, 250 - 138 - 11), (3, 0), (3, 0), (1, 0)],
                                                       cl=balanced([16, 18, 3, 1])), "invalid bit length repeat")
    add("run_of_18_past_the_last_length", lambda s: s.dynamic([0, 1, 2], ll0, {0: 1}, final=True,
                                                              items=[(3, 0), (16, 2), (18, 127), (18, 250 - 138 - 11), (3, 0), (3, 0), (18, 0)]), "invalid bit length repeat")
    # ---- HLIT, HDIST ----
    full_lit = balanced([a, b, 256, 285])
    add("hlit_286", lambda s: s.dynamic([a, b, a, b, (28, 0, 3, 0)], full_lit, {3: 1}, final=True))
    add("hlit_287", lambda s: s.dynamic([a, b], full_lit, {3: 1}, final=True, hlit=287), "too many length or distance symbols")
    add("hlit_288", lambda s: s.dynamic([a, b], full_lit, {3: 1}, final=True, hlit=288), "too many length or distance symbols")
    add("hdist_30", lambda s: s.dynamic([a, b, a, b, (0, 0, 3, 0)], balanced([a, b, 256, 257]), {3: 1, 29: 1}, final=True))
    add("hdist_31", lambda s: s.dynamic([a, b], full_lit, {3: 1, 29: 1}, final=True, hdist=31), "too many length or distance symbols")
    add("hdist_32", lambda s: s.dynamic([a, b], full_lit, {3: 1, 29: 1}, final=True, hdist=32), "too many length or distance symbols")
    # ---- the three codes: complete, incomplete, over-subscribed ----
    items0 = [(3, 0), (16, 2), (18, 127), (18, 250 - 138 - 11), (3, 0), (3, 0), (1, 0)]
    add("code_length_code_complete", lambda s: s.dynamic([0, 1, 2], ll0, {0: 1}, final=True, items=items0, cl={3: 2, 16: 2, 18: 2, 1: 2}))
    add("code_length_code_incomplete", lambda s: s.dynamic([0, 1, 2], ll0, {0: 1}, final=True, items=items0, cl={3: 2, 16: 2, 18: 2, 1: 3}), "invalid code lengths set")
    add("code_length_code_over_subscribed", lambda s: s.dynamic([0, 1, 2], ll0, {0: 1}, final=True, items=items0, cl={3: 2, 16: 2, 18: 2, 1: 2, 0: 2}),
        "invalid code lengths set")
    add("literal_code_incomplete", lambda s: s.dynamic([a, b], {a: 2, b: 2, 256: 2}, {0: 1}, final=True), "invalid literal/lengths set")
    add("literal_code_over_subscribed", lambda s: s.dynamic([a, b], {a: 1, b: 1, 256: 1}, {0: 1}, final=True), "invalid literal/lengths set")
    add("distance_code_incomplete", lambda s: s.dynamic([a, b], ll4, {0: 2, 1: 2, 2: 2}, final=True), "invalid distances set")
    add("distance_code_over_subscribed", lambda s: s.dynamic([a, b], ll4, {0: 1, 1: 1, 2: 1}, final=True), "invalid distances set")
    add("no_end_of_block_code", lambda s: s.dynamic([a, b], {a: 1, b: 1}, {0: 1}, final=True, end=False, hlit=257), "invalid code -- missing end-of-block")
    # ---- fixed codes: the symbols that take part in the code and may not occur ----
    add("fixed_block_of_every_literal", lambda s: s.fixed(list(range(256)) + [(0, 0, 0, 0), (27, 31, 4, 1)], final=True))
    add("fixed_symbol_286", lambda s: s.fixed([a, ("L", 286), a], final=True), "invalid literal/length code")
    add("fixed_symbol_287", lambda s: s.fixed([a, ("L", 287), a], final=True), "invalid literal/length code")
    add("fixed_distance_code_30", lambda s: s.fixed([a, (0, 0, 30, 0), a], final=True), "invalid distance code")
    add("fixed_distance_code_31", lambda s: s.fixed([a, (0, 0, 31, 0), a], final=True), "invalid distance code")
    add("length_258_as_symbol_284_extra_31", lambda s: s.fixed([a, b, (27, 31, 1, 0), (27, 31, 0, 0), (28, 0, 1, 0)], final=True))
    # ---- distances ----
    add("distance_equals_bytes_written", lambda s: s.fixed([a, b, c, (0, 0, 2, 0), (3, 0, 4, 1), (28, 0, 6, 3)], final=True))
    add("distance_one_more_than_bytes_written", lambda s: s.fixed([a, b, c, (0, 0, 3, 0)], final=True), "invalid distance too far back")
    add("distance_in_an_empty_output", lambda s: s.fixed([(0, 0, 0, 0)], final=True), "invalid distance too far back")
    add("distance_32768_at_32768", lambda s: (s.fixed([a, b, c] + _fill(32765)), s.fixed([(28, 0, 29, 8191), (0, 0, 29, 8191)], final=True)))
    add("distance_32768_at_32767", lambda s: (s.fixed([a, b, c] + _fill(32764)), s.fixed([(28, 0, 29, 8191)], final=True)), "invalid distance too far back")
    add("distance_32768_across_a_stored_block", lambda s: (s.fixed([a, b, c]), s.stored(bytes(range(256)) * 128 + b"xyz"), s.fixed([(28, 0, 29, 8191)] * 3, final=True)))
    # ---- the end of the output ----
    add("match_ends_at_65536", lambda s: (s.fixed([a, b, c] + _fill(65536 - 3 - 258)), s.fixed([(28, 0, 29, 8191)], final=True)))
    add("match_ends_at_65537", lambda s: (s.fixed([a, b, c] + _fill(65537 - 3 - 258)), s.fixed([(28, 0, 29, 8191)], final=True)), TOO_LONG)
    add("short_match_ends_at_65536", lambda s: (s.fixed([a, b, c] + _fill(65530)), s.fixed([(0, 0, 2, 0)], final=True)))
    add("short_match_ends_at_65537", lambda s: (s.fixed([a, b, c] + _fill(65531)), s.fixed([(0, 0, 2, 0)], final=True)), TOO_LONG)
    add("literal_ends_at_65536", lambda s: (s.fixed(_fill(65535)), s.fixed([c], final=True)))
    add("literal_ends_at_65537", lambda s: (s.fixed(_fill(65536)), s.fixed([c], final=True)), TOO_LONG)
    add("stored_ends_at_65536", lambda s: (s.fixed(_fill(65536 - 700)), s.stored(bytes(range(100)) * 7, final=True)))
    add("stored_ends_at_65537", lambda s: (s.fixed(_fill(65537 - 700)), s.stored(bytes(range(100)) * 7, final=True)), TOO_LONG)
    # ---- stored blocks ----
    add("stored_of_0_bytes", lambda s: (s.stored(b""), s.fixed([a]), s.stored(b""), s.stored(b"", final=True)))
    add("stored_of_65535_bytes", lambda s: s.stored(bytes(range(255)) * 257, final=True), note="five bytes more than a member holds: for zlib alone")
    add("stored_that_fills_the_member", lambda s: s.stored((bytes(range(251)) * 262)[:MAX_RAW - 5], final=True))
    add("stored_of_65535_bytes_past_the_member", lambda s: s.stored(bytes(range(255)) * 4, final=True, length=65535), NO_EOF)
    add("stored_partly_in_the_bit_buffer_partly_past_the_member", lambda s: s.stored(b"ab", final=True, length=20), NO_EOF)
    add("stored_of_3_of_4_bytes", lambda s: (s.fixed([a, b]), s.stored(b"abc", final=True, length=4)), NO_EOF)
    add("stored_len_is_not_the_complement_of_nlen", lambda s: s.stored(b"abcd", final=True, nlen=4 ^ 0xFFFF ^ 0x0100), "invalid stored block lengths")
    add("stored_len_0_nlen_0", lambda s: s.stored(b"", final=True, nlen=0), "invalid stored block lengths")
    for k in range(8):   # a stored block behind every bit offset
        add("stored_behind_%d_one_bit_literals" % k, lambda s, k=k: (s.dynamic([a] * k, {a: 1, 256: 1}, {}), s.stored(b"0123456789", final=True)))
    # ---- block type, the end of the data ----
    add("block_type_3", lambda s: (s.fixed([a]), s.header(True, 3), s.put(0, 5)), "invalid block type")
    add("no_final_block", lambda s: (s.fixed([a, b, c]), s.stored(b"abc")), NO_EOF)
    add("data_ends_in_a_symbol", lambda s: s.dynamic(deep_tokens[:30], chain(lit16), chain(dist16), final=True), NO_EOF, cut=-3)
    add("data_ends_in_a_dynamic_header", lambda s: s.dynamic([a, b], ll4, dl4, final=True), NO_EOF, cut=6)
    add("no_data_at_all", lambda s: s.fixed([a], final=True), NO_EOF, cut=0)
    add("bytes_left_before_the_trailer", lambda s: s.fixed([a, b, c, (2, 0, 2, 0)], final=True), tail=b"\xaa\x55\x00\xff\x01")
    add("a_whole_stream_left_before_the_trailer", lambda s: s.fixed([a, b, c], final=True), tail=zlib.compress(b"another", 6)[2:-4])
    names = [c_.name for c_ in out]
    assert len(set(names)) == len(names)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------
GEN_SIZES = (0, 1, 3, 4, 300, 1025, 5000, 65533, 65536)
GEN_DEPTHS = (7, 9, 10, 11, 15)
_BUDGET = MAX_RAW * 8
_HEADER_BITS = 17 + 19 * 3 + 316 * 14   # the most a dynamic header takes: every length an item of 7 + 7 bits


def _fill_bits(n):
    """an upper bound of the bits a final fixed block of _fill(n) takes, with its header and end-of-block code"""
    return 3 + 9 + 13 * (n // 258) + 18 + 2 * 9 + 7 + 7   # (+ 7: the padding of the last byte)


def _random_match(rng, have, room, ls_ok, ds_ok):
    """a match of the given symbols that fits `have` bytes written and `room` bytes left; None if there is none"""
    ls_c = [x for x in ls_ok if LEN_BASE[x] <= room]
    ds_c = [x for x in ds_ok if DIST_BASE[x] <= have]
    if not ls_c or not ds_c:
        return None
    bias = [x for x in (0, 7, 8, 27, 28) if x in ls_c]
    ls = rng.choice(bias) if bias and rng.random() < 0.6 else rng.choice(ls_c)
    top = min((1 << LEN_EXTRA[ls]) - 1, room - LEN_BASE[ls])
    lx = rng.choice((0, top, rng.randrange(top + 1)))
    ds = rng.choice((ds_c[0], ds_c[-1], ds_c[-1], rng.choice(ds_c)))
    top = min((1 << DIST_EXTRA[ds]) - 1, have - DIST_BASE[ds])
    dx = rng.choice((0, top, top, rng.randrange(top + 1)))
    return (ls, lx, ds, dx)


def generate(seed, total=None):
    """One legal stream of 1 to 4 random blocks and a closing block, `total` bytes of output (default: drawn from GEN_SIZES).
    Returns the Stream.  While it is written the bits are counted: a token, or a block, is only started when the stream can
    still be closed within MAX_RAW bytes behind it (by _fill, 13 bits for 258 bytes), so no stream is ever over the size."""
    rng = random.Random(seed)
    s = Stream()
    s.seed = seed
    total = rng.choice(GEN_SIZES) if total is None else total
    have = 0
    nblocks = rng.randrange(1, 5)
    for bi in range(nblocks):
        left = total - have
        target = left if bi == nblocks - 1 else rng.randrange(0, left + 1)
        kind = rng.randrange(4)
        if s.bits() + _HEADER_BITS + 64 + _fill_bits(left) > _BUDGET:
            break
        if kind == 0:      # stored
            n = min(target, 65535, max(0, (_BUDGET - s.bits() - 64 - _fill_bits(left)) // 8 - 8), rng.choice((target, 40000, 700)))
            period = bytes(rng.randrange(256) for _ in range(min(n, 64) if n > 2000 else n))   # (a long one repeats 64 random bytes)
            s.stored((period * (n // max(len(period), 1) + 1))[:n])
            have += n
            continue
        # the codes first, over the symbols the tokens may use and unused ones that make the tables large
        lits = set(rng.sample(range(256), rng.choice((1, 2, 5, 40, 256)))) | {0, 255}
        ls_ok = sorted(set(rng.sample(range(29), rng.randrange(1, 29))) | set(rng.sample((0, 7, 8, 27, 28), rng.randrange(1, 6))))
        ds_ok = sorted(set(rng.sample(range(30), rng.randrange(2, 20))) | {0, 29} | set(range(rng.choice((0, 16, 30)))))
        maxlen = rng.choice(GEN_DEPTHS)
        ll = random_complete(rng, sorted(lits | {256} | {257 + x for x in ls_ok}), maxlen)
        dl = random_complete(rng, ds_ok, maxlen)
        lc, dc = s.dynamic_header(ll, dl, rng=rng)
        toks, made = [], 0
        p_match = rng.choice((0.1, 0.5, 0.9)) if total < 10000 else 0.97
        lit_pool = sorted(lits)
        while made < target:
            t = _random_match(rng, have + made, target - made, ls_ok, ds_ok) if have + made and rng.random() < p_match else None
            if t is None:
                t = rng.choice((0, 255, rng.choice(lit_pool)))
            n = 1 if isinstance(t, int) else match_len(t)
            cost = lc[t][1] if isinstance(t, int) else lc[257 + t[0]][1] + LEN_EXTRA[t[0]] + dc[t[2]][1] + DIST_EXTRA[t[2]]
            if s.bits() + cost + 15 + _fill_bits(total - have - made - n) > _BUDGET:
                break
            s.token(t, lc, dc)
            toks.append(t)
            made += n
        s.code(lc[256])
        s.blocks.append(("tokens", toks))
        have += made
    # the closing block: what is left in the cheapest way, or an empty block of any kind
    left = total - have
    kind = rng.randrange(3)
    if left or kind == 0:
        s.fixed(_fill(left, have), final=True)
    elif kind == 1:
        s.stored(b"", final=True)
    else:
        s.dynamic([], {256: 1, 0: 1}, {}, final=True)
    assert s.bits() <= _BUDGET
    s.total = total
    return s


# ---------------------------------------------------------------------------------------------------------------------
# the mutator
# ---------------------------------------------------------------------------------------------------------------------
def mutate(raw, rng):
    """`raw` with 1 to 3 bits flipped -- two in five of the flips in the first 40 or 400 bits, where the block header and the
    code lengths are -- or, one time in ten, cut short"""
    if len(raw) > 1 and rng.random() < 0.1:
        return raw[:rng.randrange(1, len(raw))]
    x = bytearray(raw)
    nbits = len(x) * 8
    for _ in range(rng.choice((1, 1, 2, 3))):
        bit = rng.randrange(min(nbits, rng.choice((40, 400, nbits, nbits, nbits))))
        x[bit >> 3] ^= 1 << (bit & 7)
    return bytes(x)


def zlib_made(seed):
    """a raw stream from zlib's compressor: text, a few symbols, or random bytes, at a level and strategy of the seed's"""
    rng = random.Random(seed)
    n = rng.choice((0, 1, 20, 300, 3000))
    kind = rng.randrange(3)
    data = bytes(rng.choice(b"ACGT\n@+#FJ:1234") for _ in range(n)) if kind == 0 else bytes(rng.choice(b"AC") for _ in range(n)) if kind == 1 else \
        bytes(rng.randrange(256) for _ in range(n))
    c = zlib.compressobj(rng.choice((0, 1, 6, 9)), zlib.DEFLATED, -15, 9, rng.choice((zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE)))
    return c.compress(data) + c.flush()


def seeds(default):
    """the seeds of the generator and the mutator: SIMU_DEFLATE_SEEDS=a-b widens the hunt"""
    env = os.environ.get("SIMU_DEFLATE_SEEDS")
    if env:
        lo, hi = env.split("-")
        return list(range(int(lo), int(hi) + 1))
    return list(default)


GEN_SEEDS = range(1, 181)        # generate(seed)
MUT_SEEDS = range(1, 241)        # per seed: one zlib-made and one generated stream (300, 1,025 or 5,000 bytes of output: smaller ones are all header), four mutations of each
MUT_PER_STREAM = 4


def mutated(seed_list):
    """[(label, source, raw)]: source is "zlib" or "craft"; the label names the seed and the mutation"""
    out = []
    for seed in seed_list:
        rng = random.Random(seed * 7919 + 1)
        for source, raw in (("zlib", zlib_made(seed)), ("craft", generate(seed, total=(300, 1025, 5000)[seed % 3]).raw())):
            for k in range(MUT_PER_STREAM):
                out.append(("%s seed %d mutation %d" % (source, seed, k), source, mutate(raw, rng)))
    return out
