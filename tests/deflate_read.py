"""A reader of one raw DEFLATE stream (RFC 1951) that keeps what zlib throws away: for every block its type, the code
lengths and the TOKENS -- which bytes left as literals, which as matches of what length from how far back.  The tests of
the device compressor (test_gpu_deflate_texts.py) assert token lists with it; every other member goes through zlib.
Written to be read, not to be fast: one bit at a time.

  read(raw) -> Stream
    .blocks   [Block]: .final, .kind (0 stored, 1 fixed, 2 dynamic), .lit_lens / .dist_lens (code lengths by symbol; None in
              a stored block), .tokens (("lit", byte) | ("match", length, distance) | ("end",)), .stored (bytes of a stored
              block), and, for writing the block again with deflate_craft.Stream: .craft (the tokens as that writer takes
              them: the length and distance SYMBOLS with their extra bits) and .header (hlit, hdist, hclen, cl, items)
    .out      the expansion of the tokens (a match copies byte by byte, so it may overlap what it writes)
    .end      bytes of `raw` the stream takes (what lies behind is not looked at)
    .tokens() the tokens of all blocks in one list
  rewrite(stream) -> the same bytes again, from the blocks alone (tests/test_deflate_read_cpu.py holds the two together)

A stream that is not legal raises ValueError: this is a reader for streams a test has reason to believe in, not a judge."""
import deflate_craft as D


class Block:
    def __init__(self, final, kind):
        self.final, self.kind = final, kind
        self.lit_lens = self.dist_lens = None
        self.tokens, self.craft = [], []
        self.stored = None
        self.header = None


class Stream:
    def __init__(self):
        self.blocks, self.out, self.end = [], bytearray(), 0

    def tokens(self):
        return [t for b in self.blocks for t in b.tokens]


class _Bits:
    def __init__(self, raw):
        self.raw, self.pos = raw, 0

    def bit(self):
        if self.pos >> 3 >= len(self.raw):
            raise ValueError("the stream ends inside a block")
        b = (self.raw[self.pos >> 3] >> (self.pos & 7)) & 1
        self.pos += 1
        return b

    def take(self, n):                   # a field: least significant bit first
        v = 0
        for i in range(n):
            v |= self.bit() << i
        return v

    def symbol(self, table):             # a Huffman code: most significant bit first
        code = 0
        for n in range(1, 16):
            code = (code << 1) | self.bit()
            s = table.get((code, n))
            if s is not None:
                return s
        raise ValueError("bits that are no code, before bit %d" % self.pos)


def _decoder(lens):
    return {cl: s for s, cl in D.canon(lens).items()}


def _dynamic_header(r, b):
    hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
    if hlit > 286 or hdist > 30:
        raise ValueError("too many length or distance symbols")
    cl = {}
    for k in range(hclen):
        n = r.take(3)
        if n:
            cl[D.CLEN_ORDER[k]] = n
    cc = _decoder([cl.get(i, 0) for i in range(19)])
    seq, items = [], []
    while len(seq) < hlit + hdist:
        a = r.symbol(cc)
        if a < 16:
            items.append((a, 0))
            seq.append(a)
            continue
        x = r.take({16: 2, 17: 3, 18: 7}[a])
        items.append((a, x))
        if a == 16:
            if not seq:
                raise ValueError("a repeat with nothing to repeat")
            seq += [seq[-1]] * (3 + x)
        else:
            seq += [0] * ((3 if a == 17 else 11) + x)
    if len(seq) != hlit + hdist:
        raise ValueError("a run past the last length")
    b.header = dict(hlit=hlit, hdist=hdist, hclen=hclen, cl=cl, items=items)
    return seq[:hlit], seq[hlit:]


def read(raw):
    r, s = _Bits(bytes(raw)), Stream()
    out = s.out
    while True:
        b = Block(r.bit(), r.take(2))
        s.blocks.append(b)
        if b.kind == 0:
            r.pos = (r.pos + 7) & ~7
            n, nn = r.take(16), r.take(16)
            if n ^ nn != 0xFFFF:
                raise ValueError("invalid stored block lengths")
            at = r.pos >> 3
            if at + n > len(r.raw):
                raise ValueError("the stream ends inside a block")
            b.stored = r.raw[at:at + n]
            out += b.stored
            r.pos += 8 * n
        elif b.kind == 3:
            raise ValueError("invalid block type")
        else:
            if b.kind == 1:
                b.lit_lens, b.dist_lens = list(D.FIXED_LIT), list(D.FIXED_DIST)
            else:
                b.lit_lens, b.dist_lens = _dynamic_header(r, b)
            lit, dist = _decoder(b.lit_lens), _decoder(b.dist_lens)
            while True:
                sym = r.symbol(lit)
                if sym < 256:
                    b.tokens.append(("lit", sym))
                    b.craft.append(sym)
                    out.append(sym)
                elif sym == 256:
                    b.tokens.append(("end",))
                    break
                else:
                    ls = sym - 257
                    if ls > 28:
                        raise ValueError("invalid literal/length code")
                    lx = r.take(D.LEN_EXTRA[ls])
                    ds = r.symbol(dist)
                    if ds > 29:
                        raise ValueError("invalid distance code")
                    dx = r.take(D.DIST_EXTRA[ds])
                    length, distance = D.LEN_BASE[ls] + lx, D.DIST_BASE[ds] + dx
                    if distance > len(out):
                        raise ValueError("invalid distance too far back")
                    b.tokens.append(("match", length, distance))
                    b.craft.append((ls, lx, ds, dx))
                    for _ in range(length):
                        out.append(out[-distance])
        if b.final:
            break
    s.end = (r.pos + 7) >> 3
    s.out = bytes(out)
    return s


def rewrite(stream):
    """the stream written again by deflate_craft.Stream from what read() kept of it"""
    w = D.Stream()
    for b in stream.blocks:
        final = bool(b.final)
        if b.kind == 0:
            w.stored(b.stored, final=final)
        elif b.kind == 1:
            w.fixed(b.craft, final=final)
        else:
            h = b.header
            w.dynamic(b.craft, {i: n for i, n in enumerate(b.lit_lens) if n}, {i: n for i, n in enumerate(b.dist_lens) if n}, final=final,
                      cl=h["cl"], hlit=h["hlit"], hdist=h["hdist"], hclen=h["hclen"], items=h["items"])
    return w.raw()
