"""BAM files for the tests (SAMv1 sections 4.1-4.2), with no samtools / pysam: a writer from SAM fields with BGZF members of
any size and zlib level / strategy, optional fields of every type (SAMv1 section 4.2.4), the lines `samtools view -F 0xD04
-q 20` prints of such a file (the eleven mandatory fields only), and the `bin` of a record (reg2bin, SAMv1 section 5.3)."""
import struct
import zlib

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
OPS = "MIDNSHP=X"
NT16 = "=ACMGRSVTWYHKDBN"
_NT16_CODE = {c: i for i, c in enumerate(NT16)}


def reg2bin(beg, end):
    """The smallest bin of the binning index that holds [beg, end) (0-based, end exclusive)."""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


# ---- BGZF ----
def bgzf_member(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    """One member: gzip header with the BC subfield, raw DEFLATE of `data` (at most 65,280 bytes), CRC-32, ISIZE."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    raw = c.compress(data) + c.flush()
    bsize = 18 + len(raw) + 8 - 1
    assert bsize < 65536, "member too large"
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize) + raw +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def bgzf(data, member=65280, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, eof=True, cuts=None):
    """`data` as BGZF: members of at most `member` input bytes, cut at the offsets `cuts` too; the EOF member behind them."""
    bounds = sorted(set([c for c in (cuts or []) if 0 < c < len(data)] + list(range(0, len(data), member)) + [len(data)]))
    out = [bgzf_member(data[a:b], level, strategy) for a, b in zip(bounds, bounds[1:])]
    return b"".join(out) + (EOF_MEMBER if eof else b"")


def members(buf):
    """(offset, BSIZE, ISIZE) of the whole members of `buf`, and the bytes they make up."""
    out, p = [], 0
    while p + 12 <= len(buf):
        xlen = struct.unpack_from("<H", buf, p + 10)[0]
        if p + 12 + xlen > len(buf):
            break
        q, bsize = p + 12, None
        while q + 4 <= p + 12 + xlen:
            slen = struct.unpack_from("<H", buf, q + 2)[0]
            if buf[q:q + 2] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", buf, q + 4)[0]
            q += 4 + slen
        if p + bsize + 1 > len(buf):
            break
        out.append((p, bsize, struct.unpack_from("<I", buf, p + bsize + 1 - 4)[0]))
        p += bsize + 1
    return out, p


# ---- records ----
def parse_cigar(c):
    if c in (b"*", b""):
        return []
    ops, n = [], b""
    for ch in c:
        ch = bytes([ch])
        if ch.isdigit():
            n += ch
        elif ch.decode() in OPS and n:
            ops.append((int(n), OPS.index(ch.decode())))
            n = b""
        else:
            return None
    return ops if not n else None


def header(refs, text=b""):
    """magic, l_text, text, n_ref, (l_name, name, l_ref) per reference"""
    out = [b"BAM\1", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        out += [struct.pack("<i", len(name) + 1), name + b"\0", struct.pack("<i", length)]
    return b"".join(out)


AUX_FORMAT = {"A": "c", "c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f", "d": "d"}
AUX_ARRAYS = "cCsSiIf"


def aux_tag(tag, ty, value):
    """One optional field: tag (two bytes), a type letter of A c C s S i I f d Z H, or "B" + the element type for an array."""
    if ty in ("Z", "H"):
        return tag + ty.encode() + value + b"\0"
    if ty[0] == "B":
        return tag + b"B" + ty[1].encode() + struct.pack("<I", len(value)) + b"".join(struct.pack("<" + AUX_FORMAT[ty[1]], v) for v in value)
    return tag + ty.encode() + struct.pack("<" + AUX_FORMAT[ty], value)


def aux_every_type(rng):
    """One field of each of the eleven scalar and string types and one array of each of the seven element types: the twelve
    types other than a CG array that a reader steps over, as a list of fields.  Values hold bytes that read as type letters."""
    lo = {"c": -128, "C": 0, "s": -32768, "S": 0, "i": -2 ** 31, "I": 0}
    hi = {"c": 127, "C": 255, "s": 32767, "S": 65535, "i": 2 ** 31 - 1, "I": 2 ** 32 - 1}
    out = [aux_tag(b"XA", "A", bytes([rng.choice(b"ZBHid")]))]
    for k, ty in enumerate("cCsSiI"):
        out.append(aux_tag(b"X%d" % k, ty, rng.choice((lo[ty], hi[ty], rng.randrange(lo[ty], hi[ty] + 1)))))
    out += [aux_tag(b"XF", "f", rng.random() * 100), aux_tag(b"XD", "d", rng.random() * 1e300),
            aux_tag(b"XZ", "Z", bytes(rng.choice(b"CGBIZH ") for _ in range(rng.randrange(0, 40)))),
            aux_tag(b"XH", "H", b"%02X" % rng.randrange(256) * rng.randrange(0, 9))]
    for k, sub in enumerate(AUX_ARRAYS):
        vals = [rng.random() for _ in range(rng.randrange(0, 9))] if sub == "f" else [rng.randrange(lo[sub], hi[sub] + 1) for _ in range(rng.randrange(0, 9))]
        out.append(aux_tag(b"Y%d" % k, "B" + sub, vals))
    return out


def aligner_tags(rng, L):
    """NM:i MD:Z AS:i XS:i RG:Z with seeded values, in the integer widths an aligner's writer picks (the smallest that holds)"""
    def small(tag, v):
        return aux_tag(tag, "C" if v < 256 else "S" if v < 65536 else "I", v)
    md = b"%d%s%d" % (rng.randrange(L), bytes([rng.choice(b"ACGT")]), rng.randrange(L)) if rng.random() < 0.5 else b"%d" % L
    return b"".join([small(b"NM", rng.choice((0, 0, 1, 2, 300))), aux_tag(b"MD", "Z", md), small(b"AS", rng.randrange(70000)),
                     small(b"XS", rng.randrange(300)), aux_tag(b"RG", "Z", b"lane%d" % rng.randrange(4))])


def record(fields, ref_id, use_cg=False, aux=b"", name=None, aux_behind_cg=b"", cg_type=b"I"):
    """One record from the eleven SAM fields (bytes).  A CIGAR that does not parse is stored as none; a quality string of
    another length than the sequence is stored as absent (0xFF); use_cg / more than 65,535 operations: the placeholder
    kSmN and the real CIGAR in CG:B:I (CG:B:i with cg_type b"i"), between the optional fields `aux` and `aux_behind_cg`."""
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = fields[:11]
    rid = -1 if rname == b"*" else ref_id[rname]
    nrid = rid if rnext == b"=" else -1 if rnext == b"*" else ref_id[rnext]
    ops = parse_cigar(cigar) or []
    l_seq = 0 if seq == b"*" else len(seq)
    ref_len = sum(n for n, o in ops if o in (0, 2, 3, 7, 8))
    pos0 = int(pos) - 1
    if use_cg or len(ops) > 65535:
        aux = aux + b"CGB" + cg_type + struct.pack("<I", len(ops)) + b"".join(struct.pack("<I", n << 4 | o) for n, o in ops)
        ops = [(l_seq, 4), (ref_len, 3)]
    aux += aux_behind_cg
    bin_ = reg2bin(pos0, pos0 + max(ref_len, 1)) if pos0 >= 0 else 4680
    seq_b = bytearray((l_seq + 1) // 2)
    for i in range(l_seq):
        seq_b[i // 2] |= _NT16_CODE.get(chr(seq[i]).upper(), 15) << (4 if i % 2 == 0 else 0)
    if qual == b"*" or len(qual) != l_seq:
        qual_b = b"\xff" * l_seq
    else:
        qual_b = bytes(c - 33 for c in qual)
    nm = (name if name is not None else qname) + b"\0"
    body = (struct.pack("<iiBBHHHIiii", rid, pos0, len(nm), int(mapq), bin_, len(ops), int(flag), l_seq, nrid, int(pnext) - 1, int(tlen)) + nm +
            b"".join(struct.pack("<I", n << 4 | o) for n, o in ops) + bytes(seq_b) + qual_b + aux)
    return struct.pack("<I", len(body)) + body


def bam_stream(lines, refs=None, text=b"@HD\tVN:1.6\n", use_cg=(), aux=None):
    """Decompressed BAM (header + records) of SAM lines (bytes, tab separated).  `refs`: (name, length) in order; names the
    lines use that it lacks are appended.  use_cg: indices of lines stored with the CG:B:I placeholder.  aux: {line index:
    the record's optional fields as bytes, or (fields before CG, fields behind CG, b"I" or b"i")}."""
    aux = aux or {}
    refs = list(refs or [])
    ref_id = {n: i for i, (n, _) in enumerate(refs)}
    recs = []
    for i, ln in enumerate(lines):
        f = ln.split(b"\t")
        for n in (f[2], f[6]):
            if n not in (b"*", b"=") and n not in ref_id:
                ref_id[n] = len(refs)
                refs.append((n, 1 << 30))
        a = aux.get(i, b"")
        a = (a, b"", b"I") if isinstance(a, bytes) else a
        recs.append(record(f, ref_id, use_cg=i in use_cg, aux=a[0], aux_behind_cg=a[1], cg_type=a[2]))
    return header(refs, text) + b"".join(recs)


# ---- what `samtools view -F 0xD04 -q 20` prints ----
def parse_stream(d):
    """(reference names, [(offset, record bytes incl. block_size)]) of a decompressed BAM stream."""
    assert d[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", d, 4)[0]
    q = 8 + l_text
    n_ref = struct.unpack_from("<i", d, q)[0]
    q += 4
    names = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", d, q)[0]
        names.append(d[q + 4:q + 4 + ln].split(b"\0")[0])
        q += 8 + ln
    recs = []
    while q + 4 <= len(d):
        bs = struct.unpack_from("<I", d, q)[0]
        recs.append((q, d[q:q + 4 + bs]))
        q += 4 + bs
    return names, recs


def _cigar_ops(r):
    rid, pos, lname, _mapq, _bin, ncig, _flag, lseq = struct.unpack_from("<iiBBHHHI", r, 4)
    cig = 36 + lname
    ops = [struct.unpack_from("<I", r, cig + 4 * i)[0] for i in range(ncig)]
    aux = cig + 4 * ncig + (lseq + 1) // 2 + lseq
    if ops and rid >= 0 and pos >= 0 and ops[0] & 15 == 4 and ops[0] >> 4 == lseq:   # htslib's bam_tag2cigar
        p, end = aux, len(r)
        sizes = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}
        while p + 3 <= end:
            tag, ty = r[p:p + 2], chr(r[p + 2])
            p += 3
            if ty in "ZH":
                p = r.find(b"\0", p) + 1
                if p == 0:   # not terminated before the record ends: nothing lies behind it
                    break
            elif ty == "B":
                if p + 5 > end:
                    break
                sub, n = chr(r[p]), struct.unpack_from("<I", r, p + 1)[0]
                if sub not in sizes:
                    break
                if tag == b"CG" and sub in "Ii":
                    if len(ops) <= n < 1 << 29 and p + 5 + 4 * n <= end:
                        ops = [struct.unpack_from("<I", r, p + 5 + 4 * i)[0] for i in range(n)]
                    break
                p += 5 + n * sizes[sub]
            elif ty in sizes:
                p += sizes[ty]
            else:
                break
    return ops


def render(r, names):
    """The eleven fields of one record as samtools prints them (no optional fields), without the line break."""
    rid, pos, lname, mapq, _bin, _ncig, flag, lseq, nrid, npos, tlen = struct.unpack_from("<iiBBHHHIiii", r, 4)
    name = r[36:36 + lname].split(b"\0")[0]
    ops = _cigar_ops(r)
    cigar = b"".join(b"%d%s" % (o >> 4, OPS[o & 15].encode()) for o in ops) or b"*"
    s0 = 36 + lname + 4 * _ncig
    seq = bytes(ord(NT16[(r[s0 + i // 2] >> (4 if i % 2 == 0 else 0)) & 15]) for i in range(lseq)) or b"*"
    q0 = s0 + (lseq + 1) // 2
    qual = b"*" if lseq == 0 or r[q0] == 0xFF else bytes(c + 33 for c in r[q0:q0 + lseq])
    rn = lambda i: b"*" if i < 0 else names[i]   # noqa: E731
    rnext = b"*" if nrid < 0 else b"=" if nrid == rid else names[nrid]
    return b"\t".join([name, b"%d" % flag, rn(rid), b"%d" % (pos + 1), b"%d" % mapq, cigar, rnext, b"%d" % (npos + 1), b"%d" % tlen, seq, qual])


def view(d):
    """`samtools view -F 0xD04 -q 20` of a decompressed BAM stream: the kept records as lines."""
    names, recs = parse_stream(d)
    out = []
    for _, r in recs:
        flag, mapq = struct.unpack_from("<H", r, 18)[0], r[13]
        if flag & 0xD04 == 0 and mapq >= 20:
            out.append(render(r, names) + b"\n")
    return b"".join(out)


def inflate(buf):
    """All members of a BGZF buffer inflated with zlib."""
    out, p = [], 0
    while p < len(buf):
        d = zlib.decompressobj(31)
        out.append(d.decompress(buf[p:]))
        p = len(buf) - len(d.unused_data)
    return b"".join(out)
