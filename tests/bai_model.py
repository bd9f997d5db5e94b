"""The BAI index of a coordinate-sorted BAM in plain Python, from the bytes of the file alone (the rule: simuscop_amd/csrc/
sg_bamindex.h; SAMv1 section 5.2): members with bam_util.members, inflation with zlib, a record walk with start offsets,
the index, its serialisation; a parser of .bai bytes; and query(), the standard reader.  No samtools, no pysam, and
nothing of the code under test."""
import bisect
import struct
import zlib

import bam_util

OPEN = 2 ** 64 - 1
PSEUDO_BIN = 37450
REF_OPS = (0, 2, 3, 7, 8)          # M D N = X


class MemberMap:
    """Where the uncompressed bytes of a run of BGZF members lie in the file: the members of `buf`, the first at file
    offset `base`; `u0` is the uncompressed position of the first one's first byte."""

    def __init__(self, buf, base=0, u0=0):
        ms, used = bam_util.members(buf)
        assert used == len(buf), "bytes behind the last whole member"
        self.ustart, self.foff, self.text = [], [], []
        u = u0
        for off, bsize, isize in ms:
            self.ustart.append(u)
            self.foff.append(base + off)
            d = zlib.decompressobj(31).decompress(buf[off:off + bsize + 1])
            assert len(d) == isize
            self.text.append(d)
            u += isize
        self.end_u = u

    def voff(self, u):
        """bgzf_tell at uncompressed position u: a position at a member's end is the next member's start."""
        i = bisect.bisect_right(self.ustart, u) - 1
        return self.foff[i] << 16 | (u - self.ustart[i])


def fields(r):
    """(refID, beg, end, bin, has 0x4, the record's own bin field) of one record (bytes, block_size included)."""
    ref, pos, lname, _mapq, binf, ncig, flag = struct.unpack_from("<iiBBHHH", r, 4)
    ref_len = 0
    for k in range(ncig):
        op = struct.unpack_from("<I", r, 36 + lname + 4 * k)[0]
        if op & 15 in REF_OPS:
            ref_len += op >> 4
    unm = bool(flag & 4)
    end = pos + (1 if unm or ref_len == 0 else ref_len)
    return ref, pos, end, (bam_util.reg2bin(pos, end) if ref >= 0 else None), unm, binf


def file_records(bam):
    """([(name, length)], [record]) of a BAM file's bytes, a record being a dict: raw, voff, end (the next record's voff,
    the end-of-file block's for the last), ref, beg, stop, bin, unmapped, bin_field."""
    mm = MemberMap(bam)
    d = b"".join(mm.text)
    assert d[:4] == b"BAM\1"
    q = 8 + struct.unpack_from("<i", d, 4)[0]
    n_ref = struct.unpack_from("<i", d, q)[0]
    q += 4
    refs = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", d, q)[0]
        refs.append((d[q + 4:q + 4 + ln - 1], struct.unpack_from("<i", d, q + 4 + ln)[0]))
        q += 8 + ln
    recs = []
    while q < len(d):
        n = 4 + struct.unpack_from("<I", d, q)[0]
        r = d[q:q + n]
        assert len(r) == n
        ref, beg, stop, bin_, unm, binf = fields(r)
        recs.append(dict(raw=r, voff=mm.voff(q), ref=ref, beg=beg, stop=stop, bin=bin_, unmapped=unm, bin_field=binf))
        q += n
    assert mm.text[-1] == b"" and bam.endswith(bam_util.EOF_MEMBER), "no end-of-file block"
    for a, b in zip(recs, recs[1:]):
        a["end"] = b["voff"]
    if recs:
        recs[-1]["end"] = mm.foff[-1] << 16
    return refs, recs


def chunk_rows(recs):
    """The chunk rows of one call over `recs` (dicts with ref, bin, voff, in file order): [(key, beg, end)] grouped by
    key = refID << 32 | bin, keys ascending, file order within a key; a chunk ends where the next record starts, the one
    that ends the call stays OPEN; runs of refID -1 end a chunk and make none."""
    rows, prev = [], None
    for i, r in enumerate(recs):
        key = None if r["ref"] < 0 else r["ref"] << 32 | r["bin"]
        end = recs[i + 1]["voff"] if i + 1 < len(recs) else OPEN
        if key is not None and key == prev:
            rows[-1][2] = end
        elif key is not None:
            rows.append([key, r["voff"], end])
        prev = key
    return sorted((tuple(r) for r in rows), key=lambda r: r[0])


def linear_and_counts(recs, ref_len):
    """What the device keeps of a stem: the linear cells of all references back to back (OPEN: untouched) and
    counts[3 n_ref + 1] (records without 0x4, with 0x4, smallest voff per reference; then the refID -1 records)."""
    first, at = [], 0
    for ln in ref_len:
        first.append(at)
        at += (ln + 16383) >> 14
    lin = [OPEN] * at
    counts = [0, 0, OPEN] * len(ref_len) + [0]
    for r in recs:
        if r["ref"] < 0:
            counts[-1] += 1
            continue
        c = 3 * r["ref"]
        counts[c + (1 if r["unmapped"] else 0)] += 1
        counts[c + 2] = min(counts[c + 2], r["voff"])
        for w in range(r["beg"] >> 14, ((r["stop"] - 1) >> 14) + 1):
            lin[first[r["ref"]] + w] = min(lin[first[r["ref"]] + w], r["voff"])
    return lin, counts


def index(recs, n_ref):
    """The index of a file's records (each with its `end`): per reference {bins: {bin: [(beg, end)]}, pseudo: None or
    ((first voff, last end), (mapped, unmapped)), linear: [ioffset]}, and n_no_coor."""
    refs = [dict(bins={}, pseudo=None, linear=[]) for _ in range(n_ref)]
    no_coor, prev = 0, None
    for r in recs:
        if r["ref"] < 0:
            no_coor += 1
            prev = None
            continue
        R = refs[r["ref"]]
        key = (r["ref"], r["bin"])
        if key == prev:
            R["bins"][r["bin"]][-1][1] = r["end"]
        else:
            R["bins"].setdefault(r["bin"], []).append([r["voff"], r["end"]])
        prev = key
        p = R["pseudo"] or [[r["voff"], r["end"]], [0, 0]]
        p[0][1] = r["end"]
        p[1][1 if r["unmapped"] else 0] += 1
        R["pseudo"] = p
        lin = R["linear"]
        last = (r["stop"] - 1) >> 14
        lin.extend([OPEN] * (last + 1 - len(lin)))
        for w in range(r["beg"] >> 14, last + 1):
            lin[w] = min(lin[w], r["voff"])
    for R in refs:                       # an untouched window takes the value of the next touched one on its right
        for w in range(len(R["linear"]) - 2, -1, -1):
            if R["linear"][w] == OPEN:
                R["linear"][w] = R["linear"][w + 1]
    return refs, no_coor


def serialise(refs, no_coor):
    out = [b"BAI\1", struct.pack("<i", len(refs))]
    for R in refs:
        out.append(struct.pack("<i", len(R["bins"]) + (1 if R["pseudo"] else 0)))
        for b in sorted(R["bins"]):
            out.append(struct.pack("<Ii", b, len(R["bins"][b])))
            out += [struct.pack("<QQ", beg, end) for beg, end in R["bins"][b]]
        if R["pseudo"]:
            out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, *R["pseudo"][0], *R["pseudo"][1]))
        out.append(struct.pack("<i", len(R["linear"])))
        out += [struct.pack("<Q", v) for v in R["linear"]]
    out.append(struct.pack("<Q", no_coor))
    return b"".join(out)


def bai_of(bam):
    """The .bai bytes of a BAM file's bytes."""
    refs, recs = file_records(bam)
    return serialise(*index(recs, len(refs)))


def parse(bai):
    """(refs as index() gives them, n_no_coor) of .bai bytes; every byte must be used."""
    assert bai[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<i", bai, 4)[0]
    q, refs = 8, []
    for _ in range(n_ref):
        R = dict(bins={}, pseudo=None, linear=[])
        n_bin = struct.unpack_from("<i", bai, q)[0]
        q += 4
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, q)
            q += 8
            chunks = [list(struct.unpack_from("<QQ", bai, q + 16 * i)) for i in range(n_chunk)]
            q += 16 * n_chunk
            if b == PSEUDO_BIN:
                assert n_chunk == 2
                R["pseudo"] = chunks
            else:
                assert b not in R["bins"] and b < PSEUDO_BIN
                R["bins"][b] = chunks
        n_intv = struct.unpack_from("<i", bai, q)[0]
        q += 4
        R["linear"] = list(struct.unpack_from("<%dQ" % n_intv, bai, q))
        q += 8 * n_intv
        refs.append(R)
    no_coor = struct.unpack_from("<Q", bai, q)[0]
    assert q + 8 == len(bai)
    return refs, no_coor


def reg2bins(beg, end):
    """SAMv1 section 5.3: the bins that may hold records overlapping [beg, end)."""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


class Reader:
    """A BAM file's bytes read at virtual offsets, member by member."""

    def __init__(self, bam):
        self.bam = bam
        self.cache = {}

    def member(self, off):
        if off not in self.cache:
            bsize = struct.unpack_from("<H", self.bam, off + 16)[0]
            self.cache[off] = (zlib.decompressobj(31).decompress(self.bam[off:off + bsize + 1]), off + bsize + 1)
        return self.cache[off]

    def read(self, voff, n):
        """(n bytes from voff on, the voff behind them); fewer bytes at the end of the file."""
        off, within = voff >> 16, voff & 0xFFFF
        out = b""
        while len(out) < n and off < len(self.bam):
            d, nxt = self.member(off)
            take = d[within:within + n - len(out)]
            out += take
            within += len(take)
            if within == len(d):
                off, within = nxt, 0
        return out, off << 16 | within


def query(bai, bam, ref, beg, end):
    """The records of `bam` on reference `ref` that overlap [beg, end), found through the parsed index `bai` as a reader
    of the format does: the chunks of reg2bins whose end lies behind the linear index's offset of beg's window, read in
    offset order until a record starts at or behind `end`.  Returns the records' bytes in file order."""
    R = bai[0][ref]
    lin = R["linear"]
    w = beg >> 14
    min_off = lin[w] if w < len(lin) else (lin[-1] if lin else 0)
    chunks = sorted(tuple(c) for b in reg2bins(beg, end) for c in R["bins"].get(b, []) if c[1] > min_off)
    rd = Reader(bam)
    out, seen = [], set()
    for c_beg, c_end in chunks:
        v = c_beg
        while v < c_end:
            head, _ = rd.read(v, 4)
            if len(head) < 4:
                break
            n = 4 + struct.unpack("<I", head)[0]
            r, nxt = rd.read(v, n)
            r_ref, r_beg, r_stop, _bin, _unm, _binf = fields(r)
            if r_ref != ref or r_beg >= end:
                break
            if r_stop > beg and v not in seen:
                seen.add(v)
                out.append((v, r))
            v = nxt
    return [r for _, r in sorted(out)]
