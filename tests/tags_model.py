"""The rule of the truth BAM's NM, MD and XE tags (simuReads --truth-tags, DESIGN.md "Truth tags") from its definition:
the CIGAR is expanded into one label per alignment column, SEQ and FASTA letters are paired by index arithmetic, MD is
put together with itertools.groupby, and XE is what errors_model's per-base layout counts for the read.  No walk over
runs and no code shared with the engine: the engine's statement (truth_tags_walk, truth_xe, sg_truth.h) is what it checks."""
import itertools
import struct

import numpy as np

import errors_model as EM

OP_M, OP_I, OP_D, OP_N, OP_S = 0, 1, 2, 3, 4
TAG_NM, TAG_MD, TAG_XE = 1, 2, 4
TAG_ALL = 7


def ref_letter(fasta_byte):
    """The letter MD shows for a FASTA byte: its upper case when that is A, C, G or T, else N (the engine's base codes keep
    no IUPAC letter, and a kept carriage return is an unknown base too)."""
    ch = bytes([fasta_byte]).upper()
    return ch if ch in (b"A", b"C", b"G", b"T") else b"N"


def nm_md(ops, seq, fasta, pos=0):
    """(NM, MD text) of a mapped record: ops = [(len, op)], seq = SEQ in BAM orientation, fasta = the contig's bytes as the
    file holds them (line ends taken out), pos = the record's 0-based POS."""
    labels = [(op, k) for k, (n, op) in enumerate(ops) for _ in range(n)]            # one per column: its op and its run
    on_query = np.array([op in (OP_M, OP_I, OP_S) for op, _ in labels], dtype=np.int64)
    on_ref = np.array([op in (OP_M, OP_D, OP_N) for op, _ in labels], dtype=np.int64)
    qi = np.cumsum(on_query) - on_query                                              # the column's SEQ index, reference offset
    ri = np.cumsum(on_ref) - on_ref
    assert int(on_query.sum()) == len(seq), "the operations do not cover SEQ"
    assert pos + int(on_ref.sum()) <= len(fasta), "the alignment runs past the contig's end"
    tokens = []                                                                      # (kind, run, letter) of the M and D columns
    nm = 0
    for c, (op, run) in enumerate(labels):
        if op == OP_M:
            r = ref_letter(fasta[pos + int(ri[c])])
            s = seq[int(qi[c]):int(qi[c]) + 1]
            same = s == r and r != b"N"
            tokens.append(("=" if same else "x", None, r))
            nm += not same
        elif op == OP_D:
            tokens.append(("^", run, ref_letter(fasta[pos + int(ri[c])])))
            nm += 1
        elif op == OP_I:
            nm += 1
    out, m = [], 0
    for (kind, _run), grp in itertools.groupby(tokens, key=lambda t: (t[0], t[1])):
        grp = list(grp)
        if kind == "=":
            m += len(grp)
        elif kind == "x":
            for _, _, r in grp:
                out.append(b"%d" % m + r)
                m = 0
        else:
            out.append(b"%d^" % m + b"".join(r for _, _, r in grp))
            m = 0
    out.append(b"%d" % m)
    return nm, b"".join(out)


def xe(codes, reverse, events, read):
    """XE of a read whose template lies in its chain: `codes` the template's chain codes in chain direction, `events`
    ev_pack words in read direction, `read` the read in FASTQ orientation.  It is what the read adds to Q.errors, I.bases
    and D.bases of the true error counts."""
    t = EM.Table(max(len(read), 1), 0, 1, len(codes))
    t.add(codes, reverse, events, read, b"!" * len(read), 0)
    return int(t.Q[..., EM.ERRORS].sum() + t.I[..., 1].sum() + t.D[..., 1].sum())


def tags(ops, seq, fasta, pos, inside, codes=None, reverse=False, events=(), read=b"", mask=TAG_ALL, cap=2048):
    """{'NM': n, 'XE': n, 'MD': text} with the tags the record gets, and whether an MD text was dropped."""
    out, dropped = {}, False
    if ops:
        nm, md = nm_md(ops, seq, fasta, pos)
        if mask & TAG_NM:
            out["NM"] = nm
        if mask & TAG_MD:
            if len(md) <= cap:
                out["MD"] = md
            else:
                dropped = True
    if inside and mask & TAG_XE:
        out["XE"] = xe(codes, reverse, events, read)
    return out, dropped


def tag_bytes(t):
    """The bytes behind the qualities: NM:I, XE:I, MD:Z in this order."""
    b = b""
    if "NM" in t:
        b += b"NMI" + struct.pack("<I", t["NM"])
    if "XE" in t:
        b += b"XEI" + struct.pack("<I", t["XE"])
    if "MD" in t:
        b += b"MDZ" + t["MD"] + b"\0"
    return b


def parse_tags(b):
    """The optional fields of a record as {tag: value}, in their order (types I and Z only)."""
    out, i = {}, 0
    while i < len(b):
        tag, typ = b[i:i + 2].decode(), b[i + 2:i + 3]
        if typ == b"I":
            out[tag] = struct.unpack_from("<I", b, i + 3)[0]
            i += 7
        else:
            assert typ == b"Z", (tag, typ)
            e = b.index(b"\0", i + 3)
            out[tag] = b[i + 3:e]
            i = e + 1
    return out
