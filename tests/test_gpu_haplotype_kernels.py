"""The kernels of sg_haplotypes.hip one by one against numpy, every byte exact, through the C ABI on a bare context:
ref_ingest_kernel (line shapes, contig lengths and alignments chosen on purpose, an offset above 2^32, an image the
grid walks twice), its line-structure check (one changed byte refused, the byte restored accepted), ref_scan_kernel,
hap_copy_kernel and encode_bytes_kernel (every pair of residues mod 16 at every length 1..49 for both kinds, parts of
65,536 bytes, more pieces than the grid has workgroups), hap_patch_kernel (more patches than its grid has lanes), the
two encoders against each other, and every refusal of sg_hap_check.h through the ABI with its legal neighbour.

The model is numpy indexing of the bytes the test generated through TABLE, written out below from the header's
definition of the codes (include/simuscop_amd.h), not from the kernel's constants.  pack2_kernel's outputs are not
reachable through the ABI; test_gpu_reads_placed.py and test_gpu_fragment_kernel.py pin them through the reads."""
import ctypes as C

import numpy as np
import pytest

import simuscop_amd
from simuscop_amd import SgContig, SgHapPatch, SgHapPiece

pytestmark = pytest.mark.gpu

SG_ERR_INVALID, SG_ERR_FORMAT = 1, 5
TOP = 2 ** 64 - 1

# A0 C1 T2 G3 in either case, N / n 4, X / x 6, everything else 5
TABLE = np.full(256, 5, dtype=np.uint8)
TABLE[ord("A")] = TABLE[ord("a")] = 0
TABLE[ord("C")] = TABLE[ord("c")] = 1
TABLE[ord("T")] = TABLE[ord("t")] = 2
TABLE[ord("G")] = TABLE[ord("g")] = 3
TABLE[ord("N")] = TABLE[ord("n")] = 4
TABLE[ord("X")] = TABLE[ord("x")] = 6

PIECE = np.dtype([("dst", "<u8"), ("src", "<u8"), ("len", "<u4"), ("chain", "<u4"), ("contig", "<u4"), ("kind", "<u4")])
PATCH = np.dtype([("dst", "<u8"), ("chain", "<u4"), ("base", "<u4")])
assert PIECE.itemsize == C.sizeof(SgHapPiece) and PATCH.itemsize == C.sizeof(SgHapPatch)

LF, CRLF, NONE = b"\n", b"\r\n", b""
NO_LF = np.array([b for b in range(256) if b != 10], dtype=np.uint8)               # bases of the one-line form
NO_BREAKS = np.array([b for b in range(256) if b not in (10, 13)], dtype=np.uint8)   # bases of a shape that has breaks


@pytest.fixture(scope="module")
def eng():
    return simuscop_amd.load_engine()


@pytest.fixture
def ctx(eng):
    c = C.c_void_p()
    assert eng.sg_create(C.byref(c), 0, 1) == 0, eng.sg_last_error(None)
    yield c
    eng.sg_destroy(c)


def _err(eng, ctx):
    return eng.sg_last_error(ctx).decode(errors="replace")


def _ptr(a):
    return a.ctypes.data_as(C.c_char_p)


def _upload(eng, ctx, image, size=None, at=0):
    """begin + one chunk (`image`: bytes or a uint8 array) at offset `at` of an image of `size` bytes"""
    n = len(image)
    assert eng.sg_reference_begin(ctx, n if size is None else size) == 0, _err(eng, ctx)
    if n:
        assert eng.sg_reference_chunk(ctx, at, image if isinstance(image, bytes) else _ptr(image), n) == 0, _err(eng, ctx)
    assert eng.sg_sync(ctx) == 0


def _poke(eng, ctx, at, byte):
    b = bytes([byte])
    assert eng.sg_reference_chunk(ctx, at, b, 1) == 0, _err(eng, ctx)
    assert eng.sg_sync(ctx) == 0


def _commit(eng, ctx, table):
    """table: (raw_offset, length, line_bases, line_width) rows"""
    tab = (SgContig * max(1, len(table)))(*[SgContig(*r) for r in table])
    return eng.sg_reference_commit(ctx, tab, len(table))


def _pieces(rows):
    return np.array([tuple(r) for r in rows], dtype=PIECE) if len(rows) else np.zeros(0, dtype=PIECE)


def _build(eng, ctx, lens, pieces, lit=b"", patches=None):
    la = (C.c_uint64 * max(1, len(lens)))(*lens)
    pa = pieces.ctypes.data_as(C.POINTER(SgHapPiece)) if len(pieces) else None
    qa = patches.ctypes.data_as(C.POINTER(SgHapPatch)) if patches is not None and len(patches) else None
    return eng.sg_build_haplotypes(ctx, len(lens), la, pa, len(pieces), lit if len(lit) else None, len(lit), qa,
                                   0 if patches is None else len(patches))


def _codes(eng, ctx, chain, n, offset=0):
    out = np.full(max(1, n), 0xEE, dtype=np.uint8)
    assert eng.sg_haplotype_codes(ctx, chain, offset, n, _ptr(out)) == 0, _err(eng, ctx)
    return out[:n]


def _same(got, want, what, owner=lambda off: ""):
    """exact; a failure lists the first ten differing offsets with got, expected and what owns the offset"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if bad.size:
        lines = ["%s: %d bytes differ" % (what, bad.size)]
        lines += ["  offset %d: got %d, expected %d  %s" % (o, got[o], want[o], owner(int(o))) for o in bad[:10]]
        pytest.fail("\n".join(lines))


def _identity(eng, ctx, seqs, what, shapes=None):
    """ref_codes through one identity piece per contig, each chain against TABLE[sequence]"""
    lens = [len(s) for s in seqs]
    rows = [(0, 0, n, i, i, 0) for i, n in enumerate(lens)]
    assert _build(eng, ctx, lens, _pieces(rows)) == 0, _err(eng, ctx)
    for i, s in enumerate(seqs):
        shape = "" if shapes is None else "line shape %r" % (shapes[i],)
        _same(_codes(eng, ctx, i, lens[i]), TABLE[s], "%s: contig %d of %d bases %s" % (what, i, lens[i], shape),
              lambda off: "" if shapes is None or not shapes[i][0] else "(line %d, column %d)" % divmod(off, shapes[i][0]))


# ---- FASTA images --------------------------------------------------------------------------------------------------------
def _fasta(contigs, final_newline=True):
    """contigs: (sequence as uint8 array, line_bases, break) with break LF, CRLF or NONE (the one-line form: line_bases is
    ignored, line_width == line_bases == length).  Header i is as long as puts the first base at residue i mod 16.
    Returns (image bytes, sg_contig rows)."""
    out, table, tail = bytearray(), [], 0
    for i, (seq, lb, brk) in enumerate(contigs):
        k = (i - len(out) - 2) % 16 or 16
        out += b">" + b"h" * k + b"\n"
        first, n = len(out), len(seq)
        assert first % 16 == i % 16
        raw = seq.tobytes()
        if brk == NONE:
            out += raw + b"\n"          # (the byte behind a contig's last base belongs to nobody)
            table.append((first, n, n, n))
            tail = 1 if n else 0
        else:
            for s in range(0, n, lb):
                out += raw[s:s + lb] + brk
            table.append((first, n, lb, lb + len(brk)))
            tail = len(brk) if n else 0
    if not final_newline and tail:
        del out[-tail:]
    return bytes(out), table


def _scan_model(image):
    """(sorted offsets of '>' and '@' at a line start, comment flag) of an image, by numpy"""
    a = np.frombuffer(image, dtype=np.uint8) if isinstance(image, bytes) else image
    start = np.empty(a.size, dtype=bool)
    if a.size:
        start[0] = True
        start[1:] = a[:-1] == 10
    return np.flatnonzero(start & ((a == ord(">")) | (a == ord("@")))), bool(np.any(start & (a == ord(";"))))


def _scan(eng, ctx, cap, null=False):
    offs = (C.c_uint64 * max(1, cap))()
    n, flags = C.c_uint32(), C.c_uint32(0xFFFF0000)
    assert eng.sg_reference_scan(ctx, None if null else offs, cap, C.byref(n), C.byref(flags)) == 0, _err(eng, ctx)
    return n.value, list(offs[:min(cap, n.value)]), flags.value


def _check_scan(eng, ctx, image, what):
    want, comment = _scan_model(image)
    n, got, flags = _scan(eng, ctx, len(want) + 4)
    assert n == len(want) and sorted(got) == want.tolist() and flags == (1 if comment else 0), (what, n, len(want), flags, sorted(got)[:10], want[:10])


# ---- ingest ----------------------------------------------------------------------------------------------------------------
LINE_BASES = (1, 2, 5, 15, 16, 17, 31, 32, 33, 60, 61)


def _ingest_contigs(rng):
    shapes = []
    for lb in LINE_BASES:
        for brk in (LF, CRLF):
            for n in sorted({0, 1, 15, 16, 17, 32, lb - 1, lb, lb + 1, 16 * lb, 3 * lb, 3 * lb + 1}):
                shapes.append((n, lb, brk))
    for n in sorted({0, 1, 2, 5, 15, 16, 17, 31, 32, 33, 48, 60, 61, 183, 976}):
        shapes.append((n, 0, NONE))
    shapes = shapes + shapes                                          # twice: other neighbours, other residues mod 16
    shapes += [(4099, 61, LF), (5003, 60, CRLF), (3001, 17, LF), (2048, 16, CRLF), (7777, 5, LF), (6000, 0, NONE), (3904, 61, CRLF)]
    order = rng.permutation(len(shapes))
    shapes = [shapes[i] for i in order]
    mid = len(shapes) // 2
    shapes = [(0, 60, LF)] + shapes[:mid] + [(0, 17, CRLF), (0, 0, NONE)] + shapes[mid:] + [(32, 17, CRLF), (0, 60, LF)]
    out = []
    for n, lb, brk in shapes:
        alphabet = NO_LF if brk == NONE else NO_BREAKS
        out.append((alphabet[rng.integers(0, alphabet.size, size=n)], lb, brk))
    return out


@pytest.mark.parametrize("final_newline", [True, False], ids=["final_newline", "no_final_newline"])
def test_ingest_line_shapes_lengths_and_alignments(eng, ctx, final_newline):
    """More than 500 contigs in one image: line_bases 1, 2, 5, 15, 16, 17, 31, 32, 33, 60, 61 with LF, with CR LF and as one line,
    lengths 0, 1, 15, 16, 17, 32, lb - 1, lb, lb + 1, 16 lb, 3 lb, 3 lb + 1 and a few of thousands, empty contigs first,
    last, in the middle and twice in a row, first bases at every residue mod 16, bases of all byte values but the break
    bytes.  Without the final newline the file ends behind the last base of a contig whose last block takes the fast path;
    the empty contig behind it begins at the file's end."""
    contigs = _ingest_contigs(np.random.default_rng(20 + final_newline))
    image, table = _fasta(contigs, final_newline)
    assert {r[0] % 16 for r in table} == set(range(16)) and len(table) > 500
    if not final_newline:
        image = image[:table[-2][0] + 32 + 2]    # 32 bases in lines of 17 + CR LF: one break inside
        table[-1] = (len(image), 0, 60, 61)      # (its header went with the rest: a contig is what the table says)
        assert image[-1] not in b"\r\n"
    _upload(eng, ctx, image)
    _check_scan(eng, ctx, image, "scan of the ingest image")
    assert _commit(eng, ctx, table) == 0, _err(eng, ctx)
    shapes = [(t[2] if c[2] != NONE else 0, c[2], t[0] % 16) for c, t in zip(contigs, table)]
    _identity(eng, ctx, [c[0] for c in contigs], "ingest", shapes)


def test_ingest_of_a_contig_above_4_gib(eng, ctx):
    """raw_offset above 2^32: the line and column arithmetic is 32-bit, the offset is not.  Only the chunk that holds the
    contigs is uploaded; the rest of the image stays as the allocation left it and is not read."""
    rng = np.random.default_rng(5)
    contigs = [(NO_BREAKS[rng.integers(0, NO_BREAKS.size, size=n)], lb, brk) for n, lb, brk in ((301, 60, LF), (200, 17, CRLF), (77, 0, NONE))]
    part, table = _fasta(contigs)
    base = 2 ** 32 + 11
    table = [(base + r[0], r[1], r[2], r[3]) for r in table]
    _upload(eng, ctx, part, size=base + len(part), at=base)
    assert _commit(eng, ctx, table) == 0, _err(eng, ctx)
    _identity(eng, ctx, [c[0] for c in contigs], "ingest above 4 GiB")


def test_ingest_and_scan_walk_their_grids_twice(eng, ctx):
    """One image above 64 MiB: the ingest grid covers 67,108,864 bases a trip, the scan's 33,554,432 bytes.  A contig of a
    few thousand bases and its header lie wholly in the part only a later trip sees; a newline put into that part is
    refused, the byte restored commits, and every code and every header offset is the model's."""
    rng = np.random.default_rng(64)
    lb, big = 60, 67_108_864 + 100_020
    seqs = [NO_BREAKS[rng.integers(0, NO_BREAKS.size, size=n, dtype=np.uint8)] for n in (1000, big, 5000)]
    parts, table, at = [], [], 0
    for i, s in enumerate(seqs):
        head = np.frombuffer(b">c%d\n" % i, dtype=np.uint8)
        lines = np.full((-(-s.size // lb), lb + 1), 10, dtype=np.uint8)      # every line with its break
        padded = np.zeros(lines.shape[0] * lb, dtype=np.uint8)
        padded[:s.size] = s
        lines[:, :lb] = padded.reshape(-1, lb)
        body = lines.reshape(-1)[:s.size + (s.size - 1) // lb + 1].copy()   # bases, the breaks between them, one behind
        body[-1] = 10
        table.append((at + head.size, s.size, lb, lb + 1))
        parts += [head, body]
        at += head.size + body.size
    image = np.concatenate(parts)
    assert image.size == at and table[2][0] > 2 * 33_554_432 and table[1][0] + 67_108_864 < image.size
    want, comment = _scan_model(image)
    assert want.size > 1000 and np.any(want > 67_108_864) and np.any((want > 33_554_432) & (want < 67_108_864))
    _upload(eng, ctx, image)
    n, got, flags = _scan(eng, ctx, int(want.size) + 4)
    assert n == want.size and flags == int(comment)
    assert np.array_equal(np.sort(np.array(got, dtype=np.int64)), want)
    # a base of the second trip's part of the long contig, and one of the last contig
    for contig, base_index in ((1, 67_108_864 + 50_000), (2, 2500)):
        pos = table[contig][0] + base_index + base_index // lb
        assert image[pos] not in (10, 13)
        _poke(eng, ctx, pos, 10)
        assert _commit(eng, ctx, table) == SG_ERR_FORMAT and "width" in _err(eng, ctx), (contig, _err(eng, ctx))
        _poke(eng, ctx, pos, int(image[pos]))
    assert _commit(eng, ctx, table) == 0, _err(eng, ctx)
    _identity(eng, ctx, seqs, "ingest of 64 MiB", [(lb, LF, t[0] % 16) for t in table])


# ---- line structure --------------------------------------------------------------------------------------------------------
def _refused_then_accepted(eng, ctx, image, table, pos, byte, what):
    """the image with `byte` at `pos` is SG_ERR_FORMAT, "width"; with the byte restored it commits"""
    assert image[pos] != byte, what
    _upload(eng, ctx, image)
    _poke(eng, ctx, pos, byte)
    rc = _commit(eng, ctx, table)
    assert rc == SG_ERR_FORMAT and "width" in _err(eng, ctx), "%s: byte %d at %d was not refused (rc %d, %s)" % (what, byte, pos, rc, _err(eng, ctx))
    _poke(eng, ctx, pos, image[pos])
    assert _commit(eng, ctx, table) == 0, "%s: the restored image: %s" % (what, _err(eng, ctx))


def _one_contig(n, lb, brk, seed=1, tail=None):
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGTacgtNnRYKMxX", dtype=np.uint8)[rng.integers(0, 16, size=n)]
    image, table = _fasta([(seq, lb, brk)])
    if tail is not None:                      # what follows the contig's last base
        image = image[:_raw_pos(table[0], n - 1) + 1] + tail
    return image, table, seq


def _raw_pos(row, base_index):
    first, _, lb, lw = row
    return first + (base_index // lb) * lw + base_index % lb


@pytest.mark.parametrize("brk", [LF, CRLF], ids=["lf", "crlf"])
def test_a_newline_in_place_of_a_base_is_refused_at_every_position_of_a_fast_path_block(eng, ctx, brk):
    """Lines of 17 bases: block b = 1..16 has first_len == b, so position k of a block comes from the first load in block
    k + 1 and from the second load (taken behind the break) in block k; 304 bases keep block 16 off the contig's last."""
    image, table, seq = _one_contig(304, 17, brk)
    for k in range(16):
        for b, load in ((k + 1, "first"), (k, "second")):
            if b == 0:
                continue                      # (first_len >= 1: position 0 always comes from the first load)
            assert 1 <= b <= 16 and (17 - (16 * b) % 17 > k) == (load == "first")
            _refused_then_accepted(eng, ctx, image, table, _raw_pos(table[0], 16 * b + k), 10, "block %d position %d (%s load)" % (b, k, load))
    # first_len >= 16: the whole block from one load
    image, table, seq = _one_contig(100, 40, brk)
    for k in (0, 7, 15):
        _refused_then_accepted(eng, ctx, image, table, _raw_pos(table[0], k), 10, "block 0 of a 40-base line, position %d" % k)


@pytest.mark.parametrize("brk", [LF, CRLF], ids=["lf", "crlf"])
def test_a_newline_or_carriage_return_in_place_of_a_base_in_the_byte_loop(eng, ctx, brk):
    """a contig's last block, lines shorter than a block, a contig shorter than a block; (16, 16) is one fast-path block"""
    for n, lb, bases in ((40, 17, (32, 33, 34, 39)), (23, 5, (0, 4, 5, 16, 22)), (7, 60, (0, 6)), (16, 16, (0, 15)), (48, 15, (15, 16, 47))):
        image, table, seq = _one_contig(n, lb, brk)
        for i in bases:
            for byte in (10, 13):
                _refused_then_accepted(eng, ctx, image, table, _raw_pos(table[0], i), byte, "%d bases in lines of %d, base %d" % (n, lb, i))
    # a carriage return as a base of a fast-path block, in either load's part
    image, table, seq = _one_contig(304, 17, brk)
    for i in (16 * 5 + 2, 16 * 5 + 9, 0):
        _refused_then_accepted(eng, ctx, image, table, _raw_pos(table[0], i), 13, "carriage return at base %d" % i)


def test_a_letter_in_place_of_a_break_byte_is_refused(eng, ctx):
    cases = []   # (bases, line_bases, break, index of the base in front of the break, what)
    for brk in (LF, CRLF):
        cases += [(304, 17, brk, 16, "inside block 1 (first_len 1)"), (304, 17, brk, 16 * 9 + 8, "inside block 9 (first_len 9)"),
                  (304, 17, brk, 16 * 15 + 14, "inside block 15 (first_len 15)"),
                  (64, 16, brk, 15, "right behind block 0 (first_len 16)"), (64, 16, brk, 47, "right behind block 2 (first_len 16)"),
                  (100, 32, brk, 31, "right behind block 1 of a 32-base line"), (100, 48, brk, 47, "right behind block 2 of a 48-base line"),
                  (40, 17, brk, 33, "byte loop: the last block"), (23, 5, brk, 4, "byte loop: short lines, first break"),
                  (23, 5, brk, 19, "byte loop: short lines, last break"), (31, 15, brk, 14, "byte loop: lines of 15"),
                  (33, 16, brk, 31, "right behind block 1, one base left"),
                  (18, 1, brk, 7, "byte loop: lines of one base"), (18, 1, brk, 16, "byte loop: lines of one base, second block")]
    for n, lb, brk, i, what in cases:
        image, table, seq = _one_contig(n, lb, brk)
        for t in range(len(brk)):
            pos = _raw_pos(table[0], i) + 1 + t
            assert image[pos] == brk[t]
            for byte in (ord("A"), 0, ord(">")) if t == 0 else (ord("A"),):
                _refused_then_accepted(eng, ctx, image, table, pos, byte, "%s, %r byte %d" % (what, brk, t))


def test_what_the_line_check_accepts(eng, ctx):
    """A carriage return is a base of the one-line form (code 5); what follows a contig's last base is not looked at: any
    byte, or the end of the file."""
    rng = np.random.default_rng(3)
    for n in (5, 16, 17, 100):
        seq = NO_LF[rng.integers(0, NO_LF.size, size=n)].copy()
        seq[[0, n // 2, n - 1]] = 13
        image, table = _fasta([(seq, 0, NONE)])
        _upload(eng, ctx, image)
        assert _commit(eng, ctx, table) == 0, _err(eng, ctx)
        _identity(eng, ctx, [seq], "one line with carriage returns")
    for n, lb, brk in ((32, 16, LF), (64, 16, CRLF), (51, 17, LF), (40, 17, CRLF), (10, 5, LF), (7, 60, CRLF), (96, 32, LF), (48, 48, CRLF)):
        for tail in (b"", b"A", b"AAAA", b"\r", b">x\n", b"\x00\xff"):
            image, table, seq = _one_contig(n, lb, brk, tail=tail)
            _upload(eng, ctx, image)
            assert _commit(eng, ctx, table) == 0, (n, lb, brk, tail, _err(eng, ctx))
            _identity(eng, ctx, [seq], "%d bases in lines of %d, then %r" % (n, lb, tail))


# ---- scan ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residue", range(16), ids=lambda r: "residue_%d" % r)
def test_scan_finds_headers_at_every_residue_of_a_word(eng, ctx, residue):
    """'>' and '@' at a line start at offsets 16 + r and 48 + r (r == 0: raw[p - 1] is the last byte of the word in front),
    the same characters inside a line and behind a lone carriage return at the same residue are not headers."""
    img = bytearray(b"A" * 144)
    for at, ch, before in ((16, b">", 10), (48, b"@", 10), (80, b">", ord("A")), (96, b"@", 13), (112, b">", ord(">"))):
        img[at + residue - 1] = before
        img[at + residue] = ch[0]
    image = bytes(img)
    want, _ = _scan_model(image)
    assert want.tolist() == [16 + residue, 48 + residue]
    _upload(eng, ctx, image)
    _check_scan(eng, ctx, image, "residue %d" % residue)


def test_scan_edges(eng, ctx):
    for image in (b">", b"@", b">a\nAC\n", b"@a\nAC\n>", b"ACGT\n>", b"ACGTACGTACGTACG\n@", b"ACGTACGTACGTACGT\n>", b"AC>GT\nAC@GT\n", b"ACGT\r>x\r@y\n",
                  b"\n>", b">>\n>\n\n>", b"", b"A" * 15 + b">", b"A" * 16 + b">" + b"A" * 15 + b"@"):
        _upload(eng, ctx, image)
        _check_scan(eng, ctx, image, repr(image))
    # a comment line raises the flag, is not listed and leaves the list alone
    image = b">a\nAC\n;note\n>b\nAC\n" + b"A" * 11 + b"\n;" + b"\n@c\n"
    want, comment = _scan_model(image)
    assert want.tolist() == [0, 12, 32] and comment
    _upload(eng, ctx, image)
    _check_scan(eng, ctx, image, "comment lines")
    image = image.replace(b";", b"A")
    _upload(eng, ctx, image)
    _check_scan(eng, ctx, image, "no comment lines")
    # a shorter image in a context that held a longer one: nothing behind its end is found
    long_image = b">a\n" + b"A" * 17 + b"\n>" + b"A" * 200 + b"\n>b\n"
    short = long_image[:20]
    assert len(short) % 16 and long_image[20:22] == b"\n>"
    _upload(eng, ctx, long_image)
    _check_scan(eng, ctx, long_image, "the longer image")
    _upload(eng, ctx, short)
    _check_scan(eng, ctx, short, "the shorter image")
    assert _scan_model(short)[0].tolist() == [0]


def test_scan_caps(eng, ctx):
    image = b"".join(b">c%d\nACGT\n" % i for i in range(10))
    want = _scan_model(image)[0].tolist()
    assert len(want) == 10
    _upload(eng, ctx, image)
    assert _scan(eng, ctx, 0, null=True) == (10, [], 0)
    n, got, flags = _scan(eng, ctx, 10)
    assert (n, sorted(got), flags) == (10, want, 0)
    n, got, flags = _scan(eng, ctx, 3)
    assert n == 10 and len(set(got)) == 3 and set(got) <= set(want) and flags == 0
    n, got, flags = _scan(eng, ctx, 11)
    assert (n, sorted(got)) == (10, want)


# ---- assembly --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sources():
    """the bytes every assembly test copies from: three contigs and the literal bytes (all 256 values), never changed"""
    rng = np.random.default_rng(11)
    alphabet = np.frombuffer(b"ACGTacgtNnXxRY-*", dtype=np.uint8)
    contigs = [alphabet[rng.integers(0, 16, size=n)] for n in (300_001, 1, 4099)]
    lit = rng.integers(0, 256, size=262_147, dtype=np.uint8)
    lit[:256] = np.arange(256, dtype=np.uint8)
    lit[-256:] = np.arange(256, dtype=np.uint8)[::-1]
    image, table = _fasta([(contigs[0], 60, LF), (contigs[1], 60, LF), (contigs[2], 61, CRLF)])
    for a in contigs + [lit]:
        a.setflags(write=False)
    return dict(contigs=contigs, codes=[TABLE[c] for c in contigs], lit=lit, lit_codes=TABLE[lit], image=image, table=table)


def _reference(eng, ctx, sources):
    _upload(eng, ctx, sources["image"])
    assert _commit(eng, ctx, sources["table"]) == 0, _err(eng, ctx)


def _model(lens, pieces, sources, patches=None):
    chains = [np.full(n, 0xAA, dtype=np.uint8) for n in lens]
    for dst, src, ln, ch, contig, kind in pieces.tolist():
        chains[ch][dst:dst + ln] = (sources["lit_codes"] if kind else sources["codes"][contig])[src:src + ln]
    if patches is not None:
        for c in range(len(lens)):
            m = patches["chain"] == c
            chains[c][patches["dst"][m].astype(np.int64)] = TABLE[patches["base"][m]]
    return chains


def _check_build(eng, ctx, lens, pieces, sources, what, patches=None, lit=None):
    lit = sources["lit"].tobytes() if lit is None else lit
    assert _build(eng, ctx, lens, pieces, lit, patches) == 0, _err(eng, ctx)
    model = _model(lens, pieces, sources, patches)

    def owner(c):
        mine = pieces[pieces["chain"] == c]

        def f(off):
            p = mine[(mine["dst"] <= off) & (off < mine["dst"] + mine["len"])]
            return "no piece" if not len(p) else "piece dst %d src %d len %d contig %d kind %d (dst %% 16 = %d, src %% 16 = %d)" % (
                p[0]["dst"], p[0]["src"], p[0]["len"], p[0]["contig"], p[0]["kind"], p[0]["dst"] % 16, p[0]["src"] % 16)
        return f
    for c, n in enumerate(lens):
        _same(_codes(eng, ctx, c, n), model[c], "%s: chain %d of %d bases" % (what, c, n), owner(c))
    return model


def _tile(rows, chain, at, src_room, rng, want_dst, want_src, ln, kind, contig=0):
    """append a filler that moves `at` to residue want_dst mod 16, then the piece itself at a source offset of residue
    want_src; returns the new end"""
    fill = (want_dst - at) % 16
    if fill:
        k = int(rng.integers(0, 2))
        rows.append((at, int(rng.integers(0, 1000)), fill, chain, 0, k))
        at += fill
    src = 16 * int(rng.integers(0, (src_room - ln - want_src) // 16 + 1)) + want_src
    assert src + ln <= src_room and src % 16 == want_src and at % 16 == want_dst
    rows.append((at, src, ln, chain, contig, kind))
    return at + ln


def test_copy_every_pair_of_residues_at_every_length(eng, ctx, sources):
    """One build: for both kinds every (dst mod 16, src mod 16) with every length 1..49 -- 25,088 pieces and their fillers,
    more than the 16,384 workgroups of hap_copy_kernel's grid --, shuffled, on three interleaved chains; pieces of 65,535
    to 200,000 bytes (the host cuts them at 65,536) at odd residues; chains of 0, 1, 63, 64 and 65 bases; source ranges
    that reach the last literal byte and a contig's last base."""
    _reference(eng, ctx, sources)
    rng = np.random.default_rng(16)
    n0, n_lit = sources["contigs"][0].size, sources["lit"].size
    rows, ends = [], [0, 0, 0]
    for kind in (0, 1):
        for d in range(16):
            for s in range(16):
                for ln in range(1, 50):
                    c = int(rng.integers(0, 3))
                    ends[c] = _tile(rows, c, ends[c], n_lit if kind else n0, rng, d, s, ln, kind)
    # long pieces on chains of their own, both kinds
    long_ends = [0, 0]
    for kind in (0, 1):
        for ln, d, s in ((65_535, 3, 9), (65_536, 5, 1), (65_537, 15, 7), (131_073, 1, 15), (200_000, 11, 13)):
            long_ends[kind] = _tile(rows, 3 + kind, long_ends[kind], n_lit if kind else n0, rng, d, s, ln, kind)
    lens = ends + long_ends + [0, 1, 63, 64, 65]
    rows += [(0, n_lit - 1, 1, 6, 0, 1),                                         # the last literal byte
             (0, n0 - 63, 63, 7, 0, 0),                                          # ... contig 0's last base
             (0, 0, 1, 8, 1, 0), (1, n_lit - 63, 63, 8, 0, 1),                   # contig 1 is one base
             (0, 4099 - 65, 65, 9, 2, 0)]
    pieces = _pieces(rows)
    assert len(pieces) > 40_000
    pieces = pieces[rng.permutation(len(pieces))]
    _check_build(eng, ctx, lens, pieces, sources, "every residue pair")


def test_literal_bytes_of_all_values_and_the_two_encoders(eng, ctx, sources):
    """All 256 byte values as one literal piece (encode_bytes_kernel), as one chain of sg_upload_haplotypes (encode_kernel)
    and as patches (hap_patch_kernel): each is TABLE."""
    every = np.arange(256, dtype=np.uint8)
    _reference(eng, ctx, sources)
    pieces = _pieces([(0, 0, 256, 0, 0, 1), (0, 0, 256, 1, 0, 0)])
    assert _build(eng, ctx, [256, 256], pieces, every.tobytes()) == 0, _err(eng, ctx)
    built = _codes(eng, ctx, 0, 256)
    _same(built, TABLE, "a literal piece of all byte values")
    patches = np.zeros(256, dtype=PATCH)
    patches["dst"], patches["chain"], patches["base"] = every, 1, every[::-1]
    assert _build(eng, ctx, [256, 256], pieces, every.tobytes(), patches) == 0, _err(eng, ctx)
    _same(_codes(eng, ctx, 1, 256), TABLE[::-1], "patches of all byte values")
    raw = every.tobytes()
    ptrs = (C.c_char_p * 1)(raw)
    assert eng.sg_upload_haplotypes(ctx, 1, ptrs, (C.c_uint64 * 1)(256)) == 0, _err(eng, ctx)
    uploaded = _codes(eng, ctx, 0, 256)
    _same(uploaded, TABLE, "sg_upload_haplotypes of all byte values")
    _same(uploaded, built, "the two encoders")


def test_builds_and_uploads_follow_each_other_on_one_context(eng, ctx, sources):
    """A build, a larger one, a smaller one, an upload, a build, an upload: each gives exactly its own model, nothing of
    the earlier chains shows and the ranges past the new lengths are refused."""
    _reference(eng, ctx, sources)
    n_lit = sources["lit"].size

    def build(lens, seed):
        rng = np.random.default_rng(seed)
        rows = []
        for c, n in enumerate(lens):
            at = 0
            while at < n:
                ln = min(n - at, int(rng.integers(1, 700)))
                kind = int(rng.integers(0, 2))
                rows.append((at, int(rng.integers(0, (n_lit if kind else 300_001) - ln)), ln, c, 0, kind))
                at += ln
        _check_build(eng, ctx, lens, _pieces(rows), sources, "build %r" % (lens,))
        _past_the_end(lens)

    def _past_the_end(lens):
        out = C.create_string_buffer(16)
        for c, n in enumerate(lens):
            assert eng.sg_haplotype_codes(ctx, c, n, 1, out) == SG_ERR_INVALID and "past the end" in _err(eng, ctx)
            assert eng.sg_haplotype_codes(ctx, c, n, 0, out) == 0
        assert eng.sg_haplotype_codes(ctx, len(lens), 0, 0, out) == SG_ERR_INVALID and "chain index" in _err(eng, ctx)

    def upload(strings):
        ptrs = (C.c_char_p * len(strings))(*strings)
        lens = [len(s) for s in strings]
        assert eng.sg_upload_haplotypes(ctx, len(strings), ptrs, (C.c_uint64 * len(strings))(*lens)) == 0, _err(eng, ctx)
        for c, s in enumerate(strings):
            _same(_codes(eng, ctx, c, len(s)), TABLE[np.frombuffer(s, dtype=np.uint8)], "upload: chain %d" % c)
        _past_the_end(lens)

    build([1000, 500], 1)
    build([5000, 3000, 10, 0, 77], 2)
    build([100], 3)
    upload([b"ACGTNXacgtnx-" * 40, b"G", b"TTTT" * 600])
    build([300, 2000], 4)
    upload([b"xXnN" * 5])
    build([64], 5)


# ---- patches ---------------------------------------------------------------------------------------------------------------
def test_patch_placements(eng, ctx, sources):
    """first and last base of chains, both sides of piece boundaries, literal bytes, a chain of one base; every base value"""
    _reference(eng, ctx, sources)
    rows = [(0, 5, 100, 0, 0, 0), (100, 0, 50, 0, 0, 1), (150, 1000, 107, 0, 0, 0),
            (0, 9, 1, 1, 0, 1),
            (0, 0, 64, 2, 2, 0), (64, 100, 64, 2, 0, 1)]
    lens = [257, 1, 128]
    where = [(0, 0), (0, 256), (0, 99), (0, 100), (0, 149), (0, 150), (0, 120), (1, 0), (2, 0), (2, 63), (2, 64), (2, 127), (2, 100)]
    patches = np.zeros(len(where), dtype=PATCH)
    patches["chain"], patches["dst"] = [w[0] for w in where], [w[1] for w in where]
    patches["base"] = [ord(c) for c in "gTnxA*c\x00GtNXa"]
    _check_build(eng, ctx, lens, _pieces(rows), sources, "patch placements", patches)
    # every base value, in an order of its own
    rows = [(0, 0, 300, 0, 0, 0), (300, 17, 212, 0, 0, 1)]
    rng = np.random.default_rng(8)
    patches = np.zeros(256, dtype=PATCH)
    patches["dst"], patches["base"] = rng.permutation(512)[:256], rng.permutation(256)
    _check_build(eng, ctx, [512], _pieces(rows), sources, "patches of every value", patches)


def test_more_patches_than_the_grid_has_lanes(eng, ctx, sources):
    """1,100,000 patches at distinct offsets of two chains: hap_patch_kernel's grid is 1,048,576 lanes"""
    _reference(eng, ctx, sources)
    rng = np.random.default_rng(9)
    rows = [(k * 300_000, 1, 300_000, 0, 0, 0) for k in range(3)] + [(k * 200_000, 7 + k, 200_000, 1, 0, 1) for k in range(2)]
    lens = [900_000, 400_000]
    n = 1_100_000
    at = rng.permutation(1_300_000)[:n]
    patches = np.zeros(n, dtype=PATCH)
    patches["chain"] = at >= 900_000
    patches["dst"] = np.where(at >= 900_000, at - 900_000, at)
    patches["base"] = rng.integers(0, 256, size=n)
    model = _check_build(eng, ctx, lens, _pieces(rows), sources, "1.1 million patches", patches)
    unpatched = _model(lens, _pieces(rows), sources)
    assert sum(int(np.count_nonzero(a != b)) for a, b in zip(model, unpatched)) > 500_000


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _refused(eng, ctx, rc, code, part, what):
    assert rc == code and part in _err(eng, ctx), "%s: rc %d, message %r" % (what, rc, _err(eng, ctx))


def test_refusals_of_the_reference_calls(eng, ctx):
    offs, n, flags = (C.c_uint64 * 4)(), C.c_uint32(), C.c_uint32()
    one = (SgContig * 1)(SgContig(3, 4, 60, 61))
    # before any image
    _refused(eng, ctx, eng.sg_reference_chunk(ctx, 0, b"A", 1), SG_ERR_INVALID, "outside sg_reference_begin's size", "chunk before begin")
    _refused(eng, ctx, eng.sg_reference_scan(ctx, offs, 4, C.byref(n), C.byref(flags)), SG_ERR_INVALID, "sg_reference_scan: call sg_reference_begin first", "scan before begin")
    _refused(eng, ctx, eng.sg_reference_commit(ctx, one, 1), SG_ERR_INVALID, "sg_reference_commit: call sg_reference_begin first", "commit before begin")
    _refused(eng, ctx, _build(eng, ctx, [4], _pieces([(0, 0, 4, 0, 0, 0)])), SG_ERR_INVALID, "call sg_reference_commit first", "build before commit")
    assert _build(eng, ctx, [0, 0], _pieces([])) == 0, "chains of no bases need no reference"
    image = b">a\nACGT\n>b\n" + b"ACGTA" * 12 + b"\n" + b"ACGTA" * 2
    assert eng.sg_reference_begin(ctx, len(image)) == 0
    for off, nb, what in ((1, len(image), "past the end by one"), (len(image) + 1, 0, "nothing behind the end"), (TOP, 1, "offset + bytes == 2^64"),
                          (TOP - len(image) + 1, len(image), "offset = 2^64 - bytes"), (2, TOP - 1, "bytes near 2^64")):
        _refused(eng, ctx, eng.sg_reference_chunk(ctx, off, image, nb), SG_ERR_INVALID, "outside sg_reference_begin's size", "chunk " + what)
    assert eng.sg_reference_chunk(ctx, len(image), image, 0) == 0
    assert eng.sg_reference_chunk(ctx, 0, image, len(image)) == 0 and eng.sg_sync(ctx) == 0
    first_b = image.index(b">b\n") + 3
    good = [(3, 4, 60, 61), (first_b, 70, 60, 61)]
    assert len(image) == first_b + 71
    for row, code, part, what in (((3, 4, 0, 61), SG_ERR_INVALID, "contig 1 has an impossible line shape", "line_bases 0"),
                                  ((3, 4, 60, 59), SG_ERR_INVALID, "contig 1 has an impossible line shape", "line_width < line_bases"),
                                  ((first_b, 71, 60, 61), SG_ERR_INVALID, "contig 1 runs past the end of the file", "past the image by one"),
                                  ((first_b + 1, 70, 60, 61), SG_ERR_INVALID, "contig 1 runs past the end of the file", "shifted past the image by one"),
                                  ((TOP - 69, 70, 60, 61), SG_ERR_INVALID, "contig 1 runs past the end of the file", "raw_offset = 2^64 - length"),
                                  ((TOP - 70, 70, 60, 61), SG_ERR_INVALID, "contig 1 runs past the end of the file", "raw_offset + extent == 2^64"),
                                  ((TOP, 1, 60, 61), SG_ERR_INVALID, "contig 1 runs past the end of the file", "raw_offset = 2^64 - 1"),
                                  ((len(image) + 1, 0, 0, 0), SG_ERR_INVALID, "contig 1 runs past the end of the file", "an empty contig behind the end")):
        _refused(eng, ctx, _commit(eng, ctx, [good[0], row]), code, part, what)
    assert _commit(eng, ctx, good + [(len(image), 0, 0, 0)]) == 0, _err(eng, ctx)    # ends exactly at the image's end
    _identity(eng, ctx, [np.frombuffer(b"ACGT", np.uint8), np.frombuffer(b"ACGTA" * 14, np.uint8), np.zeros(0, np.uint8)], "the accepted neighbour")
    # the commit released the image
    _refused(eng, ctx, eng.sg_reference_chunk(ctx, 0, image, 1), SG_ERR_INVALID, "outside sg_reference_begin's size", "chunk after commit")
    _refused(eng, ctx, eng.sg_reference_scan(ctx, offs, 4, C.byref(n), C.byref(flags)), SG_ERR_INVALID, "call sg_reference_begin first", "scan after commit")
    _refused(eng, ctx, eng.sg_reference_commit(ctx, one, 1), SG_ERR_INVALID, "call sg_reference_begin first", "commit after commit")


def test_refusals_of_build_and_codes(eng, ctx, sources):
    out = C.create_string_buffer(64)
    _refused(eng, ctx, eng.sg_haplotype_codes(ctx, 0, 0, 1, out), SG_ERR_INVALID, "no haplotypes on the device", "codes before any chains")
    _reference(eng, ctx, sources)
    n0, n_lit = 300_001, sources["lit"].size
    lit = sources["lit"].tobytes()
    lens = [100, 50]
    good = [(0, n0 - 60, 60, 0, 0, 0), (60, n_lit - 40, 40, 0, 0, 1), (0, 4099 - 50, 50, 1, 2, 0)]
    _check_build(eng, ctx, lens, _pieces(good), sources, "the legal list")

    def refused(rows, part, what, patches=None, code=SG_ERR_INVALID):
        _refused(eng, ctx, _build(eng, ctx, lens, _pieces(rows), lit, patches), code, part, what)

    def with_piece(i, row):
        rows = list(good)
        rows[i] = row
        return rows
    refused(with_piece(1, (61, n_lit - 40, 40, 0, 0, 1)), "piece 1 falls outside its chain", "past its chain by one")
    refused(with_piece(0, (0, n0 - 59, 60, 0, 0, 0)), "piece 0 falls outside its contig", "past its contig by one")
    refused(with_piece(1, (60, n_lit - 39, 40, 0, 0, 1)), "piece 1 falls outside the literal bytes", "past the literals by one")
    refused(with_piece(2, (0, 4099 - 50, 50, 2, 2, 0)), "piece 2 falls outside its chain", "chain index out of range")
    refused(with_piece(2, (0, 0, 50, 1, 3, 0)), "piece 2 falls outside its contig", "contig index out of range")
    refused(with_piece(2, (0, 0, 50, 1, 1, 0)), "piece 2 falls outside its contig", "longer than its one-base contig")
    # the values whose sums wrap at 2^64: each returns before any launch
    refused(with_piece(1, (TOP, 0, 1, 0, 0, 1)), "piece 1 falls outside its chain", "dst = 2^64 - 1, len 1")
    refused(with_piece(1, (TOP - 39, n_lit - 40, 40, 0, 0, 1)), "piece 1 falls outside its chain", "dst = 2^64 - len")
    refused(with_piece(0, (0, TOP - 59, 60, 0, 0, 0)), "piece 0 falls outside its contig", "contig src = 2^64 - len")
    refused(with_piece(0, (0, TOP, 60, 0, 0, 0)), "piece 0 falls outside its contig", "contig src = 2^64 - 1")
    refused(with_piece(1, (60, TOP - 39, 40, 0, 0, 1)), "piece 1 falls outside the literal bytes", "literal src = 2^64 - len")
    # patches
    patch = np.zeros(1, dtype=PATCH)
    for dst, chain, ok in ((99, 0, True), (100, 0, False), (49, 1, True), (50, 1, False), (0, 2, False), (TOP, 0, False)):
        patch["dst"], patch["chain"], patch["base"] = dst, chain, ord("A")
        if ok:
            assert _build(eng, ctx, lens, _pieces(good), lit, patch) == 0, _err(eng, ctx)
        else:
            refused(good, "patch 0 falls outside its chain", "patch at %d of chain %d" % (dst, chain), patch)
    # tiling
    refused(good[:2], "the pieces of chain 1 do not add up to its length", "a chain without pieces")
    refused(with_piece(1, (60, 0, 39, 0, 0, 1)), "the pieces of chain 0 do not add up to its length", "adds up short")
    refused(with_piece(0, (0, 0, 61, 0, 0, 0)), "overlaps another piece of chain 0", "adds up over")
    both = [(0, 0, 40, 0, 0, 0), (30, 0, 40, 0, 0, 1), (80, 5, 20, 0, 0, 0), good[2]]      # [0,40) [30,70) [80,100): sum 100
    refused(both, "of chain 0", "adds up right with an overlap and a gap")
    assert "overlaps" in _err(eng, ctx) and "piece 1" in _err(eng, ctx)
    refused(both[::-1], "overlaps another piece of chain 0", "the same in another order")
    twice = [(0, 0, 50, 0, 0, 0), (0, 0, 50, 0, 0, 0), good[2]]
    refused(twice, "piece 1 overlaps another piece of chain 0", "one half twice, the other never")
    # accepted: any order, pieces of length 0 at the start, in the middle and at the end
    shuffled = [good[2], (100, 0, 0, 0, 0, 0), good[1], (0, 0, 0, 0, 0, 1), good[0], (60, n0, 0, 0, 0, 0), (50, n_lit, 0, 1, 0, 1)]
    _check_build(eng, ctx, lens, _pieces(shuffled), sources, "shuffled, with pieces of length 0")
    # the chains of the last accepted build are still the ones read back
    for c, n, off, nb, part, what in ((2, 0, 0, 0, "chain index out of range", "chain out of range"), (0, 100, 1, 100, "range past the end of the chain", "past the end by one"),
                                      (0, 100, 101, 0, "range past the end of the chain", "nothing behind the end"), (0, 100, TOP, 1, "range past the end of the chain", "offset + n == 2^64"),
                                      (1, 50, TOP - 9, 10, "range past the end of the chain", "offset = 2^64 - n"), (1, 50, 10, TOP - 9, "range past the end of the chain", "n = 2^64 - offset")):
        _refused(eng, ctx, eng.sg_haplotype_codes(ctx, c, off, nb, out), SG_ERR_INVALID, part, "codes: " + what)
    assert eng.sg_haplotype_codes(ctx, 0, 100, 0, out) == 0 and eng.sg_haplotype_codes(ctx, 1, 49, 1, out) == 0
