"""SAM lines placed by hand for the kernels of simuscop_amd/csrc/sg_train.hip (test infrastructure; pure Python, no engine
call): short lines (about 30 bytes) whose totals name the line they come from, the FASTA / VCF / BED files around them,
the sg_train_setup struct parsed from those files, and the restatement (oracle/train_oracle.cpp) called on the same bytes.

The C ABI returns totals, not rows, so the inputs carry the row in the totals: `n_isize` lies above any chunk's line count
and the forward line number k has TLEN = k + 1 -- a lost, doubled or misnumbered line is one named cell of `isize`
(where_is turns the cell back into line, thread, tile and spine round of the three-launch scan).  Reverse lines (TLEN < 0)
have a quality symbol of their own ('#', forward 'F'), windows are named by their place in the (GC, read count) list.

The scan's geometry (sg_train.hip: kScanItems, kScanTile, the 256 tiles of a spine round) is restated here as the edges the
generators aim at; tests/test_train_lines_cpu.py shows on the restatement alone that they hit them."""
import ctypes as C
import os

import numpy as np

import simuscop_amd

ITEMS, TILE, ROUND = 8, 2048, 2048 * 256        # items a thread, items a tile, items a spine round
LINE_ELEM, LINE_TILE, LINE_ROUND = 64, 64 * 2048, 64 * 2048 * 256   # the line scan's element, tile and round in bytes
N_ISIZE = 1 << 20

ARRAYS = ("subs1", "subs2", "kmers", "quality", "isize", "ins_len", "del_len")
SCALARS = ("lines", "reads_counted", "cigar_chars", "insert_events", "delete_events", "isize_overflow", "indel_len_overflow", "skipped_overhang",
           "gc_rejected", "gc_windows", "capped")


def where_is(k):
    """Line (or gated read) number k as the scan sees it."""
    return "item %d = thread %d (its item %d), tile %d, spine round %d" % (k, k // ITEMS, k % ITEMS, k // TILE, k // ROUND)


def kmer_count(k):
    return sum(4 ** m for m in range(1, k + 1))


# ---- files ----
def random_bases(n, seed):
    """n bases without runs of N and without soft-masking (numpy's legacy generator: the same bytes everywhere)."""
    return np.frombuffer(b"ACGT", np.uint8)[np.random.RandomState(seed).randint(0, 4, n)].tobytes()


def write_fasta(path, contigs):
    with open(path, "wb") as f:
        for name, s in contigs:
            f.write(b">" + name + b"\n" + b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)))
    return path


def write_inputs(wd, contigs, vcf_rows=(), bed_rows=None):
    """wd/ref.fa, wd/known.vcf and (bed_rows given) wd/targets.bed; returns (fasta, vcf, bed or None)."""
    os.makedirs(wd, exist_ok=True)
    fa = write_fasta(os.path.join(wd, "ref.fa"), contigs)
    vcf = os.path.join(wd, "known.vcf")
    open(vcf, "wb").write(b"##fileformat=VCFv4.2\n" + b"".join(r + b"\n" for r in vcf_rows))
    bed = None
    if bed_rows is not None:
        bed = os.path.join(wd, "targets.bed")
        open(bed, "wb").write(b"".join(r + b"\n" for r in bed_rows))
    return fa, vcf, bed


def vcf_row(contig, pos, ref, alt, gt=b"0/1", qual=b"50", info=b"DP=40"):
    return b"\t".join([contig, b"%d" % pos, b".", ref, alt, qual, b"PASS", info, b"GT", gt])


def fasta_keys_and_lengths(fa):
    keys, lens = [], []
    for part in open(fa, "rb").read().split(b">")[1:]:
        head, _, body = part.partition(b"\n")
        name = head.split()[0]
        keys.append(name[3:] if name.startswith(b"chr") else name)
        lens.append(len(body) - body.count(b"\n"))
    return keys, lens


def reference_on_device(eng, ctx, fasta_path, line_len=60):
    """The FASTA image of a write_fasta file on the context (sg_reference_begin / _chunk / _commit); returns the contig keys."""
    image = open(fasta_path, "rb").read()
    assert eng.sg_reference_begin(ctx, len(image)) == 0
    assert eng.sg_reference_chunk(ctx, 0, image, len(image)) == 0
    assert eng.sg_sync(ctx) == 0
    rows, keys, off = [], [], 0
    while off < len(image):                      # headers and bodies of a write_fasta file
        assert image[off:off + 1] == b">"
        e = image.index(b"\n", off)
        name = image[off + 1:e].split()[0]
        nxt = image.find(b">", e)
        body_end = len(image) if nxt < 0 else nxt
        body = image[e + 1:body_end]
        length = len(body) - body.count(b"\n")
        rows.append(simuscop_amd.SgContig(e + 1, length, line_len, line_len + 1))
        keys.append(name[3:] if name.startswith(b"chr") else name)
        off = body_end
    tab = (simuscop_amd.SgContig * len(rows))(*rows)
    assert eng.sg_reference_commit(ctx, tab, len(rows)) == 0, eng.sg_last_error(ctx)
    return keys


def setup_from_files(keys, lens, vcf, bed, T, keep):
    """sg_train_setup from the VCF / BED files, parsed here the way vcfparser.cpp:26-106 and Genome.cpp:238-299, 684-739 do (the
    product's own parsers are exercised through `seqToProfile`).  T: .bases and .bins; `keep` holds the arrays alive."""
    row = {k: i for i, k in enumerate(keys)}
    abbr = lambda n: n.split(b"chrom", 1)[1] if b"chrom" in n else (n.split(b"chr", 1)[1] if b"chr" in n else n)   # noqa: E731
    snv, ins, dele = [], [], []
    for line in open(vcf, "rb"):
        if line.startswith(b"#"):
            continue
        f = line.split(b"\t")   # (the line break stays with the last field, as after fgets: "1/1\n" is not "1/1")
        if len(f) < 10:
            continue
        info = f[7]
        if b"DP=" in info and int(info.split(b"DP=", 1)[1].split(b";", 1)[0]) < 10:
            continue
        if float(f[5]) < 20:
            continue
        c = row.get(abbr(f[0]))
        if c is None:
            continue
        pos, homo = int(f[1]), f[9].split(b":")[0] != b"1/1"
        if len(f[3]) > 1:
            dele.append((c, pos + 1, len(f[3]) - 1))
        elif len(f[4]) > 1:
            ins.append((c, pos, len(f[4]) - 1))
        else:
            snv.append((c, pos, f[4][:1], 1 if homo else 0))
    st = simuscop_amd.SgTrainSetup()
    karr = (C.c_char_p * len(keys))(*keys)
    keep += [karr]
    st.contig_keys, st.n_contigs, st.bases, st.kmer, st.bins = karr, len(keys), T.bases.encode(), 3, T.bins
    st.n_isize, st.n_indel_len, st.count_gc, st.window = 2048, 256, 1, 1000

    def arr(ctype, vals):
        a = (ctype * max(1, len(vals)))(*vals)
        keep.append(a)
        return a
    st.n_snv = len(snv)
    st.snv_contig, st.snv_pos = arr(C.c_uint32, [x[0] for x in snv]), arr(C.c_int64, [x[1] for x in snv])
    alt = b"".join(x[2] for x in snv)
    keep.append(alt)
    st.snv_alt, st.snv_homo = alt, arr(C.c_uint8, [x[3] for x in snv])
    st.n_ins, st.ins_contig, st.ins_pos, st.ins_len = len(ins), arr(C.c_uint32, [x[0] for x in ins]), arr(C.c_int64, [x[1] for x in ins]), arr(C.c_int32, [x[2] for x in ins])
    st.n_del, st.del_contig, st.del_pos, st.del_len = len(dele), arr(C.c_uint32, [x[0] for x in dele]), arr(C.c_int64, [x[1] for x in dele]), arr(C.c_int32, [x[2] for x in dele])
    if bed:
        per = {}
        for line in open(bed, "rb"):
            f = line.rstrip(b"\n").split(b"\t")
            c = row.get(abbr(f[0]))
            if c is None or lens[c] <= 0:
                continue
            e = int(f[2])
            sp, ep = max(1, int(f[1]) - 50 + 1), min(lens[c], (lens[c] - (-e) % lens[c] if e <= 0 else e) + 50)
            k, s0 = (ep - sp + 1) // 1000, sp
            for i in range(max(k, 0)):
                e0 = ep if i == k - 1 else s0 + 999
                per.setdefault(c, []).append((s0, e0))
                s0 = e0 + 1
            if s0 <= ep:
                per.setdefault(c, []).append((s0, ep))
        first, sp, ep = [0], [], []
        for c in range(len(keys)):
            for a, b in per.get(c, []):
                sp.append(a)
                ep.append(b)
            first.append(len(sp))
        st.target_first, st.target_spos, st.target_epos = arr(C.c_uint64, first), arr(C.c_int64, sp), arr(C.c_int64, ep)
    return st


# ---- the restatement on the same bytes ----
class Totals:
    """What a training pass returns: the counts struct, its arrays as numpy views, the (GC, read count) pairs, the return code."""

    def __init__(self, kmer, bins, n_isize=N_ISIZE, n_indel_len=256, pairs_cap=0):
        kc = kmer_count(kmer)
        self.a = {"subs1": np.zeros((kc, bins, 4), np.uint64), "subs2": np.zeros((kc, bins, 4), np.uint64), "kmers": np.zeros((bins, kc), np.uint64),
                  "quality": np.zeros((16, bins, 94), np.uint64), "isize": np.zeros(n_isize, np.uint64), "ins_len": np.zeros(n_indel_len, np.uint64),
                  "del_len": np.zeros(n_indel_len, np.uint64)}
        self.st = simuscop_amd.SgTrainCounts()
        for k, v in self.a.items():
            setattr(self.st, k, v.ctypes.data_as(C.POINTER(C.c_uint64)))
        self.cap = max(1, pairs_cap)
        self.gc, self.rc, self.n = (C.c_double * self.cap)(), (C.c_double * self.cap)(), C.c_uint64()
        self.code = None

    def pairs(self):
        assert self.n.value <= self.cap, (self.n.value, self.cap)
        return list(zip(self.gc[:self.n.value], self.rc[:self.n.value]))

    def scalar(self, name):
        return getattr(self.st, name)


def declare(lib):
    cp, u64, u32, dp = C.c_char_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)
    lib.orc_train.argtypes = [cp, u64, cp, cp, cp, cp, C.c_int, C.c_int, u32, u32, C.POINTER(simuscop_amd.SgTrainCounts), dp, dp, u64, C.POINTER(u64)]
    lib.orc_train_count.argtypes = [cp, u64, cp, cp, C.c_int, C.c_int, u32, u32, C.POINTER(simuscop_amd.SgTrainCounts)]
    lib.orc_train_set_max_reads.argtypes = [u64]
    lib.orc_train_set_max_reads.restype = None
    return lib


def restate(lib, sam, files, kmer=3, bins=10, bases=b"ACTG", n_isize=N_ISIZE, n_indel_len=256, max_reads=0, gc=True, pairs_cap=None):
    """orc_train (gc) or orc_train_count on `sam`; .code is the restatement's return code (1: a line of fewer than eleven fields)."""
    declare(lib)
    fa, vcf, bed = files
    t = Totals(kmer, bins, n_isize, n_indel_len, (sam.count(b"\n") + 2 if pairs_cap is None else pairs_cap) if gc else 0)
    lib.orc_train_set_max_reads(max_reads)
    try:
        if gc:
            t.code = lib.orc_train(sam, len(sam), fa.encode(), vcf.encode(), (bed or "").encode(), bases, kmer, bins, n_isize, n_indel_len, C.byref(t.st),
                                   t.gc, t.rc, t.cap, C.byref(t.n))
        else:
            t.code = lib.orc_train_count(sam, len(sam), fa.encode(), bases, kmer, bins, n_isize, n_indel_len, C.byref(t.st))
    finally:
        lib.orc_train_set_max_reads(0)
    return t


def what_the_line_does(lib, lines, k, files, **kw):
    """(windows opened, reads counted, turned away) by line k behind lines[:k]: the restatement's counters with and without it."""
    a = restate(lib, b"".join(x + b"\n" for x in lines[:k]), files, **kw)
    b = restate(lib, b"".join(x + b"\n" for x in lines[:k + 1]), files, **kw)
    assert a.code == 0 and b.code == 0
    return (b.st.gc_windows - a.st.gc_windows, b.st.reads_counted - a.st.reads_counted, b.st.gc_rejected - a.st.gc_rejected)


def assert_same(got, want, what=""):
    """Every counter array and scalar, and the pairs in order, as doubles compared for equality.  An `isize` cell names its line."""
    for k in ARRAYS:
        if not np.array_equal(got.a[k], want.a[k]):
            bad = np.argwhere(got.a[k] != want.a[k])
            first = tuple(int(v) for v in bad[0])
            msg = [what, k, "%d cells differ, first %r: got %d, want %d" % (len(bad), first, got.a[k][first], want.a[k][first])]
            if k == "isize":
                msg.append("TLEN %d belongs to line %s" % (first[0], where_is(first[0] - 1)))
            raise AssertionError(tuple(msg))
    for k in SCALARS:
        assert got.scalar(k) == want.scalar(k), (what, k, got.scalar(k), want.scalar(k))
    gp, wp = got.pairs(), want.pairs()
    if gp != wp:
        at = next((i for i, (x, y) in enumerate(zip(gp, wp)) if x != y), min(len(gp), len(wp)))
        raise AssertionError((what, "pairs", len(gp), len(wp), "first difference at pair %d" % at, gp[at:at + 2], wp[at:at + 2]))


# ---- lines ----
def sam_line(contig, pos, tlen, seq, qual=None, cigar=None, mapq=b"60", name=b"r", more=None):
    """One line of `samtools view` text.  Forward reads carry quality 'F', reverse reads (TLEN < 0) '#'."""
    if qual is None:
        qual = (b"#" if tlen < 0 else b"F") * len(seq)
    if cigar is None:
        cigar = b"%dM" % len(seq)
    f = [name, b"0", contig, b"%d" % pos, mapq, cigar, b"=", b"0", b"%d" % tlen, seq, qual]
    if more is not None:
        f.append(more)
    return b"\t".join(f)


def text_of(lines):
    return b"".join(x + b"\n" for x in lines)


def padded(line, length, fill=b"x"):
    """`line` with a twelfth field of filler so that it is `length` bytes long, its line break included."""
    n = length - len(line) - 2
    assert n >= 0, (length, len(line))
    return line + b"\t" + (fill * (n // len(fill) + 1))[:n]


def line_ends(text):
    return np.flatnonzero(np.frombuffer(text, np.uint8) == 10)


REF4 = (b"chr1", random_bases(4000, 11))


def read_at(ref, pos, n, k):
    """The n reference bases at 1-based pos with one substitution whose place and base follow from k."""
    s = bytearray(ref[pos - 1:pos - 1 + n])
    if n:
        s[k % n] = b"ACGT"[(k // 3) % 4]
    return bytes(s)


def numbered(k, length=None, tlen=None, contig=b"chr1", ref=REF4[1], n=4):
    """Counted line number k of a text on REF4: forward with TLEN k + 1, or (tlen given) as asked; optionally padded."""
    pos = 1 + (k * 7) % (len(ref) - 64)
    ln = sam_line(contig, pos, k + 1 if tlen is None else tlen, read_at(ref, pos, n, k))
    return ln if length is None else padded(ln, length)


def break_text(lengths):
    """Counted lines number 0, 1, ... of the given byte lengths (break included); 0 stands for an empty line, which takes
    no number."""
    out, k = [], 0
    for n in lengths:
        if n == 0:
            out.append(b"")
        else:
            out.append(numbered(k, n))
            k += 1
    return text_of(out) if out else b""


def text_of_length(total, n_lines, last_break=True):
    """`total` bytes in n_lines counted lines of nearly equal length (filler in the twelfth field)."""
    each = total // n_lines
    lengths = [each] * (n_lines - 1) + [total - each * (n_lines - 1)]
    t = break_text(lengths)
    assert len(t) == total
    return t if last_break else t[:-1]


# ---- the scans over lines ----
SHORT = 50   # the short contig's length: countGC's window shrinks to it for good
SCAN_EDGES = (8, 16, 64, TILE, 2 * TILE, 3 * TILE, ROUND)   # a thread's, a tile's and a spine round's first items


ODD_TARGETS = {"nested": (31252, 31359), "row 105": (31551, 31749), "row 109": (32751, 32949)}   # 0-based windows, every long contig


def scan_contigs(exome):
    """Three long contigs, one shorter than the window, X (turned away); exome: targets every 300 bases, 0-based windows
    [300 j + 51, 300 j + 249], one nested in target 104 and rows 105 / 109 swapped in the file (ODD_TARGETS: their windows)."""
    contigs = [(b"chr1", random_bases(120000, 21)), (b"chr2", random_bases(120000, 22)), (b"chr3", random_bases(90000, 23)),
               (b"chrS", random_bases(SHORT, 24)), (b"chrX", random_bases(3000, 25))]
    bed = None
    if exome:
        bed = []
        for name, s in contigs[:3]:
            rows = [b"%s\t%d\t%d" % (name, 300 * j + 100, 300 * j + 200) for j in range((len(s) - 2000) // 300)]
            rows[105], rows[109] = rows[109], rows[105]              # out of order
            rows.insert(103, b"%s\t%d\t%d" % (name, 31301, 31310))   # nested in target 104: window [31252, 31359] in [31251, 31449]
            bed += rows
        bed.append(b"chrS\t10\t20")
    return contigs, bed


def exome_window(m):
    """0-based window of the regular targets that ends at or behind m (scan_contigs)."""
    j = max(0, (m - 249 + 299) // 300)
    return 300 * j + 51, 300 * j + 249


def scan_lines(n, exome=False, variant=0, short_at=None, drop_every=0):
    """n lines for GateOp / StateOp / CutOp / WindowOp.  The events are laid out by gated-read number d: the edges of the
    scan (8 k, 2,048 k, 524,288, and one item either side) get a contig change, a window opening, a read at the window's
    left or right end or one base outside it -- which of them is chosen by `variant` (0..5) --, and between the edges stretches of
    64 reads alternate between eight windows a thread, two windows a thread and one window over many threads; reads 8,300 to
    12,500 lie in ONE window (several tiles).  drop_every: every so-manyth line is one the filters drop (MAPQ 3), so that
    the gated-read number differs from the line number.  short_at: the gated read at which the contig shorter than a window
    is first visited.  Counted forward line k has TLEN k + 1, every third read is reverse.
    Returns (lines, aims): aims[line number] = (event, gated-read number)."""
    contigs, _ = scan_contigs(exome)
    seqs = dict(contigs)
    long_names = [b"chr1", b"chr2", b"chr3"]
    edges = set(SCAN_EDGES)
    edge_event = [("contig", "same", "open"), ("open", "contig", "same"), ("same", "open", "contig"), ("right", "left-1", "right+1"),
                  ("left-1", "right+1", "left"), ("open", "same", "back")][variant % 6]
    lines, aims = [], {}
    ws, ci, m, d = 1000, 0, 0, 0
    cur = long_names[0]

    def window(m):
        if exome:
            return exome_window(m)
        L = len(seqs[cur])
        r = min((m // ws + 1) * ws - 1, L - 1)
        return r - ws + 1, r
    ev = "contig"
    while len(lines) < n:
        k = len(lines)
        if drop_every and k % drop_every == drop_every - 1:
            lines.append(sam_line(cur, m + 1, 0, b"ACGT", mapq=b"3"))
            continue
        if d == 0:
            ev = "first"
        elif short_at is not None and d == short_at:
            ev = "short"
        else:
            base = next((e for e in (d - 1, d, d + 1) if e in edges), None)
            if base is not None:
                ev = edge_event[d - base + 1]
            elif 8300 <= d < 12500:
                ev = "same"
            elif d % 4096 == 2500:
                ev = "contig"
            else:
                phase = (d // 64) % 4
                ev = "open" if phase == 0 or (phase == 1 and d % 4 == 0) else "same"
        L = len(seqs[cur])
        l, r = window(m)
        if ev in ("open", "right+1") and (r + 1 + 8 >= L - 1700 if exome else r + 1 + 8 >= L):
            ev = "contig"                                    # the run has reached its contig's end
        if ev == "short":
            cur, m, ws = b"chrS", 7, min(ws, SHORT)
            pos0 = m
        elif ev in ("contig", "first"):
            ci += 1
            cur = long_names[ci % 3]
            m = (d * 37) % 500 + (51 if exome else 0)
            pos0 = m
        elif cur == b"chrS":                                 # leave the short contig at once
            ci += 1
            cur, m = long_names[ci % 3], 400 + d % 50
            pos0, ev = m, "contig"
        elif ev == "same":
            pos0 = min(r, max(l, m) + d % 3)
        elif ev == "open":
            pos0 = (exome_window(r + 1)[0] + (d % 2) * 198) if exome else r + 1 + d % 8
        elif ev == "right":
            pos0 = r
        elif ev == "right+1":
            pos0 = r + 1
        elif ev == "left":
            pos0 = max(l, 0)
        elif ev == "left-1":
            pos0 = max(l - 1, 0)
        else:                                                # back: a step backwards, far behind the window
            pos0 = max(0, l - 700)
        m = max(m, pos0)
        rev = d % 3 == 2
        seq = read_at(seqs[cur], pos0 + 1, 4, k)
        lines.append(sam_line(cur, pos0 + 1, -(k + 1) if rev else k + 1, seq))
        aims[k] = (ev, d)
        d += 1
    return lines, aims


def edge_lines(aims, n):
    """The line numbers whose gated-read number lies on an edge of the scan or one either side of it."""
    want = set()
    for e in SCAN_EDGES:
        want.update((e - 1, e, e + 1))
    return sorted(k for k, (_, d) in aims.items() if d in want and k < n)


# ---- train_fields_kernel: one line per clause ----
KEY63 = b"k" * 63


def fields_contigs():
    """200 contigs of 200 bases: chr7 first, the keys 1 / 10 / 100 (prefixes of each other), a key of 63 bytes, `last` last."""
    names = [b"chr7", b"chr1", b"chr10", b"chr100", KEY63] + [b"n%03d" % i for i in range(5, 199)] + [b"last"]
    return [(n, random_bases(200, 300 + i)) for i, n in enumerate(names)]


def fields_clauses():
    """[(what, line, counted)]: every clause of train_fields_kernel with its neighbour; reads of four bases at POS 20."""
    seqs = dict(fields_contigs())
    s7 = seqs[b"chr7"][19:23]

    def ln(contig=b"chr7", pos=b"20", mapq=b"60", seq=None, qual=None, more=None, tlen=b"0"):
        key = contig if contig in seqs else b"chr7"
        sq = seqs[key][19:23] if seq is None else seq
        f = [b"c", b"0", contig, pos, mapq, b"%dM" % max(1, len(sq)), b"=", b"0", tlen, sq, b"F" * len(sq) if qual is None else qual]
        return b"\t".join(f + ([more] if more is not None else []))
    return [("POS 0", ln(pos=b"0"), 0), ("POS 1", ln(pos=b"1"), 1), ("POS +15", ln(pos=b"+15"), 1), ("POS -0", ln(pos=b"-0"), 0),
            ("MAPQ 14", ln(mapq=b"14"), 0), ("MAPQ 15", ln(mapq=b"15"), 1), ("MAPQ +15", ln(mapq=b"+15"), 1), ("MAPQ -0", ln(mapq=b"-0"), 0),
            ("chr7", ln(b"chr7"), 1), ("chrom7", ln(b"chrom7", seq=s7), 1), ("7", ln(b"7", seq=s7), 1), ("xchr7", ln(b"xchr7", seq=s7), 1),
            ("chr", ln(b"chr", seq=s7), 0), ("key 1", ln(b"chr1"), 1), ("key 10", ln(b"chr10"), 1), ("key 100", ln(b"chr100"), 1),
            ("key 1000", ln(b"chr1000", seq=s7), 0), ("key 63 bytes", ln(KEY63), 1), ("key 62 bytes", ln(KEY63[:62], seq=s7), 0),
            ("first of 200", ln(b"chr7", pos=b"100"), 1), ("last of 200", ln(b"last"), 1), ("no key", ln(b"nokey", seq=s7), 0),
            ("SEQ *", ln(seq=b"*", qual=b"*"), 0), ("QUAL shorter", ln(qual=b"FFF"), 1), ("QUAL longer", ln(qual=b"FFFFF"), 1), ("QUAL equal", ln(qual=b"ABCD"), 1),
            ("eleven fields", ln(), 1), ("twelve fields", ln(more=b"NM:i:0"), 1), ("empty eleventh", ln(qual=b""), 1),
            ("forward TLEN", ln(tlen=b"77"), 1), ("reverse TLEN", ln(tlen=b"-77"), 1)]


TEN_FIELDS = b"r\t0\tchr7\t20\t60\t4M\t=\t0\t0\tACGT"


def fields_text(shift, rotate):
    """`shift` ordinary counted lines on chr7 (line k with TLEN k + 1), then the clause lines, the list rotated by `rotate`:
    clause number `rotate` is line number `shift` of the text."""
    ref = dict(fields_contigs())[b"chr7"]
    cl = fields_clauses()
    cl = cl[rotate % len(cl):] + cl[:rotate % len(cl)]
    lines = [sam_line(b"chr7", 1 + k % 150, k + 1, read_at(ref, 1 + k % 150, 4, k)) for k in range(shift)] + [c[1] for c in cl]
    return lines, shift + sum(c[2] for c in cl)


# ---- train_verdict_kernel / train_effects_kernel ----
VERDICT_N_INDEL, VERDICT_N_ISIZE = 8, 4096


def verdict_case():
    """(contigs, vcf rows, lines, expected scalars and cells): reads of 50 bases on a contig of 4,000, ascending so that
    countGC counts every one of them; the known events of the VCF at 500 (insertion of 2), 900 / 700 (insertions in file order
    with the larger position first), 1500 (deletion of 3: VCF row at 1499) and 2000 (an insertion of 1 written twice)."""
    ref = REF4[1]
    A = lambda p: ref[p - 1:p]   # noqa: E731
    vcf = [vcf_row(b"chr1", 500, A(500), A(500) + b"AC"),
           vcf_row(b"chr1", 900, A(900), A(900) + b"AC"), vcf_row(b"chr1", 700, A(700), A(700) + b"AC"),
           vcf_row(b"chr1", 1499, ref[1498:1502], A(1499)),
           vcf_row(b"chr1", 2000, A(2000), A(2000) + b"A"), vcf_row(b"chr1", 2000, A(2000), A(2000) + b"A")]
    lines = []

    def add(pos, cigar, tlen=0, n=50):
        lines.append(sam_line(b"chr1", pos, tlen, ref[pos - 1:pos - 1 + n] if pos - 1 + n <= len(ref) else (ref[pos - 1:] + b"A" * n)[:n], cigar=cigar))
    for cg in (b"50M", b"5S45M", b"5H45M", b"10M2I38M", b"10M3D40M", b"10M5N35M", b"25=25X", b"50", b"M", b"*", b"5M1I5M2I5M3D32M"):
        add(100 + len(lines), cg)
    # the CIGAR characters: every line but 5H45M adds its own (3+5+0+8+8+8+6+2+1+1+15); the unknown events so far: insertions of
    # 2, 1, 2; deletions of 3, 3
    for d in (-1, 0, 1):                          # insertion of 2 behind 500: the event is at POS + 10 - 1
        add(491 + d, b"10M2I38M")                 # known only at d = 0
    for n in (1, 3):
        add(491, b"10M%dI%dM" % (n, 40 - n))      # the position with another length: unknown
    add(691, b"10M2I38M")                         # 700: in the file, behind 900 -- the reference's loop stops before it: unknown
    add(891, b"10M2I38M")                         # 900: known
    for d in (-1, 0, 1):                          # deletion of 3 at 1500: the event is at POS + 10
        add(1490 + d, b"10M3D40M")                # known only at d = 0
    for n in (2, 4):
        add(1490, b"10M%dD40M" % n)
    add(1991, b"10M1I39M")                        # written twice in the VCF: known
    add(2100, b"10M7I33M")                        # the last cell of ins_len
    add(2101, b"10M8I32M")                        # one past it: indel_len_overflow
    add(2102, b"10M7D40M")
    add(2103, b"10M8D40M")
    for t in (VERDICT_N_ISIZE - 1, VERDICT_N_ISIZE, 0, -1):
        add(2200 + len(lines), b"50M", tlen=t)
    add(len(ref) - 49, b"50M", tlen=9)            # ends on the contig's last base
    add(len(ref) - 48, b"50M", tlen=10)           # one base over: skipped_overhang
    want = {"reads_counted": 1 + 1 + 4 + 1,      # 50M, M (no digit, and the last character is M), the four TLEN lines, the last-base read
            "skipped_overhang": 1, "isize_overflow": 1,
            # unknown insertions: 3 (first block: 2; 1 and 2) + 2 (d = -1, +1) + 2 (n = 1, 3) + 1 (700) + 2 (7, 8) = 10; deletions: 2 + 2 + 2 + 2 = 8
            "insert_events": 10, "delete_events": 8, "indel_len_overflow": 2,
            "ins_len": {1: 2, 2: 5, 3: 1, 7: 1}, "del_len": {2: 1, 3: 4, 4: 1, 7: 1},
            "isize": {VERDICT_N_ISIZE - 1: 1, 9: 1}}
    return [REF4], vcf, lines, want


# ---- the count kernels ----
COUNT_LENGTHS = (1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 151, 1000)
PRINTABLE = bytes(range(33, 127))


def count_case(n_lines):
    """(contigs, vcf rows, lines) for train_count_lds_kernel / train_count_kernel: reads of COUNT_LENGTHS mixed, forward and
    reverse, ascending on two contigs of 9,000 bases that hold an N every 97 bases (so that it stands at each context place
    in front of some base, and among a read's first K - 1 bases) and a literal X every 389 (the k-mer trie's place holder:
    the bases behind it count in the short contexts of a read's first bases, Profile.cpp:94-101, :220-226), known SNVs every
    41 bases -- 0/1 and 1/1 in turn, the ALT
    every printable character in turn -- which the reads show at even line numbers, lower-case stretches in every fifth
    read, and the quality bytes 32, 33, 126 and 127 in every read.  Counted forward line k has TLEN k + 1."""
    contigs, vcf = [], []
    for c, name in enumerate((b"chr1", b"chr2")):
        s = bytearray(random_bases(9000, 40 + c))
        for p in range(50 + c, len(s), 97):
            s[p] = ord("N")
        for p in range(211 + c, len(s), 389):               # a literal X: the reference's trie takes it for its place holder
            s[p] = ord("X")
        s[1000:1002], s[1500:1503], s[2000:2003] = b"XX", b"XAX", b"XNX"
        contigs.append((name, bytes(s)))
    alts = {0: {}, 1: {}}
    for c, (name, s) in enumerate(contigs):
        for j, p in enumerate(range(30, len(s) - 5, 41)):          # 1-based positions
            alt = PRINTABLE[(j + 7 * c) % len(PRINTABLE)]
            alts[c][p] = alt
            vcf.append(vcf_row(name, p, s[p - 1:p], bytes([alt]), gt=b"1/1" if j % 2 else b"0/1"))
    lines = []
    c, pos = 0, 1
    for k in range(n_lines):
        n = COUNT_LENGTHS[(k * 5 + k // 12) % len(COUNT_LENGTHS)]
        name, s = contigs[c]
        if pos + n > len(s):
            c, pos = c ^ 1, 1 + k % 3
            name, s = contigs[c]
        seq = bytearray(read_at(s, pos, n, k))
        if k % 2 == 0:
            for p in range(pos, pos + n):
                if p in alts[c]:
                    seq[p - pos] = alts[c][p]
        if k % 5 == 0:
            seq[n // 3:n // 2 + 1] = bytes(seq[n // 3:n // 2 + 1]).lower()
        qual = bytes((32, 33, 126, 127, 70, 35)[(i + k) % 6] for i in range(n))
        rev = k % 3 == 1
        lines.append(sam_line(name, pos, -(k + 1) if rev else k + 1, bytes(seq), qual=qual))
        pos += 1 + k % 4
    return contigs, vcf, lines


def tiny_reads(n_lines):
    """n_lines counted reads of 1 to 3 bases on REF4 (the grid stride of train_count_kernel at six-base contexts)."""
    ref = REF4[1]
    return [sam_line(b"chr1", 1 + k % 3900, -(k + 1) if k % 4 == 3 else k + 1, read_at(ref, 1 + k % 3900, 1 + k % 3, k)) for k in range(n_lines)]


# ---- train_window_gc_kernel ----
def window_case(ws, n_windows, reads=(1,)):
    """Whole genome: a contig of `ws` bases first (countGC's window shrinks to ws for good), then one of n_windows windows
    plus a last one cut short, with an N as the first / last / middle base of windows 3 / 4 / 5, no G or C in window 6; window w
    gets reads[w % len(reads)] reads.  Returns (contigs, lines)."""
    body = bytearray(random_bases(ws * n_windows + ws // 2 + 1, 60 + ws))
    if n_windows > 7:
        body[3 * ws] = body[5 * ws - 1] = body[5 * ws + ws // 2] = ord("N")
        body[6 * ws:7 * ws] = bytes(b"AT"[i % 2] for i in range(ws))
    contigs = [(b"chrS", random_bases(ws, 59)), (b"chr1", bytes(body))]
    lines = [sam_line(b"chrS", 1, 1, contigs[0][1][:1])]
    for w in range(n_windows + 1):
        for j in range(reads[w % len(reads)]):
            k = len(lines)
            pos = w * ws + (j * 7) % ws + 1
            if pos <= len(body):
                lines.append(sam_line(b"chr1", pos, k + 1, bytes(body[pos - 1:pos])))
    return contigs, lines


def exome_window_case():
    """Exome: targets of 1, 14, 15, 16, 400 and 1,500 bases before the padding of 50 either side, each with 1 to 9 reads: the read count is scaled by winSize * rc / targetSize.  Returns (contigs, bed rows, lines)."""
    ref = random_bases(30000, 77)
    bed, lines = [], []
    for j, size in enumerate((1, 14, 15, 16, 400, 1500, 1, 16, 400)):
        a = 1000 + 3000 * j
        bed.append(b"chr1\t%d\t%d" % (a, a + size))
        for r in range(1 + (j * 4) % 9):
            k = len(lines)
            pos = a - 40 + r                                  # inside the padded target, ascending
            lines.append(sam_line(b"chr1", pos, k + 1, ref[pos - 1:pos + 3]))
    return [(b"chr1", ref)], bed, lines


def cap_on_line(lib, lines, k, files, **kw):
    """The max_reads with which line k is the capping line: the reads counted up to and with it (it must be counted itself)."""
    t = restate(lib, text_of(lines[:k + 1]), files, **kw)
    assert what_the_line_does(lib, lines, k, files, **kw)[1] == 1, (k, "is not counted")
    return t.st.reads_counted


ODD_BYTES = (0x0B, 0x09, 0x8A, 0xFF, 0x7F, 0x80, 0x1A, 0x2A, 0x0A ^ 0x80, 0x4A)


def odd_byte_texts():
    """[(text, what)]: numbered lines whose filler holds the bytes that differ from a line break in one bit or in the top
    bit, directly in front of the break and directly behind it (the next line's name), in lines of whole 64-byte elements
    and of other lengths (the word-at-a-time count of LineOp::load against the byte loop of LineOp::store).  No NUL."""
    out = []
    for length in (64, 65, 100):
        lines = []
        for k in range(40):
            b, a = bytes([ODD_BYTES[k % len(ODD_BYTES)]]), bytes([ODD_BYTES[(k + 3) % len(ODD_BYTES)]])
            pos = 1 + (k * 7) % 3000
            ln = sam_line(b"chr1", pos, k + 1, read_at(REF4[1], pos, 4, k), name=(b"" if a == b"\t" else a) + b"r")
            n = length - len(ln) - 2
            fill = bytes(ODD_BYTES[(i + k) % len(ODD_BYTES)] for i in range(n - 1)) + b
            lines.append(ln + b"\t" + fill)
            assert len(lines[-1]) + 1 == length
        out.append((text_of(lines), "lines of %d bytes" % length))
    return out


def exome_cap(lib, lines, k, files, **kw):
    """(lines, max_reads) for a cap on line k with targets, where the limit is 2 * max_reads: line k must be counted and the
    reads counted up to it even.  One of the up to six lines in front of k (never line 0) is replaced by a line the filters
    drop until both hold; item 0 cannot cap (the least limit is 2)."""
    assert k >= 1
    dropped = sam_line(b"chr1", 5, 0, b"ACGT", mapq=b"3")
    for j in [None] + list(range(k - 1, max(0, k - 7), -1)):
        trial = list(lines)
        if j is not None:
            trial[j] = dropped
        n = restate(lib, text_of(trial[:k + 1]), files, **kw).st.reads_counted
        if n % 2 == 0 and n >= 2 and what_the_line_does(lib, trial, k, files, **kw)[1] == 1:
            return trial, n // 2
    raise AssertionError("no counted capping line with an even count at line %d" % k)
