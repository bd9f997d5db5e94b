"""sg_train.hip kernel by kernel on the MI355X, on SAM lines placed by hand (tests/train_lines.py): the three-launch scan with
its five operators on its own edges (8 items a thread, 2,048 a tile, 256 tiles a spine round), train_fields_kernel clause by
clause on the edges of its 256-line blocks, the verdict / effects kernels, the two count kernels on mixed read lengths and
bin counts, train_window_gc_kernel past its grid stride.  Everything goes through sg_train_count and sg_train_begin / _feed /
_finish on a bare context; the expectation is orc_train_count / orc_train (oracle/train_oracle.cpp) on the same bytes: every
counter array and scalar equal, the (GC, read count) pairs equal in order.  Integer work: no tolerance.  Forward line k has
TLEN k + 1 with n_isize = 2^20, so a lost, doubled or misnumbered line is one named cell (the message names thread, tile
and spine round).  tests/test_train_lines_cpu.py shows that the inputs reach the edges they are made for."""
import ctypes as C
import functools

import pytest

import simuscop_amd
import train_lines as TL

pytestmark = pytest.mark.gpu


class Device:
    """A bare engine context with the reference of `files` on it; .count / .train run one training session each."""

    def __init__(self, files):
        self.files = files
        self.eng = simuscop_amd.load_engine()
        self.ctx = C.c_void_p()
        assert self.eng.sg_create(C.byref(self.ctx), 0, 1) == 0
        TL.reference_on_device(self.eng, self.ctx, files[0])
        self.keys, self.lens = TL.fasta_keys_and_lengths(files[0])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.eng.sg_destroy(self.ctx)

    def count(self, sam, kmer=3, bins=10, bases=b"ACTG", n_isize=TL.N_ISIZE, n_indel_len=256):
        t = TL.Totals(kmer, bins, n_isize, n_indel_len)
        karr = (C.c_char_p * len(self.keys))(*self.keys)
        t.code = self.eng.sg_train_count(self.ctx, sam, len(sam), karr, len(self.keys), bases, kmer, bins, n_isize, n_indel_len, C.byref(t.st))
        t.error = self.eng.sg_last_error(self.ctx) if t.code else b""
        return t

    def train(self, chunks, kmer=3, bins=10, bases=b"ACTG", n_isize=TL.N_ISIZE, n_indel_len=256, max_reads=0):
        eng, ctx = self.eng, self.ctx
        keep = []

        class TT:
            pass
        TT.bases, TT.bins = bases.decode(), bins
        st = TL.setup_from_files(self.keys, self.lens, self.files[1], self.files[2], TT, keep)
        st.kmer, st.n_isize, st.n_indel_len, st.max_reads = kmer, n_isize, n_indel_len, max_reads
        assert eng.sg_train_begin(ctx, C.byref(st)) == 0, eng.sg_last_error(ctx)
        t = TL.Totals(kmer, bins, n_isize, n_indel_len, sum(c.count(b"\n") for c in chunks) + 2)
        t.code = 0
        for c in chunks:
            t.code = eng.sg_train_feed(ctx, c, len(c))
            if t.code:
                break
        if t.code == 0:
            t.code = eng.sg_train_finish(ctx, C.byref(t.st), t.gc, t.rc, t.cap, C.byref(t.n))
        t.error = eng.sg_last_error(ctx) if t.code else b""
        eng.sg_train_end(ctx)
        return t


def _cut(lines, at):
    """The text of `lines` in chunks cut in front of the line numbers `at`."""
    at = [0] + [a for a in sorted(set(at)) if 0 < a < len(lines)] + [len(lines)]
    return [TL.text_of(lines[a:b]) for a, b in zip(at, at[1:])]


@pytest.fixture(scope="module")
def ref4(tmp_path_factory):
    return TL.write_inputs(str(tmp_path_factory.mktemp("ref4")), [TL.REF4])


@pytest.fixture(scope="module")
def scan_files(tmp_path_factory):
    out = {}
    for exome in (False, True):
        contigs, bed = TL.scan_contigs(exome)
        out[exome] = TL.write_inputs(str(tmp_path_factory.mktemp("scan%d" % exome)), contigs, (), bed)
    return out


@functools.lru_cache(maxsize=None)
def _scan_lines(n, exome, variant, short_at=None, drop=0):
    return TL.scan_lines(n, exome, variant, short_at=short_at, drop_every=drop)[0]


# ---- LineOp: element = 64 bytes, tile = 131,072 bytes, spine round = 33,554,432 bytes ----
def test_line_breaks_at_every_residue_and_elements_of_0_1_and_64_breaks(oracle_lib, ref4):
    texts = [("a break at each residue of an element", TL.break_text([65] * 64)), ("lines of one element", TL.break_text([64] * 70)),
             ("lines of 63 bytes", TL.break_text([63] * 70)), ("64 empty lines in one element", TL.break_text([128] + [0] * 64 + [64])),
             ("empty lines over an element's edge", TL.break_text([100] + [0] * 130 + [77, 0, 0, 64])),
             ("empty lines only", b"\n" * 200), ("one empty line", b"\n")]
    texts += [(what, t) for t, what in TL.odd_byte_texts()]
    with Device(ref4) as dev:
        for what, text in texts:
            want = TL.restate(oracle_lib, text, ref4, gc=False)
            assert want.code == 0 and want.st.lines == len([x for x in text.split(b"\n") if x])
            TL.assert_same(dev.count(text), want, what)


@pytest.mark.parametrize("total", [1, 63, 64, 65, TL.LINE_TILE - 1, TL.LINE_TILE, TL.LINE_TILE + 1, TL.LINE_ROUND - 64, TL.LINE_ROUND, TL.LINE_ROUND + 64])
def test_text_lengths_on_the_edges_of_element_tile_and_round(total, oracle_lib, ref4):
    """Texts of exactly `total` bytes (a few hundred lines with filler in the twelfth field), with their last line break and
    without it: the last line then loses its last character -- its qualities are one short and count no quality cell."""
    n_lines = 1 if total < 200 else 300
    with Device(ref4) as dev:
        if total >= 63:
            text = TL.text_of_length(total, n_lines)
            want = TL.restate(oracle_lib, text, ref4, gc=False)
            assert want.code == 0 and want.st.lines == n_lines == want.st.reads_counted
            TL.assert_same(dev.count(text), want, "%d bytes" % total)
        # the last byte is no break: a bare line of `total` bytes for the small sizes, the text above without its break else
        open_text = TL.numbered(0, total + 1)[:total] if 63 <= total < 200 else (b"x" if total == 1 else TL.text_of_length(total + 1, n_lines)[:total])
        assert len(open_text) == total and open_text[-1:] != b"\n"
        want = TL.restate(oracle_lib, open_text, ref4, gc=False)
        assert want.code == 0 and want.st.lines == (0 if total == 1 else n_lines)      # ("x" chopped is an empty line: no read)
        TL.assert_same(dev.count(open_text), want, "%d bytes, no last break" % total)


def test_a_break_as_the_last_byte_of_a_tile_and_of_a_round(oracle_lib, ref4):
    with Device(ref4) as dev:
        for first, what in ((TL.LINE_TILE, "element 2,047 of tile 0"), (TL.LINE_ROUND, "tile 255 of round 0")):
            text = TL.text_of_length(first, 300) + TL.break_text([64, 65, 0, 0, 63, 200])
            assert int(TL.line_ends(text)[299]) == first - 1
            want = TL.restate(oracle_lib, text, ref4, gc=False)
            assert want.code == 0 and want.st.lines == 304
            TL.assert_same(dev.count(text), want, what)
        # a last line without a break whose qualities are as long as its bases before the chop: no quality cell from it
        lines = [TL.numbered(k) for k in range(3)]
        text = TL.text_of(lines)[:-1]
        want = TL.restate(oracle_lib, text, ref4, gc=False)
        assert want.st.reads_counted == 3 and want.a["quality"].sum() == 8
        TL.assert_same(dev.count(text), want, "the chopped quality string")


# ---- train_fields_kernel ----
@pytest.mark.parametrize("shift", [255, 256, 257])
def test_fields_clause_by_clause_on_the_edge_of_a_block(shift, oracle_lib, tmp_path):
    """Each of the 31 clause lines in turn as line number `shift` of the text (the fields kernel's blocks hold 256 lines),
    the other clauses behind it; the counted reads are the written number."""
    files = TL.write_inputs(str(tmp_path), TL.fields_contigs())
    n = len(TL.fields_clauses())
    with Device(files) as dev:
        for rotate in range(n):
            lines, counted = TL.fields_text(shift, rotate)
            assert counted == shift + 22
            text = TL.text_of(lines)
            want = TL.restate(oracle_lib, text, files, gc=False)
            got = dev.count(text)
            TL.assert_same(got, want, TL.fields_clauses()[rotate][0])
            assert got.code == 0 and got.st.reads_counted == shift + 22 and got.st.lines == shift + n
        # ten fields: the reference's error, wherever the line stands
        for at in (0, shift, shift + n):
            text = TL.text_of(lines[:at] + [TL.TEN_FIELDS] + lines[at:])
            assert TL.restate(oracle_lib, text, files, gc=False).code == 1
            got = dev.count(text)
            assert got.code != 0 and b"11 mandatory fields" in got.error, (at, got.code, got.error)


# ---- GateOp, StateOp, CutOp, WindowOp ----
@pytest.mark.parametrize("exome", [False, True])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048, 2049])
def test_scans_over_chunks_that_end_on_the_edges(n, exome, oracle_lib, scan_files):
    """Chunks of n lines, every variant of the events on the edges, without and with dropped lines between the gated ones; the
    last item of the chunk is the last item of a thread (8), of a tile (2,048), or one either side."""
    files = scan_files[exome]
    with Device(files) as dev:
        for variant in range(6):
            for drop in (0, 5):
                lines = _scan_lines(2600, exome, variant, None, drop)[:n]
                text = TL.text_of(lines)
                want = TL.restate(oracle_lib, text, files)
                assert want.code == 0 and want.st.lines == n
                TL.assert_same(dev.train([text]), want, "variant %d, every %dth line dropped" % (variant, drop))


@pytest.mark.parametrize("variant", [1, 5, 3])
@pytest.mark.parametrize("exome", [False, True])
def test_scans_enter_the_spines_second_round_by_line_count(exome, variant, oracle_lib, scan_files):
    """524,488 lines in one chunk (about 21 MB): the spine of every operator runs a second round of 256 tiles, and 200 items
    lie in it -- counted reads and more than 70 window openings, so the exclusive prefix the spine writes for tile 256 numbers
    windows and places reads.  Variant 1: a contig run begins exactly at item 524,288; variant 5: item 524,287 opens a window
    and the reads counted in it begin with item 524,288; variant 3: a read at `right`, one at `left - 1`, one at `right + 1`.
    Reads 8,300 to 12,500 share one window over several tiles.  Then the same text in two chunks cut in front of line 524,288: a
    run that continues across a feed."""
    files = scan_files[exome]
    lines = _scan_lines(TL.ROUND + 200, exome, variant)
    text = TL.text_of(lines)
    want = TL.restate(oracle_lib, text, files)
    assert want.code == 0 and want.st.lines == TL.ROUND + 200 and want.st.gc_windows > 100000
    with Device(files) as dev:
        TL.assert_same(dev.train([text]), want, "one chunk")
        TL.assert_same(dev.train(_cut(lines, [TL.ROUND])), want, "cut in front of line 524,288")


@pytest.mark.parametrize("exome", [False, True])
def test_a_contig_shorter_than_the_window_met_on_a_tile_edge(exome, oracle_lib, scan_files):
    """Gated read 2,048 is the first on the contig of 50 bases: ref_min shrinks for good in the tile behind it, and in the next
    feed when the text is cut there or one line later."""
    files = scan_files[exome]
    with Device(files) as dev:
        for drop in (0, 5):
            lines = _scan_lines(4200, exome, 1, TL.TILE, drop)
            at = next(k for k, x in enumerate(lines) if b"chrS" in x)
            want = TL.restate(oracle_lib, TL.text_of(lines), files)
            assert want.code == 0
            for cuts in ([], [at], [at + 1], [at - 1, at, at + 1]):
                TL.assert_same(dev.train(_cut(lines, cuts)), want, "cuts %r" % cuts)


@pytest.mark.parametrize("exome", [False, True])
def test_feeds_cut_on_the_edges(exome, oracle_lib, scan_files):
    """One text in 1, 2 and 5 chunks cut on the scan's edges, with a chunk of empty lines only and a chunk without a gated read
    between two that have some; variant 5 opens a window with the last item before each edge, so that a chunk's first read
    opens nothing and rides in the window of the chunk before."""
    files = scan_files[exome]
    dropped = [TL.sam_line(b"chr1", 100 + i, 0, b"ACGT", mapq=b"3") for i in range(9)]
    with Device(files) as dev:
        for variant in (5, 0, 4):
            lines = _scan_lines(4200, exome, variant)
            want = TL.restate(oracle_lib, TL.text_of(lines), files)
            assert want.code == 0 and want.st.lines == 4200
            for cuts in ([], [8], [2047], [2048], [2049], [7, 8, 2048, 4096], [9, 2047, 2049, 4097]):
                TL.assert_same(dev.train(_cut(lines, cuts)), want, "variant %d, cuts %r" % (variant, cuts))
            a, b = TL.text_of(lines[:2048]), TL.text_of(lines[2048:])
            TL.assert_same(dev.train([a, b"\n" * 100, b]), want, "a chunk of empty lines between")
            want2 = TL.restate(oracle_lib, a + TL.text_of(dropped) + b, files)
            assert want2.st.lines == 4209 and want2.st.reads_counted == want.st.reads_counted
            TL.assert_same(dev.train([a, TL.text_of(dropped), b]), want2, "a chunk without a gated read between")


@pytest.mark.parametrize("exome,k", [(False, k) for k in (0, 7, 8, 2047, 2048, 2999, 3000)] + [(True, k) for k in (1, 7, 8, 2047, 2048, 2999, 3000)])
def test_the_cap_on_the_edges(exome, k, oracle_lib, scan_files):
    """max_reads such that the capping line is item 0, 7, 8, 2,047, 2,048, a chunk's last line (2,999) and the next chunk's
    first (3,000).  Behind the capping line lie a line the filters drop, a line of ten fields, which is never read, and reads
    that would open windows.  With targets the limit is twice max_reads, so the count at the capping line is made even and
    item 1 stands for item 0."""
    files = scan_files[exome]
    lines = list(_scan_lines(4200, exome, 2))
    if exome:
        lines, cap = TL.exome_cap(oracle_lib, lines, k, files)
    else:
        cap = TL.cap_on_line(oracle_lib, lines, k, files)
    lines[k + 1:k + 1] = [TL.sam_line(b"chr1", 5, 0, b"ACGT", mapq=b"3"), TL.TEN_FIELDS]   # (the first adds nothing to the prefix count)
    want = TL.restate(oracle_lib, TL.text_of(lines), files, max_reads=cap)
    assert want.code == 0 and want.st.capped == 1 and want.st.lines == k + 1 and want.st.reads_counted == (2 * cap if exome else cap)
    with Device(files) as dev:
        for cuts in ([], [3000], [8, 2048, 3000]):
            got = dev.train(_cut(lines, cuts), max_reads=cap)
            assert got.code == 0, got.error
            TL.assert_same(got, want, "capping line %s, cuts %r" % (TL.where_is(k), cuts))
        # without the cap the ten-field line is the reference's error
        assert TL.restate(oracle_lib, TL.text_of(lines), files).code == 1
        got = dev.train([TL.text_of(lines)])
        assert got.code != 0 and b"11 mandatory fields" in got.error


# ---- train_verdict_kernel / train_effects_kernel ----
def test_cigars_known_events_and_the_ends_of_the_rows(oracle_lib, tmp_path):
    contigs, vcf, lines, written = TL.verdict_case()
    files = TL.write_inputs(str(tmp_path), contigs, vcf)
    text = TL.text_of(lines)
    kw = dict(n_isize=TL.VERDICT_N_ISIZE, n_indel_len=TL.VERDICT_N_INDEL)
    want = TL.restate(oracle_lib, text, files, **kw)
    with Device(files) as dev:
        got = dev.train([text], **kw)
        TL.assert_same(got, want, "verdict case")
        for name, v in written.items():
            if isinstance(v, dict):
                assert {i: int(got.a[name][i]) for i in range(len(got.a[name])) if got.a[name][i]} == v, name
            else:
                assert got.scalar(name) == v, name
        assert got.st.cigar_chars == 211
        for cuts in ([11], [3, 18, 24, 33]):
            TL.assert_same(dev.train(_cut(lines, cuts), **kw), want, "cuts %r" % cuts)


# ---- the count kernels ----
# bins a group of train_count_lds_kernel (60 KB of LDS): 9 at k-mer 1 and 2, 6 at 3, 3 at 4, 1 at 5, none at 6 (train_count_kernel)
@pytest.mark.parametrize("kmer,bases,bins,n_lines", [
    (1, b"ACTG", 50, 257), (1, b"GTCA", 151, 256), (2, b"GTCA", 7, 255), (2, b"ACTG", 1, 257),
    (3, b"ACTG", 12, 4097), (3, b"GTCA", 7, 257), (3, b"ACTG", 50, 256), (3, b"GTCA", 2, 255), (3, b"ACTG", 151, 257),
    (4, b"GTCA", 6, 257), (4, b"ACTG", 7, 4097), (4, b"ACTG", 50, 255),
    (5, b"ACTG", 1, 256), (5, b"GTCA", 2, 257), (5, b"GTCA", 7, 4097),
    (6, b"ACTG", 7, 4097), (6, b"GTCA", 50, 257), (6, b"GTCA", 151, 255), (6, b"ACTG", 1, 256)])
def test_count_kernels_on_mixed_read_lengths(kmer, bases, bins, n_lines, oracle_lib, tmp_path):
    """Reads of 1 to 1,000 bases in one chunk (shorter than sixteen bases, than the bin count, than the context), forward and
    reverse, over Ns, known SNVs shown and not shown, ALTs of every printable character, lower-case bases, quality bytes 32 / 33 /
    126 / 127; bin counts that the group size does and does not divide; 255 / 256 / 257 / 4,097 lines around the read slices."""
    contigs, vcf, lines = TL.count_case(n_lines)
    files = TL.write_inputs(str(tmp_path), contigs, vcf)
    text = TL.text_of(lines)
    kw = dict(kmer=kmer, bases=bases, bins=bins)
    want = TL.restate(oracle_lib, text, files, **kw)
    assert want.code == 0 and want.st.reads_counted == n_lines
    with Device(files) as dev:
        TL.assert_same(dev.train([text], **kw), want, "k-mer %d, %s, %d bins" % (kmer, bases.decode(), bins))
        plain = TL.restate(oracle_lib, text, files, gc=False, **kw)      # sg_train_count: no known variants
        TL.assert_same(dev.count(text, **kw), plain, "sg_train_count")


@pytest.mark.parametrize("n_lines", [32769, 70000])
def test_count_kernel_walks_its_grid_twice(n_lines, oracle_lib, ref4):
    """Six-base contexts fit no LDS: train_count_kernel, 32,768 waves, more reads than waves (of 1 to 3 bases each)."""
    text = TL.text_of(TL.tiny_reads(n_lines))
    want = TL.restate(oracle_lib, text, ref4, gc=False, kmer=6, bins=3)
    assert want.code == 0 and want.st.reads_counted == n_lines
    with Device(ref4) as dev:
        TL.assert_same(dev.count(text, kmer=6, bins=3), want, "%d reads" % n_lines)


# ---- train_window_gc_kernel ----
@pytest.mark.parametrize("ws,n_windows", [(1, 40), (63, 40), (64, 40), (65, 40), (1000, 12), (64, 16385), (64, 40000)])
def test_window_gc(ws, n_windows, oracle_lib, tmp_path):
    """Windows of ws bases (the window shrinks to a first contig of that length): an N first, last and in the middle (-1, not
    pushed), no G or C (0, not pushed), the contig's last window, 1 to 3 reads a window; 16,385 and 40,000 windows pass the
    kernel's 16,384 waves."""
    contigs, lines = TL.window_case(ws, n_windows, (1, 2, 3) if n_windows < 1000 else (1,))
    files = TL.write_inputs(str(tmp_path), contigs)
    text = TL.text_of(lines)
    want = TL.restate(oracle_lib, text, files)
    assert want.code == 0 and want.st.gc_windows == n_windows + 2 and want.st.reads_counted == len(lines)
    if ws >= 63:
        assert want.n.value == n_windows + 1 - 4                 # all but the last, the three with an N and the one without G or C
    with Device(files) as dev:
        got = dev.train([text])
        TL.assert_same(got, want, "windows of %d" % ws)
        if n_windows > 1000:
            TL.assert_same(dev.train(_cut(lines, [16384, 16385])), want, "cut at the stride")


def test_exome_windows_scale_their_read_counts(oracle_lib, tmp_path):
    contigs, bed, lines = TL.exome_window_case()
    files = TL.write_inputs(str(tmp_path), contigs, (), bed)
    want = TL.restate(oracle_lib, TL.text_of(lines), files)
    with Device(files) as dev:
        got = dev.train([TL.text_of(lines)])
        TL.assert_same(got, want, "exome windows")
        assert [rc for _, rc in got.pairs()] == [10.0, 44.0, 78.0, 34.0, 16.0, 1.0, 70.0, 17.0]
        # a read behind the last target: a window without sequence (GC -1), never pushed, the read turned away
        more = lines + [TL.sam_line(b"chr1", 29000, 99, contigs[0][1][28999:29003]), TL.sam_line(b"chr1", 29500, 100, contigs[0][1][29499:29503])]
        want = TL.restate(oracle_lib, TL.text_of(more), files)
        assert want.st.gc_rejected == 2 and want.st.gc_windows == 10 and want.n.value == 9
        TL.assert_same(dev.train([TL.text_of(more)]), want, "behind the last target")
