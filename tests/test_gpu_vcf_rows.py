"""The device VCF reader on the MI355X (sg_vcf_*, simuscop_amd/csrc/sg_vcf.hip) over a bare context, against vcf_model:
fragments, counts, kept rows per kind in file order, the malformed numbers and the undecided fragments with their bytes --
exactly, for plain text cut anywhere between calls and for the same text as BGZF members of several sizes; then the
refusals of corrupt and cut members, which deliver nothing."""
import ctypes as C
import random
import struct

import pytest

import bam_util
import simuscop_amd
import vcf_model as M

pytestmark = pytest.mark.gpu

TILE = 2048   # values per block of the scan (sg_scan.hip)


@pytest.fixture(scope="module")
def ctx():
    lib = simuscop_amd.load_engine()
    c = C.c_void_p()
    assert lib.sg_create(C.byref(c), 0, 1) == 0
    yield c
    lib.sg_destroy(c)


def run(ctx, pieces, bgzf=False, keys=M.KEYS):
    """One session over `pieces` (texts, or runs of BGZF members): (counts, rows per kind, undecided [(number, bytes)])."""
    simuscop_amd.vcf_begin(ctx, keys)
    try:
        und = []
        for p in pieces:
            und += simuscop_amd.vcf_feed(ctx, p, bgzf)
        c, last = simuscop_amd.vcf_finish(ctx)
        und += last
        rows = {k: simuscop_amd.vcf_rows(ctx, k, n) for k, n in (("snv", c.kept_snv), ("ins", c.kept_ins), ("del", c.kept_del))}
        return c, rows, und
    finally:
        simuscop_amd.vcf_end(ctx)


def check(ctx, text, pieces=None, bgzf=False):
    """The device on `pieces` (default: the text in one call) against the model on `text`."""
    want = M.parse(text)
    frs = M.fragments(text)
    c, rows, und = run(ctx, [text] if pieces is None else pieces, bgzf)
    assert c.fragments == want["fragments"] and c.text_bytes == len(text)
    # a fragment the device hands back is in none of its lists: the model's lists without them
    handed = set(want["undecided"])
    assert [n for n, _ in und] == want["undecided"] and c.undecided == len(handed)
    assert [b for _, b in und] == [frs[n - 1] for n in want["undecided"]]
    for k in ("snv", "ins", "del"):
        assert rows[k] == [r for r in want["rows"][k] if r[0] not in handed], k
    n_dev = {k: sum(1 for no, f in enumerate(frs, 1) if no not in handed and M.row(f)[0] == k) for k in ("snv", "ins", "del")}
    assert (c.n_snv, c.n_ins, c.n_del) == (n_dev["snv"], n_dev["ins"], n_dev["del"])
    bad = [n for n in want["malformed"] if n not in handed]
    assert c.malformed == len(bad) and list(c.malformed_first[:min(len(bad), 11)]) == bad[:11]
    return c, want


def test_one_fragment_per_clause(ctx):
    c, want = check(ctx, M.clause_text())
    assert c.undecided == sum(1 for _, _, d in M.CLAUSES if not d) and c.kept_snv > 20 and c.kept_ins == 1 and c.kept_del == 1


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 7])
def test_line_counts_around_the_wave_the_block_and_the_scan_tile(ctx, n):
    check(ctx, M.random_text(100 + n, n, odd=0.05))


def test_cut_between_calls_at_every_byte_of_a_window(ctx):
    """Three lines in the middle of a text, the cut at each of their bytes: inside every field, on a tab, on the line
    break, inside "DP="."""
    lines = [M.mk(info=b"AF=0.5;DP=31;MQ=60", sample=b"1/1:2,9"), M.mk(chrom=b"chrom2", ref=b"ACGT", pos=b"77"), M.mk(alt=b"AGG", qual=b"19.9999999")]
    head, tail = M.random_text(5, 40), M.random_text(6, 40)
    text = head + b"".join(lines) + tail
    want = M.parse(text)
    for cut in range(len(head), len(head) + sum(map(len, lines)) + 1):
        c, rows, und = run(ctx, [text[:cut], text[cut:]])
        assert c.fragments == want["fragments"] and not und, cut
        assert rows == want["rows"], cut


def test_cuts_everywhere_and_empty_calls(ctx):
    text = M.random_text(9, 700, odd=0.08)
    rng = random.Random(4)
    cuts = sorted(rng.randrange(len(text)) for _ in range(60))
    pieces = [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])] + [b""]
    check(ctx, text, pieces)


@pytest.mark.parametrize("size", [19998, 19999, 20000, 40001])
@pytest.mark.parametrize("brk", [True, False])
def test_long_lines_are_the_parsers_fragments(ctx, size, brk):
    """A data line of `size` bytes (its line break included, when it has one): the fragment behind byte 19,999 is parsed
    on its own, a line of exactly 19,999 bytes with a line break is one fragment."""
    row = M.mk(fmt=b"GT", sample=b"1/1", end=b"")
    filler = b"\t".join(b"0/1" for _ in range(20000))
    line = (row + b"\t" + filler)[:size - (1 if brk else 0)] + (b"\n" if brk else b"")
    assert len(line) == size
    text = M.mk(pos=b"1") + M.mk(pos=b"2") + line
    c, want = check(ctx, text)
    assert c.fragments == 2 + -(-size // M.FRAG)
    check(ctx, text, [text[:len(text) - 30000 if size > 30000 else 50], text[len(text) - 30000 if size > 30000 else 50:]])


def test_long_header_line_whose_tail_is_a_row(ctx):
    text = M.long_header_text()
    c, want = check(ctx, text)
    assert (3, 77, 1, ord("G"), M.KNOWN | M.HOMO) in want["rows"]["snv"] and c.kept_snv == 3 and c.fragments == 6


def test_crlf_no_final_break_only_headers_and_nothing(ctx):
    check(ctx, M.random_text(21, 300).replace(b"\r\n", b"\n").replace(b"\n", b"\r\n"))
    check(ctx, M.random_text(22, 300, final_break=False))
    c, _ = check(ctx, b"##a\n#CHROM\tPOS\n##b")
    assert c.fragments == 3 and c.kept_snv == 0
    c, _ = check(ctx, b"")
    assert c.fragments == 0
    c, rows, und = run(ctx, [])
    assert c.fragments == 0 and not und


def test_eleven_malformed_fragments_over_three_calls(ctx):
    good, bad = M.mk(), b"chr1\t5\tx\n"
    a = (good * 3 + bad) * 4
    b = (bad + good) * 5
    cc = good + bad * 4 + good
    c, want = check(ctx, a + b + cc, [a, b, cc])
    assert c.malformed == 13 and len(want["malformed"]) == 13


def test_two_contexts_and_a_reused_one(ctx):
    lib = simuscop_amd.load_engine()
    other = C.c_void_p()
    assert lib.sg_create(C.byref(other), 0, 2) == 0
    try:
        t1, t2 = M.random_text(31, 500, odd=0.05), M.random_text(32, 300, odd=0.05)
        simuscop_amd.vcf_begin(ctx, M.KEYS)
        simuscop_amd.vcf_begin(other, M.KEYS[:2])
        simuscop_amd.vcf_feed(ctx, t1[:7000])
        simuscop_amd.vcf_feed(other, t2)
        simuscop_amd.vcf_feed(ctx, t1[7000:])
        c1, _ = simuscop_amd.vcf_finish(ctx)
        c2, _ = simuscop_amd.vcf_finish(other)
        w1, w2 = M.parse(t1), M.parse(t2, M.KEYS[:2])
        assert simuscop_amd.vcf_rows(ctx, "snv", c1.kept_snv) == w1["rows"]["snv"]
        assert simuscop_amd.vcf_rows(other, "snv", c2.kept_snv) == w2["rows"]["snv"]
        simuscop_amd.vcf_end(ctx)
        simuscop_amd.vcf_end(other)
        check(ctx, t2)   # the first context again
    finally:
        simuscop_amd.vcf_end(ctx)
        lib.sg_destroy(other)


def test_calls_in_front_of_begin_and_behind_finish(ctx):
    lib = simuscop_amd.load_engine()
    n, c = C.c_uint64(), simuscop_amd.SgVcfCounts()
    assert lib.sg_vcf_feed(ctx, b"x\n", 2) == 1 and b"sg_vcf_begin" in lib.sg_last_error(ctx)
    assert lib.sg_vcf_feed_bgzf(ctx, b"x", 1) == 1 and lib.sg_vcf_finish(ctx, C.byref(c)) == 1
    assert lib.sg_vcf_rows(ctx, 1, 0, 0, None) == 1 and lib.sg_vcf_undecided(ctx, None, 0, C.byref(n), None, 0, C.byref(n)) == 1
    simuscop_amd.vcf_begin(ctx, M.KEYS)
    try:
        assert lib.sg_vcf_begin(ctx, None, 0) == 1
        simuscop_amd.vcf_feed(ctx, M.mk())
        simuscop_amd.vcf_finish(ctx)
        assert lib.sg_vcf_feed(ctx, b"x\n", 2) == 1 and b"finished" in lib.sg_last_error(ctx)
        assert lib.sg_vcf_rows(ctx, 1, 0, 2, None) == 1 and lib.sg_vcf_rows(ctx, 4, 0, 0, None) == 1
        assert simuscop_amd.vcf_rows(ctx, "snv", 1) == [(1,) + M.SNV[1:]]   # the context is still usable
    finally:
        simuscop_amd.vcf_end(ctx)


def test_a_line_longer_than_64_mib_is_refused_with_its_offset(ctx):
    """Finished or left unfinished by the call: SG_ERR_INVALID naming where the line starts, nothing delivered, and the
    session goes on as if the call had not been made."""
    lib = simuscop_amd.load_engine()
    head = M.mk(pos=b"5") + M.mk(pos=b"6")
    big = b"x" * ((64 << 20) + 1)
    simuscop_amd.vcf_begin(ctx, M.KEYS)
    try:
        simuscop_amd.vcf_feed(ctx, head)
        for text in (big, M.mk(pos=b"7") + big + b"\n" + M.mk(pos=b"8")):
            assert lib.sg_vcf_feed(ctx, text, len(text)) == 1
            msg = lib.sg_last_error(ctx).decode()
            assert "text offset %d " % (len(head) + (0 if text is big else len(M.mk(pos=b"7")))) in msg and "64 MiB" in msg, msg
        simuscop_amd.vcf_feed(ctx, M.mk(pos=b"9", end=b""))
        c, _ = simuscop_amd.vcf_finish(ctx)
        assert c.fragments == 3 and c.text_bytes == len(head) + len(M.mk(pos=b"9", end=b""))
        assert [r[1] for r in simuscop_amd.vcf_rows(ctx, "snv", c.kept_snv)] == [5, 6, 9]
    finally:
        simuscop_amd.vcf_end(ctx)
    check(ctx, M.mk() + b"y" * (1 << 20) + b"\n" + M.mk())   # a long line below the limit is the parser's fragments


# ---- the same texts as BGZF members ----
@pytest.mark.parametrize("member", [150, 4096, 65280])
def test_bgzf_members_of_three_sizes(ctx, member):
    text = M.clause_text() + M.random_text(40 + member, 600 if member < 1000 else 3000, odd=0.05)
    gz = bam_util.bgzf(text, member=member, level=1 if member == 4096 else 6)
    offs = [o for o, _, _ in bam_util.members(gz)[0]]
    third = offs[len(offs) // 3], offs[2 * len(offs) // 3]
    check(ctx, text, [gz], bgzf=True)
    check(ctx, text, [gz[:third[0]], gz[third[0]:third[1]], gz[third[1]:]], bgzf=True)


def test_bgzf_lines_across_members_empty_members_and_the_fragment_boundary(ctx):
    """A line across two and across three members, members of 0 bytes between them, a member boundary on the 19,999th byte
    of a long line."""
    long_line = (M.mk(fmt=b"GT", sample=b"1/1", end=b"") + b"\t" + b"\t".join(b"0/1" for _ in range(9000)))[:30000] + b"\n"
    text = M.mk(pos=b"11") + M.mk(pos=b"22", ref=b"ACG") + M.mk(pos=b"33", alt=b"AT") + long_line + M.mk(pos=b"44")
    l1 = len(M.mk(pos=b"11"))
    at = 3 * l1 + 2 + 1          # where the long line starts (the second and third rows are 2 and 1 bytes longer)
    assert text[at:at + 5] == b"chr20" and text[at - 1:at] == b"\n"
    cuts = [10, l1 + 5, l1 + 9, l1 + 9, l1 + 20, at + M.FRAG, at + M.FRAG + 1]   # (a cut given twice: an empty member)
    bounds = sorted(cuts + [0, len(text)])
    gz = [bam_util.bgzf_member(text[a:b]) for a, b in zip(bounds, bounds[1:])]
    assert any(struct.unpack("<I", m[-4:])[0] == 0 for m in gz)
    check(ctx, text, [b"".join(gz) + bam_util.EOF_MEMBER], bgzf=True)
    check(ctx, text, gz + [bam_util.EOF_MEMBER], bgzf=True)


def test_a_corrupt_or_cut_member_delivers_nothing(ctx):
    lib = simuscop_amd.load_engine()
    text = M.random_text(77, 2000)
    gz = bam_util.bgzf(text, member=4096, eof=False)
    mem = bam_util.members(gz)[0]
    k = len(mem) // 2
    first, rest = gz[:mem[k][0]], gz[mem[k][0]:]
    bad_at = mem[k + 3][0]
    crc_at = bad_at + mem[k + 3][1] + 1 - 8 - mem[k][0]
    corrupt = rest[:crc_at] + bytes([rest[crc_at] ^ 0x10]) + rest[crc_at + 1:]
    cut = rest[:len(rest) - 9]
    simuscop_amd.vcf_begin(ctx, M.KEYS)
    try:
        simuscop_amd.vcf_feed(ctx, first, True)
        assert lib.sg_vcf_feed_bgzf(ctx, corrupt, len(corrupt)) == 1
        msg = lib.sg_last_error(ctx).decode()
        assert "file offset %d" % bad_at in msg and "CRC-32" in msg, msg
        assert lib.sg_vcf_feed_bgzf(ctx, cut, len(cut)) == 1
        msg = lib.sg_last_error(ctx).decode()
        assert "file offset %d" % mem[-1][0] in msg and "cut short" in msg, msg
        simuscop_amd.vcf_feed(ctx, rest, True)   # the intact members behind the two failures: as if they had not been tried
        c, _ = simuscop_amd.vcf_finish(ctx)
        want = M.parse(text)
        assert c.fragments == want["fragments"] and c.text_bytes == len(text)
        assert simuscop_amd.vcf_rows(ctx, "snv", c.kept_snv) == want["rows"]["snv"]
        assert simuscop_amd.vcf_rows(ctx, "del", c.kept_del) == want["rows"]["del"]
    finally:
        simuscop_amd.vcf_end(ctx)
