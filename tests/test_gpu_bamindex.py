"""The BAI index kernels on the MI355X (sg_bamindex_*, simuscop_amd/csrc/sg_bamindex.hip) over a bare context, against
bai_model on the members the device made: after bamsort_merge + bamindex_add the chunk rows, the first offset, the linear
index and the counts equal the model run on the fetched members; the same through the sg_deflate_bgzf source with a
skipped front and a last record that runs past the text; and the refusals."""
import ctypes as C
import random
import struct

import pytest

import bai_model as M
import simuscop_amd

pytestmark = pytest.mark.gpu

TILE = simuscop_amd.BAMSORT_TILE
MAXLEN = 1 << 29
REFS = [MAXLEN, 5000, 70000, MAXLEN]        # reference 1 stays empty in most cases


@pytest.fixture(scope="module")
def ctx():
    lib = simuscop_amd.load_engine()
    c = C.c_void_p()
    assert lib.sg_create(C.byref(c), 0, 1) == 0
    yield c
    lib.sg_destroy(c)


def rec(ref, pos, ops=((100, 0),), flag=0, name=b"r", pad=0, bin_field=0xBEEF):
    """A BAM record with no sequence and `pad` bytes of optional fields; its own bin field is wrong on purpose."""
    nm = name + b"\0"
    body = (struct.pack("<iiBBHHHIiii", ref, pos, len(nm), 0, bin_field, len(ops), flag, 0, -1, -1, 0) + nm +
            b"".join(struct.pack("<I", n << 4 | o) for n, o in ops) + bytes((7 * i + 1) & 255 for i in range(pad)))
    return struct.pack("<I", len(body)) + body


def key(r):
    return struct.unpack_from("<II", r, 4)[0] << 32 | struct.unpack_from("<II", r, 4)[1]


def model_recs(records, mm, u0=0):
    out, u = [], u0
    for r in records:
        ref, beg, stop, bin_, unm, _ = M.fields(r)
        out.append(dict(ref=ref, beg=beg, stop=stop, bin=bin_, unmapped=unm, voff=mm.voff(u)))
        u += len(r)
    return out


def check_merge(ctx, records, file_off=0, refs=REFS):
    """`records` in file order (keys ascending): one merge, one add, everything against the model."""
    assert [key(r) for r in records] == sorted(key(r) for r in records)
    stream, members, _, lens = simuscop_amd.bamsort_merge(ctx, [(b"".join(records), [key(r) for r in records], [len(r) for r in records])])
    assert stream == b"".join(records)
    simuscop_amd.bamindex_begin(ctx, refs)
    rows, first = simuscop_amd.bamindex_add(ctx, simuscop_amd.BAMINDEX_MERGE, file_off)
    lin, counts = simuscop_amd.bamindex_finish(ctx, refs)
    want = model_recs(records, M.MemberMap(members, file_off))
    assert rows == M.chunk_rows(want)
    assert first == (want[0]["voff"] if want else M.OPEN)
    w_lin, w_counts = M.linear_and_counts(want, refs)
    assert counts == w_counts
    assert lin == w_lin
    return rows, want


def spread(rng, n):
    """n records over references 0, 2, 3 and -1 in key order: runs of one bin, bins met again, 0x4 records, odd lengths."""
    out = []
    for _ in range(n):
        ref = rng.choice((0, 0, 2, 3, -1))
        if ref < 0:
            out.append(rec(-1, -1, (), flag=4 | 8, pad=rng.randrange(40)))
            continue
        pos = rng.randrange(0, 60000) if ref == 2 else rng.choice((rng.randrange(0, 1 << 18), rng.randrange(0, 3 << 14)))
        ln = rng.choice((1, 50, 150, 151, 9000))
        ln = min(ln, REFS[ref] - pos)
        ops = rng.choice((((ln, 0),), ((5, 4), (ln, 0), (3, 1)), ((ln, 7),))) if rng.random() < 0.9 else ()
        out.append(rec(ref, pos, ops, flag=4 if rng.random() < 0.1 else 0, pad=rng.randrange(300)))
    return sorted(out, key=lambda r: key(r))


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 1))
def test_record_counts(ctx, n):
    check_merge(ctx, spread(random.Random(n), n), file_off=n * 977)


def test_members_and_lengths(ctx):
    """A record that starts in one 32 KiB member and ends in the next, one that ends exactly on a member boundary, one
    longer than 32 KiB, one that ends exactly at the text's end."""
    a = rec(0, 10, pad=200)
    fill = 32768 - 3 * len(a) - 60
    records = [a, a, a, rec(0, 11, pad=fill - len(rec(0, 11))), rec(0, 12, pad=100),          # the fourth ends at 32768 - 60, the fifth straddles
               rec(0, 13, pad=0)]
    at = sum(len(r) for r in records)
    records.append(rec(0, 14, pad=65536 - at - len(rec(0, 14))))                               # ends exactly on 65536
    records.append(rec(0, 15, pad=40000))                                                      # longer than a member
    at = sum(len(r) for r in records)
    records.append(rec(2, 16, pad=(-at - len(rec(2, 16))) % 32768))                            # the text ends on a member boundary
    assert sum(len(r) for r in records[:7]) == 65536 and sum(len(r) for r in records) % 32768 == 0
    check_merge(ctx, records, file_off=123456789)
    check_merge(ctx, records[:-1] + [rec(2, 16, pad=5)])                                        # ... and inside a member


def test_every_start_residue(ctx):
    records, at = [], 0
    seen = set()
    rng = random.Random(2)
    for i in range(400):
        r = rec(0, 100 + i, ((rng.randrange(1, 300), 0), (2, 1), (rng.randrange(1, 99), 2)), pad=rng.randrange(0, 33), name=b"n" * rng.randrange(1, 9))
        seen.add(at % 16)
        at += len(r)
        records.append(r)
    assert seen == set(range(16))
    check_merge(ctx, records)


def test_positions_and_bins(ctx):
    big = 3
    records = [
        rec(0, 0, ((1, 0),)),                                            # POS 0
        rec(0, (1 << 14) - 5, ((10, 0),)),                               # crosses 2^14
        rec(0, (1 << 17) - 5, ((10, 0),)),                               # crosses 2^17
        rec(0, (1 << 20) - 1, ((2, 8),)),
        rec(0, (1 << 23) - 1, ((2, 0),)),
        rec(0, (1 << 26) - 7, ((3, 0), (10, 2), (3, 0))),                # crosses 2^26: bin 0
        rec(0, (1 << 26) + 100, ((50, 0), (3 << 14, 3), (50, 0))),       # an N of three windows
        rec(0, (1 << 27), ((20, 0), ((5 << 14) + 3, 2), (1, 0))),        # a D of five
        rec(0, MAXLEN - 100, ((100, 0),)),                               # ends at 2^29
        rec(big, MAXLEN - 1, ((1, 0),)),
        rec(big, MAXLEN - 1, (), flag=4),                                # a 0x4 record at the last base
    ]
    rows, want = check_merge(ctx, records)
    assert [w["bin"] for w in want[:6]] == [4681, 585, 73, 9, 1, 0]
    assert want[8]["stop"] == MAXLEN
    assert all(w["bin"] != 0xBEEF for w in want)


def test_unmapped_mates_of_another_bin_and_unplaced_reads(ctx):
    """A 0x4 record in front of its mapped mate at the same POS: [POS, POS + 1) is in a leaf bin, the mate that crosses
    a window is not -- two chunks, and the 0x4 record in the linear index."""
    p = (1 << 14) - 50
    records = []
    for i in range(40):
        records += [rec(0, p + i, (), flag=4 | 64), rec(0, p + i, ((100, 0),), flag=8 | 128)]
    records += [rec(0, 5 << 14, (), flag=4)]                           # alone in its window
    records += [rec(-1, -1, (), flag=4 | 8, pad=i) for i in range(300)]
    rows, want = check_merge(ctx, records)
    assert sorted({r[0] for r in rows}) == [585, 4681, 4686] and len(rows) == 81
    lin, counts = simuscop_amd.bamindex_finish(ctx, REFS)
    assert lin[5] == want[80]["voff"] and counts[-1] == 300 and counts[1] == 41


def test_a_block_that_spans_two_references(ctx):
    records = [rec(0, 100 + i) for i in range(200)] + [rec(2, i, flag=4 if i % 3 == 0 else 0) for i in range(100)] + \
              [rec(3, 7, pad=i) for i in range(300)]
    check_merge(ctx, records)


def deflate_call(ctx, text, file_off, skip, lens):
    members = simuscop_amd.deflate_bgzf(ctx, text)
    rows, first = simuscop_amd.bamindex_add(ctx, simuscop_amd.BAMINDEX_DEFLATE, file_off, skip, lens)
    return members, rows, first


@pytest.mark.parametrize("seed", range(4))
def test_texts_of_sg_deflate_bgzf_chained(ctx, seed):
    """Two texts cut inside a record, the first with a front that belongs to no record of the index: each call's rows
    against the model, and the two calls joined equal the model of the concatenation."""
    rng = random.Random(50 + seed)
    records = spread(rng, rng.choice((40, 700, 3000)))
    records = [r for r in records if M.fields(r)[0] >= 0] + [r for r in records if M.fields(r)[0] < 0][:seed]
    front = bytes(rng.randrange(256) for _ in range(rng.choice((1, 35, 333))))
    text = front + b"".join(records)
    starts, at = [], len(front)
    for r in records:
        starts.append(at)
        at += len(r)
    k = rng.randrange(1, len(records) - 1)                             # the record the cut goes through
    cut = starts[k] + rng.choice((1, 3, 4, 11, 35, len(records[k]) - 1))
    simuscop_amd.bamindex_begin(ctx, REFS)
    m1, rows1, first1 = deflate_call(ctx, text[:cut], 1000, len(front), [len(r) for r in records[:k + 1]])
    m2, rows2, first2 = deflate_call(ctx, text[cut:], 1000 + len(m1), starts[k + 1] - cut, [len(r) for r in records[k + 1:]])
    lin, counts = simuscop_amd.bamindex_finish(ctx, REFS)
    mm = M.MemberMap(m1 + m2, 1000)
    want = model_recs(records, mm, len(front))
    assert rows1 == M.chunk_rows(want[:k]) and first1 == want[0]["voff"]
    assert rows2 == M.chunk_rows(want[k:]) and first2 == want[k]["voff"]          # the cut record is the second call's first
    assert (lin, counts) == M.linear_and_counts(want, REFS)
    # joined as the driver joins them, against the model of the whole
    eof = (1000 + len(m1) + len(m2)) << 16
    rows = [(a, b, first2 if e == M.OPEN else e) for a, b, e in rows1] + [(a, b, eof if e == M.OPEN else e) for a, b, e in rows2]
    bai, _, _ = simuscop_amd.bai_build(REFS, rows, lin, counts)
    for a, b in zip(want, want[1:]):
        a["end"] = b["voff"]
    want[-1]["end"] = eof
    assert bai == M.serialise(*M.index(want, len(REFS)))


def test_refusals_leave_the_context_working(ctx):
    eng = simuscop_amd.load_engine()
    records = [rec(0, 5), rec(2, 9)]
    check_merge(ctx, records)
    with pytest.raises(simuscop_amd.SimuError, match="2\\^29"):
        simuscop_amd.bamindex_begin(ctx, [1000, MAXLEN + 1])
    simuscop_amd.deflate_bgzf(ctx, b"x" * 100)                          # now the merge is no longer the latest compression
    with pytest.raises(simuscop_amd.SimuError, match="latest compression"):
        simuscop_amd.bamindex_add(ctx, simuscop_amd.BAMINDEX_MERGE, 0)
    simuscop_amd.bamsort_merge(ctx, [(b"".join(records), [key(r) for r in records], [len(r) for r in records])])
    with pytest.raises(simuscop_amd.SimuError, match="latest compression"):
        simuscop_amd.bamindex_add(ctx, simuscop_amd.BAMINDEX_DEFLATE, 0, 0, [len(records[0])])
    with pytest.raises(simuscop_amd.SimuError, match="sg_bamsort_merge first"):
        c2 = C.c_void_p()
        assert eng.sg_create(C.byref(c2), 0, 1) == 0
        try:
            simuscop_amd.bamindex_begin(c2, REFS)
            simuscop_amd.bamindex_add(c2, simuscop_amd.BAMINDEX_MERGE, 0)
        finally:
            eng.sg_destroy(c2)
    with pytest.raises(simuscop_amd.SimuError, match="outside its reference"):   # a record behind its reference's end
        bad = [rec(1, 4990, ((20, 0),))]
        simuscop_amd.bamsort_merge(ctx, [(bad[0], [key(bad[0])], [len(bad[0])])])
        simuscop_amd.bamindex_add(ctx, simuscop_amd.BAMINDEX_MERGE, 0)
    check_merge(ctx, records)
