"""The depth state and its finishing pass on the MI355X (sg_depth.hip) through Session and sg_depth_add_spans: spans the
test chooses go into the difference array, and what depth_fetch, depth_runs and depth_bins give back is compared with
numpy (add.at on a difference array, cumsum).  Lengths and span ends aim at the finishing pass's tile (depth_info)."""
import ctypes as C
import os

import numpy as np
import pytest

import simuscop_amd
import truth_util as U
from profile_shapes import Shape

pytestmark = pytest.mark.gpu

SG_ERR_INVALID = 1


@pytest.fixture(scope="module")
def sess(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("depth_spans"))
    prof = U.write_identity_profile(os.path.join(wd, "identity.profile"), Shape(3, 53))
    cfg, _, _ = U.acgt_case(wd, prof, "SE", lengths=(20000, 5000))
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=11) as s:
        yield s


def model_depth(ln, start, end):
    d = np.zeros(ln + 1, dtype=np.int64)
    np.add.at(d, start, 1)
    np.add.at(d, end, -1)
    return np.cumsum(d)[:ln]


def model_runs(depth):
    if not len(depth):
        return np.zeros((0, 2), dtype=np.uint32)
    starts = np.concatenate(([0], 1 + np.flatnonzero(depth[1:] != depth[:-1])))
    return np.stack([starts, depth[starts]], axis=1).astype(np.uint32)


def model_bins(depth, bin_width):
    if not len(depth):
        return np.zeros(0, dtype=np.uint64)
    return np.add.reduceat(depth.astype(np.uint64), np.arange(0, len(depth), bin_width))


def edge_spans(ln, tile):
    """Spans that start or end exactly at 0, LN and, for every tile boundary kT inside the contig, kT - 1, kT, kT + 1."""
    marks = {0, ln}
    for k in range(1, ln // tile + 2):
        marks |= {p for p in (k * tile - 1, k * tile, k * tile + 1) if 0 <= p <= ln}
    marks = sorted(marks)
    return [(a, b) for a in marks for b in marks if a <= b]


def spans_of(lengths, tile, seed, n_random):
    rng = np.random.default_rng(seed)
    cs, ss, es = [], [], []
    for c, ln in enumerate(lengths):
        edges = edge_spans(ln, tile)
        a = rng.integers(0, ln + 1, n_random)
        w = np.minimum(rng.geometric(1.0 / 150, n_random), ln - a)     # read-sized, cut at the contig's end
        s = np.concatenate([[e[0] for e in edges], a]).astype(np.uint64)
        e = np.concatenate([[e[1] for e in edges], a + w]).astype(np.uint64)
        cs.append(np.full(len(s), c, dtype=np.uint32))
        ss.append(s)
        es.append(e)
    order = rng.permutation(sum(len(x) for x in cs))                   # contigs mixed, as reads of several chains are
    return np.concatenate(cs)[order], np.concatenate(ss)[order], np.concatenate(es)[order]


def check_contig(sess, c, ln, want, tile, bins=True):
    assert np.array_equal(sess.depth_fetch(c, 0, ln), want.astype(np.uint32)), ("fetch", c, ln)
    got = sess.depth_runs(c)
    assert np.array_equal(got, model_runs(want)), ("runs", c, ln)
    if not bins:
        return
    for b in sorted({2, 7, tile, tile + 1, 1000, ln, ln + 5}):
        assert np.array_equal(sess.depth_bins(c, b), model_bins(want, b)), ("bins", c, ln, b)


def test_lengths_around_the_tile(sess):
    sess.depth_begin([1])                                 # (the tile size is read from a state)
    tile = sess.depth_info()[2]
    assert tile >= 256 and tile % 256 == 0
    lengths = [1, tile - 1, tile, tile + 1, 3 * tile + 1]
    sess.depth_begin(lengths)
    assert sess.depth_info() == (len(lengths), 0, tile)
    c, s, e = spans_of(lengths, tile, 1, 3000)
    sess.depth_add_spans(c, s, e)
    assert sess.depth_info()[1] == int((e - s).sum())
    for k, ln in enumerate(lengths):
        want = model_depth(ln, s[c == k].astype(np.int64), e[c == k].astype(np.int64))
        assert want.max() > 3 or ln == 1
        check_contig(sess, k, ln, want, tile)
        # a range that begins and ends inside tiles
        if ln > 10:
            assert np.array_equal(sess.depth_fetch(k, 5, ln - 9), want[5:ln - 4].astype(np.uint32))


def test_many_contigs_in_one_state(sess):
    sess.depth_begin([1])
    tile = sess.depth_info()[2]
    lengths = [500] * 300
    sess.depth_begin(lengths)
    c, s, e = spans_of(lengths, tile, 2, 2000)
    sess.depth_add_spans(c, s, e)
    order = np.argsort(c, kind="stable")
    cuts = np.searchsorted(c[order], np.arange(301))
    for k in range(300):
        idx = order[cuts[k]:cuts[k + 1]]
        want = model_depth(500, s[idx].astype(np.int64), e[idx].astype(np.int64))
        check_contig(sess, k, 500, want, tile, bins=k % 25 == 0)
        assert np.array_equal(sess.depth_bins(k, 7), model_bins(want, 7))


def test_identical_spans_pass_16_bits(sess):
    sess.depth_begin([1])
    tile = sess.depth_info()[2]
    ln = 2 * tile + 50
    sess.depth_begin([300, ln])
    n = 70000
    a = tile - 40                                         # the stretch lies across a tile boundary
    sess.depth_add_spans(np.full(n, 1, np.uint32), np.full(n, a, np.uint64), np.full(n, a + 100, np.uint64))
    want = np.zeros(ln, dtype=np.int64)
    want[a:a + 100] = n
    check_contig(sess, 1, ln, want, tile)
    assert int(sess.depth_bins(1, ln).sum()) == 7_000_000 == int(sess.depth_bins(1, 3).sum())
    assert sess.depth_runs(1).tolist() == [[0, 0], [a, n], [a + 100, 0]]
    assert not sess.depth_fetch(0, 0, 300).any() and sess.depth_runs(0).tolist() == [[0, 0]]


def test_state_adds_resets_and_is_replaced(sess):
    sess.depth_begin([1])
    tile = sess.depth_info()[2]
    lengths = [tile + 3, 700]
    sess.depth_begin(lengths)
    c, s, e = spans_of(lengths, tile, 3, 500)
    sess.depth_add_spans(c, s, e)
    sess.depth_runs(0)                                    # (a finishing pass between the two adds)
    sess.depth_add_spans(c, s, e)
    for k, ln in enumerate(lengths):
        want = 2 * model_depth(ln, s[c == k].astype(np.int64), e[c == k].astype(np.int64))
        check_contig(sess, k, ln, want, tile, bins=False)
    assert sess.depth_info()[1] == 2 * int((e - s).sum())
    sess.depth_reset()
    assert sess.depth_info() == (2, 0, tile)
    for k, ln in enumerate(lengths):
        assert not sess.depth_fetch(k, 0, ln).any()
        assert sess.depth_runs(k).tolist() == [[0, 0]] and not sess.depth_bins(k, 9).any()
    # other lengths: the state is replaced, what the first held is gone
    sess.depth_add_spans(c, s, e)
    other = [90, 2 * tile, 5]
    sess.depth_begin(other)
    assert sess.depth_info() == (3, 0, tile)
    for k, ln in enumerate(other):
        assert not sess.depth_fetch(k, 0, ln).any()
    sess.depth_add_spans([1, 2], [tile - 1, 0], [tile + 1, 5])
    assert sess.depth_runs(1).tolist() == [[0, 0], [tile - 1, 1], [tile + 1, 0]] and sess.depth_runs(2).tolist() == [[0, 1]]
    with pytest.raises(simuscop_amd.SimuError, match="contig"):
        sess.depth_fetch(3, 0, 1)


def _spans(contig, start, end):
    n = len(contig)
    return (C.c_uint32 * n)(*contig), (C.c_uint64 * n)(*start), (C.c_uint64 * n)(*end), n


def test_bad_spans_add_nothing(sess):
    lengths = [1000, 40]
    sess.depth_begin(lengths)
    sess.depth_add_spans([0, 1], [10, 0], [500, 40])
    before = [sess.depth_fetch(k, 0, ln) for k, ln in enumerate(lengths)]
    eng, ctx = sess.eng, sess.ctx
    for contig, start, end, word in (([0, 0, 0], [1, 2, 3], [5, 1001, 9], b"inside"),      # end > LN
                                     ([0, 1, 0], [1, 30, 3], [5, 20, 9], b"inside"),        # start > end
                                     ([0, 2, 0], [1, 0, 3], [5, 1, 9], b"contig"),          # no such contig
                                     ([1], [41], [41], b"inside")):
        assert eng.sg_depth_add_spans(ctx, *_spans(contig, start, end)) == SG_ERR_INVALID
        assert word in eng.sg_last_error(ctx), eng.sg_last_error(ctx)
        for k, ln in enumerate(lengths):
            assert np.array_equal(sess.depth_fetch(k, 0, ln), before[k])
    n = C.c_uint64()
    one = (C.c_uint64 * 1)()
    assert eng.sg_depth_bins(ctx, 2, 5, None, 0, C.byref(n)) == SG_ERR_INVALID and b"contig" in eng.sg_last_error(ctx)
    assert eng.sg_depth_runs(ctx, 2, None, 0, C.byref(n)) == SG_ERR_INVALID
    assert eng.sg_depth_bins(ctx, 0, 0, None, 0, C.byref(n)) == SG_ERR_INVALID
    assert eng.sg_depth_fetch(ctx, 1, 30, 11, (C.c_uint32 * 11)()) == SG_ERR_INVALID
    assert eng.sg_depth_bins(ctx, 0, 100, one, 1, C.byref(n)) != 0 and n.value == 10       # cap too small: the count, and an error


def test_calls_before_begin_are_refused():
    eng = simuscop_amd.load_engine()
    ctx = C.c_void_p()
    assert eng.sg_create(C.byref(ctx), 0, 1) == 0
    try:
        n, m = C.c_uint64(), C.c_uint64()
        a, b, t = C.c_uint32(), C.c_uint64(), C.c_uint32()
        calls = {
            "sg_depth_add": lambda: eng.sg_depth_add(ctx, C.byref(m)),
            "sg_depth_add_spans": lambda: eng.sg_depth_add_spans(ctx, *_spans([0], [0], [1])),
            "sg_depth_bins": lambda: eng.sg_depth_bins(ctx, 0, 10, None, 0, C.byref(n)),
            "sg_depth_runs": lambda: eng.sg_depth_runs(ctx, 0, None, 0, C.byref(n)),
            "sg_depth_fetch": lambda: eng.sg_depth_fetch(ctx, 0, 0, 1, (C.c_uint32 * 1)()),
            "sg_depth_reset": lambda: eng.sg_depth_reset(ctx),
            "sg_depth_info": lambda: eng.sg_depth_info(ctx, C.byref(a), C.byref(b), C.byref(t)),
            "sg_depth_end": lambda: eng.sg_depth_end(ctx),
        }
        for name, call in calls.items():
            assert call() == SG_ERR_INVALID, name
            assert name.encode() in eng.sg_last_error(ctx) and b"sg_depth_begin" in eng.sg_last_error(ctx)
        # begin .. end .. and the calls are refused again; a depth without a sampled pass cannot take one
        lens = (C.c_uint64 * 2)(100, 50)
        assert eng.sg_depth_begin(ctx, lens, 2) == 0, eng.sg_last_error(ctx)
        assert eng.sg_depth_add(ctx, C.byref(m)) == SG_ERR_INVALID
        assert eng.sg_depth_add_spans(ctx, *_spans([1], [0], [50])) == 0
        assert eng.sg_depth_end(ctx) == 0
        for name, call in calls.items():
            assert call() == SG_ERR_INVALID, name
    finally:
        eng.sg_destroy(ctx)
