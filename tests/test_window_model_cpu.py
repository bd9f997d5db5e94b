"""The plain model of the device window planner (tests/window_model.py) and the inputs of tests/test_gpu_window_plan.py,
without a GPU.

First half: hand-worked cases, every number written out.  With std = 0 the factor is means[gc] exactly, so weights,
segment sums, counts, the remainder, planned fragments and slots follow by arithmetic on paper.

Second half: the inputs of the GPU test discriminate.  Each property asserted here on the exact inputs the GPU test
runs is the reason why a device that is wrong in the stated way fails there: a fused z, a reassociated segment sum, a
count rounded to nearest, an atomic on the wrong segment."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import window_model as WM
from window_model import Gen, Model

# ---- hand-worked: frag 4, std 0 ------------------------------------------------------------------------------------------
#            AAAA CCGG ACGT NACG GGA  C
HAND_CHAIN = b"AAAACCGGACGTNACGGGAC"
HAND_MEANS = [0.0] * 101
for _g, _v in ((0, 1.0), (50, 2.0), (66, 2.25), (100, 3.0)):
    HAND_MEANS[_g] = _v
HAND_GENS = [Gen(0, 19, 0, 0), Gen(19, 1, 0, 0), Gen(8, 8, 0, 2)]     # segment 1 has no generator


def hand_model(full_tile_form):
    return Model(HAND_MEANS, 0.0, WM.quantile_table(3), 3, 4, full_tile_form, 9)


def test_hand_tiling_gc_and_ordinals():
    t = WM.tile(HAND_GENS, 4, 3)
    assert t.start == [0, 4, 8, 12, 16, 19, 8, 12]
    assert t.len == [4, 4, 4, 4, 3, 1, 4, 4]                   # a generator's last window is shorter; a last window of 1 base
    assert t.seg == [0, 0, 0, 0, 0, 0, 2, 2]
    assert t.ord == [0, 1, 2, 3, 4, 5, 0, 1]                   # the ordinal runs on into the segment's second generator
    assert t.seg_first == [0, 6, 6, 8] and t.gen_first == [0, 5, 6, 8]
    assert WM.gc_of([HAND_CHAIN], t.chain, t.start, t.len) == [0, 100, 50, -1, 66, 100, 50, -1]   # 100 * 2 // 3 = 66; an N: -1
    assert WM.gc_percent(b"ACRG") == 50 and WM.gc_percent(b"RRRR") == 0 and WM.gc_percent(b"RN") == -1   # R: neither GC nor N


@pytest.mark.parametrize("full_tile_form", [0, 1])
def test_hand_weights_and_segment_sums(full_tile_form):
    """f = means[gc]: 1, 3, 2, 0 (N), 2.25, 3.  Full windows: f / 4 (or f * 4 / 16, the same number at a power of two);
    the window of 3 bases 2.25 * 3 / 16, the window of 1 base 3 * 1 / 16.  All are exact in binary."""
    _, w, seg_w = WM.build([HAND_CHAIN], HAND_GENS, 3, hand_model(full_tile_form), seed=5)
    assert w == [0.25, 0.75, 0.5, 0.0, 0.421875, 0.1875, 0.5, 0.0]
    assert seg_w == [2.109375, 0.0, 0.5]                        # 0.25 + 0.75 + 0.5 + 0 + 0.421875 + 0.1875; nothing; 0.5 + 0


def test_the_two_weight_forms_differ_where_frag_is_no_power_of_two():
    m0, m1 = WM.model(37, full_tile_form=0), WM.model(37, full_tile_form=1)
    f = 0.1
    assert WM.weight(f, 37, m1) == f / 37 and WM.weight(f, 37, m0) == f * 37 / 1369
    fs = [k / 997 for k in range(1, 200)]                       # (the last bit, for a share of the factors)
    assert sum(1 for x in fs if WM.weight(x, 37, m1) != WM.weight(x, 37, m0)) >= 20
    assert WM.weight(f, 36, m1) == WM.weight(f, 36, m0) == f * 36 / 1369


def hand_plan(reads0, reads2, paired):
    t, w, seg_w = WM.build([HAND_CHAIN], HAND_GENS, 3, hand_model(1), seed=5)
    gens = WM.active_gens(HAND_GENS, t, [0, 2])
    assert [(g.seg, g.first_window) for g in gens] == [(0, 0), (0, 5), (1, 6)]
    return WM.plan(w, gens, [(reads0, seg_w[0]), (reads2, seg_w[2])], 4, paired)


def test_hand_counts_remainder_and_slots():
    """Segment 0, 10 reads, W = 2.109375 (the 2.2204e-16 is below half a unit in its last place and changes nothing):
    w * 10 / W = 1.185, 3.556, 2.370, 0, exactly 2.0, 0.889 -> 1 3 2 0 2 0, sum 8, the missing 2 go to the first window.
    Segment 2, 3 reads, W = 0.5: 0.5 + 2.2204e-16 is two units above 0.5, 1.5 / that = 2.9999999999999987 -> 2 (not 3),
    the window with the N gets 0, the missing read goes to the first window."""
    p = hand_plan(10, 3, paired=1)
    assert [r[4] for r in p.rows] == [3, 3, 2, 0, 2, 0, 3, 0]
    assert p.remainder == [2, 1]
    assert p.raw[4] == 2.0 and p.raw[6] == 2.9999999999999987
    assert [round(q) for q in p.raw[:6]] == [1, 4, 2, 0, 2, 1]                       # rounding to nearest: other counts
    # paired: planned = (n + 1) // 2 -> 2 2 1 0 1 0 | 2 0
    assert [r[6] for r in p.rows] == [0, 2, 4, 5, 5, 6, 6, 8] and p.slot_first == [0, 6, 8] and p.slots == [6, 2]
    assert [r[:4] + r[5:6] for r in p.rows] == [(0, 0, 0, 4, 0), (0, 0, 4, 4, 0), (0, 0, 8, 4, 0), (0, 0, 12, 4, 0), (0, 0, 16, 3, 0),
                                                (19, 0, 0, 1, 0), (8, 0, 0, 4, 1), (8, 0, 4, 4, 1)]
    s = hand_plan(10, 3, paired=0)                                                    # single: planned = n
    assert [r[4] for r in s.rows] == [3, 3, 2, 0, 2, 0, 3, 0]
    assert [r[6] for r in s.rows] == [0, 3, 6, 8, 8, 10, 10, 13] and s.slots == [10, 3]


def test_hand_fewer_reads_than_windows():
    p = hand_plan(1, 1, paired=1)                   # every quotient is below 1: all reads are the first window's remainder
    assert [r[4] for r in p.rows] == [1, 0, 0, 0, 0, 0, 1, 0] and p.remainder == [1, 1] and p.slots == [1, 1]
    assert [r[6] for r in p.rows] == [0, 1, 1, 1, 1, 1, 1, 2]


def test_hand_slice():
    p = hand_plan(10, 3, paired=1)
    assert WM.slice_rows(p, 1, 2) == [(8, 0, 0, 4, 3, 0, 0), (8, 0, 4, 4, 0, 0, 2)]
    assert WM.slice_rows(p, 0, 1) == p.rows[:6] and WM.slice_rows(p, 0, 2) == p.rows


def _oracle_word0(lib, c, key):
    out = (ctypes.c_uint32 * 4)()
    lib.orc_philox4x32_10((ctypes.c_uint32 * 4)(*c), (ctypes.c_uint32 * 2)(*key), out)
    return out[0]


def test_draw_address_and_redraw_against_the_oracle_philox(oracle_lib):
    """The draw of a window: word 0 of the oracle's Philox at (window ordinal, attempt, segment ordinal, 2 | ctx24 << 8),
    key (seed low, seed high).  Two cells, Q = (-1, 0, 2): z = Q[k] + (Q[k+1] - Q[k]) * t; with mean 0 the first
    attempt whose draw falls into the upper cell is taken, worked here from the oracle's words."""
    seed, ctx24 = 0x0000_0007_0000_0009, 0x03_0004
    ords, segs = [0, 1, 2, 5, 0xFFFF_FFFF, 77], [0, 0, 3, 3, 9, 0xFFFF_FFF0]
    for a in (0, 1, 4):
        got = WM.gc_words(ords, a, segs, ctx24, seed).tolist()
        assert got == [_oracle_word0(oracle_lib, (o, a, s, 2 | (ctx24 << 8)), (9, 7)) for o, s in zip(ords, segs)]
    m = Model([0.0] * 101, 1.0, [-1.0, 0.0, 2.0], 1, 16, 1, ctx24)
    d = WM.factors([50] * len(ords), ords, segs, m, seed)
    for i, (o, s) in enumerate(zip(ords, segs)):
        a = 0
        while True:
            x = _oracle_word0(oracle_lib, (o, a, s, 2 | (ctx24 << 8)), (9, 7))
            t = (2 * (x & 0x7FFF_FFFF) + 1) / 2.0 ** 32
            z = -1.0 + 1.0 * t if x >> 31 == 0 else 0.0 + 2.0 * t
            if z >= 0.0:
                break
            a += 1
        assert (d.f[i], d.attempts[i]) == (z, a + 1)
    assert max(d.attempts) > 1 and min(d.attempts) == 1
    assert WM.factors([-1, -1], [0, 1], [0, 0], m, seed).f == [0.0, 0.0]             # an N: factor 0, no draw


# ---- the inputs of the GPU test ------------------------------------------------------------------------------------------
def z_one_rounding(qk, d, t):
    """what fma(d, t, Q[k]) returns"""
    return float(Fraction(d) * Fraction(t) + Fraction(qk))


@pytest.fixture(scope="module")
def built():
    """{frag: (gens, n_segs, note, tiling, gc, draws, weights, segment weights)} of the sg_windows_build inputs"""
    out = {}
    for frag, kw in WM.BUILD_ARGS.items():
        gens, n_segs, note = WM.build_gens(frag, **kw)
        m = WM.model(frag)
        t = WM.tile(gens, frag, n_segs)
        gc = WM.gc_of(WM.chains(), t.chain, t.start, t.len)
        d = WM.factors(gc, t.ord, t.seg, m, WM.SEEDS[0])
        w = [WM.weight(f, n, m) for f, n in zip(d.f, t.len)]
        out[frag] = (gens, n_segs, note, t, gc, d, w, WM.segment_weights(w, t.seg_first))
    return out


def test_inputs_stay_within_their_sizes(built):
    assert sum(len(c) for c in WM.chains()) < 2_000_000
    for frag, (gens, n_segs, note, t, *_ ) in built.items():
        assert t.n < 40_000, frag
    sizes = {frag: sorted({b[3].seg_first[k + 1] - b[3].seg_first[k] for k in range(b[1])}) for frag, b in built.items()}
    for frag in (16, 37):
        assert set(sizes[frag]) >= {0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 8193}
    assert set(sizes[1000]) >= {0, 1, 2, 63, 64, 65, 4097}
    gens, n_segs = WM.many_gens()
    assert len(gens) == 2_000 and WM.tile(gens, 16, n_segs).n < 40_000
    assert len(WM.explicit_windows()) < 40_000
    for frag, (gens, n_segs, note, t, *_ ) in built.items():           # generators of 1, frag - 1, frag, frag + 1, k * frag bases
        assert {1, frag - 1, frag, frag + 1, 64 * frag} <= {g.hap_len for g in gens}
        assert {len([g for g in gens if g.seg == s]) for s in range(10)} >= {0, 1, 2, 3}
        assert t.seg_first[4] == t.seg_first[3] and t.seg_first[n_segs] == t.seg_first[n_segs - 1]   # unnamed: middle, end


def test_segment_sums_depend_on_the_order(built):
    """For a segment of more than 4,096 windows the left-to-right sum differs in bits from numpy's pairwise sum, from the
    right-to-left sum, and from the sum of 4,096-window tiles whose halves are added separately."""
    for frag in (16, 37):
        *_, t, gc, d, w, seg_w = built[frag]
        differing = 0
        for k in (7, 8, 9):
            ws = w[t.seg_first[k]:t.seg_first[k + 1]]
            assert len(ws) > 4096 or k == 7
            halves = 0.0
            for b in range(0, len(ws), 4096):
                tile = ws[b:b + 4096]
                halves = halves + (WM.left_to_right(tile[:len(tile) // 2]) + WM.left_to_right(tile[len(tile) // 2:]))
            others = (float(np.sum(np.array(ws))), WM.left_to_right(ws[::-1]), halves)
            differing += all(o != seg_w[k] for o in others)
        assert differing >= 1, frag
    ws = built[16][6][built[16][3].seg_first[9]:built[16][3].seg_first[10]]
    assert len(ws) == 8193 and float(np.sum(np.array(ws))) != built[16][7][9] != WM.left_to_right(ws[::-1])


def _fused_counts(gc, ords, segs, lens, m, seed):
    """(weighed windows, those whose z differs with one rounding, those whose weight differs)"""
    two = WM.factors(gc, ords, segs, m, seed)
    one = WM.factors(gc, ords, segs, m, seed, z_fn=z_one_rounding)
    weighed = [i for i in range(len(gc)) if gc[i] >= 0]
    z_diff = sum(1 for i in weighed if WM.z_two_roundings(*two.taken[i]) != z_one_rounding(*two.taken[i]))
    w_diff = sum(1 for i in weighed if WM.weight(two.f[i], lens[i], m) != WM.weight(one.f[i], lens[i], m))
    return np.array([len(weighed), z_diff, w_diff])


def test_a_fused_z_changes_weights(built):
    """z with one rounding (an FMA) differs from z with two for at least 1 % of the weighed windows, and the weight
    with it: over the builds, and over the explicit windows of sg_window_weights.  How often the two differ is a matter
    of the table: in a cell 2^-12 or 2^-20 wide the product (Q[k+1] - Q[k]) * t lies ten or twenty binary places below
    Q[k], and its own rounding reaches the sum's last place once in about 2^10 or 2^20 draws; with two cells the product
    is as large as the sum and a quarter of the draws differ.  Hence the two-cell table for the build with the long
    segments and in the explicit windows; the finer tables are there for their indexes, not for this."""
    total = np.zeros(3, dtype=np.int64)
    for frag in (16, 37, 1000):
        gens, n_segs, note, t, gc, *_ = built[frag]
        n = min(t.n, 6_000)
        c = _fused_counts(gc[:n], t.ord[:n], t.seg[:n], t.len[:n], WM.model(frag), WM.SEEDS[0])
        if WM.LG_OF_FRAG[frag] == 1:
            assert c[1] >= 0.01 * c[0] and c[2] >= 0.01 * c[0], (frag, c)
        total += c
    assert total[1] >= 0.01 * total[0] and total[2] >= 0.01 * total[0], total
    rows = WM.explicit_windows()
    segs, ords = WM.explicit_ordinals(len(rows))
    gc = WM.gc_of(WM.chains(), *zip(*rows))
    total = np.zeros(3, dtype=np.int64)
    for lg in (1, 12, 20):
        c = _fused_counts(gc, ords, segs, [r[2] for r in rows], WM.model(16, lg_cells=lg), WM.SEEDS[0])
        if lg == 1:
            assert c[1] >= 0.01 * c[0] and c[2] >= 0.01 * c[0], (lg, c)
        total += c
    assert total[1] >= 0.01 * total[0] and total[2] >= 0.01 * total[0], total


def test_redraws_cells_and_gc_values(built):
    redraws = deep = 0
    for frag, (gens, n_segs, note, t, gc, d, w, seg_w) in built.items():
        redraws += sum(a - 1 for a in d.attempts if a > 1)
        deep += sum(1 for a in d.attempts if a >= 4)                # attempt index a >= 3
        assert {-1, 0, 100} <= set(gc), frag
        assert 0.25 < sum(1 for a in d.attempts if a > 1) / sum(1 for a in d.attempts if a) < 0.5    # about a third is redrawn
        lg = WM.LG_OF_FRAG[frag]
        if lg <= 12:
            assert {0, (1 << lg) - 1} <= set(d.cells), frag          # the first and the last cell of the table
    assert redraws >= 1000 and deep >= 1
    rows = WM.explicit_windows()
    segs, ords = WM.explicit_ordinals(len(rows))
    gc = WM.gc_of(WM.chains(), *zip(*rows))
    assert {-1, 0, 100} <= set(gc)
    d = WM.factors(gc, ords, segs, WM.model(16, lg_cells=1), WM.SEEDS[0])
    assert {0, 1} <= set(d.cells) and max(d.attempts) >= 4


def test_seeds_and_contexts_give_other_draws():
    o, s = list(range(50)), [3] * 50
    base = WM.gc_words(o, 0, s, WM.CTX24S[0], WM.SEEDS[0]).tolist()
    assert base != WM.gc_words(o, 0, s, WM.CTX24S[1], WM.SEEDS[0]).tolist()
    assert base != WM.gc_words(o, 0, s, WM.CTX24S[0], WM.SEEDS[1]).tolist()


def _mixed(built, frag):
    gens, n_segs, note, t, gc, d, w, seg_w = built[frag]
    segs = WM.all_segments(t)
    ag = WM.active_gens(gens, t, segs)
    return {paired: WM.plan(w, ag, WM.active_rows(t, seg_w, segs, "mixed"), frag, paired) for paired in (0, 1)}, segs


@pytest.fixture(scope="module")
def mixed_plans(built):
    return _mixed(built, 16)


def test_the_plan_inputs_reach_every_rule(built, mixed_plans):
    plans, segs = mixed_plans
    gens, n_segs, note, t, *_ = built[16]
    assert len(segs) >= 200 and segs != list(range(len(segs)))         # active segments skip stored (empty) ordinals
    p = plans[1]
    n_act = len(segs)
    assert len(p.rows) < 40_000 and plans[0].slot_first[-1] < 300_000
    assert sum(1 for q in p.raw if int(q) != round(q)) >= 1             # nearest instead of truncation: another count
    assert sum(1 for r in p.remainder if r > 0) >= 1
    sizes = [p.seg_first[a + 1] - p.seg_first[a] for a in range(n_act)]
    reads = [WM.reads_of("mixed", a, sizes[a]) for a in range(n_act)]
    assert any(r < n for r, n in zip(reads, sizes)) and any(r == n for r, n in zip(reads, sizes)) and 1 in reads and max(reads) > 2000
    assert any(n > 4096 for n in sizes)
    # waves of 64 consecutive windows: three or more segments, one segment only, beginning inside a segment
    seg_of = [r[5] for r in p.rows]
    waves = [seg_of[i:i + 64] for i in range(0, len(seg_of), 64)]
    assert any(len(set(x)) >= 3 for x in waves) and any(len(set(x)) == 1 for x in waves)
    assert any(i and seg_of[i] == seg_of[i - 1] for i in range(0, len(seg_of), 64))
    # one atomic per wave on the first lane's segment would move reads between segments: some wave holds a window of
    # another segment than its first lane's with a count above zero
    assert any(r[4] > 0 and r[5] != seg_of[i - i % 64] for i, r in enumerate(p.rows))
    # the segment whose windows all hold an N: weight 0.0, every read is the first window's
    a_n = segs.index(note["all_n"])
    rows_n = p.rows[p.seg_first[a_n]:p.seg_first[a_n + 1]]
    assert built[16][7][note["all_n"]] == 0.0 and rows_n[0][4] == reads[a_n] and all(r[4] == 0 for r in rows_n[1:])


@pytest.mark.parametrize("frag", [16, 37])
def test_the_cuts_of_the_runs(built, frag):
    """WM.CUTS: one run is a single segment (of 8,193 windows), one begins at a segment whose first window got a
    remainder; the sampled batches stay under 300,000 planned fragments."""
    plans, segs = _mixed(built, frag)
    n = len(segs)
    single = remainder_first = 0
    for k, m in WM.CUTS[frag]:
        assert 0 < k < m < n
        for a0, a1 in ((0, k), (k, m), (m, n)):
            single += a1 - a0 == 1
            remainder_first += a0 > 0 and plans[1].remainder[a0] > 0
    assert single >= 1 and remainder_first >= 1
    assert any(plans[1].seg_first[a1] - plans[1].seg_first[a0] > 4096 for k, m in WM.CUTS[frag] for a0, a1 in ((0, k), (k, m), (m, n)))
    assert plans[0].slot_first[-1] < 300_000 and len(plans[0].rows) < 40_000
    seg_of = [r[5] for r in plans[1].rows]
    assert any(len(set(seg_of[i:i + 64])) >= 3 for i in range(0, len(seg_of), 64))       # the wave-straddling segments are in


def test_subset_plan_points_into_the_store(built):
    gens, n_segs, note, t, gc, d, w, seg_w = built[16]
    segs = WM.subset_segments(t)
    assert segs == [0, 2, 4, note["all_n"]]
    ag = WM.active_gens(gens, t, segs)
    firsts = [g.first_window for g in ag]
    assert firsts == sorted(firsts) and firsts[0] == 0 and firsts[1] == t.seg_first[2] and firsts[-1] == t.seg_first[note["all_n"]]
    assert firsts[1] != 1                                                # not contiguous: stored segments are skipped
