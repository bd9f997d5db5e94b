"""The device window planner (sg_window_weights / sg_windows_build / sg_plan_windows / sg_plan_range) in plain Python,
written from the definitions in include/simuscop_amd.h (the comment blocks over sg_window_weights and sg_windows_build)
and from oracle/philox.h for the address of the GC draw -- not from the kernels.

Every floating-point value is a Python float (IEEE binary64); every operation is one `*`, `/`, `+` or `-` on two of
them, so each rounds once: no fused operation, no np.sum.  numpy is used for integers only (the Philox words of many
windows at once, byte counts).

  tile(gens, frag, n_segs)            windows of the generators, their segment and their ordinal in the segment
  gc_percent(window bytes)            100 * (#C + #G) // len, -1 with an N
  factors(...) / weight(...)          GC factor (redrawn while negative) and weight of a window
  segment_weights(...)                left-to-right sums
  plan(...)                           read counts, remainder, planned fragments, slot bases, slots per segment
  slice_rows(...)                     a run [a0, a1) of active segments as a batch of its own

The second half holds the inputs that tests/test_window_model_cpu.py examines and tests/test_gpu_window_plan.py runs: the
same functions make them on both sides."""
from __future__ import annotations

import dataclasses

import numpy as np

from test_philox_base_rounds import philox

KIND_GC = 2            # oracle/philox.h: c0 = window ordinal in segment, c1 = attempt, c2 = segment ordinal -> word 0
TOTAL_EPS = 2.2204e-16  # Segment::setReadCount divides by totalWL + this


@dataclasses.dataclass
class Model:
    """sg_gc_model"""
    means: list            # [101] floats
    std: float
    quantiles: list        # [2^lg_cells + 1] floats
    lg_cells: int
    frag: int
    full_tile_form: int
    ctx24: int


@dataclasses.dataclass
class Gen:
    """sg_window_gen"""
    hap_base: int
    hap_len: int
    chain: int
    seg: int
    first_window: int = 0


@dataclasses.dataclass
class Tiling:
    chain: list
    start: list
    len: list
    seg: list              # segment ordinal of every window
    ord: list              # ordinal inside the segment, counted through all generators of the segment
    seg_first: list        # [n_segs + 1]
    gen_first: list        # [n_gens + 1]: first window of every generator

    @property
    def n(self):
        return len(self.len)


def n_windows(hap_len, frag):
    return (hap_len + frag - 1) // frag


def tile(gens, frag, n_segs):
    """A generator of hap_len bases gives ceil(hap_len / frag) windows, the last one shorter; generators come ordered by
    segment; a segment no generator names has no windows."""
    t = Tiling([], [], [], [], [], [0] * (n_segs + 1), [0])
    count = [0] * n_segs
    for g in gens:
        for i in range(n_windows(g.hap_len, frag)):
            t.chain.append(g.chain)
            t.start.append(g.hap_base + i * frag)
            t.len.append(min(frag, g.hap_len - i * frag))
            t.seg.append(g.seg)
            t.ord.append(count[g.seg])
            count[g.seg] += 1
        t.gen_first.append(t.n)
    for k in range(n_segs):
        t.seg_first[k + 1] = t.seg_first[k] + count[k]
    return t


def gc_percent(window: bytes):
    """calculateGCPercent: -1 with any N; other letters count as neither GC nor N."""
    if b"N" in window:
        return -1
    return 100 * (window.count(b"C") + window.count(b"G")) // len(window)


def gc_of(chains, chain, start, length):
    return [gc_percent(chains[c][s:s + n]) for c, s, n in zip(chain, start, length)]


def gc_words(win_ord, attempt, seg_ord, ctx24, seed):
    """Word 0 of Philox4x32-10 at (window ordinal, attempt, segment ordinal, kind | ctx24 << 8), key = the seed's halves."""
    c3 = (KIND_GC | (ctx24 << 8)) & 0xFFFFFFFF
    return philox(10, np.asarray(win_ord, dtype=np.uint64), attempt, np.asarray(seg_ord, dtype=np.uint64), c3,
                  k0=seed & 0xFFFFFFFF, k1=(seed >> 32) & 0xFFFFFFFF)[0]


def cell_and_t(x, lg_cells):
    """cell k = x >> (32 - lg_cells); t = (2 * low bits + 1) * 2^-(33 - lg_cells): the middle of the draw's own interval"""
    tail = 32 - lg_cells
    return x >> tail, float(2 * (x & ((1 << tail) - 1)) + 1) * 2.0 ** -(tail + 1)


def z_two_roundings(qk, d, t):
    return qk + d * t


@dataclasses.dataclass
class Draws:
    f: list                # the factor of every window (0.0 for GC -1)
    attempts: list         # attempts used (0 for GC -1): 1 = the first draw was taken
    cells: list            # the cell of every draw made, taken or not
    taken: list            # (Q[k], Q[k+1] - Q[k], t) of the draw that was taken, None for GC -1


def factors(gc, win_ord, seg_ord, m: Model, seed, z_fn=z_two_roundings):
    """0 for GC -1; else attempts a = 0, 1, ...: z = Q[k] + (Q[k+1] - Q[k]) * t, f = mean[gc] + std * z, the first
    f >= 0 is taken.  z_fn replaces the evaluation of z (the CPU test looks at what a fused one would give)."""
    n = len(gc)
    out = Draws([0.0] * n, [0] * n, [], [None] * n)
    Q = m.quantiles
    pending = [i for i in range(n) if gc[i] >= 0]
    a = 0
    while pending:
        words = gc_words([win_ord[i] for i in pending], a, [seg_ord[i] for i in pending], m.ctx24, seed).tolist()
        again = []
        for i, x in zip(pending, words):
            k, t = cell_and_t(x, m.lg_cells)
            out.cells.append(k)
            d = Q[k + 1] - Q[k]
            z = z_fn(Q[k], d, t)
            f = m.means[gc[i]] + m.std * z
            if f >= 0.0:
                out.f[i], out.attempts[i], out.taken[i] = f, a + 1, (Q[k], d, t)
            else:
                again.append(i)
        pending = again
        a += 1
    return out


def weight(f, length, m: Model):
    if m.full_tile_form and length == m.frag:
        return f / m.frag
    return f * length / (m.frag * m.frag)


def weights_of(chains, chain, start, length, seg_ord, win_ord, m: Model, seed):
    """What sg_window_weights returns: (weights, gc)"""
    gc = gc_of(chains, chain, start, length)
    f = factors(gc, win_ord, seg_ord, m, seed).f
    return [weight(x, n, m) for x, n in zip(f, length)], gc


def left_to_right(values):
    acc = 0.0
    for v in values:
        acc = acc + v
    return acc


def segment_weights(weights, seg_first):
    return [left_to_right(weights[seg_first[k]:seg_first[k + 1]]) for k in range(len(seg_first) - 1)]


def build(chains, gens, n_segs, m: Model, seed):
    """What sg_windows_build computes: (tiling, per-window weights = the store, per-segment weights)"""
    t = tile(gens, m.frag, n_segs)
    w, _ = weights_of(chains, t.chain, t.start, t.len, t.seg, t.ord, m, seed)
    return t, w, segment_weights(w, t.seg_first)


@dataclasses.dataclass
class Plan:
    rows: list             # sg_window rows: (hap_base, chain, spos, len, n_reads, seg, slot_base)
    seg_first: list        # [n_active + 1]
    slot_first: list       # [n_active + 1]
    remainder: list        # what the first window of every active segment got on top
    raw: list              # w * reads / (W + eps) of every window before truncation

    @property
    def slots(self):
        return [self.slot_first[a + 1] - self.slot_first[a] for a in range(len(self.seg_first) - 1)]


def planned_of(n_reads, paired):
    return 0 if n_reads <= 0 else ((n_reads + 1) // 2 if paired else n_reads)


def plan(store, gens, active, frag, paired):
    """store: the weights of sg_windows_build; gens: Gen rows with seg = index in `active` and first_window pointing into
    the store; active: (reads, W) per active segment."""
    rows, raw, seg_first = [], [], [0] * (len(active) + 1)
    for g in gens:
        reads, W = active[g.seg]
        for i in range(n_windows(g.hap_len, frag)):
            q = store[g.first_window + i] * reads / (W + TOTAL_EPS)
            raw.append(q)
            rows.append([g.hap_base, g.chain, i * frag, min(frag, g.hap_len - i * frag), int(q), g.seg, 0])
        seg_first[g.seg + 1] = len(rows)
    for a in range(len(active)):   # (an active segment without windows is refused by the device; here it would be empty)
        seg_first[a + 1] = max(seg_first[a + 1], seg_first[a])
    remainder = []
    for a, (reads, _) in enumerate(active):
        total = 0
        for r in rows[seg_first[a]:seg_first[a + 1]]:
            total += r[4]
        remainder.append(max(0, reads - total))
        if seg_first[a + 1] > seg_first[a]:
            rows[seg_first[a]][4] += remainder[-1]
    slot, slot_first = 0, []
    for i, r in enumerate(rows):
        if i == seg_first[r[5]]:
            slot_first.append(slot)
        r[6] = slot
        slot += planned_of(r[4], paired)
    slot_first.append(slot)
    return Plan([tuple(r) for r in rows], seg_first, slot_first, remainder, raw)


def slice_rows(p: Plan, a0, a1):
    """The rows of segments [a0, a1) with seg - a0 and slot_base - slot_first[a0]."""
    return [(hb, c, sp, ln, nr, seg - a0, sb - p.slot_first[a0]) for hb, c, sp, ln, nr, seg, sb in p.rows[p.seg_first[a0]:p.seg_first[a1]]]


# ------------------------------------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_window_plan.py, examined in tests/test_window_model_cpu.py
# ------------------------------------------------------------------------------------------------------------------------
SEEDS = (0x1234_5678_9ABC_DEF1, 77)
CTX24S = (0x02_0011, 5)             # population << 16 | chromosome
STD = 0.23
LG_OF_FRAG = {16: 1, 37: 12, 1000: 20}   # table size of each build (two cells: a fused z shows most often)
BUILD_ARGS = {16: dict(n_small=200, big=True), 37: dict(n_small=60, big=True), 1000: dict(n_small=3, big=False)}   # build_gens
CUTS = {16: ((8, 9), (50, 120)), 37: ((8, 9), (20, 45))}   # sg_plan_range runs [0, k), [k, m), [m, n) of a build's active segments
CHAIN0_LEN, CHAIN1_LEN = 1_100_000, 100_003
A_RUN, G_RUN, N_RUN = (10_000, 13_000), (20_000, 23_000), (70_000, 75_000)
N_SINGLES = [30_000 + 701 * k for k in range(40)]
OTHER_LETTERS = [60_000 + 997 * k for k in range(20)]


def _letters(n, tag):
    """n bytes of ACGT from Philox words (the same on every machine): GC content between 20 % and 80 %, changing every
    4,096 bytes."""
    words = philox(10, np.arange((n + 15) // 16, dtype=np.uint64), tag, 0, 0, k0=1, k1=2)
    u = np.ascontiguousarray(words.T).view(np.uint8).reshape(-1)[:n].astype(np.int64)
    block = np.arange(n) >> 12
    is_gc = (u >> 1) < 26 + (block * 37) % 77
    pick = np.where(is_gc, np.where(u & 1, ord("C"), ord("G")), np.where(u & 1, ord("A"), ord("T")))
    return pick.astype(np.uint8)


_CHAINS = []


def chains():
    """Two chains (1.2 MB together): runs of A, of G and of N, single N and single R bytes in chain 0; chain 1 of odd length."""
    if not _CHAINS:
        c0 = _letters(CHAIN0_LEN, 1)
        c0[A_RUN[0]:A_RUN[1]] = ord("A")
        c0[G_RUN[0]:G_RUN[1]] = ord("G")
        c0[N_RUN[0]:N_RUN[1]] = ord("N")
        c0[N_SINGLES] = ord("N")
        c0[OTHER_LETTERS] = ord("R")
        c1 = _letters(CHAIN1_LEN, 2)
        c1[5_000] = ord("N")
        _CHAINS.extend([c0.tobytes(), c1.tobytes()])
    return _CHAINS


_TABLES = {}


def quantile_table(lg_cells):
    """2^lg_cells + 1 increasing knots of a bell-shaped law of unit variance (the logistic one: the engine reads whatever
    table it is given), the end knots at 0.25 / n of the mass like the host's table."""
    if lg_cells not in _TABLES:
        n = 1 << lg_cells
        p = np.arange(n + 1, dtype=np.float64) / n
        p[0], p[n] = 0.25 / n, 1.0 - 0.25 / n
        _TABLES[lg_cells] = (np.log(p / (1.0 - p)) * (3.0 ** 0.5 / np.pi)).tolist()
    return _TABLES[lg_cells]


def model(frag, lg_cells=None, full_tile_form=1, ctx24=CTX24S[0], std=STD):
    """means between 0.2 and 0.4 std: more than a third of the first draws are negative and drawn again"""
    lg = LG_OF_FRAG[frag] if lg_cells is None else lg_cells
    return Model([std * (0.2 + 0.002 * g) for g in range(101)], std, quantile_table(lg), lg, frag, full_tile_form, ctx24)


# (a) explicit windows ----------------------------------------------------------------------------------------------------
WINDOW_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2051)


def explicit_windows():
    """(chain, start, len) rows for sg_window_weights: every length at the start offsets 0..15 of a 16-byte group, windows
    of one letter, with one N at the first, last and a middle byte, with a letter that is neither, in the second chain,
    and ending on the last byte of either chain (the last chain's last byte: the load that reaches furthest)."""
    rows = []
    for ln in WINDOW_LENGTHS:
        for off in range(16):
            rows.append((0, 200_000 + 4_096 * off + off, ln))
    for ln in (16, 37, 1000):
        rows += [(0, A_RUN[0] + 3, ln), (0, G_RUN[0] + 5, ln)]                  # GC 0 and GC 100
        n = N_SINGLES[3]
        rows += [(0, n, ln), (0, n - ln + 1, ln), (0, n - ln // 2, ln)]         # an N first, last, in the middle
        rows.append((0, OTHER_LETTERS[2] - ln // 3, ln))
        rows += [(1, 17, ln), (1, 4_990, ln), (1, CHAIN1_LEN - ln, ln), (0, CHAIN0_LEN - ln, ln)]
    rows += [(1, CHAIN1_LEN - 1, 1), (1, CHAIN1_LEN - 2051, 2051), (1, 0, 1025)]
    return rows


def explicit_ordinals(n):
    """segment and window ordinals of the explicit windows: small and large ones, not in step with each other"""
    return [(i * 7) % 13 if i % 5 else 3_000_000 + i for i in range(n)], [i if i % 3 else 0xFFFF_0000 + i for i in range(n)]


# (b) builds --------------------------------------------------------------------------------------------------------------
def small_sizes(n):
    """window counts 1..130 of n segments"""
    return [(i * 53) % 130 + 1 for i in range(n)]


def build_gens(frag, n_small=200, big=True):
    """(gens, n_segs, note) of one sg_windows_build call.  Segment ordinals:
      0: 1 window (hap_len 1)          1: 2 (frag + 1)             2: 63 (frag - 1 | 62 frag)      3: none
      4: 64 (k * frag)                 5: 65 (frag | frag + 1 | 62 frag - 3, on chain 1)
      6: 4095                          7: 4096 (two generators)    8: 4097 (three, two on chain 1)  9: 8193 (last of 1 base)
      10 .. 10 + n_small - 1: 1..130 windows each, over the runs of A, G, the single N and R bytes of chain 0
      then one over the run of N (every window holds an N), and a last ordinal that no generator names.
    Without `big` (frag 1000: 8,193 windows would be 8 MB) segment 6 has 4,097 windows from five generators that overlap
    on the chain, and 7..9 have none."""
    F = frag
    gens, note = [], {}
    pos = [250_000, 1_000]   # next free byte of chain 0 / chain 1

    def add(seg, hap_len, chain=0):
        gens.append(Gen(pos[chain], hap_len, chain, seg))
        pos[chain] += hap_len + 3        # (generators need not touch)

    add(0, 1)
    add(1, F + 1)
    add(2, F - 1), add(2, 62 * F)
    add(4, 64 * F)
    add(5, F, 1), add(5, F + 1, 1), add(5, 62 * F - 3, 1)
    if big:
        add(6, 4095 * F)
        add(7, 4000 * F), add(7, 96 * F - 5)
        add(8, 4000 * F + 1), add(8, 90 * F, 1), add(8, 6 * F - 1, 1)
        add(9, 8192 * F + 1)
    else:
        for i, k in enumerate((820, 820, 820, 820, 817)):
            gens.append(Gen(50_000 + 13 * i, k * F, 0, 6))
    pos[0] = 0
    sizes = small_sizes(n_small)
    for i, k in enumerate(sizes):
        add(10 + i, k * F - (i % F if k > 1 else 0))
    assert pos[0] <= 250_000
    note["all_n"] = 10 + n_small
    gens.append(Gen(N_RUN[0] + 1, min(N_RUN[1] - N_RUN[0] - 2, 313 * F), 0, note["all_n"]))
    n_segs = note["all_n"] + 2
    for g in gens:
        assert g.hap_base + g.hap_len <= (CHAIN0_LEN, CHAIN1_LEN)[g.chain]
    return gens, n_segs, note


def many_gens(n=2_000, frag=16):
    """n generators of 1..40 bases in one call, one to three a segment (gen_of's search over many)"""
    gens, seg = [], 0
    for i in range(n):
        gens.append(Gen(100 + 45 * i, (i * 29) % 40 + 1, i % 2, seg))
        if i % 3 != 1:
            seg += 1 + (i % 11 == 0)     # (now and then an ordinal that no generator names)
    return gens, seg + 1


# (c) plans ---------------------------------------------------------------------------------------------------------------
def active_gens(gens, tiling, segs):
    """The generators of the built segments `segs` as sg_plan_windows takes them: seg = index in the active list,
    first_window = the generator's first window in the store."""
    index = {s: a for a, s in enumerate(segs)}
    return [Gen(g.hap_base, g.hap_len, g.chain, index[g.seg], tiling.gen_first[i]) for i, g in enumerate(gens) if g.seg in index]


def reads_of(rule, a, n_win):
    if rule == "one":
        return 1
    if rule == "below":
        return max(1, n_win // 2)
    if rule == "equal":
        return n_win
    if rule == "thousands":
        return 2_000 + 37 * a
    assert rule == "mixed"
    return (1, max(1, n_win // 2), n_win, 300 + 11 * a)[a % 4] if n_win < 4000 else 5_000 + a


def subset_segments(tiling):
    """the 1st, 3rd, 4th and last of the built segments that have windows (the last one: every window holds an N)"""
    have = [k for k in range(len(tiling.seg_first) - 1) if tiling.seg_first[k + 1] > tiling.seg_first[k]]
    return [have[0], have[2], have[3], have[-1]]


def all_segments(tiling):
    return [k for k in range(len(tiling.seg_first) - 1) if tiling.seg_first[k + 1] > tiling.seg_first[k]]


def active_rows(tiling, seg_w, segs, rule):
    """(reads, W) per active segment"""
    return [(reads_of(rule, a, tiling.seg_first[s + 1] - tiling.seg_first[s]), seg_w[s]) for a, s in enumerate(segs)]
