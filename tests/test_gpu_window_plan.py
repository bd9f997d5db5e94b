"""The device window planner through its C ABI, call by call, against the plain model of tests/window_model.py:

  (a) sg_window_weights   gc_kernel, gc_weight_kernel               weights and GC% bit for bit
  (b) sg_windows_build    tile_kernel, gen_of, seg_sum_kernel        segment weights bit for bit, window counts
  (c) sg_plan_windows     window_reads_kernel, seg_remainder_kernel, planned_kernel, the u32 scan, slot_base_kernel,
                          seg_slots_kernel                           planned fragments of every active segment
  (d) sg_plan_range       slice_kernel, and the sg_window rows of (c), which never leave the device: the batch sampled from
                          them gives the text and the truth rows of the same batch planned on the host from the model's rows

Weights and sums are compared as bit patterns (uint64 views), counts, slots and text exactly: no tolerance.  The inputs
come from window_model.py; tests/test_window_model_cpu.py shows on the same inputs why a fused z, a reassociated segment
sum, a count rounded to nearest or an atomic on the wrong segment cannot pass here."""
import ctypes as C

import numpy as np
import pytest

import simuscop_amd
import window_model as WM
from simuscop_amd import SgActiveSeg, SgBatch, SgGcModel, SgGcWindow, SgWindow, SgWindowGen

pytestmark = pytest.mark.gpu

GC_WINDOW = np.dtype([("start", "<u8"), ("chain", "<u4"), ("len", "<u4")])
WINDOW_GEN = np.dtype([("hap_base", "<u8"), ("hap_len", "<u8"), ("chain", "<u4"), ("seg", "<u4"), ("first_window", "<u8")])
ACTIVE_SEG = np.dtype([("reads", "<i8"), ("weight", "<f8"), ("seg_size", "<u4"), ("pad", "<u4")])
WINDOW = np.dtype([("hap_base", "<u8"), ("chain", "<u4"), ("spos", "<u4"), ("len", "<u4"), ("n_reads", "<i4"), ("seg", "<u4"), ("slot_base", "<u4")])
assert (GC_WINDOW.itemsize, WINDOW_GEN.itemsize, ACTIVE_SEG.itemsize, WINDOW.itemsize) == tuple(
    C.sizeof(t) for t in (SgGcWindow, SgWindowGen, SgActiveSeg, SgWindow))
PREFIX = b"@pop#7#"
BATCH_ID = 0x1234


@pytest.fixture(scope="module")
def eng():
    return simuscop_amd.load_engine()


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Ctx:
    """One engine context holding the chains of window_model.chains(), uploaded as bytes."""

    def __init__(self, eng, seed=WM.SEEDS[0], chains=None, profile=False, upload=True):
        self.eng, self.ctx = eng, C.c_void_p()
        assert eng.sg_create(C.byref(self.ctx), 0, seed) == 0, eng.sg_last_error(None)
        self.keep = []
        if upload:
            bufs = WM.chains() if chains is None else chains
            arr = (C.c_char_p * len(bufs))(*bufs)
            lens = (C.c_uint64 * len(bufs))(*[len(b) for b in bufs])
            assert eng.sg_upload_haplotypes(self.ctx, len(bufs), arr, lens) == 0, self.err()
        if profile:
            self.load_profile()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.eng.sg_destroy(self.ctx)

    def err(self):
        return self.eng.sg_last_error(self.ctx).decode()

    def load_profile(self):
        """A small profile as tests/test_profile_shapes_cpu.py builds one: reads of 36 bases, k-mer 1, 6 bins, sequencing
        indels of up to 4 bases at 1 % each, a fixed insert size."""
        L, bins, n_qual, n_indel = 36, 6, 94, 4
        sub = np.tile(np.array([0.90, 0.94, 0.97, 1.0]), 4 * bins)
        qual = np.tile(np.linspace(1.0 / n_qual, 1.0, n_qual), 16 * bins)
        indel = np.linspace(1.0 / n_indel, 1.0, n_indel)
        p = simuscop_amd.SgProfileCdf(n_bases=4, bases=b"ACTG", kmer=1, bins=bins, read_length=L, n_qual=n_qual, min_qual=33,
                                      insert_rate=0.01, del_rate=0.01, n_ins=n_indel, n_del=n_indel, insert_size=90)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        p.ins_cdf = p.del_cdf = dp(indel)
        p.subs_cdf1, p.qual_cdf = dp(sub), dp(qual)
        assert self.eng.sg_load_profile(self.ctx, C.byref(p)) == 0, self.err()

    # ---- the calls -----------------------------------------------------------------------------------------------------
    def c_model(self, m: WM.Model):
        means, q = np.array(m.means, dtype=np.float64), np.array(m.quantiles, dtype=np.float64)
        self.keep = [means, q]
        return SgGcModel(ptr(means, C.c_double), m.std, ptr(q, C.c_double), m.lg_cells, m.frag, m.full_tile_form, m.ctx24)

    def window_weights(self, rows, segs, ords, m, want=0):
        """rows: (chain, start, len).  Returns (weights as uint64 bit patterns, gc) or the refusal's message."""
        n = len(rows)
        w = np.zeros(n, dtype=GC_WINDOW)
        w["chain"], w["start"], w["len"] = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
        so, wo = np.array(segs, dtype=np.uint32), np.array(ords, dtype=np.uint32)
        out, gc = np.full(n, np.nan), np.full(n, -99, dtype=np.int32)
        cm = self.c_model(m)
        rc = self.eng.sg_window_weights(self.ctx, ptr(w, SgGcWindow), ptr(so, C.c_uint32), ptr(wo, C.c_uint32), n, C.byref(cm),
                                        ptr(out, C.c_double), ptr(gc, C.c_int32))
        if want:
            assert rc != 0
            return self.err()
        assert rc == 0, self.err()
        return out.view(np.uint64), gc.tolist()

    def gc_percent(self, rows):
        """rows: (chain, start, len).  Returns the GC% of every window."""
        w = np.zeros(len(rows), dtype=GC_WINDOW)
        w["chain"], w["start"], w["len"] = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
        gc = np.full(len(rows), -99, dtype=np.int32)
        assert self.eng.sg_gc_percent(self.ctx, ptr(w, SgGcWindow), len(rows), ptr(gc, C.c_int32)) == 0, self.err()
        return gc.tolist()

    @staticmethod
    def c_gens(gens):
        g = np.zeros(max(len(gens), 1), dtype=WINDOW_GEN)
        for name in WINDOW_GEN.names:
            g[name][:len(gens)] = [getattr(x, name) for x in gens]
        return g

    def build(self, store_id, gens, n_segs, m, want=0):
        """Returns (segment weights as uint64 bit patterns, n_windows) or the refusal's message."""
        g = self.c_gens(gens)
        out, n = np.full(max(n_segs, 1), np.nan), C.c_uint64(0xDEAD)
        cm = self.c_model(m)
        rc = self.eng.sg_windows_build(self.ctx, store_id, ptr(g, SgWindowGen), len(gens), n_segs, C.byref(cm), ptr(out, C.c_double), C.byref(n))
        if want:
            assert rc != 0
            return self.err()
        assert rc == 0, self.err()
        return out[:n_segs].view(np.uint64), n.value

    def plan_windows(self, store_id, gens, active, frag, paired, batch_id=BATCH_ID, prefix=PREFIX, seg_size=None, want=0):
        """active: (reads, W) rows.  Returns (slots per active segment, n_windows) or the refusal's message."""
        g = self.c_gens(gens)
        a = np.zeros(max(len(active), 1), dtype=ACTIVE_SEG)
        a["reads"][:len(active)], a["weight"][:len(active)] = [r for r, _ in active], [w for _, w in active]
        a["seg_size"][:len(active)] = seg_sizes(len(active)) if seg_size is None else seg_size
        slots, n = np.full(max(len(active), 1), 0xDEAD, dtype=np.uint64), C.c_uint64(0xDEAD)
        rc = self.eng.sg_plan_windows(self.ctx, store_id, ptr(g, SgWindowGen), len(gens), ptr(a, SgActiveSeg), len(active), frag, batch_id,
                                      paired, prefix, ptr(slots, C.c_uint64), C.byref(n))
        if want:
            assert rc != 0
            return self.err()
        assert rc == 0, self.err()
        return slots[:len(active)].tolist(), n.value

    def plan_range(self, a0, a1, want=0):
        rc = self.eng.sg_plan_range(self.ctx, a0, a1)
        if want:
            assert rc != 0
            return self.err()
        assert rc == 0, self.err()

    def plan_host(self, rows, seg_first, n_active, paired):
        """sg_plan on a host-made batch of the model's rows: the same batch_id and prefix, first_window = first_slot = 0."""
        w = np.array(rows, dtype=WINDOW)
        ss, sf = np.array(seg_sizes(n_active), dtype=np.uint32), np.array(seg_first, dtype=np.uint32)
        b = SgBatch(BATCH_ID, paired, PREFIX, ptr(w, SgWindow), len(rows), ptr(ss, C.c_uint32), ptr(sf, C.c_uint32), n_active, 0, 0)
        assert self.eng.sg_plan(self.ctx, C.byref(b)) == 0, self.err()

    def sample(self):
        """(text of mate 1, text of mate 2, fragments) of the planned batch"""
        assert self.eng.sg_sample(self.ctx) == 0, self.err()
        b1, b2, nf = C.c_uint64(), C.c_uint64(), C.c_uint64()
        assert self.eng.sg_result(self.ctx, C.byref(b1), C.byref(b2), C.byref(nf)) == 0, self.err()
        t1, t2 = C.create_string_buffer(max(b1.value, 1)), C.create_string_buffer(max(b2.value, 1))
        assert self.eng.sg_fetch(self.ctx, t1, t2 if b2.value else None) == 0, self.err()
        return t1.raw[:b1.value], t2.raw[:b2.value], nf.value


def seg_sizes(n_active):
    return [1000 + 7 * a for a in range(n_active)]


def bits(values):
    return np.array(values, dtype=np.float64).view(np.uint64)


def same(a, b):
    """(a plain bool: megabytes of text are not diffed on a failure)"""
    return a == b


def assert_same_bits(got, want, what):
    want = bits(want)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} differ, first at {bad[0]}: {got[bad[0]]:#018x} != {want[bad[0]]:#018x}"


# ---- (a) sg_window_weights --------------------------------------------------------------------------------------------------
ROWS = WM.explicit_windows()
SEGS, ORDS = WM.explicit_ordinals(len(ROWS))


def model_weights(m, seed, rows=ROWS, segs=SEGS, ords=ORDS):
    return WM.weights_of(WM.chains(), [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], segs, ords, m, seed)


@pytest.mark.parametrize("full_tile_form", [0, 1])
@pytest.mark.parametrize("lg_cells", [1, 12, 20])
def test_window_weights_equal_the_model_bit_for_bit(eng, lg_cells, full_tile_form):
    """Window lengths 1 .. 2051 at the start offsets 0..15 of a 16-byte group (gc_kernel's 16-byte loads and the mask of its
    tail), windows of one letter, with one N first, last and in the middle, with an R, in the second chain; frag 16, 37 and
    1000, so that every form of the weight meets windows of exactly frag bases and shorter (and longer) ones."""
    with Ctx(eng) as c:
        for frag in (16, 37, 1000):
            m = WM.model(frag, lg_cells=lg_cells, full_tile_form=full_tile_form)
            want_w, want_gc = model_weights(m, WM.SEEDS[0])
            got_w, got_gc = c.window_weights(ROWS, SEGS, ORDS, m)
            assert got_gc == want_gc, [(i, ROWS[i], a, b) for i, (a, b) in enumerate(zip(got_gc, want_gc)) if a != b][:5]
            assert_same_bits(got_w, want_w, f"frag {frag}")
            assert {r[2] for r in ROWS} >= {frag, 1, 15} and {-1, 0, 100} <= set(want_gc)


def test_window_ending_on_the_last_byte_of_the_last_chain(eng):
    """gc_kernel loads 16 bytes at every 16th byte of a window, so the load of a window's tail reaches up to 15 bytes past
    the window: for a window that ends on the last chain's last byte, past the chains.  Settled by reading
    sg_api_haplotypes.cpp: chain_layout (used by sg_upload_haplotypes and sg_build_haplotypes alike) puts a guard of 256 bytes in front
    of every chain and behind the last one, rounds every chain up to 64 bytes and the whole buffer up to 1,024, and both
    routes fill the guards with N before the chains are copied in; the allocation is `total` bytes.  The load stays inside
    the allocation, and the kernel masks the bytes past the window off before it counts, so the guard's N do not count
    either: what this test checks, at every tail length 1..16 and for both chains' ends."""
    ch = WM.chains()
    rows = [(1, len(ch[1]) - n, n) for n in list(range(1, 18)) + [37, 1000, 2051]] + [(0, len(ch[0]) - n, n) for n in range(1, 18)]
    segs, ords = WM.explicit_ordinals(len(rows))
    m = WM.model(16, lg_cells=12)
    with Ctx(eng) as c:
        got_w, got_gc = c.window_weights(rows, segs, ords, m)
        want_w, want_gc = model_weights(m, WM.SEEDS[0], rows, segs, ords)
        assert got_gc == want_gc and -1 not in want_gc
        assert_same_bits(got_w, want_w, "windows at the chains' ends")


def test_seeds_and_contexts_address_the_draws(eng):
    """Two seeds and two ctx24 values: each pair gives the model's bits, different pairs give different bits, the same
    pair gives the same bits on a second call."""
    seen = {}
    for seed in WM.SEEDS:
        with Ctx(eng, seed=seed) as c:
            for ctx24 in WM.CTX24S:
                m = WM.model(16, lg_cells=12, ctx24=ctx24)
                got, _ = c.window_weights(ROWS, SEGS, ORDS, m)
                assert_same_bits(got, model_weights(m, seed)[0], f"seed {seed:#x} ctx24 {ctx24:#x}")
                seen[(seed, ctx24)] = got.copy()
            again, _ = c.window_weights(ROWS, SEGS, ORDS, WM.model(16, lg_cells=12, ctx24=WM.CTX24S[0]))
            assert (again == seen[(seed, WM.CTX24S[0])]).all()
    keys = list(seen)
    for i in range(len(keys)):
        for j in range(i):
            assert (seen[keys[i]] != seen[keys[j]]).sum() > len(ROWS) // 2, (keys[i], keys[j])


def test_window_weights_refusals(eng):
    ch = WM.chains()
    with Ctx(eng) as c:
        good = WM.model(16, lg_cells=12)
        assert "window runs past its chain" in c.window_weights([(0, 0, 16), (1, len(ch[1]) - 15, 16)], [0, 0], [0, 1], good, want=1)
        assert "window runs past its chain" in c.window_weights([(0, len(ch[0]), 1)], [0], [0], good, want=1)
        assert "chain out of range" in c.window_weights([(2, 0, 16)], [0], [0], good, want=1)
        for lg in (0, 21):
            bad = WM.Model(good.means, good.std, good.quantiles, lg, 16, 1, 0)
            assert "bad model" in c.window_weights([(0, 0, 16)], [0], [0], bad, want=1)
        bad = WM.Model(good.means, good.std, good.quantiles, 12, 0, 1, 0)
        assert "bad model" in c.window_weights([(0, 0, 16)], [0], [0], bad, want=1)
        c.window_weights([(0, 0, 16)], [0], [0], good)                      # and the context goes on working
    with Ctx(eng, upload=False) as c:
        assert "sg_upload_haplotypes first" in c.window_weights([(0, 0, 16)], [0], [0], WM.model(16, lg_cells=12), want=1)


def test_work_buffers_shared_by_calls_of_different_sizes(eng):
    """sg_window_weights and sg_gc_percent carve one arena of the context, sg_windows_build another, and both keep the
    size of the largest call: 8,193 windows, then 3, a build, 5, and 8,193 again on one context give, bit for bit, what
    each call gives on a context of its own.  Two chains of 331 and 257 bases (an N in the first), windows of 16 and 37
    bases at every start."""
    c0 = bytearray(WM._letters(331, 7).tobytes())
    c0[100] = ord("N")
    small = [bytes(c0), WM._letters(257, 8).tobytes()]

    def rows(n):
        return [(i % 2, (i * 7) % (len(small[i % 2]) - 37), (16, 37)[(i // 2) % 2]) for i in range(n)]

    m16, m37 = WM.model(16, lg_cells=14), WM.model(37)            # (tables of 2^14 and 2^12 cells)
    gens = [WM.Gen(0, 300, 0, 0), WM.Gen(5, 200, 1, 1), WM.Gen(9, 37, 0, 3)]
    calls = [lambda c: c.window_weights(rows(8193), *WM.explicit_ordinals(8193), m16),
             lambda c: c.gc_percent(rows(3)),
             lambda c: c.build(1, gens, 5, m16),
             lambda c: c.window_weights(rows(5), *WM.explicit_ordinals(5), m37),
             lambda c: c.gc_percent(rows(8193))]

    def plain(r):
        return [x.tolist() if isinstance(x, np.ndarray) else x for x in r] if isinstance(r, tuple) else r

    with Ctx(eng, chains=small) as c:
        shared = [plain(call(c)) for call in calls]
    for i, call in enumerate(calls):
        with Ctx(eng, chains=small) as c:
            assert plain(call(c)) == shared[i], f"call {i}"
    assert -1 in shared[4] and len(set(shared[4])) > 10 and shared[2][1] == 19 + 13 + 3 and any(shared[0][0])


# ---- (b) sg_windows_build ---------------------------------------------------------------------------------------------------
_BUILT = {}


def built(frag):
    """(gens, n_segs, note, tiling, weights, segment weights) of the model for the build of `frag`, computed once"""
    if frag not in _BUILT:
        gens, n_segs, note = WM.build_gens(frag, **WM.BUILD_ARGS[frag])
        _BUILT[frag] = (gens, n_segs, note) + WM.build(WM.chains(), gens, n_segs, WM.model(frag), WM.SEEDS[0])
    return _BUILT[frag]


@pytest.mark.parametrize("frag", [16, 37, 1000])
def test_windows_build_equals_the_model_bit_for_bit(eng, frag):
    """Segments of 1, 2, 63, 64, 65, 4095, 4096, 4097 and 8193 windows (frag 1000: up to 4097) of one, two and three
    generators of 1, frag - 1, frag, frag + 1 and k * frag bases; ordinals that no generator names, in the middle and at the
    end, weigh exactly 0.0.  The per-window weights stay on the device: sg_window_weights on the model's windows and
    ordinals of the same tiling gives the model's weights, and their left-to-right sum is seg_weight_out."""
    gens, n_segs, note, t, w, seg_w = built(frag)
    with Ctx(eng) as c:
        got, n = c.build(1, gens, n_segs, WM.model(frag))
        assert n == t.n
        assert_same_bits(got, seg_w, f"segment weights, frag {frag}")
        assert got[3] == 0 and got[n_segs - 1] == 0 and got[note["all_n"]] == 0          # +0.0
        per_window, _ = c.window_weights(list(zip(t.chain, t.start, t.len)), t.seg, t.ord, WM.model(frag))
        assert_same_bits(per_window, w, f"window weights of the tiling, frag {frag}")


def test_windows_build_with_2000_generators(eng):
    gens, n_segs = WM.many_gens()
    m = WM.model(16, lg_cells=12)
    t, w, seg_w = WM.build(WM.chains(), gens, n_segs, m, WM.SEEDS[1])
    with Ctx(eng, seed=WM.SEEDS[1]) as c:
        got, n = c.build(9, gens, n_segs, m)
        assert n == t.n and len(gens) == 2000
        assert_same_bits(got, seg_w, "segment weights of 2,000 generators")


def test_windows_build_refusals(eng):
    ch = WM.chains()
    G = WM.Gen
    with Ctx(eng) as c:
        m = WM.model(16)
        for bad in ([G(0, 16, 2, 0)], [G(0, 0, 0, 0)], [G(len(ch[1]) - 15, 16, 1, 0)], [G(0, 16, 0, 0), G(len(ch[0]), 1, 0, 1)]):
            assert "does not lie inside its chain" in c.build(1, bad, 2, m, want=1)
        assert "generators must be ordered by segment" in c.build(1, [G(0, 16, 0, 1), G(16, 16, 0, 0)], 2, m, want=1)
        assert "generators must be ordered by segment" in c.build(1, [G(0, 16, 0, 2)], 2, m, want=1)        # seg >= n_segs
        for lg, frag in ((0, 16), (21, 16), (12, 0)):
            assert "bad model" in c.build(1, [G(0, 16, 0, 0)], 1, WM.Model(m.means, m.std, m.quantiles, lg, frag, 1, 0), want=1)
    with Ctx(eng, upload=False) as c:
        assert "sg_upload_haplotypes" in c.build(1, [G(0, 16, 0, 0)], 1, WM.model(16), want=1)


# ---- (c) sg_plan_windows ----------------------------------------------------------------------------------------------------
def plan_case(segs, rule, paired, frag=16):
    gens, n_segs, note, t, w, seg_w = built(frag)
    ag = WM.active_gens(gens, t, segs)
    active = WM.active_rows(t, seg_w, segs, rule)
    return ag, active, WM.plan(w, ag, active, frag, paired)


@pytest.mark.parametrize("paired", [0, 1], ids=["single", "paired"])
def test_plan_windows_equals_the_model(eng, paired):
    """The 1st, 3rd, 4th and last built segment (first_window skips the stored segments between them; the last one holds an
    N in every window: weight 0.0, every read is the remainder of its first window) with 1 read, fewer reads than
    windows, as many, and thousands; then every built segment at once -- 200 of 1..130 windows, so that waves of 64
    windows hold one segment, several, or begin inside one, and the long ones of up to 8,193."""
    gens, n_segs, note, t, w, seg_w = built(16)
    with Ctx(eng, profile=True) as c:
        got, n = c.build(1, gens, n_segs, WM.model(16))
        assert_same_bits(got, seg_w, "segment weights")
        for rule in ("one", "below", "equal", "thousands"):
            ag, active, p = plan_case(WM.subset_segments(t), rule, paired)
            assert c.plan_windows(1, ag, active, 16, paired) == (p.slots, len(p.rows)), rule
            assert p.rows[p.seg_first[3]][4] == active[3][0] and active[3][1] == 0.0           # the all-N segment
        ag, active, p = plan_case(WM.all_segments(t), "mixed", paired)
        assert len(active) >= 200
        slots, n = c.plan_windows(1, ag, active, 16, paired)
        assert n == len(p.rows)
        assert slots == p.slots, [(a, x, y) for a, (x, y) in enumerate(zip(slots, p.slots)) if x != y][:8]


def test_two_stores_alive_at_once(eng):
    """Store 1 (the frag-16 build) and store 2 (2,000 generators), then store 2 built again from other generators: plans
    from store 1, then store 2, then store 1 again equal the model before and after (the stores' sizes differ, and each
    plan is checked against its own).  sg_windows_drop ends both."""
    gens, n_segs, note, t, w, seg_w = built(16)
    m2 = WM.model(16, lg_cells=12, ctx24=WM.CTX24S[1])
    with Ctx(eng, profile=True) as c:
        c.build(1, gens, n_segs, WM.model(16))
        for n_gens in (2000, 700):
            g2, s2 = WM.many_gens(n_gens)
            t2, w2, sw2 = WM.build(WM.chains(), g2, s2, m2, WM.SEEDS[0])
            assert_same_bits(c.build(2, g2, s2, m2)[0], sw2, f"store 2 of {n_gens} generators")
            segs2 = WM.all_segments(t2)[5:200:3]
            ag2 = WM.active_gens(g2, t2, segs2)
            act2 = WM.active_rows(t2, sw2, segs2, "thousands")
            p2 = WM.plan(w2, ag2, act2, 16, 1)
            ag1, act1, p1 = plan_case(WM.subset_segments(t), "thousands", 1)
            for store, a_g, act, p in ((1, ag1, act1, p1), (2, ag2, act2, p2), (1, ag1, act1, p1)):
                assert c.plan_windows(store, a_g, act, 16, 1) == (p.slots, len(p.rows)), store
                c.plan_range(0, len(act))
                dev = c.sample()                                  # the rows, through the text they cause
                c.plan_host(p.rows, p.seg_first, len(act), 1)
                assert dev[2] > 0 and same(dev, c.sample()), store
            ag, active, p = plan_case(WM.subset_segments(t), "thousands", 0)
            assert c.plan_windows(1, ag, active, 16, 0) == (p.slots, len(p.rows))
            assert t.n != t2.n
        eng.sg_windows_drop(c.ctx)
        assert "no window weights under this store id" in c.plan_windows(1, ag, active, 16, 0, want=1)
        assert "no window weights under this store id" in c.plan_windows(2, ag2, act2, 16, 1, want=1)


def test_plan_refusals(eng):
    gens, n_segs, note, t, w, seg_w = built(1000)
    G = WM.Gen
    with Ctx(eng, profile=True) as c:
        assert "call sg_plan_windows first" in c.plan_range(0, 1, want=1)
        c.build(1, gens, n_segs, WM.model(1000))
        segs = [0, 2, 4]
        ag = WM.active_gens(gens, t, segs)
        active = WM.active_rows(t, seg_w, segs, "thousands")
        assert "no window weights under this store id" in c.plan_windows(5, ag, active, 1000, 1, want=1)
        past = [G(g.hap_base, g.hap_len, g.chain, g.seg, g.first_window) for g in ag]
        past[-1].first_window = t.n - 63                                         # 64 windows from there: one past the store
        assert "generator 3 points past the stored weights" in c.plan_windows(1, past, active, 1000, 1, want=1)
        assert "generators must be ordered by segment" in c.plan_windows(1, [ag[3], ag[0]], active, 1000, 1, want=1)
        assert "generators must be ordered by segment" in c.plan_windows(1, ag, active[:2], 1000, 1, want=1)     # seg >= n_active
        assert "does not lie inside its chain" in c.plan_windows(1, [G(0, 16, 7, 0)], active[:1], 1000, 1, want=1)
        assert "active segment without windows" in c.plan_windows(1, [ag[0], ag[3]], active, 1000, 1, want=1)   # none for index 1
        assert "seg_size 0" in c.plan_windows(1, ag, active, 1000, 1, seg_size=[5, 0, 5], want=1)
        assert "bad name_prefix" in c.plan_windows(1, ag, active, 1000, 1, prefix=b"", want=1)
        assert "bad name_prefix" in c.plan_windows(1, ag, active, 1000, 1, prefix=b"@" * 991, want=1)
        assert "batch_id must fit 16 bits" in c.plan_windows(1, ag, active, 1000, 1, batch_id=0x10000, want=1)
        p = WM.plan(w, ag, active, 1000, 1)
        assert c.plan_windows(1, ag, active, 1000, 1, prefix=b"@" * 990, batch_id=0xFFFF) == (p.slots, len(p.rows))
        for a0, a1 in ((1, 1), (2, 1), (0, 4), (3, 4)):
            assert "empty or out-of-range run of segments" in c.plan_range(a0, a1, want=1)
        c.plan_range(0, 3)
        eng.sg_windows_drop(c.ctx)
        assert "no window weights under this store id" in c.plan_windows(1, ag, active, 1000, 1, want=1)
        assert "no window weights under this store id" in c.plan_windows(0, ag, active, 1000, 1, want=1)
    with Ctx(eng) as c:
        c.build(1, gens, n_segs, WM.model(1000))
        assert "sg_load_profile first" in c.plan_windows(1, [], [], 1000, 1, want=1)


# ---- (d) the rows, through what they cause ----------------------------------------------------------------------------------
@pytest.mark.parametrize("frag,paired", [(16, 1), (37, 0), (37, 1)], ids=["frag16_paired", "frag37_single", "frag37_paired"])
def test_device_rows_sample_the_text_of_the_models_rows(eng, frag, paired):
    """Every built segment of a build is active (the wave-straddling ones and those of more than 4,096 windows): the batch
    of sg_plan_windows + sg_plan_range(0, n_active) gives, for both mates, the text of sg_plan on the model's rows; and
    the runs [0, k), [k, m), [m, n_active), sampled one after the other, concatenate to that text -- at two cuts, one run
    a single segment (of 8,193 windows), runs beginning at segments whose first window got a remainder.  (A single-end
    fragment is its window, so single-end reads of 36 bases come from the build of 37-base windows only; there the
    generators' shorter last windows give no read, which is part of the text too.)"""
    gens, n_segs, note, t, w, seg_w = built(frag)
    ag, active, p = plan_case(WM.all_segments(t), "mixed", paired, frag)
    n_act = len(active)
    with Ctx(eng, profile=True) as c:
        c.plan_host(p.rows, p.seg_first, n_act, paired)
        host = c.sample()
        print("fragments", host[2], "of", p.slot_first[-1], "planned; text bytes", len(host[0]), len(host[1]))
        assert p.slot_first[-1] // 2 < host[2] <= p.slot_first[-1] < 300_000
        assert len(host[0]) > 50 * host[2] and (len(host[1]) > 50 * host[2]) == bool(paired)
        c.build(1, gens, n_segs, WM.model(frag))
        assert c.plan_windows(1, ag, active, frag, paired) == (p.slots, len(p.rows))
        c.plan_range(0, n_act)
        assert same(c.sample(), host), "the device-planned batch gives another text than the model's rows"
        for k, m in WM.CUTS[frag]:
            parts = []
            for a0, a1 in ((0, k), (k, m), (m, n_act)):
                c.plan_range(a0, a1)
                parts.append(c.sample())
            assert sum(x[2] for x in parts) == host[2]
            assert same(b"".join(x[0] for x in parts), host[0]) and same(b"".join(x[1] for x in parts), host[1]), (k, m)


def test_device_rows_give_the_truth_rows_of_the_models_rows(eng):
    """sg_truth_reads (where every read came from) reads the rows too, but is refused for chains uploaded as bytes: it wants
    the piece map of chains assembled on the device.  So here the same chains are assembled by sg_build_haplotypes from a
    reference image that holds them as two contigs, one piece each; then the truth rows of every slot and both mates of
    the device-planned batch are those of the host-planned batch of the model's rows, and so is the text."""
    import test_gpu_haplotypes as H
    from simuscop_amd import SgContig, SgHapPiece, SgTruthRead
    ch = WM.chains()
    gens, n_segs, note, t, w, seg_w = built(16)
    ag, active, p = plan_case(WM.all_segments(t), "mixed", 1)
    n_act, width = len(active), 100_000
    image, rows = H._fasta_image([(b"c0", ch[0]), (b"c1", ch[1])], width)
    with Ctx(eng, profile=True, upload=False) as c:
        H._upload(eng, c.ctx, image)
        tab = (SgContig * 2)(*[SgContig(first, len(seq), width, width + 1) for _, first, seq in rows])
        assert eng.sg_reference_commit(c.ctx, tab, 2) == 0, c.err()
        pieces = (SgHapPiece * 2)(SgHapPiece(0, 0, len(ch[0]), 0, 0, 0), SgHapPiece(0, 0, len(ch[1]), 1, 1, 0))
        lens = (C.c_uint64 * 2)(len(ch[0]), len(ch[1]))
        assert eng.sg_build_haplotypes(c.ctx, 2, lens, pieces, 2, None, 0, None, 0) == 0, c.err()
        assert eng.sg_truth_map(c.ctx, pieces, b"\1\1", 2, (C.c_int32 * 2)(0, 1), 2) == 0, c.err()

        n_slots, words = p.slot_first[-1], C.sizeof(SgTruthRead) // 4

        def truth():
            text = c.sample()
            out = []
            for mate in (0, 1):
                arr = (SgTruthRead * n_slots)()
                assert eng.sg_truth_reads(c.ctx, mate, 0, n_slots, arr) == 0, c.err()
                out.append(np.frombuffer(bytes(arr), dtype=np.uint32).reshape(n_slots, words))
            return text, out

        c.plan_host(p.rows, p.seg_first, n_act, 1)
        host_text, host_rows = truth()
        c.build(1, gens, n_segs, WM.model(16))
        assert c.plan_windows(1, ag, active, 16, 1) == (p.slots, len(p.rows))
        c.plan_range(0, n_act)
        dev_text, dev_rows = truth()
        assert same(dev_text, host_text)
        for mate in (0, 1):
            live = host_rows[mate][:, 0] != 0                                      # (a slot without a read: only `live` is defined)
            assert (dev_rows[mate][:, 0] == host_rows[mate][:, 0]).all() and live.sum() > n_slots // 2
            assert (dev_rows[mate][live] == host_rows[mate][live]).all()
