"""The emit side of a sampling pass (edge_kernel, fragment_kernel, header_kernel, emit_fast_kernel, emit_kernel /
emit_slow_kernel) read by read against tests/read_model.py, on templates the test places by hand.

Per case: the engine context of a Session (so that the profile file goes through host/profile.cpp and
sg_load_prepared_profile), chains the test authors -- ingested as a reference image and assembled one piece per chain, so
that a piece map exists -- and one sg_plan of hand-made sg_window rows; then sg_sample, sg_result, sg_fetch.  The text is
split into records and every record is compared with the model's (tests/test_read_model_cpu.py holds the model to the
whole oracle): names, bases, qualities; no record for a dead slot; byte totals; and the rows of sg_truth_reads
(live, chain, tmpl_off, reverse, read_len, n_events, the events, inside) against the model's placement and indel walk.
A failure lists up to 20 differing reads with slot, mate, the first differing line and cycle, where the template lies
relative to its chain's start and end, the model's events and the emit path.

Paired cases use windows of length 1 and the one-column insert profile (read_model.one_column_profile): a window's spos
is the fragment's start, spos + insertSize + 1 - L the start of mate 2's template.  Every case asserts the kernel it ran.

SG_SLOWQ_CAP, SG_CLEAN_CAP and SG_NO_CLEAN_STEPS are read with getenv once per pass (launch_text in sg_api.cpp, emit_path
in sg_kernels.hip), so test_chain_edges_with_small_queues sets them with monkeypatch for one more pass each."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import read_model as RM
import simuscop_amd
import test_gpu_haplotypes as H
from profile_shapes import Shape
from simuscop_amd import SgBatch, SgContig, SgEmitPathInfo, SgHapPiece, SgTruthRead, SgWindow

pytestmark = pytest.mark.gpu

WINDOW = np.dtype([("hap_base", "<u8"), ("chain", "<u4"), ("spos", "<u4"), ("len", "<u4"), ("n_reads", "<i4"), ("seg", "<u4"), ("slot_base", "<u4")])
TRUTH = np.dtype([("live", "<u4"), ("chain", "<u4"), ("reverse", "<u4"), ("read_len", "<u4"), ("tmpl_off", "<u8"), ("n_events", "<u4"),
                  ("inside", "<u4"), ("events", "<u4", (32,))])
assert WINDOW.itemsize == C.sizeof(SgWindow) and TRUTH.itemsize == C.sizeof(SgTruthRead)
STRAIGHT, K3_LDS, ANY_LDS, GLOBAL = 1, 2, 3, 4     # SG_EMIT_* (include/simuscop_amd.h)
SEED, BATCH_ID, PREFIX = 0x5EED0123456789AB, 0x2B1, b"@placed#7#"
L0, INSERT0 = 60, 150                               # the shared profiles: reads of 60 bases, fragments of 151
K3 = Shape(3, 30, read_length=L0, indel_scale=4.0)  # straight-line kernel
K2 = Shape(2, 30, read_length=L0, indel_scale=4.0)  # generic kernel


def letters(n, seed):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Run:
    def __init__(self, text, fragments, path, n_slots, queued, requeued):
        self.text, self.fragments, self.path, self.n_slots, self.queued, self.requeued = text, fragments, path, n_slots, queued, requeued

    @property
    def path_text(self):
        p = self.path
        return f"main_kernel {p.main_kernel} slow_rows_lds {p.slow_rows_lds} lds_bytes {p.lds_bytes} clean_cap {p.clean_cap}"


class Rig:
    """The engine context of a Session on the one-column profile of `shape`, and the model of the same file."""

    def __init__(self, oracle_lib, wd, shape, paired=True, insert=INSERT0):
        os.makedirs(wd, exist_ok=True)
        prof = RM.one_column_profile(os.path.join(wd, shape.tag + ".profile"), shape)
        fa, cfg = os.path.join(wd, "ref.fa"), os.path.join(wd, "config.txt")
        cases._fasta_of(fa, [(b"chrT", letters(3000, 1))])
        cases._config(cfg, ref=fa, profile=prof, name="t", output=os.path.join(wd, "out"), layout="PE" if paired else "SE", threads=1,
                      verbose=0, coverage=1, insertSize=insert)
        self.paired, self.chains, self.profile = paired, None, prof
        self.model = RM.ReadModel(oracle_lib, prof, paired, insert, SEED, BATCH_ID, PREFIX)
        assert self.model.L == shape.read_length and (not paired or (self.model.n_isize == 1 and self.model.isz == insert + 1 and self.model.has_sub2))
        self.sess = simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=SEED, truth_bam=1)
        self.eng, self.ctx = self.sess.eng, self.sess.ctx
        self.ok(self.eng.sg_set_seed(self.ctx, SEED))

    def close(self):
        self.model.close()
        self.sess.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def ok(self, rc):
        assert rc == 0, self.eng.sg_last_error(self.ctx).decode()

    def set_chains(self, chains):
        """The chains as contigs of a reference image, one piece each, with the piece map."""
        eng, ctx, n, width = self.eng, self.ctx, len(chains), 100_000
        image, rows = H._fasta_image([(b"c%d" % i, c) for i, c in enumerate(chains)], width)
        H._upload(eng, ctx, image)
        tab = (SgContig * n)(*[SgContig(first, len(seq), width, width + 1) for _, first, seq in rows])
        self.ok(eng.sg_reference_commit(ctx, tab, n))
        pieces = (SgHapPiece * n)(*[SgHapPiece(0, 0, len(c), i, i, 0) for i, c in enumerate(chains)])
        lens = (C.c_uint64 * n)(*[len(c) for c in chains])
        self.ok(eng.sg_build_haplotypes(ctx, n, lens, pieces, n, None, 0, None, 0))
        self.ok(eng.sg_truth_map(ctx, pieces, b"\1" * n, n, (C.c_int32 * n)(*range(n)), n))
        self.chains = chains

    def run(self, windows, seg_sizes, first_window=0, first_slot=0):
        eng, ctx = self.eng, self.ctx
        w = np.array(windows, dtype=WINDOW)
        n_segs = len(seg_sizes)
        ss = np.array(seg_sizes, dtype=np.uint32)
        sf = np.searchsorted(w["seg"], np.arange(n_segs + 1)).astype(np.uint32)
        assert (np.diff(w["seg"].astype(np.int64)) >= 0).all() and sf[-1] == len(w)
        b = SgBatch(BATCH_ID, 1 if self.paired else 0, PREFIX, ptr(w, SgWindow), len(w), ptr(ss, C.c_uint32), ptr(sf, C.c_uint32), n_segs,
                    first_window, first_slot)
        self.ok(eng.sg_plan(ctx, C.byref(b)))
        self.ok(eng.sg_sample(ctx))
        b1, b2, nf = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.ok(eng.sg_result(ctx, C.byref(b1), C.byref(b2), C.byref(nf)))
        t1, t2 = C.create_string_buffer(max(b1.value, 1)), C.create_string_buffer(max(b2.value, 1))
        self.ok(eng.sg_fetch(ctx, t1, t2 if self.paired else None))
        path, q, r = SgEmitPathInfo(), C.c_uint64(), C.c_int()
        self.ok(eng.sg_emit_path(ctx, C.byref(path)))
        self.ok(eng.sg_emit_info(ctx, C.byref(q), C.byref(r)))
        n_slots = int(w["slot_base"][-1]) + planned_of(int(w["n_reads"][-1]), self.paired) if len(w) else 0
        assert self.paired or b2.value == 0
        return Run((t1.raw[:b1.value], t2.raw[:b2.value]), nf.value, path, n_slots, q.value, bool(r.value))

    def truth(self, mate, n_slots):
        arr = (SgTruthRead * max(n_slots, 1))()
        self.ok(self.eng.sg_truth_reads(self.ctx, mate, 0, n_slots, arr))
        return np.frombuffer(bytes(arr), dtype=TRUTH)[:n_slots]


def planned_of(n, paired):
    return 0 if n <= 0 else ((n + 1) // 2 if paired else n)


def table(rows, paired):
    """sg_window rows from (hap_base, chain, spos, len, n_reads, seg), in the order given: slot_base filled in."""
    out, base = [], 0
    for hap_base, chain, spos, wlen, n, seg in rows:
        out.append((hap_base, chain, spos, wlen, n, seg, base))
        base += planned_of(n, paired)
    return out


class Read:
    __slots__ = ("slot", "mate", "s", "off", "reverse", "ev", "reset", "name", "length", "rec", "seg_size")


def expect(model, chains, windows, seg_sizes, first_window=0, first_slot=0, per_read=None):
    """(plan, reads per mate): what the model owes for the batch.  per_read: the local slots whose bases and qualities are
    computed (None: all); every read has its name, its events and its record length."""
    plan = model.plan(windows, [len(c) for c in chains], first_window)
    reads = {m: [] for m in ((0, 1) if model.paired else (0,))}
    for k, s in enumerate(plan):
        if s is None:
            continue
        for m in reads:
            r = Read()
            r.slot, r.mate, r.s = k, m, s
            r.off, r.reverse = model.placement(s, m)
            r.ev, r.reset = model.events(m, first_slot + k)
            r.name = model.name(s.pos, seg_sizes[s.seg], s.fragcount, m)
            r.length = len(r.name) + 5 + 2 * (model.L + sum(n if kind == "I" else -n for _, kind, n in r.ev))
            r.rec, r.seg_size = None, seg_sizes[s.seg]
            if per_read is None or k in per_read:
                r.rec = model.slot_record(chains, s, m, first_slot + k, seg_sizes[s.seg])
                assert len(r.rec) == r.length and r.rec.startswith(r.name + b"\n")
            reads[m].append(r)
    return plan, reads


def classes_of(reads):
    out = {}
    for rs in reads.values():
        for r in rs:
            c = "reset" if r.reset else RM.ReadModel.read_class(r.ev)
            out[c] = out.get(c, 0) + 1
    return out


def differences(model, chains, plan, reads, run, first_slot=0):
    """Every read of the run's text that is not the model's, as text lines."""
    bad = []
    for m, want in reads.items():
        got = RM.split_records(run.text[m])
        if len(got) != len(want):
            bad.append(f"mate {m + 1}: {len(got)} records, the model has {len(want)} live slots")
            continue
        for g, r in zip(got, want):
            if (g == r.rec) if r.rec is not None else (len(g) == r.length and g.startswith(r.name + b"\n")):
                continue
            ref = r.rec if r.rec is not None else model.slot_record(chains, r.s, m, first_slot + r.slot, r.seg_size)
            line, cyc = RM.first_cycle(g, ref)
            clen = len(chains[r.s.chain])
            bad.append(f"slot {first_slot + r.slot} mate {m + 1}: first difference in line {line} ({('name', 'bases', '+', 'qualities')[min(line, 3)]}) "
                       f"at cycle {cyc}; template {r.off} from the start of chain {r.s.chain}, {clen - r.off - model.L} before its end "
                       f"(chain of {clen} = {clen % 64} mod 64), reverse {int(r.reverse)}, fragment of {r.s.flen}; n_events {len(r.ev)} "
                       f"{r.ev[:4]} reset {int(r.reset)}; {run.path_text}\n  got  {g!r}\n  want {ref!r}")
        if sum(r.length for r in want) != len(run.text[m]):
            bad.append(f"mate {m + 1}: text of {len(run.text[m])} bytes, the records' lengths sum to {sum(r.length for r in want)}")
    if run.fragments != sum(s is not None for s in plan):
        bad.append(f"sg_result reports {run.fragments} fragments, the plan has {sum(s is not None for s in plan)}")
    return bad


def truth_differences(rig, plan, reads):
    """sg_truth_reads of the pass against the model's placement and events."""
    bad, n = [], len(plan)
    live = np.array([s is not None for s in plan], dtype=bool)
    for m, want in reads.items():
        rows = rig.truth(m, n)
        if ((rows["live"] != 0) != live).any():
            bad.append(f"mate {m + 1}: live differs at slots {np.flatnonzero((rows['live'] != 0) != live)[:10].tolist()}")
            continue
        for r in want:
            t = rows[r.slot]
            ev = [j | (k << 16) | ((kind == "D") << 31) for j, kind, k in r.ev]
            got = (int(t["chain"]), int(t["tmpl_off"]), int(t["reverse"]), int(t["read_len"]), int(t["n_events"]), int(t["inside"]),
                   t["events"][:min(len(ev), 32)].tolist())
            exp = (r.s.chain, r.off, int(r.reverse), (r.length - len(r.name) - 5) // 2, len(ev), 1, ev[:32])
            if got != exp:
                bad.append(f"slot {r.slot} mate {m + 1}: truth row (chain, tmpl_off, reverse, read_len, n_events, inside, events) {got}, the model {exp}")
    return bad


def check(rig, windows, seg_sizes, main_kernel, first_window=0, first_slot=0, per_read=None, expected=None, truth=True):
    """One pass on the rig's chains against the model; returns (run, plan, reads)."""
    plan, reads = expected or expect(rig.model, rig.chains, windows, seg_sizes, first_window, first_slot, per_read)
    run = rig.run(windows, seg_sizes, first_window, first_slot)
    assert run.path.main_kernel == main_kernel, run.path_text
    assert run.n_slots == len(plan)
    bad = differences(rig.model, rig.chains, plan, reads, run, first_slot)
    if truth:
        bad += truth_differences(rig, plan, reads)
    assert not bad, f"{len(bad)} differences, the first {min(len(bad), 20)}:\n" + "\n".join(bad[:20])
    return run, plan, reads


@pytest.fixture(scope="module")
def rigs(oracle_lib, tmp_path_factory):
    """The shared contexts: (k-mer, paired) -> Rig on the 60-base profiles, opened on first use."""
    made = {}

    def get(kmer, paired=True):
        if (kmer, paired) not in made:
            made[(kmer, paired)] = Rig(oracle_lib, str(tmp_path_factory.mktemp(f"k{kmer}_{int(paired)}")), K3 if kmer == 3 else K2, paired)
        return made[(kmer, paired)]

    yield get
    for r in made.values():
        r.close()


KERNELS = [(3, STRAIGHT), (2, ANY_LDS)]
KERNEL_IDS = ["straight_line_k3", "generic_k2"]


# ---- chain edges ------------------------------------------------------------------------------------------------------------
EDGE_CHAINS = [letters(n, 100 + n) for n in (960, 1025, 1087)]          # clen % 64 = 0, 1, 63
assert [len(c) % 64 for c in EDGE_CHAINS] == [0, 1, 63]


def edge_windows(L, isz, pairs=8):
    """Per chain: fragment starts at 0..16 and 56..72; fragment ends 0..40 before the chain's end (mate 2's template ends
    on the last base at 0); fragments clipped by the end to isz - 1, - 2, - 3, ... L + 1, L (flen == L: both mates read one
    template) and to L - 1, L - 2, 1 (dead).  Two segments per chain, the second with hap_base 512, so that the name's
    position is not the chain offset; segment sizes that the positions exceed."""
    rows = []
    for c, chain in enumerate(EDGE_CHAINS):
        clen = len(chain)
        starts = list(range(0, 17)) + list(range(56, 73)) + [clen - isz - d for d in range(40, -1, -1)]
        cuts = sorted({1, 2, 3, 30, 31, 32, 33, isz - L - 1, isz - L} | set(range(60, isz - L, 9)))
        starts += [clen - isz + k for k in cuts] + [clen - L + 1, clen - L + 2, clen - 1]
        for seg, lo, hi, base in ((2 * c, 0, 512, 0), (2 * c + 1, 512, clen, 512)):
            rows += [(base, c, s - base, 1, 2 * pairs, seg) for s in starts if lo <= s < hi]
    return table(rows, True), [300 + 7 * s for s in range(2 * len(EDGE_CHAINS))]


_EDGE = {}


def edge_case(rig, kmer):
    """(windows, segment sizes, (plan, reads)) of the chain-edge case, the model's side computed once per k-mer"""
    if kmer not in _EDGE:
        windows, seg_sizes = edge_windows(L0, INSERT0 + 1)
        _EDGE[kmer] = (windows, seg_sizes, expect(rig.model, EDGE_CHAINS, windows, seg_sizes))
    return _EDGE[kmer]


@pytest.mark.parametrize("kmer,main", KERNELS, ids=KERNEL_IDS)
def test_chain_edges(rigs, kmer, main):
    rig = rigs(kmer)
    rig.set_chains(EDGE_CHAINS)
    windows, seg_sizes, expected = edge_case(rig, kmer)
    run, plan, reads = check(rig, windows, seg_sizes, main, expected=expected)
    dead = sum(s is None for s in plan)
    assert dead == 3 * 3 * 8 and len(plan) - dead > 2000
    assert {s.flen for s in plan if s} >= {L0, L0 + 1, INSERT0, INSERT0 + 1}
    ends = {(s.chain, len(EDGE_CHAINS[s.chain]) - s.foff - s.flen) for s in plan if s}
    assert all((c, 0) in ends and (c, 40) in ends for c in range(3))
    cl = classes_of(reads)
    print("read classes", cl, "queued items", run.queued)
    assert min(cl.get(k, 0) for k in ("none", "ins", "del", "many")) >= 10, cl


@pytest.mark.parametrize("env", [{"SG_SLOWQ_CAP": "1"}, {"SG_CLEAN_CAP": "64"}, {"SG_NO_CLEAN_STEPS": "1"}], ids=lambda e: "_".join(e))
def test_chain_edges_with_small_queues(rigs, monkeypatch, env):
    """The chain-edge case on the straight-line kernel with a slow-item queue of one entry (the pass is emitted again by the
    generic kernel: requeued), with the smallest clean list and with none."""
    rig = rigs(3)
    rig.set_chains(EDGE_CHAINS)
    windows, seg_sizes, expected = edge_case(rig, 3)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    run, _, _ = check(rig, windows, seg_sizes, STRAIGHT, expected=expected)
    if "SG_SLOWQ_CAP" in env:
        assert run.requeued
    else:
        assert not run.requeued and run.path.clean_cap == (64 if "SG_CLEAN_CAP" in env else 0), run.path_text


def test_the_comparison_reports_wrong_reads(rigs, oracle_lib):
    """The harness itself, on the chain-edge pass.  Against a model with batch_id + 1 (the same names and placement, other
    draws) nearly every read is reported, each line with slot, mate, cycle, the template's place, the events and the emit
    path; against the plan of windows moved by one base every live read's truth row is."""
    rig = rigs(3)
    rig.set_chains(EDGE_CHAINS)
    windows, seg_sizes, (plan, reads) = edge_case(rig, 3)
    run = rig.run(windows, seg_sizes)
    n_reads = sum(len(v) for v in reads.values())
    with RM.ReadModel(oracle_lib, rig.profile, True, INSERT0, SEED, BATCH_ID + 1, PREFIX) as wrong:
        bad = differences(wrong, EDGE_CHAINS, *expect(wrong, EDGE_CHAINS, windows, seg_sizes), run)
    assert len(bad) > 0.99 * n_reads, (len(bad), n_reads)
    for word in ("slot ", " mate ", "at cycle ", "from the start of chain ", "before its end", "n_events ", "main_kernel 1", "got ", "want "):
        assert word in bad[0], (word, bad[0])
    def move(hb, c, sp):          # dead windows stay; (mate 2 of a fragment clipped by the end keeps its template)
        return sp if len(EDGE_CHAINS[c]) - hb - sp < L0 else (sp - 1 if sp else 1)

    moved = [(hb, c, move(hb, c, sp), ln, n, seg, sb) for hb, c, sp, ln, n, seg, sb in windows]
    plan2, reads2 = expect(rig.model, EDGE_CHAINS, moved, seg_sizes)
    assert [s is None for s in plan2] == [s is None for s in plan]
    assert len(truth_differences(rig, plan2, reads2)) > 0.85 * n_reads


def test_sharded_chain_edges(rigs):
    """The chain-edge batch as two shards cut at a segment boundary whose slot is no multiple of 63: first_window and
    first_slot on the second; each part is the model at its global slots, and the parts concatenate to the unsharded text."""
    rig = rigs(3)
    rig.set_chains(EDGE_CHAINS)
    windows, seg_sizes, expected = edge_case(rig, 3)
    whole = rig.run(windows, seg_sizes)
    cut_seg = 3
    w0 = [w for w in windows if w[5] < cut_seg]
    cut_slot = windows[len(w0)][6]
    assert cut_slot % 63 and cut_slot % 64 and 0 < len(w0) < len(windows)
    w1 = [(hb, c, sp, ln, n, seg - cut_seg, sb - cut_slot) for hb, c, sp, ln, n, seg, sb in windows[len(w0):]]
    a, _, _ = check(rig, w0, seg_sizes[:cut_seg], STRAIGHT)
    b, _, _ = check(rig, w1, seg_sizes[cut_seg:], STRAIGHT, first_window=len(w0), first_slot=cut_slot)
    assert a.text[0] + b.text[0] == whole.text[0] and a.text[1] + b.text[1] == whole.text[1]
    assert a.fragments + b.fragments == whole.fragments


# ---- one non-ACGT base --------------------------------------------------------------------------------------------------------
def n_chains():
    """Six chains of 1,400 bases, each with one non-ACGT base: N or R at p = 640, 671, 703 (p % 64 = 0, 31, 63)."""
    out = []
    for i, (p, ch) in enumerate((p, ch) for ch in b"NR" for p in (640, 671, 703)):
        c = bytearray(letters(1400, 200 + i))
        c[p] = ch
        out.append((p, bytes(c)))
    return out


@pytest.mark.parametrize("kmer,main", KERNELS, ids=KERNEL_IDS)
def test_one_unknown_base_pe(rigs, kmer, main):
    """Forward templates (mate 1) starting at p - L - 30 .. p + 10 and reverse templates (mate 2) over the same range: the
    base inside the template at every cycle, in the slack behind it only, and 1 to 10 bases in front of its start."""
    rig = rigs(kmer)
    chains = n_chains()
    rig.set_chains([c for _, c in chains])
    isz, rows = INSERT0 + 1, []
    for c, (p, _) in enumerate(chains):
        assert p % 64 in (0, 31, 63)
        for t in range(p - L0 - 30, p + 11):
            rows.append((0, c, t, 1, 4, c))                      # mate 1's template starts at t
            rows.append((0, c, t - (isz - L0), 1, 4, c))         # mate 2's template starts at t
    run, plan, reads = check(rig, table(rows, True), [5000] * len(chains), main)
    assert len(plan) == 6 * 2 * 101 * 2 and all(plan)
    inside = sum(b"N" in r.rec.split(b"\n")[1] for m in reads for r in reads[m])
    print("reads with an N", inside, "queued items", run.queued)
    assert inside > 1000


@pytest.mark.parametrize("kmer,main", KERNELS, ids=KERNEL_IDS)
def test_one_unknown_base_se(rigs, kmer, main):
    """Single-end over the same chains: windows of L starts and fragments of L bases, so both strands read the template
    at the drawn start; the starts cover p - 2 L - 30 .. p + 10 + L."""
    rig = rigs(kmer, paired=False)
    chains = n_chains()
    rig.set_chains([c for _, c in chains])
    rows = [(0, c, t, L0, 12, c) for c, (p, _) in enumerate(chains) for t in range(p - 2 * L0 - 30, p + 11, 7)]
    run, plan, reads = check(rig, table(rows, False), [5000] * len(chains), main)
    strands = [s.strand for s in plan]
    assert all(plan) and len(plan) > 1500 and min(strands.count(0), strands.count(1)) > len(plan) // 3


# ---- bases in front of the template -------------------------------------------------------------------------------------------
def test_sixteen_dinucleotides_in_front_of_one_fragment(rigs):
    """One fragment of 151 bases at sixteen interior offsets of one chain, each time with another dinucleotide in front of
    it and (turned round: in front of mate 2's read) behind it.  A read's first contexts are X-prefixed, so the bases
    outside the template must not matter: one window per pass at slot 0, and all sixteen passes give the same bases and
    qualities for both mates (and the model's)."""
    rig = rigs(3)
    isz = INSERT0 + 1
    frag, chain, at = letters(isz, 31), bytearray(), []
    for i in range(16):
        di = bytes(b"ACGT"[i >> 2:(i >> 2) + 1] + b"ACGT"[i & 3:(i & 3) + 1])
        chain += letters(97 + i, 300 + i) + di
        at.append(len(chain))
        chain += frag + di
    chain += letters(120, 399)
    rig.set_chains([bytes(chain)])
    seen = set()
    for start in at:
        run, plan, reads = check(rig, table([(0, 0, start, 1, 12, 0)], True), [10 ** 6], STRAIGHT)
        seen.add(tuple(tuple(rec.split(b"\n", 1)[1] for rec in RM.split_records(t)) for t in run.text))
    assert len(seen) == 1 and len(at) == 16


# ---- dead slots among live ones -----------------------------------------------------------------------------------------------
DEAD_CHAIN = letters(3000, 77)


def dead_windows(n_slots, L):
    """Windows of length 1 (live) and windows whose every start is clipped below a read (dead), one per run of slots, so
    that the dead slots are 0, 5, 6, 62, 63, 64, 100, 101, 255, 256 and the last one (those below n_slots)."""
    dead = {s for s in (0, 5, 6, 62, 63, 64, 100, 101, 255, 256) if s < n_slots} | {n_slots - 1}
    if n_slots == 1:
        dead = set()
    rows, s, clen = [], 0, len(DEAD_CHAIN)
    while s < n_slots:
        e = s
        while e < n_slots and (e in dead) == (s in dead):
            e += 1
        if s in dead:
            rows.append((0, 0, clen - L + 1, L - 1, 2 * (e - s), 0))
        else:
            rows.append((0, 0, 100 + 13 * len(rows), 1, 2 * (e - s), 0))
        s = e
    return table(rows, True), dead


@pytest.mark.parametrize("kmer,main", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("n_slots", [1, 62, 63, 64, 65, 255, 256, 257, 1009])
def test_dead_slots_among_live_ones(rigs, kmer, main, n_slots):
    rig = rigs(kmer)
    if rig.chains != [DEAD_CHAIN]:
        rig.set_chains([DEAD_CHAIN])
    windows, dead = dead_windows(n_slots, L0)
    if n_slots == 1009:      # and a window where only late attempts succeed: some of its 40 slots live, the rest dead
        windows = table([w[:6] for w in windows] + [(0, 0, len(DEAD_CHAIN) - L0, L0, 80, 0)], True)
    run, plan, reads = check(rig, windows, [10 ** 6], main)
    assert {k for k, s in enumerate(plan[:n_slots]) if s is None} == dead
    if n_slots == 1009:
        tail = [s is not None for s in plan[n_slots:]]
        assert len(tail) == 40 and 0 < sum(tail) < 40 and tail == sorted(tail, reverse=True)


@pytest.mark.parametrize("kmer,main", KERNELS, ids=KERNEL_IDS)
def test_every_slot_dead(rigs, kmer, main):
    rig = rigs(kmer)
    rig.set_chains([DEAD_CHAIN])
    clen = len(DEAD_CHAIN)
    windows = table([(0, 0, clen - L0 + 1, L0 - 1, 2 * 65, 0), (0, 0, clen - 1, 1, 2 * 200, 0)], True)
    run, plan, reads = check(rig, windows, [10 ** 6], main)
    assert run.text == (b"", b"") and run.fragments == 0 and len(plan) == 265 and not any(plan)
    assert not rig.truth(0, 265)["live"].any() and not rig.truth(1, 265)["live"].any()


# ---- read lengths -------------------------------------------------------------------------------------------------------------
SWEEP_CHAIN = letters(1201, 55)


def sweep_windows(L, isz, pairs=5):
    clen = len(SWEEP_CHAIN)
    starts = list(range(0, 12)) + list(range(100, 700, 9)) + [clen - isz - d for d in range(11, -1, -1)] + [clen - isz + 1, clen - L]
    return table([(0, 0, s, 1, 2 * pairs, 0) for s in starts], True)


@pytest.mark.parametrize("kmer,main,L", [(3, STRAIGHT, L) for L in range(50, 82)] + [(2, ANY_LDS, L) for L in (50, 57, 70)],
                         ids=lambda v: str(v))
def test_read_length_sweep(oracle_lib, tmp_path, kmer, main, L):
    """L = 50 .. 81 (every residue mod 16 twice: plain16 whole steps, the odd last 8-base item, the partial last item),
    fragments of 2 L + 30 at the chain's start, inside it and at its end.  The batch holds, by the model's own indel walk,
    reads without an indel, with one insertion, one deletion and two or more events, and at L = 50 and 51 reads that a
    net deletion would take under 50 bases (reset).  At L = 50 a read with one deletion and nothing else cannot exist -- any
    deletion alone leaves fewer than 50 bases and the read is reset -- so there the one-deletion class must be empty, and
    deletions are present in the reset reads and in the reads of two or more events."""
    with Rig(oracle_lib, str(tmp_path), Shape(kmer, 30, read_length=L, indel_scale=4.0), True, 2 * L + 29) as rig:
        rig.set_chains([SWEEP_CHAIN])
        run, plan, reads = check(rig, sweep_windows(L, 2 * L + 30), [700], main)
        cl = classes_of(reads)
        print("L", L, "read classes", cl, "queued items", run.queued)
        assert all(cl.get(k, 0) >= 1 for k in ("none", "ins", "many")), cl
        assert cl.get("del", 0) >= 1 if L > 50 else cl.get("del", 0) == 0, cl
        assert L > 51 or cl.get("reset", 0) >= 1, cl
        assert sum(s is not None for s in plan) == len(plan) > 400


# ---- the width of the name ----------------------------------------------------------------------------------------------------
BIG = 1_100_000


def name_windows(paired):
    """One segment whose size exceeds the chain: 99,900 fragments at 6-digit positions, then windows at 7-digit positions
    for the fragments numbered 99,901 .. 100,100 (the name's own part "pos#count/m\\n" goes from 16 to 17 bytes at
    1000000#100000/1: text in the read's row, then header_kernel)."""
    per = 2 if paired else 1
    rows = [(0, 0, 100_000 + 8_000 * i, 1 if paired else 50, 999 * per, 0) for i in range(100)]
    rows += [(0, 0, 1_000_000 + 450 * i, 1 if paired else 50, 10 * per, 0) for i in range(20)]
    return table(rows, paired)


@pytest.mark.parametrize("paired", [True, False], ids=["pe", "se"])
def test_name_width(oracle_lib, tmp_path, paired):
    """100,100 fragments of 50-base reads on a chain of 1.1 M bases.  The name line and the record length (from the model's
    indel walk) are compared for every record; bases and qualities for the fragments numbered 99,980 .. 100,020, every
    997th record and the first and last 64 -- the per-read oracle calls are sampled to keep the test at a few seconds."""
    with Rig(oracle_lib, str(tmp_path), Shape(3, 30, read_length=50, indel_scale=4.0), paired, 129) as rig:
        block = letters(1000, 9)
        chain = block * (BIG // 1000)
        rig.set_chains([chain])
        windows = name_windows(paired)
        n = 100_100
        per_read = set(range(99_979, 100_020)) | set(range(0, n, 997)) | set(range(64)) | set(range(n - 64, n))
        run, plan, reads = check(rig, windows, [2_000_000], STRAIGHT, per_read=per_read)
        assert len(plan) == n and all(plan)
        widths = {len(r.name) - len(PREFIX) + 1 for r in reads[0]}
        print("own parts (with the line end) of", sorted(widths), "bytes")
        assert widths >= ({16, 17} if paired else {14, 15})
        assert plan[99_998].fragcount == 99_999 and plan[99_999].fragcount == 100_000 and plan[99_999].pos >= 1_000_000


# ---- many indels --------------------------------------------------------------------------------------------------------------
def test_indel_storm_on_placed_templates(oracle_lib, tmp_path):
    """indel_scale 25 at L = 151 on the straight-line kernel: 2,000 fragments at interior offsets and 200 at each edge of
    the chain; items that two events reach into (the slow queue) and deletions clipped by the read's end."""
    L, insert = 151, 399
    with Rig(oracle_lib, str(tmp_path), Shape(3, 53, read_length=L, indel_scale=25.0), True, insert) as rig:
        chain = letters(4003, 91)
        rig.set_chains([chain])
        clen, isz = len(chain), insert + 1
        starts = [500 + 11 * i for i in range(250)] + list(range(25)) + [clen - isz - d for d in range(24, -1, -1)]
        run, plan, reads = check(rig, table([(0, 0, s, 1, 16, 0) for s in starts], True), [3000], STRAIGHT)
        cl = classes_of(reads)
        clipped = sum(1 for m in reads for r in reads[m] for j, kind, k in r.ev if kind == "D" and j + k == L)
        print("read classes", cl, "deletions that end the read", clipped, "queued items", run.queued)
        assert len(plan) == 2400 and all(plan) and cl.get("many", 0) > 2000 and clipped >= 1 and run.queued > 0 and not run.requeued
