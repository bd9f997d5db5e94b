"""The front of a sampling pass -- batch_map_kernel at plan time, edge_kernel and fragment_kernel in the pass -- on
hand-placed windows, read by read against tests/read_model.py with the harness of test_gpu_reads_placed.py (Rig, check:
names, bases, qualities, byte totals, the fragment count of sg_result, and the rows of sg_truth_reads, whose chain comes
from the slot -> window look-up).

What can go wrong here is the bookkeeping, not the draws: which window owns a slot (blocks of 256 slots, windows that span
blocks, more windows than lanes in a block, runs of empty windows longer than a block), which windows are edge windows
(an attempt can fail) and which segments hold one (their fragment numbers come from edge_kernel's scan, the others' from
slot arithmetic), the attempts of an edge window drawn 64 at a time, and the first indel draw handed from a read's lane
to the lane that walks it.

Shapes: reads of 60 bases, fragments of 151 (the one-column insert profile), chains of a few thousand bases, a few
hundred to a few thousand slots.  `SAFE` windows lie where every start leaves 151 bases; `sixtieth` / `tenth` windows
lie on a chain's last 60 starts so that one start in 60 / 10 leaves a whole read: they give up after 1000 failures with
about 17 / 100 fragments made."""
import pytest

import read_model as RM
import test_gpu_reads_placed as placed
from profile_shapes import Shape
from test_gpu_reads_placed import INSERT0, L0, STRAIGHT, ANY_LDS, Rig, check, letters, table
from test_gpu_reads_placed import rigs  # noqa: F401  (the module's shared contexts, a set of their own for this module)

pytestmark = pytest.mark.gpu

ISZ = INSERT0 + 1
CHAINS = [letters(6000, 501), letters(2500, 502)]
CLEN = [len(c) for c in CHAINS]


def per(paired):
    return 2 if paired else 1


def safe(spos, frags, seg, chain=0, paired=True):
    """A window of 200 starts (paired; single end: 60, the fragment's length) none of whose attempts can fail."""
    wlen = 200 if paired else L0
    assert spos + wlen - 1 + (ISZ if paired else wlen) <= CLEN[chain]
    return (0, chain, spos, wlen, frags * per(paired), seg)


def sixtieth(frags, seg, chain=0, paired=True):
    """Starts clen - 60 .. clen - 1: only the first leaves a read of 60 bases."""
    return (0, chain, CLEN[chain] - L0, L0, frags * per(paired), seg)


def tenth(frags, seg, chain=0):
    """(paired) starts clen - 60 .. clen - 51: one in ten succeeds, about 100 fragments before the window gives up"""
    return (0, chain, CLEN[chain] - L0, 10, frags * 2, seg)


def never_fails(frags, seg, chain=0):
    """(paired) an edge window by the test (its last start leaves fewer than 151 bases) all of whose attempts succeed"""
    return (0, chain, CLEN[chain] - ISZ - 10, 30, frags * 2, seg)


def use_chains(rig):
    if rig.chains != CHAINS:
        rig.set_chains(CHAINS)


def dead_of(plan):
    return [k for k, s in enumerate(plan) if s is None]


# ---- slot -> window ------------------------------------------------------------------------------------------------------------
def test_one_window_over_three_blocks(rigs):
    """700 fragments of one window: slots 255 | 256, 257, 511 | 512 lie in three blocks that start inside the window."""
    rig = rigs(3)
    use_chains(rig)
    _, plan, _ = check(rig, table([safe(100, 700, 0)], True), [4000], STRAIGHT)
    assert len(plan) == 700 and all(plan) and [plan[k].fragcount for k in (255, 256, 257, 511, 512)] == [256, 257, 258, 512, 513]


@pytest.mark.parametrize("paired", [True, False], ids=["pe", "se"])
@pytest.mark.parametrize("n_slots", [1, 63, 64, 255, 256, 257])
def test_batch_sizes(rigs, paired, n_slots):
    """Windows of 1 .. 5 fragments up to n_slots, in two segments."""
    rig = rigs(3, paired)
    use_chains(rig)
    rows, left = [], n_slots
    while left:
        n = min(left, 1 + len(rows) % 5)
        rows.append(safe(50 + 7 * len(rows), n, 0 if len(rows) < 20 else 1, paired=paired))
        left -= n
    _, plan, _ = check(rig, table(rows, paired), [900, 1100], STRAIGHT)
    assert len(plan) == n_slots and all(plan)


def test_more_windows_than_lanes_start_in_one_block(rigs):
    rig = rigs(3)
    use_chains(rig)
    rows = [(0, 0, 10 + 3 * i, 1, 1 + (i & 1), i // 100) for i in range(300)]   # n_reads 1 and 2: one pair each
    _, plan, _ = check(rig, table(rows, True), [500, 600, 700], STRAIGHT)
    assert len(plan) == 300 and all(plan) and plan[299].fragcount == 100


@pytest.mark.parametrize("kmer,main", [(3, STRAIGHT), (2, ANY_LDS)], ids=["straight_line_k3", "generic_k2"])
def test_runs_of_empty_windows(rigs, kmer, main):
    """More than 256 empty windows (n_reads 0 and negative) at the batch's start, between two windows that own slots --
    across a segment boundary -- and at its end; two empty windows that share their slot_base with the window behind."""
    rig = rigs(kmer)
    use_chains(rig)
    def empty(n, seg):
        return [(0, 0, 20 + i, 1, 0 if i % 3 else -3, seg) for i in range(n)]
    rows = empty(300, 0) + [safe(400, 5, 0)] + empty(150, 0) + empty(150, 1) + [safe(900, 300, 1)] + empty(2, 1) + [safe(1500, 7, 1)]
    rows += empty(300, 1) + empty(5, 2)
    windows = table(rows, True)
    assert windows[300 + 1 + 300 + 1][6] == windows[300 + 1 + 300 + 3][6] == 305
    _, plan, _ = check(rig, windows, [3000, 3100, 3200], main)
    assert len(plan) == 312 and all(plan)


def test_empty_batch(rigs):
    rig = rigs(3)
    use_chains(rig)
    run, plan, _ = check(rig, [], [1000], STRAIGHT, truth=False)
    assert run.text == (b"", b"") and run.fragments == 0 and plan == []
    run, plan, _ = check(rig, table([(0, 0, 5, 1, 0, 0), (0, 0, 6, 1, -1, 0)], True), [1000], STRAIGHT, truth=False)
    assert run.text == (b"", b"") and run.fragments == 0 and plan == []


# ---- edge windows and flagged segments -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [True, False], ids=["pe", "se"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_edge_window_that_gives_up(rigs, paired, where):
    """A window that makes about 17 of its 40 fragments, in front of, between and behind the safe windows of its segment:
    the fragment numbers behind it continue from what it made.  An unflagged segment follows."""
    rig = rigs(3, paired)
    use_chains(rig)
    others = [safe(300 + 400 * i, 50, 0, paired=paired) for i in range(3)]
    at = {"first": 0, "middle": 2, "last": 3}[where]
    rows = others[:at] + [sixtieth(40, 0, paired=paired)] + others[at:] + [safe(200, 30, 1, paired=paired), safe(2000, 30, 1, paired=paired)]
    windows = table(rows, paired)
    run, plan, _ = check(rig, windows, [5000, 700], STRAIGHT)
    dead = dead_of(plan)
    first = windows[at][6]
    assert 5 <= len(dead) <= 35 and dead == list(range(first + 40 - len(dead), first + 40)), dead
    assert run.fragments == 250 - len(dead)
    if where != "last":   # the first fragment behind the edge window
        assert plan[first + 40].fragcount == first + 40 - len(dead) + 1
    assert plan[190].fragcount == 1 and plan[249].fragcount == 60


MIXED_SEG_SIZES = [5000, 777, 2222]


def mixed_rows():
    """Segment 0 (flagged: a window that gives up in its middle), segment 1 (no edge window), segment 2 on the other chain
    (flagged: first a window that makes more than 64 fragments and gives up, then an edge window that never fails)."""
    return [safe(100, 60, 0), sixtieth(40, 0), safe(1000, 50, 0),
            safe(300, 120, 1), safe(2500, 80, 1),
            tenth(150, 2, chain=1), safe(50, 70, 2, chain=1), never_fails(100, 2, chain=1), safe(700, 30, 2, chain=1)]


def test_flagged_and_unflagged_segments(rigs):
    """Two flagged segments round an unflagged one; block 0 holds slots of segment 0 (flagged) and of segment 1 (not)."""
    rig = rigs(3)
    use_chains(rig)
    windows = table(mixed_rows(), True)
    assert windows[3][6] == 150 and windows[5][6] == 350            # segment 1 = slots 150 .. 349
    run, plan, _ = check(rig, windows, MIXED_SEG_SIZES, STRAIGHT)
    dead = dead_of(plan)
    d0, d2 = [k for k in dead if k < 150], [k for k in dead if k >= 350]
    assert dead == d0 + d2 and 5 <= len(d0) <= 35 and d0[-1] == 99
    made = 150 - len(d2)
    assert 70 <= made <= 135 and d2 == list(range(350 + made, 500)), (made, d2)    # more than one round of 64 attempts counted
    assert plan[150].fragcount == 1 and plan[349].fragcount == 200 and plan[500].fragcount == made + 1
    assert all(plan[570:670]) and plan[-1].fragcount == made + 200 and {s.chain for s in plan if s} == {0, 1}


def test_every_window_is_an_edge_window(rigs):
    rig = rigs(3)
    use_chains(rig)
    rows = [sixtieth(40, 0), never_fails(10, 0), tenth(3, 0), sixtieth(1, 1, chain=1), never_fails(130, 1, chain=1), tenth(150, 1, chain=1)]
    run, plan, _ = check(rig, table(rows, True), [901, 902], STRAIGHT)
    assert len(plan) == 334 and 30 <= len(dead_of(plan)) <= 120 and run.fragments == 334 - len(dead_of(plan))


def test_shard_of_a_mixed_batch(rigs):
    """Segments 1 and 2 of the mixed batch as a shard (first_window 3, first_slot 150) are the same reads as in the whole."""
    rig = rigs(3)
    use_chains(rig)
    windows = table(mixed_rows(), True)
    whole = rig.run(windows, MIXED_SEG_SIZES)
    head = windows[:3]
    tail = [(hb, c, sp, ln, n, seg - 1, sb - 150) for hb, c, sp, ln, n, seg, sb in windows[3:]]
    a, _, _ = check(rig, head, MIXED_SEG_SIZES[:1], STRAIGHT)
    b, _, _ = check(rig, tail, MIXED_SEG_SIZES[1:], STRAIGHT, first_window=3, first_slot=150)
    assert a.text[0] + b.text[0] == whole.text[0] and a.text[1] + b.text[1] == whole.text[1]
    assert a.fragments + b.fragments == whole.fragments


# ---- names ---------------------------------------------------------------------------------------------------------------------
def test_long_prefix(oracle_lib, tmp_path, monkeypatch):
    """A prefix longer than 16 bytes (header_kernel writes the names) on a batch with a flagged and an unflagged segment."""
    monkeypatch.setattr(placed, "PREFIX", b"@a_population_with_a_name#chr21#")
    assert len(placed.PREFIX) > 16
    with Rig(oracle_lib, str(tmp_path), placed.K3, True) as rig:
        rig.set_chains(CHAINS)
        _, plan, reads = check(rig, table(mixed_rows()[:5], True), MIXED_SEG_SIZES[:2], STRAIGHT)
        assert reads[0][0].name.startswith(b"@a_population_with_a_name#chr21#") and len(plan) == 350


def test_name_longer_than_its_row(oracle_lib, tmp_path):
    """The name's own part "pos#count/m\\n" goes from 16 to 17 bytes inside a flagged segment: 8-digit positions, fragment
    numbers up to 10,1xx behind a window that gave some up.  Names and record lengths of every record; bases and
    qualities of the first and last 64, every 499th and those round the step."""
    big = 10_100_000
    with Rig(oracle_lib, str(tmp_path), Shape(3, 30, read_length=50, indel_scale=4.0), True, 129) as rig:
        rig.set_chains([letters(1000, 9) * (big // 1000)])
        rows = [(0, 0, big - 50, 50, 2 * 40, 0)] + [(0, 0, 10_000_000 + 900 * i, 1, 2 * 100, 0) for i in range(101)]
        windows = table(rows, True)
        made = len(rig.model.plan_window(windows[0], 0, big)[0])
        step = 40 + 9_999 - made                       # the slot of fragment number 10,000
        per_read = set(range(64)) | set(range(10_140 - 64, 10_140)) | set(range(0, 10_140, 499)) | set(range(step - 20, step + 20))
        expected = placed.expect(rig.model, rig.chains, windows, [20_000_000], per_read=per_read)
        _, plan, reads = check(rig, windows, [20_000_000], STRAIGHT, expected=expected)
        assert 0 < made < 40 and len(plan) == 10_140 and plan[step].fragcount == 10_000 and plan[step].pos >= 10_000_000
        widths = {len(r.name) - len(placed.PREFIX) + 1 for r in reads[0]}
        assert widths >= {16, 17}, widths


# ---- the indel walk --------------------------------------------------------------------------------------------------------------
def zero_length_profile(path, shape, sd="0.1"):
    """read_model.one_column_profile with 0.2 of the mass of the indel lengths moved from length 1 to length 0: a
    candidate can come to nothing (Profile::getIndelSeq draws the length, Profile.cpp:1556-1574)."""
    plain_profile(path, shape, sd)
    lines = open(path).read().split("\n")
    for sec in ("[Insert Frequency]", "[Deletion Frequency]"):
        at = lines.index(sec) + 1
        f = [float(v) for v in lines[at].split("\t")]
        assert f[0] == 0 and f[1] > 0.3
        f[0], f[1] = 0.2, f[1] - 0.2
        lines[at] = "\t".join("%.6g" % v for v in f)
    with open(path, "w") as out:
        out.write("\n".join(lines))
    return path


plain_profile = RM.one_column_profile


def test_walks_on_a_profile_with_many_indels(oracle_lib, tmp_path, monkeypatch):
    """Reads of 51 bases at 25 times the indel rates, a fifth of the indel lengths 0: the walk of a listed read starts
    from the draw its own lane made (call e = 0) and goes on with call 1.  By the model alone the batch must hold reads
    all of whose candidates drew the length 0 (no event after a candidate), reads reset because they would keep fewer
    than 50 bases, and reads with one and with several events."""
    L, insert = 51, 131
    monkeypatch.setattr(RM, "one_column_profile", zero_length_profile)
    with Rig(oracle_lib, str(tmp_path), Shape(3, 30, read_length=L, indel_scale=25.0), True, insert) as rig:
        chain = letters(3001, 93)
        rig.set_chains([chain])
        zero_draws = []
        plain = RM.ReadModel.rand_index

        def counting(x, cdf):
            k = plain(x, cdf)
            zero_draws.append(k == 0)
            return k

        starts = list(range(0, 8)) + [200 + 9 * i for i in range(100)] + [len(chain) - insert - 1 - d for d in range(8)]
        windows = table([(0, 0, s, 1, 2 * 6, 0) for s in starts] + [(0, 0, len(chain) - L, L, 2 * 30, 0)], True)
        rig.model.rand_index = counting
        try:
            no_event_after_candidate = 0
            for slot in range(windows[-1][6] + 30):
                for m in (0, 1):
                    del zero_draws[:]
                    ev, reset = rig.model.events(m, slot)
                    no_event_after_candidate += bool(zero_draws) and all(zero_draws) and not ev and not reset
            expected = placed.expect(rig.model, rig.chains, windows, [2000])
        finally:
            del rig.model.rand_index
        cl = placed.classes_of(expected[1])
        print("read classes", cl, "reads whose candidates all drew the length 0", no_event_after_candidate)
        assert no_event_after_candidate >= 3 and cl.get("reset", 0) >= 3 and min(cl.get(k, 0) for k in ("none", "ins", "del", "many")) >= 10, cl
        run, plan, _ = check(rig, windows, [2000], STRAIGHT, expected=expected)
        assert len(plan) == 116 * 6 + 30 and 0 < len(dead_of(plan)) < 30


# ---- the bad-block bit ---------------------------------------------------------------------------------------------------------
def test_unknown_base_in_every_block_of_a_word(rigs):
    """The bit "a 64-base block of the chains buffer holds a non-ACGT base" lies in 16-bit words, one per 1024 bases;
    fragment_kernel reads a template's blocks from one word or from two neighbouring ones.  Sixteen N, 1088 bases (17
    blocks) apart, fall into every block position of a word whatever the chain's offset in the buffer; templates of
    both mates start 90 bases before each N to 10 behind it, so that their two or three blocks lie in one word and
    across two, with the N's block first, in the middle, last, and just outside.  A read that misses its bit samples
    an N from the 2-bit codes: wrong bases."""
    rig = rigs(3)
    at = [1000 + 1088 * i for i in range(16)]
    chain = bytearray(letters(at[-1] + 600, 601))
    for p in at:
        chain[p] = ord("N")
    rig.set_chains([bytes(chain)])
    rows = []
    for p in at:
        for t in range(p - L0 - 30, p + 11, 3):
            rows.append((0, 0, t, 1, 4, 0))                      # mate 1's template starts at t
            rows.append((0, 0, t - (ISZ - L0), 1, 4, 0))         # mate 2's template starts at t
    run, plan, reads = check(rig, table(rows, True), [10 ** 6], STRAIGHT)
    with_n = sum(b"N" in r.rec.split(b"\n")[1] for m in reads for r in reads[m])
    print("reads with an N", with_n, "of", 2 * len(plan), "queued items", run.queued)
    assert all(plan) and len(plan) == 16 * 34 * 2 * 2 and with_n > 1000 and run.queued > 0


def test_unknown_base_under_long_reads(oracle_lib, tmp_path):
    """Reads of 1100 bases: a template with its slack spans 18 or 19 blocks, more than the two-word test takes, so its
    blocks are tested one by one.  One N; templates of both mates that hold it near their start, in their middle and
    near their end, and templates that do not reach it."""
    L, insert = 1100, 2229
    with Rig(oracle_lib, str(tmp_path), Shape(3, 30, read_length=L, indel_scale=0.25), True, insert) as rig:
        chain = bytearray(letters(9000, 602))
        p = 4500
        chain[p] = ord("N")
        rig.set_chains([bytes(chain)])
        isz, rows = insert + 1, []
        for t in (p - L - 40, p - L + 1, p - L + 30, p - 600, p - 31, p, p + 20):
            rows.append((0, 0, t, 1, 4, 0))
            rows.append((0, 0, t - (isz - L), 1, 4, 0))
        run, plan, reads = check(rig, table(rows, True), [10 ** 6], STRAIGHT)
        with_n = sum(b"N" in r.rec.split(b"\n")[1] for m in reads for r in reads[m])
        print("reads with an N", with_n, "of", 2 * len(plan), "queued items", run.queued)
        assert all(plan) and len(plan) == 28 and with_n >= 8 and run.queued > 0
