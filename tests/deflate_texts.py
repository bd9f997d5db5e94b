"""Texts for the device BGZF compressor (tests/test_gpu_deflate_texts.py), each aimed at one mechanism of sg_deflate.hip and
each asserting, on the CPU and while it is made, that it has the property it is made for (a generator that cannot build its
text fails; nothing is skipped).  deflate_model.py says what tokens the compressor's rules give for a text; the generators
use its hash restatement to place grams, and tests/test_deflate_read_cpu.py runs every generator without a GPU.

Every generator returns (name, text, facts): `facts` is a dict of what the GPU test asserts on top of the round trip, e.g.
  "matches": [(member, position in the member, length, distance)] that the member's tokens must hold,
  "literal_spans": [(member, start, end)] whose bytes must all leave as literals."""
import random

import numpy as np

import deflate_model as M

CHUNK = M.CHUNK


def rand_bytes(n, seed, alphabet=None):
    rng = np.random.default_rng(seed)
    if alphabet is None:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return np.frombuffer(bytes(alphabet), np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def grams_unique(text):
    """no 8-byte gram occurs twice inside a member (so no copy can be found, whatever the hash does)"""
    for at in range(0, len(text), CHUNK):
        m = text[at:at + CHUNK]
        seen = set()
        for i in range(len(m) - 7):
            g = m[i:i + 8]
            if g in seen:
                return False
            seen.add(g)
    return True


def filler(n, seed, avoid=b""):
    """n random bytes, no two neighbours equal and none of `avoid`: no run bit is set inside it"""
    rng = random.Random(seed)
    ok = [b for b in range(256) if b not in avoid]
    out = bytearray()
    while len(out) < n:
        b = rng.choice(ok)
        if not out or out[-1] != b:
            out.append(b)
    return bytes(out)


# ---- all-equal text ----------------------------------------------------------------------------------------------------
def equal_tokens(n, b):
    """The tokens of a member of n equal bytes, from the rules of sg_deflate.h and gz_tokens / gz_merge.  The member ends at
    the frame's end: with n = 64 j + r, r > 0, lane 511 - j holds r bytes, the j lanes behind it are full.  A run needs a
    previous DATA byte, so the member's first byte is a literal; what follows in its lane is a run if it is at least 5 long,
    else literals; every later lane is one run of 64.  Inside an aligned group of four lanes (lane index / 4, whatever the
    data's start) a run that starts a lane is absorbed by the run that ends the lane before."""
    j, r = divmod(n, 64)
    lanes = []                                     # (lane index, literals, run length or 0)
    if r:
        lanes.append((511 - j, 1 if r - 1 >= 5 else r, r - 1 if r - 1 >= 5 else 0))
    for i in range(j):
        lane = 512 - j + i
        lanes.append((lane, 0, 64) if (r or i) else (lane, 1, 63))
    toks, open_run = [], False
    for lane, lits, run in lanes:
        toks += [("lit", b)] * lits
        if run and open_run and lits == 0 and lane % 4:
            toks[-1] = ("match", toks[-1][1] + run, 1)
        elif run:
            toks.append(("match", run, 1))
        open_run = run > 0
    return toks + [("end",)]


# ---- runs ---------------------------------------------------------------------------------------------------------------
RUN_LENGTHS = range(3, 71)
RUN_OFFSETS = (0, 1, 59, 60, 61, 62, 63)
MEMBER_EDGE_RUNS = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 33, 63, 64, 65, 70)     # (each costs a member of filler)


def runs_text(seed):
    """Runs of L = 3..70 equal bytes starting at the lane offsets 0, 1, 59..63, between filler that has no runs and no
    repeated gram; every run has a byte value of its own inside its member, so that no copy competes with the runs.  Also:
    the same lengths placed so that they cross a 256-byte group edge, and so that they cross the 32,768-byte member edge."""
    rng = random.Random(seed)
    out = bytearray()
    placed = []          # (start, length, byte)
    jobs = [(L, off, None) for L in RUN_LENGTHS for off in RUN_OFFSETS]
    jobs += [(L, None, ("group", rng.randrange(1, L))) for L in RUN_LENGTHS]        # `head` bytes before a 256-byte edge
    jobs += [(L, None, ("member", rng.randrange(1, L))) for L in MEMBER_EDGE_RUNS]
    rng.shuffle(jobs)
    values = list(range(256))
    for L, off, edge in jobs:
        at = len(out) + 80 + rng.randrange(64)           # room for filler
        if edge is None:
            start = at + (off - at) % 64
        elif edge[0] == "group":
            start = at + (-at) % 256 + 256 - edge[1]
        else:
            start = (at // CHUNK + 1) * CHUNK - edge[1]
        gap = start - len(out)
        assert gap >= 8
        b = values[len(placed) % 256]                     # (asserted below: no member holds two long runs of one byte)
        fill = filler(gap, rng.randrange(1 << 30), avoid=bytes([b] + [x for _, _, x in placed[-1:]]))
        out += fill
        out += bytes([b]) * L
        placed.append((start, L, b))
    out += filler(100, 1, avoid=bytes([out[-1]]))
    text = bytes(out)
    for start, L, b in placed:   # the runs are exactly as long as stated
        assert text[start:start + L] == bytes([b]) * L and text[start - 1] != b and text[start + L] != b
    # no copy competes: a run's byte value occurs in runs of >= 8 at most once per member
    for at in range(0, len(text), CHUNK):
        inside = [b for start, L, b in placed if L >= 8 and start < at + CHUNK and start + L > at]
        assert len(inside) == len(set(inside)), "a member holds two long runs of one byte"
    return "runs", text, {"runs": [(s, L) for s, L, _ in placed]}


def runs_inside_a_lane(runs):
    """[(member, position in the member, length)] of the runs that lie inside one lane: the rules give them one literal and a
    match (L - 1, 1) from six bytes on, literals below"""
    return [(start // CHUNK, start % CHUNK, L) for start, L in runs if start // 64 == (start + L - 1) // 64]


# ---- the six-match cap --------------------------------------------------------------------------------------------------
def cap_text(seed0=1):
    """Members in which some lanes hold eight runs of six equal bytes (one literal and a match (5, 1) each, if taken), in a
    text where no 8-byte gram occurs twice.  Returns the lanes too: (member, lane)."""
    for seed in range(seed0, seed0 + 50):
        rng = random.Random(seed)
        n = CHUNK + 64 * 37 + 20          # a full member and a short one whose frame starts inside a lane
        text = bytearray(filler(n, seed))
        lanes = []
        q0_last = CHUNK - (n - CHUNK)
        for member, lane in [(0, 0), (0, 1), (0, 5), (0, 255), (0, 256), (0, 510), (0, 511)] + [(1, 512 - 37 + i) for i in (0, 1, 17, 36)]:
            base = lane * 64 - (q0_last if member else 0) + member * CHUNK
            assert base >= member * CHUNK
            vals = rng.sample(range(256), 16)
            body = b"".join(bytes([vals[i]]) * 6 + bytes([vals[8 + i]]) for i in range(8))      # 8 x (6 + 1) = 56 bytes
            lane_bytes = body + filler(8, rng.randrange(1 << 30), avoid=bytes([vals[15]]))
            text[base:base + 64] = lane_bytes
            # the bytes around the lane must not lengthen its first or last run
            if base > member * CHUNK and text[base - 1] == lane_bytes[0]:
                text[base - 1] ^= 0x55
            lanes.append((member, lane))
        text = bytes(text)
        if grams_unique(text):
            return "six_match_cap", text, {"cap_lanes": lanes, "q0_last": q0_last}
    raise AssertionError("no text without a repeated gram in 50 seeds")


# ---- copies -------------------------------------------------------------------------------------------------------------
PERIODS = (2, 3, 7, 8, 9, 63, 64, 65, 151, 152, 32767)


def period_text(p, seed, n=2 * CHUNK + 4000):
    """a unit of p bytes (no two neighbours equal) over and over"""
    return "period_%d" % p, (filler(p, seed * 1000 + p) * (n // p + 1))[:n], {"period": p}


def place(text, at, piece):
    text[at:at + len(piece)] = piece


def _wins_slot(text, pos):
    """the gram at the even position `pos` of a full member is the one the table keeps for its slot"""
    F = M.Frame(text)
    return pos % 2 == 0 and F.entry[int(F.slot[pos])] == pos


def _alone(text, src, dst, n):
    """text[src:src+n] == text[dst:dst+n] and the bytes before and behind the two differ: the copy is exactly n long"""
    return text[src:src + n] == text[dst:dst + n] and text[src - 1] != text[dst - 1] and text[src + n] != text[dst + n]


COPY_KINDS = ("overlap", "back2", "back3", "short_acgt", "short_qual", "short_hash")


def directed_copy_text(kind):
    """One full member of filler (no runs, no A C G T #) with source pieces near its start and repeats further on.
      "overlap"    distance smaller than length: pieces of period 3, 5 and 12, 52 bytes long, at the start of a lane, that occur
                   nowhere else: all but their first bytes copy from themselves
      "back2", "back3"   a 20-byte repeat whose start falls at residue 2 / 3 (mod 4): no probe falls on its start; the
                   probe at residue 0 / 1 behind it finds the gram two bytes in (the source's even position) and grows back
      "short_acgt", "short_qual", "short_hash"   repeats of 8, 9, 10, 11 bytes made of A/C/G/T, of quality symbols, and of
                   quality symbols with a '#': at min_copy 12 the first and the third kind are taken, the second is not
    A seed whose source gram loses its table slot to an earlier position is passed over (the next seed is tried)."""
    assert kind in COPY_KINDS
    avoid = b"ACGT#"
    for seed in range(1, 200):
        rng = random.Random(seed)
        text = bytearray(filler(CHUNK, seed + 17, avoid=avoid))
        facts = {"matches": [], "literal_spans": []}
        sources = []        # even positions whose gram must own its slot
        if kind == "overlap":
            for i, (period, first_hit) in enumerate(((3, 2), (5, 0), (12, 0))):
                unit = filler(period, seed + period, avoid=avoid)
                dst = 64 * (20 + 3 * i)
                place(text, dst, (unit * 30)[:52])     # 52 bytes of the unit's repetition, at a lane's start: the copy's source is the piece itself
                sources.append(dst + first_hit)        # the even position whose gram the first probe with a hit (k = 5, 5, 12) finds
            text = bytes(text)
        elif kind in ("back2", "back3"):
            piece = filler(20, seed + 5, avoid=avoid)
            res = 2 if kind == "back2" else 3
            src, dst = 64, 64 * 40 + 8 + res
            place(text, src, piece)
            place(text, dst, piece)
            text = bytes(text)
            if not _alone(text, src, dst, 20):
                continue
            sources.append(src + 2)                    # the gram the probe at dst + 2 (residue 0 or 1) looks up
            facts["matches"].append((0, dst, 20, dst - src))
            facts["grown_back"] = 2
        else:
            alphabet = {"short_acgt": b"ACGT", "short_qual": b"FJ<7-,", "short_hash": b"FJ<7-,"}[kind]
            ok = True
            for i, L in enumerate((8, 9, 10, 11)):
                piece = bytearray(filler(L, seed * 100 + L, avoid=bytes(b for b in range(256) if b not in alphabet)))
                if kind == "short_hash":
                    piece[2 + i] = ord("#")
                src, dst = 64 + 64 * i, 64 * (40 + 3 * i) + 8
                place(text, src, piece)
                place(text, dst, piece)
                ok = ok and _alone(bytes(text), src, dst, L)
                sources.append(src)
                if kind == "short_qual":
                    facts["literal_spans"].append((0, dst, dst + L))
                else:
                    facts["matches"].append((0, dst, L, dst - src))
            text = bytes(text)
            if not ok:
                continue
        if all(_wins_slot(text, q) for q in sources):
            return kind, text, facts
    raise AssertionError("no text for %s" % kind)


def tag_collision_pair(seed=1, tries=1 << 22):
    """two different grams with the same slot and the same 17-bit tag under gz_hash: the same 32-bit hash.  With the low
    word fixed the hash is (c + hi) * K mod 2^32, a bijection of hi, so two grams collide only with different low words:
    pick lo1, hi1, lo2 and solve for hi2."""
    rng = random.Random(seed)
    for _ in range(tries):
        g1 = bytes(rng.choice(b"abcdefghijklmnop") for _ in range(8))
        lo2 = bytes(rng.choice(b"qrstuvwxyz012345") for _ in range(4))
        lo1, hi1 = int.from_bytes(g1[:4], "little"), int.from_bytes(g1[4:], "little")
        l2 = int.from_bytes(lo2, "little")
        hi2 = (lo1 * 0x9E3779B1 + hi1 - l2 * 0x9E3779B1) & 0xFFFFFFFF
        g2 = lo2 + hi2.to_bytes(4, "little")
        # keep the pair free of runs, so that no run bit interferes
        if all(g2[i] != g2[i + 1] for i in range(7)) and all(g1[i] != g1[i + 1] for i in range(7)):
            assert g1 != g2 and M.hash_of(g1) == M.hash_of(g2)
            return g1, g2
    raise AssertionError("no colliding pair found")


def tag_collision_text(seed=3):
    """gram A early at an even position (it takes the slot), gram B -- same slot, same tag, other bytes -- later at probed
    positions: the probe says "hit", the verification must refuse it, and B's bytes leave as literals.  Then A again, later
    still: a true copy through the same slot."""
    a, b = tag_collision_pair(seed)
    text = bytearray(filler(CHUNK, seed + 23, avoid=a + b))
    place(text, 66, a)
    pos_b = [64 * 30 + 8, 64 * 31 + 9, 64 * 300 + 12]
    for p in pos_b:
        place(text, p, b)
    pos_a = 64 * 200 + 16
    place(text, pos_a, a + a[:4])     # twelve bytes: taken at the default min_copy whatever the bytes are
    place(text, 66 + 8, a[:4])
    text = bytes(text)
    F = M.Frame(text)
    assert F.entry[M.slot_tag(a)[0]] == 66, "another gram took the slot first"
    assert M.slot_tag(a) == M.slot_tag(b) and a != b
    return "tag_collision", text, {"literal_spans": [(0, p, p + 8) for p in pos_b], "matches": [(0, pos_a, 12, pos_a - 66)]}


# ---- byte values --------------------------------------------------------------------------------------------------------
def byte_value_texts():
    out = []
    r = rand_bytes(3 * CHUNK, 77)
    out.append(("nul_at_start_full", bytes(700) + r[:CHUNK - 700] + r[:900], {}))
    for n in (1, 2, 5, 8, 9, 64, 65, 200, 700):           # a short last chunk that ENDS with NULs (the pad behind it is zeros) ...
        out.append(("nul_at_end_%d" % n, r[:CHUNK] + r[:300] + bytes(n), {}))
        out.append(("nul_at_start_%d" % n, r[:CHUNK] + bytes(n) + r[:300], {}))    # ... and one that STARTS with them (so does the frame before it)
        out.append(("nul_only_%d" % n, bytes(n), {}))
    out.append(("nul_mixed", b"".join(bytes(k) + r[100 * k:100 * k + 7] for k in range(1, 120)), {}))
    out.append(("ff_only", b"\xff" * (CHUNK + 777), {}))
    out.append(("ff_mixed", b"".join(b"\xff" * k + r[50 * k:50 * k + 5] for k in range(1, 120)), {}))
    out.append(("all_values_in_order", bytes(range(256)) * 200, {}))
    out.append(("all_values_random", r, {}))
    return out


# ---- codes the sample never saw ---------------------------------------------------------------------------------------
STEEP = b"!\"$%&'()*+,-./0"      # fifteen symbols, none of A C G T #


def unseen_codes_text(members=1026, seed=9):
    """Every stride-th member (the ones the histogram sees) is ONE member drawn from a distribution that halves from symbol
    to symbol, so that the literal code built from it is limited at 15 bits; all other members hold none of its bytes:
    uniform random bytes of the other 241 values (15-bit literals throughout: the largest members there are), with a
    64-byte piece repeated at distances the sampled member never uses."""
    stride = M.sample_stride(members)
    assert stride == 3
    rng = np.random.default_rng(seed)
    p = np.array([2.0 ** -(i + 1) for i in range(len(STEEP))])
    p /= p.sum()
    sampled = np.frombuffer(STEEP, np.uint8)[rng.choice(len(STEEP), CHUNK, p=p)].tobytes()
    others = bytes(b for b in range(256) if b not in STEEP)
    out = []
    for m in range(members):
        if m % stride == 0:
            out.append(sampled)
        else:
            body = bytearray(rand_bytes(CHUNK, seed * 100000 + m, others))
            piece = bytes(body[2:66])
            for at in (20002, 30000 - (m % 7) * 2):
                body[at:at + 64] = piece
            out.append(bytes(body))
    text = b"".join(out)[:(members - 1) * CHUNK + 12345]
    return "unseen_codes", text, {"stride": stride, "sampled": sampled}


# ---- seeded mixtures ----------------------------------------------------------------------------------------------------
def _pieces(rng):
    n = rng.randrange(1, 400)
    kind = rng.randrange(9)
    s = rng.randrange(1 << 30)
    if kind == 0:
        return bytes([rng.randrange(256)]) * n
    if kind == 1:
        return rand_bytes(n, s)
    if kind == 2:
        return rand_bytes(n, s, b"ACGT")
    if kind == 3:
        return rand_bytes(n, s, b"FFFFFFFFFFFFF<,#")
    if kind == 4:
        return (rand_bytes(rng.choice(PERIODS[:-1]), s) * 400)[:n]
    if kind == 5:
        return bytes(rng.choice((1, 2, 3, 70)))
    if kind == 6:
        return b"\xff" * rng.randrange(1, 80)
    if kind == 7:
        return b"@r%d#%d/1\n" % (rng.randrange(10 ** 9), rng.randrange(100))
    return b"".join(bytes([rng.randrange(256)]) * rng.randrange(3, 12) for _ in range(rng.randrange(1, 20)))


def mixture(seed):
    """a random concatenation of the pieces above -- earlier pieces come back, whole or in part, at random offsets -- of a
    random total length up to a few members"""
    rng = random.Random(seed)
    total = rng.choice((rng.randrange(1, 300), rng.randrange(1, CHUNK), rng.randrange(CHUNK - 70, CHUNK + 70), rng.randrange(1, 3 * CHUNK + 100)))
    out, pool = bytearray(), []
    while len(out) < total:
        if pool and rng.random() < 0.4:
            p = rng.choice(pool)
            a = rng.randrange(len(p))
            p = p[a:a + rng.randrange(1, 200)]
        else:
            p = _pieces(rng)
            pool.append(p)
        out += p
    return bytes(out[:total])
