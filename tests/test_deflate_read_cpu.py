"""The DEFLATE token reader of the tests (tests/deflate_read.py) against zlib and against the writer of deflate_craft.py,
without the GPU.  test_gpu_deflate_texts.py asserts token lists read with it; a reader that is quietly wrong would make those
assertions worthless.  On every stream here the reader's expansion is what zlib.decompressobj(-15) returns, it stops where
zlib stops, and its blocks, written again by deflate_craft.Stream, are the stream's own bytes: the 33 legal streams of the
directed corpus, the 180 generated ones (whose tokens are known: the reader returns them), what zlib's compressor writes at
levels 1, 6, 9 and with Z_FIXED, Z_RLE and Z_HUFFMAN_ONLY, and members assembled from the host's plan as test_deflate_plan.py
assembles them (whose tokens are known too).

The second half holds the self-checks of what else test_gpu_deflate_texts.py stands on: deflate_model.py (its tokens expand
to the text, on every text of deflate_texts.py; its closed forms) and the generators of deflate_texts.py (each text has the
property it is made for: the facts it states hold in the model's tokens, the colliding grams collide, the text that is to
reach the six-match cap has no gram twice, the sampled member of the unseen-codes text makes a 15-bit code)."""
import heapq
import random
import zlib

import numpy as np
import pytest

import deflate_craft as D
import deflate_model as M
import deflate_read as R
import deflate_texts as T
import test_deflate_plan as P

CHUNK = M.CHUNK


def check(raw, what):
    """reader == zlib on the output and on where the stream ends; reader -> writer == the stream's bytes"""
    d = zlib.decompressobj(-15)
    want = d.decompress(raw)
    assert d.eof, what
    s = R.read(raw)
    assert s.out == want, what
    assert raw[s.end:] == d.unused_data, what
    assert R.rewrite(s) == raw[:s.end], what
    assert s.blocks[-1].final and not any(b.final for b in s.blocks[:-1]), what
    assert all(b.tokens[-1] == ("end",) for b in s.blocks if b.kind), what
    return s


def craft_tokens(s):
    """the reader's tokens in the writer's form, block by block"""
    return [("stored", b.stored) if b.kind == 0 else ("tokens", b.craft) for b in s.blocks]


def test_directed_legal_streams():
    legal = [c for c in D.directed() if c.legal]
    assert len(legal) == 33
    for c in legal:
        s = check(c.raw, c.name)
        assert craft_tokens(s) == c.blocks, c.name
    by = {c.name: R.read(c.raw) for c in legal}
    assert max(by["codes_of_1_to_15_bits"].blocks[0].lit_lens) == 15 and max(by["codes_of_1_to_15_bits"].blocks[0].dist_lens) == 15
    assert ("match", 258, 32768) in by["match_ends_at_65536"].tokens()
    assert ("match", 258, 1) in by["length_258_as_symbol_284_extra_31"].tokens()
    assert [b.kind for b in by["stored_of_0_bytes"].blocks] == [0, 1, 0, 0]


def test_generated_streams():
    seeds = D.seeds(D.GEN_SEEDS)
    assert len(seeds) >= 180
    kinds = set()
    for seed in seeds:
        g = D.generate(seed)
        s = check(g.raw(), "seed %d" % seed)
        assert craft_tokens(s) == g.blocks, seed
        kinds |= {b.kind for b in s.blocks}
    assert kinds == {0, 1, 2}


def _texts():
    rng = random.Random(11)
    fq = []
    for i in range(120):
        fq.append(b"@r%d/1\n%s\n+\n%s\n" % (rng.randrange(10 ** 9), bytes(rng.choice(b"ACGT") for _ in range(150)), bytes(rng.choice(b"#,-7<AFJ") for _ in range(150))))
    fq = b"".join(fq)
    return {"empty": b"", "one_byte": b"A", "fastq": fq, "two_symbols": bytes(rng.choice(b"AC") for _ in range(20000)),
            "random": bytes(rng.randrange(256) for _ in range(9000)), "one_symbol": b"\0" * 70000, "repeat": fq[:3000] * 12}


@pytest.mark.parametrize("level,strategy", [(1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED),
                                            (6, zlib.Z_RLE), (6, zlib.Z_HUFFMAN_ONLY)])
def test_zlib_made_streams(level, strategy):
    matches = 0
    for name, text in _texts().items():
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        raw = c.compress(text) + c.flush()
        s = check(raw, (name, level, strategy))
        assert s.out == text
        toks = s.tokens()
        matches += sum(1 for t in toks if t[0] == "match")
        if strategy == zlib.Z_HUFFMAN_ONLY:
            assert b"".join(b.stored if b.kind == 0 else bytes(t[1] for t in b.tokens if t[0] == "lit") for b in s.blocks) == text
        if strategy == zlib.Z_RLE:
            assert all(t[2] == 1 for t in toks if t[0] == "match")
        if strategy == zlib.Z_FIXED:
            assert all(b.kind != 2 for b in s.blocks)   # (random bytes leave as stored blocks)
    assert (matches == 0) == (strategy == zlib.Z_HUFFMAN_ONLY)
    # a stream in several blocks of several kinds (full flushes), bytes behind it
    a, b = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy), zlib.compressobj(0, zlib.DEFLATED, -15)
    t = _texts()
    raw = a.compress(t["fastq"]) + a.flush(zlib.Z_FULL_FLUSH) + b.compress(t["random"]) + b.flush(zlib.Z_FULL_FLUSH)
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    raw += c.compress(t["repeat"]) + c.flush()
    s = check(raw + b"\x01\x02\x03", "several blocks")
    assert s.out == t["fastq"] + t["random"] + t["repeat"] and {blk.kind for blk in s.blocks} >= {0}


@pytest.mark.parametrize("kind", ["fastq", "uniform", "one_symbol", "short"])
def test_members_assembled_from_the_plan(kind):
    rng = np.random.default_rng(5)
    data = {"fastq": lambda: P._fastq(rng, 90), "uniform": lambda: bytes(rng.integers(0, 256, 5000, dtype=np.uint8)), "one_symbol": lambda: b"A" * 3000,
            "short": lambda: b"ACGTACGTACGTAC"}[kind]()
    toks = P.tokens(data)
    m = P._member(data, toks, P._plan(*P.histograms(toks)))
    s = check(m[18:-8], kind)
    assert s.out == data and len(s.blocks) == 1 and s.blocks[0].kind == 2
    assert min(s.blocks[0].lit_lens) >= 1 and len(s.blocks[0].lit_lens) == 286 and len(s.blocks[0].dist_lens) == 30
    assert s.tokens() == [("match",) + t if isinstance(t, tuple) else ("lit", t) for t in toks] + [("end",)]


# ---------------------------------------------------------------------------------------------------------------------
# the model of the compressor's token choice and the text generators
# ---------------------------------------------------------------------------------------------------------------------
def model_holds(name, text, facts, stats=None):
    """the model's tokens are a parse of the text (written as a fixed block, zlib returns the member) and hold the facts"""
    per_member = M.text_tokens(text, stats)
    assert len(per_member) == (len(text) + CHUNK - 1) // CHUNK
    for i, toks in enumerate(per_member):
        want = text[i * CHUNK:(i + 1) * CHUNK]
        assert M.expand(toks) == want, (name, i)
        assert toks[-1] == ("end",) and all(t[0] != "match" or (3 <= t[1] <= 256 and t[2] <= at) for at, t in M.positions(toks)), (name, i)
    at = [dict(M.positions(t)) for t in per_member]
    for member, pos, length, dist in facts.get("matches", []):
        assert at[member].get(pos) == ("match", length, dist), (name, member, pos, length, dist, at[member].get(pos))
    for member, a, b in facts.get("literal_spans", []):
        assert all(at[member].get(p, ("",))[0] == "lit" for p in range(a, b)), (name, member, a, b)
    return per_member


def test_equal_tokens_closed_form_by_hand():
    """deflate_texts.equal_tokens at the sizes worked out by hand from sg_deflate.h, and against the model at every size"""
    assert T.equal_tokens(CHUNK, 65) == [("lit", 65), ("match", 255, 1)] + [("match", 256, 1)] * 127 + [("end",)]
    assert T.equal_tokens(1, 7) == [("lit", 7), ("end",)]
    assert T.equal_tokens(5, 7) == [("lit", 7)] * 5 + [("end",)]
    assert T.equal_tokens(6, 7) == [("lit", 7), ("match", 5, 1), ("end",)]
    assert T.equal_tokens(64, 7) == [("lit", 7), ("match", 63, 1), ("end",)]
    assert T.equal_tokens(64 * 4 + 63, 7) == [("lit", 7), ("match", 62, 1), ("match", 256, 1), ("end",)]       # lane 507 | lanes 508-511
    assert T.equal_tokens(64 * 5 + 5, 7) == [("lit", 7)] * 5 + [("match", 64, 1), ("match", 256, 1), ("end",)]
    for b in (0, 65, 255):
        for n in list(range(1, 700)) + [CHUNK - 65, CHUNK - 64, CHUNK - 1, CHUNK]:
            assert M.member_tokens(bytes([b]) * n) == T.equal_tokens(n, b), (b, n)


def test_model_tokens_written_by_the_craft_writer_inflate_to_the_text():
    """model -> deflate_craft.Stream (a fixed block) -> zlib: the model's lengths and distances are real copies"""
    def craft(t):
        ls = max(i for i in range(29) if D.LEN_BASE[i] <= t[1] and (i < 28 or t[1] == 258))
        ds = max(i for i in range(30) if D.DIST_BASE[i] <= t[2])
        return (ls, t[1] - D.LEN_BASE[ls], ds, t[2] - D.DIST_BASE[ds])
    for seed in range(1, 13):
        text = T.mixture(seed)[:CHUNK]
        toks = M.member_tokens(text)
        s = D.Stream()
        s.fixed([t[1] if t[0] == "lit" else craft(t) for t in toks[:-1]], final=True)
        assert zlib.decompress(s.raw(), -15) == text, seed
        assert R.read(s.raw()).tokens() == toks, seed


def test_hash_restatement_and_colliding_grams():
    # gz_hash by hand on two grams: ((lo * 0x9E3779B1 + hi) mod 2^32) * 0x85EBCA77 mod 2^32
    assert M.hash_of(bytes(8)) == 0 and M.hash_of(b"\x01" + bytes(7)) == (0x9E3779B1 * 0x85EBCA77) & 0xFFFFFFFF
    assert M.hash_of(bytes(4) + b"\x01" + bytes(3)) == 0x85EBCA77
    a, b = T.tag_collision_pair(3)
    assert a != b and len(a) == len(b) == 8 and M.slot_tag(a) == M.slot_tag(b)
    stats = {}
    name, text, facts = T.tag_collision_text()
    model_holds(name, text, facts, stats)
    assert stats["tag_collisions"] >= 3        # the probes hit, the verification refuses


def test_generated_texts_have_the_properties_they_are_made_for():
    stats = {}
    name, text, facts = T.runs_text(1)
    model_holds(name, text, facts, stats)
    lengths = {L for _, L in facts["runs"]}
    assert lengths == set(T.RUN_LENGTHS) and min(lengths) < M.MIN_RUN + 1 < max(lengths)
    assert {s % 64 for s, L in facts["runs"]} >= set(T.RUN_OFFSETS)
    assert sum(1 for s, L in facts["runs"] if s // 256 != (s + L - 1) // 256) >= len(T.RUN_LENGTHS)
    assert sum(1 for s, L in facts["runs"] if s // CHUNK != (s + L - 1) // CHUNK) == len(T.MEMBER_EDGE_RUNS)
    assert stats["absorbed"] >= 10 and len(T.runs_inside_a_lane(facts["runs"])) >= 100

    stats = {}
    name, text, facts = T.cap_text()
    assert T.grams_unique(text) and not T.grams_unique(text[:100] + text[:100])
    per_member = model_holds(name, text, facts, stats)
    assert stats["capped_lanes"] == len(facts["cap_lanes"]) == 11 and not stats.get("short_left") and not stats.get("tag_collisions")
    for member, lane in facts["cap_lanes"]:
        base = lane * 64 - (facts["q0_last"] if member else 0)
        assert sum(1 for p, t in M.positions(per_member[member]) if base <= p < base + 64 and t[0] == "match") == M.LANE_MATCHES

    for kind in T.COPY_KINDS:
        stats = {}
        name, text, facts = T.directed_copy_text(kind)
        toks = model_holds(name, text, facts, stats)[0]
        assert facts["matches"] or facts["literal_spans"] or kind == "overlap"
        if kind == "overlap":
            assert sum(1 for t in toks if t[0] == "match" and t[2] < t[1]) >= 3
        if kind.startswith("back"):
            assert stats["grown_back"] == 1 and facts["matches"][0][1] % 4 == (2 if kind == "back2" else 3)
        if kind == "short_qual":
            assert stats["short_left"] == 4 and not stats.get("short_taken")
        if kind in ("short_acgt", "short_hash"):
            assert stats["short_taken"] == 4 and not stats.get("short_left") and [m[2] for m in facts["matches"]] == [8, 9, 10, 11]

    for p in T.PERIODS:
        name, text, facts = T.period_text(p, 1)
        for toks in model_holds(name, text, facts):
            assert all(t[2] % p == 0 for t in toks if t[0] == "match")
    for name, text, facts in T.byte_value_texts():
        model_holds(name, text, facts)
    assert {b for _, t, _ in T.byte_value_texts() for b in t} == set(range(256))


def test_unseen_codes_text_limits_the_code_at_15_bits():
    name, text, facts = T.unseen_codes_text()
    n_mem = (len(text) + CHUNK - 1) // CHUNK
    assert n_mem >= 1026 and M.sample_stride(n_mem) == 3 and facts["stride"] == 3
    assert all(text[i * CHUNK:(i + 1) * CHUNK] == facts["sampled"] for i in range(0, n_mem - 1, 3))
    assert not set(text[CHUNK:3 * CHUNK]) & set(T.STEEP)
    toks = M.member_tokens(facts["sampled"])
    lit, dist = P.histograms([(t[1], t[2]) if t[0] == "match" else t[1] for t in toks[:-1]])
    plan = P._plan(lit * (n_mem // 3), dist * (n_mem // 3))
    assert max(plan["lit_len"][:256]) == 15 and min(plan["lit_len"][b] for b in T.STEEP) <= 2
    assert all(plan["lit_len"][b] >= 14 for b in set(text[CHUNK:3 * CHUNK]))
    # the limit is at work: a Huffman code of this histogram (every symbol counted once more, as the host does) is deeper
    heap = [(int(n) * (n_mem // 3) + 1, i, 0) for i, n in enumerate(lit)]
    heapq.heapify(heap)
    while len(heap) > 1:
        (w1, i1, d1), (w2, i2, d2) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (w1 + w2, min(i1, i2), max(d1, d2) + 1))
    assert heap[0][2] > 15


def test_mixtures_reach_every_branch_of_the_model():
    stats, sizes = {}, []
    for seed in range(1, 41):
        text = T.mixture(seed)
        sizes.append(len(text))
        model_holds("mixture %d" % seed, text, {}, stats)
    for key in ("tag_collisions", "grown_back", "short_left", "short_taken", "absorbed", "capped_lanes"):
        assert stats.get(key, 0) > 0, (key, stats)
    assert min(sizes) < 300 and max(sizes) > 2 * CHUNK
