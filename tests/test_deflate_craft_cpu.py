"""The DEFLATE writer of the tests (tests/deflate_craft.py) against zlib, without the GPU.  A writer that is quietly wrong would
make test_gpu_inflate_adversarial.py worthless, so: every legal stream of the directed corpus inflates to the bytes its own
tokens predict (an LZ77 expansion written here, not a read-back of zlib), every illegal one is refused by zlib for the
stated reason and all thirteen reasons occur; the generator's streams are all legal, all fit a member, and reach codes of 15
bits, length 258 at distance 32768 and 65,536 bytes of output; both of the mutator's outcomes are frequent for both kinds of
source."""
import collections
import zlib

import deflate_craft as D

MESSAGES = ("invalid block type", "invalid stored block lengths", "too many length or distance symbols", "invalid code lengths set",
            "invalid bit length repeat", "invalid code -- missing end-of-block", "invalid literal/lengths set", "invalid distances set",
            "invalid literal/length code", "invalid distance code", "invalid distance too far back")
OUTCOMES = MESSAGES + (D.NO_EOF, D.TOO_LONG)


def expand(blocks):
    """what the blocks say: stored bytes as they are, a literal as one byte, a match as `length` bytes from `distance` back"""
    out = bytearray()
    for kind, body in blocks:
        if kind == "stored":
            out += body
            continue
        for t in body:
            if isinstance(t, int):
                out.append(t)
            else:
                n, dist = D.match_len(t), D.match_dist(t)
                assert 1 <= dist <= len(out), "the writer's own tokens reach before the output"
                for _ in range(n):
                    out.append(out[-dist])
    return bytes(out)


def test_directed_legal_streams_inflate_to_what_their_tokens_say():
    corpus = D.directed()
    legal = [c for c in corpus if c.legal]
    assert len(legal) >= 30
    for c in legal:
        d = zlib.decompressobj(-15)
        got = d.decompress(c.raw)
        assert d.eof, c.name
        assert got == expand(c.blocks), c.name
        assert len(got) <= D.MAXI, c.name
        assert D.reference(c.raw) == (True, got, None), c.name
    # only the stored block of 65,535 bytes is too large for a member; it is in the corpus for this file alone
    assert [c.name for c in corpus if not c.fits] == ["stored_of_65535_bytes"]
    # leftover bytes: zlib ends the stream and leaves them
    for c in legal:
        if "left_before_the_trailer" in c.name:
            d = zlib.decompressobj(-15)
            d.decompress(c.raw)
            assert d.eof and d.unused_data, c.name


def test_directed_legal_streams_hold_what_their_names_say():
    by = {c.name: c for c in D.directed()}

    def matches(name):
        return [(D.match_len(t), D.match_dist(t), len(expand(by[name].blocks))) for k, b in by[name].blocks if k == "tokens" for t in b if not isinstance(t, int)]

    assert (258, 32768, 65536) in matches("match_ends_at_65536")
    assert any(t[:2] == (258, 32768) for t in matches("distance_32768_at_32768"))
    assert len(expand(by["stored_that_fills_the_member"].blocks)) + 5 == D.MAX_RAW == len(by["stored_that_fills_the_member"].raw)
    assert len(expand(by["stored_of_65535_bytes"].blocks)) == 65535
    s = D.Stream()
    lit16 = list(range(16))
    s.dynamic(lit16[:15], D.chain(lit16[:15] + [256]), {}, final=True)
    assert s.used_lit == 15 and sorted(D.chain(lit16).values()) == list(range(1, 16)) + [15]
    # symbol 284 with extra bits 31 is length 258
    assert D.match_len((27, 31, 0, 0)) == 258 and D.LEN_BASE[28] == 258


def test_directed_illegal_streams_are_refused_for_the_stated_reason():
    seen = collections.Counter()
    for c in D.directed():
        if c.legal:
            continue
        assert c.outcome in OUTCOMES, c.name
        legal, _, outcome = D.reference(c.raw)
        assert not legal and outcome == c.outcome, (c.name, outcome)
        if c.outcome in MESSAGES:
            try:
                zlib.decompressobj(-15).decompress(c.raw)
                raise AssertionError(c.name)
            except zlib.error as e:
                assert str(e).endswith(c.outcome), (c.name, str(e))
        seen[c.outcome] += 1
    assert sorted(seen) == sorted(OUTCOMES), set(OUTCOMES) - set(seen)   # each of the thirteen outcomes occurs


def test_every_legal_case_has_its_illegal_neighbour():
    by = {c.name: c.legal for c in D.directed()}
    pairs = (("distance_equals_bytes_written", "distance_one_more_than_bytes_written"), ("distance_32768_at_32768", "distance_32768_at_32767"),
             ("match_ends_at_65536", "match_ends_at_65537"), ("short_match_ends_at_65536", "short_match_ends_at_65537"),
             ("literal_ends_at_65536", "literal_ends_at_65537"), ("stored_ends_at_65536", "stored_ends_at_65537"),
             ("one_distance_code_of_length_1_used", "one_distance_code_of_length_1_other_bit"), ("no_distance_code_literals_only", "no_distance_code_but_a_match"),
             ("one_literal_code_of_length_1_empty_block", "one_literal_code_of_length_1_other_bit"),
             ("code_length_code_complete", "code_length_code_incomplete"), ("code_length_code_complete", "code_length_code_over_subscribed"),
             ("hlit_286", "hlit_287"), ("hlit_286", "hlit_288"), ("hdist_30", "hdist_31"), ("hdist_30", "hdist_32"),
             ("run_of_16_as_second_item", "run_of_16_as_first_item"), ("run_of_16_as_second_item", "run_of_18_past_the_last_length"),
             ("codes_of_1_to_15_bits", "literal_code_incomplete"), ("codes_of_1_to_15_bits", "literal_code_over_subscribed"),
             ("codes_of_1_to_15_bits", "distance_code_incomplete"), ("codes_of_1_to_15_bits", "distance_code_over_subscribed"),
             ("stored_of_0_bytes", "stored_len_is_not_the_complement_of_nlen"), ("stored_that_fills_the_member", "stored_of_65535_bytes_past_the_member"),
             ("fixed_block_of_every_literal", "no_final_block"), ("codes_of_1_to_15_bits", "data_ends_in_a_symbol"),
             ("fixed_block_of_every_literal", "fixed_symbol_286"), ("fixed_block_of_every_literal", "fixed_distance_code_30"),
             ("hlit_286", "no_end_of_block_code"))
    for good, bad in pairs:
        assert by[good] is True and by[bad] is False, (good, bad)


def test_generated_streams_are_legal_fit_a_member_and_reach_the_edges():
    refused = too_big = 0
    lit_depth = dist_depth = far_258 = 0
    sizes = collections.Counter()
    kinds = collections.Counter()
    for seed in D.seeds(D.GEN_SEEDS):
        s = D.generate(seed)
        raw = s.raw()
        legal, out, outcome = D.reference(raw)
        refused += not legal
        too_big += len(raw) > D.MAX_RAW
        assert legal and out == expand(s.blocks) and len(out) == s.total, (seed, outcome)
        sizes[len(out)] += 1
        lit_depth, dist_depth = max(lit_depth, s.used_lit), max(dist_depth, s.used_dist)
        for k, b in s.blocks:
            kinds[k] += 1
            if k == "tokens":
                far_258 += sum(1 for t in b if not isinstance(t, int) and D.match_len(t) == 258 and D.match_dist(t) == 32768)
    print("generator: %d streams, sizes %s, deepest literal/length code used %d, distance code %d, 258 at 32768: %d, blocks %s" %
          (sum(sizes.values()), sorted(sizes.items()), lit_depth, dist_depth, far_258, dict(kinds)))
    assert refused == 0 and too_big == 0
    assert lit_depth == 15 and dist_depth == 15     # codes of 15 bits, used by tokens
    assert far_258 >= 1
    assert sizes[65536] >= 1 and set(sizes) == set(D.GEN_SIZES)
    assert kinds["stored"] >= 10 and kinds["tokens"] >= 100


def test_generator_stays_inside_the_member_at_its_worst():
    # the largest output with literals wherever the budget lets them: the bound holds while the stream is written
    for seed in range(1000, 1012):
        s = D.generate(seed, total=65536)
        raw = s.raw()
        assert len(raw) <= D.MAX_RAW and D.reference(raw)[0] and len(expand(s.blocks)) == 65536, seed


def test_both_outcomes_of_a_mutation_are_frequent():
    n, ok = collections.Counter(), collections.Counter()
    for _, source, raw in D.mutated(D.seeds(D.MUT_SEEDS)):
        n[source] += 1
        ok[source] += D.reference(raw)[0]
    print("mutator: zlib accepts %d of %d zlib-made and %d of %d crafted" % (ok["zlib"], n["zlib"], ok["craft"], n["craft"]))
    for source in ("zlib", "craft"):
        assert n[source] >= 500
        assert 10 * ok[source] >= n[source], source                 # zlib accepts at least a tenth ...
        assert 10 * (n[source] - ok[source]) >= n[source], source   # ... and refuses at least a tenth


def test_member_trailer_is_zlibs_output_and_the_sweep_sizes_are_on_the_edge():
    for c in D.directed():
        if not c.fits:
            continue
        m = D.member(c.raw)
        out = D.reference(c.raw)[1][:D.MAXI]
        assert m[18:-8] == c.raw and int.from_bytes(m[-4:], "little") == len(out) and int.from_bytes(m[-8:-4], "little") == zlib.crc32(out)
        assert int.from_bytes(m[16:18], "little") + 1 == len(m)
    s = D.CRC_SIZES
    assert set(range(2101)) <= set(s) and {65281, 65533, 65534, 65535, 65536} <= set(s) and max(s) == 65536
    assert all(k * 1024 + d in s for k in range(1, 64) for d in (-1, 0, 1, 2, 3, 4))
    assert sum(1 for n in s if n > 3 and n % 1024 in (1, 2, 3)) >= 3 * 63
    for n in (0, 1, 7, 8, 9, 1025, 65536):
        p = D.crc_payload(n)
        assert len(p) == n and len(set(p[:8])) == min(n, 8)
        assert len(zlib.compress(p, 1)) <= max(64, n // 8)
