"""sg_truth_align -- the truth-alignment rule as the engine library states it (host code, no GPU) -- against the Python
model of the same rule (tests/truth_model.py): one hand-made case per clause of the rule with the CIGAR it must give
written out, then seeded random piece tables and event lists, and the invariants every alignment keeps."""
import random

import pytest

import simuscop_amd
import truth_model as tm
from truth_model import D, I, M, N, S


def both(pieces, off, L, reverse, events=()):
    got = simuscop_amd.truth_align(pieces, off, L, reverse, [tm.ev_pack(*e) for e in events])
    exp = tm.align(pieces, off, L, reverse, events)
    assert got == exp, (got, exp, pieces, off, L, reverse, events)
    return got


REF = [(0, 1000, 500, 0, 0, 1)]   # one reference piece: chain offset x is contig position 1000 + x


def test_plain_read():
    assert both(REF, 100, 50, False) == (0, 1100, [(50, M)])


def test_each_strand_counts_events_from_its_own_end():
    # an insertion of 2 behind read base 10: forward 11M2I39M; reverse the same event sits 11 bases from the chain END
    assert both(REF, 100, 50, False, [(10, 2, False)]) == (0, 1100, [(11, M), (2, I), (39, M)])
    assert both(REF, 100, 50, True, [(10, 2, False)]) == (0, 1100, [(39, M), (2, I), (11, M)])
    assert both(REF, 100, 50, True, [(10, 3, True)]) == (0, 1100, [(37, M), (3, D), (10, M)])


def test_insertion_behind_the_last_base_is_clipped():
    assert both(REF, 100, 50, False, [(49, 3, False)]) == (0, 1100, [(50, M), (3, S)])
    assert both(REF, 100, 50, True, [(49, 3, False)]) == (0, 1100, [(3, S), (50, M)])


def test_deletion_at_index_0_moves_the_position():
    assert both(REF, 100, 50, False, [(0, 4, True)]) == (0, 1104, [(46, M)])
    assert both(REF, 100, 50, True, [(0, 4, True)]) == (0, 1100, [(46, M)])      # the read's start is the chain's end


def test_events_inside_a_literal_piece():
    pieces = [(0, 1000, 120, 0, 0, 1), (120, 7, 10, 0, 1, 0), (130, 1120, 300, 0, 0, 0)]   # a 10-base variant insertion
    assert both(pieces, 100, 50, False) == (0, 1100, [(20, M), (10, I), (20, M)])
    # a deletion of 3 of the literal's bases shortens the I; an insertion inside it lengthens it
    assert both(pieces, 100, 50, False, [(22, 3, True)]) == (0, 1100, [(20, M), (7, I), (20, M)])
    assert both(pieces, 100, 50, False, [(22, 2, False)]) == (0, 1100, [(20, M), (12, I), (20, M)])
    # a deletion across the literal's end: its bases vanish, the reference base behind becomes D
    assert both(pieces, 100, 50, False, [(28, 4, True)]) == (0, 1100, [(20, M), (8, I), (2, D), (18, M)])


def test_variant_deletion_is_D():
    pieces = [(0, 1000, 120, 0, 0, 1), (120, 1125, 300, 0, 0, 0)]
    assert both(pieces, 100, 50, False) == (0, 1100, [(20, M), (5, D), (30, M)])
    assert both(pieces, 100, 50, True) == (0, 1100, [(20, M), (5, D), (30, M)])


def test_target_gap_is_N():
    pieces = [(0, 1000, 120, 0, 0, 1), (120, 5000, 300, 0, 0, 1)]
    assert both(pieces, 100, 50, False) == (0, 1100, [(20, M), (3880, N), (30, M)])
    # the segment may begin with a literal: the gap in front of its first reference piece is still N
    pieces = [(0, 1000, 120, 0, 0, 1), (120, 0, 4, 0, 1, 1), (124, 5000, 300, 0, 0, 0)]
    assert both(pieces, 100, 50, False) == (0, 1100, [(20, M), (4, I), (3880, N), (26, M)])


def test_backward_joint_and_contig_change_end_the_alignment():
    back = [(0, 1000, 120, 0, 0, 1), (120, 1000, 300, 0, 0, 0)]      # a second copy of the same slice
    assert both(back, 100, 50, False) == (0, 1100, [(20, M), (30, S)])
    assert both(back, 100, 50, False, [(25, 2, False), (40, 3, True)]) == (0, 1100, [(20, M), (29, S)])
    other = [(0, 1000, 120, 0, 0, 1), (120, 0, 300, 1, 0, 1)]
    assert both(other, 100, 50, True) == (0, 1100, [(20, M), (30, S)])


def test_read_inside_a_literal_is_unmapped():
    pieces = [(0, 1000, 100, 0, 0, 1), (100, 0, 200, 0, 1, 0), (300, 1100, 100, 0, 0, 0)]
    assert both(pieces, 120, 50, False) == (-1, -1, [])
    assert both(pieces, 120, 50, True, [(3, 2, False)]) == (-1, -1, [])
    # one reference base is enough
    assert both(pieces, 51, 50, False) == (0, 1051, [(49, M), (1, S)])


def test_32_events():
    ev = [(4 * i, 1, i % 2 == 1) for i in range(32)]
    c, pos, ops = both(REF, 0, 151, False, ev)
    assert (c, pos) == (0, 1000) and len(ops) == 65 and tm.query_length(ops) == 151
    both(REF, 0, 151, True, ev)


def test_bad_arguments_are_refused():
    with pytest.raises(simuscop_amd.SimuError):
        simuscop_amd.truth_align(REF, 480, 50, False)                              # runs off the pieces
    with pytest.raises(simuscop_amd.SimuError):
        simuscop_amd.truth_align(REF, 0, 50, False, [tm.ev_pack(10, 2, True), tm.ev_pack(11, 1, False)])   # inside a deletion
    with pytest.raises(simuscop_amd.SimuError):
        simuscop_amd.truth_align(REF, 0, 50, False, [tm.ev_pack(0, 1, True)] * 2, cap=0)


@pytest.mark.parametrize("seed", range(10))
def test_random_tables_match_the_model(seed):
    rng = random.Random(7700 + seed)
    mapped = 0
    for _ in range(2500):
        pieces, off, L, reverse, events = tm.random_case(rng)
        contig, pos, ops = both(pieces, off, L, reverse, events)
        n_ins = sum(k for _, k, d in events if not d)
        n_del = sum(k for _, k, d in events if d)
        if not ops:
            assert (contig, pos) == (-1, -1)
            continue
        mapped += 1
        # the query length is the read's; neighbours differ; clips and gaps only where they may stand
        assert tm.query_length(ops) == L + n_ins - n_del
        assert all(a[1] != b[1] for a, b in zip(ops, ops[1:])) and all(n > 0 for n, _ in ops)
        core = [o for _, o in ops if o != S]
        assert core[0] == M and core[-1] == M
        assert all(o != S for _, o in ops[1:-1])
    assert mapped > 2000


def test_reference_span_of_reads_on_one_piece():
    """On unbroken reference the span is the template minus the deleted bases at its two ends."""
    rng = random.Random(99)
    for _ in range(3000):
        L = rng.choice((50, 100, 151))
        _, _, _, reverse, events = tm.random_case(rng, L)
        contig, pos, ops = both(REF, 200, L, reverse, events)
        gone = [False] * L
        for j, k, d in events:
            if d:
                for x in range(j, j + k):
                    gone[x] = True
        if all(gone):
            assert ops == []
            continue
        lead = next(i for i in range(L) if not gone[i])
        trail = next(i for i in range(L) if not gone[L - 1 - i])
        if reverse:
            lead, trail = trail, lead
        assert pos == 1200 + lead and tm.reference_span(ops) == L - lead - trail
