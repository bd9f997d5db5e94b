"""The truth BAM's coordinate sort on the MI355X (sg_bamsort_*, simuscop_amd/csrc/sg_bamsort.hip) against Python's stable
`sorted`: the merge on synthetic records over a bare context -- counts around the wave and the sort block, keys that are
equal, ascending, descending, differ in one byte only or are 2^64 - 1, 1 / 2 / 7 runs with empty ones, record lengths
from the shortest legal record to the longest the record kernel makes at L = 410, every residue mod 16 at source and
destination -- its BGZF members against zlib, its index, and a sorted pass through a Session against `sorted` of the
unsorted pass's records, with and without tags."""
import ctypes as C
import random
import struct

import pytest

import cases
import profile_shapes as PS
import simuscop_amd
import truth_util as U
from profile_shapes import Shape

pytestmark = pytest.mark.gpu

SEED = (cases.FAKE_SEC << 32) | cases.FAKE_NSEC
TILE = simuscop_amd.BAMSORT_TILE
KMAX = 2 ** 64 - 1
MIN_LEN = 4 + 32 + 2                                    # block_size, the fixed fields, a one-letter name and its NUL
# the record kernel's image at L = 410: fixed part, a 255-byte name, 256 operations, L + 512 bases, all three tags
MAX_LEN = 36 + 256 + 4 * 256 + (922 + 1) // 2 + 922 + 7 + 7 + 3 + 2048 + 1


@pytest.fixture(scope="module")
def ctx():
    lib = simuscop_amd.load_engine()
    c = C.c_void_p()
    assert lib.sg_create(C.byref(c), 0, 1) == 0
    yield c
    lib.sg_destroy(c)


def record(rng, key, n):
    """n bytes that read as a BAM record at `key`: block_size, refID, POS, then bytes of any value."""
    assert n >= MIN_LEN
    return struct.pack("<III", n - 4, key >> 32, key & 0xFFFFFFFF) + rng.randbytes(n - 12)


def make_runs(rng, keys_per_run, lens=None):
    runs = []
    for keys in keys_per_run:
        ln = [next(lens) if lens else rng.choice((MIN_LEN, 150, 299, 300, 301, 317, rng.randrange(MIN_LEN, 700))) for _ in keys]
        runs.append((b"".join(record(rng, k, n) for k, n in zip(keys, ln)), list(keys), ln))
    return runs


def model(runs):
    """The records in run order, sorted stably by key: (stream, keys, lens)."""
    recs = []
    for data, keys, lens in runs:
        at = 0
        for k, n in zip(keys, lens):
            recs.append((k, data[at:at + n]))
            at += n
        assert at == len(data)
    recs = sorted(recs, key=lambda r: r[0])
    return b"".join(r for _, r in recs), [k for k, _ in recs], [len(r) for _, r in recs]


def check(ctx, runs):
    stream, members, keys, lens = simuscop_amd.bamsort_merge(ctx, runs)
    w_stream, w_keys, w_lens = model(runs)
    assert keys == w_keys and lens == w_lens                      # sg_bamsort_index
    assert stream == w_stream
    if stream:
        assert U.inflate_members(members, want_eof=False) == stream   # the members are the stream's
    else:
        assert members == b""
    return stream


def split(keys, n_runs, rng):
    """keys cut into n_runs runs, one of them empty when there are several; each run ascending (what a merge is given)."""
    cuts = [rng.randrange(len(keys) + 1) for _ in range(max(0, n_runs - 2))]
    if n_runs > 1:
        cuts.append(rng.choice(cuts + [0, len(keys)]))            # a cut twice: an empty run among them
    cuts.sort()
    parts = [keys[a:b] for a, b in zip([0] + cuts, cuts + [len(keys)])]
    return [sorted(p) for p in parts]


COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 1)


@pytest.mark.parametrize("n", COUNTS)
def test_merge_counts_and_key_orders(ctx, n):
    rng = random.Random(n)
    pos = [rng.randrange(1 << 20) for _ in range(n)]
    for kind, keys in (("equal", [7 << 32 | 99] * n), ("ascending", sorted(pos)), ("descending", sorted(pos, reverse=True)),
                       ("random with ties", [rng.randrange(3) << 32 | rng.randrange(40) for _ in range(n)])):
        for n_runs in (1, 2, 7):
            if kind == "descending":   # one run whose keys do not ascend: still sorted, it is a sort and not a merge
                cuts = sorted(rng.randrange(n + 1) for _ in range(n_runs - 1))
                parts = [keys[a:b] for a, b in zip([0] + cuts, cuts + [n])]
            else:
                parts = split(keys, n_runs, rng)
            check(ctx, make_runs(rng, parts))


def test_no_runs_and_empty_runs(ctx):
    assert check(ctx, []) == b""
    assert check(ctx, [(b"", [], [])]) == b""
    assert check(ctx, [(b"", [], []), (b"", [], [])]) == b""


@pytest.mark.parametrize("byte", range(8))
def test_keys_that_differ_in_one_byte_only(ctx, byte):
    rng = random.Random(100 + byte)
    base = 0x0102030405060708 & ~(0xFF << (8 * byte))
    keys = [base | (rng.randrange(256) << (8 * byte)) for _ in range(2 * TILE + 5)]
    check(ctx, make_runs(rng, split(keys, 2, rng)))
    check(ctx, make_runs(rng, [keys]))


def test_the_largest_key_among_others(ctx):
    rng = random.Random(5)
    keys = [rng.choice((KMAX, KMAX - 1, 0, 1, 5 << 32 | 0xFFFFFFFF, 6 << 32, 0xFFFFFFFF << 32, rng.getrandbits(64))) for _ in range(TILE + 300)]
    check(ctx, make_runs(rng, split(keys, 7, rng)))
    check(ctx, make_runs(rng, [[KMAX] * 70, [KMAX] * 3 + [0]]))   # (the second run does not ascend)


def test_record_lengths_and_every_residue(ctx):
    """Lengths from the shortest legal record to the longest the record kernel makes at L = 410, and every pair of
    residues mod 16 of a record's source and destination offsets."""
    rng = random.Random(11)
    want = [MIN_LEN, MIN_LEN + 1, 47, 48, 49, 63, 64, 65, 1023, 1024, 1025, 1039, 1040, 1041, MAX_LEN - 1, MAX_LEN] + list(range(MIN_LEN, MIN_LEN + 33))
    lens = want + [rng.randrange(MIN_LEN, 420) for _ in range(2 * TILE)]
    rng.shuffle(lens)
    keys = [rng.randrange(1 << 16) for _ in lens]
    runs = make_runs(rng, split(keys, 7, rng), iter(lens))
    check(ctx, runs)
    # which residues the case had: source offsets in upload order, destination offsets in sorted order
    src, at = [], 0
    for _, ks, ls in runs:
        for k, n in zip(ks, ls):
            src.append((k, at % 16, n))
            at += n
    pairs, at = set(), 0
    for k, s16, n in sorted(src, key=lambda r: r[0]):
        pairs.add((s16, at % 16))
        at += n
    assert len(pairs) == 256


@pytest.mark.parametrize("seed", range(6))
def test_seeded_random_mixes(ctx, seed):
    rng = random.Random(1000 + seed)
    n = rng.choice((5, 300, TILE + rng.randrange(-3, 4), 2 * TILE + 77))
    pool = [rng.getrandbits(64) for _ in range(rng.choice((1, 3, 50)))] + [KMAX, 0]
    keys = [rng.choice(pool) if rng.random() < 0.5 else (rng.randrange(4) << 32 | rng.randrange(5000)) for _ in range(n)]
    lens = (rng.choice((MIN_LEN, MAX_LEN)) if rng.random() < 0.02 else rng.randrange(MIN_LEN, 400) for _ in iter(int, 1))
    check(ctx, make_runs(rng, split(keys, rng.choice((1, 2, 7)), rng), lens))


def test_a_merge_leaves_the_context_working_and_refuses_bad_tables(ctx):
    eng = simuscop_amd.load_engine()
    rng = random.Random(3)
    runs = make_runs(rng, [[3, 3, 9]])
    data, keys, lens = runs[0]
    with pytest.raises(simuscop_amd.SimuError, match="do not add up"):
        simuscop_amd.bamsort_merge(ctx, [(data + b"x", keys, lens)])
    n = C.c_uint64()
    assert eng.sg_bamsort_index(ctx, None, None, 0, C.byref(n)) != 0          # a refused merge leaves no index
    check(ctx, runs)
    assert eng.sg_bamsort_index(ctx, None, None, 0, C.byref(n)) == 0 and n.value == 3
    buf = C.create_string_buffer(8)
    assert eng.sg_bamsort_fetch(ctx, 0, sum(lens) - 4, 8, buf) != 0            # past the end of the stream


# ---- a sorted pass through a Session ----
@pytest.mark.parametrize("shape,layout", [(Shape(3, 53), "PE"), (Shape(3, 52), "SE")])
def test_sorted_pass_equals_sorted_records_of_the_pass(shape, layout, tmp_path):
    cfg = PS.build_shape_case(shape, str(tmp_path), layout)
    ties = checked = 0
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=SEED, truth_bam=1) as sess:
        sess.weighted_length()
        sess.set_reads(sess.planned_reads)
        for chrom in range(sess.n_chromosomes):
            if not sess.prepare_batch(chrom):
                continue
            sess.sample()
            sess.result()
            for tags in (0, simuscop_amd.TAG_ALL):
                rb, _ = sess.truth_bam(tags)
                plain = sess.fetch_truth(False, rb)
                info, tag_info = sess.truth_info(), sess.truth_tag_info()
                recs, at = [], 0
                while at < len(plain):
                    n = 4 + struct.unpack_from("<I", plain, at)[0]
                    ref, pos = struct.unpack_from("<II", plain, at + 4)
                    recs.append((ref << 32 | pos, plain[at:at + n]))
                    at += n
                want = sorted(recs, key=lambda r: r[0])
                sb, n_rec = sess.bamsort_pass(tags)
                assert (sb, n_rec) == (rb, len(recs))
                assert sess.bamsort_fetch(False, sb) == b"".join(r for _, r in want)
                keys, lens = sess.bamsort_index()
                assert keys == [k for k, _ in want] and lens == [len(r) for _, r in want]
                assert sess.truth_info() == info                  # the counts are the unsorted pass's
                t2 = sess.truth_tag_info()
                assert all(getattr(t2, f) == getattr(tag_info, f) for f, _ in t2._fields_)
                assert sess.fetch_truth(False, sb) == sess.bamsort_fetch(False, sb)
                with pytest.raises(simuscop_amd.SimuError, match="not compressed"):
                    sess.bamsort_fetch(True, 1)
                ties += len(keys) - len(set(keys))
                checked += len(keys)
                # an unsorted pass afterwards is what it was
                rb2, _ = sess.truth_bam(tags)
                assert rb2 == rb and sess.fetch_truth(False, rb) == plain
    assert checked > 2000 and ties > 0
