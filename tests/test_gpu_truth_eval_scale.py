"""truthEval on the MI355X, second round (the inputs: eval_inputs.py; what each is for: test_truth_eval_inputs_cpu.py), every
result exactly eval_model's: more records in one call and more truth rows than eval_score_kernel / eval_missing_kernel have
lanes; every reachable cell of the table through the ABI and through eval.tsv; the radix sort at 1, 2, 3, 4, 5, 7 and 8
passes with keys that end inside a digit; names of 0, 1, 2 and 254 bytes, prefixes, bytes outside 33..126, an embedded NUL;
runs of duplicated reads across the sort's blocks; files without records and a truth of one record; the refID map the
command line makes of two different @SQ lists, headers of several members, no EOF member; files of three batches of the
command line; and the session's stages call by call."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import bam_util as B
import eval_inputs as E
import eval_model as M
import simuscop_amd
from simuscop_amd import build
from test_gpu_truth_eval import calls_of, engine, header_bytes, model

pytestmark = pytest.mark.gpu

EXE = os.path.join(build.LIBDIR, "truthEval")
SCORE_LANES = 512 * 256          # sg_eval.hip: kScoreBlocks x kScoreThreads; a launch of eval_score_kernel / eval_missing_kernel has no more lanes
SORT_TILE = 1024                 # sg::kSortTile (sg_bamsort.h): keys of one sort block
BAM_BATCH = (16 << 20) + 65536   # host/input_stream.h: kBamBatch + kMaxMember, what one batch of the command line holds at most
SG_ERR_INVALID, SG_ERR_OVERFLOW = 1, 4


@pytest.fixture(scope="module")
def ctx():
    lib = simuscop_amd.load_engine()
    c = C.c_void_p()
    assert lib.sg_create(C.byref(c), 0, 1) == 0
    yield c
    lib.sg_destroy(c)


def command(tmp_path, truth_file, test_file, *flags, to_file=True, label="x"):
    """One run of the command line -> (eval.tsv's bytes, stderr)."""
    tp, qp, out = str(tmp_path / (label + ".truth.bam")), str(tmp_path / (label + ".test.bam")), str(tmp_path / (label + ".tsv"))
    open(tp, "wb").write(truth_file)
    open(qp, "wb").write(test_file)
    args = [EXE, "--truth", tp, "--bam", qp, "--quiet", *flags] + (["--out", out] if to_file else [])
    r = subprocess.run(args, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return (open(out, "rb").read() if to_file else r.stdout), r.stderr.decode(errors="replace")


def total(res):
    return sum(sum(row) for row in res["table"].values())


# ---- 1. one call beyond the grid ----
def test_one_call_beyond_the_grid(ctx):
    truth, test = E.minimal_records(140000)
    t_stream, q_stream = E.stream(E.REFS, E.pack(truth)), E.stream(E.TEST_REFS, E.pack(test))
    want = E.model_of(t_stream, q_stream)
    assert len(truth) > SCORE_LANES and len(test) > SCORE_LANES      # one call's records, and the truth's rows: the grid-stride loops go round
    assert len(truth) > 100 * SORT_TILE
    assert want["repeated"] > 100 and sum(want["missing"].values()) > 1000 and len(want["table"]) == 6 * 256
    tf, qf = B.bgzf(t_stream, level=1), B.bgzf(q_stream, level=1)
    assert len(calls_of(qf, 40)) >= 3
    whole = engine(ctx, tf, qf, feed="all")
    assert whole == want
    assert engine(ctx, tf, qf, feed=40) == whole


# ---- 2. every cell ----
_sweep = {}


def sweep():
    if not _sweep:
        _sweep["streams"] = E.cell_sweep()
        _sweep["model"] = E.model_of(*_sweep["streams"])
        for member in (997, 65280):
            _sweep[member] = tuple(B.bgzf(s, member=member, level=1) for s in _sweep["streams"])
        assert model(*_sweep[65280]) == _sweep["model"]
    return _sweep


@pytest.mark.parametrize("feed", ["all", 1])
def test_every_cell(ctx, feed):
    s = sweep()
    assert sum(1 for row in s["model"]["table"].values() for v in row if v) == 7168
    assert engine(ctx, *s[997], feed=feed) == s["model"]


def test_every_cell_in_the_tsv(tmp_path):
    s = sweep()
    text, _ = command(tmp_path, *s[65280])
    assert text == M.tsv(s["model"])
    assert text.count(b"#M\t") == 2 * 3 * 256 and text.count(b"#X\t") == 6 and text.count(b"#R\t") == 256


# ---- 3. radix passes ----
@pytest.mark.parametrize("key_bits", [8, 9, 16, 17, 24, 33, 56, 63])
def test_radix_passes(ctx, key_bits):
    s = sweep()
    if "bits64" not in s:
        s["bits64"] = engine(ctx, *s[65280], key_bits=64)
    assert s["model"]["truth_records"] > 8 * SORT_TILE
    assert engine(ctx, *s[65280], key_bits=key_bits) == s["bits64"] == s["model"]


# ---- 4. names ----
_names = {}


def names():
    if not _names:
        _names.update(E.name_shapes())
        _names["model"] = model(B.bgzf(_names["truth"]), B.bgzf(_names["test"]))
    return _names


@pytest.mark.parametrize("key_bits", [64, 4])
def test_names(ctx, key_bits):
    n = names()
    whole = (B.bgzf(n["truth"]), B.bgzf(n["test"]))
    small = (B.bgzf(n["truth"], member=997), B.bgzf(n["test"], member=997))
    assert engine(ctx, *whole, key_bits=key_bits) == n["model"]
    assert engine(ctx, *small, feed=3, key_bits=key_bits) == n["model"]


def test_names_through_the_command_line(tmp_path):
    n = names()
    text, _ = command(tmp_path, B.bgzf(n["truth"]), B.bgzf(n["test"], member=4000))
    assert text == M.tsv(n["model"])


# ---- 5. duplicated reads ----
@pytest.mark.parametrize("key_bits", [1, 4, 64])
def test_duplicate_runs(ctx, key_bits):
    d = E.dup_runs(key_bits)
    want = E.model_of(d["truth"], d["test"])
    assert want["truth_duplicates"] == d["counts"]["truth_duplicates"] == 86 and want["ambiguous"] == 11
    got = engine(ctx, B.bgzf(d["truth"]), B.bgzf(d["test"]), key_bits=key_bits)    # (engine() compares sg_eval_truth_done's *duplicates with the counts)
    assert got == want


def test_a_truth_of_identical_records(ctx):
    t, q = E.identical_truth()
    want = E.model_of(t, q)
    assert want["truth_duplicates"] == 300 and want["ambiguous"] == 5 and not want["table"] and not any(want["missing"].values())
    for bits in (64, 1):
        assert engine(ctx, B.bgzf(t), B.bgzf(q), key_bits=bits) == want


# ---- 6. empty and tiny ----
def tiny_cases():
    few_t = [E.truth_read(b"t%d" % i, i & 1, ("plain", "edited", "unmapped")[i % 3], i) for i in range(9)]
    few_q = [E.answer(t, "exact" if not t[1] & 4 else "invented", 30 + i, i) for i, t in enumerate(few_t)]
    one = E.truth_read(b"only", 0, "edited", 5)
    unmapped_only = [E.answer(t, "lost" if not t[1] & 4 else "both_unmapped", 0, i) for i, t in enumerate(few_t)]
    empty_t, empty_q = E.stream(E.REFS, []), E.stream(E.TEST_REFS, [])
    return dict(no_truth=(empty_t, E.stream(E.TEST_REFS, E.pack(few_q))),
                no_test=(E.stream(E.REFS, E.pack(few_t)), empty_q),
                neither=(empty_t, empty_q),
                one_row=(E.stream(E.REFS, E.pack([one])), E.stream(E.TEST_REFS, E.pack([E.answer(one, "near", 44), E.answer(one, "exact", 60)]))),
                no_sq=(E.stream(E.REFS, E.pack(few_t)), E.stream([], E.pack(unmapped_only))))


TINY = ["no_truth", "no_test", "neither", "one_row", "no_sq"]


def tiny_expectations(label, want):
    if label == "no_truth":
        assert want["unknown"] == want["test_records"] == 9 and want["truth_records"] == 0 and not want["table"]
    if label == "no_test":
        assert sum(want["missing"].values()) == want["truth_records"] == 9 and want["test_records"] == 0 and not want["table"]
    if label == "neither":
        assert want["truth_records"] == want["test_records"] == 0
    if label == "one_row":
        assert want["repeated"] == 1 and want["table"] == {(0, "edited", 44): [0, 1, 0, 0, 0, 0, 0, 0]}
    if label == "no_sq":
        assert total(want) == 9 and all(row[5] + row[7] == sum(row) for row in want["table"].values())


@pytest.mark.parametrize("label", TINY)
def test_empty_and_tiny(ctx, label):
    t, q = tiny_cases()[label]
    want = E.model_of(t, q)
    tiny_expectations(label, want)
    assert engine(ctx, B.bgzf(t), B.bgzf(q)) == want
    assert engine(ctx, B.bgzf(t, member=50), B.bgzf(q, member=50), feed=1, key_bits=1) == want


@pytest.mark.parametrize("label", TINY)
def test_empty_and_tiny_through_the_command_line(tmp_path, label):
    t, q = tiny_cases()[label]
    text, _ = command(tmp_path, B.bgzf(t), B.bgzf(q))
    assert text == M.tsv(E.model_of(t, q))


# ---- 7. the refID map the host makes ----
MAP_TRUTH_REFS = [(b"chrA", 500000), (b"chrB", 300000), (b"chrC", 100000), (b"chrA", 500000), (b"chrT", 9000)]   # chrA twice; chrT: the test lacks it
MAP_TEST_REFS = [(b"chrZ", 700000), (b"chrC", 100000), (b"chrB", 300000), (b"chrB", 300000), (b"chrA", 500000)]   # another order; chrB twice; chrZ
_refmap = {}


def refmap_case():
    """Truth reads on all five of the truth's entries, each answered from every one of the test's five entries at a shift of
    0, 1, 47 or 60 bases: exact, near, near only at --min-overlap 1, or wrong_place where the names meet (the first entry of a name held twice), wrong_contig
    where they do not."""
    if not _refmap:
        truth, test = [], []
        for k in range(600):
            t = E.truth_read(b"map%d" % k, k & 1, ("plain", "edited")[k % 2], k)
            t = t[:2] + (k % 5,) + t[3:]
            truth.append(t)
            test.append((t[0], t[1], (k // 5) % 5, t[3] + (0, 1, 47, 60)[k % 4], (k * 11) % 256, t[5]))
        _refmap["streams"] = (E.stream(MAP_TRUTH_REFS, E.pack(truth)), E.stream(MAP_TEST_REFS, E.pack(test)))
        _refmap["model"] = {pct: E.model_of(*_refmap["streams"], pct=pct) for pct in (1, 10, 100)}
    return _refmap


def test_refmap_inputs_meet_and_miss():
    c = refmap_case()
    cats = [sum(row[i] for row in c["model"][10]["table"].values()) for i in range(8)]
    assert cats[0] > 20 and cats[1] > 20 and cats[2] > 20 and cats[4] > 100 and sum(cats) == 600
    tn, t = M.records(c["streams"][0])
    qn, q = M.records(c["streams"][1])
    # the truth's second chrA holds reads that the test's chrA (the first chrA by name) does not meet; the test's second chrB meets chrB
    assert any(a.ref == 3 and b.ref == 4 for a, b in zip(t, q)) and any(a.ref == 1 and b.ref == 3 and a.pos == b.pos and a.name == b.name for a, b in zip(t, q))
    assert len({M.tsv(c["model"][pct], pct) for pct in (1, 10, 100)}) == 3


@pytest.mark.parametrize("big", ["neither", "truth", "test", "both"])
def test_refmap_of_the_command_line(tmp_path, big):
    c = refmap_case()
    t, q = c["streams"]
    if big in ("truth", "both"):
        t = E.big_header(t)
    if big in ("test", "both"):
        q = E.big_header(q)
    tf, qf = B.bgzf(t), B.bgzf(q)
    assert (len(B.members(tf)[0]) > 4) == (big in ("truth", "both")) and (len(B.members(qf)[0]) > 4) == (big in ("test", "both"))
    text, err = command(tmp_path, tf, qf)
    assert text == M.tsv(c["model"][10]) and "EOF marker" not in err


def test_refmap_without_the_eof_member(tmp_path):
    c = refmap_case()
    text, err = command(tmp_path, B.bgzf(c["streams"][0], eof=False), B.bgzf(c["streams"][1], eof=False))
    assert text == M.tsv(c["model"][10]) and err.count("EOF marker is absent") == 2


@pytest.mark.parametrize("pct", [1, 100])
def test_refmap_other_overlaps(tmp_path, pct):
    c = refmap_case()
    text, _ = command(tmp_path, B.bgzf(c["streams"][0]), B.bgzf(c["streams"][1]), "--min-overlap", str(pct))
    assert text == M.tsv(c["model"][pct], pct) != M.tsv(c["model"][10], pct)


def test_refmap_to_standard_output(tmp_path):
    c = refmap_case()
    text, _ = command(tmp_path, B.bgzf(c["streams"][0]), B.bgzf(c["streams"][1]), to_file=False)
    assert text == M.tsv(c["model"][10]) and not os.path.exists(str(tmp_path / "x.tsv"))


# ---- 8. batches of the command line ----
def test_files_of_three_batches(tmp_path):
    d = E.long_records(1200, 20000)
    want = E.model_of(d["truth"], d["test"])
    files = {}
    for side in ("truth", "test"):
        f = files[side] = B.bgzf(d[side], level=0)
        bt = E.batches(f, BAM_BATCH)
        assert len(f) > 2 * (16 << 20) and len(bt) >= 3
        starts = {o for o, _ in B.parse_stream(d[side])[1]}
        assert all(b[2] not in starts for b in bt[1:])            # every later batch begins inside a record
    recs = B.parse_stream(d["test"])[1]
    at = [o for o, r in recs if r[36:36 + r[12] - 1] == d["twice"]]
    bt = E.batches(files["test"], BAM_BATCH)
    assert len(at) == 2 and at[0] < bt[0][3] and at[1] >= bt[-1][2]   # its primaries: in the first and in the last batch
    assert want["repeated"] == 1 and want["table"][(0, "plain", 4 * 13)][4] >= 1   # the first one is scored: wrong_contig at its MAPQ
    outs = [command(tmp_path, files["truth"], files["test"], label="run%d" % i)[0] for i in range(2)]
    assert outs[0] == outs[1] == M.tsv(want)


# ---- 9. the session's stages ----
def small_pair():
    t = [E.truth_read(b"st%d" % i, i & 1, ("plain", "edited", "unmapped")[i % 3], i) for i in range(40)]
    q = [E.answer(r, "exact" if not r[1] & 4 else "both_unmapped", 10 + i, i) for i, r in enumerate(t[:30])]
    return E.stream(E.REFS, E.pack(t)), E.stream(E.TEST_REFS, E.pack(q))


def result_of(table, counts):
    res = dict(table={}, missing={})
    for mate in (0, 1):
        for ci, cls in enumerate(M.CLASSES):
            res["missing"][(mate, cls)] = counts.missing[mate * 3 + ci]
            for mapq in range(256):
                at = ((mate * 3 + ci) * 256 + mapq) * 8
                if any(table[at:at + 8]):
                    res["table"][(mate, cls, mapq)] = list(table[at:at + 8])
    for k in ("test_records", "secondary", "supplementary", "unknown", "ambiguous", "repeated", "truth_records", "truth_duplicates"):
        res[k] = getattr(counts, k)
    return res


def test_stages(ctx):
    lib = simuscop_amd.load_engine()
    t, q = small_pair()
    want = E.model_of(t, q)
    tf, qf = B.bgzf(t), B.bgzf(q)
    n_ref, skip = header_bytes(t)
    q_ref, q_skip = header_bytes(q)
    ident = (C.c_int32 * q_ref)(0, 1, 2, -1)
    table, counts = (C.c_uint64 * simuscop_amd.SG_EVAL_CELLS)(), simuscop_amd.SgEvalCounts()

    def refused(rc, text, code=SG_ERR_INVALID):
        assert rc == code and text in lib.sg_last_error(ctx).decode(), (rc, lib.sg_last_error(ctx))

    def ok(rc):
        assert rc == 0, lib.sg_last_error(ctx).decode()
    lib.sg_eval_end(ctx)
    lib.sg_eval_end(ctx)                                           # no session: nothing to end, twice
    # before sg_eval_begin
    refused(lib.sg_eval_truth_bgzf(ctx, tf, len(tf)), "sg_eval_truth_bgzf: call sg_eval_begin first")
    refused(lib.sg_eval_truth_done(ctx, None, None), "sg_eval_truth_done: call sg_eval_begin first")
    refused(lib.sg_eval_test_refmap(ctx, ident, q_ref, q_skip), "sg_eval_test_refmap: call sg_eval_truth_done first")
    refused(lib.sg_eval_test_bgzf(ctx, qf, len(qf)), "sg_eval_test_bgzf: call sg_eval_test_refmap first")
    refused(lib.sg_eval_finish(ctx, table, len(table), C.byref(counts)), "sg_eval_finish: call sg_eval_test_refmap and feed the test file first")
    try:
        ok(lib.sg_eval_begin(ctx, n_ref, 64, 10, skip))
        refused(lib.sg_eval_test_refmap(ctx, ident, q_ref, q_skip), "sg_eval_test_refmap: call sg_eval_truth_done first")
        refused(lib.sg_eval_finish(ctx, table, len(table), C.byref(counts)), "sg_eval_finish: call sg_eval_test_refmap")
        ok(lib.sg_eval_truth_bgzf(ctx, tf, len(tf)))
        # a new session in the middle of one: clean, and its result is the model's
        ok(lib.sg_eval_begin(ctx, n_ref, 64, 10, skip))
        ok(lib.sg_eval_truth_bgzf(ctx, tf, len(tf)))
        ok(lib.sg_eval_truth_bgzf(ctx, None, 0))
        refused(lib.sg_eval_test_bgzf(ctx, qf, len(qf)), "sg_eval_test_bgzf: call sg_eval_test_refmap first")
        n_truth, n_dup = C.c_uint64(), C.c_uint64()
        ok(lib.sg_eval_truth_done(ctx, C.byref(n_truth), C.byref(n_dup)))
        assert (n_truth.value, n_dup.value) == (40, 0)
        refused(lib.sg_eval_truth_bgzf(ctx, tf, len(tf)), "feed the truth before sg_eval_truth_done")
        refused(lib.sg_eval_truth_done(ctx, None, None), "sg_eval_truth_done: call sg_eval_begin first, once")
        refused(lib.sg_eval_test_bgzf(ctx, qf, len(qf)), "sg_eval_test_bgzf: call sg_eval_test_refmap first")
        refused(lib.sg_eval_test_refmap(ctx, (C.c_int32 * q_ref)(0, 1, n_ref, -1), q_ref, q_skip), "sg_eval_test_refmap: entry 2 names no truth reference")
        refused(lib.sg_eval_test_refmap(ctx, (C.c_int32 * q_ref)(0, 1, 2, -2), q_ref, q_skip), "sg_eval_test_refmap: entry 3 names no truth reference")
        ok(lib.sg_eval_test_refmap(ctx, ident, q_ref, q_skip))
        # finish with no test member fed: every row is missing, twice the same
        nothing = []
        for _ in range(2):
            ok(lib.sg_eval_finish(ctx, table, len(table), C.byref(counts)))
            nothing.append(result_of(table, counts))
        assert nothing[0] == nothing[1] == E.model_of(t, E.stream(E.TEST_REFS, []))
        assert sum(nothing[0]["missing"].values()) == 40
        # the whole session; finish twice
        ok(lib.sg_eval_begin(ctx, n_ref, 64, 10, skip))
        ok(lib.sg_eval_truth_bgzf(ctx, tf, len(tf)))
        ok(lib.sg_eval_truth_bgzf(ctx, None, 0))
        ok(lib.sg_eval_truth_done(ctx, None, None))
        ok(lib.sg_eval_test_refmap(ctx, ident, q_ref, q_skip))
        ok(lib.sg_eval_test_bgzf(ctx, qf, len(qf)))
        ok(lib.sg_eval_test_bgzf(ctx, None, 0))
        refused(lib.sg_eval_finish(ctx, table, simuscop_amd.SG_EVAL_CELLS - 1, C.byref(counts)), "sg_eval_finish: the table holds SG_EVAL_CELLS cells", SG_ERR_OVERFLOW)
        both = []
        for _ in range(2):
            ok(lib.sg_eval_finish(ctx, table, len(table), C.byref(counts)))
            both.append(result_of(table, counts))
        assert both[0] == both[1] == want and sum(want["missing"].values()) == 10
    finally:
        lib.sg_eval_end(ctx)
        lib.sg_eval_end(ctx)
    refused(lib.sg_eval_finish(ctx, table, len(table), C.byref(counts)), "sg_eval_finish: call sg_eval_test_refmap")
    assert engine(ctx, tf, qf) == want


def test_a_reference_id_outside_the_test_header(ctx):
    """A test record with refID = n_ref of its own header: the call that brings it is refused at the record's offset, the
    session has failed, and the context takes the next session."""
    lib = simuscop_amd.load_engine()
    t, q = small_pair()
    want = E.model_of(t, q)
    n_ref, skip = header_bytes(t)
    q_ref, q_skip = header_bytes(q)
    off, r = B.parse_stream(q)[1][17]
    bad = q[:off + 4] + struct.pack("<i", q_ref) + q[off + 8:]
    tf, qf, bf = B.bgzf(t), B.bgzf(q), B.bgzf(bad)
    table, counts = (C.c_uint64 * simuscop_amd.SG_EVAL_CELLS)(), simuscop_amd.SgEvalCounts()
    assert lib.sg_eval_begin(ctx, n_ref, 64, 10, skip) == 0
    try:
        assert lib.sg_eval_truth_bgzf(ctx, tf, len(tf)) == 0 and lib.sg_eval_truth_bgzf(ctx, None, 0) == 0
        assert lib.sg_eval_truth_done(ctx, None, None) == 0
        assert lib.sg_eval_test_refmap(ctx, (C.c_int32 * q_ref)(0, 1, 2, -1), q_ref, q_skip) == 0
        assert lib.sg_eval_test_bgzf(ctx, bf, len(bf)) == SG_ERR_INVALID
        said = lib.sg_last_error(ctx).decode()
        assert "decompressed offset %d: reference id outside the header's list" % off in said, said
        for rc in (lib.sg_eval_test_bgzf(ctx, qf, len(qf)), lib.sg_eval_finish(ctx, table, len(table), C.byref(counts))):
            assert rc == SG_ERR_INVALID and "the session has failed" in lib.sg_last_error(ctx).decode()
    finally:
        lib.sg_eval_end(ctx)
    assert engine(ctx, tf, qf) == want
