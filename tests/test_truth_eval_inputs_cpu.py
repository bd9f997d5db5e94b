"""The inputs of test_gpu_truth_eval_scale.py (eval_inputs.py) make what they are for, shown on eval_model without a GPU: the
sweep hits exactly the reachable cells, with counts that every listed index mistake moves; the names hold every shape of the
list, and a model that compares 253 bytes or forgets the mate gives another result; the duplicated read's run lies across
a block of 256 sorted keys (sg_eval_key is host code); the scale and long-record inputs cross the boundaries they aim at."""
import os
import struct

import bam_util as B
import eval_inputs as E
import eval_model as M

SCORE_LANES = 512 * 256   # sg_eval.hip: kScoreBlocks x kScoreThreads, the lanes of eval_score_kernel and eval_missing_kernel
BAM_BATCH = (16 << 20) + 65536   # host/input_stream.h: kBamBatch + kMaxMember, the bytes a reader's buffer is topped up to
B_SEGMENT = 16384         # sg::kBamSegment


def cell(mate, ci, mapq, cat):
    return ((mate * 3 + ci) * 256 + mapq) * 8 + cat


def flat(res, index=cell):
    """The result's table as the 12,288 cells, written through `index` (cells that fall outside are dropped, as a kernel's
    stray add would not show in the table either)."""
    out = [0] * 12288
    for (mate, cls, mapq), row in res["table"].items():
        for cat, v in enumerate(row):
            at = index(mate, M.CLASSES.index(cls), mapq, cat)
            if v and 0 <= at < len(out):
                out[at] += v
    return out


_sweep = {}


def sweep():
    if not _sweep:
        _sweep["streams"] = E.cell_sweep()
        _sweep["model"] = E.model_of(*_sweep["streams"])
    return _sweep


def test_sweep_hits_every_reachable_cell_and_no_other():
    want = sweep()["model"]
    cells = E.reachable_cells()
    assert len(cells) == 7168 == 2 * (2 * 6 + 2) * 256
    table = flat(want)
    expect = [0] * 12288
    for mate, ci, mapq, cat in cells:
        expect[cell(mate, ci, mapq, cat)] = E.sweep_count(mate, ci, cat, mapq)
    assert table == expect and sum(1 for v in table if v) == 7168
    assert 15000 < want["test_records"] < 21000


def test_sweep_counts_move_under_every_index_mistake():
    want = sweep()["model"]
    right = flat(want)
    wrong = dict(mate_and_class_strides_swapped=lambda m, c, q, k: ((c * 2 + m) * 256 + q) * 8 + k,
                 category_stride_7=lambda m, c, q, k: ((m * 3 + c) * 256 + q) * 7 + k,
                 mapq_stride_257=lambda m, c, q, k: ((m * 3 + c) * 257 + q) * 8 + k,
                 mapq_stride_255=lambda m, c, q, k: ((m * 3 + c) * 255 + q) * 8 + k,
                 mapq_off_by_one=lambda m, c, q, k: ((m * 3 + c) * 256 + (q + 1) % 256) * 8 + k,
                 class_order_reversed=lambda m, c, q, k: ((m * 3 + 2 - c) * 256 + q) * 8 + k,
                 mapq_and_category_swapped=lambda m, c, q, k: ((m * 3 + c) * 8 + k) * 256 + q)
    for label, index in wrong.items():
        moved = flat(want, index)
        assert sum(1 for a, b in zip(moved, right) if a != b) > 1000, label


def test_sweep_scalars_and_missing():
    want = sweep()["model"]
    assert want["missing"] == E.SWEEP_MISSING and len(set(want["missing"].values())) == 6 and min(want["missing"].values()) > 0
    for k in ("test_records", "secondary", "supplementary", "unknown", "ambiguous", "repeated", "truth_records", "truth_duplicates"):
        assert want[k] > 0, k
    assert (want["secondary"], want["supplementary"], want["unknown"], want["ambiguous"], want["repeated"], want["truth_duplicates"]) == (4, 5, 6, 3, 7, 2)


# ---- names ----
def name_fields(data):
    """[(offset of the name field, the field, flag)] of a stream's records."""
    return [(off + 36, r[36:36 + r[12]], struct.unpack_from("<H", r, 18)[0]) for off, r in B.parse_stream(data)[1]]


def test_names_hold_every_shape():
    n = E.name_shapes()
    s = n["shapes"]
    for side in ("truth", "test"):
        data = n[side]
        fields = name_fields(data)
        names = [f.split(b"\0")[0] for _, f, _ in fields]
        assert len(data) >= 40000
        assert {1 + 1, 2 + 1, 255, 1} <= {len(f) for _, f, _ in fields}                      # l_read_name of `a`, `bc`, 254 bytes, the empty name
        for key in ("one", "two", "first_a", "first_b", "last_1", "last_2", "prefix", "longer", "b01", "b7f", "b80", "bff", "mixed", "pair", "nomate",
                    "nul_truth", "nul_test", "dup", "nocigar", "span0", "cg"):
            assert s[key] in names, (side, key)
        assert names.count(b"") == 1 and [f for _, f, _ in fields if f.split(b"\0")[0] == b""] == [b"\0"]
        assert s["longer"].startswith(s["prefix"]) and s["first_a"][1:] == s["first_b"][1:] and s["last_1"][:-1] == s["last_2"][:-1]
        assert all(len(s[k]) == 254 for k in E.N254)
        # boundary segments that begin inside a name with bytes outside 33..126
        inside = [o for o, f, _ in fields if (o + len(f) - 1) // B_SEGMENT != (o - 1) // B_SEGMENT and any(c < 33 or c > 126 for c in f[:-1])]
        assert len(inside) >= 2, (side, inside)
        assert b"NM" in data and b"MDZ" in data and b"RGZlane" in data                     # aligner_tags
        assert b"CGBI" in data
    t_fields, q_fields = name_fields(n["truth"]), name_fields(n["test"])
    assert b"ab\0cd\0" in [f for _, f, _ in t_fields] and b"ab\0" in [f for _, f, _ in q_fields] and b"ab\0" not in [f for _, f, _ in t_fields]
    assert b"ef\0gh\0" in [f for _, f, _ in q_fields] and b"ef\0" in [f for _, f, _ in t_fields]
    assert sorted(fl & 0xC0 for _, f, fl in t_fields if f == b"pair\0") == [0x40, 0x80] and [fl for _, f, fl in t_fields if f == b"nomate\0"] == [0]
    assert [f for _, f, _ in t_fields].count(s["dup"] + b"\0") == 2
    tn, t = M.records(n["truth"])
    by = {a.name: a for a in t}
    assert (by[s["cg"]].cls, by[s["cg"]].span) == ("edited", 52) and by[s["cg"]].ops == [(50, 4), (52, 3)]
    assert (by[s["nocigar"]].span, by[s["nocigar"]].unmapped) == (1, False) and by[s["span0"]].span == 0 and by[s["span0"]].cls == "edited"


def retold(data, name=lambda nm: nm, flag=lambda f: f):
    """The stream with every record's name and flag passed through the two functions."""
    names, recs = B.parse_stream(data)
    out = [data[:recs[0][0]]]
    for _, r in recs:
        lname = r[12]
        nm = name(r[36:36 + lname].split(b"\0")[0]) + b"\0"
        body = r[4:12] + bytes([len(nm)]) + r[13:18] + struct.pack("<H", flag(struct.unpack_from("<H", r, 18)[0])) + r[20:36] + nm + r[36 + lname:]
        out.append(struct.pack("<I", len(body)) + body)
    return b"".join(out)


def test_names_tell_a_wrong_compare():
    n = E.name_shapes()
    want = E.model_of(n["truth"], n["test"])
    assert want["truth_duplicates"] == 2 and want["ambiguous"] == 1 and want["unknown"] == 3 and want["repeated"] == 0
    assert sum(want["missing"].values()) == 0
    scored = sum(sum(row) for row in want["table"].values())
    assert scored == want["truth_records"] - 2 == want["test_records"] - 4
    # the model joins `ab\0cd` with `ab` and `ef` with `ef\0gh`: with those reads taken out of the test file, two rows are missing
    qn, q = M.records(n["test"])
    tn, t = M.records(n["truth"])
    less = M.evaluate(tn, t, qn, [a for a in q if a.name not in (b"ab", b"ef")])
    assert sum(less["missing"].values()) == 2 and less["unknown"] == want["unknown"]
    # 253 bytes compared: last_1 and last_2 are one read, held twice
    short = E.model_of(retold(n["truth"], name=lambda nm: nm[:253]), retold(n["test"], name=lambda nm: nm[:253]))
    assert short["table"] != want["table"] and short["truth_duplicates"] > want["truth_duplicates"] and short["unknown"] < want["unknown"]
    # the mate ignored: `pair` is held twice, the stranger on mate 1 finds `nomate`
    no_mate = E.model_of(retold(n["truth"], flag=lambda f: f & ~0x80), retold(n["test"], flag=lambda f: f & ~0x80))
    assert no_mate["table"] != want["table"] and no_mate["truth_duplicates"] == 4 and no_mate["unknown"] == want["unknown"] - 1
    # the length in 7 bits, or the first byte skipped: other results too
    assert E.model_of(retold(n["truth"], name=lambda nm: nm[1:]), retold(n["test"], name=lambda nm: nm[1:])) != want


# ---- duplicated reads ----
def test_dup_runs_straddle_a_block_of_the_sort():
    for bits in (1, 4, 64):
        d = E.dup_runs(bits)
        reads = d["reads"]
        pos, keys = E.sorted_positions(reads, bits)
        at = sorted(pos[i] for i, r in enumerate(reads) if r[0] == d["big"])
        assert len(at) == 65 and at[0] // 256 != at[-1] // 256, (bits, at[0], at[-1])
        assert len({keys[i] for i, r in enumerate(reads) if r[0] == d["big"]}) == 1
        held = {}
        for r in reads:
            held[(r[0], r[1] & 0x80)] = held.get((r[0], r[1] & 0x80), 0) + 1
        assert sorted(set(held.values())) == [1, 2, 3, 65]
        if bits == 64:
            assert at == list(range(at[0], at[0] + 65))          # no other read has the key
        if bits == 1:
            big_key = keys[[r[0] for r in reads].index(d["big"])]
            between = [i for i, r in enumerate(reads) if held[(r[0], r[1] & 0x80)] == 1 and keys[i] == big_key and at[0] < pos[i] < at[-1]]
            assert between                                         # a read held once inside the run of equal keys
        want = E.model_of(d["truth"], d["test"])
        c = d["counts"]
        for k in ("truth_records", "truth_duplicates", "ambiguous", "test_records", "unknown", "repeated", "secondary", "supplementary"):
            assert want[k] == c[k], (bits, k)
        assert sum(want["missing"].values()) == c["missing"] and sum(sum(r) for r in want["table"].values()) == c["scored"]


def test_identical_truth():
    want = E.model_of(*E.identical_truth())
    assert want["truth_records"] == want["truth_duplicates"] == 300 and want["ambiguous"] == want["test_records"] == 5
    assert not want["table"] and not any(want["missing"].values())


# ---- scale ----
def test_scale_is_beyond_one_launch():
    truth, test = E.minimal_records(140000)
    assert len(truth) > SCORE_LANES and len(test) > SCORE_LANES
    t_stream = E.stream(E.REFS, E.pack(truth[:2000]))
    assert 44 <= (len(t_stream) - 100) / 2000 <= 56              # about 52 bytes a record
    cats = {}
    for q in test[:20000]:
        cats[q[1] & 0x904] = cats.get(q[1] & 0x904, 0) + 1
    assert {0, 4, 0x100, 0x800} <= set(cats)
    # the records of one call follow from where the members are cut: 40 members of 65,280 bytes hold about 50,000 records,
    # all members more than a launch
    q_stream = E.stream(E.TEST_REFS, E.pack(test))
    offs = [o for o, _ in B.parse_stream(q_stream)[1]]
    per_call = [sum(1 for o in offs if a <= o < a + 40 * 65280) for a in range(0, len(q_stream), 40 * 65280)]
    assert sum(per_call) == len(test) and len(per_call) >= 3 and max(per_call) < SCORE_LANES < len(offs)


# ---- long records ----
def test_long_records_fill_three_batches(tmp_path):
    d = E.long_records(1200, 20000)
    for side in ("truth", "test"):
        data = d[side]
        f = B.bgzf(data, level=0)
        assert len(f) > 2 * (16 << 20)
        bt = E.batches(f, BAM_BATCH)
        assert len(bt) >= 3 and sum(b[1] for b in bt) == len(f) and sum(b[3] for b in bt) == len(data)
        recs = B.parse_stream(data)[1]
        starts = {o for o, _ in recs}
        assert any(b[2] not in starts for b in bt[1:])            # a batch begins inside a record
        if side == "test":
            at = [i for i, (o, r) in enumerate(recs) if r[36:36 + r[12] - 1] == d["twice"]]
            assert len(at) == 2 and at[0] < len(recs) // 3 and at[1] > 2 * len(recs) // 3
            first_batch = [i for i, b in enumerate(bt) if b[2] <= recs[at[0]][0] < b[2] + b[3]]
            last_batch = [i for i, b in enumerate(bt) if b[2] <= recs[at[1]][0] < b[2] + b[3]]
            assert first_batch == [0] and last_batch == [len(bt) - 1]
    want = E.model_of(d["truth"], d["test"])
    assert want["repeated"] == 1 and want["truth_records"] == 1200 and sum(want["missing"].values()) == 0


def test_big_header_covers_three_members():
    t, q = E.identical_truth()
    for data in (t, q, B.header(E.REFS, E.TEXT)):
        big = E.big_header(data)
        names, recs = B.parse_stream(big)
        end = recs[0][0] if recs else len(big)
        assert end >= 3 * 65280 and names == B.parse_stream(data)[0]
        assert [r for _, r in recs] == [r for _, r in B.parse_stream(data)[1]]


def test_readme_lists_the_files():
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "README.md")).read()
    for name in ("eval_model.py", "test_truth_eval_cpu.py", "test_gpu_truth_eval.py", "eval_inputs.py", "test_truth_eval_inputs_cpu.py",
                 "test_gpu_truth_eval_scale.py"):
        assert "`%s`" % name in text, name
