"""truthEval on the MI355X (sg_eval_*, simuscop_amd/csrc/sg_eval.hip; the command line simuscop_amd/lib/truthEval) against
eval_model, the plain-Python statement of the rule: a crafted join with every category, class and scalar count, written
with members of 997 and 65,280 bytes and fed one member per call and all in one call; the same with 4-bit keys, where every
look-up walks a long run of colliding names; duplicates in the truth next to a colliding distinct name; repeated primaries
within one feed call and across calls; the closed loop simuReads --truth-bam -> truthEval through the command lines; and
malformed test files, which end with the offset, a non-zero exit and no output file."""
import ctypes as C
import os
import random
import struct
import subprocess

import pytest

import bam_util as B
import cases
import eval_model as M
import simuscop_amd
from simuscop_amd import build

pytestmark = pytest.mark.gpu

EXE = os.path.join(build.LIBDIR, "truthEval")
SIMU = os.path.join(build.LIBDIR, "simuReads")
SEED = (cases.FAKE_SEC << 32) | cases.FAKE_NSEC
L = 150
TRUTH_REFS = [(b"chrA", 500000), (b"chrB", 300000), (b"chrC", 100000)]
TEST_REFS = [(b"chrZ", 700000), (b"chrC", 100000), (b"chrA", 500000), (b"chrB", 300000)]   # another order, one contig the truth lacks
B_SEGMENT = 16384   # sg::kBamSegment: the boundary search's segment
EDITED = [b"60M2D90M", b"30M1I119M", b"10S140M", b"70M500N80M", b"75=1X74=", b"50M3D40M2I58M"]


@pytest.fixture(scope="module")
def ctx():
    lib = simuscop_amd.load_engine()
    c = C.c_void_p()
    assert lib.sg_create(C.byref(c), 0, 1) == 0
    yield c
    lib.sg_destroy(c)


# ---- the engine through the ABI ----
def header_bytes(stream):
    l_text = struct.unpack_from("<i", stream, 4)[0]
    q = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, q)[0]
    q += 4
    for _ in range(n_ref):
        q += 8 + struct.unpack_from("<i", stream, q)[0]
    return n_ref, q


def calls_of(buf, feed):
    """The feed calls of a file: "all" in one call; N: N members per call."""
    if feed == "all":
        return [buf]
    mem, whole = B.members(buf)
    assert whole == len(buf)
    starts = [m[0] for m in mem][::feed] + [len(buf)]
    return [buf[a:b] for a, b in zip(starts, starts[1:])]


def engine(ctx, truth_file, test_file, feed="all", key_bits=64, pct=10, truth_feed=None):
    """-> the result in eval_model.evaluate's form."""
    lib = simuscop_amd.load_engine()

    def ok(rc):
        assert rc == 0, lib.sg_last_error(ctx).decode()
    t_stream, q_stream = B.inflate(truth_file), B.inflate(test_file)
    t_names, q_names = M.records(t_stream[:header_bytes(t_stream)[1]])[0], M.records(q_stream[:header_bytes(q_stream)[1]])[0]
    n_ref, skip = header_bytes(t_stream)
    ok(lib.sg_eval_begin(ctx, n_ref, key_bits, pct, skip))
    try:
        for part in calls_of(truth_file, truth_feed or feed):
            ok(lib.sg_eval_truth_bgzf(ctx, part, len(part)))
        ok(lib.sg_eval_truth_bgzf(ctx, None, 0))
        n_truth, n_dup = C.c_uint64(), C.c_uint64()
        ok(lib.sg_eval_truth_done(ctx, C.byref(n_truth), C.byref(n_dup)))
        ids = {}
        for i, n in enumerate(t_names):
            ids.setdefault(n, i)
        refmap = (C.c_int32 * max(1, len(q_names)))(*[ids.get(n, -1) for n in q_names])
        ok(lib.sg_eval_test_refmap(ctx, refmap, len(q_names), header_bytes(q_stream)[1]))
        for part in calls_of(test_file, feed):
            ok(lib.sg_eval_test_bgzf(ctx, part, len(part)))
        ok(lib.sg_eval_test_bgzf(ctx, None, 0))
        table = (C.c_uint64 * simuscop_amd.SG_EVAL_CELLS)()
        counts = simuscop_amd.SgEvalCounts()
        ok(lib.sg_eval_finish(ctx, table, len(table), C.byref(counts)))
    finally:
        lib.sg_eval_end(ctx)
    assert (n_truth.value, n_dup.value) == (counts.truth_records, counts.truth_duplicates)
    assert (counts.truth_bytes, counts.test_bytes) == (len(t_stream), len(q_stream))
    res = dict(table={}, missing={})
    for mate in (0, 1):
        for ci, cls in enumerate(M.CLASSES):
            res["missing"][(mate, cls)] = counts.missing[mate * 3 + ci]
            for mapq in range(256):
                at = ((mate * 3 + ci) * 256 + mapq) * 8
                row = list(table[at:at + 8])
                if any(row):
                    res["table"][(mate, cls, mapq)] = row
    for k in ("test_records", "secondary", "supplementary", "unknown", "ambiguous", "repeated", "truth_records", "truth_duplicates"):
        res[k] = getattr(counts, k)
    return res


def model(truth_file, test_file, pct=10):
    tn, t = M.records(B.inflate(truth_file))
    qn, q = M.records(B.inflate(test_file))
    return M.evaluate(tn, t, qn, q, pct)


def totals(res):
    return [sum(row[c] for row in res["table"].values()) for c in range(8)]


# ---- crafted files ----
def sam(name, flag, rname, pos, mapq, cigar, rng):
    seq = bytes(rng.choice(b"ACGT") for _ in range(L))
    return b"\t".join([name, b"%d" % flag, rname, b"%d" % pos, b"%d" % mapq, cigar, b"*", b"0", b"0", seq, b"I" * L])


def truth_lines(rng, n_pairs=600, prefix=b"sim"):
    """Pairs on three contigs: plain, edited and unmapped reads (some of those placed at their mate)."""
    lines = []
    for i in range(n_pairs):
        name = b"%s#%s#%d%%2#%d" % (prefix, rng.choice((b"A", b"B", b"C")), rng.randrange(1, 90000), i)
        for mate in (0, 1):
            flag = 1 | (0x40, 0x80)[mate] | (0x10 if rng.random() < 0.5 else 0)
            ref, pos = rng.choice(TRUTH_REFS)[0], rng.randrange(1, 90000)
            u = rng.random()
            if u < 0.06:
                lines.append(sam(name, flag | 4, b"*", 0, 0, b"*", rng))
            elif u < 0.10:
                lines.append(sam(name, flag | 4, ref, pos, 0, b"*", rng))
            elif u < 0.45:
                lines.append(sam(name, flag, ref, pos, 60, rng.choice(EDITED), rng))
            else:
                lines.append(sam(name, flag, ref, pos, 60, b"%dM" % L, rng))
    return lines


def fields(line):
    f = line.split(b"\t")
    return f[0], int(f[1]), f[2], int(f[3]), f[5]


def span_of(cigar):
    return sum(n for n, op in B.parse_cigar(cigar) if op in M.REF_OPS) if cigar != b"*" else 1


def derived_test_lines(rng, truth):
    """What an aligner might have made of the truth's reads: every category, the scalar counts, shuffled."""
    out = []
    for ln in truth:
        name, flag, rname, pos, cigar = fields(ln)
        mapq = rng.choice((0, 1, 59, 60, 255))
        u = rng.random()
        if u < 0.03:
            continue                                                           # dropped: `missing`
        if flag & 4:
            if u < 0.5:
                out.append(sam(name, flag, b"*", 0, 0, b"*", rng))             # both_unmapped
            else:
                out.append(sam(name, flag & ~4, rng.choice(TEST_REFS)[0], rng.randrange(1, 90000), mapq, b"%dM" % L, rng))   # invented
            continue
        span = span_of(cigar)
        if u < 0.40:
            q = (flag, rname, pos, cigar)                                      # exact
        elif u < 0.60:
            q = (flag, rname, pos + rng.choice((1, span - 1, span, span + 7, -1, -(L - 1), -L, 14, 135, 136)), b"%dM" % L)
        elif u < 0.68:
            q = (flag, rname, pos, rng.choice(EDITED + [b"%dM" % L, b"%dM" % (L - 1), b"1M"]))   # same start, maybe another end
        elif u < 0.76:
            q = (flag ^ 0x10, rname, pos, cigar)
        elif u < 0.84:
            q = (flag, rng.choice([r for r, _ in TRUTH_REFS if r != rname]), pos, cigar)
        elif u < 0.88:
            q = (flag, b"chrZ", pos, cigar)
        else:
            q = (flag | 4, rng.choice((b"*", rname)), pos, b"*")               # lost
        out.append(sam(name, q[0], q[1], max(1, q[2]) if q[1] != b"*" else 0, mapq, q[3], rng))
        if rng.random() < 0.05:
            out.append(sam(name, q[0] | 0x100, rname, pos + 3000, 0, b"%dM" % L, rng))
        if rng.random() < 0.04:
            out.append(sam(name, q[0] | 0x800, rname, pos + 5000, mapq, b"60S90M", rng))
        if rng.random() < 0.03:
            out.append(sam(name, q[0], rname, pos + 9, 1, b"%dM" % L, rng))    # a second primary: which one is first is the shuffle's
    for i in range(25):
        out.append(sam(b"stranger#%d" % i, rng.choice((0x41, 0x81, 0x91)), b"chrA", 100 + i, 60, b"%dM" % L, rng))
    rng.shuffle(out)
    return out


def bam_file(lines, refs, member, text=b"@HD\tVN:1.6\n"):
    return B.bgzf(B.bam_stream(lines, refs=refs, text=text), member=member)


_crafted = {}


def crafted():
    if not _crafted:
        rng = random.Random(20)
        truth = truth_lines(rng)
        test = derived_test_lines(rng, truth)
        for member in (997, 65280):
            _crafted[member] = (bam_file(truth, TRUTH_REFS, member), bam_file(test, TEST_REFS, member))
        _crafted["model"] = model(*_crafted[997])
    return _crafted


def test_the_crafted_inputs_cover_the_rule():
    c = crafted()
    want = c["model"]
    assert len(B.inflate(c[997][0])) > 340000 and len(B.inflate(c[997][0])) // B_SEGMENT >= 20
    assert all(n > 0 for n in totals(want)), totals(want)
    assert {k[1] for k in want["table"]} == set(M.CLASSES) and {k[0] for k in want["table"]} == {0, 1}
    assert {0, 1, 59, 60, 255} <= {k[2] for k in want["table"]}
    for k in ("secondary", "supplementary", "unknown", "repeated"):
        assert want[k] > 0, k
    assert sum(want["missing"].values()) > 0 and want["ambiguous"] == 0 == want["truth_duplicates"]
    assert model(*c[65280]) == want



@pytest.mark.parametrize("member", [997, 65280])
@pytest.mark.parametrize("feed", [1, "all"])
def test_crafted_join(ctx, member, feed):
    c = crafted()
    assert engine(ctx, *c[member], feed=feed) == c["model"]


def test_truth_and_test_fed_differently(ctx):
    c = crafted()
    assert engine(ctx, c[997][0], c[65280][1], feed="all", truth_feed=7) == c["model"]


@pytest.mark.parametrize("pct", [1, 100])
def test_crafted_join_other_overlaps(ctx, pct):
    c = crafted()
    want = model(*c[65280], pct=pct)
    assert want != c["model"] and engine(ctx, *c[65280], pct=pct) == want


def test_collisions(ctx):
    c = crafted()
    four, full = engine(ctx, *c[65280], key_bits=4), engine(ctx, *c[65280], key_bits=64)
    assert four == full == c["model"]
    assert engine(ctx, *c[997], feed=40, key_bits=1) == c["model"]


def test_duplicates_in_the_truth(ctx):
    lib = simuscop_amd.load_engine()
    rng = random.Random(31)
    truth = truth_lines(rng, 120, prefix=b"dup")
    by_name = {}
    for ln in truth:
        by_name.setdefault((fields(ln)[0], 1 if fields(ln)[1] & 0x80 else 0), ln)
    reads = sorted(by_name)
    twice, thrice = reads[:6], reads[6:9]
    for r in twice:
        truth.append(by_name[r])
    for r in thrice:
        truth += [by_name[r]] * 2
    rng.shuffle(truth)
    dup = set(twice + thrice)
    key4 = lambda r: lib.sg_eval_key(r[0], len(r[0]), r[1], 4)   # noqa: E731
    colliding = [r for r in reads if r not in dup and key4(r) == key4(twice[0])]
    assert colliding and lib.sg_eval_key(colliding[0][0], len(colliding[0][0]), colliding[0][1], 64) != lib.sg_eval_key(twice[0][0], len(twice[0][0]), twice[0][1], 64)
    # the mate of a duplicated read is no duplicate: same name, other mate
    assert any((r[0], 1 - r[1]) not in dup for r in dup)
    test = [by_name[r] for r in reads] + [by_name[twice[0]]]
    rng.shuffle(test)
    tf, qf = bam_file(truth, TRUTH_REFS, 4000), bam_file(test, TRUTH_REFS, 4000)
    want = model(tf, qf)
    assert want["truth_duplicates"] == 2 * 6 + 3 * 3 and want["ambiguous"] == len(dup) + 1 and want["repeated"] == 0
    assert sum(totals(want)) == len(reads) - len(dup) == totals(want)[0] + totals(want)[7]   # every other read, the colliding one too, is scored
    for bits in (4, 64):
        assert engine(ctx, tf, qf, feed=3, key_bits=bits) == want


def test_repeated_primaries_are_decided_by_file_order(ctx, tmp_path):
    rng = random.Random(47)
    truth = truth_lines(rng, 200, prefix=b"det")
    mapped = [ln for ln in truth if not fields(ln)[1] & 4]
    a, b = mapped[3], mapped[90]
    test = list(truth)
    rng.shuffle(test)
    test = [ln for ln in test if fields(ln)[0] not in (fields(a)[0], fields(b)[0])]

    def copy_of(ln, shift, mapq):
        name, flag, rname, pos, cigar = fields(ln)
        return sam(name, flag, rname, pos + shift, mapq, cigar, rng)
    # read a: three primaries far apart (the first in the file is the exact one); read b: two next to each other
    test.insert(10, copy_of(a, 0, 60))
    test.insert(150, copy_of(a, 400, 1))
    test.insert(300, copy_of(a, 800, 59))
    test[200:200] = [copy_of(b, 1, 255), copy_of(b, 0, 0)]
    stream = B.bam_stream(test, refs=TRUTH_REFS)
    member, per_call = 997, 8
    ends = {}
    for off, r in B.parse_stream(stream)[1]:
        nm = r[36:36 + r[12] - 1]
        if nm in (fields(a)[0], fields(b)[0]) and (1 if struct.unpack_from("<H", r, 18)[0] & 0x80 else 0) == (1 if fields(a if nm == fields(a)[0] else b)[1] & 0x80 else 0):
            ends.setdefault(nm, []).append((off + len(r) - 1) // member // per_call)   # the call that brings the record's last byte
    assert len(set(ends[fields(a)[0]])) == 3 and len(ends[fields(b)[0]]) == 2 and len(set(ends[fields(b)[0]])) == 1, ends
    tf, qf = bam_file(truth, TRUTH_REFS, 65280), B.bgzf(stream, member=member)
    want = model(tf, qf)
    assert want["repeated"] == 3 and sum(want["missing"].values()) == 2     # (the other mates of a and b were taken out)
    a_cls = "plain" if fields(a)[4] == b"%dM" % L else "edited"
    assert want["table"][(1 if fields(a)[1] & 0x80 else 0, a_cls, 60)][0] >= 1
    b_key = (1 if fields(b)[1] & 0x80 else 0, "plain" if fields(b)[4] == b"%dM" % L else "edited", 255)
    assert want["table"][b_key][1] == 1 and sum(want["table"][b_key]) == 1   # b's first primary: MAPQ 255, one base off
    assert engine(ctx, tf, qf, feed=per_call) == want == engine(ctx, tf, qf, feed="all") == engine(ctx, tf, qf, feed=1)
    # two runs of the command line: the same bytes, the model's
    tp, qp = str(tmp_path / "t.bam"), str(tmp_path / "q.bam")
    open(tp, "wb").write(tf)
    open(qp, "wb").write(qf)
    outs = []
    for i in range(2):
        out = str(tmp_path / ("eval%d.tsv" % i))
        r = subprocess.run([EXE, "--truth", tp, "--bam", qp, "--out", out, "--quiet"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] == M.tsv(want)


# ---- the closed loop through the command lines ----
LOOP = {"wgs_pe_xten": "test", "wgs_se_hs2000": "s1"}
_loop = {}


def simu(cfg, out, *flags):
    r = subprocess.run([SIMU, cfg, "--seed", str(SEED), "--out", out, "--quiet", *flags], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]


def truth_eval(truth, bam, out):
    r = subprocess.run([EXE, "--truth", truth, "--bam", bam, "--out", out, "--quiet", "--stats"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out, "rb").read(), r.stderr


def loop_base(name, tmp_path_factory):
    if name not in _loop:
        wd = str(tmp_path_factory.mktemp(name))
        cfg = cases.build_case(name, wd)
        plain = os.path.join(wd, "plain")
        simu(cfg, plain, "--truth-bam")
        truth = os.path.join(plain, LOOP[name] + ".truth.bam")
        # no read name twice: from the FASTQ files of this run (the oracle said so when the case was chosen)
        n_reads = 0
        for f in sorted(os.listdir(plain)):
            if f.endswith((".fq", ".fastq")):
                names = open(os.path.join(plain, f), "rb").read().split(b"\n")[0::4]
                names = [n for n in names if n]
                assert len(set(names)) == len(names) > 0, f
                n_reads += len(names)
        text, err = truth_eval(truth, truth, os.path.join(wd, "self.tsv"))
        _loop[name] = dict(wd=wd, cfg=cfg, truth=truth, text=text, n_reads=n_reads, err=err)
    return _loop[name]


def rows(text, tag):
    return [ln.split(b"\t")[1:] for ln in text.split(b"\n") if ln.startswith(tag + b"\t")]


@pytest.mark.parametrize("name", sorted(LOOP))
def test_closed_loop_truth_against_itself(name, tmp_path_factory):
    b = loop_base(name, tmp_path_factory)
    scalars = {k.decode(): int(v) for k, v in rows(b["text"], b"#T")}
    assert scalars["truth_records"] == scalars["test_records"] == b["n_reads"] > 1000
    for k in ("truth_duplicates", "unknown", "repeated", "ambiguous", "secondary", "supplementary"):
        assert scalars[k] == 0, k
    assert all(int(r[2]) == 0 for r in rows(b["text"], b"#X")) and len(rows(b["text"], b"#X")) == 6
    cells = [[int(v) for v in r[3:]] for r in rows(b["text"], b"#M")]
    assert sum(sum(r) for r in cells) == b["n_reads"]
    assert all(r[1] == r[2] == r[3] == r[4] == r[5] == r[6] == 0 for r in cells)      # exact or both_unmapped only
    assert sum(r[0] for r in cells) > 0
    assert {r[0] for r in rows(b["text"], b"#M")} == ({b"0", b"1"} if name == "wgs_pe_xten" else {b"0"})
    roc = rows(b["text"], b"#R")
    assert roc and all(r[3] == r[4] and r[1] == r[2] for r in roc)
    tn, t = M.records(B.inflate(open(b["truth"], "rb").read()))
    assert b["text"] == M.tsv(M.evaluate(tn, t, tn, t))
    assert '"truth_records": %d' % b["n_reads"] in b["err"] and '"t_inflate"' in b["err"]


@pytest.mark.parametrize("flags", [("--truth-sort",), ("--truth-tags",)], ids=["sorted", "tags"])
@pytest.mark.parametrize("name", sorted(LOOP))
def test_closed_loop_other_forms_of_the_truth(name, flags, tmp_path_factory):
    b = loop_base(name, tmp_path_factory)
    out = os.path.join(b["wd"], flags[0].strip("-"))
    simu(b["cfg"], out, "--truth-bam", *flags)
    other = os.path.join(out, LOOP[name] + ".truth.bam")
    assert open(other, "rb").read() != open(b["truth"], "rb").read()
    assert truth_eval(b["truth"], other, os.path.join(out, "as_test.tsv"))[0] == b["text"]
    assert truth_eval(other, b["truth"], os.path.join(out, "as_truth.tsv"))[0] == b["text"]


# ---- malformed test files ----
def test_a_refused_member_ends_the_session(ctx):
    """Through the ABI: a damaged member is refused with its file offset, every later call of the session says that it has
    failed, and the context takes a new session."""
    lib = simuscop_amd.load_engine()
    c = crafted()
    tf, qf = c[65280]
    mem, _ = B.members(qf)
    bad = mem[len(mem) // 2]
    corrupt = bytearray(qf)
    for k in range(30, 60):
        corrupt[bad[0] + k] ^= 0x5A
    corrupt = bytes(corrupt)
    n_ref, skip = header_bytes(B.inflate(tf))
    assert lib.sg_eval_begin(ctx, n_ref, 64, 10, skip) == 0
    try:
        assert lib.sg_eval_truth_bgzf(ctx, tf, len(tf)) == 0 and lib.sg_eval_truth_bgzf(ctx, None, 0) == 0
        assert lib.sg_eval_truth_done(ctx, None, None) == 0
        refmap = (C.c_int32 * len(TEST_REFS))(-1, 2, 0, 1)
        assert lib.sg_eval_test_refmap(ctx, refmap, len(TEST_REFS), header_bytes(B.inflate(qf))[1]) == 0
        assert lib.sg_eval_test_bgzf(ctx, corrupt, len(corrupt)) != 0
        assert b"file offset %d:" % bad[0] in lib.sg_last_error(ctx)
        table, counts = (C.c_uint64 * simuscop_amd.SG_EVAL_CELLS)(), simuscop_amd.SgEvalCounts()
        for rc in (lib.sg_eval_test_bgzf(ctx, qf, len(qf)), lib.sg_eval_finish(ctx, table, len(table), C.byref(counts))):
            assert rc != 0 and b"the session has failed" in lib.sg_last_error(ctx)
    finally:
        lib.sg_eval_end(ctx)
    assert engine(ctx, tf, qf) == c["model"]


def test_bad_input_names_the_offset_and_writes_nothing(tmp_path):
    c = crafted()
    tf, qf = c[997]
    tp = str(tmp_path / "t.bam")
    open(tp, "wb").write(tf)
    mem, _ = B.members(qf)
    # 1. cut inside a member
    cut = mem[len(mem) * 3 // 5]
    truncated = qf[:cut[0] + cut[1] // 2]
    # 2. a member whose DEFLATE data is damaged (its header and trailer stand)
    bad = mem[len(mem) // 2]
    corrupt = bytearray(qf)
    for k in range(30, 60):
        corrupt[bad[0] + k] ^= 0x5A
    # 3. the last record runs past the end of the stream
    stream = B.inflate(qf)
    last_off, last = B.parse_stream(stream)[1][-1]
    past = B.bgzf(stream[:last_off + len(last) - 40], member=997)
    for label, data, where in (("truncated", truncated, "file offset %d " % cut[0]), ("corrupt", bytes(corrupt), "file offset %d" % bad[0]),
                               ("past_end", past, "decompressed offset %d " % last_off)):
        qp, out = str(tmp_path / (label + ".bam")), str(tmp_path / (label + ".tsv"))
        open(qp, "wb").write(data)
        r = subprocess.run([EXE, "--truth", tp, "--bam", qp, "--out", out, "--quiet"], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and where in r.stderr and not os.path.exists(out), (label, r.returncode, r.stderr)
