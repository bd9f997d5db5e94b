"""The engine's pass state (sg_ctx::Pass, sg_api.h) seen through the C ABI: which call is accepted at which stage of a
pass and what a refusal says; that the text readers settle a queued pass themselves, so that they return the whole text
without sg_result in front of them, also of a batch whose slow-item queue overflowed; and that new chains retire a
finished pass's rows but not its text."""
import ctypes as C

import pytest

import cases
import simuscop_amd

pytestmark = pytest.mark.gpu

OK, INVALID = 0, 1
STALE = "the chains or the profile changed since sg_sample"


def _calls(sess):
    """name -> a call of that entry point on the session's context that returns (rc, what it read)."""
    eng, ctx = sess.eng, sess.ctx
    u = [C.c_uint64() for _ in range(3)]
    buf = C.create_string_buffer(64)

    def fetch_range():
        rc = eng.sg_fetch_range(ctx, 0, 0, 64, buf)
        return rc, buf.raw

    def fetch_compressed():
        rc = eng.sg_fetch_compressed(ctx, 0, 0, 28, buf)
        return rc, buf.raw[:28]

    def device_output():
        d1, d2 = C.c_void_p(), C.c_void_p()
        rc = eng.sg_device_output(ctx, C.byref(d1), C.byref(d2))
        return rc, bool(d1.value) and bool(d2.value)

    def detach_outputs():
        h = C.c_void_p()
        rc = eng.sg_detach_outputs(ctx, C.byref(h))
        if rc == OK:
            assert eng.sg_release_outputs(ctx, h) == OK
        return rc, None

    def emit_info():
        r = C.c_int()
        return eng.sg_emit_info(ctx, C.byref(u[0]), C.byref(r)), None

    def emit_path():
        return eng.sg_emit_path(ctx, C.byref(simuscop_amd.SgEmitPathInfo())), None

    def truth_reads():
        rows = (simuscop_amd.SgTruthRead * 4)()
        return eng.sg_truth_reads(ctx, 0, 0, 4, rows), None

    return {
        "sg_sample": lambda: (eng.sg_sample(ctx), None),
        "sg_result": lambda: (eng.sg_result(ctx, C.byref(u[0]), C.byref(u[1]), C.byref(u[2])), (u[0].value, u[1].value, u[2].value)),
        "sg_fetch_range": fetch_range,
        "sg_device_output": device_output,
        "sg_compress": lambda: (eng.sg_compress(ctx, C.byref(u[0]), C.byref(u[1])), None),
        "sg_fetch_compressed": fetch_compressed,
        "sg_detach_outputs": detach_outputs,
        "sg_emit_info": emit_info,
        "sg_emit_path": emit_path,
        "sg_truth_reads": truth_reads,
        "sg_errtab_add": lambda: (eng.sg_errtab_add(ctx, C.byref(u[0]), C.byref(u[1])), None),
    }


def test_call_order_matrix(tmp_path):
    """One context walked through a pass's stages; at each, every entry point that reads a pass, in the order given
    (sg_detach_outputs last where it succeeds: it ends the stage).  A row is (call, return code, substring of
    sg_last_error or None where the call leaves none).  Every cell that differs is reported, not only the first."""
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path))
    wrong, seen = [], {}
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=5, truth_errors=1, truth_bam=1) as sess:
        call = _calls(sess)

        def stage(name, rows):
            for fn, rc_want, msg_want in rows:
                rc, got = call[fn]()
                seen[(name, fn)] = got
                msg = sess.eng.sg_last_error(sess.ctx).decode()
                if rc != rc_want or (rc_want != OK and msg_want is not None and not (msg.startswith(fn + ":") and msg_want in msg)):
                    wrong.append((name, fn, rc, msg if rc else ""))

        nothing_sampled = [("sg_result", INVALID, "call sg_sample first"), ("sg_fetch_range", INVALID, "call sg_sample first"),
                           ("sg_device_output", INVALID, "call sg_sample first"), ("sg_compress", INVALID, "call sg_result first"),
                           ("sg_fetch_compressed", INVALID, "call sg_compress first"), ("sg_emit_info", INVALID, "call sg_result first"),
                           ("sg_emit_path", INVALID, None), ("sg_detach_outputs", INVALID, "call sg_result first")]
        all_ok = [("sg_result", OK, None), ("sg_fetch_range", OK, None), ("sg_device_output", OK, None), ("sg_compress", OK, None),
                  ("sg_fetch_compressed", OK, None), ("sg_emit_info", OK, None), ("sg_emit_path", OK, None)]
        # (no batch yet: no chains, and the session begins its error table with its first batch)
        stage("created", [("sg_sample", INVALID, "call sg_plan first")] + nothing_sampled +
              [("sg_truth_reads", INVALID, "no piece map"), ("sg_errtab_add", INVALID, "call sg_errtab_begin first")])
        sess.weighted_length()
        sess.set_reads(sess.planned_reads)
        assert sess.prepare_batch(0)
        rows_refused = [("sg_truth_reads", INVALID, "call sg_result first"), ("sg_errtab_add", INVALID, "call sg_result first")]
        stage("planned", nothing_sampled + rows_refused)
        sess.sample()
        # the calls that ask for sg_result first: the text readers behind them settle the pass themselves
        stage("sampled", [r for r in nothing_sampled if "sg_sample" not in (r[2] or "")] + rows_refused +
              [("sg_fetch_range", OK, None), ("sg_device_output", OK, None)])
        stage("resulted", [("sg_fetch_compressed", INVALID, "call sg_compress first")] + all_ok +
              [("sg_truth_reads", OK, None), ("sg_errtab_add", OK, None), ("sg_detach_outputs", OK, None)])
        assert seen[("sampled", "sg_fetch_range")] == seen[("resulted", "sg_fetch_range")] and seen[("resulted", "sg_device_output")]
        stage("detached", nothing_sampled + rows_refused)
        # the same plan again: the last pass's members are not this one's
        stage("sampled again", [("sg_sample", OK, None), ("sg_result", OK, None), ("sg_fetch_compressed", INVALID, "call sg_compress first"),
                                ("sg_fetch_range", OK, None)])
        assert seen[("sampled again", "sg_result")] == seen[("resulted", "sg_result")]
        assert seen[("sampled again", "sg_fetch_range")] == seen[("resulted", "sg_fetch_range")]
        # new chains: the rows are no longer theirs, the plan is gone, the text stays
        one = b"ACGT" * 250
        arr, lens = (C.c_char_p * 1)(one), (C.c_uint64 * 1)(len(one))
        assert sess.eng.sg_upload_haplotypes(sess.ctx, 1, arr, lens) == OK
        stage("new chains", [("sg_truth_reads", INVALID, STALE), ("sg_errtab_add", INVALID, STALE), ("sg_sample", INVALID, "call sg_plan first")] +
              all_ok + [("sg_detach_outputs", OK, None)])
        assert seen[("new chains", "sg_result")] == seen[("resulted", "sg_result")]
        assert seen[("new chains", "sg_fetch_range")] == seen[("resulted", "sg_fetch_range")]
        stage("new chains, detached", [("sg_sample", INVALID, "call sg_plan first")] + nothing_sampled)
    assert not wrong, wrong


def _text_bytes(eng, ctx, mate):
    """A settled pass's text size without sg_result: the largest offset at which an empty sg_fetch_range is in range."""
    lo, hi = 0, 1 << 40
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if eng.sg_fetch_range(ctx, mate, mid, 0, None) == OK:
            lo = mid
        else:
            hi = mid - 1
    return lo


def _whole_text(eng, ctx):
    out = []
    for mate in (0, 1):
        n = _text_bytes(eng, ctx, mate)
        buf = C.create_string_buffer(n)
        assert eng.sg_fetch_range(ctx, mate, 0, n, buf) == OK, eng.sg_last_error(ctx)
        out.append(buf.raw)
    return tuple(out)


def _read_by_fetch(sess):
    # (a read is at most L + 512 bases, a name's prefix at most 990 bytes: a record stays below 4 KiB)
    cap = sess.batch_slots * 4096
    b1, b2 = C.create_string_buffer(cap), C.create_string_buffer(cap)
    assert sess.eng.sg_fetch(sess.ctx, b1, b2) == OK, sess.eng.sg_last_error(sess.ctx)
    n1, n2, _ = sess.result()
    return b1.raw[:n1], b2.raw[:n2]


def _read_by_fetch_range(sess):
    return _whole_text(sess.eng, sess.ctx)


def _read_by_device_output(sess):
    d1, d2 = C.c_void_p(), C.c_void_p()
    assert sess.eng.sg_device_output(sess.ctx, C.byref(d1), C.byref(d2)) == OK and d1.value and d2.value
    return _whole_text(sess.eng, sess.ctx)


@pytest.mark.parametrize("seed, read", [(9101, _read_by_fetch), (9102, _read_by_fetch_range), (9103, _read_by_device_output)],
                         ids=["sg_fetch", "sg_fetch_range", "sg_device_output"])
def test_text_without_sg_result_on_an_overflowing_batch(tmp_path, monkeypatch, seed, read):
    """sg_sample, then a text reader with no sg_result in between, on a batch whose slow-item queue overflows (one slot):
    the text is the one sg_result, sg_fetch give.  The reader's session comes first and each reader has a seed of its
    own: device blocks come back dirty from the block cache, and the bytes of an earlier identical pass would stand in
    for items that were never written."""
    cfg = cases.build_case("indel_rich_n_islands_pe", str(tmp_path))
    monkeypatch.setenv("SG_SLOWQ_CAP", "1")

    def session():
        sess = simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=seed)
        sess.weighted_length()
        sess.set_reads(sess.planned_reads)
        assert sess.prepare_batch(0)
        sess.sample()
        return sess

    with session() as sess:
        early = read(sess)
        n1, n2, _ = sess.result()
        assert (len(early[0]), len(early[1])) == (n1, n2) and sess.emit_info()[1] is True
    with session() as sess:
        n1, n2, _ = sess.result()
        late = sess.fetch(n1, n2)
        assert sess.emit_info()[1] is True      # (otherwise nothing was deferred and the test proves nothing)
    assert n1 > 0 and n2 > 0
    assert early[0] == late[0] and early[1] == late[1]
