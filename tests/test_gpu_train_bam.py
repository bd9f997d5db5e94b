"""`seqToProfile -b x.bam --decode-bam` on the MI355X: BGZF inflated and the BAM records decoded on the device
(sg_inflate.hip, sg_bam.hip) give the same .profile and .gc, byte for byte, as `--sam` on the lines `samtools view -F 0xD04
-q 20` prints of that BAM (tests/bam_util.py renders them; the --sam route is pinned to oracle/train_oracle.cpp by
test_gpu_train.py), and the same counters.  The BAMs are written by tests/bam_util.py: records the filter drops between the
ones it keeps, records without sequence, quality or CIGAR, a CG:B:I record, reads on contigs the FASTA lacks, names and
qualities that look like a record header, members from 150 B to 64 KiB (records straddle dozens of members), a header over
several members, every kind of cut between two calls of sg_train_feed_bgzf."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest

import bam_util as B
import simuscop_amd
import test_gpu_train as G
import train_util as TU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "simuscop_amd", "lib", "seqToProfile")


def _extra_lines(L, rng):
    """Records the filter drops, ones it keeps, and the odd shapes a BAM can hold."""
    s = bytes(rng.choice(b"ACGT") for _ in range(L))
    q = bytes(rng.choice(b"#-7<AFJ") for _ in range(L))
    mk = lambda name, flag, chrom, pos, mapq, cigar, seq=s, qual=q: b"\t".join(   # noqa: E731
        [name, b"%d" % flag, chrom, b"%d" % pos, b"%d" % mapq, cigar, b"=" if chrom != b"*" else b"*", b"0", b"0", seq, qual])
    drop = [mk(b"u", 4, b"*", 0, 0, b"*"), mk(b"s", 0x100, b"chr1", 5000, 60, b"%dM" % L), mk(b"d", 0x400, b"chr1", 5000, 60, b"%dM" % L),
            mk(b"p", 0x800, b"chr1", 5000, 60, b"%dM" % L), mk(b"q", 0, b"chr1", 5000, 19, b"%dM" % L)]
    # a quality string whose raw bytes read as a record header: block_size 64, refID 0, pos 0, l_read_name 9 ...
    fake = bytes(c + 33 for c in (64, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 9, 60, 0, 0)) + q[16:]
    keep = [mk(b"f", 0x200, b"chr1", 6000, 60, b"%dM" % L), mk(b"m20", 0, b"chr1", 6100, 20, b"%dM" % L), mk(b"m255", 0, b"chr1", 6200, 255, b"%dM" % L),
            mk(b"noseq", 0, b"chr1", 6300, 60, b"%dM" % L, b"*", b"*"), mk(b"noqual", 0, b"chr1", 6400, 60, b"%dM" % L, s, b"*"),
            mk(b"nocigar", 0, b"chr1", 6500, 60, b"*"), mk(b"absent", 0, b"chrUn_x", 100, 60, b"%dM" % L),
            mk(b"fakehdr", 0, b"chr1", 6600, 60, b"%dM" % L, s, fake), mk(b"@\x21\x21\x21", 0, b"chr1", 6700, 60, b"%dM" % L),
            mk(b"cg", 0, b"chr1", 6800, 60, b"20M2I%dM" % (L - 22))]
    return drop, keep


def _training_bam(oracle_lib, wd, exome):
    lines, fa1, T = G._sampled_lines(oracle_lib, wd, coverage=12)
    fa, vcf, bed, sam = TU.training_inputs(wd, fa1, lines, T.L, exome=exome)
    rng = random.Random(11)
    body = [ln for ln in sam.split(b"\n") if ln]
    drop, keep = _extra_lines(T.L, rng)
    mixed = []
    for i, ln in enumerate(body):   # interleaved
        mixed.append(ln)
        if i % 997 == 0:
            mixed.append(drop[(i // 997) % len(drop)])
        if i == len(body) // 2:
            mixed += keep
    cg = {i for i, ln in enumerate(mixed) if ln.startswith(b"cg\t")}
    refs = []
    for chunk in open(fa, "rb").read().split(b">")[1:]:
        name, seq = chunk.split(b"\n", 1)
        refs.append((name.split()[0], len(seq) - seq.count(b"\n")))
    text = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    d = B.bam_stream(mixed, refs=refs, text=text, use_cg=cg)
    return d, fa, vcf, bed, T


def _run(args, **kw):
    r = subprocess.run([EXE, *args, "--quiet", "--stats"], capture_output=True, timeout=600, **kw)
    stats = [json.loads(x) for x in r.stderr.decode(errors="replace").splitlines() if x.startswith("{")]
    return r, stats[-1] if stats else None


COUNTERS = ("lines", "reads_counted", "gc_rejected", "gc_windows", "gc_pairs", "skipped_overhang", "read_length", "bins", "gc_fitted", "capped")


@pytest.mark.parametrize("exome", [False, True])
def test_decode_bam_writes_the_profile_of_the_sam_route(exome, oracle_lib, tmp_path):
    wd = str(tmp_path)
    d, fa, vcf, bed, T = _training_bam(oracle_lib, wd, exome)
    sam_path = os.path.join(wd, "view.sam")
    open(sam_path, "wb").write(B.view(d))
    tg = ["-t", bed] if bed else []
    want = os.path.join(wd, "want.profile")
    r, ws = _run(["--sam", sam_path, "-v", vcf, "-r", fa, "-o", want, *tg])
    assert r.returncode == 0, r.stderr[-2000:]
    want_body = open(want, "rb").read().split(b"\n", 2)[2]
    variants = [dict(member=65280, level=6), dict(member=997, level=1), dict(member=150, level=0)] if not exome else \
               [dict(member=40000, level=9), dict(member=333, level=6)]
    # a header of several members: a long comment block in front of the records
    if not exome:
        variants.append(dict(member=65280, level=6, big_header=True))
    for k, v in enumerate(variants):
        dd = d
        if v.get("big_header"):
            co = b"".join(b"@CO\t%s\n" % (b"x" * 200) for _ in range(1200))
            names, recs = B.parse_stream(d)
            l_text = int.from_bytes(d[4:8], "little")
            hdr_end = recs[0][0]
            dd = b"BAM\1" + (l_text + len(co)).to_bytes(4, "little") + d[8:8 + l_text] + co + d[8 + l_text:hdr_end] + d[hdr_end:]
            assert B.view(dd) == B.view(d)
        bam = os.path.join(wd, "x%d.bam" % k)
        open(bam, "wb").write(B.bgzf(dd, member=v["member"], level=v["level"]))
        got = os.path.join(wd, "got%d.profile" % k)
        r, gs = _run(["-b", bam, "--decode-bam", "-v", vcf, "-r", fa, "-o", got, *tg])
        assert r.returncode == 0, (v, r.stderr[-2000:])
        assert b"samtools not specified" not in r.stderr and b"EOF marker" not in r.stderr
        lines = open(got, "rb").read().split(b"\n", 2)
        assert lines[1] == b"#reads: " + bam.encode()
        assert lines[2] == want_body, v
        assert os.path.exists(want + ".gc") == os.path.exists(got + ".gc")
        if os.path.exists(want + ".gc"):
            assert open(want + ".gc", "rb").read() == open(got + ".gc", "rb").read()
        for c in COUNTERS:
            assert gs[c] == ws[c], (v, c, gs[c], ws[c])
        assert gs["bam_bytes"] == os.path.getsize(bam)
        assert gs["bam_records"] == len(B.parse_stream(dd)[1])
    if exome:
        return
    # --max-reads: both routes end at the same read
    cap = ws["reads_counted"] // 3
    want_c, got_c = os.path.join(wd, "want_cap.profile"), os.path.join(wd, "got_cap.profile")
    r, wsc = _run(["--sam", sam_path, "-v", vcf, "-r", fa, "-o", want_c, "--max-reads", str(cap)])
    assert r.returncode == 0 and wsc["capped"] == 1
    bam = os.path.join(wd, "x1.bam")
    r, gsc = _run(["-b", bam, "--decode-bam", "-v", vcf, "-r", fa, "-o", got_c, "--max-reads", str(cap)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(got_c, "rb").read().split(b"\n", 2)[2] == open(want_c, "rb").read().split(b"\n", 2)[2]
    for c in COUNTERS:
        assert gsc[c] == wsc[c], (c, gsc[c], wsc[c])
    # no EOF member: samtools' warning, the same profile; through standard input as well
    noeof = os.path.join(wd, "noeof.bam")
    open(noeof, "wb").write(B.bgzf(d, member=65280, level=6, eof=False))
    got_n = os.path.join(wd, "got_noeof.profile")
    r, _ = _run(["-b", noeof, "--decode-bam", "-v", vcf, "-r", fa, "-o", got_n])
    assert r.returncode == 0 and b"EOF marker is absent" in r.stderr, r.stderr[-2000:]
    assert open(got_n, "rb").read().split(b"\n", 2)[2] == want_body
    got_s = os.path.join(wd, "got_stdin.profile")
    with open(noeof, "rb") as f:
        r, _ = _run(["-b", "-", "--decode-bam", "-v", vcf, "-r", fa, "-o", got_s], stdin=f)
    assert r.returncode == 0 and b"EOF marker is absent" in r.stderr, r.stderr[-2000:]
    assert open(got_s, "rb").read().split(b"\n", 2)[2] == want_body
    # a truncated member: an error, no file
    blob = B.bgzf(d, member=65280, level=6)
    trunc = os.path.join(wd, "trunc.bam")
    open(trunc, "wb").write(blob[:len(blob) // 2])
    got_t = os.path.join(wd, "got_trunc.profile")
    r, _ = _run(["-b", trunc, "--decode-bam", "-v", vcf, "-r", fa, "-o", got_t])
    assert r.returncode != 0 and b"truncated" in r.stderr and not os.path.exists(got_t), r.stderr[-2000:]
    # a corrupt member in the middle: an error naming its offset, no file
    ms, _ = B.members(blob)
    bad = bytearray(blob)
    bad[ms[3][0] + ms[3][1] + 1 - 8] ^= 0x55   # its CRC-32
    badp = os.path.join(wd, "crc.bam")
    open(badp, "wb").write(bytes(bad))
    r, _ = _run(["-b", badp, "--decode-bam", "-v", vcf, "-r", fa, "-o", got_t])
    assert r.returncode != 0 and b"offset %d" % ms[3][0] in r.stderr and not os.path.exists(got_t), r.stderr[-2000:]
    # a header without records: the --sam route's refusal
    names, recs = B.parse_stream(d)
    empty = os.path.join(wd, "empty.bam")
    open(empty, "wb").write(B.bgzf(d[:recs[0][0]]))
    r, _ = _run(["-b", empty, "--decode-bam", "-v", vcf, "-r", fa, "-o", got_t])
    assert r.returncode == 1 and b"single match" in r.stderr, r.stderr[-2000:]
    # not a BAM file
    r, _ = _run(["-b", sam_path, "--decode-bam", "-v", vcf, "-r", fa, "-o", got_t])
    assert r.returncode != 0 and not os.path.exists(got_t)


def test_feed_bgzf_at_every_kind_of_cut(oracle_lib, tmp_path):
    """sg_train_feed_bgzf against sg_train_feed through the ABI: the members handed over one per call, cut inside the header,
    at a record start, inside block_size, inside the fixed fields, the name, the sequence; counts identical."""
    wd = str(tmp_path)
    lines, fa1, T = G._sampled_lines(oracle_lib, wd, coverage=3)
    rng = random.Random(3)
    drop, keep = _extra_lines(T.L, rng)
    lines = lines[:6000] + drop + keep + lines[6000:9000] + TU.filter_lines(T.L)
    d = B.bam_stream(lines, refs=[(b"chr1", 10 ** 6)], use_cg={i for i, ln in enumerate(lines) if ln.startswith(b"cg\t")})
    sam = B.view(d)
    names, recs = B.parse_stream(d)
    h = recs[0][0]
    cuts = [h - 5, h, h + 2]
    for j, (o, r) in enumerate(recs[1:400]):
        cuts.append(o + (0, 2, 4, 20, 37, 60, len(r) // 2, len(r) - 1)[j % 8])
    eng = simuscop_amd.load_engine()
    ctx = C.c_void_p()
    assert eng.sg_create(C.byref(ctx), 0, 1) == 0
    try:
        keys = G._reference_on_device(eng, ctx, fa1)
        karr = (C.c_char_p * len(keys))(*keys)
        ncarr = (C.c_char_p * len(names))(*names)

        def session(feed):
            st = simuscop_amd.SgTrainSetup(contig_keys=karr, n_contigs=len(keys), bases=T.bases.encode(), kmer=3, bins=T.bins, n_isize=1024,
                                           n_indel_len=256, count_gc=1, window=1000)
            assert eng.sg_train_begin(ctx, C.byref(st)) == 0, eng.sg_last_error(ctx)
            feed()
            got, ga = TU.count_arrays(simuscop_amd.SgTrainCounts, T.kc, T.bins, 1024)
            assert eng.sg_train_finish(ctx, C.byref(got), None, None, 0, None) == 0, eng.sg_last_error(ctx)
            return got, ga

        want, wa = session(lambda: eng.sg_train_feed(ctx, sam, len(sam)) == 0 or pytest.fail(eng.sg_last_error(ctx)))
        assert want.lines == sam.count(b"\n") and want.reads_counted > 1000
        for label, blob, per_call in (("cuts", B.bgzf(d, cuts=sorted(cuts)), 1), ("tiny", B.bgzf(d, member=64, level=1), 7),
                                      ("whole", B.bgzf(d, member=65280), 1 << 30)):
            ms, _ = B.members(blob)

            def feed_bam():
                assert eng.sg_train_bam_start(ctx, ncarr, len(names), h) == 0, eng.sg_last_error(ctx)
                bounds = [m[0] for m in ms][::per_call] + [len(blob)]
                for a, b in zip(bounds, bounds[1:]):
                    assert eng.sg_train_feed_bgzf(ctx, blob[a:b], b - a) == 0, (label, eng.sg_last_error(ctx))
                assert eng.sg_train_feed_bgzf(ctx, None, 0) == 0, eng.sg_last_error(ctx)
                nrec = C.c_uint64()
                assert eng.sg_train_bam_info(ctx, C.byref(nrec), None, None) == 0 and nrec.value == len(recs)
            got, ga = session(feed_bam)
            G._same_counts(got, ga, want, wa)
        # a record cut by the end of the stream
        blob = B.bgzf(d[:recs[-1][0] + 50])

        def feed_cut():
            assert eng.sg_train_bam_start(ctx, ncarr, len(names), h) == 0
            assert eng.sg_train_feed_bgzf(ctx, blob, len(blob)) == 0, eng.sg_last_error(ctx)
            assert eng.sg_train_feed_bgzf(ctx, None, 0) == 1
            assert b"runs past the end" in eng.sg_last_error(ctx)
        st = simuscop_amd.SgTrainSetup(contig_keys=karr, n_contigs=len(keys), bases=T.bases.encode(), kmer=3, bins=T.bins, n_isize=1024,
                                       n_indel_len=256, count_gc=1, window=1000)
        assert eng.sg_train_begin(ctx, C.byref(st)) == 0
        feed_cut()
        eng.sg_train_end(ctx)
        # a record with an op code above 8, and one whose block_size is smaller than its fixed fields
        for what, patch in (("op", lambda x, o: x.__setitem__(slice(o + 36 + x[o + 12], o + 37 + x[o + 12]), bytes([x[o + 36 + x[o + 12]] | 0x0F]))),
                            ("short", lambda x, o: x.__setitem__(slice(o + 20, o + 24), (10 ** 6).to_bytes(4, "little")))):
            x = bytearray(d)
            patch(x, recs[100][0])
            blob = B.bgzf(bytes(x))
            assert eng.sg_train_begin(ctx, C.byref(st)) == 0
            assert eng.sg_train_bam_start(ctx, ncarr, len(names), h) == 0
            assert eng.sg_train_feed_bgzf(ctx, blob, len(blob)) == 1, what
            assert b"offset %d" % recs[100][0] in eng.sg_last_error(ctx), (what, eng.sg_last_error(ctx))
            eng.sg_train_end(ctx)
        assert np.any(wa["subs1"])
    finally:
        eng.sg_destroy(ctx)
