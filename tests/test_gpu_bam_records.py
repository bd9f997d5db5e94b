"""BAM records on the MI355X (simuscop_amd/csrc/sg_bam.hip) of the shapes an aligner writes and tests/bam_util.py's plain
records lack: optional fields on every record (NM:i MD:Z AS:i XS:i RG:Z), a CG array in front of, behind and between fields
of all twelve other types (A c C s S i I f d Z H and B arrays of every element type), as CG:B:i, shorter than n_cigar, hidden
by an unknown type letter, beside a Z field that is not terminated; and records longer than a 16 KiB boundary segment,
than several of them, than a BGZF member and than several calls of sg_train_feed_bgzf.  The expectation is that of
test_gpu_train_bam.py: the .profile, .gc and counters of `--sam` on the lines tests/bam_util.py renders, byte for byte, and
through the ABI the counts of sg_train_feed on those lines."""
import ctypes as C
import os
import random

import pytest

import bam_util as B
import simuscop_amd
import test_gpu_train as G
import test_gpu_train_bam as TB
import train_util as TU

pytestmark = pytest.mark.gpu

B_SEGMENT = 16384   # kBamSegment of sg_bam.h


def _line(name, flag, pos, mapq, cigar, seq, qual, chrom=b"chr1"):
    return b"\t".join([name, b"%d" % flag, chrom, b"%d" % pos, b"%d" % mapq, cigar, b"=", b"0", b"0", seq, qual])


def _tagged_cases(L, rng, chrom=b"chr1", pos=None):
    """(lines, {index in lines: aux}, indices stored with the CG placeholder): every way CG can lie among other fields.
    pos: all of them at this position (one the caller knows countGC's window has not passed); default: 7000, 7050, ..."""
    s = bytes(rng.choice(b"ACGT") for _ in range(L))
    q = bytes(rng.choice(b"#-7<AFJ") for _ in range(L))
    every = B.aux_every_type(rng)
    al = B.aligner_tags(rng, L)
    lines, aux, cg = [], {}, set()

    def add(name, cigar, a, use_cg):
        aux[len(lines)] = a
        if use_cg:
            cg.add(len(lines))
        lines.append(_line(name, 0, 7000 + 50 * len(lines) if pos is None else pos, 60, cigar, s, q, chrom))

    # each CIGAR has an insertion of its own length: the insertion-length counts tell which CG was found
    add(b"cg_first", b"20M1I%dM" % (L - 21), (b"", b"".join(every) + al, b"I"), True)
    add(b"cg_last", b"20M2I%dM" % (L - 22), (al + b"".join(every), b"", b"I"), True)
    add(b"cg_middle", b"20M3I%dM" % (L - 23), (b"".join(every[:11]), b"".join(every[11:]), b"I"), True)
    add(b"cg_behind_arrays", b"20M4I%dM" % (L - 24), (b"".join(every[11:] + every[:11]), al, b"I"), True)
    add(b"cg_signed", b"20M5I%dM" % (L - 25), (b"".join(every[::-1]), b"", b"i"), True)
    for k, t in enumerate(every):   # behind each single type
        add(b"cg_behind_%d" % k, b"30M%dI%dM" % (6 + k, L - 36 - k), (t, al, b"I"), True)
    # CG with fewer operations than n_cigar: ignored, as htslib's bam_tag2cigar ignores it; the record keeps kSmN
    add(b"cg_short", b"%dS100N" % L, al + B.aux_tag(b"CG", "BI", [L << 4]), False)
    # a Z field that is not terminated before the record ends: nothing is found behind it, nothing is read past the record
    add(b"z_open", b"%dS100N" % L, al + b"XZZnever ends", False)
    # an unknown type letter: the walk stops, the CG behind it is not found
    add(b"unknown_type", b"20M7I%dM" % (L - 27), (al + b"XQ?abcdefg", b"", b"I"), True)
    return lines, aux, cg


def _refs_of(fa):
    refs = []
    for chunk in open(fa, "rb").read().split(b">")[1:]:
        name, seq = chunk.split(b"\n", 1)
        refs.append((name.split()[0], len(seq) - seq.count(b"\n")))
    return refs


def test_optional_fields_on_every_record(oracle_lib, tmp_path):
    wd = str(tmp_path)
    lines, fa1, T = G._sampled_lines(oracle_lib, wd, coverage=12)
    fa, vcf, bed, sam = TU.training_inputs(wd, fa1, lines, T.L, exome=False)
    rng = random.Random(21)
    body = [ln for ln in sam.split(b"\n") if ln]
    drop, keep = TB._extra_lines(T.L, rng)
    # seqToProfile always counts GC, and countGC turns a read away, before its CIGAR is looked at, when it starts left of the
    # window (Profile.cpp:552-554, :282-285).  So the records whose CIGAR hangs on the optional-field walk stand where the
    # body line beside them stands, and the --sam runs below show that none of them was turned away.
    at = body[len(body) // 2].split(b"\t")
    tagged, tagged_aux, tagged_cg = _tagged_cases(T.L, rng, chrom=at[2], pos=int(at[3]))
    mixed, aux, cg = [], {}, set()
    for i, ln in enumerate(body):
        mixed.append(ln)
        if i % 997 == 0:
            mixed.append(drop[(i // 997) % len(drop)])
        if i == len(body) // 2:
            mixed += keep
            for k, t in enumerate(tagged):
                if k in tagged_aux:
                    aux[len(mixed)] = tagged_aux[k]
                if k in tagged_cg:
                    cg.add(len(mixed))
                mixed.append(t)
    cg |= {i for i, ln in enumerate(mixed) if ln.startswith(b"cg\t")}
    for i in range(len(mixed)):   # realistic fields on every record
        if i not in aux:
            aux[i] = B.aligner_tags(rng, T.L)
    refs = _refs_of(fa)
    text = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    d = B.bam_stream(mixed, refs=refs, text=text, use_cg=cg, aux=aux)
    plain = B.bam_stream(mixed, refs=refs, text=text, use_cg=cg - {i for i, ln in enumerate(mixed) if ln.startswith(b"unknown_type\t")})
    view = B.view(d)
    # the optional fields change no line, except where they hide CG
    assert view.replace(b"\t%dS%dN\t" % (T.L, T.L - 7), b"\t20M7I%dM\t" % (T.L - 27)) == B.view(plain) and len(d) > len(plain) + 20 * len(mixed)
    assert view.count(b"\t%dS100N\t" % T.L) == 2 and view.count(b"\t%dS%dN\t" % (T.L, T.L - 7)) == 1
    for k in range(1, 6):
        assert b"\t20M%dI%dM\t" % (k, T.L - 20 - k) in view
    sam_path = os.path.join(wd, "view.sam")
    open(sam_path, "wb").write(view)
    want = os.path.join(wd, "want.profile")
    r, ws = TB._run(["--sam", sam_path, "-v", vcf, "-r", fa, "-o", want])
    assert r.returncode == 0, r.stderr[-2000:]
    want_body = open(want, "rb").read().split(b"\n", 2)[2]
    # the same text without those records, and with every CG hidden: no more reads are turned away with them than without,
    # so all of them reach the CIGAR walk, and what the walk finds is in the profile
    bare = os.path.join(wd, "bare.sam")
    names = tuple(t.split(b"\t")[0] + b"\t" for t in tagged)
    open(bare, "wb").write(b"".join(ln + b"\n" for ln in view.split(b"\n")[:-1] if not ln.startswith(names)))
    r, bs = TB._run(["--sam", bare, "-v", vcf, "-r", fa, "-o", os.path.join(wd, "bare.profile")])
    assert r.returncode == 0, r.stderr[-2000:]
    print("lines %d / %d without, gc_rejected %d / %d" % (ws["lines"], bs["lines"], ws["gc_rejected"], bs["gc_rejected"]))
    assert ws["lines"] == bs["lines"] + len(tagged) and ws["gc_rejected"] == bs["gc_rejected"]
    hidden = os.path.join(wd, "hidden.sam")
    hidden_d = B.bam_stream(mixed, refs=refs, text=text, use_cg=cg, aux={i: (b"XQ?", b"", b"I") for i in cg})   # (an unknown type in front of each CG)
    open(hidden, "wb").write(B.view(hidden_d))
    assert B.view(hidden_d).count(b"\t%dS" % T.L) >= len(cg)
    r, _ = TB._run(["--sam", hidden, "-v", vcf, "-r", fa, "-o", os.path.join(wd, "hidden.profile")])
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(os.path.join(wd, "hidden.profile"), "rb").read().split(b"\n", 2)[2] != want_body
    for k, v in enumerate((dict(member=65280, level=6), dict(member=997, level=1))):
        bam = os.path.join(wd, "x%d.bam" % k)
        open(bam, "wb").write(B.bgzf(d, member=v["member"], level=v["level"]))
        got = os.path.join(wd, "got%d.profile" % k)
        r, gs = TB._run(["-b", bam, "--decode-bam", "-v", vcf, "-r", fa, "-o", got])
        assert r.returncode == 0, (v, r.stderr[-2000:])
        assert open(got, "rb").read().split(b"\n", 2)[2] == want_body, v
        assert os.path.exists(want + ".gc") == os.path.exists(got + ".gc")
        if os.path.exists(want + ".gc"):
            assert open(want + ".gc", "rb").read() == open(got + ".gc", "rb").read()
        for c in TB.COUNTERS:
            assert gs[c] == ws[c], (v, c, gs[c], ws[c])
        assert gs["bam_bytes"] == os.path.getsize(bam)
        assert gs["bam_records"] == len(B.parse_stream(d)[1])


def _big(name, flag, pos, n, rng, fake_headers):
    """a record of n bases.  fake_headers: its qualities read, every 64 bytes, as the fixed fields of a record (block_size 60,
    refID 0, pos 0, l_read_name 9, mapq 60 ...), so that the boundary speculation finds starts inside it that are none"""
    s = bytes(rng.choice(b"ACGT") for _ in range(1000)) * (n // 1000)
    if fake_headers:
        unit = bytes(c + 33 for c in (60, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 9, 60, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                      65, 65, 65, 65, 65, 65, 65, 65, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
        assert len(unit) == 64
        q = unit * (n // 64) + b"F" * (n % 64)
    else:
        q = bytes(rng.choice(b"#-7<AFJ") for _ in range(1000)) * (n // 1000)
    return _line(name, flag, pos, 60, b"%dM" % n, s, q)


def test_records_longer_than_segments_members_and_calls(oracle_lib, tmp_path):
    wd = str(tmp_path)
    lines, fa1, T = G._sampled_lines(oracle_lib, wd, coverage=3)
    rng = random.Random(31)
    tagged, tagged_aux, tagged_cg = _tagged_cases(T.L, rng)
    big = {n: _big(b"big%d" % n, 0x100, 2000, n, rng, fake_headers=n != 12000) for n in (12000, 40000, 150000)}
    kept = _big(b"kept40000", 0, 1000, 40000, rng, fake_headers=True)
    assert len(lines) > 9000

    def build(with_kept):
        out = lines[:3000] + [big[12000]] + lines[3000:3003] + [big[40000]] + lines[3003:3004] + [big[150000], big[12000]] + lines[3004:6000]
        base = len(out)
        out += tagged + ([kept] if with_kept else []) + lines[6000:9000] + [big[150000]] + lines[9000:9010]
        aux = {base + k: a for k, a in tagged_aux.items()}
        arng = random.Random(5)
        for i in range(len(out)):
            if i not in aux and i % 3:
                aux[i] = B.aligner_tags(arng, T.L)
        return B.bam_stream(out, refs=[(b"chr1", 10 ** 7)], use_cg={base + k for k in tagged_cg}, aux=aux)

    eng = simuscop_amd.load_engine()
    ctx = C.c_void_p()
    assert eng.sg_create(C.byref(ctx), 0, 1) == 0
    try:
        keys = G._reference_on_device(eng, ctx, fa1)
        karr = (C.c_char_p * len(keys))(*keys)
        st = simuscop_amd.SgTrainSetup(contig_keys=karr, n_contigs=len(keys), bases=T.bases.encode(), kmer=3, bins=T.bins, n_isize=1024,
                                       n_indel_len=256, count_gc=1, window=1000)

        st_all = simuscop_amd.SgTrainSetup(contig_keys=karr, n_contigs=len(keys), bases=T.bases.encode(), kmer=3, bins=T.bins, n_isize=1024,
                                           n_indel_len=256, count_gc=0, window=1000)

        def session(feed, setup=st):
            assert eng.sg_train_begin(ctx, C.byref(setup)) == 0, eng.sg_last_error(ctx)
            feed()
            got, ga = TU.count_arrays(simuscop_amd.SgTrainCounts, T.kc, T.bins, 1024)
            assert eng.sg_train_finish(ctx, C.byref(got), None, None, 0, None) == 0, eng.sg_last_error(ctx)
            return got, ga

        for with_kept in (False, True):
            d = build(with_kept)
            sam = B.view(d)
            names, recs = B.parse_stream(d)
            ncarr = (C.c_char_p * len(names))(*names)
            h = recs[0][0]
            sizes = sorted(len(r) for _, r in recs)
            assert sizes[-1] > 3 * 65536 and sum(1 for n in sizes if n > 4 * B_SEGMENT) >= 2 and sum(1 for n in sizes if B_SEGMENT < n < 2 * B_SEGMENT) >= 2
            assert (b"kept40000\t" in sam) == with_kept and b"big" not in sam
            want, wa = session(lambda: eng.sg_train_feed(ctx, sam, len(sam)) == 0 or pytest.fail(eng.sg_last_error(ctx).decode()))
            assert want.lines == sam.count(b"\n") and want.reads_counted > 1000
            if with_kept:   # the kept record of 40,000 bases is a line to both routes (under countGC it is turned away; see below)
                less = sam.replace(kept + b"\n", b"")
                assert len(less) == len(sam) - len(kept) - 1
                without, _ = session(lambda: eng.sg_train_feed(ctx, less, len(less)) == 0 or pytest.fail("feed"))
                assert want.lines == without.lines + 1
            # the lines hold the CIGARs of the CG arrays, each with an insertion of its own length: without countGC, which turns
            # reads away by their window (Profile.cpp:283-285), every one of them is counted; with it, some
            want_all, wa_all = session(lambda: eng.sg_train_feed(ctx, sam, len(sam)) == 0 or pytest.fail("feed"), st_all)
            assert all(wa_all["ins_len"][ins] >= 1 for ins in range(1, 24)), wa_all["ins_len"][:24]
            if with_kept:   # ... and the kept record of 40,000 bases is a read whose bases are counted
                less_all, la_all = session(lambda: eng.sg_train_feed(ctx, less, len(less)) == 0 or pytest.fail("feed"), st_all)
                print("kept record: reads_counted %d / %d without it, quality counts %d / %d" %
                      (want_all.reads_counted, less_all.reads_counted, wa_all["quality"].sum(), la_all["quality"].sum()))
                assert want_all.reads_counted == less_all.reads_counted + 1
                assert wa_all["quality"].sum() - la_all["quality"].sum() > 20000
            for label, blob, per_call in (("one member per call", B.bgzf(d, member=65280, level=1), 1), ("small members", B.bgzf(d, member=3000, level=1), 5),
                                          ("all members in one call", B.bgzf(d, member=65280), 1 << 30)):
                ms, _ = B.members(blob)

                def feed_bam():
                    assert eng.sg_train_bam_start(ctx, ncarr, len(names), h) == 0, eng.sg_last_error(ctx)
                    bounds = [m[0] for m in ms][::per_call] + [len(blob)]
                    for a, b in zip(bounds, bounds[1:]):
                        assert eng.sg_train_feed_bgzf(ctx, blob[a:b], b - a) == 0, (label, eng.sg_last_error(ctx))
                    assert eng.sg_train_feed_bgzf(ctx, None, 0) == 0, eng.sg_last_error(ctx)
                    nrec = C.c_uint64()
                    assert eng.sg_train_bam_info(ctx, C.byref(nrec), None, None) == 0 and nrec.value == len(recs), (label, nrec.value, len(recs))
                got, ga = session(feed_bam)
                G._same_counts(got, ga, want, wa)
                got, ga = session(feed_bam, st_all)   # every read counted: each CG array's CIGAR and the long read are in the counts
                G._same_counts(got, ga, want_all, wa_all)
        # the largest record cut by the end of the stream, in a call of its own members and behind whole records
        d = build(False)
        names, recs = B.parse_stream(d)
        ncarr = (C.c_char_p * len(names))(*names)
        last_big = max(i for i, (_, r) in enumerate(recs) if len(r) > 200000)
        for per_call in (1, 1 << 30):
            blob = B.bgzf(d[:recs[last_big][0] + 170000], member=65280, level=1)
            ms, _ = B.members(blob)
            assert eng.sg_train_begin(ctx, C.byref(st)) == 0
            assert eng.sg_train_bam_start(ctx, ncarr, len(names), recs[0][0]) == 0
            bounds = [m[0] for m in ms][::per_call] + [len(blob)]
            for a, b in zip(bounds, bounds[1:]):
                assert eng.sg_train_feed_bgzf(ctx, blob[a:b], b - a) == 0, eng.sg_last_error(ctx)
            assert eng.sg_train_feed_bgzf(ctx, None, 0) == 1
            msg = eng.sg_last_error(ctx)
            assert b"runs past the end" in msg and b"offset %d " % recs[last_big][0] in msg, msg
            eng.sg_train_end(ctx)
    finally:
        eng.sg_destroy(ctx)


def test_large_records_through_the_command_line(oracle_lib, tmp_path):
    wd = str(tmp_path)
    lines, fa1, T = G._sampled_lines(oracle_lib, wd, coverage=3)
    fa, vcf, bed, sam = TU.training_inputs(wd, fa1, lines, T.L, exome=False)
    rng = random.Random(41)
    body = [ln for ln in sam.split(b"\n") if ln]
    big = [_big(b"big%d" % n, 0x100, 2000, n, rng, fake_headers=n != 12000) for n in (12000, 40000, 150000)]
    kept = _big(b"kept40000", 0, 1000, 40000, rng, fake_headers=True)
    refs = _refs_of(fa)
    text = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    for with_kept in (False, True):
        mixed = body[:500] + big[:1] + body[500:502] + big[1:2] + body[502:503] + big[2:] + ([kept] if with_kept else []) + body[503:] + big[2:] + body[:3]
        d = B.bam_stream(mixed, refs=refs, text=text)
        view = B.view(d)
        assert b"big" not in view and (b"kept40000" in view) == with_kept
        sam_path = os.path.join(wd, "view%d.sam" % with_kept)
        open(sam_path, "wb").write(view)
        want = os.path.join(wd, "want%d.profile" % with_kept)
        r, ws = TB._run(["--sam", sam_path, "-v", vcf, "-r", fa, "-o", want])
        assert r.returncode == 0, r.stderr[-2000:]
        for k, member in enumerate((65280, 20000)):
            bam = os.path.join(wd, "x%d_%d.bam" % (with_kept, k))
            open(bam, "wb").write(B.bgzf(d, member=member, level=1))
            got = os.path.join(wd, "got%d_%d.profile" % (with_kept, k))
            rg, gs = TB._run(["-b", bam, "--decode-bam", "-v", vcf, "-r", fa, "-o", got])
            # a line of 40,000 bases is a line like any other to the --sam route (it refuses lines above 64 MB only), so to both
            assert rg.returncode == 0, (with_kept, member, rg.stderr[-2000:])
            assert open(got, "rb").read().split(b"\n", 2)[2] == open(want, "rb").read().split(b"\n", 2)[2], (with_kept, member)
            assert os.path.exists(want + ".gc") == os.path.exists(got + ".gc")
            if os.path.exists(want + ".gc"):
                assert open(want + ".gc", "rb").read() == open(got + ".gc", "rb").read()
            for c in TB.COUNTERS:
                assert gs[c] == ws[c], (with_kept, member, c, gs[c], ws[c])
            assert gs["bam_records"] == len(B.parse_stream(d)[1])
