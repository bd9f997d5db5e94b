"""`simuReads --truth-bam` on the MI355X: every read's true alignment as BAM records made on the device (sg_truth.hip).

  1. the records carry the FASTQ: name, bases and qualities of every record, turned back by flag 0x10, are the
     oracle(philox) FASTQ record in the same place, and the FASTQ files do not change with the option;
  2. the device states the host rule: sg_truth_reads through sg_truth_align (pinned to tests/truth_model.py by
     test_truth_align_cpu.py) gives every record's refID, POS and CIGAR; the other fields follow from the two mates;
  3. replay, independent of both: with a profile that substitutes nothing, every M base of every record is the
     reference's base (or a known alternative allele) at the place the record names;
  4. the loop closes: the project's own trainer reads the file (`seqToProfile -b truth.bam --decode-bam`) and counts what
     the restatement of the reference's trainer counts on the same records;
  5. sharded runs give the same record stream; refused combinations are refused."""
import collections
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import bam_util as B
import cases
import profile_shapes as PS
import simuscop_amd
import simuscop_amd.build as build
import train_util as TU
import truth_model as tm
import truth_util as U
from profile_shapes import Shape
from simuscop_amd import synth

pytestmark = pytest.mark.gpu

SIMU = os.path.join(build.LIBDIR, "simuReads")
TRAIN = os.path.join(build.LIBDIR, "seqToProfile")
SEED = (cases.FAKE_SEC << 32) | cases.FAKE_NSEC
EVIDENCE = os.environ.get("TRUTH_EVIDENCE_DIR", "")


def simu(cfg, out, *flags, env=None, ok=True):
    r = subprocess.run([SIMU, cfg, "--seed", str(SEED), "--out", out, "--quiet", "--stats", *flags], capture_output=True, text=True,
                       timeout=900, env=dict(os.environ, **(env or {})))
    if ok:
        assert r.returncode == 0, r.stderr[-2000:]
    return r


def stat(stderr, key):
    return int(re.search(key + r"=(-?\d+)", stderr).group(1))


def stems(d):
    return sorted(x[:-len(".truth.bam")] for x in os.listdir(d) if x.endswith(".truth.bam"))


def fastq_of_stem(d, stem):
    """The stem's reads in record order: SE one file; PE mate 1 then mate 2 of every fragment."""
    se = os.path.join(d, stem + ".fq")
    if os.path.exists(se):
        return U.read_fastq(se)
    a, b = U.read_fastq(os.path.join(d, stem + "_1.fq")), U.read_fastq(os.path.join(d, stem + "_2.fq"))
    assert len(a) == len(b)
    return [x for pair in zip(a, b) for x in pair]


# ---------------------------------------------------------------------------------------------------------------------
# 1. records equal the FASTQ
# ---------------------------------------------------------------------------------------------------------------------
def _shape_cfg(shape, layout):
    return lambda wd: PS.build_shape_case(shape, wd, layout)


RUNS = {
    "k3_b53_PE_fast_kernel": _shape_cfg(Shape(3, 53), "PE"),
    "k3_b52_SE_fast_kernel": _shape_cfg(Shape(3, 52), "SE"),
    "k5_b10_PE": _shape_cfg(Shape(5, 10), "PE"),
    "k2_b409_L410_PE": lambda wd: PS.build_shape_case(Shape(2, 409, read_length=410), wd, "PE", coverage=12),
    "wgs_pe_variants": lambda wd: cases.build_case("wgs_pe_variants", wd),
    "wes_pe_targets": lambda wd: cases.build_case("wes_pe_targets", wd),
    "tumor_se_mixture": lambda wd: cases.build_case("tumor_se_mixture", wd),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_records_equal_the_fastq(name, oracle_lib, tmp_path):
    wd = str(tmp_path)
    cfg = RUNS[name](wd)
    odir, gdir, pdir = os.path.join(wd, "oracle_out"), os.path.join(wd, "truth_out"), os.path.join(wd, "plain_out")
    assert oracle_lib.orc_simulate(cfg.encode(), 1, cases.FAKE_SEC, cases.FAKE_NSEC, odir.encode(), 8) == 0, oracle_lib.orc_last_error().decode()
    n_reads = oracle_lib.orc_last_read_count()
    err = simu(cfg, gdir, "--truth-bam").stderr
    simu(cfg, pdir)
    # the FASTQ files are those of a run without the option, and the oracle's
    fq = sorted(x for x in os.listdir(pdir))
    assert fq and fq == sorted(x for x in os.listdir(gdir) if not x.endswith(".truth.bam")) == sorted(os.listdir(odir))
    for f in fq:
        a = open(os.path.join(pdir, f), "rb").read()
        assert a == open(os.path.join(gdir, f), "rb").read() == open(os.path.join(odir, f), "rb").read(), f
    total = unmapped = 0
    assert stems(gdir)
    for stem in stems(gdir):
        text, refs, recs, _ = U.read_truth_bam(os.path.join(gdir, stem + ".truth.bam"))
        assert text.startswith(b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n") and text.endswith(b"@PG\tID:simuReads\n")
        assert [ln for ln in text.split(b"\n") if ln.startswith(b"@SQ")] == [b"@SQ\tSN:%s\tLN:%d" % r for r in refs] and refs
        # one reference per FASTA contig in file order, under the first token of its header line (`chr20`, not the `20` of
        # the read names), with its length
        assert refs == U.fasta_contigs(re.search(r"^ref = (\S+)", open(cfg).read(), re.M).group(1))
        want = fastq_of_stem(odir, stem)
        assert len(recs) == len(want)
        paired = not os.path.exists(os.path.join(odir, stem + ".fq"))
        for i, (rec, (nm, seq, qual)) in enumerate(zip(recs, want)):
            if paired:
                assert nm.endswith(b"/1" if i % 2 == 0 else b"/2")
                nm = nm[:-2]
            assert U.fastq_view(rec) == (nm, seq, qual), (stem, i, rec, nm)
            assert sum(n for n, o in rec["ops"] if o in (0, 1, 4)) == (len(seq) if rec["ops"] else 0)
            unmapped += not rec["ops"]
        total += len(recs)
    assert total == n_reads == stat(err, "reads") == stat(err, "truth_records") and total > 1000
    assert unmapped == stat(err, "truth_unmapped") and unmapped < total // 10
    assert stat(err, "truth_bytes") > 100 * total and 0 < stat(err, "truth_bgzf_bytes") < stat(err, "truth_bytes")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the device states the host rule
# ---------------------------------------------------------------------------------------------------------------------
# the smallest passes: one read, and 257 reads -- the scan of the record lengths takes 256 values a block
FEW_READS = {"wgs_se_hs2000_1_read": 1, "wgs_se_hs2000_257_reads": 257}


def _reads_that_give(sess, slots):
    """the read count whose first chromosome's pass has exactly `slots` fragment slots"""
    for reads in range(max(1, slots - 2), 2 * slots + 8):
        sess.set_reads(reads)
        if sess.prepare_batch(0) and sess.batch_slots == slots:
            return reads
    pytest.fail("no set_reads() value gives %d slots" % slots)


@pytest.mark.parametrize("name", ["k3_b53_PE_fast_kernel", "k3_b52_SE_fast_kernel", "k5_b10_PE", "wgs_pe_variants", "wes_pe_targets"] + list(FEW_READS))
def test_device_records_follow_the_host_rule(name, tmp_path):
    wd = str(tmp_path)
    few = FEW_READS.get(name)
    cfg = cases.build_case("wgs_se_hs2000", wd) if few else RUNS[name](wd)
    paired = "layout = PE" in open(cfg).read()
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=SEED, truth_bam=1) as sess:
        L = None
        sess.weighted_length()
        sess.set_reads(_reads_that_give(sess, few) if few else sess.planned_reads)
        checked = with_events = gapped = clipped = 0
        for chrom in range(1 if few else sess.n_chromosomes):
            if not sess.prepare_batch(chrom):
                continue
            sess.sample()
            sess.result()
            n = sess.batch_slots
            rb, gb = sess.truth_bam()
            stream = sess.fetch_truth(False, rb)
            assert U.inflate_members(sess.fetch_truth(True, gb), want_eof=False) == stream
            recs = U.records_of_stream(stream)
            assert sess.truth_info()[0] == len(recs)
            rows = [sess.truth_reads(m, 0, n) for m in range(2 if paired else 1)]
            pieces = {}
            it = iter(recs)
            for t in range(n):
                alns = []
                for m in range(len(rows)):
                    r = rows[m][t]
                    if not r.live:
                        continue
                    if r.chain not in pieces:
                        pieces[r.chain] = sess.truth_pieces(r.chain)
                    if L is None:
                        L = int(re.search(r"readLength: (\d+)", open(re.search(r"profile = (\S+)", open(cfg).read()).group(1)).read()).group(1))
                    ev = [r.events[e] for e in range(r.n_events)]
                    a = simuscop_amd.truth_align(pieces[r.chain], r.tmpl_off, L, bool(r.reverse), ev) if r.inside else (-1, -1, [])
                    alns.append((m, r, a))
                    with_events += bool(ev)
                assert len(alns) in (0, len(rows))
                for k, (m, r, a) in enumerate(alns):
                    rec = next(it)
                    want = U.expected_pair_fields(a, paired, m, bool(r.reverse), alns[1 - k][2] if paired else None)
                    got = {key: rec[key] for key in want}
                    assert got == want and rec["ops"] == a[2], (chrom, t, m, rec, a, want)
                    assert len(rec["seq"]) == r.read_len
                    checked += 1
                    gapped += any(o in (2, 3) for _, o in a[2])
                    clipped += any(o == 4 for _, o in a[2])
            assert next(it, None) is None
        if few:
            assert 0 < checked <= few
        else:
            assert checked > 1000 and with_events > 20, (checked, with_events, gapped, clipped)
        if name in ("wgs_pe_variants", "wes_pe_targets"):
            assert gapped > 0


def test_calls_without_a_piece_map_are_refused():
    eng = simuscop_amd.load_engine()
    ctx = C.c_void_p()
    assert eng.sg_create(C.byref(ctx), 0, 1) == 0
    try:
        chain = b"ACGT" * 1000
        arr = (C.c_char_p * 1)(chain)
        lens = (C.c_uint64 * 1)(len(chain))
        assert eng.sg_upload_haplotypes(ctx, 1, arr, lens) == 0
        flags = b"\1"
        piece = (simuscop_amd.SgHapPiece * 1)(simuscop_amd.SgHapPiece(0, 0, len(chain), 0, 0, 0))
        assert eng.sg_truth_map(ctx, piece, flags, 1, None, 0) != 0 and b"piece map" in eng.sg_last_error(ctx)
        a, b = C.c_uint64(), C.c_uint64()
        assert eng.sg_truth_bam(ctx, C.byref(a), C.byref(b)) != 0 and b"piece map" in eng.sg_last_error(ctx)
        assert eng.sg_truth_reads(ctx, 0, 0, 0, None) != 0 and b"piece map" in eng.sg_last_error(ctx)
        assert eng.sg_fetch_truth(ctx, 0, 0, 0, None) != 0
    finally:
        eng.sg_destroy(ctx)


def test_a_refused_map_leaves_the_earlier_one():
    """sg_truth_map checks the whole piece list before it changes the context: pieces that do not tile their chain (one
    of length 0 among them), another count than sg_build_haplotypes had, a contig without a reference id."""
    import test_gpu_haplotypes as H
    eng = simuscop_amd.load_engine()
    ctx = H._ctx(eng)
    try:
        seq = synth.synth_contig(5000, 3, 0, n_runs=False).tobytes()
        image, rows = H._fasta_image([(b"chr1", seq)], 60)
        H._upload(eng, ctx, image)
        tab = (simuscop_amd.SgContig * 1)(simuscop_amd.SgContig(rows[0][1], len(seq), 60, 61))
        assert eng.sg_reference_commit(ctx, tab, 1) == 0, eng.sg_last_error(ctx)
        P = simuscop_amd.SgHapPiece
        good = [(300, 1000, 200, 0, 0, 0), (0, 100, 300, 0, 0, 0), (0, 2000, 400, 1, 0, 0)]    # (dst, src, len, chain, contig, kind)
        lens = (C.c_uint64 * 2)(500, 400)
        arr = (P * 3)(*[P(*p) for p in good])
        assert eng.sg_build_haplotypes(ctx, 2, lens, arr, 3, None, 0, None, 0) == 0, eng.sg_last_error(ctx)
        ids = (C.c_int32 * 1)(7)
        assert eng.sg_truth_map(ctx, arr, b"\0\1\1", 3, ids, 1) == 0, eng.sg_last_error(ctx)

        def mapped():
            out = []
            for chain in range(2):
                buf, n = (simuscop_amd.SgTruthPiece * 4)(), C.c_uint64()
                assert eng.sg_truth_pieces(ctx, chain, buf, 4, C.byref(n)) == 0, eng.sg_last_error(ctx)
                out.append([(p.dst, p.src, p.len, p.contig, p.kind, p.seg_first) for p in buf[:n.value]])
            return out
        first = mapped()
        assert first == [[(0, 100, 300, 0, 0, 1), (300, 1000, 200, 0, 0, 0)], [(0, 2000, 400, 0, 0, 1)]]
        for bad, n, ref, word in (
                ([(0, 100, 500, 0, 0, 0), (500, 1000, 0, 0, 0, 0), (0, 2000, 400, 1, 0, 0)], 3, ids, b"tile"),   # a piece of length 0
                ([(0, 100, 300, 0, 0, 0), (310, 1000, 190, 0, 0, 0), (0, 2000, 400, 1, 0, 0)], 3, ids, b"tile"),   # a hole
                ([(0, 100, 300, 0, 0, 0), (300, 1000, 200, 0, 0, 0), (0, 2000, 300, 1, 0, 0)], 3, ids, b"tile"),   # a chain's end left out
                (good[:2], 2, ids, b"count"),
                ([(300, 1000, 200, 0, 0, 0), (0, 100, 300, 0, 0, 0), (0, 2000, 400, 1, 1, 0)], 3, ids, b"ref_ids"),  # the last piece's contig
                (good, 3, (C.c_int32 * 1)(-1), b"reference id")):
            a = (P * len(bad))(*[P(*p) for p in bad])
            assert eng.sg_truth_map(ctx, a, b"\1\1\1", n, ref, 1) != 0
            assert word in eng.sg_last_error(ctx), eng.sg_last_error(ctx)
            assert mapped() == first
    finally:
        eng.sg_destroy(ctx)


def test_sq_names_are_the_first_tokens_of_the_fasta(tmp_path):
    """@SQ: one line per contig in file order, named as the file names it -- prefix, case and all, whatever stands behind
    the first blank left out.  A contig whose key the file holds again (`3` after `chr3`) is listed once: no read comes
    from the second sequence, and SAM wants every SN once.  The records' refIDs are indexes of that list."""
    wd = str(tmp_path)
    prof = U.write_identity_profile(os.path.join(wd, "identity.profile"), Shape(3, 53))
    cfg, fa, seqs = U.acgt_case(wd, prof, "SE")
    body = {k: v for k, v in seqs.items()}
    extra = synth.synth_contig(30000, 6, 9, n_runs=False).tobytes().upper()
    cases._fasta_of(fa, [(b"chr3 first of two", body["chr3"]), (b"Contig_8\tx=1", body["chr8"]), (b"3", extra), (b"chrom11", extra[:9000])])
    out = os.path.join(wd, "out")
    simu(cfg, out, "--truth-bam")
    (stem,) = stems(out)
    text, refs, recs, _ = U.read_truth_bam(os.path.join(out, stem + ".truth.bam"))
    assert refs == [(b"chr3", len(body["chr3"])), (b"Contig_8", len(body["chr8"])), (b"chrom11", 9000)]
    assert [ln for ln in text.split(b"\n") if ln.startswith(b"@SQ")] == [b"@SQ\tSN:%s\tLN:%d" % r for r in refs]
    by_name = {"chr3": body["chr3"], "Contig_8": body["chr8"], "chrom11": extra[:9000]}
    m_bases, bad = _replay(recs, refs, by_name)
    assert bad == 0 and m_bases > 100 * len(recs) and {rec["rid"] for rec in recs} == {0, 1, 2}


# ---------------------------------------------------------------------------------------------------------------------
# 3. replay
# ---------------------------------------------------------------------------------------------------------------------
def _replay(recs, refs, seqs, alleles=None):
    """Every M base of every mapped record against the reference; returns (M bases, mismatches not explained by `alleles`)."""
    m_bases = bad = 0
    for rec in recs:
        if not rec["ops"]:
            continue
        ref = seqs[refs[rec["rid"]][0].decode()]      # (by the FASTA's own name for the contig)
        alt = (alleles or {}).get(refs[rec["rid"]][0].decode(), {})
        q, p = 0, rec["pos"]
        for n, o in rec["ops"]:
            if o == 0:
                s, r = rec["seq"][q:q + n], ref[p:p + n]
                assert len(r) == n, "an alignment runs off its contig"
                if s != r:
                    for i in range(n):
                        if s[i] != r[i] and chr(s[i]) not in alt.get(p + i, ()):
                            bad += 1
                m_bases += n
                q += n
                p += n
            elif o in (1, 4):
                q += n
            else:
                p += n
        assert q == len(rec["seq"])
    return m_bases, bad


@pytest.mark.parametrize("layout,shape", [("PE", Shape(3, 53)), ("SE", Shape(5, 10)), ("PE", Shape(3, 54))], ids=["PE_fast", "SE_k5", "PE_k3_generic"])
def test_replay_without_substitutions(layout, shape, oracle_lib, tmp_path):
    wd = str(tmp_path)
    prof = U.write_identity_profile(os.path.join(wd, "identity.profile"), shape)
    cfg, fa, seqs = U.acgt_case(wd, prof, layout)
    out, odir = os.path.join(wd, "out"), os.path.join(wd, "oracle_out")
    assert oracle_lib.orc_simulate(cfg.encode(), 1, cases.FAKE_SEC, cases.FAKE_NSEC, odir.encode(), 8) == 0, oracle_lib.orc_last_error().decode()
    simu(cfg, out, "--truth-bam")
    (stem,) = stems(out)
    _, refs, recs, _ = U.read_truth_bam(os.path.join(out, stem + ".truth.bam"))
    m_bases, bad = _replay(recs, refs, seqs)
    assert bad == 0 and m_bases > 100 * len(recs) and len(recs) > 1000
    assert all(rec["ops"] for rec in recs), "a read of a variant-free genome without an alignment"
    # The events by size, taken twice.  From the oracle's FASTQ records alone: a read of L + k bases gained k, one of
    # L - k lost k (no CIGAR is looked at).  From the CIGARs alone: the template is L reference bases, so a record
    # gained its I and S bases, lost its D bases, and lost what its M and D bases leave of L (template bases deleted
    # at an end, where the rule drops the D).  Every record is in both counts; one whose M and D bases pass L has no place
    # in the second and fails.  A record with one event -- nearly all that have any -- counts under that event's length.
    L = shape.read_length
    fq = fastq_of_stem(odir, stem)
    assert len(fq) == len(recs)
    by_length = collections.Counter(len(seq) - L for _, seq, _ in fq)
    by_cigar, ops_by_length = collections.Counter(), collections.Counter()
    for rec in recs:
        total = collections.Counter()
        for n, o in rec["ops"]:
            assert o in (0, 1, 2, 4), rec       # (no variant, no target: nothing else can stand here)
            total[o] += n
            if o != 0:
                ops_by_length["D" if o == 2 else "I", n] += 1
        at_an_end = L - total[0] - total[2]
        assert at_an_end >= 0, ("more reference under a read than its template has", rec)
        by_cigar[total[1] + total[4] - total[2] - at_an_end] += 1
    print("net length change: records", sorted(by_length.items()), "\nCIGAR operations by length", sorted(ops_by_length.items()))
    assert by_cigar == by_length
    assert sum(v for k, v in by_length.items() if k > 0) > 10 and sum(v for k, v in by_length.items() if k < 0) > 10, by_length
    if layout == "PE":   # mates of one fragment: same name, facing each other, TLEN the fragment
        for a, b in zip(recs[0::2], recs[1::2]):
            assert a["name"] == b["name"] and a["flag"] == 99 and b["flag"] == 147 and a["tlen"] == -b["tlen"] > 0
            assert a["npos"] == b["pos"] and b["npos"] == a["pos"] and a["pos"] <= b["pos"]


def test_replay_with_variants(tmp_path):
    wd = str(tmp_path)
    prof = U.write_identity_profile(os.path.join(wd, "identity.profile"), Shape(3, 53))
    cfg, fa, seqs = U.acgt_case(wd, prof, "PE", variants=True, coverage=10)
    out = os.path.join(wd, "out")
    simu(cfg, out, "--truth-bam")
    (stem,) = stems(out)
    _, refs, recs, _ = U.read_truth_bam(os.path.join(out, stem + ".truth.bam"))
    alleles = U.known_alleles(wd)
    m_bases, bad = _replay(recs, refs, seqs, alleles)
    _, unexplained = _replay(recs, refs, seqs)
    assert bad == 0 and unexplained > 0 and len(recs) > 1000   # (the alternative alleles are in the reads)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the loop through the project's own trainer
# ---------------------------------------------------------------------------------------------------------------------
def _train_cli(args):
    r = subprocess.run([TRAIN, *args, "--quiet", "--stats"], capture_output=True, timeout=900)
    st = [json.loads(x) for x in r.stderr.decode(errors="replace").splitlines() if x.startswith("{")]
    return r, st[-1] if st else None


def _closed_loop(oracle_lib, wd, prof, insert):
    """PE truth BAM of a variant-free ACGT genome -> (bam path, fasta, empty vcf, view text, records)."""
    cfg, fa, seqs = U.acgt_case(wd, prof, "PE", coverage=30, insert=insert, lengths=(400000, 60000))
    out = os.path.join(wd, "out")
    simu(cfg, out, "--truth-bam")
    (stem,) = stems(out)
    bam = os.path.join(out, stem + ".truth.bam")
    _, refs, recs, d = U.read_truth_bam(bam)
    vcf = os.path.join(wd, "empty.vcf")
    open(vcf, "w").write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n")
    return bam, fa, vcf, B.view(d), recs


def test_closed_loop_through_the_trainer(oracle_lib, tmp_path):
    import test_gpu_train as G
    import test_train_profile_cpu as TP
    TP.declare(oracle_lib)
    wd = str(tmp_path)
    shape = Shape(3, 50)
    prof = U.write_identity_profile(os.path.join(wd, "identity.profile"), shape)
    bam, fa, vcf, sam, recs = _closed_loop(oracle_lib, wd, prof, 400)
    assert sam.count(b"\n") == len(recs) > 50_000     # every record passes `-F 0xD04 -q 20`
    sam_path = os.path.join(wd, "view.sam")
    open(sam_path, "wb").write(sam)
    # the trainer's whole run on the BAM file = the restatement's on the lines of that file
    want, got = os.path.join(wd, "want.profile"), os.path.join(wd, "got.profile")
    assert oracle_lib.orc_train_profile(sam, len(sam), fa.encode(), vcf.encode(), b"", b"ACTG", 3, 50, want.encode(), sam_path.encode(), b"stamp\n") == 0
    r, st = _train_cli(["-b", bam, "--decode-bam", "-v", vcf, "-r", fa, "-o", got])
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(got, "rb").read().split(b"\n", 2)[2] == open(want, "rb").read().split(b"\n", 2)[2]
    # (how many reads the trainer's countGC gate lets through on simulated data nobody has measured: any is enough here;
    # the counters below are taken with the gate off)
    assert st["lines"] == len(recs) and st["reads_counted"] > 0 and st.get("bam_records", len(recs)) == len(recs)
    # the counters, every read through the filters (count_gc = 0): device = restatement; no substitution was counted;
    # the indel events are the I and D operations of the records
    oracle_lib.orc_train_count.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32,
                                           C.POINTER(simuscop_amd.SgTrainCounts)]
    kc = 4 + 16 + 64
    wantc, wa = TU.count_arrays(simuscop_amd.SgTrainCounts, kc, 50, 1024)
    assert oracle_lib.orc_train_count(sam, len(sam), fa.encode(), b"ACTG", 3, 50, 1024, 256, C.byref(wantc)) == 0
    eng = simuscop_amd.load_engine()
    ctx = C.c_void_p()
    assert eng.sg_create(C.byref(ctx), 0, 1) == 0
    try:
        keys = G._reference_on_device(eng, ctx, fa)
        gotc, ga = TU.count_arrays(simuscop_amd.SgTrainCounts, kc, 50, 1024)
        karr = (C.c_char_p * len(keys))(*keys)
        assert eng.sg_train_count(ctx, sam, len(sam), karr, len(keys), b"ACTG", 3, 50, 1024, 256, C.byref(gotc)) == 0, eng.sg_last_error(ctx)
        G._same_counts(gotc, ga, wantc, wa)
    finally:
        eng.sg_destroy(ctx)
    for key in ("subs1", "subs2"):
        t = wa[key].reshape(kc, 50, 4)
        names = PS.kmer_names(3, "ACTG")
        off = sum(int(t[c, :, k].sum()) for c in range(kc) for k in range(4) if k != "ACTG".index(names[c][-1]))
        assert off == 0 and t.sum() > 1_000_000, (key, off, int(t.sum()))
    assert wantc.insert_events == sum(1 for rec in recs for _, o in rec["ops"] if o == 1) > 100
    assert wantc.delete_events == sum(1 for rec in recs for _, o in rec["ops"] if o == 2) > 100


def test_closed_loop_on_a_shipped_profile_report(oracle_lib, tmp_path):
    """HiSeqXTen -> reads -> truth BAM -> seqToProfile: the run must work; what the trained profile's rates are beside the
    generating one's is written to the evidence directory (TRUTH_EVIDENCE_DIR), no threshold: nobody has measured what the
    trainer's own filters (countGC, single-nM reads only) do to simulated data."""
    wd = str(tmp_path)
    src = os.path.join(cases.TESTDATA, cases.PROFILES["xten"])
    cfg, fa, seqs = U.acgt_case(wd, src, "PE", coverage=30, insert=350, lengths=(400000, 60000))
    out = os.path.join(wd, "out")
    simu(cfg, out, "--truth-bam")
    (stem,) = stems(out)
    vcf = os.path.join(wd, "empty.vcf")
    open(vcf, "w").write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n")
    got = os.path.join(wd, "trained.profile")
    r, st = _train_cli(["-b", os.path.join(out, stem + ".truth.bam"), "--decode-bam", "-v", vcf, "-r", fa, "-o", got])
    assert r.returncode == 0 and st["reads_counted"] > 0, r.stderr[-2000:]

    def rates(path):
        secs, cur = {}, None
        for ln in open(path).read().split("\n"):
            if ln.startswith("["):
                cur = ln
                secs[cur] = []
            elif cur and ln.strip():
                secs[cur].append(ln)
        bins = int(re.search(r"binCount: (\d+)", open(path).read()).group(1))
        sub = np.zeros(bins)
        rows, ident = 0, None
        k = 0
        for ln in secs["[Substitution Probs]"]:
            if ln.startswith("kmer:"):
                ident, k = "ACTG".index(ln.split(":")[1].strip()[-1]), 0
                continue
            v = [float(x) for x in ln.split("\t")]
            if k < bins and sum(v) > 0:      # mate 1 rows
                sub[k] += 1.0 - v[ident] / sum(v)
                rows += k == 0
            k += 1
        return dict(insert_rate=float(secs["[Insert Rate]"][0]), delete_rate=float(secs["[Deletion Rate]"][0]),
                    mate1_error_by_bin=(sub / max(rows, 1)).round(6).tolist())
    rep = dict(generating=rates(src), trained=rates(got), trainer_stats=st)
    if EVIDENCE:
        os.makedirs(EVIDENCE, exist_ok=True)
        with open(os.path.join(EVIDENCE, "closed_loop_xten.json"), "w") as f:
            json.dump(rep, f, indent=1)
    print(json.dumps(rep)[:2000])


# ---------------------------------------------------------------------------------------------------------------------
# 5. sharding and refusal
# ---------------------------------------------------------------------------------------------------------------------
def test_sharded_runs_give_the_same_records(tmp_path):
    wd = str(tmp_path)
    cfg = cases.build_case("wgs_pe_variants", wd)
    one = os.path.join(wd, "one")
    simu(cfg, one, "--truth-bam")
    (stem,) = stems(one)
    text, refs, recs, d1 = U.read_truth_bam(os.path.join(one, stem + ".truth.bam"))
    # two ranks by hand: parts; the header in part 0 only, the EOF block in the last part only
    two = os.path.join(wd, "two")
    for r in range(2):
        simu(cfg, two, "--truth-bam", "--rank", str(r), "--world", "2")
    p0 = open(os.path.join(two, stem + ".truth.bam.part0"), "rb").read()
    p1 = open(os.path.join(two, stem + ".truth.bam.part1"), "rb").read()
    assert p0[-28:] != B.EOF_MEMBER and p1[-28:] == B.EOF_MEMBER
    assert U.inflate_members(p1)[:4] != b"BAM\1"
    # the parts hold the records of the one-rank run: every rank samples its run of segments of EVERY batch, so the parts
    # in rank order are the same records in another order (as the FASTQ parts are); mates stay next to each other
    def sorted_records(d):
        return sorted(r for _, r in B.parse_stream(d)[1])
    hdr_end = B.parse_stream(d1)[1][0][0]
    d2 = U.inflate_members(p0 + p1)
    assert d2[:hdr_end] == d1[:hdr_end] and sorted_records(d2) == sorted_records(d1)
    r2 = [U.parse_record(r) for _, r in B.parse_stream(d2)[1]]
    assert all(a["name"] == b["name"] and a["flag"] & 0x40 and b["flag"] & 0x80 for a, b in zip(r2[0::2], r2[1::2]))
    # --gpus 2 (both children on this device): merged like the FASTQ parts
    both = os.path.join(wd, "both")
    simu(cfg, both, "--truth-bam", "--gpus", "2", env={"SIMUSCOP_SAME_DEVICE": "1"})
    assert sorted(os.listdir(both)) == sorted(os.listdir(one))
    assert U.read_truth_bam(os.path.join(both, stem + ".truth.bam"))[3] == d2    # the two parts, merged: one header, one EOF block
    # with --gzip both kinds of file end in one EOF block
    gz = os.path.join(wd, "gz")
    simu(cfg, gz, "--truth-bam", "--gzip", "--gpus", "2", env={"SIMUSCOP_SAME_DEVICE": "1"})
    assert U.read_truth_bam(os.path.join(gz, stem + ".truth.bam"))[3] == d2
    for f in os.listdir(gz):
        assert open(os.path.join(gz, f), "rb").read().count(B.EOF_MEMBER) >= 1 and open(os.path.join(gz, f), "rb").read()[-28:] == B.EOF_MEMBER


def test_refused_and_unwritten(tmp_path):
    wd = str(tmp_path)
    cfg = cases.build_case("wgs_pe_xten", wd)
    r = simu(cfg, os.path.join(wd, "a"), "--truth-bam", "--host-haplotypes", ok=False)
    assert r.returncode != 0 and "--truth-bam" in r.stderr and "--host-haplotypes" in r.stderr
    assert not os.path.exists(os.path.join(wd, "a")) or not os.listdir(os.path.join(wd, "a"))
    r = simu(cfg, os.path.join(wd, "b"), "--truth-bam", "--no-write")
    assert stat(r.stderr, "truth_records") == stat(r.stderr, "reads") > 1000 and stat(r.stderr, "truth_bgzf_bytes") > 0
    assert not os.path.exists(os.path.join(wd, "b")) or not os.listdir(os.path.join(wd, "b"))
    # without the option: no records, and the fields are there
    r = simu(cfg, os.path.join(wd, "c"))
    assert stat(r.stderr, "truth_records") == 0 and stat(r.stderr, "truth_bytes") == 0
    assert not [x for x in os.listdir(os.path.join(wd, "c")) if "truth" in x]
    # in process, through simu_run
    st = simuscop_amd.run_config(cfg, seed=SEED, output_dir=os.path.join(wd, "d"), quiet=1, truth_bam=1)
    assert st.truth_records == st.reads and stems(os.path.join(wd, "d"))
    with pytest.raises(simuscop_amd.SimuError, match="--host-haplotypes"):
        simuscop_amd.run_config(cfg, seed=SEED, output_dir=os.path.join(wd, "e"), quiet=1, truth_bam=1, host_haplotypes=1)
