"""GPU box: how fast the training path takes SAM text (SURVEY 8(f)-4 measurement).  Reads sampled by the engine on a 1.4 Mbp
contig (40x, XTen PE) become `samtools view` lines sorted by position; K contigs chr1..chrK of that one sequence and K copies
of the lines (contig field rewritten) make a text of K x 250 MB.  Prints the --stats line of `seqToProfile` and GB/s of SAM
text through the kernels; with `rocprofv3 --kernel-trace --stats -- python3 tools/train_bench.py` the per-kernel times.
--bam: the same reads written as BAM (tests/bam_util.py, BGZF members of 65,280 bytes at zlib levels 1 and 6) and read by
`seqToProfile -b x.bam --decode-bam` (BGZF inflate, record boundaries and rendering on the GPU): compressed GB/s and records/s
end to end, next to the --sam figures, and the profile checked against the --sam one.
--vcf or --vcf=ROWS: the VCF of known variants (default 5,000,000 rows, what a single-sample whole-genome call set holds): a synthetic
single-sample file on the bench's contigs with the INFO and FORMAT fields a caller writes, plain and as BGZF at zlib levels 1
and 6, read by the host's fgets loop (`-v x.vcf`, the yardstick), by `-v x.vcf --device-vcf` and by `-v x.vcf.gz`, alternated
three times: t_vcf and t_total of every run, the raw --stats lines, the profiles checked against the host route's.
usage: python tools/train_bench.py [--bam] [--vcf | --vcf=ROWS] [K=8] [workdir]"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases  # noqa: E402
import histo_util as H  # noqa: E402
import train_util as TU  # noqa: E402

BAM = "--bam" in sys.argv
ARGS = [a for a in sys.argv[1:] if a != "--bam"]
VCF_ROWS = 0
for a in [a for a in ARGS if a == "--vcf" or a.startswith("--vcf=")]:   # --vcf: 5,000,000 rows; --vcf=ROWS
    VCF_ROWS = int(a[6:]) if a.startswith("--vcf=") else 5000000
    ARGS.remove(a)
K = int(ARGS[0]) if len(ARGS) > 0 else 8
wd = ARGS[1] if len(ARGS) > 1 else tempfile.mkdtemp(prefix="trainbench_")
os.makedirs(wd, exist_ok=True)
SIMU = os.path.join(ROOT, "simuscop_amd", "lib", "simuReads")
EXE = os.path.join(ROOT, "simuscop_amd", "lib", "seqToProfile")
sam_path, fa_path, vcf_path = os.path.join(wd, "reads.sam"), os.path.join(wd, "ref.fa"), os.path.join(wd, "none.vcf")
if not os.path.exists(sam_path):
    t0 = time.time()
    cfg, fa1 = H.histogram_config(cases, wd, "xten", "PE", 40, 350)
    out = os.path.join(wd, "gpu")
    subprocess.run([SIMU, cfg, "--seed", "78", "--out", out, "--quiet"], check=True)
    L, isz_max = 151, 551   # HiSeqXTen profile, insertSize 350: the support of its insert-size law (Profile.cpp:912-930)
    ref = H.read_fasta_one(fa1)
    f1, f2 = sorted(os.path.join(out, f) for f in os.listdir(out))
    lines = TU.sam_from_pairs(ref, H.Fastq(f1), H.Fastq(f2), L, isz_max, cuts=(10 ** 9, 10 ** 9))
    lines.sort(key=lambda l: int(l.split(b"\t", 4)[3]))
    text = b"\n".join(lines) + b"\n"
    seq = open(fa1, "rb").read().split(b"\n", 1)[1]
    with open(fa_path, "wb") as f, open(sam_path, "wb") as s:
        for k in range(1, K + 1):
            f.write(b">chr%d\n" % k + seq)
            s.write(text.replace(b"\tchr1\t", b"\tchr%d\t" % k))
    open(vcf_path, "w").write("##fileformat=VCFv4.2\n")
    print("inputs made in %.1f s: %d lines x %d" % (time.time() - t0, len(lines), K), file=sys.stderr)
best = None
for rep in range(3):
    r = subprocess.run([EXE, "--sam", sam_path, "-v", vcf_path, "-r", fa_path, "-o", os.path.join(wd, "out.profile"), "--quiet", "--stats"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    st = json.loads(r.stderr.strip().split("\n")[-1])
    st["sam_GBps_through_the_kernels"] = st["sam_bytes"] / st["t_reads"] / 1e9
    st["lines_per_s"] = st["lines"] / st["t_reads"]
    if best is None or st["t_reads"] < best["t_reads"]:
        best = st
print(json.dumps(best))


def _bgzf_part(args):
    import bam_util as B
    data, level = args
    return b"".join(B.bgzf_member(data[i:i + 65280], level) for i in range(0, len(data), 65280))


def _vcf_part(args):
    """`n` rows on contig `name` from position `first` on, `step` apart: nine in ten are SNVs, the rest short insertions and
    deletions; INFO and FORMAT as a germline caller writes them; a few rows below the depth and quality thresholds."""
    import random
    name, first, step, n, seed = args
    rng = random.Random(seed)
    out = []
    for i in range(n):
        r = rng.random()
        ref, alt = ("ACGT"[rng.randrange(4)], "ACGT"[rng.randrange(4)]) if r < 0.9 else (("A", "A" + "CGT"[:rng.randrange(1, 4)]) if r < 0.95 else ("G" + "TCA"[:rng.randrange(1, 4)], "G"))
        dp, hom = rng.randrange(6, 70), rng.random() < 0.4
        alt_n = dp if hom else dp // 2
        qual = rng.uniform(12, 2500)
        out.append("%s\t%d\t.\t%s\t%s\t%.2f\t.\tAC=%d;AF=%s;AN=2;BaseQRankSum=%.3f;DP=%d;ExcessHet=3.0103;FS=%.3f;MLEAC=%d;MLEAF=%s;MQ=60.00;MQRankSum=0.000;"
                   "QD=%.2f;ReadPosRankSum=%.3f;SOR=%.3f\tGT:AD:DP:GQ:PL\t%s:%d,%d:%d:%d:%d,%d,%d\n" %
                   (name, first + i * step, ref, alt, qual, 2 if hom else 1, "1.00" if hom else "0.500", rng.uniform(-3, 3), dp, rng.uniform(0, 9),
                    2 if hom else 1, "1.00" if hom else "0.500", qual / dp, rng.uniform(-3, 3), rng.uniform(0.1, 3), "1/1" if hom else "0/1",
                    dp - alt_n, alt_n, dp, min(99, int(qual / 10)), int(qual), 0 if not hom else int(qual / 12), int(qual * 0.9)))
    return "".join(out).encode()


def write_vcf(path, rows):
    """The synthetic call set: rows at distinct, ascending positions on the bench's contigs as far as they have room, the rest
    on contigs the FASTA lacks (counted, not kept)."""
    import multiprocessing
    seq_len = len(open(fa_path, "rb").read().split(b">chr2")[0].split(b"\n", 1)[1].replace(b"\n", b""))
    per = min(rows // K, seq_len - 2000)
    tasks, left, extra = [], rows, 0
    while left > 0:
        on_ref = len(tasks) // 4 < K
        name = "chr%d" % (len(tasks) // 4 + 1) if on_ref else "chrU%d" % extra
        extra += 0 if on_ref else 1
        n = min(left, (per + 3) // 4)
        step = max(1, (seq_len - 2000) // per)
        tasks.append((name, 1000 + (len(tasks) % 4) * ((per + 3) // 4) * step if on_ref else 1000, step, n, 1000 + len(tasks)))
        left -= n
    head = "##fileformat=VCFv4.2\n" + "".join("##contig=<ID=chr%d,length=%d>\n" % (k, seq_len) for k in range(1, K + 1)) + \
           '##INFO=<ID=DP,Number=1,Type=Integer,Description="Approximate read depth">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n'
    with multiprocessing.Pool(16) as pool:
        parts = pool.map(_vcf_part, tasks)
        text = head.encode() + b"".join(parts)
        open(path, "wb").write(text)
        step = 65280 * 256
        for level in (1, 6):
            blobs = pool.map(_bgzf_part, [(text[i:i + step], level) for i in range(0, len(text), step)])
            import bam_util as B
            open(path + ".l%d.gz" % level, "wb").write(b"".join(blobs) + B.EOF_MEMBER)
    return len(text)


if VCF_ROWS:
    big = os.path.join(wd, "bench_%d.vcf" % VCF_ROWS)
    if not os.path.exists(big + ".l6.gz"):
        t0 = time.time()
        n_text = write_vcf(big, VCF_ROWS)
        print("VCF of %d rows made in %.1f s: %d bytes of text, %d / %d at levels 1 / 6" %
              (VCF_ROWS, time.time() - t0, n_text, os.path.getsize(big + ".l1.gz"), os.path.getsize(big + ".l6.gz")), file=sys.stderr)
    routes = [("host", big, []), ("device_vcf", big, ["--device-vcf"]), ("gz_l1", big + ".l1.gz", []), ("gz_l6", big + ".l6.gz", [])]
    runs, host_body = {name: [] for name, _, _ in routes}, None
    for rep in range(3):   # alternated: every route once per round
        for name, path, extra in routes:
            out = os.path.join(wd, "vcf_%s.profile" % name)
            t0 = time.time()
            r = subprocess.run([EXE, "--sam", sam_path, "-v", path, "-r", fa_path, "-o", out, "--quiet", "--stats", *extra], capture_output=True, text=True)
            wall = time.time() - t0
            assert r.returncode == 0, r.stderr[-2000:]
            st = json.loads(r.stderr.strip().split("\n")[-1])
            st.update(route=name, rep=rep, wall=round(wall, 4), vcf_file_bytes=os.path.getsize(path))
            print(json.dumps(st))
            body = open(out, "rb").read().split(b"\n", 2)[2]
            host_body = body if host_body is None else host_body
            assert body == host_body, "profile differs from the host route's"
            assert st["vcf_on_device"] == (0 if name == "host" else 1) and st["vcf_fragments"] == VCF_ROWS + K + 3
            runs[name].append(st)
    for name, _, _ in routes:
        tv, tt = sorted(s["t_vcf"] for s in runs[name]), sorted(s["t_total"] for s in runs[name])
        print(json.dumps({"route": name, "rows": VCF_ROWS, "t_vcf": tv, "t_total": tt, "t_reads_min": min(s["t_reads"] for s in runs[name]),
                          "text_GBps_min_t_vcf": runs[name][0]["vcf_bytes"] / tv[0] / 1e9, "undecided": runs[name][0]["vcf_undecided"]}))
if not BAM:
    sys.exit(0)


def write_bam(path, level):
    """The lines of reads.sam as a BAM: chr1's records encoded once, copies for chr2..chrK with refID / next_refID patched."""
    import multiprocessing
    import numpy as np
    import bam_util as B
    sam = open(sam_path, "rb").read()
    one = [ln for ln in sam.split(b"\n") if ln and ln.split(b"\t", 3)[2] == b"chr1"]
    seq_len = len(open(fa_path, "rb").read().split(b">chr2")[0].split(b"\n", 1)[1].replace(b"\n", b""))
    refs = [(b"chr%d" % k, seq_len) for k in range(1, K + 1)]
    ref_id = {n: i for i, (n, _) in enumerate(refs)}
    recs = [B.record(ln.split(b"\t"), ref_id) for ln in one]
    offs = np.cumsum([0] + [len(r) for r in recs[:-1]])
    base = np.frombuffer(b"".join(recs), np.uint8)
    mate = base[offs + 24] != 0xFF
    parts = [B.header(refs, b"@HD\tVN:1.6\n")]
    for k in range(K):
        a = base.copy()
        a[offs + 4] = k
        a[offs[mate] + 24] = k
        parts.append(a.tobytes())
    data = b"".join(parts)
    step = 65280 * 256
    with multiprocessing.Pool(16) as pool:
        blobs = pool.map(_bgzf_part, [(data[i:i + step], level) for i in range(0, len(data), step)])
    with open(path, "wb") as f:
        f.write(b"".join(blobs) + B.EOF_MEMBER)
    return len(data)


want_body = open(os.path.join(wd, "out.profile"), "rb").read().split(b"\n", 2)[2]
for level in (1, 6):
    bam = os.path.join(wd, "reads_l%d.bam" % level)
    if not os.path.exists(bam):
        t0 = time.time()
        raw = write_bam(bam, level)
        print("BAM level %d made in %.1f s: %d bytes inflated, %d compressed" % (level, time.time() - t0, raw, os.path.getsize(bam)), file=sys.stderr)
    bb = None
    for rep in range(3):
        out = os.path.join(wd, "bam_l%d.profile" % level)
        r = subprocess.run([EXE, "-b", bam, "--decode-bam", "-v", vcf_path, "-r", fa_path, "-o", out, "--quiet", "--stats"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert open(out, "rb").read().split(b"\n", 2)[2] == want_body, "profile differs from the --sam route"
        st = json.loads(r.stderr.strip().split("\n")[-1])
        assert st["lines"] == best["lines"] and st["reads_counted"] == best["reads_counted"]
        st["level"] = level
        st["bam_GBps_end_to_end"] = st["bam_bytes"] / st["t_reads"] / 1e9
        st["records_per_s_end_to_end"] = st["bam_records"] / st["t_reads"]
        st["bam_GBps_decode_stage"] = st["bam_bytes"] / st["t_inflate"] / 1e9
        st["sam_lines_per_s_same_reads"] = best["lines_per_s"]
        if bb is None or st["t_reads"] < bb["t_reads"]:
            bb = st
    print(json.dumps(bb))
