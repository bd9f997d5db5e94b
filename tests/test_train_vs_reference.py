"""Profile training against the unmodified reference seqToProfile: the restatement of Profile::train
(oracle/train_oracle.cpp, which tests/test_gpu_train.py holds the product to byte for byte) writes the reference's .profile
and .gc files, byte for byte, on whole-genome and exome inputs, without known variants, at every context length and at the
bin counts of the edges, on single-end lines, CIGAR insertions and deletions the VCF knows and does not know, an ALT that is
no base, a last line without a line break, and seeded random inputs of the crafted families of tests/train_util.py.

The reference reads its input through `<samtools> view -F 0xD04 -q 20 <bam>` (Profile.cpp:135, :1448);
tests/stub_samtools.sh stands in for samtools and prints the SAM text unfiltered, as the product's --sam route reads it.
Where oracle/_ref/seqToProfile is not built, its recorded runs (tests/golden/reference_train_runs.json) stand in for it.
Every input is first checked against train_util.reference_undefined: where the reference's output is undefined
(reads over a contig's end, iSizeDist read past its row, the GC thinning's edges) a run of it pins nothing."""
import ctypes as C
import hashlib
import os
import random
import time

import pytest

import cases
import ref_runs
import test_train_counts as TC
import test_train_profile_cpu as TP
import train_util as TU

STAMP = time.asctime(time.gmtime(cases.FAKE_SEC)).encode() + b"\n"   # Profile::saveResults under the frozen clock (:1263-1265)


@pytest.fixture(scope="module")
def sim(oracle_lib, tmp_path_factory):
    """Read pairs the oracle sampled on one contig of 1.4 Mbp (12x, no crafted lines)."""
    TP.declare(TC._declare(oracle_lib))
    wd = str(tmp_path_factory.mktemp("train_ref"))
    sam1, fa1, T = TC.make_sam(oracle_lib, os.path.join(wd, "sim"), coverage=12, crafted=False)
    return dict(lines=sam1.rstrip(b"\n").split(b"\n"), fa1=fa1, L=T.L)


def _pure_match(line, L):
    f = line.split(b"\t")
    return f[1] in (b"0", b"99", b"147") and f[5] == b"%dM" % L


def widen(lines, L, inside=lambda pos: True):
    """`lines` with train_util.wide_insert_line put behind the last pair line of nominal length whose position `inside`
    accepts (a line countGC counts: the copy lands in the same window)."""
    for i in range(len(lines) - 1, -1, -1):
        if _pure_match(lines[i], L) and inside(int(lines[i].split(b"\t")[3])):
            return lines[:i + 1] + [TU.wide_insert_line(lines[i])] + lines[i + 1:]
    raise AssertionError("no line to widen iSizeDist behind")


def inside_targets(bed, margin=300):
    rows = [r.split(b"\t") for r in open(bed, "rb").read().split(b"\n") if r.startswith(b"chr1\t")]
    spans = [(int(a) + margin, int(b) - margin) for _, a, b in rows if int(b) - int(a) > 2 * margin]
    return lambda pos: any(a <= pos <= b for a, b in spans)


def whole_input(wd, sim, exome=False, seed=5):
    """The `trained` fixture's input (tests/test_train_profile_cpu.py) without its two lines over chr1's end and one line
    that widens iSizeDist: what is left is defined for the reference."""
    fa, vcf, bed, sam = TU.training_inputs(wd, sim["fa1"], sim["lines"], sim["L"], exome=exome, seed=seed)
    lines = TU.defined_lines(sam.rstrip(b"\n").split(b"\n"), TU.fasta_lengths(fa))
    lines = widen(lines[:len(sim["lines"])], sim["L"], inside_targets(bed) if bed else (lambda pos: True)) + lines[len(sim["lines"]):]
    return fa, vcf, bed, lines


def check(oracle_lib, wd, fa, vcf, bed, lines, kmer=3, bins=50, final_newline=True, expect_gc=None):
    """The restatement and the reference (or its record) on the same files: the same exit status 0, .profile and .gc."""
    sam = b"\n".join(lines) + (b"\n" if final_newline else b"")
    open(os.path.join(wd, "reads.sam"), "wb").write(sam)
    assert os.path.dirname(fa) == wd and os.path.dirname(vcf) == wd and (bed is None or os.path.dirname(bed) == wd)
    ub = TU.reference_undefined(oracle_lib, fa, vcf, bed, sam)
    assert not ub, ub[:5]
    rc, want = ref_runs.run_train(wd, "reads.sam", os.path.basename(fa), os.path.basename(vcf), bed and os.path.basename(bed), kmer, bins)
    assert rc == 0
    got = os.path.join(wd, "orc.profile")
    assert oracle_lib.orc_train_profile(sam, len(sam), fa.encode(), vcf.encode(), (bed or "").encode(), b"ACTG", kmer, bins, got.encode(),
                                        b"reads.sam", STAMP) == 0
    mine = {f.replace("orc.", "ref."): hashlib.md5(open(os.path.join(wd, f), "rb").read()).hexdigest()
            for f in ("orc.profile", "orc.profile.gc") if os.path.exists(os.path.join(wd, f))}
    if expect_gc is not None:
        assert ("ref.profile.gc" in want) == expect_gc
    if mine != want and os.path.exists(os.path.join(wd, "ref.profile")):   # say where (the binary ran here)
        for f in sorted(want):
            a = open(os.path.join(wd, f), "rb").read().split(b"\n")
            b = open(os.path.join(wd, f.replace("ref.", "orc.")), "rb").read().split(b"\n")
            bad = [(i + 1, x[:120], y[:120]) for i, (x, y) in enumerate(zip(a, b)) if x != y][:4]
            assert a == b, (f, len(a), len(b), bad)
    assert mine == want
    return sam


def test_whole_genome_input(sim, oracle_lib, tmp_path):
    """Six contigs, known variants, reads that step backwards and every filter of processRead."""
    wd = str(tmp_path)
    fa, vcf, bed, lines = whole_input(wd, sim)
    check(oracle_lib, wd, fa, vcf, bed, lines, expect_gc=True)


def test_simulated_pairs_only(sim, oracle_lib, tmp_path):
    """The plainest input: the sampled pairs on chr1 (flags 99 / 147) in order.  Here the GC windows the reference thins
    start from its counters' stale values (Profile.cpp:728, :735-739), which zero-initialised counters got wrong."""
    wd = str(tmp_path)
    fa, vcf, _, _ = TU.training_inputs(wd, sim["fa1"], [], sim["L"])
    pairs = sorted((ln for ln in sim["lines"] if ln.split(b"\t")[1] in (b"99", b"147")), key=lambda ln: int(ln.split(b"\t")[3]))
    check(oracle_lib, wd, fa, vcf, None, widen(pairs, sim["L"]), expect_gc=True)


def test_exome_input(sim, oracle_lib, tmp_path):
    wd = str(tmp_path)
    fa, vcf, bed, lines = whole_input(wd, sim, exome=True)
    check(oracle_lib, wd, fa, vcf, bed, lines)


def test_without_known_variants(sim, oracle_lib, tmp_path):
    wd = str(tmp_path)
    fa, vcf, bed, lines = whole_input(wd, sim)
    open(vcf, "wb").write(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n")
    check(oracle_lib, wd, fa, vcf, bed, lines)


@pytest.mark.parametrize("kmer,bins", [(1, 50), (5, 50), (3, 10), (3, 200)])
def test_context_lengths_and_bins(kmer, bins, sim, oracle_lib, tmp_path):
    """-k 1 and -k 5 (the longest the reference takes), -B 10 (the fewest), and -B above the read length: the reference
    clamps it to the read length (Profile.cpp:184-188)."""
    wd = str(tmp_path)
    fa, vcf, bed, lines = whole_input(wd, sim)
    check(oracle_lib, wd, fa, vcf, bed, lines, kmer=kmer, bins=bins)


def test_single_end_lines(sim, oracle_lib, tmp_path):
    """Flag 0 and TLEN 0 only: no insert size is counted, every read is a first mate."""
    wd = str(tmp_path)
    fa, vcf, _, _ = TU.training_inputs(wd, sim["fa1"], [], sim["L"])
    se = []
    for ln in sim["lines"]:
        f = ln.split(b"\t")
        if f[1] == b"99":
            f[1], f[6], f[7], f[8] = b"0", b"*", b"0", b"0"
            se.append(b"\t".join(f))
    check(oracle_lib, wd, fa, vcf, None, sorted(se, key=lambda ln: int(ln.split(b"\t")[3])))


def _snv_rows(vcf):
    return [r.split(b"\t") for r in open(vcf, "rb").read().split(b"\n") if r.startswith(b"chr1\t") and len(r.split(b"\t")[3]) == 1]


def with_odd_alts(wd, sim, fa, vcf, lines):
    """Rewrites `vcf`: four known SNVs of chr1 get the ALT N, R, n and *; returns `lines` (of whole_input) with reads that
    show those ALTs, forward and as mate 2, and reads over them with an insertion and a deletion the VCF does not know, in
    position order among the sampled reads (countGC turns away reads that step backwards, Profile.cpp:552-554)."""
    rows = _snv_rows(vcf)
    chr1 = open(fa, "rb").read().split(b">")[1].split(b"\n", 1)[1].replace(b"\n", b"")
    L, rng = sim["L"], random.Random(11)
    alts = dict(zip((r[1] for r in rows[12:16]), (b"N", b"R", b"n", b"*")))
    text = []
    for t in open(vcf, "rb").read().split(b"\n"):
        f = t.split(b"\t")
        if t.startswith(b"chr1\t") and f[1] in alts:
            f[4] = alts[f[1]]
        text.append(b"\t".join(f))
    open(vcf, "wb").write(b"\n".join(text))
    extra = []
    for p, alt in alts.items():
        pos = int(p)
        for off, tlen in ((40, 300), (10, -300)):
            extra.append(TU._crafted(rng, b"chr1", chr1, pos - off, L, tlen, alt_at=(off, alt[0])))
        extra.append(TU._crafted(rng, b"chr1", chr1, pos - 60, L, 0, cigar=b"30M2I%dM" % (L - 32)))
        extra.append(TU._crafted(rng, b"chr1", chr1, pos - 60, L, 0, cigar=b"30M4D%dM" % (L - 30)))
    n_sim = len(sim["lines"]) + 1
    return sorted(lines[:n_sim] + extra, key=lambda ln: int(ln.split(b"\t")[3])) + lines[n_sim:]


def test_indels_known_and_unknown_and_an_alt_that_is_no_base(sim, oracle_lib, tmp_path):
    """CIGAR insertions and deletions at the VCF's own places and lengths and beside them (whole_input's chr2 lines), more
    on chr1 among the counted reads; known SNVs whose ALT is N or a letter of no base, with reads that show it (the
    reference compares raw characters, Profile.cpp:407-413, :466-468)."""
    wd = str(tmp_path)
    fa, vcf, bed, lines = whole_input(wd, sim)
    check(oracle_lib, wd, fa, vcf, bed, with_odd_alts(wd, sim, fa, vcf, lines))


def test_last_line_without_a_line_break(sim, oracle_lib, tmp_path):
    """fgets leaves the last line without its line break and Profile::train chops its last character anyway (:1459):
    the quality string is one short, and that read's qualities are not counted (:457)."""
    wd = str(tmp_path)
    fa, vcf, _, _ = TU.training_inputs(wd, sim["fa1"], [], sim["L"])
    pairs = sorted((ln for ln in sim["lines"][:20000] if ln.split(b"\t")[1] in (b"99", b"147")), key=lambda ln: int(ln.split(b"\t")[3]))
    lines = widen(pairs, sim["L"])
    check(oracle_lib, wd, fa, vcf, None, lines, final_newline=False)
    check(oracle_lib, wd, fa, vcf, None, lines[:-1] + [lines[-1][:-1]])    # the same as that line cut by one, with a break


# ---- seeded random inputs: pieces of the crafted families of train_util.training_inputs, kept clear of the undefined ----
N_RANDOM = 20


def random_input(rng, wd, sim):
    L = sim["L"]
    exome = rng.random() < 0.3
    fa, vcf, bed, sam = TU.training_inputs(wd, sim["fa1"], [], L, exome=exome, seed=rng.randrange(1000))
    lens = TU.fasta_lengths(fa)
    crafted = TU.defined_lines(sam.rstrip(b"\n").split(b"\n"), lens)
    # a stretch of chr1 of 80-400 kbp (exome: 600-1200 kbp, enough targets for 50 windows)
    span = rng.randrange(600000, 1200000) if exome else rng.randrange(80000, 400000)
    a = rng.randrange(0, 1400000 - span)
    pairs = [ln for ln in sim["lines"] if a <= int(ln.split(b"\t")[3]) < a + span]
    if rng.random() < 0.25:     # single-end
        pairs = [b"\t".join(f[:1] + [b"0"] + f[2:6] + [b"*", b"0", b"0"] + f[9:]) for f in (ln.split(b"\t") for ln in pairs) if f[1] == b"99"]
    pairs.sort(key=lambda ln: int(ln.split(b"\t")[3]))
    # families of crafted lines, by their contig and name
    fam = {}
    for ln in crafted:
        f = ln.split(b"\t")
        fam.setdefault(f[2] if f[0].startswith(b"c") else b"filter", []).append(ln)
    picked = []
    for name in sorted(fam):
        if rng.random() < 0.6:
            ls = fam[name]
            k = rng.randrange(1, len(ls) + 1)
            s = rng.randrange(0, len(ls) - k + 1)
            picked += ls[s:s + k]
    if rng.random() < 0.3:
        open(vcf, "wb").write(b"##fileformat=VCFv4.2\n")
    lines = pairs + picked
    if rng.random() < 0.5:
        lines = widen(pairs, L, inside_targets(bed) if bed else (lambda pos: True)) + picked
    kmer = rng.randrange(1, 6)
    bins = rng.choice([10, 17, 50, 64, 150, 151, 400])
    return fa, vcf, bed, lines, kmer, bins, rng.random() < 0.2


def random_inputs(oracle_lib, wd, sim):
    """N_RANDOM inputs from seeds 0, 1, ...: a seed whose input the reference leaves undefined is passed over."""
    out, seed = [], 0
    while len(out) < N_RANDOM:
        d = os.path.join(wd, "seed%d" % seed)
        os.makedirs(d, exist_ok=True)
        fa, vcf, bed, lines, kmer, bins, open_end = random_input(random.Random(seed), d, sim)
        sam = b"\n".join(lines) + (b"" if open_end else b"\n")
        if not TU.reference_undefined(oracle_lib, fa, vcf, bed, sam):
            out.append((seed, d, fa, vcf, bed, lines, kmer, bins, open_end))
        seed += 1
        assert seed < 4 * N_RANDOM
    return out


def test_random_inputs(sim, oracle_lib, tmp_path):
    for seed, d, fa, vcf, bed, lines, kmer, bins, open_end in random_inputs(oracle_lib, str(tmp_path), sim):
        try:
            check(oracle_lib, d, fa, vcf, bed, lines, kmer=kmer, bins=bins, final_newline=not open_end)
        except AssertionError as e:
            raise AssertionError(f"seed {seed} (kmer {kmer}, bins {bins}, exome {bed is not None}): {e}") from None


def test_the_guard_finds_what_the_fixture_input_leaves_undefined(sim, oracle_lib, tmp_path):
    """The `trained` fixture's own input, as tests/test_train_profile_cpu.py uses it, holds a read that starts behind
    chr1's end -- on it the reference aborts (std::out_of_range from substr, Genome.cpp:435) -- one that hangs over it, and
    an iSizeDist too short for five modal insert sizes: the guard names all three."""
    wd = str(tmp_path)
    fa, vcf, bed, sam = TU.training_inputs(wd, sim["fa1"], sim["lines"], sim["L"])
    ub = b"\n".join(TU.reference_undefined(oracle_lib, fa, vcf, bed, sam))
    assert b"starts behind" in ub and b"hangs over" in ub and b"modal insert size" in ub
