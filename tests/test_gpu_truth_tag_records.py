"""`simuReads --truth-tags` on the MI355X through a Session (sg_truth_tags.hip, the tagged record kernel of sg_truth.hip):

  1. records: for every read of every pass the tagged record is the untagged record with block_size raised and the
     model's tag bytes (tests/tags_model.py) behind it, byte for byte, and sg_truth_tag_info's sums are the model's;
  2. pass sizes around the wave (64 records) and the text block (256 reads), and every subset of the tag mask;
  3. meaning: with a profile that substitutes nothing MD and NM show the variants and the sequencing indels only, XE the
     sequencing indels only; with a shipped profile the XE values add up to the true error counts of the same passes;
  4. the cap: variant deletions around kTruthMaxMd bases long make MD texts that fit, fit for some flanks, and never fit."""
import os
import re

import pytest

import cases
import errors_model as EM
import simuscop_amd
import tags_model as TM
import tags_util as TU
import test_gpu_error_counts as EC
import test_gpu_truth_bam as TB
import truth_util as U

pytestmark = pytest.mark.gpu

MAX_READS = 4000   # per population: the model is Python

# name -> (config maker, paired, populations): each the smallest shape at which its part of the kernels can go wrong
CASES = {
    "short_reads_se": (lambda wd: cases.build_case("short_reads_se", wd), False, 1),                    # L = 52: one partial 64-lane chunk
    "derived_L64": (EC._derived(64), True, 1),                                                          # the chunk boundary
    "derived_L65": (EC._derived(65), True, 1),
    "wgs_pe_xten": (lambda wd: cases.build_case("wgs_pe_xten", wd), True, 1),                           # L = 151
    "long_reads_pe": (lambda wd: cases.build_case("long_reads_pe", wd), True, 1),                       # L = 600: ten chunks
    "indel_storm_se": (lambda wd: cases.build_case("indel_storm_se", wd), False, 1),                    # many events per read
    "indel_rich_n_islands_pe": (lambda wd: cases.build_case("indel_rich_n_islands_pe", wd), True, 1),   # N in the reference, two contigs
    "wgs_pe_variants": (lambda wd: cases.build_case("wgs_pe_variants", wd), True, 1),                   # chain != reference
    "wes_pe_targets": (lambda wd: cases.build_case("wes_pe_targets", wd), True, 1),                     # exome targets, two contigs
    "tumor_se_mixture": (lambda wd: cases.build_case("tumor_se_mixture", wd), False, 4),                # four populations
}


def run_case(cfg, paired, popus, max_reads=MAX_READS):
    """Every (population, chromosome) pass; returns what the clauses test below counts."""
    L = TU.read_length(cfg)
    fastas = TU.fasta_sequences(TU.config_value(cfg, "ref"))
    met = dict(records=0, passes=0, caret=0, neighbours=0, n_op=0, reverse=0, unmapped_inside=0, no_tag=0, mismatch=0, xe=0, dropped=0)
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=TB.SEED, truth_bam=1) as sess:
        for p in range(popus):
            sess.weighted_length(p)
            sess.set_reads(min(sess.planned_reads, max_reads), p)
            for chrom in range(sess.n_chromosomes):
                if not sess.prepare_batch(chrom, p):
                    continue
                sess.sample()
                sess.result()
                _, _, model, info = TU.tagged_pass(sess, paired, L, fastas)
                met["passes"] += 1
                met["records"] += len(model)
                met["dropped"] += info.md_dropped
                for t, _, rec, row in model:
                    md = t.get("MD", b"")
                    met["caret"] += b"^" in md
                    met["neighbours"] += re.search(rb"[A-Z]0[A-Z]", md) is not None
                    met["mismatch"] += re.search(rb"[0-9][A-Z]", md) is not None
                    met["n_op"] += any(o == TM.OP_N for _, o in rec["ops"])
                    met["reverse"] += bool(rec["flag"] & 0x10)
                    met["unmapped_inside"] += not rec["ops"] and bool(row.inside)
                    met["no_tag"] += not t
                    met["xe"] += t.get("XE", 0) > 0
    return met


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    done = {}   # every case runs once for the whole file

    def run(name):
        if name not in done:
            make, paired, popus = CASES[name]
            done[name] = run_case(make(str(tmp_path_factory.mktemp(name))), paired, popus)
        return done[name]
    return run


@pytest.mark.parametrize("name", sorted(CASES))
def test_tagged_records_are_the_untagged_ones_plus_the_models_tags(name, runs):
    met = runs(name)
    print(name, met)
    assert met["passes"] >= CASES[name][2] and met["records"] > 500
    assert met["mismatch"] > 0 and met["xe"] > 0


def test_the_cases_meet_every_clause(runs):
    """Nothing above is vacuous: over the cases together there are records with a deletion, with neighbouring mismatches
    and turned round.  N operations have a test of their own below (no case here yields one); an unmapped read whose
    template lies in its chain is rare: it is counted and printed, and the host rule's CPU test covers it."""
    total = {}
    for name in CASES:
        for k, v in runs(name).items():
            total[k] = total.get(k, 0) + v
    print(total)
    assert total["caret"] > 0 and total["neighbours"] > 0 and total["reverse"] > 0
    assert runs("indel_storm_se")["caret"] > 100


def test_an_absent_segment_gives_n_operations(tmp_path):
    """None of the suite's cases yields an N operation (wes_pe_targets: 0 of its 50,370 records at full size; fragments end
    with their segment's string).  A copy-number loss does: the haplotype that lacks the segment joins its neighbours, and
    a read across the joint skips the segment with one N."""
    wd = str(tmp_path)
    prof = os.path.join(cases.TESTDATA, cases.PROFILES["hs2000"])
    cfg, fa, _ = U.acgt_case(wd, prof, "PE", variants=False, coverage=30, lengths=(60000, 5000))
    var = os.path.join(wd, "variations.txt")
    cases._write(var, ["c\tv\tchr3\t20001\t30000\t1\t1", "c\tv\tchr3\t40001\t45000\t1\t1"])
    with open(cfg, "a") as f:
        f.write("variation = %s\n" % var)
    met = run_case(cfg, True, 1, max_reads=12000)
    print(met)
    assert met["n_op"] > 0 and met["records"] > 1000


# ---------------------------------------------------------------------------------------------------------------------
# 2. pass sizes and tag masks
# ---------------------------------------------------------------------------------------------------------------------
def _session(tmp_path_factory, case, **kw):
    cfg = cases.build_case(case, str(tmp_path_factory.mktemp(case)))
    return cfg, simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=TB.SEED, truth_bam=1, **kw)


@pytest.fixture(scope="module")
def hs2000(tmp_path_factory):
    cfg, s = _session(tmp_path_factory, "wgs_se_hs2000")
    with s as sess:
        sess.weighted_length()
        yield sess, TU.read_length(cfg), TU.fasta_sequences(TU.config_value(cfg, "ref"))


@pytest.fixture(scope="module")
def xten(tmp_path_factory):
    cfg, s = _session(tmp_path_factory, "wgs_pe_xten", truth_errors=1)
    with s as sess:
        sess.weighted_length()
        yield sess, TU.read_length(cfg), TU.fasta_sequences(TU.config_value(cfg, "ref"))


def _pass_of(fix, slots, paired):
    """A pass of exactly `slots` fragment slots (the read count that gives them is looked for, as in the error counts'
    test); a size that no read count gives fails the test."""
    sess, L, fastas = fix
    found = None
    for reads in range(max(1, slots - 2), 2 * slots + 8):
        sess.set_reads(reads)
        if sess.prepare_batch(0) and sess.batch_slots == slots:
            found = reads
            break
    assert found is not None, "no set_reads() value gives %d slots" % slots
    sess.sample()
    sess.result()
    plain, _, model, info = TU.tagged_pass(sess, paired, L, fastas)
    assert 0 < len(plain) <= (2 if paired else 1) * slots and info.n_nm > 0


@pytest.mark.parametrize("slots", [1, 63, 64, 65, 255, 256, 257])
def test_passes_of_a_few_reads(slots, hs2000):
    """A wave takes 64 records, text_offset addresses the text in blocks of 256 reads; SE: one read a slot."""
    _pass_of(hs2000, slots, False)


@pytest.mark.parametrize("slots", [1, 63, 64, 65])
def test_passes_of_a_few_pairs(slots, xten):
    """Two records a slot: 64 pairs are two full waves, 65 leave two records to a third."""
    _pass_of(xten, slots, True)


def test_every_subset_of_the_tag_mask(xten):
    sess, L, fastas = xten
    sess.set_reads(600)
    assert sess.prepare_batch(0)
    sess.sample()
    sess.result()
    sizes = {}
    for mask in range(8):
        plain, stream, model, info = TU.tagged_pass(sess, True, L, fastas, mask)
        sizes[mask] = len(stream)
        assert (info.n_nm > 0, info.n_md > 0, info.n_xe > 0) == (bool(mask & 1), bool(mask & 2), bool(mask & 4))
    rb, _ = sess.truth_bam()
    assert sizes[0] == rb and sess.truth_tag_info().tag_bytes == 0           # mask 0 is sg_truth_bam
    assert sizes[7] - sizes[0] == sum(sizes[m] - sizes[0] for m in (1, 2, 4))
    with pytest.raises(simuscop_amd.SimuError, match="mask"):
        sess.truth_bam(8)


# ---------------------------------------------------------------------------------------------------------------------
# 3. meaning
# ---------------------------------------------------------------------------------------------------------------------
def _event_bases(row, L):
    """Bases the read's sequencing events insert and delete (deletions clipped to the template), and whether an event
    touches the template's first or last base: such an event lies outside the alignment (a D in front of the first or
    behind the last M base is dropped, an insertion there is soft-clipped), so XE counts it and NM cannot."""
    total, edge = 0, False
    for e in range(row.n_events):
        j, k, is_del = EM.ev_unpack(row.events[e])
        if is_del:
            k = min(k, L - j)
            edge |= j == 0 or j + k == L
        else:
            edge |= j == L - 1
        total += k
    return total, edge


def _identity_passes(tmp_path, variants):
    wd = str(tmp_path)
    prof = U.write_identity_profile(os.path.join(wd, "identity.profile"), shipped="xten")
    cfg, fa, _ = U.acgt_case(wd, prof, "PE", variants=variants)
    L = TU.read_length(cfg)
    fastas = TU.fasta_sequences(fa)
    out = []
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=TB.SEED, truth_bam=1) as sess:
        sess.weighted_length()
        sess.set_reads(min(sess.planned_reads, MAX_READS))
        for chrom in range(sess.n_chromosomes):
            if sess.prepare_batch(chrom):
                sess.sample()
                sess.result()
                out += TU.tagged_pass(sess, True, L, fastas)[2]
    return wd, L, out


def test_identity_profile_without_variants(tmp_path):
    """Every MD is one number, the record's M bases -- but for a sequencing deletion, which MD shows as ^letters between
    two numbers that still add up to the M bases; no MD holds a mismatch.  NM is the record's I and D bases, XE the
    events' bases, and the two are equal for every read whose events keep clear of the template's ends (_event_bases)."""
    _, L, model = _identity_passes(tmp_path, False)
    with_indels = at_edge = 0
    for t, dropped, rec, row in model:
        assert rec["ops"] and not dropped and set(t) == {"NM", "MD", "XE"}
        m_bases = sum(n for n, o in rec["ops"] if o == TM.OP_M)
        indel = sum(n for n, o in rec["ops"] if o in (TM.OP_I, TM.OP_D))
        ev_bases, edge = _event_bases(row, L)
        md_numbers = [int(x) for x in re.findall(rb"[0-9]+", t["MD"])]
        assert sum(md_numbers) == m_bases and not re.search(rb"[0-9][A-Z]", t["MD"]), t    # no mismatch letter anywhere
        if not any(o == TM.OP_D for _, o in rec["ops"]):
            assert t["MD"] == b"%d" % m_bases
        assert t["NM"] == indel and t["XE"] == ev_bases
        if not edge:
            assert t["NM"] == t["XE"], (t, rec["ops"])
        at_edge += edge
        with_indels += indel > 0
    assert len(model) > 1000 and with_indels > 20 and at_edge < with_indels


def test_identity_profile_with_variants(tmp_path):
    """Every MD mismatch lies on a known allele, and XE counts the sequencing indels only."""
    wd, L, model = _identity_passes(tmp_path, True)
    known = U.known_alleles(wd)
    names = ["chr3", "chr8"]
    on_allele = 0
    for t, dropped, rec, row in model:
        assert t.get("XE", 0) == _event_bases(row, L)[0]
        if "MD" not in t:
            continue
        x = rec["pos"]
        for num, item in re.findall(rb"([0-9]+)([A-Z]|\^[A-Z]+)?", t["MD"]):
            x += int(num)
            if item.startswith(b"^"):
                x += len(item) - 1
            elif item:
                assert x in known.get(names[rec["rid"]], {}), (names[rec["rid"]], x, t["MD"], rec["pos"])
                on_allele += 1
                x += 1
    assert on_allele > 50 and any(t.get("NM", 0) > t.get("XE", 0) for t, _, _, _ in model)


def test_xe_adds_up_to_the_true_error_counts(xten):
    """A shipped profile, truth_errors in the same session: the sum of XE is Q.errors + I.bases + D.bases of the passes."""
    sess, L, fastas = xten
    sess.set_reads(3000)
    total = 0
    sess.errors_reset()
    for chrom in range(sess.n_chromosomes):
        if not sess.prepare_batch(chrom):
            continue
        sess.sample()
        sess.result()
        sess.truth_bam(simuscop_amd.TAG_XE)
        total += sess.truth_tag_info().xe_sum
        sess.errors_add()
    info = sess.errors_info()
    t = EM.Table.of_flat(sess.errors_counts(), info.cycles, info.qual_lo, info.n_qual, info.tmpl_len)
    assert total == int(t.Q[..., EM.ERRORS].sum() + t.I[..., 1].sum() + t.D[..., 1].sum()) > 1000


# ---------------------------------------------------------------------------------------------------------------------
# 4. the cap
# ---------------------------------------------------------------------------------------------------------------------
def test_variant_deletions_around_the_cap(tmp_path):
    """Homozygous deletions of kTruthMaxMd - 7, - 4 and - 1 bases in a 60 kb ACGT genome under the identity profile.  A
    record that spans one has the text <flank>^<letters><flank>: the first always fits (two flanks of at most three
    digits; a read with a sequencing indel of its own can still exceed the cap), the last never does, the middle one fits
    when the flanks have three digits between them -- with 75-base reads, when one of them is shorter than ten bases -- as
    the model says."""
    wd = str(tmp_path)
    prof = U.write_identity_profile(os.path.join(wd, "identity.profile"), shipped="hs2000")
    cfg, fa, _ = U.acgt_case(wd, prof, "PE", variants=False, coverage=30, lengths=(60000, 5000))
    cap = 2048
    dels = [(8000, cap - 7), (25000, cap - 4), (42000, cap - 1)]
    var = os.path.join(wd, "variations.txt")
    cases._write(var, ["d\tv\tchr3\t%d\t%d\thomo" % (p, n) for p, n in dels])
    with open(cfg, "a") as f:
        f.write("variation = %s\n" % var)
    L = TU.read_length(cfg)
    fastas = TU.fasta_sequences(fa)
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=TB.SEED, truth_bam=1) as sess:
        sess.weighted_length()
        sess.set_reads(min(sess.planned_reads, 12000))
        assert sess.prepare_batch(0)
        sess.sample()
        sess.result()
        _, _, model, info = TU.tagged_pass(sess, True, L, fastas)
    assert info.max_md == cap
    spanning = {n: [0, 0] for _, n in dels}        # deletion length -> records with MD, without
    plain_dropped = {n: 0 for _, n in dels}        # ... without, among the reads that have no sequencing indel
    others = 0
    for t, dropped, rec, row in model:
        big = [n for n, o in rec["ops"] if o == TM.OP_D and n >= cap - 7]
        if not big:
            assert not dropped and (not rec["ops"] or "MD" in t)
            others += 1
            continue
        assert len(big) == 1 and t["NM"] >= big[0] and ("MD" in t) != dropped
        spanning[big[0]][1 if dropped else 0] += 1
        plain_dropped[big[0]] += dropped and row.n_events == 0
    print(spanning, plain_dropped, info.md_dropped)
    # always fits -- unless a sequencing deletion adds a second ^run to the text, which the identity profile still makes
    assert spanning[cap - 7][0] > 0 and plain_dropped[cap - 7] == 0
    assert spanning[cap - 1][0] == 0 and spanning[cap - 1][1] > 0            # never fits
    assert sum(spanning[cap - 4]) > 0
    assert info.md_dropped == sum(v[1] for v in spanning.values()) > 0 and others > 1000
