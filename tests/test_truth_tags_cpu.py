"""The truth BAM's NM, MD and XE tags without a GPU: the host statement of the rule (sg_truth_tags: truth_tags_walk and
truth_xe, sg_truth.h) against the model (tests/tags_model.py) on one hand-made record per clause, on seeded random
records and at the MD cap; the runs that are refused before the engine exists; the new names' place in the structs and
the ABI list; and the stand-alone sanitizer build of the host rule (tools/tags_sanitized.sh)."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import cases
import errors_model as EM
import simuscop_amd
import simuscop_amd.build as build
import tags_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMU = os.path.join(build.LIBDIR, "simuReads")
M, I, D, N, S = range(5)
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def codes_of(fasta):
    """The engine's base codes of FASTA bytes (A0 C1 T2 G3, N 4, X 6, anything else 5; either case)."""
    table = {ord("A"): 0, ord("C"): 1, ord("T"): 2, ord("G"): 3, ord("N"): 4, ord("X"): 6}
    return bytes(table.get(b & 0xDF, 5) for b in fasta)


def engine(ops, seq, fasta, cap=2048, **xe_kw):
    return simuscop_amd.truth_tags([(n << 4) | o for n, o in ops], seq, codes_of(fasta), cap, **xe_kw)


def check(ops, seq, fasta, md=None, nm=None):
    """Engine == model (== the text written out by hand where one is given)."""
    present, g_nm, g_md, g_xe = engine(ops, seq, fasta)
    w_nm, w_md = TM.nm_md(ops, seq, fasta)
    assert present == TM.TAG_NM | TM.TAG_MD and g_xe is None
    assert (g_nm, g_md) == (w_nm, w_md), (ops, seq, fasta)
    assert re.fullmatch(rb"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*", g_md)
    if md is not None:
        assert (g_md, g_nm) == (md, nm)


# ---- one record per clause ----
def test_all_match():
    check([(8, M)], b"ACGTACGT", b"ACGTACGT", b"8", 0)


def test_mismatch_first_and_last():
    check([(6, M)], b"TCGTAG", b"ACGTAC", b"0A4C0", 2)


def test_neighbouring_mismatches_have_a_zero_between_them():
    check([(6, M)], b"ACTGAC", b"ACGTAC", b"2G0T2", 2)


def test_deletion_followed_by_a_mismatch():
    check([(3, M), (2, D), (3, M)], b"ACGAAC", b"ACGTTCAC", b"3^TT0C2", 3)


def test_deletion_after_an_insertion():
    # the insertion writes nothing and does not end the count; the deletion's letters are the reference's
    check([(2, M), (3, I), (2, D), (2, M)], b"ACGGGAC", b"ACTTAC", b"2^TT2", 5)
    # two deletions with an insertion between them stay two runs
    check([(2, M), (1, D), (2, I), (2, D), (1, M)], b"ACGGA", b"ACTCCA", b"2^T0^CC1", 5)


def test_n_run_advances_the_reference_and_writes_nothing():
    check([(3, M), (4, N), (3, M)], b"ACGTTT", b"ACGAAAATTT", b"6", 0)
    check([(3, M), (4, N), (3, M)], b"ACGTCT", b"ACGAAAATTT", b"4T1", 1)


def test_leading_and_trailing_soft_clips():
    check([(2, S), (4, M), (3, S)], b"GGACGTCCC", b"ACGT", b"4", 0)
    check([(2, S), (4, M), (3, S)], b"GGACTTCCC", b"ACGT", b"2G1", 1)


def test_read_n_on_reference_n_is_a_mismatch():
    check([(5, M)], b"ACNTA", b"ACNTA", b"2N2", 1)
    check([(5, M)], b"ACNTA", b"ACGTA", b"2G2", 1)


def test_reference_codes_5_and_6_come_out_as_n():
    assert codes_of(b"RXacgtn\r") == bytes([5, 6, 0, 1, 3, 2, 4, 5])
    check([(6, M)], b"ACAATA", b"ACRXTA", b"2N0N2", 2)
    check([(2, M), (3, D), (2, M)], b"ACTA", b"ACRXNTA", b"2^NNN2", 3)
    check([(4, M)], b"ACGT", b"AC\rT", b"2N1", 1)


def test_lower_case_fasta_matches_like_upper_case():
    check([(8, M)], b"ACGTACGT", b"acgtACgt", b"8", 0)
    check([(4, M), (2, D), (2, M)], b"ACGTGT", b"acgtacgt", b"4^AC2", 2)


def test_reverse_read():
    """SEQ is already in BAM orientation, so NM and MD do not look at the strand; XE pairs the read in FASTQ orientation with
    the template in read direction, complemented."""
    fasta = b"ACGTTGCAAC"
    read_fq = b"GTTGAAACGT"                               # the complement of the template, turned round, one base changed
    seq = read_fq.translate(COMP)[::-1]
    assert seq == b"ACGTTTCAAC"
    present, nm, md, xe = engine([(10, M)], seq, fasta, tmpl_codes=codes_of(fasta), reverse=True, read=read_fq)
    assert present == TM.TAG_ALL and (nm, md, xe) == (1, b"5G4", 1)
    assert (nm, md) == TM.nm_md([(10, M)], seq, fasta) and xe == TM.xe(np.frombuffer(codes_of(fasta), dtype=np.uint8), True, [], read_fq)
    # with a sequencing deletion of two template bases in read direction: D in the record, two bases in XE
    ev = [EM.ev_pack(3, 2, True)]
    read_fq = b"GTTAACGT"
    seq = read_fq.translate(COMP)[::-1]
    present, nm, md, xe = engine([(5, M), (2, D), (3, M)], seq, fasta, tmpl_codes=codes_of(fasta), reverse=True, events=ev, read=read_fq)
    assert (nm, md, xe) == (2, b"5^GC3", 2)
    assert xe == TM.xe(np.frombuffer(codes_of(fasta), dtype=np.uint8), True, ev, read_fq)


def test_unmapped_but_inside_gets_xe_alone():
    tmpl = b"ACGTAC"
    present, nm, md, xe = engine([], b"", b"", tmpl_codes=codes_of(tmpl), read=b"ACCTNC")
    assert (present, nm, md, xe) == (TM.TAG_XE, None, None, 2)
    t, dropped = TM.tags([], b"", b"", -1, True, np.frombuffer(codes_of(tmpl), dtype=np.uint8), False, [], b"ACCTNC")
    assert t == {"XE": 2} and not dropped and TM.tag_bytes(t) == b"XEI\2\0\0\0"


def test_not_inside_gets_no_tag():
    assert engine([], b"", b"") == (0, None, None, None)
    assert TM.tags([], b"", b"", -1, False) == ({}, False)


def test_a_template_base_that_is_no_letter_is_no_error_and_insertions_count():
    tmpl = b"ACNTAC"
    ev = [EM.ev_pack(1, 2, False)]
    read = b"ACGGGTAC"
    _, _, _, xe = engine([], b"", b"", tmpl_codes=codes_of(tmpl), events=ev, read=read)
    assert xe == 2 == TM.xe(np.frombuffer(codes_of(tmpl), dtype=np.uint8), False, ev, read)


def test_refused_records():
    with pytest.raises(simuscop_amd.SimuError):
        engine([(4, M)], b"ACG", b"ACGT")                 # the operations do not cover SEQ
    with pytest.raises(simuscop_amd.SimuError):
        engine([(4, M)], b"ACGT", b"ACG")                 # ... or run past the reference given
    with pytest.raises(simuscop_amd.SimuError):
        engine([], b"", b"", tmpl_codes=codes_of(b"ACGT"), read=b"ACG")     # the events do not give the read's length


# ---- random records ----
def _random_record(rng):
    n_runs = rng.randint(1, 7)
    ops, last = [], None
    for k in range(n_runs):
        edge = k == 0 or k == n_runs - 1
        op = M if n_runs == 1 else (rng.choice([M, M, M, S]) if edge else rng.choice([M, M, I, D, N]))
        if op == last:
            op = I if op == M else M
        last = op
        ops.append((rng.randint(1, 12), op))
    fasta, seq = bytearray(), bytearray()
    for n, op in ops:
        if op in (M, D, N):
            ref = bytes(rng.choice(b"ACGTacgtNRX") if rng.random() < 0.15 else rng.choice(b"ACGT") for _ in range(n))
            fasta += ref
            if op == M:
                seq += bytes(rng.choice(b"ACGTN") if rng.random() < 0.15 else (c & 0xDF) for c in ref)
        else:
            seq += bytes(rng.choice(b"ACGTN") for _ in range(n))
    return ops, bytes(seq), bytes(fasta)


def test_random_records():
    rng = random.Random(20240611)
    met = dict(caret=0, zero=0, n_op=0, dropped=0)
    for _ in range(20000):
        ops, seq, fasta = _random_record(rng)
        cap = rng.choice([2048, 2048, rng.randint(1, 12)])
        present, nm, md, _ = engine(ops, seq, fasta, cap)
        w_nm, w_md = TM.nm_md(ops, seq, fasta)
        assert nm == w_nm and present & TM.TAG_NM
        if len(w_md) <= cap:
            assert md == w_md, (ops, seq, fasta)
            met["caret"] += b"^" in md
            met["zero"] += re.search(rb"[A-Z]0[A-Z^]", md) is not None
        else:
            assert md is None and not present & TM.TAG_MD
            met["dropped"] += 1
        met["n_op"] += any(o == N for _, o in ops)
    assert all(v > 500 for v in met.values()), met


def test_random_reads_xe():
    rng = random.Random(77)
    with_events = 0
    for _ in range(2000):
        L = rng.randint(20, 90)
        codes = np.array([rng.choice([4, 5, 6]) if rng.random() < 0.05 else rng.randrange(4) for _ in range(L)], dtype=np.uint8)
        ev, j, np_ = [], rng.randint(0, L // 3), 0
        shown = [1] * L
        while j < L and len(ev) < rng.choice([0, 0, 3, 8]):
            k, is_del = rng.randint(1, 6), rng.random() < 0.5
            ev.append(EM.ev_pack(j, k, is_del))
            if is_del:
                for x in range(j, min(L, j + k)):
                    shown[x] = 0
                j += k
            else:
                shown[j] += k
                j += 1
            j += rng.randint(0, 20)
        np_ = sum(shown)
        read = bytes(rng.choice(b"ACGTN") for _ in range(np_))
        rev = rng.random() < 0.5
        _, _, _, xe = engine([], b"", b"", tmpl_codes=codes.tobytes(), reverse=rev, events=ev, read=read)
        assert xe == TM.xe(codes, rev, ev, read), (codes, rev, ev, read)
        with_events += bool(ev)
    assert with_events > 500


# ---- the cap ----
def test_md_of_exactly_the_cap_and_one_more():
    cap = 64
    fasta = b"AC" + b"G" * (cap - 3) + b"TT"                                  # 2 ^ G... 2: cap - 3 letters + 3 bytes = cap
    ops = [(2, M), (cap - 3, D), (2, M)]
    present, nm, md, _ = engine(ops, b"ACTT", fasta, cap)
    assert md == b"2^" + b"G" * (cap - 3) + b"2" and len(md) == cap and nm == cap - 3 and present & TM.TAG_MD
    assert (nm, md) == TM.nm_md(ops, b"ACTT", fasta)
    fasta = b"AC" + b"G" * (cap - 2) + b"TT"
    ops = [(2, M), (cap - 2, D), (2, M)]
    present, nm, md, _ = engine(ops, b"ACTT", fasta, cap)
    assert md is None and present == TM.TAG_NM and nm == cap - 2              # dropped: NM stays
    assert len(TM.nm_md(ops, b"ACTT", fasta)[1]) == cap + 1
    t, dropped = TM.tags(ops, b"ACTT", fasta, 0, False, cap=cap)
    assert t == {"NM": cap - 2} and dropped


# ---- command lines and in-process runs that are refused before the engine exists ----
def test_cli_refuses_tags_without_the_truth_bam(tmp_path):
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path / "base"))
    out = str(tmp_path / "out")
    r = subprocess.run([SIMU, cfg, "--quiet", "--out", out, "--truth-tags"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr[-300:])
    assert "--truth-tags" in r.stderr and "--truth-bam" in r.stderr and "GPU engine error" not in r.stderr
    assert not os.path.exists(out) or not os.listdir(out)


def test_in_process_refusals(tmp_path):
    cfg = cases.build_case("wgs_pe_xten", str(tmp_path / "base"))
    out = str(tmp_path / "out")
    with pytest.raises(simuscop_amd.SimuError, match="--truth-tags needs --truth-bam"):
        simuscop_amd.run_config(cfg, seed=1, output_dir=out, quiet=1, truth_tags=1)
    with pytest.raises(simuscop_amd.SimuError, match="--host-haplotypes"):
        simuscop_amd.run_config(cfg, seed=1, output_dir=out, quiet=1, truth_tags=1, truth_bam=1, host_haplotypes=1)
    with pytest.raises(simuscop_amd.SimuError, match="--truth-tags needs --truth-bam"):
        simuscop_amd.run_config(cfg, seed=1, output_dir=out, quiet=1, truth_tags=1, host_haplotypes=1)
    assert not os.path.exists(out) or not os.listdir(out)


# ---- struct order and the ABI list ----
def test_new_names_are_in_the_header_the_abi_list_and_the_structs():
    hdr = open(os.path.join(ROOT, "include", "simuscop_amd.h")).read()
    declared = set(re.findall(r"\b(sg_truth_[a-z_0-9]+)\s*\(", hdr)) | set(re.findall(r"\b(sg_fetch_truth)\s*\(", hdr))
    assert declared == {"sg_truth_align", "sg_truth_map", "sg_truth_pieces", "sg_truth_reads", "sg_truth_bam", "sg_fetch_truth", "sg_truth_info",
                        "sg_truth_bam_tags", "sg_truth_tag_info", "sg_truth_tags"}
    assert declared <= set(simuscop_amd.ENGINE_SYMBOLS)
    eng = simuscop_amd.load_engine()
    for name in declared:
        getattr(eng, name)
    assert "typedef struct sg_truth_tag_counts {" in hdr
    for name, bit in (("SG_TAG_NM", 1), ("SG_TAG_MD", 2), ("SG_TAG_XE", 4)):
        assert re.search(r"#define %s %du\b" % (name, bit), hdr)
    assert (simuscop_amd.TAG_NM, simuscop_amd.TAG_MD, simuscop_amd.TAG_XE, simuscop_amd.TAG_ALL) == (1, 2, 4, 7)
    # the option sits next to truth_bam, the stats behind t_truth; the last fields stay the last
    opts = [f[0] for f in simuscop_amd.SimuOptions._fields_]
    i = opts.index("truth_bam")
    assert opts[i:i + 2] == ["truth_bam", "truth_tags"] and opts[-2:] == ["truth_variants", "truth_depth"]
    stats = [f[0] for f in simuscop_amd.SimuStats._fields_]
    i = stats.index("t_truth")
    assert stats[i:i + 5] == ["t_truth", "truth_tag_bytes", "truth_md_dropped", "truth_nm_sum", "truth_xe_sum"]
    assert stats[-3:] == ["depth_bases", "depth_rows", "t_depth"]
    # the structs of the host library and of the Python glue list their fields in one order
    shdr = open(os.path.join(ROOT, "simuscop_amd", "csrc", "host", "simulate.h")).read()
    c_opts = re.findall(r"^\s*(?:int32_t|uint64_t|const char\*|void\*)\s+(\w+);", shdr[shdr.index("typedef struct simu_options"):shdr.index("} simu_options;")], re.M)
    assert [o for o in opts if o.startswith("truth_")] == [o for o in c_opts if o.startswith("truth_")]
    flat = []
    for chunk in re.sub(r"//[^\n]*", "", shdr[shdr.index("typedef struct simu_stats {") + 27:shdr.index("} simu_stats;")]).split(";"):
        names = re.sub(r"^\s*(uint64_t|double|float|int32_t|uint32_t)\s+", "", chunk.strip())
        flat += [re.sub(r"\[\d+\]", "", n.strip()) for n in names.split(",") if n.strip()]
    assert flat == stats
    assert callable(simuscop_amd.truth_tags) and callable(simuscop_amd.Session.truth_tag_info)
    assert simuscop_amd.default_options(truth_tags=1).truth_tags == 1 and simuscop_amd.default_options().truth_tags == 0


# ---- the host rule under the sanitizers ----
def test_the_host_rule_under_the_sanitizers(tmp_path):
    """tools/tags_sanitized.sh: sg_truth_tags in a stand-alone program with its own main, AddressSanitizer +
    UndefinedBehaviorSanitizer, against a base-by-base walk.  CPU only."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "tags_sanitized.sh"), "4000", "99"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    assert "all as the base-by-base walk has them" in r.stdout
