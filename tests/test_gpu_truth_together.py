"""All four truth options in one run, over more than one stem, on the MI355X.

`--truth-depth`, `--truth-variants` and `--truth-errors` share one driver lifecycle (begin on first use, open per stem,
add per piece, render / write / reset when the stem closes) and, with `--truth-bam`, one engine prelude per pass.  Every
other truth test runs one or two of them; here they run together: two contigs, two populations with variation rows of
every kind and a SNP row, two abundance rows (two stems).  One output must not move another: each file of the combined
run is, byte for byte, the file of a run with that option alone, the FASTQ files are those of every run, and each
output's counts in the `stats:` line are its solo run's.  The same through a Session, where the caller adds and resets."""
import os
import re

import pytest

import cases
import simuscop_amd
import test_gpu_truth_bam as TB
import truth_util as U

pytestmark = pytest.mark.gpu

# option -> (flags, file suffix, the output's fields of the stats line)
OPTIONS = {
    "bam": (("--truth-bam",), ".truth.bam", ("truth_records", "truth_unmapped", "truth_bytes", "truth_bgzf_bytes")),
    "depth": (("--truth-depth", "1"), ".truth.depth.bedgraph", ("depth_bases", "depth_rows")),
    "variants": (("--truth-variants",), ".truth.variants.tsv", ("variant_rows", "variant_dropped", "variant_hits")),
    "errors": (("--truth-errors",), ".truth.errors.tsv", ("errors_bases", "errors_subst")),
}
FASTQ = ("_1.fq", "_2.fq")


def two_stem_case(wd):
    _, fa, _ = U.acgt_case(wd, os.path.join(cases.TESTDATA, cases.PROFILES["xten"]), "PE", lengths=(20000, 21000))
    cases._write(os.path.join(wd, "variations.txt"), [
        "i\ta\tchr3\t3000\ttcgagt\thomo", "d\ta\tchr3\t7000\t8\thet", "s\ta\tchr3\t5000\tA\tG\thomo",
        "s\tb\tchr8\t9000\tC\tT\thet", "i\tb\tchr8\t12000\tacgtac\thet", "d\tb\tchr3\t15000\t6\thomo"])
    cases._write(os.path.join(wd, "snp.txt"), ["rs0\tchr8\t4000\tA/C\t+\tA"])
    cases._write(os.path.join(wd, "abundance.txt"), ["1.0\t0", "0.4\t0.6"])
    cfg = os.path.join(wd, "together.txt")
    cases._config(cfg, ref=fa, profile=os.path.join(cases.TESTDATA, cases.PROFILES["xten"]), name="a, b",
                  variation=os.path.join(wd, "variations.txt"), snp=os.path.join(wd, "snp.txt"),
                  abundance=os.path.join(wd, "abundance.txt"), output=os.path.join(wd, "out"), layout="PE", threads=1, verbose=0,
                  coverage=5, insertSize=400)
    return cfg


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{name: (output directory, stderr)} of the combined run and of the four runs with one option each."""
    wd = str(tmp_path_factory.mktemp("together"))
    cfg = two_stem_case(wd)
    out = {}
    for name, flags in [("all", sum((OPTIONS[k][0] for k in OPTIONS), ()))] + [(k, OPTIONS[k][0]) for k in OPTIONS]:
        d = os.path.join(wd, "out_" + name)
        out[name] = (d, TB.simu(cfg, d, *flags).stderr)
    return cfg, out


def test_each_file_is_its_solo_runs_file(runs):
    _, out = runs
    d_all, _ = out["all"]
    stems = TB.stems(d_all)
    assert len(stems) == 2
    assert sorted(os.listdir(d_all)) == sorted(stem + sfx for stem in stems for sfx in FASTQ + tuple(v[1] for v in OPTIONS.values()))
    for stem in stems:
        for name, (_, sfx, _) in OPTIONS.items():
            d_solo, _ = out[name]
            assert sorted(os.listdir(d_solo)) == sorted(s + x for s in stems for x in FASTQ + (sfx,)), name
            a, b = open(os.path.join(d_all, stem + sfx), "rb").read(), open(os.path.join(d_solo, stem + sfx), "rb").read()
            assert a and a == b, (stem, name)
            for fq in FASTQ:
                assert open(os.path.join(d_all, stem + fq), "rb").read() == open(os.path.join(d_solo, stem + fq), "rb").read(), (stem, name, fq)
    # two stems, two files: a state that was not reset between them, or reads counted for the other stem, shows here
    for _, sfx, _ in OPTIONS.values():
        assert open(os.path.join(d_all, stems[0] + sfx), "rb").read() != open(os.path.join(d_all, stems[1] + sfx), "rb").read(), sfx


def test_each_outputs_stats_are_its_solo_runs(runs):
    _, out = runs
    _, err_all = out["all"]
    for name, (_, _, fields) in OPTIONS.items():
        _, err_solo = out[name]
        for f in fields:
            print(name, f, TB.stat(err_all, f), TB.stat(err_solo, f))
            assert TB.stat(err_all, f) == TB.stat(err_solo, f), (name, f)
        for other, (_, _, theirs) in OPTIONS.items():          # ... and a solo run feeds no other output's fields
            if other != name:
                assert all(TB.stat(err_solo, f) == 0 for f in theirs), (name, other)
    for f in ("truth_records", "depth_bases", "depth_rows", "variant_rows", "variant_hits", "errors_bases", "errors_subst"):
        assert TB.stat(err_all, f) > 0, f
    assert TB.stat(err_all, "variant_rows") == 7 and TB.stat(err_all, "variant_dropped") == 0
    assert all(re.search(k + r"=[0-9.]+", err_all) for k in ("truth_s", "depth_s", "variants_s", "errors_s"))


def one_pass(cfg, **options):
    """A session's first pass with work, then what each enabled output says of it: twice, with a reset between."""
    got = {}
    with simuscop_amd.Session(cfg, device=0, write_files=0, quiet=1, seed=TB.SEED, **options) as sess:
        sess.weighted_length()
        sess.set_reads(sess.planned_reads)
        chrom = next(c for c in range(sess.n_chromosomes) if sess.prepare_batch(c))
        sess.sample()
        sess.result()
        if options.get("truth_bam"):
            got["bam"] = (sess.truth_bam(), sess.truth_info())
        for name, add, reset in (("depth", "depth_add", "depth_reset"), ("variants", "variants_add", "variants_reset"),
                                 ("errors", "errors_add", "errors_reset")):
            if not options.get("truth_" + name):
                continue
            first = getattr(sess, add)()
            getattr(sess, reset)()
            got[name] = (first, getattr(sess, add)())
    return chrom, got


def test_a_session_with_all_four_adds_what_four_sessions_add(runs):
    cfg, _ = runs
    chrom, together = one_pass(cfg, truth_bam=1, truth_depth=1, truth_variants=1, truth_errors=1)
    assert sorted(together) == sorted(OPTIONS)
    (rec_bytes, gz_bytes), (records, unmapped) = together["bam"]
    assert records > 100 and rec_bytes > 0 and gz_bytes > 0
    assert together["depth"][0] > 0 and together["variants"][0][1] > 0 and together["errors"][0][0] > 0
    for name in OPTIONS:
        solo_chrom, solo = one_pass(cfg, **{"truth_" + name: 1})
        print(name, together[name], solo[name])
        assert solo_chrom == chrom and solo[name] == together[name], name
        if name != "bam":
            assert together[name][0] == together[name][1], name    # after the reset the same pass adds the same again
