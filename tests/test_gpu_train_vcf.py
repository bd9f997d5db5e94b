"""`seqToProfile -v x.vcf.gz` and `-v x.vcf --device-vcf` on the MI355X: the VCF inflated and parsed on the device
(sg_vcf.hip) trains the .profile and .gc, byte for byte, that the host's fgets loop trains on the same text -- on the small
whole-genome and exome inputs of test_gpu_train.py (known SNVs, an insertion, a deletion, rows the filters drop, a contig
the FASTA lacks) -- with the same warnings, the same "total ..." line and the same exit codes; then what the route refuses."""
import gzip
import hashlib
import json
import os
import random
import subprocess

import pytest

import bam_util as B
import test_gpu_train as G
import train_util as TU
import vcf_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "simuscop_amd", "lib", "seqToProfile")


GOLDEN = os.path.join(ROOT, "tests", "golden", "train_vcf_default_route.json")


def build_inputs(oracle_lib, tmp_path_factory):
    """{exome: (fasta, vcf, bed, sam path)}; the reads are sampled once."""
    out = {}
    base = str(tmp_path_factory.mktemp("vcf_reads"))
    lines, fa1, T = G._sampled_lines(oracle_lib, base, coverage=6)
    for exome in (False, True):
        wd = str(tmp_path_factory.mktemp("vcf_wes" if exome else "vcf_wgs"))
        fa, vcf, bed, sam = TU.training_inputs(wd, fa1, lines, T.L, exome=exome)
        sam_path = os.path.join(wd, "reads.sam")
        open(sam_path, "wb").write(sam)
        out[exome] = (fa, vcf, bed, sam_path)
    return out


@pytest.fixture(scope="module")
def inputs(oracle_lib, tmp_path_factory):
    return build_inputs(oracle_lib, tmp_path_factory)


def default_route_digests(inp, exe, out):
    """`exe --sam ... -v known.vcf` with no VCF option: sha256 of the .profile behind its two first lines (the time stamp,
    the reads' path) and of the .gc file (None without one), and the --stats line."""
    fa, vcf, bed, sam = inp
    r = subprocess.run([exe, "--sam", sam, "-v", vcf, "-r", fa, "-o", out, "--quiet", "--stats", *(["-t", bed] if bed else [])], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    st = json.loads(r.stderr.decode().strip().splitlines()[-1])
    gc = hashlib.sha256(open(out + ".gc", "rb").read()).hexdigest() if os.path.exists(out + ".gc") else None
    return {"profile": hashlib.sha256(open(out, "rb").read().split(b"\n", 2)[2]).hexdigest(), "gc": gc}, st


def _run(args, quiet=False):
    r = subprocess.run([EXE, *args, "--stats"] + (["--quiet"] if quiet else []), capture_output=True, timeout=600)
    err = r.stderr.decode(errors="replace")
    stats = [json.loads(x) for x in err.splitlines() if x.startswith("{")]
    return r, err, stats[-1] if stats else None


def _vcf_lines(err, path):
    """The VCF's lines of stderr, the file's name taken out."""
    return [ln.replace(path, "<vcf>") for ln in err.splitlines() if ln.startswith("Warning: malformed VCF") or (ln.startswith("total ") and " SNPs, " in ln)]


def _train(inp, vcf, out, extra=()):
    fa, _, bed, sam = inp
    r, err, st = _run(["--sam", sam, "-v", vcf, "-r", fa, "-o", out, *(["-t", bed] if bed else []), *extra])
    return r, err, st


def _body(path):
    return open(path, "rb").read().split(b"\n", 1)[1]   # (the first line is the time stamp)


def _same_outputs(a, b):
    assert _body(a) == _body(b)
    assert os.path.exists(a + ".gc") == os.path.exists(b + ".gc")
    if os.path.exists(a + ".gc"):
        assert open(a + ".gc", "rb").read() == open(b + ".gc", "rb").read()


@pytest.mark.parametrize("exome", [False, True])
def test_the_three_routes_train_one_profile(exome, inputs, tmp_path):
    inp = inputs[exome]
    vcf = inp[1]
    text = open(vcf, "rb").read()
    want_model = M.parse(text, [b"1", b"2", b"X", b"S", b"M", b"3"])
    assert not want_model["undecided"]          # the shipped input holds decided forms only
    gz = str(tmp_path / "known.vcf.gz")
    open(gz, "wb").write(B.bgzf(text, member=700 if exome else 65280, level=6))
    want, got_gz, got_dev = (str(tmp_path / n) for n in ("host.profile", "gz.profile", "dev.profile"))
    r, err_h, st_h = _train(inp, vcf, want)
    assert r.returncode == 0, err_h[-2000:]
    assert st_h["vcf_on_device"] == 0 and st_h["vcf_undecided"] == 0 and st_h["vcf_bytes"] == len(text)
    assert st_h["vcf_fragments"] == want_model["fragments"] and st_h["t_vcf"] >= 0
    total = "total %d SNPs, %d inserts and %d deletions were loaded from file <vcf>" % tuple(want_model["n"][k] for k in ("snv", "ins", "del"))
    assert _vcf_lines(err_h, vcf) == [total]
    r, err, st = _train(inp, gz, got_gz)          # fails on a build without the device route: the compressed bytes go to fgets
    assert r.returncode == 0, err[-2000:]
    _same_outputs(want, got_gz)
    assert _vcf_lines(err, gz) == [total] and "EOF marker" not in err
    assert (st["vcf_on_device"], st["vcf_undecided"], st["vcf_bytes"], st["vcf_fragments"]) == (1, 0, len(text), want_model["fragments"])
    r, err, st = _train(inp, vcf, got_dev, ["--device-vcf"])
    assert r.returncode == 0, err[-2000:]
    _same_outputs(want, got_dev)
    assert _vcf_lines(err, vcf) == [total]
    assert (st["vcf_on_device"], st["vcf_undecided"], st["vcf_bytes"], st["vcf_fragments"]) == (1, 0, len(text), want_model["fragments"])
    for c in ("lines", "reads_counted", "gc_windows", "gc_pairs"):
        assert st[c] == st_h[c]


def test_undecided_rows_are_resolved_on_the_host(inputs, tmp_path):
    """QUAL written with an exponent on a known SNV, a known deletion and a dropped row, a malformed line between them: the
    device hands exactly those back, the profile is the host route's, the warning keeps its line number."""
    inp = inputs[False]
    rows = open(inp[1], "rb").read().split(b"\n")
    planted = 0
    for i, ln in enumerate(rows):
        f = ln.split(b"\t")
        if len(f) >= 10 and (f[1] in (b"60000", b"2019", b"777", b"3000")):
            f[5] = b"5e1" if f[1] != b"777" else b"5E+1"
            rows[i] = b"\t".join(f)
            planted += 1
    assert planted == 4
    rows.insert(5, b"chr1\t12\tshort")
    text = b"\n".join(rows)
    vcf, gz = str(tmp_path / "odd.vcf"), str(tmp_path / "odd.vcf.gz")
    open(vcf, "wb").write(text)
    open(gz, "wb").write(B.bgzf(text, member=300))
    assert len(M.parse(text)["undecided"]) == 3   # (the row DP=5 drops is decided before its QUAL is read)
    outs = [str(tmp_path / n) for n in ("h.profile", "g.profile", "d.profile")]
    res = [_train(inp, vcf, outs[0]), _train(inp, gz, outs[1]), _train(inp, vcf, outs[2], ["--device-vcf"])]
    for r, err, st in res:
        assert r.returncode == 0, err[-2000:]
    _same_outputs(outs[0], outs[1])
    _same_outputs(outs[0], outs[2])
    assert _vcf_lines(res[0][1], vcf) == _vcf_lines(res[1][1], gz) == _vcf_lines(res[2][1], vcf)
    assert _vcf_lines(res[0][1], vcf)[0].endswith("@line 6")
    assert [st["vcf_undecided"] for _, _, st in res] == [0, 3, 3]
    # and the rows matter: without the VCF's known variants the profile is another one
    none = str(tmp_path / "none.vcf")
    open(none, "wb").write(b"##fileformat=VCFv4.2\n")
    r, err, st = _train(inp, none, str(tmp_path / "n.profile"))
    assert r.returncode == 0 and _body(str(tmp_path / "n.profile")) != _body(outs[0])


def test_more_than_ten_malformed_lines_end_the_run_on_every_route(inputs, tmp_path):
    inp = inputs[False]
    text = open(inp[1], "rb").read() + b"".join(b"chr1\t%d\tbad\n" % i for i in range(14))
    vcf, gz = str(tmp_path / "bad.vcf"), str(tmp_path / "bad.vcf.gz")
    open(vcf, "wb").write(text)
    open(gz, "wb").write(B.bgzf(text, member=200))
    seen = []
    for k, (path, extra) in enumerate([(vcf, []), (gz, []), (vcf, ["--device-vcf"])]):
        out = str(tmp_path / ("o%d.profile" % k))
        r, err, st = _train(inp, path, out, extra)
        assert r.returncode == 1 and not os.path.exists(out), err[-1500:]
        seen.append(_vcf_lines(err, path))
    assert len(seen[0]) == 11 and seen[0] == seen[1] == seen[2]


def test_what_the_route_refuses(inputs, tmp_path):
    inp = inputs[False]
    text = open(inp[1], "rb").read()
    # gzip, but not BGZF
    plain_gz = str(tmp_path / "plain.vcf.gz")
    open(plain_gz, "wb").write(gzip.compress(text))
    out = str(tmp_path / "a.profile")
    r, err, _ = _train(inp, plain_gz, out)
    assert r.returncode == 1 and not os.path.exists(out)
    assert plain_gz in err and "not BGZF" in err and "bgzip" in err
    # no EOF member: a warning
    gz = B.bgzf(text, member=500, eof=False)
    noeof = str(tmp_path / "noeof.vcf.gz")
    open(noeof, "wb").write(gz)
    want, got = str(tmp_path / "w.profile"), str(tmp_path / "b.profile")
    assert _train(inp, inp[1], want)[0].returncode == 0
    r, err, st = _train(inp, noeof, got)
    assert r.returncode == 0 and "EOF marker" in err, err[-1500:]
    _same_outputs(want, got)
    # a member cut short, a corrupt one: an error naming the offset, no output file
    mem = B.members(gz)[0]
    cut = str(tmp_path / "cut.vcf.gz")
    open(cut, "wb").write(gz[:mem[3][0] + 20])
    out = str(tmp_path / "c.profile")
    r, err, _ = _train(inp, cut, out)
    assert r.returncode != 0 and not os.path.exists(out) and "file offset %d" % mem[3][0] in err, err[-1500:]
    at = mem[2][0] + mem[2][1] + 1 - 8
    bad = str(tmp_path / "crc.vcf.gz")
    open(bad, "wb").write(gz[:at] + bytes([gz[at] ^ 1]) + gz[at + 1:] + B.EOF_MEMBER)
    out = str(tmp_path / "d.profile")
    r, err, _ = _train(inp, bad, out)
    assert r.returncode != 0 and not os.path.exists(out) and "file offset %d" % mem[2][0] in err and "CRC-32" in err, err[-1500:]


@pytest.mark.parametrize("exome", [False, True])
def test_the_default_route_writes_the_profile_recorded_before_the_device_route_existed(exome, inputs, tmp_path):
    """No VCF option, a plain-text VCF: `vcf_on_device` = 0, and the .profile and .gc are the ones the build of the commit
    before this feature wrote on the same seeded inputs (tests/golden/train_vcf_default_route.json: recorded with that
    commit's seqToProfile; parse_vcf has since been cut into vcf_fragment and its loop)."""
    got, st = default_route_digests(inputs[exome], EXE, str(tmp_path / "d.profile"))
    assert st["vcf_on_device"] == 0 and st["vcf_undecided"] == 0
    assert got == json.load(open(GOLDEN))["wes" if exome else "wgs"]


def _extra_block(fa, L, alt):
    """Reads of a new visit to chr2 and then to chr1, ascending, so that countGC counts every one: on chr2 one with an insertion
    of 2 behind position 1029 and one with a deletion of 3 at 2020 (the events of train_util's known.vcf, on reads that are
    reached); on chr1 three that show the alternative allele `alt` at position 20000 (a heterozygous SNV counts only where a
    read shows its allele, Profile.cpp:404-415)."""
    seqs = {}
    for chunk in open(fa, "rb").read().split(b">")[1:]:
        name, seq = chunk.split(b"\n", 1)
        seqs[name.split()[0]] = seq.replace(b"\n", b"")
    c2, rng = seqs[b"chr2"], random.Random(19)
    rows = [(p, None) for p in sorted(rng.randrange(900, 2600) for _ in range(120))] + [(1000, b"30M2I%dM" % (L - 32)), (2000, b"20M3D%dM" % (L - 20))]
    block = [TU._crafted(rng, b"chr2", c2, p, L, 300, cigar=cg) for p, cg in sorted(rows, key=lambda r: r[0])]
    block += [TU._crafted(rng, b"chr1", seqs[b"chr1"], 20000 - off, L, 300, alt_at=(off, alt[0])) for off in (70, 40, 10)]
    return b"".join(ln + b"\n" for ln in block)


def test_the_model_is_the_real_host_route(inputs, tmp_path):
    """vcf_model against parse_vcf itself, through what it trains.  One crafted VCF per clause, one data row each, trained by
    the HOST route; the model's kept rows (kind, pos, contig, length or allele, homo flag) say which files must train the same
    profile and which must not.  The rows sit where the reads make them count: an SNV on chr1 under the sampled reads (a
    homozygous one changes the reference the substitutions are counted against, a heterozygous one only what is counted
    for the reads that show its allele), an insertion and a deletion that reads of the block above carry in their CIGARs (a known event is not counted).  Fourteen
    files: "chrom1" for the contig, REF and ALT both long for the deletion."""
    fa, vcf, _, sam = inputs[False]
    snv = next(ln.split(b"\t") for ln in open(vcf, "rb") if ln.startswith(b"chr1\t20000\t"))
    ref, alt = snv[3], snv[4]
    L = len(open(sam, "rb").readline().split(b"\t")[9])
    sam2 = str(tmp_path / "reads.sam")
    open(sam2, "wb").write(open(sam, "rb").read() + _extra_block(fa, L, alt))
    s = lambda **kw: M.mk(**{**dict(chrom=b"chr1", pos=b"20000", ref=ref, alt=alt, qual=b"50", info=b"DP=30"), **kw})   # noqa: E731
    d = lambda **kw: M.mk(**{**dict(chrom=b"chr2", pos=b"2019", ref=b"ACGT", alt=b"A"), **kw})                           # noqa: E731
    files = {
        "none": b"",
        "snv": s(chrom=b"chrom1"), "snv_unknown_contig": s(chrom=b"chr9"),
        "snv_dp9": s(info=b"DP=9"), "snv_dp10": s(info=b"DP=10"),
        "snv_q_below": s(qual=b"19.999999"), "snv_q_at": s(qual=b"19.9999999"),
        "snv_het": s(sample=b"1/1:9,9"), "snv_gt_with_break": s(fmt=b"GT", sample=b"1/1"),
        "del": d(alt=b"ACG"), "del_one_before": d(pos=b"2018"), "del_shorter": d(ref=b"ACG"),
        "ins": d(pos=b"1029", ref=b"A", alt=b"ACG"), "ins_longer": d(pos=b"1029", ref=b"A", alt=b"ACGT"),
    }
    keys = [b"1", b"2", b"X", b"S", b"M", b"3"]
    sig, body = {}, {}
    for name, row in files.items():
        text = b"##fileformat=VCFv4.2\n" + row
        path, out = str(tmp_path / (name + ".vcf")), str(tmp_path / (name + ".profile"))
        open(path, "wb").write(text)
        r, err, st = _run(["--sam", sam2, "-v", path, "-r", fa, "-o", out])
        assert r.returncode == 0 and st["vcf_on_device"] == 0, err[-1500:]
        body[name] = open(out, "rb").read().split(b"\n", 2)[2]
        m = M.parse(text, keys)
        sig[name] = tuple((k, r[1:]) for k in ("snv", "ins", "del") for r in m["rows"][k])
        assert ("total %d SNPs, %d inserts and %d deletions" % tuple(m["n"][k] for k in ("snv", "ins", "del"))) in err
    # what the model says of each file, written out
    kept = (20000, 0, alt[0], M.KNOWN | M.HOMO)
    assert sig["none"] == sig["snv_unknown_contig"] == sig["snv_dp9"] == sig["snv_q_below"] == ()
    assert sig["snv"] == sig["snv_dp10"] == sig["snv_q_at"] == sig["snv_gt_with_break"] == (("snv", kept),)
    assert sig["snv_het"] == (("snv", (20000, 0, alt[0], M.KNOWN)),)
    assert sig["del"] == (("del", (2020, 1, 3, M.KNOWN)),) and sig["del_one_before"] == (("del", (2019, 1, 3, M.KNOWN)),)
    assert sig["del_shorter"] == (("del", (2020, 1, 2, M.KNOWN)),) and sig["ins"] == (("ins", (1029, 1, 2, M.KNOWN)),)
    # rows that meet the reads: equal rows, equal profile; other rows, another profile
    met = [n for n in files if n not in ("del_one_before", "del_shorter", "ins_longer")]
    for a in met:
        for b in met:
            assert (body[a] == body[b]) == (sig[a] == sig[b]), (a, b)
    # a deletion one base off, or of another length, and an insertion of another length are no event any read has: kept by the
    # model, and the profile is the one without variants -- position + 1 and the lengths are exactly the parser's
    for n in ("del_one_before", "del_shorter", "ins_longer"):
        assert sig[n] != () and body[n] == body["none"], n
