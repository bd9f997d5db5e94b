"""The VCF reader's decision function on the CPU (no GPU): sg_vcf_row -- the code the device kernel runs, compiled for the
host -- against vcf_model, the plain-Python statement of the parser's rule: one hand-made fragment per clause with its
verdict written out, 20,000 seeded random fragments, the QUAL threshold against libc's atof at every precision; the same
function in a stand-alone program under the sanitizers; the refusal of a gzip file that is not BGZF before any device is
touched; and the layout of what the feature added to the ABI."""
import ctypes as C
import gzip
import os
import random
import re
import subprocess

import numpy as np
import pytest

import simuscop_amd
import vcf_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "simuscop_amd", "lib", "seqToProfile")
UND = ("undecided", 0, 0, 0, 0)


@pytest.mark.parametrize("i", range(len(M.CLAUSES)))
def test_one_fragment_per_clause(i):
    frag, verdict, on_device = M.CLAUSES[i]
    assert M.row(frag) == verdict and M.decided(frag) == on_device      # the model says what was written out by hand
    assert simuscop_amd.vcf_row(frag, M.KEYS) == (verdict if on_device else UND)


def test_the_test_inputs_hold_decided_forms_only():
    """What the GPU tests feed as "decided" text is: no fragment of it may be handed back."""
    for text in (M.random_text(1, 3000, odd=0.1), M.long_header_text(), M.random_text(2, 500, final_break=False)):
        assert M.parse(text)["undecided"] == []
    assert len(M.parse(M.clause_text())["undecided"]) == sum(1 for _, _, d in M.CLAUSES if not d)


def test_random_fragments():
    rng = random.Random(2024)
    odd = [b"1e3", b"2E1", b"inf", b"NaN", b"0x20", b" 40", b"1234567890123456", b"30e", b"5.e1"]
    n_und = 0
    for _ in range(20000):
        f = M.random_line(rng, 0.1)
        r = rng.random()
        if r < 0.15:
            f = f[:rng.randrange(1, len(f) + 1)]                       # cut anywhere: fewer fields, half a number
        elif r < 0.2:
            f = f.replace(b"\t", b"\0\t", 1) if r < 0.17 else f + b"\0"   # a NUL byte
        elif r < 0.3 and f.count(b"\t") >= 9:
            p = f.split(b"\t")
            p[5] = rng.choice(odd)
            f = b"\t".join(p)
        want = M.row(f) if M.decided(f) else UND
        n_und += want is UND
        assert simuscop_amd.vcf_row(f, M.KEYS) == want, f
    assert n_und > 500
    long = M.mk(end=b"") + b"\t" + b"x" * (M.FRAG - len(M.mk(end=b"")) - 1)
    assert len(long) == M.FRAG and simuscop_amd.vcf_row(long, M.KEYS) == M.SNV
    lib = simuscop_amd.load_engine()
    r = simuscop_amd.SgVcfRecord()
    assert lib.sg_vcf_row(long + b"x", M.FRAG + 1, None, 0, C.byref(r)) == 1 and lib.sg_vcf_row(b"", 0, None, 0, C.byref(r)) == 1


def test_qual_threshold_against_atof():
    """(float)atof(QUAL) < 20.0f, as the parser writes it, through libc: the neighbours of 20 - 2^-20 =
    19.99999904632568359375 at every precision a decided text can have, whole numbers, signs, leading zeros, random
    decimals -- about 200,000 strings, each decided on its own and each as libc has it."""
    libc = C.CDLL(None)
    libc.atof.restype = C.c_double
    libc.atof.argtypes = [C.c_char_p]
    cut = "99999904632568359375"
    texts = set()
    for k in range(0, 14):                       # 19.<k digits of the threshold>, the last digit moved by -2 .. +2
        for d in range(-2, 3):
            frac = cut[:k]
            if k:
                frac = "%0*d" % (k, max(0, min(10 ** k - 1, int(frac) + d)))
            for lead in ("", "0", "+", "00"):
                texts.add(lead + "19" + ("." + frac if k else "") )
                texts.add(lead + "19." + frac + "0" * (13 - k))
    for whole in range(0, 45):
        for tail in ("", ".", ".0", ".5", ".999999", ".0000001"):
            for sign in ("", "+", "-"):
                texts.add(sign + str(whole) + tail)
    rng = random.Random(7)
    while len(texts) < 200000:
        a = rng.choice(["19", "20", "19", "%d" % rng.randrange(0, 100000), "1", "2"])
        k = rng.randrange(0, 16 - len(a))
        texts.add(a + ("." + "".join(rng.choice("0123456789") for _ in range(k)) if k else ""))
        texts.add("19." + "9" * rng.randrange(1, 7) + "".join(rng.choice("0123456789") for _ in range(rng.randrange(0, 7))))
    texts.update([".5", ".", "", "-0", "-.5", "+.99", "20.000000000000", "19.99999904632", "19.999999046326", "19.9999990463256", "19.9999990463257"])
    lib = simuscop_amd.load_engine()
    keys = (C.c_char_p * 1)(b"20")
    r = simuscop_amd.SgVcfRecord()
    n_below = 0
    texts = sorted(t for t in texts if sum(c.isdigit() for c in t) <= 15)   # (longer digit strings are not decided on the device)
    assert len(texts) > 190000
    for t in texts:
        frag = b"chr20\t5\t.\tA\tC\t" + t.encode() + b"\tPASS\t.\tGT\t0/1\n"
        assert lib.sg_vcf_row(frag, len(frag), keys, 1, C.byref(r)) == 0
        below = bool(np.float32(libc.atof(t.encode())) < np.float32(20.0))
        assert below == bool(np.float32(M.c_atof(t.encode())) < np.float32(20.0)), t       # the model's atof is libc's
        assert r.kind == (0 if below else 1), t
        n_below += below
    assert 1000 < n_below < len(texts) - 1000
    assert np.float32(libc.atof(b"19.999999")) < np.float32(20) and not np.float32(libc.atof(b"19.9999999")) < np.float32(20)


def test_the_decision_function_under_the_sanitizers(tmp_path):
    """tools/vcf_row_sanitized.sh: sg::vcf_decide in a stand-alone program with its own main, AddressSanitizer +
    UndefinedBehaviorSanitizer, against the parser's loop body written there with atoi / atof / atol.  CPU only, no Python
    in that process, nothing preloaded."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "vcf_row_sanitized.sh"), "30000", "77"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    assert "all as the parser has them" in r.stdout


def test_a_gzip_file_that_is_not_bgzf_is_refused_before_any_device_is_touched(tmp_path):
    vcf = str(tmp_path / "x.vcf.gz")
    open(vcf, "wb").write(gzip.compress(M.clause_text()))
    out = str(tmp_path / "x.profile")
    r = subprocess.run([EXE, "--sam", str(tmp_path / "absent.sam"), "-v", vcf, "-r", str(tmp_path / "absent.fa"), "-o", out], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and not os.path.exists(out)
    assert r.stderr.strip() == "Error: VCF file %s is gzip-compressed but not BGZF: decompress it, or recompress it with bgzip" % vcf
    with pytest.raises(simuscop_amd.SimuError, match="not BGZF"):
        simuscop_amd.train_profile(str(tmp_path / "absent.fa"), vcf, out, sam=str(tmp_path / "absent.sam"), device_vcf=True)


def test_the_additions_stand_at_the_end_of_the_abi():
    hdr = open(os.path.join(ROOT, "include", "simuscop_amd.h")).read()
    names = re.findall(r"^(?:int|void|uint\d+_t|const char\*)\s+(sg_[a-z_0-9]+)\s*\(", hdr, flags=re.M)
    new = ["sg_vcf_begin", "sg_vcf_feed", "sg_vcf_feed_bgzf", "sg_vcf_undecided", "sg_vcf_finish", "sg_vcf_rows", "sg_vcf_end", "sg_vcf_row"]
    assert names[-len(new):] == new and simuscop_amd.ENGINE_SYMBOLS[-len(new):] == new
    lib = simuscop_amd.load_engine()
    for n in new:
        assert hasattr(lib, n)
    assert simuscop_amd.SimuTrainOptions._fields_[-1][0] == "device_vcf"
    assert [f[0] for f in simuscop_amd.SimuTrainStats._fields_[-5:]] == ["t_vcf", "vcf_bytes", "vcf_fragments", "vcf_undecided", "vcf_on_device"]
    th = open(os.path.join(ROOT, "simuscop_amd", "csrc", "host", "train.h")).read()
    assert th.index("int32_t decode_bam;") < th.index("int32_t device_vcf;") < th.index("} simu_train_options;")
    assert th.index("double t_inflate;") < th.index("double t_vcf;") < th.index("int32_t vcf_on_device;") < th.index("} simu_train_stats;")
    # simu_train_default_options clears exactly the struct: its size in C is the one ctypes lays out
    host = simuscop_amd.load_host()
    size = C.sizeof(simuscop_amd.SimuTrainOptions)
    buf = (C.c_ubyte * (size + 64))(*([0xEE] * (size + 64)))
    host.simu_train_default_options.argtypes = [C.c_void_p]
    host.simu_train_default_options.restype = None
    host.simu_train_default_options(C.cast(buf, C.c_void_p))
    assert all(b == 0xEE for b in buf[size:]) and bytes(buf[size - 8:size - 4]) == b"\0\0\0\0"
    assert C.sizeof(simuscop_amd.SgVcfRecord) == 32 and C.sizeof(simuscop_amd.SgVcfFragment) == 24 and C.sizeof(simuscop_amd.SgVcfCounts) == 21 * 8
