"""The unmodified reference binaries' runs: simuReads on a configuration, for the tests that hold oracle(mt) to it byte for
byte, and seqToProfile on a training input (run_train), for the tests that hold profile training to it.

Where oracle/_ref/simuReads is built (`make -C oracle ref`) it runs here and now under the frozen clock of
oracle/fakeclock.c, and what it did must be what tests/golden/reference_runs.json recorded; elsewhere the record stands in
for it.  A record is the binary's exit status (None: it never returned within the time limit) and the md5 of every file it
wrote.  SIMU_REFERENCE_RECORD=1 (with the binary built) writes the records of the tests that run instead of checking them."""
import hashlib
import json
import os
import shlex
import subprocess

import pytest

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "simuReads")
SHIM = os.path.join(ROOT, "oracle", "_ref", "libfakeclock.so")
RECORDS = os.path.join(ROOT, "tests", "golden", "reference_runs.json")
TRAIN = os.path.join(ROOT, "oracle", "_ref", "seqToProfile")
TRAIN_RECORDS = os.path.join(ROOT, "tests", "golden", "reference_train_runs.json")
STUB_SAMTOOLS = os.path.join(ROOT, "tests", "stub_samtools.sh")


def md5s(d):
    return {f: hashlib.md5(open(os.path.join(d, f), "rb").read()).hexdigest() for f in sorted(os.listdir(d))} if os.path.isdir(d) else {}


def _records():
    return json.load(open(RECORDS)) if os.path.exists(RECORDS) else {}


def run(key, cfg, out, timeout):
    """(exit status or None, {file: md5}) of the reference on `cfg`, whose output directory is `out`; `key` names the
    record.  The files the binary wrote are removed again."""
    if not os.path.exists(REF):
        rec = _records().get(key)
        if rec is None:
            pytest.skip(f"no reference binary and no stored run for {key} (tests/golden/reference_runs.json)")
        return rec["rc"], rec["files"]
    env = dict(os.environ, LD_PRELOAD=SHIM, FAKECLOCK_SEC=str(cases.FAKE_SEC), FAKECLOCK_NSEC=str(cases.FAKE_NSEC))
    try:
        rc = subprocess.run([REF, cfg], env=env, capture_output=True, text=True, timeout=timeout).returncode
    except subprocess.TimeoutExpired:
        rc = None
    files = md5s(out)
    for f in files:
        os.remove(os.path.join(out, f))
    recs = _records()
    if os.environ.get("SIMU_REFERENCE_RECORD"):
        recs[key] = {"rc": rc, "files": files}
        with open(RECORDS + ".tmp", "w") as f:
            json.dump(recs, f, indent=1, sort_keys=True)
        os.replace(RECORDS + ".tmp", RECORDS)
    elif key in recs:
        assert (rc == 0, files) == (recs[key]["rc"] == 0, recs[key]["files"]), f"{key}: the reference binary no longer does what was recorded"
    return rc, files


def train_key(wd, names, opts):
    """The record key of a training run: md5 of the input files `names` (in `wd`, in this order) and the options."""
    h = hashlib.md5()
    for n in names:
        h.update(n.encode() + b"\0" + (open(os.path.join(wd, n), "rb").read() if n else b"") + b"\0")
    h.update(" ".join(opts).encode())
    return "train/" + h.hexdigest()


def run_train(wd, sam="reads.sam", fasta="train.fa", vcf="known.vcf", bed=None, kmer=3, bins=50, timeout=300):
    """(exit status, {file: md5}) of the reference seqToProfile on the files named (all in `wd`): it reads `sam` through
    tests/stub_samtools.sh, which stands in for `samtools view`, and writes ref.profile (and ref.profile.gc) there.  It runs
    in `wd` with relative names, so the `#reads:` line is the same everywhere, under the frozen clock of oracle/fakeclock.c,
    so `#model created at` is too.  Where oracle/_ref/seqToProfile is not built, tests/golden/reference_train_runs.json
    stands in for it (a missing record is a failure, not a skip); SIMU_REFERENCE_RECORD=1 writes the records instead."""
    opts = ["-b", sam, "-r", fasta, "-v", vcf, "-o", "ref.profile", "-k", str(kmer), "-B", str(bins)] + (["-t", bed] if bed else [])
    key = train_key(wd, [sam, fasta, vcf, bed or ""], opts)
    recs = json.load(open(TRAIN_RECORDS)) if os.path.exists(TRAIN_RECORDS) else {}
    if not os.path.exists(TRAIN):
        assert key in recs, f"no reference seqToProfile (make -C oracle ref) and no stored run for {key} (tests/golden/reference_train_runs.json)"
        return recs[key]["rc"], recs[key]["files"]
    outs = ("ref.profile", "ref.profile.gc")
    for f in outs:
        if os.path.exists(os.path.join(wd, f)):
            os.remove(os.path.join(wd, f))
    env = dict(os.environ, LD_PRELOAD=SHIM, FAKECLOCK_SEC=str(cases.FAKE_SEC), FAKECLOCK_NSEC=str(cases.FAKE_NSEC))
    # (`-s` is run by popen's shell: "sh <stub>" needs no execute bit on the checked-out script)
    r = subprocess.run([TRAIN] + opts + ["-s", "sh " + shlex.quote(STUB_SAMTOOLS)], cwd=wd, env=env, capture_output=True, timeout=timeout)
    files = {f: hashlib.md5(open(os.path.join(wd, f), "rb").read()).hexdigest() for f in outs if os.path.exists(os.path.join(wd, f))}
    if os.environ.get("SIMU_REFERENCE_RECORD"):
        recs[key] = {"rc": r.returncode, "files": files}
        with open(TRAIN_RECORDS + ".tmp", "w") as f:
            json.dump(recs, f, indent=1, sort_keys=True)
        os.replace(TRAIN_RECORDS + ".tmp", TRAIN_RECORDS)
    elif key in recs:
        assert (r.returncode, files) == (recs[key]["rc"], recs[key]["files"]), f"{key}: the reference seqToProfile no longer does what was recorded"
    return r.returncode, files
