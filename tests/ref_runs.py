"""The unmodified reference binary's run on a configuration, for the tests that hold oracle(mt) to it byte for byte.

Where oracle/_ref/simuReads is built (`make -C oracle ref`) it runs here and now under the frozen clock of
oracle/fakeclock.c, and what it did must be what tests/golden/reference_runs.json recorded; elsewhere the record stands in
for it.  A record is the binary's exit status (None: it never returned within the time limit) and the md5 of every file it
wrote.  SIMU_REFERENCE_RECORD=1 (with the binary built) writes the records of the tests that run instead of checking them."""
import hashlib
import json
import os
import subprocess

import pytest

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "simuReads")
SHIM = os.path.join(ROOT, "oracle", "_ref", "libfakeclock.so")
RECORDS = os.path.join(ROOT, "tests", "golden", "reference_runs.json")


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
