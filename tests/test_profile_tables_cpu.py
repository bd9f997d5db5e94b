"""The profile-table builder (simuscop_amd/csrc/sg_profile_tables.cpp) word for word, without a GPU: the FASTQ is the
reference's only if every word of these tables is right.

tools/profile_tables_check.cpp is compiled with plain g++ from itself, the builder, sg_tables.cpp and the driver's profile
loader -- no HIP header, no engine library -- and run on the four shipped profiles (paired at insert size 350, and
single-end), on seeded synthetic profiles over every table shape (kmer 1..6, bins 1 and 7, one and two substitution
tables, both base orders, 1 / 41 / 128 quality symbols, rows with leading zero mass, indel rates of 0 and 1e-9, with and
without an insert-size table, reads of 1 and 30,000 bases) and on every refusal of the builder's checks.  Each case is one
line: word count, FNV-1a of the words, every field of the layout.  tests/profile_tables_expected.txt holds the recorded
lines; every line must match, so a change to the builder that moves or alters one word shows here."""
import os
import subprocess

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simuscop_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tools", "profile_tables_check.cpp"), os.path.join(CSRC, "sg_profile_tables.cpp"),
           os.path.join(CSRC, "sg_tables.cpp"), os.path.join(CSRC, "host", "profile.cpp")]


def test_tables_are_word_for_word_the_recorded_ones(tmp_path):
    exe = str(tmp_path / "profile_tables_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", *SOURCES, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    r = subprocess.run([exe, cases.TESTDATA], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    want = open(os.path.join(ROOT, "tests", "profile_tables_expected.txt")).read().splitlines()
    assert [ln.split()[0] for ln in got] == [ln.split()[0] for ln in want]
    for g, w in zip(got, want):
        assert g == w, w.split()[0]
    assert len(want) == 56 and sum(ln.startswith("Illumina_") for ln in want) == 8 and sum(ln.startswith("refuse_") for ln in want) == 23


def test_the_builder_includes_no_hip_header():
    """what lets the program above exist: neither file of the builder reaches hip_runtime.h, directly or through a header"""
    seen, todo = set(), [os.path.join(CSRC, "sg_profile_tables.cpp"), os.path.join(CSRC, "sg_profile_tables.h")]
    while todo:
        path = os.path.normpath(todo.pop())
        if path in seen:
            continue
        seen.add(path)
        for line in open(path):
            if line.startswith("#include <hip"):
                raise AssertionError("%s includes %s" % (path, line.strip()))
            if line.startswith('#include "'):
                todo.append(os.path.join(os.path.dirname(path), line.split('"')[1]))
    assert len(seen) >= 4
