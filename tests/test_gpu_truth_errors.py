"""`simuReads --truth-errors` on the MI355X through the command line: <stem>.truth.errors.tsv.

On a variant-free A/C/G/T genome the template of a read is the reference under it, so the whole Q block follows from the
same run's truth BAM and the FASTA, with no use of the engine's rule: every M base of every record against the reference
base under it, its cycle counted from the record's other end for a reverse read; the I and S operations are the inserted
bases (an insertion behind a read's last base has no M base behind it and is clipped); what a record's M bases leave of
its template was deleted.  Further: the host-haplotype route, stems, --no-write, and that the option only adds."""
import hashlib
import os
import re

import numpy as np
import pytest

import cases
import errors_model as EM
import test_gpu_truth_bam as TB
import truth_util as U

pytestmark = pytest.mark.gpu

SUFFIX = ".truth.errors.tsv"


def read_errors(path):
    return EM.parse_file(open(path, "rb").read())


def q_of_records(recs, seqs, refs, L):
    """{(mate, cycle, qual): [bases, errors, inserted]} of the records' M and I / S bases, the M bases, the D bases inside
    the alignments and the template bases no M base accounts for."""
    ref = [np.frombuffer(seqs[name.decode()], dtype=np.uint8) for name, _ in refs]
    cells = {}
    m_total = d_cigar = gone = 0

    def bump(key, col, n=1):
        cells.setdefault(key, [0, 0, 0])[col] += n
    for rec in recs:
        if not rec["ops"]:
            continue
        mate = 2 if rec["flag"] & 0x80 else 1
        rev = bool(rec["flag"] & 0x10)
        n = len(rec["seq"])
        seq = np.frombuffer(rec["seq"], dtype=np.uint8)
        qual = np.frombuffer(rec["qual"], dtype=np.uint8).astype(np.int64) - 33
        i, p, m_rec = 0, rec["pos"], 0
        for k, o in rec["ops"]:
            if o == 0:
                idx = np.arange(i, i + k)
                cyc = (n - 1 - idx if rev else idx) + 1
                wrong = seq[idx] != ref[rec["rid"]][p:p + k]
                for c, q, w in zip(cyc.tolist(), qual[idx].tolist(), wrong.tolist()):
                    bump((mate, c, q), 0)
                    if w:
                        bump((mate, c, q), 1)
                m_rec += k
            elif o in (1, 4):
                for x in range(i, i + k):
                    bump((mate, (n - x if rev else x + 1), int(qual[x])), 2)
            elif o == 2:
                d_cigar += k
            else:
                raise AssertionError("a skip on a genome without targets")
            if o in (0, 1, 4):
                i += k
            if o in (0, 2):
                p += k
        assert i == n
        m_total += m_rec
        gone += L - m_rec
    return cells, m_total, d_cigar, gone


@pytest.fixture(scope="module")
def acgt(tmp_path_factory):
    """One `--truth-bam --truth-depth 1000 --truth-errors` run of the XTen profile on an A/C/G/T-only genome."""
    wd = str(tmp_path_factory.mktemp("acgt"))
    cfg, fa, seqs = U.acgt_case(wd, os.path.join(cases.TESTDATA, cases.PROFILES["xten"]), "PE")
    out = os.path.join(wd, "errors_out")
    err = TB.simu(cfg, out, "--truth-bam", "--truth-depth", "1000", "--truth-errors").stderr
    (stem,) = TB.stems(out)
    return cfg, out, err, stem, seqs


def test_q_block_equals_the_truth_bam_against_the_fasta(acgt):
    cfg, out, err, stem, seqs = acgt
    _, refs, recs, _ = U.read_truth_bam(os.path.join(out, stem + ".truth.bam"))
    L = 151
    want, m_total, d_cigar, gone = q_of_records(recs, seqs, refs, L)
    got = read_errors(os.path.join(out, stem + SUFFIX))
    assert len(recs) > 4000 and m_total > 500000
    keys = set(want) | set(got["Q"])
    bad = [k for k in sorted(keys) if tuple(want.get(k, [0, 0, 0])) != (got["Q"].get(k, (0, 0, 0, 0))[0], got["Q"].get(k, (0, 0, 0, 0))[1],
                                                                          got["Q"].get(k, (0, 0, 0, 0))[3])]
    assert not bad, (len(bad), bad[0], want.get(bad[0]), got["Q"].get(bad[0]))
    assert all(v[2] == 0 for v in got["Q"].values())                 # no `other` on an A/C/G/T genome
    n_err = sum(v[1] for v in want.values())
    n_ins = sum(v[2] for v in want.values())
    assert 0 < n_err < m_total // 5 and n_ins > 0 and {k[0] for k in want} == {1, 2}
    assert sum(b for _, b in got["I"].values()) == n_ins
    # the D block: every template base no M base accounts for was deleted.  The CIGAR holds the deletions between two M
    # runs; one at a read's first base (index 1) or one that reaches the template's end (clipped to room = L + 1 - index
    # bases) has no M base on one side and never shows.  A row sums its events: x of its `events` reached the end where
    # bases == x * room + (the others, 1 .. room - 1 bases each), which bounds x from both sides and fixes it in all
    # but the last few rows.
    d_bases = sum(b for _, b in got["D"].values())
    assert d_bases == gone and d_cigar > 0
    edge_lo = edge_hi = 0
    for (m, j), (ev, b) in got["D"].items():
        room = L + 1 - j
        assert 1 <= room and ev <= b <= ev * room
        if j == 1:
            x_lo = x_hi = b                                          # every base of a deletion at the first base
            room = 1
        elif room == 1:
            x_lo = x_hi = ev
        else:
            x_lo, x_hi = max(0, b - ev * (room - 1)), (b - ev) // (room - 1)
        edge_lo, edge_hi = edge_lo + x_lo * room, edge_hi + x_hi * room
    print("D: %d bases, %d in CIGARs, %d..%d at the reads' ends" % (d_bases, d_cigar, edge_lo, edge_hi))
    assert d_bases - edge_hi <= d_cigar <= d_bases - edge_lo
    # the matrix: its diagonal and the rest are the two columns
    s_all = sum(got["S"].values())
    s_diag = sum(v for (m, f, t), v in got["S"].items() if f == t)
    assert s_all == m_total and s_all - s_diag == n_err
    assert TB.stat(err, "errors_bases") == m_total == TB.stat(err, "depth_bases") and TB.stat(err, "errors_subst") == n_err
    assert float(re.search(r"errors_s=([0-9.]+)", err).group(1)) >= 0


def test_host_haplotypes_give_the_same_file(acgt, tmp_path):
    cfg, out, err, stem, _ = acgt
    host = str(tmp_path / "host")
    r = TB.simu(cfg, host, "--truth-errors", "--host-haplotypes")
    assert open(os.path.join(host, stem + SUFFIX), "rb").read() == open(os.path.join(out, stem + SUFFIX), "rb").read()
    assert TB.stat(r.stderr, "errors_bases") == TB.stat(err, "errors_bases")


def test_no_write_counts_and_writes_nothing(acgt, tmp_path):
    cfg, _, err, _, _ = acgt
    out = str(tmp_path / "nowrite")
    r = TB.simu(cfg, out, "--no-write", "--truth-errors")
    assert TB.stat(r.stderr, "errors_bases") == TB.stat(err, "errors_bases") > 0
    assert TB.stat(r.stderr, "errors_subst") == TB.stat(err, "errors_subst") > 0
    assert not os.path.exists(out) or not os.listdir(out)


def test_the_option_only_adds(acgt, tmp_path):
    cfg, out, err, stem, _ = acgt
    plain = str(tmp_path / "plain")
    perr = TB.simu(cfg, plain, "--truth-bam", "--truth-depth", "1000").stderr
    files = sorted(os.listdir(plain))
    assert files and files == sorted(x for x in os.listdir(out) if not x.endswith(SUFFIX))
    assert any(x.endswith(".truth.bam") for x in files) and any(x.endswith(".fq") for x in files) and any(x.endswith(".bedgraph") for x in files)
    md5 = lambda p: hashlib.md5(open(p, "rb").read()).hexdigest()
    for f in files:
        assert md5(os.path.join(plain, f)) == md5(os.path.join(out, f)), f
    assert TB.stat(perr, "errors_bases") == 0 and TB.stat(perr, "errors_subst") == 0 and re.search(r"errors_s=0\.000\b", perr)
    assert TB.stat(err, "errors_bases") > 0


def test_pieces_give_the_same_file(acgt, tmp_path):
    cfg, out, err, stem, _ = acgt
    cut = str(tmp_path / "cut")
    r = TB.simu(cfg, cut, "--truth-errors", env={"SIMU_PIECE_SLOTS": "1", "SIMU_TRACE_PIECES": "1"})
    assert r.stderr.count("[piece]") >= 2                            # (a segment is never cut: at least a piece a contig)
    assert open(os.path.join(cut, stem + SUFFIX), "rb").read() == open(os.path.join(out, stem + SUFFIX), "rb").read()


def test_every_stem_gets_its_own_table(tmp_path):
    """Two abundance rows, two stems, on a variant-free A/C/G/T genome with two populations: the config writes every
    abundance row to a stem of its own, so each stem's file is compared, cell by cell and exactly, with the table made
    of that stem's own truth BAM against the FASTA (as the one-stem test above does).  A table that is not zeroed
    between the stems, or a read counted for the other stem, moves a cell.  The stats sum both stems."""
    wd = str(tmp_path)
    _, fa, seqs = U.acgt_case(wd, os.path.join(cases.TESTDATA, cases.PROFILES["xten"]), "PE")
    cases._write(os.path.join(wd, "abundance.txt"), ["1.0\t0", "0.4\t0.6"])
    cfg = os.path.join(wd, "two_stems.txt")
    cases._config(cfg, ref=fa, profile=os.path.join(cases.TESTDATA, cases.PROFILES["xten"]), name="a, b",
                  abundance=os.path.join(wd, "abundance.txt"), output=os.path.join(wd, "out"), layout="PE", threads=1, verbose=0,
                  coverage=3, insertSize=400)
    out = os.path.join(wd, "errors_out")
    err = TB.simu(cfg, out, "--truth-bam", "--truth-errors").stderr
    stems = TB.stems(out)
    assert len(stems) == 2 and sorted(x[:-len(SUFFIX)] for x in os.listdir(out) if x.endswith(SUFFIX)) == stems
    L = 151
    bases_all = errors_all = 0
    tables = []
    for stem in stems:
        _, refs, recs, _ = U.read_truth_bam(os.path.join(out, stem + ".truth.bam"))
        want, m_total, _, gone = q_of_records(recs, seqs, refs, L)
        got = read_errors(os.path.join(out, stem + SUFFIX))
        assert len(recs) > 1000 and m_total > 100000, stem
        mine = {k: [v[0], v[1], v[3]] for k, v in got["Q"].items()}
        bad = [k for k in sorted(set(want) | set(mine)) if want.get(k, [0, 0, 0]) != mine.get(k, [0, 0, 0])]
        assert not bad, (stem, len(bad), bad[0], want.get(bad[0]), mine.get(bad[0]))
        assert all(v[2] == 0 for v in got["Q"].values()) and {k[0] for k in got["Q"]} == {1, 2} and len(got["S"]) == 40
        assert sum(got["S"].values()) == m_total and sum(b for _, b in got["D"].values()) == gone
        assert sum(b for _, b in got["I"].values()) == sum(v[2] for v in want.values())
        bases_all += m_total
        errors_all += sum(v[1] for v in want.values())
        tables.append(got["Q"])
    assert tables[0] != tables[1]
    assert TB.stat(err, "errors_bases") == bases_all and TB.stat(err, "errors_subst") == errors_all > 0
