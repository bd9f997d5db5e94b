"""tests/read_model.py against the whole oracle (CPU only).

orc_simulate(philox) is pinned to the reference binary; read_model.py rebuilds single records from orc_predict_philox and
a restated plan.  Here every record of a whole oracle run is rebuilt from the model, so that the GPU test that compares
the engine with the model read by read (test_gpu_reads_placed.py) compares it with the oracle.

The genome is one N-free contig of 8 x 1000 bases without variants: both haplotype strings are the contig, each is tiled
into eight full windows of 1,000 bases (Segment::fragSize), hap-major, and no window is shorter than a read -- a window
under-produces only after 1,001 failed attempts, and an attempt fails with probability < L / 1000.  The window table is
not exported by the oracle; `replay` recovers it from the records: window w's fragments are the successful attempts
(w, 0), (w, 1) ... in order, so the records are consumed window by window while the next successful attempt of the
model's plan lands on the next record's position.  Every record must be consumed (record count == planned count), the
attempt after a window's last fragment must not have been its 1,001st failure, and then a record's slot is its index."""
import os

import numpy as np
import pytest

import cases
import read_model as RM
from profile_shapes import Shape

SEC, NSEC = cases.FAKE_SEC, cases.FAKE_NSEC
SEED = (SEC << 32) | NSEC
L, INSERT, GENOME, COVERAGE = 60, 150, 8000, 45
SHAPE = Shape(3, 30, read_length=L, indel_scale=4.0)


def genome():
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(17).integers(0, 4, GENOME)].tobytes()


def run_oracle(lib, wd, layout):
    """(model, contig, records per mate file) of one oracle(philox) run"""
    os.makedirs(wd, exist_ok=True)
    prof = RM.one_column_profile(os.path.join(wd, "one_column.profile"), SHAPE)
    fa, contig = os.path.join(wd, "ref.fa"), genome()
    cases._fasta_of(fa, [(b"chrA", contig)])
    cfg = os.path.join(wd, "config.txt")
    cases._config(cfg, ref=fa, profile=prof, name="m", output=os.path.join(wd, "out"), layout=layout, threads=1, verbose=0,
                  coverage=COVERAGE, insertSize=INSERT)
    out = os.path.join(wd, "oracle_out")
    assert lib.orc_simulate(cfg.encode(), 1, SEC, NSEC, out.encode(), 1) == 0, lib.orc_last_error().decode()
    files = sorted(f for f in os.listdir(out) if ".fq" in f)
    assert len(files) == (2 if layout == "PE" else 1)
    recs = [RM.split_records(open(os.path.join(out, f), "rb").read()) for f in files]
    assert sum(len(r) for r in recs) == lib.orc_last_read_count()
    model = RM.ReadModel(lib, prof, layout == "PE", INSERT, SEED, 0, b"@m#A#")
    return model, contig, recs


@pytest.fixture(scope="module")
def pe_run(oracle_lib, tmp_path_factory):
    model, contig, recs = run_oracle(oracle_lib, str(tmp_path_factory.mktemp("pe")), "PE")
    yield model, contig, recs
    model.close()


def name_fields(rec, paired):
    """(pos % seg_size, fragment count) of a record's name"""
    name = rec.split(b"\n", 1)[0]
    assert name.startswith(b"@m#A#")
    if paired:
        assert name[-2:] in (b"/1", b"/2")
        name = name[:-2]
    pos, count = name[len(b"@m#A#"):].split(b"#")
    return int(pos), int(count)


def replay(model, recs):
    """The window table the records imply: per record (window, attempt, pos, flen, strand); see the module's docstring."""
    n_tiles, out, i = GENOME // 1000, [], 0
    for w in range(2 * n_tiles):
        win = (0, 0, (w % n_tiles) * 1000, 1000, 0, 0, 0)
        a = fail = 0
        while True:                      # draw to the next success; consume a record if it is that fragment
            pos, flen, strand = model.attempt(win, w, a, GENOME)
            a += 1
            if flen < model.L:
                fail += 1
                assert fail <= 1000, f"window {w} gave up: the records' slots are not their indices"
                continue
            if i < len(recs) and name_fields(recs[i], model.paired)[0] == pos:
                out.append((w, a - 1, pos, flen, strand))
                i += 1
            else:
                break
    return out


def test_one_column_insert_profile(pe_run):
    model = pe_run[0]
    assert model.n_isize == 1 and model.isz == INSERT + 1 and model.has_sub2 == 1 and model.L == L


def test_every_pe_record_is_the_models(pe_run, oracle_lib):
    """Both mates of every record of the run, rebuilt from the record's own position (its name) and its index as slot;
    no record is left out."""
    model, contig, (r1, r2) = pe_run
    planned_reads = GENOME * COVERAGE // L
    table = replay(model, r1)
    assert len(table) == len(r1) == len(r2) >= planned_reads // 2 > 2000, "the replayed plan does not account for every record"
    assert len({t[0] for t in table}) == 16 and any(t[3] < model.isz for t in table), "every window; fragments clipped by the end"
    classes, bad = {}, []
    for i, (w, a, pos, flen, _) in enumerate(table):
        assert name_fields(r1[i], True) == name_fields(r2[i], True) == (pos, i + 1) and pos < GENOME
        s = RM.Slot(w, 0, pos, pos, flen, 0, i + 1, a, 0)
        for mate, recs in ((0, r1), (1, r2)):
            want = model.slot_record([contig], s, mate, i, GENOME)
            if recs[i] != want:
                bad.append((i, mate, RM.first_cycle(recs[i], want)))
            ev, reset = model.events(mate, i)
            assert len(want.split(b"\n")[1]) == L + sum(n if k == "I" else -n for _, k, n in ev), (i, mate, ev)
            c = "reset" if reset else model.read_class(ev)
            classes[c] = classes.get(c, 0) + 1
    assert not bad, (len(bad), bad[:20])
    print("read classes", classes)
    assert min(classes.get(c, 0) for c in ("none", "ins", "del", "many")) >= 20, classes


def test_se_records_one_strand_each(oracle_lib, tmp_path):
    """Single-end: a fragment is its window's length (clipped by the end), the read its first L bases or the last L turned
    round.  No window table is used for the reads: exactly one of the two strands reproduces a record, both occur.  The
    replayed plan then says which (word 2 of the attempt's draw), and the count of records is the planned count exactly."""
    model, contig, (recs,) = run_oracle(oracle_lib, str(tmp_path), "SE")
    with model:
        assert len(recs) == GENOME * COVERAGE // L
        table = replay(model, recs)
        assert len(table) == len(recs)
        seen = [0, 0]
        for i, rec in enumerate(recs):
            pos, count = name_fields(rec, False)
            assert count == i + 1
            flen = min(1000, GENOME - pos)
            fits = [model.record(contig, pos if s == 0 else pos + flen - L, s == 1, 0, i, pos, GENOME, count) == rec for s in (0, 1)]
            assert sum(fits) == 1, (i, fits)
            assert fits[table[i][4]] and table[i][2:4] == (pos, flen), (i, table[i])
            seen[fits.index(True)] += 1
        assert min(seen) > len(recs) // 3, seen


MUTATION_CAPS = {"template shifted by one base": 0.002, "is_read1 flipped on mate 2": 0.002, "slot + 1": 0.002, "batch_id + 1": 0.002,
                 "reverse strand not complemented": 0.002}


def test_the_model_discriminates(pe_run):
    """The records of the PE run against the model with one thing wrong at a time.  Fraction of records that still match,
    measured on this run (2 x 3,005 records; the flip and the complement concern mate 2 alone): template shifted by one
    base 0 / 6010, is_read1 flipped on mate 2 0 / 3005, slot + 1 0 / 6010, batch_id + 1 0 / 6010, reverse strand not
    complemented 0 / 3005.  (A record is 60 bases of 2-30 % error and 60 qualities of 41 symbols: a wrong draw or table
    cannot leave it whole.)  The caps allow 0.2 %: six and twelve
    records."""
    model, contig, (r1, r2) = pe_run
    table = replay(model, r1)
    same = {k: [0, 0] for k in MUTATION_CAPS}

    def tally(key, rec, got):
        same[key][0] += rec == got
        same[key][1] += 1

    for i, (w, a, pos, flen, _) in enumerate(table):
        for mate, rec in ((0, r1[i]), (1, r2[i])):
            off, rev = (pos, False) if mate == 0 else (pos + flen - L, True)
            args = (pos, GENOME, i + 1)
            shifted = off + 1 if off + 1 + L <= GENOME else off - 1
            tally("template shifted by one base", rec, model.record(contig, shifted, rev, mate, i, *args))
            tally("slot + 1", rec, model.record(contig, off, rev, mate, i + 1, *args))
            tally("batch_id + 1", rec, model.record(contig, off, rev, mate, i, *args, batch_id=1))
            if mate == 1:
                tally("is_read1 flipped on mate 2", rec, model.record(contig, off, rev, mate, i, *args, is_read1=1))
                tally("reverse strand not complemented", rec, model.record(contig, off, rev, mate, i, *args, complement=False))
    print({k: f"{a} / {n}" for k, (a, n) in same.items()})
    for k, (a, n) in same.items():
        assert n >= len(r1) and a <= MUTATION_CAPS[k] * n, (k, a, n)


# ---- hand-worked plan cases -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_model(pe_run):
    return pe_run[0]


def words0(model, widx, n):
    return [model.philox(widx, a, 0, RM.KIND_PLAN, model.batch_id & 0xFFFF)[0] for a in range(n)]


def test_plan_window_of_length_one(plan_model):
    """len 1: int(spos + 1 * x / 2^32) is spos for every draw, so attempt t is fragment t at spos."""
    m = plan_model
    win = (100, 0, 37, 1, 9, 0, 0)                       # 9 reads: 5 pairs
    made, attempts = m.plan_window(win, 4, 2000)
    assert attempts == 5 and made == [(t, 37, m.isz, 0) for t in range(5)]
    made, _ = m.plan_window((100, 0, 37, 1, 9, 0, 0), 4, 100 + 37 + L)      # the chain ends L bases on: flen == L
    assert made == [(t, 37, L, 0) for t in range(5)]
    slots = m.plan([win, (0, 0, 5, 1, 2, 1, 5)], [2000])
    assert [(s.window, s.foff, s.fragcount, s.seg) for s in slots] == [(0, 137, k + 1, 0) for k in range(5)] + [(1, 5, 1, 1)]


def test_plan_window_whose_every_start_is_clipped_below_a_read(plan_model):
    """Every start leaves L - 1 bases or fewer: 1,000 failures are tolerated, the 1,001st ends the window, no slot lives."""
    m = plan_model
    clen = 5000
    win = (0, 0, clen - L + 1, L - 1, 6, 0, 0)
    made, attempts = m.plan_window(win, 0, clen)
    assert made == [] and attempts == 1001
    assert m.plan([win], [clen]) == [None, None, None]


def test_plan_window_where_only_late_attempts_succeed(plan_model):
    """A window of L starts whose first start alone leaves a whole read: attempt a succeeds iff its word 0 is below
    2^32 / L (restated here from the words, not from the model's arithmetic).  Five pairs are all made, late; of forty
    the window makes those the first 1,000 failures allow and leaves the rest dead."""
    m = plan_model
    clen, widx = 5000, 11
    x = words0(m, widx, 1100)
    ok = [a for a in range(1100) if x[a] * L < (1 << 32)]
    assert ok[0] > 0 and len(ok) < 40, ok[:3]
    made, attempts = m.plan_window((0, 0, clen - L, L, 10, 0, 0), widx, clen)
    assert [t[0] for t in made] == ok[:5] and attempts == ok[4] + 1 and all(t[1:] == (clen - L, L, 0) for t in made)
    # the 1,001st failure is attempt number 1,000 + (successes before it)
    fails, live = 0, 0
    for a in range(1100):
        if a in ok:
            live += 1
        else:
            fails += 1
            if fails > 1000:
                break
    slots = m.plan([(0, 0, clen - L, L, 80, 0, 0)], [clen], first_window=widx)
    assert 0 < live < 40 and [s is not None for s in slots] == [True] * live + [False] * (40 - live)
    assert [s.attempt for s in slots[:live]] == ok[:live] and [s.fragcount for s in slots[:live]] == list(range(1, live + 1))
