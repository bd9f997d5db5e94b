"""Helpers of the --truth-errors GPU tests: the model (tests/errors_model.py) applied to every read of a Session's pass."""
import numpy as np

import errors_model as EM


def model_of_pass(sess, table, paired):
    """Adds every read of the pass just sampled (after result()) to `table`; returns (reads counted, reads skipped).
    Templates and events come from sg_truth_reads, codes from sg_haplotype_codes, text from sg_fetch."""
    b1, b2, _ = sess.result()
    texts = sess.fetch(b1, b2)
    n = sess.batch_slots
    counted = skipped = 0
    for m in range(2 if paired else 1):
        rows = texts[m].split(b"\n")
        assert rows[-1] == b"" and (len(rows) - 1) % 4 == 0
        geo = sess.truth_reads(m, 0, n)
        k = 0
        for t in range(n):
            r = geo[t]
            if not r.live:
                continue
            seq, qual = rows[4 * k + 1], rows[4 * k + 3]
            k += 1
            assert len(seq) == len(qual) == r.read_len, (m, t, len(seq), r.read_len)
            if not r.inside:
                skipped += 1
                continue
            codes = sess.haplotype_codes(r.chain, r.tmpl_off, table.L)
            table.add(codes, bool(r.reverse), [r.events[e] for e in range(r.n_events)], seq, qual, m)
            counted += 1
        assert 4 * k == len(rows) - 1, "records and live rows differ in number"
    table.skipped += skipped
    return counted, skipped


def assert_tables_equal(got_flat, want, where=""):
    got = np.asarray(got_flat).astype(np.int64)
    exp = want.flat()
    bad = np.flatnonzero(got != exp)
    if len(bad):
        g = EM.Table.of_flat(got, want.cycles, want.qual_lo, want.n_qual, want.L)
        parts = {name: int((getattr(g, name) != getattr(want, name)).sum()) for name in "QSID"}
        raise AssertionError((where, len(bad), parts, int(bad[0]), int(got[bad[0]]), int(exp[bad[0]])))
