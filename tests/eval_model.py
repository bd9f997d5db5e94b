"""A plain-Python model of truthEval (the issue's rule, written from its text): dicts keyed by (name, mate), the first
primary record of the test file in file order claims a truth read, every later one is `repeated`.  No hashing, no sorting,
no GPU: the yardstick of tests/test_truth_eval_cpu.py and tests/test_gpu_truth_eval.py."""
import struct

CATEGORIES = ["exact", "near", "wrong_place", "wrong_strand", "wrong_contig", "lost", "invented", "both_unmapped"]
CLASSES = ["plain", "edited", "unmapped"]
REF_OPS = (0, 2, 3, 7, 8)   # M D N = X


class Aln:
    """One record as the rule sees it."""
    __slots__ = ("name", "mate", "flag", "ref", "pos", "mapq", "ops")

    def __init__(self, name, flag, ref, pos, mapq, ops):
        self.name, self.flag, self.ref, self.pos, self.mapq, self.ops = name, flag, ref, pos, mapq, ops
        self.mate = 1 if flag & 0x80 else 0

    @property
    def unmapped(self):
        return bool(self.flag & 4)

    @property
    def reverse(self):
        return bool(self.flag & 0x10)

    @property
    def span(self):
        if not self.ops:
            return 1
        return sum(n for n, op in self.ops if op in REF_OPS)

    @property
    def cls(self):
        if self.unmapped:
            return "unmapped"
        return "plain" if len(self.ops) == 1 and self.ops[0][1] == 0 else "edited"


def records(stream):
    """(reference names, [Aln]) of an inflated BAM stream; the CIGAR is the record's own (a kSmN placeholder stays)."""
    assert stream[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", stream, 4)[0]
    q = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, q)[0]
    q += 4
    names = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", stream, q)[0]
        names.append(stream[q + 4:q + 4 + ln].split(b"\0")[0])
        q += 8 + ln
    out = []
    while q + 4 <= len(stream):
        bs = struct.unpack_from("<I", stream, q)[0]
        ref, pos, lname, mapq, _bin, ncig, flag = struct.unpack_from("<iiBBHHH", stream, q + 4)
        name = stream[q + 36:q + 36 + lname].split(b"\0")[0]
        ops = [struct.unpack_from("<I", stream, q + 36 + lname + 4 * i)[0] for i in range(ncig)]
        out.append(Aln(name, flag, ref, pos, mapq, [(o >> 4, o & 15) for o in ops]))
        q += 4 + bs
    return names, out


def classify(t, q, q_ref, pct):
    """The category of test record q (its contig in the truth's numbering: q_ref, None for none) against truth record t."""
    if q.unmapped and t.unmapped:
        return "both_unmapped"
    if q.unmapped:
        return "lost"
    if t.unmapped:
        return "invented"
    if q_ref is None or q_ref != t.ref:
        return "wrong_contig"
    if q.reverse != t.reverse:
        return "wrong_strand"
    t0, t1, q0, q1 = t.pos, t.pos + t.span, q.pos, q.pos + q.span
    if (t0, t1) == (q0, q1):
        return "exact"
    overlap = max(0, min(t1, q1) - max(t0, q0))
    if overlap >= 1 and overlap * 100 >= pct * min(t.span, q.span):
        return "near"
    return "wrong_place"


def evaluate(truth_names, truth, test_names, test, pct=10):
    """-> dict(table={(mate, class, mapq): [8 counts]}, missing={(mate, class): n}, and the scalar counts)."""
    by_read = {}
    for t in truth:
        by_read.setdefault((t.name, t.mate), []).append(t)
    truth_id = {}
    for i, n in enumerate(truth_names):
        truth_id.setdefault(n, i)
    res = dict(table={}, missing={(m, c): 0 for m in (0, 1) for c in CLASSES}, test_records=len(test), secondary=0, supplementary=0, unknown=0,
               ambiguous=0, repeated=0, truth_records=len(truth), truth_duplicates=sum(len(v) for v in by_read.values() if len(v) > 1))
    claimed = set()
    for q in test:
        if q.flag & 0x100:
            res["secondary"] += 1
            continue
        if q.flag & 0x800:
            res["supplementary"] += 1
            continue
        key = (q.name, q.mate)
        if key not in by_read:
            res["unknown"] += 1
        elif len(by_read[key]) > 1:
            res["ambiguous"] += 1
        elif key in claimed:
            res["repeated"] += 1
        else:
            claimed.add(key)
            t = by_read[key][0]
            q_ref = truth_id.get(test_names[q.ref]) if q.ref >= 0 else None
            cat = classify(t, q, q_ref, pct)
            res["table"].setdefault((t.mate, t.cls, q.mapq), [0] * 8)[CATEGORIES.index(cat)] += 1
    for key, v in by_read.items():
        if len(v) == 1 and key not in claimed:
            res["missing"][(v[0].mate, v[0].cls)] += 1
    return res


def tsv(res, pct=10):
    """eval.tsv of a result, byte for byte."""
    out = ["#T\tmin_overlap\t%d" % pct]
    for k in ("truth_records", "truth_duplicates", "test_records", "secondary", "supplementary", "unknown", "ambiguous", "repeated"):
        out.append("#T\t%s\t%d" % (k, res[k]))
    mapped, correct = {}, {}
    for mate in (0, 1):
        for cls in CLASSES:
            for mapq in range(256):
                row = res["table"].get((mate, cls, mapq))
                if not row or not any(row):
                    continue
                out.append("#M\t%d\t%s\t%d\t%s" % (mate, cls, mapq, "\t".join(str(v) for v in row)))
                mapped[mapq] = mapped.get(mapq, 0) + sum(row) - row[5] - row[7]
                correct[mapq] = correct.get(mapq, 0) + row[0] + row[1]
    for mate in (0, 1):
        for cls in CLASSES:
            out.append("#X\t%d\t%s\t%d" % (mate, cls, res["missing"][(mate, cls)]))
    cm = cc = 0
    for mapq in range(255, -1, -1):
        if mapped.get(mapq, 0) > 0:
            cm += mapped[mapq]
            cc += correct[mapq]
            out.append("#R\t%d\t%d\t%d\t%d\t%d" % (mapq, mapped[mapq], correct[mapq], cm, cc))
    return ("\n".join(out) + "\n").encode()
