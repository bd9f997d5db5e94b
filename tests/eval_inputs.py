"""Inputs for the second round of truthEval's tests (test_truth_eval_inputs_cpu.py says what each is for and proves it on the
model; test_gpu_truth_eval_scale.py feeds them to the device): records by the hundred thousand, every cell of the table, names
of every odd shape, runs of duplicated reads across the sort's 256-key blocks, records of 30 KB that fill several batches of
the command line, headers of several members.  Records are packed with struct (SAMv1 section 4.2), not through SAM text; a
read is a tuple (name field, flag, refID, 0-based pos, mapq, operations) until it is packed."""
import random
import struct

import bam_util as B
import eval_model as M

REFS = [(b"chrA", 500000), (b"chrB", 300000), (b"chrC", 100000)]
TEST_REFS = REFS + [(b"chrZ", 700000)]                 # the test files' list: the truth's and a contig it lacks
PLAIN, EDITED = [(50, 0)], [(20, 0), (2, 2), (30, 0)]
MAPPED_CATS, UNMAPPED_CATS = M.CATEGORIES[:6], M.CATEGORIES[6:]
TEXT = b"@HD\tVN:1.6\n"


def rec(name, flag, ref, pos, mapq, ops=(), l_seq=0, seq=b"", qual=b"", aux=b"", field=None):
    """One record; `field` is the whole name field (with its NUL) where the name alone does not say it."""
    nm = field if field is not None else name + b"\0"
    body = (struct.pack("<iiBBHHHIiii", ref, pos, len(nm), mapq, 4680, len(ops), flag, l_seq, -1, -1, 0) + nm +
            b"".join(struct.pack("<I", n << 4 | o) for n, o in ops) + seq + qual + aux)
    return struct.pack("<I", len(body)) + body


def pack(reads):
    return [rec(*r) for r in reads]


def stream(refs, recs, text=TEXT):
    return B.header(refs, text) + b"".join(recs)


def model_of(truth_stream, test_stream, pct=10):
    tn, t = M.records(truth_stream)
    qn, q = M.records(test_stream)
    return M.evaluate(tn, t, qn, q, pct)


def truth_read(name, mate, cls, k):
    """A truth read of that class; k varies strand, contig and place."""
    flag = 1 | (0x80 if mate else 0x40) | (0x10 if k & 1 else 0)
    if cls == "unmapped":
        return (name, flag | 4, -1, -1, 0, ())
    return (name, flag, k % 3, 100 + (k * 37) % 90000, 60, tuple(PLAIN if cls == "plain" else EDITED))


def answer(t, cat, mapq, k=0):
    """The test record that scores truth read t in category `cat`."""
    name, flag, ref, pos, _, ops = t
    if cat == "exact":
        return (name, flag, ref, pos, mapq, ops)
    if cat == "near":
        return (name, flag, ref, pos + 1 + k % 3, mapq, ops)
    if cat == "wrong_place":
        return (name, flag, ref, pos + 52 + k % 1000, mapq, tuple(PLAIN))   # the truth's interval is 50 or 52 bases
    if cat == "wrong_strand":
        return (name, flag ^ 0x10, ref, pos, mapq, ops)
    if cat == "wrong_contig":
        return (name, flag, 3 if k & 1 else (ref + 1) % 3, pos, mapq, ops)  # chrZ, or another of the truth's
    if cat in ("lost", "both_unmapped"):
        return (name, flag | 4, -1, -1, mapq, ())
    assert cat == "invented"
    return (name, flag & ~4, k % 4, 200 + k % 5000, mapq, tuple(PLAIN))


# ---- 1. scale ----
def minimal_records(n, seed=5):
    """-> (truth reads, test reads): n truth reads of about 50 bytes (l_seq 0, at most three operations, names `m<hex>`), and
    what an aligner might have made of them: every category at every MAPQ, some reads dropped, some primaries repeated,
    secondary / supplementary / unknown records, shuffled."""
    rng = random.Random(seed)
    truth = [truth_read(b"m%x" % i, i & 1, ("unmapped", "edited", "edited", "plain", "plain", "plain", "plain")[i % 7], i) for i in range(n)]
    test = []
    for i, t in enumerate(truth):
        u = rng.random()
        if u < 0.02:
            continue
        cats = UNMAPPED_CATS if t[1] & 4 else MAPPED_CATS
        q = answer(t, cats[rng.randrange(len(cats))], rng.randrange(256), i)
        test.append(q)
        if u > 0.98:
            test.append(answer(t, "exact" if not t[1] & 4 else "both_unmapped", 7, i))      # a second primary: the shuffle says which is first
        elif u > 0.97:
            test.append((q[0], q[1] | 0x100, 0, 5, 0, tuple(PLAIN)))
        elif u > 0.96:
            test.append((q[0], q[1] | 0x800, 1, 6, 3, tuple(PLAIN)))
        elif u > 0.95:
            test.append((b"x%x" % i, 0x41, 0, 7, 60, tuple(PLAIN)))
    rng.shuffle(test)
    return truth, test


# ---- 2. every cell ----
def sweep_count(mate, ci, cat, mapq):
    return 1 + ((mate * 3 + ci) * 5 + cat * 3 + mapq) % 4


SWEEP_MISSING = {(mate, cls): 3 + mate * 3 + ci for mate in (0, 1) for ci, cls in enumerate(M.CLASSES)}


def reachable_cells():
    return [(mate, ci, mapq, cat) for mate in (0, 1) for ci in range(3) for mapq in range(256)
            for cat in (range(6) if ci < 2 else (6, 7))]


def cell_sweep(seed=11):
    """-> (truth stream, test stream): cell (mate, class, MAPQ, category) is hit sweep_count() times, each by a read of its
    own; SWEEP_MISSING reads per (mate, class) have no test record; and one of each scalar count's kind at least."""
    rng = random.Random(seed)
    truth, test, k = [], [], 0
    for mate, ci, mapq, cat in reachable_cells():
        for _ in range(sweep_count(mate, ci, cat, mapq)):
            t = truth_read(b"s%d" % k, mate, M.CLASSES[ci], k)
            truth.append(t)
            test.append(answer(t, M.CATEGORIES[cat], mapq, k))
            k += 1
    for (mate, cls), n in SWEEP_MISSING.items():
        for _ in range(n):
            truth.append(truth_read(b"gone%d" % k, mate, cls, k))
            k += 1
    twice = truth_read(b"twice", 0, "plain", 4)
    truth += [twice, twice]
    test += [answer(twice, "exact", 60)] * 3                                     # ambiguous
    for i in range(4):
        test.append((b"s%d" % i, truth[i][1] | 0x100, 0, 10, 0, tuple(PLAIN)))   # secondary
    for i in range(5):
        test.append((b"s%d" % i, truth[i][1] | 0x800, 0, 10, 9, tuple(PLAIN)))   # supplementary
    for i in range(6):
        test.append((b"nobody%d" % i, 0x41, 0, 10, 60, tuple(PLAIN)))            # unknown
    for i in range(50, 57):
        test.append(answer(truth[i], "exact" if not truth[i][1] & 4 else "both_unmapped", 200, i))   # a primary again: repeated,
    n_first = len(test) - 7                                                      # ... as long as it stays behind the first one
    rng.shuffle(truth)
    head = test[:n_first]
    rng.shuffle(head)
    return stream(REFS, pack(truth)), stream(TEST_REFS, pack(head + test[n_first:]))


# ---- 3. names ----
def cg_record(name, flag, ref, pos, mapq, real_ops, l_seq=50):
    """kSmN in the record, the real operations in CG:B:I (l_seq bases of A with quality 30)."""
    m = sum(n for n, o in real_ops if o in M.REF_OPS)
    aux = B.aux_tag(b"CG", "BI", [n << 4 | o for n, o in real_ops])
    return rec(name, flag, ref, pos, mapq, [(l_seq, 4), (m, 3)], l_seq, b"\x11" * ((l_seq + 1) // 2), b"\x1e" * l_seq, aux)


N254 = dict(first_a=b"A" + b"q" * 253, first_b=b"B" + b"q" * 253, last_1=b"r" * 253 + b"1", last_2=b"r" * 253 + b"2", dup=b"d" * 254)


def name_shapes(seed=23):
    """-> dict(truth=stream, test=stream, shapes={label: name}): the names of the issue's list, every truth read answered by a
    test record (category and MAPQ by turns), in at least 40 KB of records a side of which most bytes are names that
    bam_guess's plausible() turns away."""
    rng = random.Random(seed)
    shapes = dict(N254, one=b"a", two=b"bc", prefix=b"prefix", longer=b"prefixed", pair=b"pair", nomate=b"nomate", b01=b"\x01", b7f=b"\x7f",
                  b80=b"\x80", bff=b"\xff", mixed=b"n\x01\x7f\x80\xffz", nul_truth=b"ab", nul_test=b"ef", empty=b"", nocigar=b"nocigar",
                  span0=b"span0", cg=b"placeholder")
    truth, answered, k = [], [], 0

    def add(name, mate=0, cls="plain", flag=None, field=None, aux=b"", ops=None):
        nonlocal k
        t = truth_read(name, mate, cls, k)
        if flag is not None:
            t = (t[0], flag, t[2], t[3], t[4], t[5])
        if ops is not None:
            t = t[:5] + (tuple(ops),)
        truth.append((t, field, aux))
        answered.append((t, field, aux))
        k += 1
        return t
    for key in ("one", "two", "first_a", "first_b", "last_1", "last_2", "prefix", "longer", "b01", "b7f", "b80", "bff", "mixed"):
        same_mate = key in ("first_a", "first_b", "last_1", "last_2", "prefix", "longer")   # (these differ in their names alone)
        add(shapes[key], mate=0 if same_mate else k & 1, cls=("plain", "edited", "unmapped")[k % 3], aux=B.aligner_tags(rng, 50) if k % 2 else b"")
    add(shapes["pair"], mate=0)
    add(shapes["pair"], mate=1, cls="edited")
    add(shapes["nomate"], flag=0)                                    # no 0x40, no 0x80: mate 0
    add(shapes["nul_truth"], field=b"ab\0cd\0")                      # l_read_name 6; the read is `ab`
    add(shapes["nul_test"])
    add(shapes["empty"], mate=1)                                     # l_read_name 1
    add(shapes["dup"])
    truth.append(truth[-1])
    add(shapes["nocigar"], ops=())                                   # mapped, no operations: span 1
    add(shapes["span0"], ops=[(10, 4), (40, 1)])                     # only S and I: span 0
    fill = []
    for i in range(230):                                             # 254 bytes none of which is printable
        nm = bytes(rng.choice((1, 2, 0x1f, 0x20, 0x7f, 0x80, 0x9c, 0xfe, 0xff)) for _ in range(250)) + b"%04d" % i
        nm = nm[:246] + bytes([0x80 + i % 100]) * 4 + nm[250:]
        fill.append(add(nm, mate=i & 1, cls=("plain", "edited", "unmapped")[i % 3], aux=B.aligner_tags(rng, 50) if i % 5 == 0 else b""))
    t_recs = [rec(*t, aux=aux, field=field) for t, field, aux in truth]
    cg_t = truth_read(shapes["cg"], 1, "edited", 77)
    t_recs.insert(9, cg_record(cg_t[0], cg_t[1], cg_t[2], cg_t[3], 60, EDITED))
    # the test file: each read once (the duplicated one too: ambiguous), by the other spelling where there is one
    test = []
    for j, (t, field, aux) in enumerate(answered):
        cats = UNMAPPED_CATS if t[1] & 4 else MAPPED_CATS
        q = answer(t, cats[j % len(cats)], (j * 41) % 256, j)
        q_field = b"ef\0gh\0" if t[0] == b"ef" else None             # (the truth's `ab\0cd` is looked up as `ab`)
        if t[0] == shapes["nomate"]:
            q = (q[0], q[1] | 0x41) + q[2:]                          # mate 0 by 0x40
            test.append(rec(q[0], q[1] ^ 0xC0, 0, 1, 3))             # the same name as mate 1: unknown
        test.append(rec(*q, aux=B.aligner_tags(rng, 50) if j % 3 == 0 else b"", field=q_field))
    test.append(cg_record(cg_t[0], cg_t[1], cg_t[2], cg_t[3] + 2, 33, [(52, 0)]))   # placeholder against placeholder: both span 52, near
    test.append(rec(shapes["prefix"][:-1], 0x41, 0, 5, 60, PLAIN))                # a prefix of a truth name that no read has: unknown
    test.append(rec(N254["last_1"][:253], 0x41, 0, 5, 60, PLAIN))                 # 253 bytes of a 254-byte name: unknown
    order = list(range(len(test)))
    rng.shuffle(order)
    return dict(truth=stream(REFS, t_recs), test=stream(TEST_REFS, [test[i] for i in order]), shapes=shapes)


# ---- 4. duplicated reads ----
def sorted_positions(reads, key_bits):
    """Where each truth row stands after a stable sort by sg_eval_key: positions[row]."""
    import simuscop_amd
    lib = simuscop_amd.load_engine()
    keys = [lib.sg_eval_key(r[0], len(r[0]), 1 if r[1] & 0x80 else 0, key_bits) for r in reads]
    order = sorted(range(len(reads)), key=lambda i: keys[i])
    pos = [0] * len(reads)
    for p, i in enumerate(order):
        pos[i] = p
    return pos, keys


def dup_runs(key_bits, seed=37):
    """-> dict(truth=stream, test=stream, reads=truth reads in file order, big=name of the read held 65 times, counts=the
    closed-form values): 700 reads held once, 6 twice, 3 three times, one 65 times whose copies (one run of equal keys, with
    whatever else has that key) lie on both sides of a multiple of 256 in sorted order: its name is searched for that."""
    for attempt in range(400):
        rng = random.Random(seed)
        once = [truth_read(b"u%d" % i, i & 1, ("plain", "edited", "unmapped")[i % 3], i) for i in range(700)]
        two = [truth_read(b"two%d" % i, i & 1, "plain", i) for i in range(6)]
        three = [truth_read(b"three%d" % i, i & 1, "edited", i) for i in range(3)]
        big = truth_read(b"big%d" % attempt, 1, "plain", 9)
        reads = once + two * 2 + three * 3 + [big] * 65
        rng.shuffle(reads)
        pos, _ = sorted_positions(reads, key_bits)
        at = [pos[i] for i, r in enumerate(reads) if r is big]
        if min(at) // 256 != max(at) // 256:
            break
    else:
        raise AssertionError("no name found whose run straddles a block")
    test = [answer(t, UNMAPPED_CATS[i % 2] if t[1] & 4 else MAPPED_CATS[i % 6], (i * 7) % 256, i) for i, t in enumerate(once[:690])]
    test += [answer(t, "exact", 60) for t in two + three + [big, big]]
    rng.shuffle(test)
    counts = dict(truth_records=700 + 12 + 9 + 65, truth_duplicates=12 + 9 + 65, ambiguous=6 + 3 + 2, missing=10, scored=690, test_records=701,
                  unknown=0, repeated=0, secondary=0, supplementary=0)
    return dict(truth=stream(REFS, pack(reads)), test=stream(TEST_REFS, pack(test)), reads=reads, big=big[0], counts=counts)


def identical_truth(n=300):
    """-> (truth stream, test stream): n copies of one record; five test records find it."""
    t = truth_read(b"same", 0, "plain", 3)
    return stream(REFS, pack([t] * n)), stream(TEST_REFS, pack([answer(t, c, 60) for c in ("exact", "near", "lost", "exact", "wrong_contig")]))


# ---- 5. long records ----
def long_records(n, l_seq, seed=41):
    """-> dict(truth=stream, test=stream, twice=name): n reads of l_seq bases with qualities (random bytes); the test file
    answers each read in the truth's order, and read `twice` a second time five records before its end."""
    rng = random.Random(seed)
    truth = [truth_read(b"long%d" % i, i & 1, ("plain", "edited", "plain", "unmapped")[i % 4], i) for i in range(n)]
    test = [answer(t, UNMAPPED_CATS[i % 2] if t[1] & 4 else MAPPED_CATS[i % 6], (i * 13) % 256, i) for i, t in enumerate(truth)]
    test.insert(n - 5, answer(truth[4], "wrong_place", 17, 1))

    def big(r):
        body = rng.randbytes((l_seq + 1) // 2 + l_seq)
        return rec(*r, l_seq=l_seq, seq=body[:(l_seq + 1) // 2], qual=body[(l_seq + 1) // 2:])
    return dict(truth=stream(REFS, [big(r) for r in truth]), test=stream(TEST_REFS, [big(r) for r in test]), twice=truth[4][0])


def batches(file_bytes, cap):
    """The batches a reader of `cap` bytes a buffer cuts a BGZF file into (each ends behind its last whole member):
    [(file offset, compressed bytes, inflated offset, inflated bytes)]."""
    mem, whole = B.members(file_bytes)
    assert whole == len(file_bytes)
    out, i, inflated = [], 0, 0
    while i < len(mem):
        start, j, n = mem[i][0], i, 0
        while j < len(mem) and mem[j][0] + mem[j][1] + 1 <= start + cap:
            n += mem[j][2]
            j += 1
        out.append((start, mem[j - 1][0] + mem[j - 1][1] + 1 - start, inflated, n))
        inflated += n
        i = j
    return out


# ---- 6. a header of several members ----
def big_header(data, nbytes=3 * 65280):
    """The stream with @CO lines added to its text until the header (all in front of the first record) has `nbytes` bytes."""
    l_text = struct.unpack_from("<i", data, 4)[0]
    names, recs = B.parse_stream(data)
    end = recs[0][0] if recs else len(data)
    co = b""
    while end + len(co) < nbytes:
        co += b"@CO\t%s\n" % (b"x" * 200)
    return b"BAM\1" + struct.pack("<i", l_text + len(co)) + data[8:8 + l_text] + co + data[8 + l_text:]
