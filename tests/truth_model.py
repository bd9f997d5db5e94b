"""A Python model of the truth-alignment rule (DESIGN.md "Truth alignments"; include/simuscop_amd.h, sg_truth_align),
written from the rule's text and not from the engine's walk: every template base gets a label first, the events are
laid over the labelled bases in read direction, and the operations come from grouping the resulting column list.

pieces: (dst, src, len, contig, kind, seg_first) of one chain in offset order; events: (j, len, is_del) in read
direction.  align() returns (contig, pos0, [(len, op)]) with op 0 M, 1 I, 2 D, 3 N, 4 S; (-1, -1, []) for an unmapped
read."""
import itertools

M, I, D, N, S = 0, 1, 2, 3, 4
OPS = "MIDNS"


def ev_pack(j, length, is_del):
    return j | (length << 16) | ((1 if is_del else 0) << 31)


def label_template(pieces, tmpl_off, L):
    """Per template base, in chain direction: (class, contig, refpos, gap) -- gap = (op, len) of the joint in front of the
    base, or None.  After a joint that cannot be aligned every base is S."""
    out = []
    last_ref = None          # (contig, next position) behind the last reference piece the template went through
    seg_began = False
    broken = False
    prev_piece = None
    for c in range(L):
        at = tmpl_off + c
        k = next(i for i, p in enumerate(pieces) if p[0] <= at < p[0] + p[2])
        dst, src, ln, contig, kind, seg_first = pieces[k]
        gap = None
        if k != prev_piece:
            if prev_piece is not None:
                # every piece between the two (none, when they tile the chain and have bases) was stepped over
                for q in range(prev_piece + 1, k + 1):
                    if pieces[q][5]:
                        seg_began = True
            if kind == 0:
                here = src + (at - dst)
                if last_ref is not None and not broken:
                    if contig != last_ref[0] or here < last_ref[1]:
                        broken = True
                    elif here > last_ref[1]:
                        gap = (N if seg_began else D, here - last_ref[1])
                last_ref = (contig, src + ln)
                seg_began = False
            prev_piece = k
        if broken:
            out.append((S, None, None, None))
        elif kind == 1:
            out.append((I, None, None, gap))
        else:
            out.append((M, contig, src + (at - dst), gap))
    return out


def align(pieces, tmpl_off, L, reverse, events=()):
    labels = label_template(pieces, tmpl_off, L)
    # the read sees the template from its own end
    deleted = [False] * L
    ins_after = [0] * L     # read-direction index -> inserted bases behind that base
    for j, k, is_del in events:
        if is_del:
            for x in range(j, j + k):
                deleted[x] = True
        else:
            ins_after[j] += k
    cols = []               # (op, contig, refpos) per column, chain direction
    for c in range(L):
        j = L - 1 - c if reverse else c
        cls, contig, refpos, gap = labels[c]
        if gap is not None:
            cols += [(gap[0], None, None)] * gap[1]
        ins = [(S if cls == S else I, None, None)] * ins_after[j]
        if reverse:
            cols += ins     # behind base j for the read = in front of it on the chain
        if deleted[j]:
            if cls == M:
                cols.append((D, contig, refpos))
        else:
            cols.append((cls, contig, refpos))
        if not reverse:
            cols += ins
    m_at = [i for i, col in enumerate(cols) if col[0] == M]
    if not m_at:
        return -1, -1, []
    first, last = m_at[0], m_at[-1]
    lead = sum(1 for col in cols[:first] if col[0] in (I, S))
    tail = sum(1 for col in cols[last + 1:] if col[0] in (I, S))
    ops = [(lead, S)] if lead else []
    ops += [(len(list(g)), op) for op, g in itertools.groupby(col[0] for col in cols[first:last + 1])]
    if tail:
        ops.append((tail, S))
    return cols[first][1], cols[first][2], ops


def cigar_text(ops):
    return "".join("%d%s" % (n, OPS[o]) for n, o in ops) or "*"


def query_length(ops):
    return sum(n for n, o in ops if o in (M, I, S))


def reference_span(ops):
    return sum(n for n, o in ops if o in (M, D, N))


def random_case(rng, L=None):
    """A seeded chain of pieces, a template inside it and a legal event list."""
    L = L or rng.choice((30, 36, 50, 76, 100, 151))
    pieces, dst = [], 0
    contig, pos = 0, rng.randrange(0, 5000)
    n_pieces = rng.randrange(1, 9)
    for i in range(n_pieces):
        ln = rng.randrange(1, 2 * L if rng.random() < 0.6 else 12)
        r = rng.random()
        seg_first = 1 if rng.random() < 0.2 else 0
        if r < 0.2 and i:
            pieces.append((dst, rng.randrange(0, 1000), ln, 0, 1, seg_first))            # literal
        else:
            r2 = rng.random()
            if r2 < 0.55:
                pass                                                                       # goes straight on
            elif r2 < 0.8:
                pos += rng.randrange(1, 40)                                                # forward gap
            elif r2 < 0.92:
                pos = max(0, pos - rng.randrange(1, 3 * L))                                # back
            else:
                contig = (contig + 1) % 3
            pieces.append((dst, pos, ln, contig, 0, seg_first))
            pos += ln
        dst += ln
    while dst < L + 2:                                                                     # room for one template
        pieces.append((dst, pos, L, contig, 0, 0))
        pos += L
        dst += L
    tmpl_off = rng.randrange(0, dst - L + 1)
    events, j = [], 0
    n_ev = rng.choice((0, 0, 1, 1, 2, 3, 8, 32))
    while len(events) < n_ev and j < L:
        j += rng.randrange(0, max(1, L // max(n_ev, 1)))
        if j >= L:
            break
        if rng.random() < 0.5:
            k = rng.randrange(1, 6)
            events.append((j, k, False))
            j += 1
        else:
            k = min(L - j, rng.randrange(1, 6))
            events.append((j, k, True))
            j += k
    return pieces, tmpl_off, L, rng.random() < 0.5, events
