"""The counting rule of `simuReads --truth-variants` (DESIGN.md "True allele counts"), written from its label
definition: a template is expanded into one label per base and every clause of the rule is tested by brute force.  It
shares no code with the engine's piece-level scan.

Pieces are (dst, src, len, contig, kind, seg_first) rows in chain order (kind 1: literal); table rows are
(contig, kind, pos, len, allele) with kind 0 SNV (allele a letter or its ASCII code), 1 insertion, 2 deletion, pos
0-based; codes are the template's chain base codes (A0 C1 T2 G3, N 4)."""
import random

CODE = {"A": 0, "C": 1, "T": 2, "G": 3, "N": 4, "X": 6}
SNV, INS, DEL = 0, 1, 2


def base_code(allele):
    if not isinstance(allele, str):
        allele = chr(allele)
    return CODE.get(allele.upper(), 5)


def labels(pieces, tmpl_off, L):
    """One label per template base: ('R', contig, x) or ('L', piece index, offset in the piece)."""
    out = []
    for o in range(tmpl_off, tmpl_off + L):
        for k, (dst, src, ln, contig, kind, _seg_first) in enumerate(pieces):
            if dst <= o < dst + ln:
                out.append(("L", k, o - dst) if kind else ("R", contig, src + (o - dst)))
                break
        else:
            raise ValueError("the template leaves the pieces")
    return out


def observe(pieces, codes, tmpl_off, L, rows):
    """{row index: [alt, total]} for one template (rows without a count are absent)."""
    lab = labels(pieces, tmpl_off, L)
    t_end = tmpl_off + L
    out = {}

    def hit(r, alt):
        c = out.setdefault(r, [0, 0])
        c[1] += 1
        if alt:
            c[0] += 1

    for r, (contig, kind, p, k, allele) in enumerate(rows):
        if kind == SNV:
            for i in range(L):
                if lab[i] == ("R", contig, p):
                    hit(r, codes[i] == base_code(allele))
        elif kind == DEL:
            if p < 1:
                continue
            for i in range(L - 1):
                if lab[i] == ("R", contig, p - 1):
                    if lab[i + 1] == ("R", contig, p):
                        hit(r, False)
                    if lab[i + 1] == ("R", contig, p + k):
                        hit(r, True)
        else:
            for i in range(L - 1):
                if lab[i] != ("R", contig, p):
                    continue
                nxt = lab[i + 1]
                if nxt == ("R", contig, p + 1):
                    hit(r, False)
                elif nxt[0] == "L" and nxt[2] == 0:
                    dst, _src, ln = pieces[nxt[1]][:3]
                    # of exactly k bases, wholly inside the template, one more template base behind it
                    if ln == k and dst >= tmpl_off and dst + ln <= t_end and dst + ln < t_end:
                        hit(r, True)
    return out


def sort_rows(rows):
    """The table's order: contig, pos, kind, then allele code point or length; no two alike."""
    def key(r):
        contig, kind, p, k, allele = r
        a = (ord(allele) if isinstance(allele, str) else allele) if kind == SNV else 0
        return (contig, p, kind, a, k)
    seen, out = set(), []
    for r in sorted(rows, key=key):
        if key(r) not in seen:
            seen.add(key(r))
            out.append(r)
    return out


def random_case(rng, L=None):
    """A seeded chain of pieces (the generator idea of truth_model.random_case: straight joints, gaps, steps back, contig
    changes, literals, short and long pieces), a template inside it, its codes, and a table whose rows crowd the
    positions the template touches: on piece ends, one off them, with the joint's gap length and with another."""
    L = L or rng.choice((8, 20, 36, 75, 100))
    pieces, dst = [], 0
    contig, pos = 0, rng.randrange(0, 300)
    for i in range(rng.randrange(1, 9)):
        ln = rng.randrange(1, 2 * L if rng.random() < 0.5 else 6)
        seg_first = 1 if rng.random() < 0.2 else 0
        if rng.random() < 0.25 and i:
            pieces.append((dst, rng.randrange(0, 1000), ln, 0, 1, seg_first))
        else:
            r2 = rng.random()
            if r2 < 0.45:
                pass
            elif r2 < 0.75:
                pos += rng.randrange(1, 6)
            elif r2 < 0.92:
                pos = max(0, pos - rng.randrange(1, 3 * L))
            else:
                contig = (contig + 1) % 3
            pieces.append((dst, pos, ln, contig, 0, seg_first))
            pos += ln
        dst += ln
    while dst < L + 2:
        pieces.append((dst, pos, L, contig, 0, 0))
        pos += L
        dst += L
    tmpl_off = rng.randrange(0, dst - L + 1)
    codes = [rng.choice((0, 1, 2, 3, 3, 4)) for _ in range(L)]
    # positions of interest: the ends of every reference piece and of the template's reference bases
    spots = set()
    for d, s, ln, c, kind, _ in pieces:
        if not kind:
            for x in (s - 1, s, s + 1, s + ln - 2, s + ln - 1, s + ln):
                if x >= 0:
                    spots.add((c, x))
    for lb in labels(pieces, tmpl_off, L)[:2] + labels(pieces, tmpl_off, L)[-2:]:
        if lb[0] == "R":
            spots.add((lb[1], lb[2]))
            spots.add((lb[1], lb[2] + 1))
    spots = sorted(spots)
    lit_lens = [p[2] for p in pieces if p[4]] or [1]
    rows = []
    for _ in range(rng.randrange(1, 14)):
        c, x = rng.choice(spots) if rng.random() < 0.8 else (rng.randrange(0, 3), rng.randrange(0, 400))
        kind = rng.randrange(0, 3)
        if kind == SNV:
            rows.append((c, SNV, x, 0, rng.choice("ACGTN")))
        elif kind == INS:
            rows.append((c, INS, x, rng.choice(lit_lens) if rng.random() < 0.7 else rng.randrange(1, 6), 0))
        else:
            rows.append((c, DEL, x, rng.randrange(1, 7), 0))
    return pieces, codes, tmpl_off, L, sort_rows(rows)


if __name__ == "__main__":
    rng = random.Random(1)
    print(random_case(rng))
