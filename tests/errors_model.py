"""The rule of the true error counts (simuReads --truth-errors, DESIGN.md "True error counts") from its definition, in
numpy: expand T', mark what the events delete and insert per template base, give every read position its label, count.
No walk over runs and no code shared with the engine: the engine's statement (errtab_walk, sg_truth.h) is what it checks.

The table has the engine's cells (sg_errtab_counts): Q[mate][cycle][quality column][bases, errors, other, inserted],
S[mate][from A C T G][to A C T G N], I / D[mate][j][events, bases]; flat() strings them together in that order."""
import numpy as np

BASES, ERRORS, OTHER, INSERTED = 0, 1, 2, 3
MAX_EVENTS = 32
_READ_CODE = np.full(256, 4, dtype=np.int64)
for _ch, _c in ((b"A", 0), (b"C", 1), (b"T", 2), (b"G", 3)):
    _READ_CODE[_ch[0]] = _c


class Refused(Exception):
    """A read the rule does not count: its events are not a pass's, or do not give its length, or a byte is out of range."""


def ev_pack(j, k, is_del):
    return j | (k << 16) | ((1 if is_del else 0) << 31)


def ev_unpack(w):
    return w & 0xFFFF, (w >> 16) & 0x7FFF, w >> 31


class Table:
    def __init__(self, cycles, qual_lo, n_qual, L):
        self.cycles, self.qual_lo, self.n_qual, self.L = cycles, qual_lo, n_qual, L
        self.Q = np.zeros((2, cycles, n_qual, 4), dtype=np.int64)
        self.S = np.zeros((2, 4, 5), dtype=np.int64)
        self.I = np.zeros((2, L, 2), dtype=np.int64)
        self.D = np.zeros((2, L, 2), dtype=np.int64)
        self.skipped = 0

    @property
    def cells(self):
        return 8 * self.cycles * self.n_qual + 40 + 8 * self.L

    def flat(self):
        return np.concatenate([self.Q.ravel(), self.S.ravel(), self.I.ravel(), self.D.ravel()])

    @classmethod
    def of_flat(cls, flat, cycles, qual_lo, n_qual, L):
        t = cls(cycles, qual_lo, n_qual, L)
        flat = np.asarray(flat).astype(np.int64)
        assert flat.size == t.cells
        a = 8 * cycles * n_qual
        t.Q = flat[:a].reshape(t.Q.shape)
        t.S = flat[a:a + 40].reshape(t.S.shape)
        t.I = flat[a + 40:a + 40 + 4 * L].reshape(t.I.shape)
        t.D = flat[a + 40 + 4 * L:].reshape(t.D.shape)
        return t

    def add(self, codes, reverse, events, bases, quals, mate):
        """Count one read (mate 0 / 1).  `codes`: the template's chain codes in chain direction; `events`: ev_pack words in
        read direction.  Raises Refused, and then has added nothing."""
        L = self.L
        codes = np.asarray(codes, dtype=np.int64)
        assert codes.size == L
        t = codes[::-1].copy() if reverse else codes.copy()         # T' in read direction
        if reverse:
            t[t < 4] ^= 2
        if len(events) > MAX_EVENTS:
            raise Refused("events")
        deleted = np.zeros(L, dtype=bool)
        ins = np.zeros(L, dtype=np.int64)
        ins_rows, del_rows, nxt = [], [], 0
        for w in events:
            j, k, is_del = ev_unpack(int(w))
            if j < nxt or j >= L or k == 0:
                raise Refused("event order")
            if is_del:
                k = min(k, L - j)
                deleted[j:j + k] = True
                del_rows.append((j, k))
                nxt = j + k
            else:
                ins[j] = k
                ins_rows.append((j, k))
                nxt = j + 1
        kept = ~deleted
        shown = kept.astype(np.int64) + ins                          # read bases template base j brings: itself, then its insertion
        first = np.cumsum(shown) - shown                             # read position of the base paired with T'[j]
        n = int(shown.sum())
        if n != len(bases) or len(bases) != len(quals) or n > self.cycles:
            raise Refused("length")
        q = np.frombuffer(bytes(quals), dtype=np.uint8).astype(np.int64) - 33 - self.qual_lo
        if (q < 0).any() or (q >= self.n_qual).any():
            raise Refused("quality")
        letter = _READ_CODE[np.frombuffer(bytes(bases), dtype=np.uint8)]
        jj = np.flatnonzero(kept)
        r = first[jj]
        tc = t[jj]
        acgt = tc < 4
        ra, ta = r[acgt], tc[acgt]
        np.add.at(self.Q, (mate, ra, q[ra], BASES), 1)
        wrong = letter[ra] != ta
        np.add.at(self.Q, (mate, ra[wrong], q[ra[wrong]], ERRORS), 1)
        np.add.at(self.S, (mate, ta, letter[ra]), 1)
        ro = r[~acgt]
        np.add.at(self.Q, (mate, ro, q[ro], OTHER), 1)
        for j, k in ins_rows:
            ri = first[j] + 1 + np.arange(k)
            np.add.at(self.Q, (mate, ri, q[ri], INSERTED), 1)
            self.I[mate, j] += (1, k)
        for j, k in del_rows:
            self.D[mate, j] += (1, k)


def format_table(t, mates):
    """The file from its definition: four blocks behind their header lines; returns (text, data lines)."""
    out, n = ["#Q\tmate\tcycle\tqual\tbases\terrors\tother\tinserted\n"], 0
    for m in range(mates):
        for c in range(t.cycles):
            for q in range(t.n_qual):
                cell = t.Q[m, c, q]
                if cell.any():
                    out.append("Q\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % ((m + 1, c + 1, t.qual_lo + q) + tuple(int(v) for v in cell)))
                    n += 1
    out.append("#S\tmate\tfrom\tto\tcount\n")
    code = {"A": 0, "C": 1, "T": 2, "G": 3, "N": 4}
    for m in range(mates):
        for f in "ACGT":
            for to in "ACGTN":
                out.append("S\t%d\t%s\t%s\t%d\n" % (m + 1, f, to, int(t.S[m, code[f], code[to]])))
                n += 1
    for tag, rows in (("I", t.I), ("D", t.D)):
        out.append("#%s\tmate\tindex\tevents\tbases\n" % tag)
        for m in range(mates):
            for j in range(t.L):
                if rows[m, j, 0]:
                    out.append("%s\t%d\t%d\t%d\t%d\n" % (tag, m + 1, j + 1, int(rows[m, j, 0]), int(rows[m, j, 1])))
                    n += 1
    return "".join(out).encode(), n


def parse_file(text):
    """{'Q': {(mate, cycle, qual): (bases, errors, other, inserted)}, 'S': {(mate, from, to): n}, 'I' / 'D': {(mate, index):
    (events, bases)}} of a --truth-errors file; checks the four header lines and their order."""
    lines = text.decode().split("\n")
    assert lines[-1] == ""
    heads = [l for l in lines if l.startswith("#")]
    assert heads == ["#Q\tmate\tcycle\tqual\tbases\terrors\tother\tinserted", "#S\tmate\tfrom\tto\tcount", "#I\tmate\tindex\tevents\tbases",
                     "#D\tmate\tindex\tevents\tbases"], heads
    out = {"Q": {}, "S": {}, "I": {}, "D": {}}
    block = None
    for l in lines[:-1]:
        if l.startswith("#"):
            block = l[1]
            continue
        f = l.split("\t")
        assert f[0] == block, l
        if block == "Q":
            out["Q"][(int(f[1]), int(f[2]), int(f[3]))] = tuple(int(v) for v in f[4:8])
        elif block == "S":
            out["S"][(int(f[1]), f[2], f[3])] = int(f[4])
        else:
            out[block][(int(f[1]), int(f[2]))] = (int(f[3]), int(f[4]))
    return out


def random_read(rng, L, n_events, qual_lo, n_qual, mismatch=0.05):
    """A template and a read that a pass could have made of it: (codes, reverse, events, bases, quals)."""
    codes = rng.integers(0, 4, L).astype(np.uint8)
    if rng.random() < 0.3:                                           # N / other / X islands
        for _ in range(int(rng.integers(1, 4))):
            a = int(rng.integers(0, L))
            codes[a:a + int(rng.integers(1, 9))] = rng.integers(4, 7)
    reverse = bool(rng.integers(0, 2))
    events, j = [], int(rng.integers(0, max(1, L // max(n_events, 1))))
    while len(events) < n_events and j < L:
        is_del = bool(rng.integers(0, 2))
        k = int(rng.integers(1, 6)) if rng.random() < 0.9 else int(rng.integers(6, 40))
        events.append(ev_pack(j, k, is_del))
        j = (j + min(k, L - j) if is_del else j + 1) + int(rng.integers(0, max(1, 2 * L // (n_events + 1))))
    t = codes[::-1].copy() if reverse else codes.copy()
    if reverse:
        t[t < 4] ^= 2
    shown = np.ones(L, dtype=np.int64)                               # read bases per template base
    for w in events:
        j, k, is_del = ev_unpack(w)
        if is_del:
            shown[j:j + k] = 0
        else:
            shown[j] += k
    src = np.repeat(np.arange(L), shown)                             # the template base a read position stands on or behind
    n = src.size
    letters = np.frombuffer(b"ACTGNNN", dtype=np.uint8)
    seq = letters[t[src]].copy()
    change = rng.random(n) < mismatch
    change[1:] |= src[1:] == src[:-1]                                # inserted bases are anything
    seq[change] = letters[rng.integers(0, 4, int(change.sum()))]
    seq[rng.random(n) < mismatch / 5] = ord("N")
    quals = bytes((33 + qual_lo + rng.integers(0, n_qual, n)).astype(np.uint8))
    return codes, reverse, events, seq.tobytes(), quals
