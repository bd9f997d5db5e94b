"""The FASTQ record a sampling pass owes for one fragment slot, in plain Python over the oracle library (test
infrastructure; nothing here comes from the engine).

A batch is a table of sampling windows (sg_window rows).  Attempt `a` of window `w` draws one Philox block at the address
(w + first_window, a) of kind PLAN: word 0 places the fragment, pos = int(spos + len * x / 2^32) in fp64; word 2 gives a
single-end read's strand; the fragment is min(bases left in the chain, insert size) long and fails when that is less
than a read.  A window stops after 1,000 failures (the 1,001st ends it) and leaves the slots it did not fill without a
record.  Fragment `done` of a window owns the slot slot_base + done (+ first_slot: the draws of a read are addressed by
the slot in the whole batch), and the name counts the fragments of its segment (oracle.cpp segYieldReads; plan_attempt,
edge_kernel and fragment_kernel in sg_pass_front.hip).  Mate 1 reads the fragment's first L bases, mate 2 (and a single-end read of strand
1) the last L, complemented and reversed; bases and qualities are orc_predict_philox on that template.

`ReadModel.events` restates the indel walk of the oracle's predict (indel_candidate, the length draws, the reset of a
read that would fall under 50 bases) so that a test can say which class of read it checked; test_read_model_cpu.py holds
it to the length of every read orc_predict_philox returns.

Paired runs here use a profile whose insert-size alphabet has one column (`one_column_profile`): every fragment is
insertSize + 1 bases long, so a test that places a window of length 1 places the templates of both mates."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

import profile_shapes as PS

KIND_PLAN, KIND_INDEL, KIND_AUX = 3, 4, 5      # oracle/philox.h
ZERO_FINAL = 2.2204e-16                         # lib/mydefine/MyDefine.cpp:20
COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
_NOT_BASE = bytes(c for c in range(256) if c not in b"ACGTacgt")
_TO_N = bytes.maketrans(_NOT_BASE, b"N" * len(_NOT_BASE))


def one_column_profile(path, shape, sd="0.1"):
    """profile_shapes' profile of `shape` with an insert-size spread so small that int(6 * sd) == 0: the alphabet is the
    single size insertSize + 1 and the mate-2 table is in use (Profile.cpp:912-930, :1420-1430)."""
    lines = PS.profile_text(shape).split("\n")
    at = lines.index("[Insert Size Standard Deviation]")
    lines[at + 1] = sd
    with open(path, "w") as f:
        f.write("\n".join(lines))
    return path


def complement_reverse(seq: bytes) -> bytes:
    """Segment::getComplementSeq + std::reverse (oracle.cpp complementInPlace): anything but ACGT becomes N."""
    return seq.translate(_TO_N).translate(COMPLEMENT)[::-1]


@dataclasses.dataclass
class Slot:
    """One fragment slot of a planned batch (None in a plan's list: a slot without a record)."""
    window: int        # index in the batch's table
    chain: int
    pos: int           # fragment start inside the segment's haplotype string
    foff: int          # ... inside the chain
    flen: int
    strand: int        # single-end only
    fragcount: int     # the name's count: fragments of the segment so far, this one included
    attempt: int
    seg: int


class ReadModel:
    def __init__(self, lib, profile_path, paired, insert_size, seed, batch_id, prefix):
        self.lib, self.paired, self.seed, self.batch_id, self.prefix = lib, bool(paired), seed, batch_id, prefix
        self.h = lib.orc_profile_load(str(profile_path).encode(), 1 if paired else 0, insert_size)
        assert self.h, lib.orc_last_error().decode()
        info = lambda i: lib.orc_profile_info(self.h, i)   # noqa: E731
        self.L, self.n_isize, self.has_sub2, self.isz = info(3), info(8), info(9), info(10)
        self.key = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, seed >> 32)
        ab = (C.c_uint64 * 2)()
        gaps = (C.c_uint64 * self.L)()
        assert lib.orc_profile_indel_gaps(self.h, ab, gaps, self.L) == self.L
        self.evA, self.evB, self.gapS = ab[0], ab[1], [0] + list(gaps)
        self.ins_cdf = np.ctypeslib.as_array(lib.orc_profile_array(self.h, 0), shape=(info(6),)).tolist()
        self.del_cdf = np.ctypeslib.as_array(lib.orc_profile_array(self.h, 1), shape=(info(7),)).tolist()
        self._b, self._q = C.create_string_buffer(2 * (self.L + 4096) + 1), C.create_string_buffer(2 * (self.L + 4096) + 1)
        self._ctr, self._out = (C.c_uint32 * 4)(), (C.c_uint32 * 4)()

    def close(self):
        if self.h:
            self.lib.orc_profile_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- draws -----------------------------------------------------------------------------------------------------------
    def philox(self, c0, c1, c2, kind, ctx24):
        c = self._ctr
        c[0], c[1], c[2], c[3] = c0 & 0xFFFFFFFF, c1, c2, kind | (ctx24 << 8)
        self.lib.orc_philox4x32_10(c, self.key, self._out)
        return tuple(self._out)

    @staticmethod
    def rand_index(x, cdf):
        """randIndxFrom (MyDefine.cpp:176-184): the first k with r <= cdf[k], r the 32-bit draw mapped into (0, 1)"""
        r = ZERO_FINAL + (1 - ZERO_FINAL) * (x / 4294967296.0)
        for k, c in enumerate(cdf):
            if r <= c:
                return k
        return len(cdf) - 1

    # ---- one read --------------------------------------------------------------------------------------------------------
    def template(self, chain: bytes, tmpl_off: int, reverse: bool, complement=True) -> bytes:
        t = chain[tmpl_off:tmpl_off + self.L]
        assert len(t) == self.L, (tmpl_off, len(chain))
        if reverse:
            t = complement_reverse(t) if complement else t[::-1]
        return t

    def read(self, chain, tmpl_off, reverse, mate, slot, is_read1=None, batch_id=None, complement=True):
        """(bases, qualities) of the read of `mate` (0 / 1) in the global `slot`; is_read1 is 0 only for mate 2."""
        t = self.template(chain, tmpl_off, reverse, complement)
        r1 = (0 if mate == 1 else 1) if is_read1 is None else is_read1
        n = self.lib.orc_predict_philox(self.h, t, self.L, r1, self.seed, self.batch_id if batch_id is None else batch_id,
                                        slot & 0xFFFFFFFF, self._b, self._q)
        return self._b.raw[:n], self._q.raw[:n]

    def name(self, pos, seg_size, fragcount, mate):
        tail = b"/%d" % (mate + 1) if self.paired else b""
        return self.prefix + b"%d#%d" % (pos % seg_size, fragcount) + tail

    def record(self, chain, tmpl_off, reverse, mate, slot, pos, seg_size, fragcount, **kw):
        b, q = self.read(chain, tmpl_off, reverse, mate, slot, **kw)
        return self.name(pos, seg_size, fragcount, mate) + b"\n" + b + b"\n+\n" + q + b"\n"

    def events(self, mate, slot):
        """The sequencing indels of the read of `mate` (0; 1 for mate 2) in `slot`: ([(j, 'I' | 'D', len)], reset).  An
        insertion follows template base j, a deletion takes bases [j, j + len) (clipped at the template's end); `reset`:
        the events would leave fewer than 50 bases, so the read has none (Profile.cpp:1640-1646)."""
        n, ctx24 = self.L, (mate << 23) | (self.batch_id & 0xFFFF)
        ev, delta, order = [], 0, 0

        def candidate(e, start):
            o = self.philox(slot, e, 0, KIND_INDEL, ctx24)
            x, y = (o[1] << 32) | o[0], (o[3] << 32) | o[2]
            room = n - start
            if x < self.gapS[room]:
                return n, 0
            g = 0
            while g + 1 < room and x < self.gapS[g + 1]:
                g += 1
            return start + g, (1 if ((y * self.evB) >> 64) < self.evA else 2)

        def length(j, cdf):
            return self.rand_index(self.philox(slot, j, 0, KIND_AUX, ctx24)[0], cdf)

        cand, kind = candidate(order, 0)
        if cand == n:
            return [], False
        order += 1
        j = 0
        while j < n:
            at = j == cand
            k = ins = 0
            if at and kind == 1:
                k = ins = length(j, self.ins_cdf)
            elif at and kind == 2:
                k = length(j, self.del_cdf)
            if not ins and k > 0:
                k = min(n - j, k)
                delta -= k
                ev.append((j, "D", k))
                j += k
            else:
                delta += k
                if k:
                    ev.append((j, "I", k))
                j += 1
            if at:
                cand, kind = (candidate(order, j) if j < n else (n, 0))
                order += 1
        if n + delta < 50:
            return [], True
        return ev, False

    @staticmethod
    def read_class(ev):
        if not ev:
            return "none"
        if len(ev) >= 2:
            return "many"
        return "ins" if ev[0][1] == "I" else "del"

    # ---- the plan --------------------------------------------------------------------------------------------------------
    def attempt(self, win, widx, attempt, clen):
        """(pos, flen, strand) of attempt `attempt` of the window with the batch-wide index widx.  win: (hap_base, chain,
        spos, len, n_reads, seg, slot_base) as in sg_window."""
        hap_base, _, spos, wlen = win[:4]
        x = self.philox(widx, attempt, 0, KIND_PLAN, self.batch_id & 0xFFFF)
        pos = int(spos + wlen * (x[0] / 4294967296.0))
        isz = self.isz if self.paired else wlen
        flen = min(clen - (hap_base + pos), isz)
        return pos, flen, (0 if self.paired else x[2] >> 31)

    def plan_window(self, win, widx, clen):
        """([(attempt, pos, flen, strand)] of the fragments made, attempts drawn)"""
        n = win[4]
        planned = 0 if n <= 0 else ((n + 1) // 2 if self.paired else n)
        made, fail, a = [], 0, 0
        while len(made) < planned:
            pos, flen, strand = self.attempt(win, widx, a, clen)
            a += 1
            if flen < self.L:
                fail += 1
                if fail > 1000:
                    break
                continue
            made.append((a - 1, pos, flen, strand))
        return made, a

    def plan(self, windows, chain_lens, first_window=0):
        """The slots of a batch (or shard) in local slot order: a Slot, or None where the window gave up.  slot_base of
        the rows must be the running sum of the planned fragments."""
        out, count, base = [], {}, 0
        for w, win in enumerate(windows):
            hap_base, chain, _, _, n, seg, slot_base = win
            planned = 0 if n <= 0 else ((n + 1) // 2 if self.paired else n)
            assert slot_base == base == len(out), (w, slot_base, base)
            made, _ = self.plan_window(win, w + first_window, chain_lens[chain])
            for a, pos, flen, strand in made:
                count[seg] = count.get(seg, 0) + 1
                out.append(Slot(w, chain, pos, hap_base + pos, flen, strand, count[seg], a, seg))
            out += [None] * (planned - len(made))
            base += planned
        return out

    def placement(self, s: Slot, mate):
        """(tmpl_off in the chain, reverse) of the read of `mate` from the fragment of slot s"""
        reverse = mate == 1 or (not self.paired and s.strand == 1)
        return (s.foff + s.flen - self.L if reverse else s.foff), reverse

    def slot_record(self, chains, s: Slot, mate, slot, seg_size):
        off, reverse = self.placement(s, mate)
        return self.record(chains[s.chain], off, reverse, mate, slot, s.pos, seg_size, s.fragcount)


def split_records(text: bytes):
    """The records of a FASTQ text, each with its four line ends; the text must hold whole records only."""
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0, "the text does not end on a record"
    return [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]


def first_cycle(got: bytes, want: bytes):
    """(line 0..3, column) of the first byte at which two records differ: line 1 is the bases, 3 the qualities"""
    g, w = got.split(b"\n"), want.split(b"\n")
    for i in range(min(len(g), len(w))):
        if g[i] != w[i]:
            n = min(len(g[i]), len(w[i]))
            return i, next((c for c in range(n) if g[i][c] != w[i][c]), n)
    return min(len(g), len(w)), 0
