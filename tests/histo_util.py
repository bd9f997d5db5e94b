"""Histograms of emitted FASTQ against their CLOSED-FORM expectation from the `.profile` (test infrastructure).

SURVEY 8(c)'s golden families, evaluated on the text alone (what a run emitted), for a run over ONE contig of at most one
segment with `ploidy = 1` and no variants -- the position in a record's name is then a coordinate of the reference
itself (Segment.cpp:809: pos % segsize):

  G1  substitution counts per (mate, bin, k-mer context, called base) against the rows of subsCdf1 / subsCdf2
      (Profile::getSubBaseIndx1/2, Profile.cpp:1527-1554; the mate-2 table is used for mate 2 of paired runs, :1420-1430)
  G2  quality counts per (mate, bin, ref base, called base, symbol) against qualityCdf (Profile::getBaseQuality, :1576-1580)
  G3  mean read-length change against the indel model (Profile::getIndelSeq, :1556-1574)
  G4  insert sizes against the truncated discretised normal of normParas (:912-930) drawn by yieldInsertSize (:1486-1493)
  G5  pairs per 1 kbp window: (count/c - gcMeans[gc]) / gcStd must be a standard normal variate (Profile::getGCFactor,
      :1507-1517; Segment.cpp:576-586, :462-476)

The expectations are the reference's own in-memory tables (the oracle's loader reproduces them; `orc_profile_array`).
Every statistic is a z-score or a Bonferroni-corrected exact binomial tail; bar |z| < 5, corrected p > 1e-4 -- with fixed
seeds the tests are deterministic."""
from __future__ import annotations

import ctypes

import numpy as np
from scipy import stats as sps

Z_MAX = 5.0
P_MIN = 1e-4

_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    _COMP[_a] = _b


class ProfileTables:
    """The reference's sampling tables as probabilities (differences of its cumulative rows)."""

    def __init__(self, lib, path, paired, insert_size):
        h = lib.orc_profile_load(path.encode(), 1 if paired else 0, insert_size)
        assert h, path
        info = lambda i: lib.orc_profile_info(h, i)  # noqa: E731
        self.N, self.kmer, self.bins, self.L, self.kc, self.nq = (info(i) for i in range(6))
        assert self.N == 4 and 1 <= self.kmer <= 6

        def arr(which, shape):
            p = lib.orc_profile_array(h, which)
            return np.ctypeslib.as_array(p, shape=shape).copy() if p else None

        def pdf(c):
            """Probabilities of randIndx (MyDefine.cpp:176-184): first k with r <= cdf[k], the last entry takes what is left."""
            p = np.diff(np.concatenate([np.zeros(c.shape[:-1] + (1,)), c], axis=-1), axis=-1)
            if c.shape[-1] > 1:
                p[..., -1] = 1.0 - c[..., -2]
            return p

        self.sub = [pdf(arr(2, (self.kc, self.bins, 4)))]
        s2 = arr(3, (self.kc, self.bins, 4)) if info(9) else None
        self.sub.append(pdf(s2) if s2 is not None else self.sub[0])
        self.qual = pdf(arr(4, (16, self.bins, self.nq)))
        n_is = info(8)
        self.isize_min = info(10)
        self.isize_pmf = pdf(arr(5, (n_is,))) if n_is else None
        self.ins_rate, self.del_rate, self.std_isize, self.gc_std = (lib.orc_profile_rate(h, i) for i in range(4))
        self.ins_len = pdf(arr(0, (info(6),)))
        self.del_len = pdf(arr(1, (info(7),)))
        self.gc_means = arr(6, (101,))
        buf = ctypes.create_string_buffer(8)
        self.kmers = []
        for i in range(self.kc):
            lib.orc_profile_kmer(h, i, buf)
            self.kmers.append(buf.raw[:self.kmer].decode())
        lib.orc_profile_free(h)
        self.bases = "".join(self.kmers[i][-1] for i in range(4))  # table order of the bases ("ACTG" in the shipped files)
        self.code = np.full(256, 255, dtype=np.uint8)
        for i, b in enumerate(self.bases):
            self.code[ord(b)] = i
        # context index from the codes of the last K source bases, oldest first in the highest base-5 digit (4 = 'X', before
        # the read's start: the contexts of a read's first K-1 bases are X-prefixed, Profile.cpp:1660-1663)
        lut = np.full(5 ** self.kmer, -1, dtype=np.int32)
        sym = self.bases + "X"
        for i, k in enumerate(self.kmers):
            lut[sum(sym.index(ch) * 5 ** (self.kmer - 1 - t) for t, ch in enumerate(k))] = i
        self.ctx_lut = lut

    def context_of(self, sc):
        """[n, L] base codes (all < 4) -> [n, L] context indexes."""
        K = self.kmer
        x = np.full((sc.shape[0], sc.shape[1] + K - 1), 4, dtype=np.int64)
        x[:, K - 1:] = sc
        v = np.zeros(sc.shape, dtype=np.int64)
        for t in range(K):
            v = v * 5 + x[:, t:t + sc.shape[1]]
        return self.ctx_lut[v]


def read_fasta_one(path):
    """The single contig of a FASTA as an upper-case uint8 array."""
    with open(path, "rb") as f:
        f.readline()
        seq = f.read().replace(b"\n", b"").upper()
    assert b">" not in seq
    return np.frombuffer(seq, dtype=np.uint8)


class Fastq:
    """One FASTQ file as arrays: text, per record the name's position, the offsets and length of bases / qualities."""

    def __init__(self, path):
        buf = np.fromfile(path, dtype=np.uint8)
        nl = np.flatnonzero(buf == 10)
        assert len(nl) % 4 == 0
        starts = np.concatenate([[0], nl[:-1] + 1])
        self.buf = buf
        self.seq_off = starts[1::4]
        self.len = (nl[1::4] - self.seq_off).astype(np.int64)
        self.qual_off = starts[3::4]
        hs, he = starts[0::4], nl[0::4]
        raw = buf.tobytes()
        self.pos = np.fromiter((int(raw[a:b].split(b"#")[2]) for a, b in zip(hs.tolist(), he.tolist())), dtype=np.int64, count=len(hs))
        self.popu = None
        self.n = len(hs)

    def populations(self):
        raw = self.buf.tobytes()
        starts = np.concatenate([[0], np.flatnonzero(self.buf == 10)[:-1] + 1])[0::4]
        out = {}
        for a in starts.tolist():
            p = raw[a + 1:raw.index(b"#", a)]
            out[p] = out.get(p, 0) + 1
        return out

    def matrix(self, off, rows, L):
        return self.buf[off[rows][:, None] + np.arange(L)[None, :]]


def _binom_two_sided(k, n, p):
    """Exact two-sided binomial tail (doubling the smaller one-sided tail), vectorised."""
    lo = sps.binom.cdf(k, n, p)
    hi = sps.binom.sf(k - 1, n, p)
    return np.minimum(1.0, 2.0 * np.minimum(lo, hi))


def categorical_report(counts, probs, min_expected=5.0):
    """counts/probs [..., K]: rows of categorical draws against their probabilities.

    * Pearson chi-square, row by row: the outcomes with an expectation of at least `min_expected` are cells of their own,
      the rest of the row is pooled into one more cell (kept if its expectation reaches the bound, otherwise the row is
      conditioned on the kept cells); dof = cells - 1 per row.  Returns its z = (chi2 - dof) / sqrt(2 dof) and dof.
    * every single cell against its exact binomial law: the smallest two-sided tail, Bonferroni-corrected.
    * an outcome of probability zero must not occur at all."""
    counts = np.asarray(counts, dtype=np.float64)
    probs = np.broadcast_to(probs, counts.shape)
    # an outcome of probability zero: a handful can come from reads whose equal-sized insertion and deletion sit a few bases
    # apart next to a real substitution (their bases are then counted under the wrong row); more than that is a sampler bug
    impossible = float(counts[probs == 0].sum())
    assert impossible <= max(3.0, 2e-6 * counts.sum()), f"{impossible:.0f} outcomes of probability zero were emitted (of {counts.sum():.0f})"
    n = counts.sum(axis=-1, keepdims=True)
    e = n * probs
    big = e >= min_expected
    c_pool = np.where(big, 0.0, counts).sum(axis=-1, keepdims=True)
    p_pool = np.where(big, 0.0, probs).sum(axis=-1, keepdims=True)
    keep_pool = n * p_pool >= min_expected
    c_all = np.concatenate([np.where(big, counts, 0.0), np.where(keep_pool, c_pool, 0.0)], axis=-1)
    p_all = np.concatenate([np.where(big, probs, 0.0), np.where(keep_pool, p_pool, 0.0)], axis=-1)
    n_c = c_all.sum(axis=-1, keepdims=True)                      # the row conditioned on the kept cells
    p_c = p_all / np.maximum(p_all.sum(axis=-1, keepdims=True), 1e-300)
    e_c = n_c * p_c
    cells = (p_all > 0)
    ncell = cells.sum(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(cells & (e_c > 0), (c_all - e_c) ** 2 / e_c, 0.0)
    rows = ncell >= 2
    chi2 = term[rows].sum()
    dof = int((ncell[rows] - 1).sum())
    z = (chi2 - dof) / np.sqrt(2.0 * dof) if dof else 0.0
    test = (np.broadcast_to(n, e.shape) > 0) & (probs > 0) & (probs < 1)
    pv = _binom_two_sided(counts[test], np.broadcast_to(n, e.shape)[test], probs[test])
    worst = int(np.argmin(pv)) if len(pv) else -1
    pmin = float(pv.min() * len(pv)) if len(pv) else 1.0
    return float(z), dof, min(1.0, pmin), int(len(pv)), (float(counts[test][worst]), float(e[test][worst])) if worst >= 0 else None


def mismatch_cut(T: ProfileTables, mate2):
    """Most mismatches a read without sequencing indels plausibly shows: m + 6 sqrt(m) + 2, m = what the tables expect."""
    p_sub = T.sub[1 if mate2 else 0]
    ident = np.array([T.bases.index(k[-1]) for k in T.kmers])
    p_mis = 1.0 - p_sub[np.arange(T.kc), :, ident]                # [kc, bins]
    full = np.array(["X" not in k for k in T.kmers])
    m_exp = float(p_mis[full].mean(axis=0)[(np.arange(T.L) * T.bins // T.L)].sum())
    return int(np.ceil(m_exp + 6.0 * np.sqrt(m_exp) + 2.0))


def sub_and_quality_counts(T: ProfileTables, fq: Fastq, src_of, rows, mate2):
    """Counts of (bin, context, called) and (bin, ref*4+called, symbol) over the records `rows` whose source bases (the
    template in read orientation, length L) `src_of(rows_chunk)` returns.  A read of nominal length can still carry an
    insertion and a deletion of the same size (about 0.3 % of the reads at the shipped rates): the stretch between them is
    shifted and reads as a run of mismatches.  Such reads are cut off by their mismatch count: more than
    m + 6 sqrt(m) + 2, with m the mismatches per read the tables expect (a Poisson tail below 1e-7 for reads without indels).
    Returns (sub counts, quality counts, reads used, mismatches)."""
    L, bins = T.L, T.bins
    cut = mismatch_cut(T, mate2)
    sub = np.zeros((bins, T.kc, 4), dtype=np.int64)
    qual = np.zeros((bins, 16, T.nq), dtype=np.int64)
    jbin = (np.arange(L) * bins // L).astype(np.int32)
    used = mism = 0
    for c0 in range(0, len(rows), 100000):
        r = rows[c0:c0 + 100000]
        src = src_of(r)                                   # [n, L] ASCII
        called = T.code[fq.matrix(fq.seq_off, r, L)]
        q = fq.matrix(fq.qual_off, r, L)
        sc = T.code[src]
        ok = (sc < 4).all(axis=1) & (called < 4).all(axis=1)
        d = (sc != called).sum(axis=1)
        ok &= d <= cut
        # ... and, below the cut, by their shape: every base from the first to the last mismatch equals the template k = 1..3
        # positions to the left or right (an insertion and a deletion of k bases a few positions apart)
        multi = np.flatnonzero(ok & (d >= 2))
        if len(multi):
            cm, sm = called[multi], sc[multi]
            mm = cm != sm
            first = mm.argmax(axis=1)
            last = L - 1 - mm[:, ::-1].argmax(axis=1)
            jj = np.arange(L)[None, :]
            inside = (jj >= first[:, None]) & (jj <= last[:, None])
            shifted = np.zeros(len(multi), dtype=bool)
            for k in (1, 2, 3):
                eq_r = np.zeros_like(mm)
                eq_r[:, k:] = cm[:, k:] == sm[:, :-k]          # called[j] == src[j-k]
                eq_l = np.zeros_like(mm)
                eq_l[:, :-k] = cm[:, :-k] == sm[:, k:]         # called[j] == src[j+k]
                shifted |= (eq_r | ~inside).all(axis=1) | (eq_l | ~inside).all(axis=1)
            ok[multi[shifted]] = False
        sc, called, q = sc[ok].astype(np.int32), called[ok].astype(np.int32), q[ok].astype(np.int32) - 33
        used += int(ok.sum())
        mism += int(d[ok].sum())
        ctx = T.context_of(sc)
        assert (ctx >= 0).all()
        b = np.broadcast_to(jbin, ctx.shape)
        sub += np.bincount(((b * T.kc + ctx) * 4 + called).ravel(), minlength=sub.size).reshape(sub.shape)
        qual += np.bincount(((b * 16 + sc * 4 + called) * T.nq + q).ravel(), minlength=qual.size).reshape(qual.shape)
    return sub, qual, used, mism


def check_sub_and_quality(T: ProfileTables, sub, qual, mate2, what):
    """Assert G1 and G2 for one mate's counts."""
    p_sub = np.transpose(T.sub[1 if mate2 else 0], (1, 0, 2))          # [bins, kc, 4]
    z, dof, pmin, cells, worst = categorical_report(sub, p_sub)
    assert abs(z) < Z_MAX and pmin > P_MIN, f"{what} G1 substitution rows: chi2 z={z:.2f} dof={dof}, corrected min p={pmin:.2e} of {cells}, worst {worst}"
    out = {"g1_z": round(z, 2), "g1_dof": dof, "g1_cells": cells, "g1_pmin": pmin}
    # only the substituted outcomes (the identity cell holds ~0.999 of a row and would hide them in a pooled statistic)
    off = sub.copy().astype(np.float64)
    ident = np.zeros_like(p_sub, dtype=bool)
    for i, k in enumerate(T.kmers):
        ident[:, i, T.bases.index(k[-1])] = True
    n = sub.sum(axis=-1, keepdims=True)
    e = n * p_sub
    sel = (~ident) & (e >= 5)
    # (binomial variance n p (1 - p) per cell: the shipped rows' p ~ 1e-3 make it n p, the generated shapes' are up to 0.3)
    chi2 = (((off - e) ** 2)[sel] / (e * np.maximum(1.0 - p_sub, 1e-12))[sel]).sum()
    d2 = int(sel.sum())
    z2 = (chi2 - d2) / np.sqrt(2.0 * d2)
    assert abs(z2) < Z_MAX, f"{what} G1 substituted outcomes: chi2 z={z2:.2f} dof={d2}"
    out.update(g1_offdiag_z=round(float(z2), 2), g1_offdiag_dof=d2, substitutions=int(off[~ident].sum()))
    p_q = np.transpose(T.qual, (1, 0, 2))                               # [bins, 16, nq]
    z, dof, pmin, cells, worst = categorical_report(qual, p_q)
    assert abs(z) < Z_MAX and pmin > P_MIN, f"{what} G2 quality rows: chi2 z={z:.2f} dof={dof}, corrected min p={pmin:.2e} of {cells}, worst {worst}"
    out.update(g2_z=round(z, 2), g2_dof=dof, g2_cells=cells, g2_pmin=pmin)
    # the rows of substituted bases on their own (ref != called: 12 of the 16 base pairs)
    offp = np.array([r * 4 + c for r in range(4) for c in range(4) if r != c])
    z, dof, pmin, cells, worst = categorical_report(qual[:, offp, :], p_q[:, offp, :])
    assert abs(z) < Z_MAX and pmin > P_MIN, f"{what} G2 quality rows of substituted bases: z={z:.2f} dof={dof} pmin={pmin:.2e}"
    out.update(g2_sub_z=round(z, 2), g2_sub_dof=dof)
    return out


def forward_source(ref, fq, L):
    def f(rows):
        return ref[fq.pos[rows][:, None] + np.arange(L)[None, :]]
    return f


def reverse_source(ref, ends, L):
    """Source of reads sampled from the reverse strand: revcomp(ref[end-L:end]); `ends` per record (absolute array)."""
    def f(rows):
        e = ends[rows]
        return _COMP[ref[(e[:, None] - 1 - np.arange(L)[None, :])]]
    return f


def recover_insert_sizes(ref, fq1: Fastq, fq2: Fastq, L, isz_max):
    """Per pair the fragment length, from the text alone: mate 2 = revcomp(ref[pos+isz-L : pos+isz]); its reverse
    complement is looked up inside ref[pos : pos+isz_max] by exact 24-base seeds and checked by its mismatch count.
    Returns an int array (-1: mate 2 not of nominal length, clipped at the contig end, or not placed)."""
    raw = ref.tobytes()
    buf2 = fq2.buf
    out = np.full(fq1.n, -1, dtype=np.int64)
    seeds = [s for s in (L // 2 - 12, 8, L - 36, L // 4, 3 * L // 4 - 12) if 0 <= s <= L - 24]
    comp = bytes(_COMP)
    pos = fq1.pos.tolist()
    so, ln = fq2.seq_off.tolist(), fq2.len.tolist()
    b2 = buf2.tobytes()
    n_ref = len(raw)
    for i in range(fq1.n):
        if ln[i] != L:
            continue
        p = pos[i]
        if p + isz_max + 8 > n_ref:
            continue
        rc = b2[so[i]:so[i] + L].translate(comp)[::-1]
        win = raw[p:p + isz_max + 8]
        for s in seeds:
            o = win.find(rc[s:s + 24])
            if o >= 0:
                a = o - s
                if a >= 0 and a + L <= len(win):
                    out[i] = a + L
                    break
    # verify the placements: the whole read against the template it was placed on
    rows = np.flatnonzero(out >= 0)
    for c0 in range(0, len(rows), 100000):
        r = rows[c0:c0 + 100000]
        e = fq1.pos[r] + out[r]
        tmpl = _COMP[ref[(e[:, None] - 1 - np.arange(L)[None, :])]]
        bad = (tmpl != fq2.matrix(fq2.seq_off, r, L)).sum(axis=1) > L // 4
        out[r[bad]] = -1
    return out


def check_insert_sizes(T: ProfileTables, isz, what):
    """G4: recovered fragment lengths against the pmf of the insert-size alphabet."""
    v = isz[isz >= 0]
    k = len(T.isize_pmf)
    assert v.min() >= T.isize_min and v.max() < T.isize_min + k, (v.min(), v.max(), T.isize_min, k)
    counts = np.bincount(v - T.isize_min, minlength=k).astype(np.float64)
    e = counts.sum() * T.isize_pmf
    sel = e >= 5
    chi2 = ((counts - e) ** 2 / e)[sel].sum()
    dof = int(sel.sum()) - 1
    z = (chi2 - dof) / np.sqrt(2.0 * dof)
    mean_e = float((np.arange(k) * T.isize_pmf).sum() + T.isize_min)
    sd_e = float(np.sqrt(((np.arange(k) + T.isize_min - mean_e) ** 2 * T.isize_pmf).sum()))
    zm = (v.mean() - mean_e) / (sd_e / np.sqrt(len(v)))
    assert abs(z) < Z_MAX and abs(zm) < Z_MAX, f"{what} G4 insert size: chi2 z={z:.2f} (dof {dof}), mean z={zm:.2f}"
    return {"g4_z": round(float(z), 2), "g4_dof": dof, "g4_mean_z": round(float(zm), 2), "pairs": int(len(v))}


def read_length_pmf(T: ProfileTables):
    """Exact law of the read length: the first loop of Profile::predict (Profile.cpp:1607-1634) as a forward recursion over
    (template position, net length change).  At position j: an insertion of a ~ insCdf bases with probability pI (then
    j+1); else a deletion of k ~ delCdf bases with probability pD/(1-pI) of the rest, cut to min(k, n-j) and SKIPPING the
    deleted positions' own draws (j += k); a read that would fall below 50 bases drops all its indels (:1627-1634).
    Returns (pmf over lengths 0..n+span, span)."""
    n = T.L
    p_i = T.ins_rate
    p_d = (1.0 - p_i) * (T.del_rate / (1.0 - p_i))
    span = 4 * len(T.ins_len) + 8
    width = n + span + 1                       # net change d in [-n, span] at index d + n
    v = np.zeros((n + 1, width))
    v[0, n] = 1.0
    for j in range(n):
        cur = v[j]
        if not cur.any():
            continue
        v[j + 1] += cur * (1.0 - p_i - p_d)
        for a, pa in enumerate(T.ins_len):       # length = index into the row (getInsertLen, Profile.cpp:1519-1521)
            if pa > 0 and a > 0:
                v[j + 1, a:] += cur[:width - a] * (p_i * pa)
        for k, pk in enumerate(T.del_len):
            if pk > 0 and k > 0:
                kk = min(k, n - j)
                v[j + kk, :width - kk] += cur[kk:] * (p_d * pk)
    fin = v[n]
    pmf = np.zeros(n + span + 1)
    for idx, pr in enumerate(fin):
        length = n + (idx - n)
        if pr > 0:
            pmf[n if length < 50 else length] += pr
    return pmf, span


def check_read_lengths(T: ProfileTables, lens, what):
    """G3: the read-length histogram against its exact law (read_length_pmf)."""
    pmf, span = read_length_pmf(T)
    assert abs(pmf.sum() - 1.0) < 1e-6, pmf.sum()   # (the tail beyond `span` inserted bases is cut)
    assert lens.max() < len(pmf)
    counts = np.bincount(lens, minlength=len(pmf)).astype(np.float64)
    z, dof, pmin, cells, worst = categorical_report(counts[None, :], pmf[None, :])
    exp_mean = float((np.arange(len(pmf)) * pmf).sum())
    sd = float(np.sqrt(((np.arange(len(pmf)) - exp_mean) ** 2 * pmf).sum()))
    # (a profile without sequencing indels: one possible length, which every read must have)
    zm = (lens.mean() - exp_mean) / (sd / np.sqrt(len(lens))) if sd > 0 else (0.0 if lens.mean() == exp_mean else np.inf)
    rep = {"g3_z": round(z, 2), "g3_dof": dof, "g3_pmin": pmin, "g3_mean_z": round(float(zm), 2), "mean_length": round(float(lens.mean()), 5),
           "expected_mean_length": round(exp_mean, 5), "changed_fraction": round(float((lens != T.L).mean()), 4),
           "expected_changed_fraction": round(float(1 - pmf[T.L]), 4)}
    ok = abs(z) < Z_MAX and abs(zm) < Z_MAX and pmin > P_MIN
    return rep, (0.0 if ok else 99.0)


def gc_percent_windows(ref, frag=1000):
    """calculateGCPercent (MyDefine.cpp:279-303) per full 1 kbp tile: 100*GC/len as an integer, -1 with any N."""
    n = len(ref) // frag
    m = ref[:n * frag].reshape(n, frag)
    gc = ((m == ord("G")) | (m == ord("C"))).sum(axis=1)
    bad = (~np.isin(m, np.frombuffer(b"ACGT", dtype=np.uint8))).any(axis=1)
    out = (100 * gc // frag).astype(np.int64)
    out[bad] = -1
    return out


def gc_factor_z(T: ProfileTables, ref, positions, paired, frag=1000):
    """G5: pairs per 1 kbp window -> the standardised GC factor each window drew.  ploidy 1, one segment: window w has
    weight f_w/frag (Segment.cpp:576), reads trunc(w * reads / WL) (:462-476), pairs ceil(n/2) (:848), so
    pairs_w = c * f_w up to +-1 with one constant c; f_w ~ N(gcMeans[gc_w], gcStd) redrawn while negative.  Returns, for
    every interior window, the standard normal variate its factor maps to under that law (window 0 takes the segment's remainder; the last, shorter tile has another weight form)."""
    gc = gc_percent_windows(ref, frag)
    nwin = len(gc)
    cnt = np.bincount(positions // frag, minlength=nwin + 1)[:nwin].astype(np.float64)
    sel = (np.arange(nwin) > 0) & (gc >= 0)
    mu = T.gc_means[np.clip(gc, 0, 100)][sel]
    sd = T.gc_std
    # the factor is N(mu, sd) redrawn while negative: a normal truncated at zero
    alpha = -mu / sd
    tail = sps.norm.sf(alpha)
    mean_f = mu + sd * sps.norm.pdf(alpha) / tail
    # a window's count stands for an interval of factors: reads = trunc(f c) covers [n, n+1) (SE, midpoint n + 1/2); pairs =
    # ceil(trunc(2 f c) / 2) covers [p - 1/2, p + 1/2) in pair units (PE, midpoint p)
    mid = cnt[sel] + (0.0 if paired else 0.5)
    if paired:
        mid[cnt[sel] == 0] = 0.25        # no pair: trunc(2 f c) = 0, the interval [0, 1/2)
    c = mid.sum() / mean_f.sum()
    f = mid / c
    u = (sps.norm.cdf((f - mu) / sd) - sps.norm.cdf(alpha)) / tail
    z = sps.norm.ppf(np.clip(u, 1e-12, 1 - 1e-12))      # standard normal under the model, whatever the truncation
    return z, gc[sel], c


def normal_report(z):
    """Moments and Kolmogorov distance of a sample against N(0,1)."""
    n = len(z)
    ks = sps.kstest(z, "norm")
    return {"n": int(n), "mean": round(float(z.mean()), 4), "var": round(float(z.var(ddof=1)), 4), "skew": round(float(sps.skew(z)), 4),
            "excess_kurtosis": round(float(sps.kurtosis(z)), 4), "ks_D": round(float(ks.statistic), 5), "ks_p": float(ks.pvalue),
            "z_var": round(float((z.var(ddof=1) - 1) / np.sqrt(2.0 / (n - 1))), 2), "z_skew": round(float(sps.skew(z) / np.sqrt(6.0 / n)), 2),
            "z_kurt": round(float(sps.kurtosis(z) / np.sqrt(24.0 / n)), 2)}


# ---- a whole run --------------------------------------------------------------------------------------------------------
def histogram_config(cases, wd, profile, layout, coverage, insert, length=1400000, seed=83):
    """One contig without N runs (a single segment: 1.4 Mbp < 1.5 segMaxSize, Genome.cpp:741-763), ploidy 1, no variants.
    `profile`: a shipped profile's key in cases.PROFILES, or the path of another profile file."""
    import os
    from simuscop_amd import synth
    fa = os.path.join(wd, "ref.fa")
    synth.write_fasta(fa, [("chr1", length)], seed=seed, n_runs=False)
    cfg = os.path.join(wd, "config.txt")
    cases._config(cfg, ref=fa, profile=profile if os.path.isfile(profile) else os.path.join(cases.TESTDATA, cases.PROFILES[profile]), name="h", output=os.path.join(wd, "out"),
                  layout=layout, threads=1, verbose=0, coverage=coverage, insertSize=insert, ploidy=1)
    return cfg, fa


def analyse_run(lib, cases, profile, layout, insert, fasta, files, what, want_gc=True, profile_path=None):
    """All closed-form families on the FASTQ files of one run (see the module docstring).  Returns the report.
    `profile_path`: a profile file other than the shipped one `profile` names."""
    import os
    paired = layout == "PE"
    T = ProfileTables(lib, profile_path or os.path.join(cases.TESTDATA, cases.PROFILES[profile]), paired, insert)
    ref = read_fasta_one(fasta)
    L = T.L
    rep = {"profile": profile, "layout": layout, "read_length": L}
    fq1 = Fastq(files[0])
    rep["records"] = fq1.n
    g3, z3 = check_read_lengths(T, fq1.len, what)
    rep["mate1"] = dict(g3)
    assert abs(z3) < Z_MAX, f"{what} G3 read length: {g3}"
    nominal = np.flatnonzero((fq1.len == L) & (fq1.pos + 1000 <= len(ref)))
    if paired:
        sub, qual, used, mism = sub_and_quality_counts(T, fq1, forward_source(ref, fq1, L), nominal, False)
        rep["mate1"].update(check_sub_and_quality(T, sub, qual, False, what + " mate 1"), reads_used=used, mismatch_rate=mism / (used * L))
        fq2 = Fastq(files[1])
        assert fq2.n == fq1.n and np.array_equal(fq1.pos, fq2.pos)
        g3, z3 = check_read_lengths(T, fq2.len, what)
        assert abs(z3) < Z_MAX, f"{what} G3 read length mate 2: {g3}"
        rep["mate2"] = dict(g3)
        isz_max = T.isize_min + len(T.isize_pmf) - 1 if T.isize_pmf is not None else insert
        isz = recover_insert_sizes(ref, fq1, fq2, L, isz_max)
        if T.isize_pmf is not None:
            rep["insert_size"] = check_insert_sizes(T, isz, what)
        placed = np.flatnonzero(isz >= 0)
        ends = fq1.pos + isz
        sub, qual, used, mism = sub_and_quality_counts(T, fq2, reverse_source(ref, ends, L), placed, True)
        rep["mate2"].update(check_sub_and_quality(T, sub, qual, True, what + " mate 2"), reads_used=used, mismatch_rate=mism / (used * L))
        starts = fq1.pos
    else:
        # SE (Segment.cpp:765-778): the fragment is the window's length from pos; read = its first L bases, or the reverse
        # complement of its last L -- strand by a fair coin, always mate-1 tables
        rows = nominal[(fq1.pos[nominal] // 1000) < (len(ref) // 1000)]
        fwd_src = forward_source(ref, fq1, L)
        ends = fq1.pos + 1000
        rev_src = reverse_source(ref, ends, L)
        is_rev = np.zeros(fq1.n, dtype=bool)
        for c0 in range(0, len(rows), 100000):
            r = rows[c0:c0 + 100000]
            called = fq1.matrix(fq1.seq_off, r, L)
            is_rev[r] = (called != rev_src(r)).sum(axis=1) < (called != fwd_src(r)).sum(axis=1)
        rsel = rows[is_rev[rows]]
        fsel = rows[~is_rev[rows]]
        zs = (len(rsel) - 0.5 * len(rows)) / np.sqrt(0.25 * len(rows))
        assert abs(zs) < Z_MAX, f"{what} SE strand coin: {len(rsel)} of {len(rows)} (z={zs:.2f})"
        rep["reverse_fraction"] = round(len(rsel) / len(rows), 4)
        s1, q1, u1, m1 = sub_and_quality_counts(T, fq1, fwd_src, fsel, False)
        s2, q2, u2, m2 = sub_and_quality_counts(T, fq1, rev_src, rsel, False)
        rep["mate1"].update(check_sub_and_quality(T, s1 + s2, q1 + q2, False, what + " SE"), reads_used=u1 + u2, mismatch_rate=(m1 + m2) / ((u1 + u2) * L))
        starts = fq1.pos
    if want_gc:
        z, gcs, c = gc_factor_z(T, ref, starts, paired)
        g5 = normal_report(z)
        g5["pairs_per_unit_factor"] = round(float(c), 2)
        # mean of the factor by GC%: windows of one GC value average to gcMeans[gc] (z of the mean per GC value)
        zmeans = [float(z[gcs == g].mean() * np.sqrt((gcs == g).sum())) for g in np.unique(gcs) if (gcs == g).sum() >= 20]
        g5["max_abs_z_of_mean_by_gc"] = round(max(abs(v) for v in zmeans), 2)
        rep["gc_factor"] = g5
        assert abs(g5["z_var"]) < Z_MAX and abs(g5["z_skew"]) < Z_MAX and abs(g5["z_kurt"]) < Z_MAX and g5["ks_p"] > 1e-6 \
            and g5["max_abs_z_of_mean_by_gc"] < Z_MAX, f"{what} G5 GC factor: {g5}"
    return rep
