"""Profiles of any shape the trainer can write (`seqToProfile -k 1..5 -B 10..L`), generated at test time, and the small
runs that sample from them.

`write_profile(path, Shape(...))` writes a `.profile` in the format of the shipped files (and of host/profile.cpp and the
reference's Profile::train): the scalar sections (indel rates and lengths, insert-size spread, GC model) come from a
shipped profile under golden/testData; the sections whose size depends on the k-mer and the bin count are made here from
a seeded generator, built to give a byte-for-byte comparison power:
  * every (mate, context, bin) substitution row differs from every other one, neighbours in context and bin included;
  * the error mass is high (2 % to 30 % per row), so that each row is drawn often in a small run;
  * the quality rows differ per (reference base, called base, bin) and have `n_qual_mass` symbols with mass (W, the
    number of alias columns, is the power of two >= that count, at least 4);
  * edge rows on top: all-zero substitution rows (an unseen context copies the base, Profile.cpp:848-853), one-hot rows
    on another base, rows whose identity has no mass; all-zero quality rows (randIndx gives the last symbol,
    MyDefine.cpp:176-184) and single-symbol quality rows on the identity pairs, which every read draws.
An off-by-one context, bin or mate table then changes bytes.

`build_shape_case(shape, wd, layout)` writes that profile, a small genome with variants, N runs and literal X runs (reads
that start with fewer than K bases, contexts reset inside a read), and the configuration.
"""
from __future__ import annotations

import dataclasses
import hashlib
import os
import random

import cases
from simuscop_amd import synth

N_QUAL = 94   # maxBaseQuality - minBaseQuality + 1 of every profile (Profile.cpp:173,208)
SCALAR_SECTIONS = ("Insert Rate", "Insert Frequency", "Deletion Rate", "Deletion Frequency", "Insert Size Standard Deviation",
                   "Log Ratio Mean Value", "Log Ratio Standard Deviation")


@dataclasses.dataclass(frozen=True)
class Shape:
    kmer: int
    bins: int
    read_length: int = 151
    n_qual_mass: int = 41        # quality symbols with mass in the widest row: 1..4 -> W 4, 8 -> 8, 41 -> 64, 65.. -> 128
    bases: str = "ACTG"
    mate2: bool = True           # False: insert-size SD 0 -> a PE run samples mate 2 from the mate-1 table
    indel_scale: float = 4.0     # sequencing indel rates of the scalar source x this: reads with >= 2 events are common
    seed: int = 1
    source: str = "xten"         # shipped profile the scalar sections come from
    edge_rows: bool = True       # False: no deterministic rows (the closed-form histograms assume random cells)

    @property
    def W(self):
        w = 4
        while w < self.n_qual_mass:
            w *= 2
        return w

    @property
    def tag(self):
        t = f"k{self.kmer}_b{self.bins}_L{self.read_length}_q{self.n_qual_mass}"
        if self.bases != "ACTG":
            t += "_" + self.bases
        if not self.mate2:
            t += "_sd0"
        if not self.edge_rows:
            t += "_plain"
        return t


def kmer_names(kmer, bases):
    """Context names in Profile::initKmers order (Profile.cpp:70-124): contexts of m = 1..K real bases, X-prefixed, in
    base-N counting order of `bases` (oldest base in the highest digit).  Index = position in this list."""
    out = []
    for m in range(1, kmer + 1):
        for v in range(4 ** m):
            s = "".join(bases[(v >> (2 * (m - 1 - t))) & 3] for t in range(m))
            out.append("X" * (kmer - m) + s)
    return out


def scalar_sections(source):
    """{section: [lines]} of the shipped profile's scalar sections."""
    lines = open(os.path.join(cases.TESTDATA, cases.PROFILES[source])).read().split("\n")
    secs, cur = {}, None
    for ln in lines:
        if ln.startswith("[") and ln.endswith("]"):
            cur = ln[1:-1]
            secs[cur] = []
        elif cur is not None and ln.strip():
            secs[cur].append(ln)
    return {k: secs[k] for k in SCALAR_SECTIONS}


def n_ins(shape):
    """Length of the insert-length table (sg_profile_cdf.n_ins): it enters the 32-bit bin-arithmetic limit."""
    return len(scalar_sections(shape.source)["Insert Frequency"][0].split("\t"))


def _g(x):
    return "%.6g" % x


def _sub_rows(rng, shape, names):
    """Lines of [Substitution Probs]: per context, bins rows of mate 1 then bins rows of mate 2."""
    out, seen = [], set()
    for ci, name in enumerate(names):
        ident = shape.bases.index(name[-1])
        out.append("kmer: " + name)
        for t in range(2):
            for b in range(shape.bins):
                u = rng.random() if shape.edge_rows else 1.0
                if u < 0.01:        # all zero: the context was never seen in training
                    row = [0.0] * 4
                elif u < 0.02:      # one-hot on another base: that base, always
                    row = [0.0] * 4
                    row[(ident + 1 + rng.randrange(3)) % 4] = 1.0
                elif u < 0.03:      # the identity has no mass
                    row = [rng.uniform(0.1, 1.0) for _ in range(4)]
                    row[ident] = 0.0
                else:
                    err = rng.uniform(0.02, 0.30)
                    w = [rng.uniform(0.05, 1.0) for _ in range(3)]
                    s = sum(w)
                    row = [0.0] * 4
                    row[ident] = 1.0 - err
                    others = [k for k in range(4) if k != ident]
                    for k, x in zip(others, w):
                        row[k] = err * x / s
                line = "\t".join(_g(x) for x in row)
                if u >= 0.03:
                    assert line not in seen      # (six significant digits of four draws: never happens, but it is the point)
                    seen.add(line)
                out.append(line)
    return out


def _qual_rows(rng, shape):
    """Lines of [Base Quality Distribution]: basePairIndx = reference index * 4 + called index, bins rows of 94."""
    out = []
    n = max(1, min(shape.n_qual_mass, N_QUAL))
    for bp in range(16):
        identity = bp // 4 == bp % 4
        out.append("basePairIndx: %d" % bp)
        for b in range(shape.bins):
            row = [0.0] * N_QUAL
            u = rng.random()
            if shape.edge_rows and identity and b % 7 == 3 and bp == 5:   # reachable all-zero row: always the last symbol
                pass
            elif shape.edge_rows and identity and b % 5 == 1:             # single-symbol row
                row[rng.randrange(N_QUAL)] = 1.0
            else:
                for k in rng.sample(range(N_QUAL), n):
                    row[k] = rng.uniform(0.05, 1.0)
                if u < 0.02 and n > 1:                    # a row of fewer symbols now and then
                    for k in rng.sample([k for k in range(N_QUAL) if row[k] > 0], n // 2):
                        row[k] = 0.0
            out.append("\t".join("0" if x == 0 else _g(x) for x in row))
    return out


def profile_text(shape):
    assert 1 <= shape.kmer <= 5 and 1 <= shape.bins <= shape.read_length and sorted(shape.bases) == list("ACGT")
    rng = random.Random(f"{shape.tag}/{shape.seed}")
    sc = scalar_sections(shape.source)
    names = kmer_names(shape.kmer, shape.bases)
    lines = ["#model generated by tests/profile_shapes.py", "", f"bases: {shape.bases}", f"readLength: {shape.read_length}",
             f"binCount: {shape.bins}", f"kmer: {shape.kmer}", ""]
    for sec in ("Insert Rate", "Insert Frequency", "Deletion Rate", "Deletion Frequency"):
        body = sc[sec]
        if sec.endswith("Rate"):
            body = [_g(float(body[0]) * shape.indel_scale)]
        lines += ["[%s]" % sec] + body + [""]
    lines += ["[Substitution Probs]"] + _sub_rows(rng, shape, names) + [""]
    lines += ["[Base Quality Distribution]"] + _qual_rows(rng, shape) + [""]
    lines += ["[Insert Size Standard Deviation]", sc["Insert Size Standard Deviation"][0] if shape.mate2 else "0", ""]
    lines += ["[Log Ratio Mean Value]"] + sc["Log Ratio Mean Value"] + [""]
    lines += ["[Log Ratio Standard Deviation]"] + sc["Log Ratio Standard Deviation"] + [""]
    return "\n".join(lines)


def write_profile(path, shape):
    with open(path, "w") as f:
        f.write(profile_text(shape))
    return path


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def write_genome(path, seed=5):
    """Two contigs: N islands every 3 kb (fragments run into them) and literal X runs of 1-7 bases (the reference's
    place-holder context character in the middle of a read) every ~4 kb."""
    a = bytearray(synth.synth_contig(90000, seed, 0, n_islands=(3000, 20)).tobytes())
    rng = random.Random(seed)
    for p in range(1700, len(a) - 10, 4100):
        a[p:p + 1 + rng.randrange(7)] = b"X" * (1 + rng.randrange(7))
    a = bytes(a[:90000])
    b = synth.synth_contig(25000, seed, 1, n_runs=False).tobytes()
    cases._fasta_of(path, [(b"chr3", a), (b"chr8", b)])
    return [("chr3", len(a)), ("chr8", len(b))]


def build_shape_case(shape, wd, layout="PE", coverage=None, profile=None, seed=5):
    """Profile (unless `profile` names one), genome, variants, configuration of one shape; returns the config path."""
    os.makedirs(wd, exist_ok=True)
    prof = profile or write_profile(os.path.join(wd, shape.tag + ".profile"), shape)
    fa = os.path.join(wd, "ref.fa")
    contigs = write_genome(fa, seed)
    L = contigs[0][1]
    cases._write(os.path.join(wd, "variations.txt"), cases._variations("v", "chr3", L / 63025520.0))
    cases._write(os.path.join(wd, "snp.txt"), cases._snps("chr3", L, 400, 3) + cases._snps("chr8", contigs[1][1], 300, 4))
    if coverage is None:
        coverage = max(2, round(1200.0 / shape.read_length))
    cfg = os.path.join(wd, "config.txt")
    cases._config(cfg, ref=fa, profile=prof, variation=os.path.join(wd, "variations.txt"), snp=os.path.join(wd, "snp.txt"),
                  name="v", output=os.path.join(wd, "out"), layout=layout, threads=1, verbose=0, coverage=coverage,
                  insertSize=max(350, 2 * shape.read_length + 50))
    return cfg
