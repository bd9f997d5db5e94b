"""Helpers of the --truth-variants GPU tests: the model's counts of one sampling pass (tests/variant_model.py applied to
sg_truth_reads, sg_truth_pieces and sg_haplotype_codes), the table a config's input files give -- read here, not by the
simulator -- the file's rows, and the crowded two-contig case."""
import os
import re

import numpy as np

import cases
import variant_model as vm
from simuscop_amd import synth

HEADER = "#chrom\tpos\ttype\tallele\talt_reads\ttotal_reads\tpopulations"
SUFFIX = ".truth.variants.tsv"

# sg_truth_read (simuscop_amd.h)
READ_DT = np.dtype([("live", "<u4"), ("chain", "<u4"), ("reverse", "<u4"), ("read_len", "<u4"), ("tmpl_off", "<u8"), ("n_events", "<u4"),
                    ("inside", "<u4"), ("events", "<u4", (32,))])


def read_length(cfg):
    prof = re.search(r"^profile = (\S+)", open(cfg).read(), re.M).group(1)
    return int(re.search(r"readLength: (\d+)", open(prof).read()).group(1))


def pass_reads(sess, paired):
    """The live reads of the last pass whose template lies inside its chain: (chain, tmpl_off) arrays."""
    n = sess.batch_slots
    chains, offs = [], []
    for m in range(2 if paired else 1):
        rows = np.frombuffer(sess.truth_reads(m, 0, n), dtype=READ_DT, count=n)
        ok = (rows["live"] != 0) & (rows["inside"] != 0)
        chains.append(rows["chain"][ok].astype(np.int64))
        offs.append(rows["tmpl_off"][ok].astype(np.int64))
    return np.concatenate(chains), np.concatenate(offs)


def model_counts(sess, L, table, paired):
    """[rows, 2] (alt, total) the label-level model gives the reads of the last pass.  Only a read with a table position
    within one base of its template is expanded into labels -- no other read can count -- and the model is given the
    pieces under the template and the rows near them, nothing else of the engine's."""
    counts = np.zeros((len(table), 2), dtype=np.int64)
    if not len(table):
        return counts, 0
    keys = np.array([(r[0] << 32) | r[2] for r in table], dtype=np.int64)
    chains, offs = pass_reads(sess, paired)
    expanded = 0
    for chain in np.unique(chains):
        pieces = sess.truth_pieces(int(chain))
        dst = np.array([p[0] for p in pieces], dtype=np.int64)
        clen = pieces[-1][0] + pieces[-1][2]
        near_rows = []                       # per piece: the table rows within one base of the piece's contig span
        spots = []
        for d, s, ln, c, kind, _ in pieces:
            if kind:
                near_rows.append((0, 0))
                continue
            lo = int(np.searchsorted(keys, (c << 32) | max(s - 1, 0), "left"))
            hi = int(np.searchsorted(keys, (c << 32) | (s + ln + 1), "right"))
            near_rows.append((lo, hi))
            for k in range(lo, hi):
                spots.append(d + (table[k][2] - s))
        if not spots:
            continue
        spots = np.unique(np.array(spots, dtype=np.int64))
        mine = offs[chains == chain]
        near = np.searchsorted(spots, mine + L + 1, "right") > np.searchsorted(spots, mine - 2, "left")
        codes = None
        for off in mine[near]:
            off = int(off)
            if codes is None:
                codes = sess.haplotype_codes(int(chain), 0, clen)
            first = int(np.searchsorted(dst, off, "right")) - 1
            last = int(np.searchsorted(dst, off + L - 1, "right")) - 1
            idx = sorted({k for q in range(first, last + 1) for k in range(*near_rows[q])})
            if not idx:
                continue
            got = vm.observe(pieces[first:last + 1], codes[off:off + L], off, L, [table[k] for k in idx])
            expanded += 1
            for r, (alt, total) in got.items():
                counts[idx[r], 0] += alt
                counts[idx[r], 1] += total
    return counts, expanded


# ---- the table the input files give ----
def abbr(name):
    i = name.find("chrom")
    if i >= 0:
        return name[i + 5:]
    i = name.find("chr")
    return name[i + 3:] if i >= 0 else name


def input_rows(cfg):
    """(kind, contig key, pos, population index, text) rows of the config's variation and SNP files, read the way the
    simulator reads them (the non-reference allele of a SNP row, complemented for the minus strand), and the config's
    population names."""
    text = open(cfg).read()
    popus = [p.strip() for p in re.search(r"^name = (.+)$", text, re.M).group(1).split(",")]
    rows = []
    m = re.search(r"^variation = (\S+)", text, re.M)
    if m:
        for ln in open(m.group(1)):
            f = ln.rstrip("\n").split("\t")
            if f[0] == "s":
                rows.append(("s", abbr(f[2]), int(f[3]), popus.index(f[1]), f[5]))
            elif f[0] in "id":
                rows.append((f[0], abbr(f[2]), int(f[3]), popus.index(f[1]), f[4]))
    m = re.search(r"^snp = (\S+)", text, re.M)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    if m:
        for ln in open(m.group(1)):
            f = ln.rstrip("\n").split("\t")
            a, b = f[3].split("/")
            ref = comp[f[5]] if f[4] == "-" else f[5]
            nuc = b if a == ref else a
            if f[4] == "-":
                nuc = comp[nuc]
            rows.append(("p", abbr(f[1]), int(f[2]), -1, nuc))
    return rows, popus


def read_file(path):
    """The rows of a .truth.variants.tsv file: (chrom, pos, type, allele, alt, total, populations)."""
    text = open(path).read()
    assert text.endswith("\n") and "\r" not in text
    lines = text[:-1].split("\n")
    assert lines[0] == HEADER
    rows = []
    for ln in lines[1:]:
        f = ln.split("\t")
        assert len(f) == 7 and re.fullmatch(r"\d+", f[1]) and re.fullmatch(r"\d+", f[4]) and re.fullmatch(r"\d+", f[5]) and f[2] in "spid", ln
        rows.append((f[0], int(f[1]), f[2], f[3], int(f[4]), int(f[5]), f[6]))
    return rows


# ---- the crowded case ----
CROWDED_LEN = (20000, 300)


def crowded_case(wd):
    """One 20 kb contig and one of 300 bases (A, C, G, T only), 75-base PE reads at coverage 30, two populations, and rows
    that stand as close to each other, to segment ends and to contig ends as the files allow."""
    os.makedirs(wd, exist_ok=True)
    fa = os.path.join(wd, "ref.fa")
    names = ["chr5", "chr6"]
    seqs = [synth.synth_contig(n, 31, i, n_runs=False).tobytes().upper() for i, n in enumerate(CROWDED_LEN)]
    cases._fasta_of(fa, [(n.encode(), s) for n, s in zip(names, seqs)])
    big, small = seqs

    def other(base, k=1):
        return "ACGT"[("ACGT".index(base) + k) % 4]

    def snv(popu, chrom, pos, zyg="homo", k=1):
        ref = chr((big if chrom == "chr5" else small)[pos - 1])
        return f"s\t{popu}\t{chrom}\t{pos}\t{ref}\t{other(ref, k)}\t{zyg}"

    LN = CROWDED_LEN[0]
    v = [
        # an SNV next to a deletion on both sides (999 is the deletion's anchor base)
        f"d\ta\tchr5\t1000\t5\thet", snv("a", "chr5", 999), snv("a", "chr5", 1005, "het"),
        # an SNV inside a het deletion
        f"d\ta\tchr5\t2000\t10\thet", snv("a", "chr5", 2004),
        # an insertion directly behind an SNV; two insertions at neighbouring positions
        snv("a", "chr5", 3000), f"i\ta\tchr5\t3000\tACGTA\thomo", f"i\ta\tchr5\t3500\tACG\thet", f"i\ta\tchr5\t3501\tTT\thomo",
        # a 3-copy CNV over several rows, a deletion at its (the segment's) first base
        f"c\ta\tchr5\t6001\t7000\t3\t2", f"d\ta\tchr5\t6001\t4\thomo", snv("a", "chr5", 6100, "het"), f"i\ta\tchr5\t6200\tGGC\thet",
        f"d\ta\tchr5\t6300\t6\thet", snv("a", "chr5", 6999),
        # a 3-copy segment shorter than a read: a template holds its sites more than once
        f"c\tb\tchr5\t9001\t9030\t3\t2", snv("b", "chr5", 9010), f"d\tb\tchr5\t9020\t2\thomo", f"i\tb\tchr5\t9025\tT\thomo",
        # a deletion that reaches the contig's end; SNVs on the contigs' first and last bases
        f"d\ta\tchr5\t{LN - 4}\t5\thet", snv("b", "chr5", LN), snv("a", "chr5", 1), snv("b", "chr6", 1), snv("a", "chr6", 300, "het"),
        snv("a", "chr6", 150), f"d\tb\tchr6\t100\t3\thet", f"i\tb\tchr6\t200\tCA\thomo",
        # one position, another allele in each population; one row in both
        snv("a", "chr5", 12000, "homo", 1), snv("b", "chr5", 12000, "homo", 2), snv("a", "chr5", 12500, "het"), snv("b", "chr5", 12500, "homo"),
        f"d\ta\tchr5\t14000\t3\thomo", f"d\tb\tchr5\t14000\t3\thet", f"d\tb\tchr5\t14000\t7\thet",
        f"i\ta\tchr5\t15000\tAC\thomo", f"i\tb\tchr5\t15000\tGT\thet", f"i\tb\tchr5\t15000\tGTT\thet",
    ]
    cases._write(os.path.join(wd, "variations.txt"), v)
    # a SNP row whose allele is the FASTA's base (the file's reference column names the other one), a SNP on an SNV's place
    fb = chr(big[13000 - 1])
    snp = cases._snps("chr5", LN, 400, 3) + cases._snps("chr6", CROWDED_LEN[1], 60, 4) + [
        f"rsF\tchr5\t13000\t{other(fb)}/{fb}\t+\t{other(fb)}",
        f"rsS\tchr5\t12000\t{chr(big[11999])}/{other(chr(big[11999]), 1)}\t+\t{chr(big[11999])}"]
    cases._write(os.path.join(wd, "snp.txt"), snp)
    cases._write(os.path.join(wd, "abundance.txt"), ["0.6\t0.4"])
    cfg = os.path.join(wd, "config.txt")
    cases._config(cfg, ref=fa, profile=os.path.join(cases.TESTDATA, cases.PROFILES["hs2000"]), variation=os.path.join(wd, "variations.txt"),
                  snp=os.path.join(wd, "snp.txt"), name="a, b", abundance=os.path.join(wd, "abundance.txt"), output=os.path.join(wd, "out"),
                  layout="PE", threads=1, verbose=0, coverage=30, insertSize=200)
    return cfg
