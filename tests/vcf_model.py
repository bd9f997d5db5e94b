"""The VCF of known variants as the reference's parser reads it, in plain Python (test infrastructure).

Written from lib/vcfparser/vcfparser.cpp:26-106 and the statement of the rule that asked for the device reader, not from the
product's code: the parser reads with fgets(buf, 20000), so its unit is a FRAGMENT of at most 19,999 bytes (or through the
line break), numbered from 1; a fragment is a C string (a NUL byte ends it); '#' first: skipped; ten tab-separated fields,
the tenth keeping the rest (fewer: malformed); the first "DP=" in INFO with atoi below 10: skipped; (float)atof(QUAL) <
20.0f: skipped; abbr_of_chr(CHROM) looked up among the contig keys; atol(POS); the genotype is field 10 up to its first ':'
and the row is heterozygous iff it is exactly "1/1"; strlen(REF) > 1: deletion (pos + 1, strlen(REF) - 1), else strlen(ALT) >
1: insertion (pos, strlen(ALT) - 1), else SNV (pos, first byte of ALT or 0, homo flag); every such row is counted, one on a
known contig is kept, kept rows stay in file order.

`row` is the exact verdict on any bytes.  `decided` says whether the text is made of the forms a device may decide itself;
the others (exponents, inf / nan / hex, over-long digit strings, white space in front of a number, a NUL byte) are the
ones it must hand back -- looked at in the parser's order, so a fragment DP has skipped is not undecided for its QUAL."""
import random
import re

import numpy as np

FRAG = 19999
HOMO, KNOWN = 1, 2
KEYS = [b"1", b"20", b"X", b"2"]

_SPACE = b" \t\n\v\f\r"
_INT = re.compile(rb"[ \t\n\v\f\r]*([+-]?)(\d*)")
_DEC = re.compile(rb"[ \t\n\v\f\r]*([+-]?)(?:(inf(?:inity)?|nan(?:\([0-9A-Za-z_]*\))?)|(0[xX](?:[0-9a-fA-F]+\.?[0-9a-fA-F]*|\.[0-9a-fA-F]+)(?:[pP][+-]?\d+)?)"
                  rb"|((?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?))", re.I)


def fragments(text):
    """What successive fgets(buf, 20000) calls return on `text`."""
    out, p = [], 0
    while p < len(text):
        nl = text.find(b"\n", p)
        end = len(text) if nl < 0 else nl + 1
        for a in range(p, end, FRAG):
            out.append(text[a:min(a + FRAG, end)])
        p = end
    return out


def c_strtol(s, bits):
    m = _INT.match(s)
    v = int(m.group(2) or b"0")
    v = -v if m.group(1) == b"-" else v
    return max(-(1 << (bits - 1)), min((1 << (bits - 1)) - 1, v))


def c_atoi(s):
    v = c_strtol(s, 64) & 0xFFFFFFFF   # (int)strtol(...)
    return v - (1 << 32) if v >> 31 else v


def c_atof(s):
    m = _DEC.match(s)
    if not m:
        return 0.0
    sign = -1.0 if m.group(1) == b"-" else 1.0
    if m.group(2):
        return sign * float(m.group(2)[:3].decode())
    if m.group(3):
        h = m.group(3).decode()
        return sign * float.fromhex(h if "p" in h.lower() else h + "p0")
    return sign * float(m.group(4).decode())


def abbr_of_chr(name):
    i = name.find(b"chrom")
    if i >= 0:
        return name[i + 5:]
    i = name.find(b"chr")
    return name[i + 3:] if i >= 0 else name


def row(frag, keys=KEYS):
    """(kind, pos, contig, value, flags) of one fragment: kind "skip" / "malformed" / "snv" / "ins" / "del"; the values of a
    skipped or malformed fragment are 0.  contig is the key's index (0 with KNOWN clear when the contig is unknown)."""
    s = frag.split(b"\0", 1)[0]
    if s[:1] == b"#":
        return ("skip", 0, 0, 0, 0)
    f = s.split(b"\t", 9)
    if len(f) < 10:
        return ("malformed", 0, 0, 0, 0)
    dp = f[7].find(b"DP=")
    if dp >= 0:
        semi = f[7].find(b";", dp)
        if c_atoi(f[7][dp + 3:semi if semi >= 0 else None]) < 10:
            return ("skip", 0, 0, 0, 0)
    if np.float32(c_atof(f[5])) < np.float32(20.0):
        return ("skip", 0, 0, 0, 0)
    chrom = abbr_of_chr(f[0])
    pos = c_strtol(f[1], 64)
    het = f[9].split(b":", 1)[0] == b"1/1"
    contig, flags = (keys.index(chrom), KNOWN) if chrom in keys else (0, 0)
    if len(f[3]) > 1:
        return ("del", pos + 1, contig, len(f[3]) - 1, flags)
    if len(f[4]) > 1:
        return ("ins", pos, contig, len(f[4]) - 1, flags)
    alt = f[4][0] if f[4] else 0
    return ("snv", pos, contig, alt - 256 if alt > 127 else alt, flags | (0 if het else HOMO))


def _int_decided(s, digits):
    if s[:1] and s[:1] in _SPACE:
        return False
    m = re.match(rb"[+-]?(\d*)", s)
    return len(m.group(1)) <= digits


def _qual_decided(s):
    if s[:1] and s[:1] in _SPACE:
        return False
    m = re.match(rb"[+-]?(\d+\.?\d*|\.\d+)?", s)
    num, rest = m.group(1), s[m.end():]
    if num is None:
        return rest[:1].lower() not in (b"i", b"n")
    return sum(c in b"0123456789" for c in num) <= 15 and rest[:1].lower() not in (b"e", b"x", b"p")


def decided(frag):
    """False when the fragment holds a form the device must hand back."""
    if frag[:1] == b"#":
        return True
    if b"\0" in frag:
        return False
    f = frag.split(b"\t", 9)
    if len(f) < 10:
        return True
    dp = f[7].find(b"DP=")
    if dp >= 0:
        semi = f[7].find(b";", dp)
        v = f[7][dp + 3:semi if semi >= 0 else None]
        if not _int_decided(v, 9):
            return False
        if c_atoi(v) < 10:
            return True
    if not _qual_decided(f[5]):
        return False
    if np.float32(c_atof(f[5])) < np.float32(20.0):
        return True
    return _int_decided(f[1], 18)


def parse(text, keys=KEYS):
    """The whole file: fragments, the three counts, kept rows per kind as (fragment number, pos, contig, value, flags), the
    numbers of the malformed fragments and of those a device hands back."""
    out = {"fragments": 0, "n": {"snv": 0, "ins": 0, "del": 0}, "rows": {"snv": [], "ins": [], "del": []}, "malformed": [], "undecided": []}
    for no, frag in enumerate(fragments(text), 1):
        out["fragments"] = no
        kind, pos, contig, value, flags = row(frag, keys)
        if not decided(frag):
            out["undecided"].append(no)
        if kind == "malformed":
            out["malformed"].append(no)
        elif kind != "skip":
            out["n"][kind] += 1
            if flags & KNOWN:
                out["rows"][kind].append((no, pos, contig, value, flags))
    return out


# ---- inputs ----
def mk(chrom=b"chr20", pos=b"1000", ref=b"A", alt=b"C", qual=b"50", info=b"DP=30", fmt=b"GT:AD", sample=b"0/1:3,4", end=b"\n", ident=b"."):
    return b"\t".join([chrom, pos, ident, ref, alt, qual, b"PASS", info, fmt, sample]) + end


S = ("skip", 0, 0, 0, 0)
M = ("malformed", 0, 0, 0, 0)
SNV = ("snv", 1000, 1, ord("C"), KNOWN | HOMO)
# One hand-made fragment per clause of the rule: (fragment, the exact verdict written out, decided on the device?)
CLAUSES = [
    (b"##fileformat=VCFv4.2\n", S, True), (b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n", S, True),
    (b"\t".join([b"chr20", b"1000", b".", b"A", b"C", b"50", b"PASS", b"DP=30", b"GT"]) + b"\n", M, True),        # nine fields
    (mk(), SNV, True),                                                                                         # ten
    (b"\n", M, True),                                                                                          # an empty line is one field
    (mk(info=b"DP=9"), S, True), (mk(info=b"DP=10"), SNV, True), (mk(info=b"DP=."), S, True),
    (mk(info=b"ADP=3;DP=50"), S, True), (mk(info=b"AF=0.5;DP="), S, True), (mk(info=b"AF=0.5"), SNV, True),
    (mk(info=b"AF=0.5;DP=50;MQ=60"), SNV, True), (mk(info=b"DP=-12"), S, True),
    (mk(qual=b"19.999999"), S, True), (mk(qual=b"19.9999999"), SNV, True), (mk(qual=b"20"), SNV, True), (mk(qual=b"."), S, True),
    (mk(qual=b"-0"), S, True), (mk(qual=b"1e3"), SNV, False), (mk(qual=b"20.5abc"), SNV, True), (mk(qual=b".5"), S, True),
    (mk(qual=b"19."), S, True), (mk(qual=b"+21"), SNV, True), (mk(qual=b"-21"), S, True), (mk(qual=b"PASS"), S, True),
    (mk(chrom=b"chr20"), SNV, True), (mk(chrom=b"20"), SNV, True), (mk(chrom=b"chrom20"), SNV, True),
    (mk(chrom=b"chrUn"), ("snv", 1000, 0, ord("C"), HOMO), True), (mk(chrom=b"scaffold_chrX"), ("snv", 1000, 2, ord("C"), KNOWN | HOMO), True),
    (mk(chrom=b"200"), ("snv", 1000, 0, ord("C"), HOMO), True), (mk(chrom=b"2"), ("snv", 1000, 3, ord("C"), KNOWN | HOMO), True),
    (mk(sample=b"1/1:9,9"), ("snv", 1000, 1, ord("C"), KNOWN), True),                                        # "1/1" is filed as heterozygous
    (mk(fmt=b"GT", sample=b"1/1"), SNV, True),                                                                # "1/1\n" is not "1/1"
    (mk(sample=b"1|1:9,9"), SNV, True), (mk(sample=b"0/1:9,9"), SNV, True),
    (mk(fmt=b"GT", sample=b"1/1", end=b""), ("snv", 1000, 1, ord("C"), KNOWN), True),                        # the end of the text, no line break
    (mk(fmt=b"GT", sample=b"1/1\t0/1"), SNV, True),                                                           # a second sample column, no ':'
    (mk(ref=b"ACG", alt=b"AT"), ("del", 1001, 1, 2, KNOWN), True), (mk(ref=b"A", alt=b"ACGT"), ("ins", 1000, 1, 3, KNOWN), True),
    (mk(alt=b""), ("snv", 1000, 1, 0, KNOWN | HOMO), True), (mk(ref=b"", alt=b"G"), ("snv", 1000, 1, ord("G"), KNOWN | HOMO), True),
    (mk(pos=b"-5"), ("snv", -5, 1, ord("C"), KNOWN | HOMO), True), (mk(pos=b"12x"), ("snv", 12, 1, ord("C"), KNOWN | HOMO), True),
    (mk(pos=b"x"), ("snv", 0, 1, ord("C"), KNOWN | HOMO), True), (mk(pos=b"123456789012345678"), ("snv", 123456789012345678, 1, ord("C"), KNOWN | HOMO), True),
    (mk(end=b"\r\n"), SNV, True), (mk(fmt=b"GT", sample=b"1/1", end=b"\r\n"), SNV, True),                      # CR LF: "1/1\r\n"
    # every form the device hands back, with what the parser makes of it
    (mk(qual=b"1E+2"), SNV, False), (mk(qual=b"inf"), SNV, False), (mk(qual=b"nan"), SNV, False), (mk(qual=b"-Infinity"), S, False),
    (mk(qual=b"0x1p5"), SNV, False), (mk(qual=b"0000000000000050"), SNV, False), (mk(qual=b" 50"), SNV, False), (mk(qual=b"5.e1"), SNV, False),
    (mk(pos=b"1234567890123456789"), ("snv", 1234567890123456789, 1, ord("C"), KNOWN | HOMO), False), (mk(pos=b" 1000"), SNV, False),
    (mk(info=b"DP=0000000030"), SNV, False), (mk(info=b"DP= 30"), SNV, False), (mk(info=b"DP=3000000000"), S, False),
    (mk(ident=b"a\0b"), M, False), (mk(sample=b"1/1\0:2"), ("snv", 1000, 1, ord("C"), KNOWN), False),
    (mk(info=b"DP=5", qual=b"1e3"), S, True), (mk(qual=b"1", pos=b" 7"), S, True),                           # skipped before the odd field is read
]


def clause_text():
    """The clause fragments as one file (those without a line break get one, but the last)."""
    frs = [f if f.endswith(b"\n") else f + b"\n" for f, _, _ in CLAUSES]
    return b"".join(frs) + mk(fmt=b"GT", sample=b"1/1", end=b"")


_CHROMS = [b"chr1", b"1", b"chr20", b"20", b"chrom20", b"chrX", b"X", b"chr2", b"chr9", b"chrUn_x", b"", b"chr", b"chr200", b"c"]
_QUALS = [b"50", b"19.9", b"20", b"20.0", b"19.999999", b"19.9999999", b"19.9999990463256", b"19.9999990463257", b".", b"", b"-3", b"+30.25",
          b"999", b"0", b"7.5", b"100.000", b"PASS", b"q", b"19", b"21"]
_INFOS = [b"DP=30", b"DP=9", b"DP=10", b"AF=0.5;DP=25;MQ=60", b"ADP=3;DP=50", b"DP=", b".", b"AF=1", b"XDP=44;Q=1", b"DP=+11", b"DP=-1", b"DP=12x;DP=1",
          b"AC=2;AN=2;DP=100;FS=0.0;MQ=60.00;QD=25.3", b"D=1;P=2", b"DP=007"]
_GTS = [b"0/1:3,4", b"1/1:9,9", b"1/1", b"1|1:1", b"0/1", b"./.:0", b"1/1:", b"1/10:2", b"1/1\t0/1", b":1/1", b""]
_ALLELES = [b"A", b"C", b"G", b"T", b"AC", b"ACGT", b"", b"N", b"<DEL>", b"G,T", b"\xc3"]


def random_line(rng, odd=0.0):
    """One line of decided forms; with probability `odd`, one with fewer fields, an empty one or a '#' line."""
    r = rng.random()
    if r < odd / 3:
        return b"\t".join([b"chr1", b"5", b"."] * rng.randrange(0, 3)) + b"\n"
    if r < 2 * odd / 3:
        return b"#" + bytes(rng.choice(b"ab\tc") for _ in range(rng.randrange(0, 30))) + b"\n"
    if r < odd:
        return b"\n"
    pos = rng.choice([b"%d" % rng.randrange(0, 10 ** rng.randrange(1, 10)), b"-4", b"+9", b"x1", b"", b"12a"])
    return mk(rng.choice(_CHROMS), pos, rng.choice(_ALLELES), rng.choice(_ALLELES), rng.choice(_QUALS), rng.choice(_INFOS),
              rng.choice([b"GT", b"GT:AD", b"."]), rng.choice(_GTS), rng.choice([b"\n", b"\n", b"\n", b"\r\n"]))


def random_text(seed, n_lines, odd=0.0, final_break=True):
    rng = random.Random(seed)
    t = b"".join(random_line(rng, odd) for _ in range(n_lines))
    return t if final_break or not t else t[:-1]


def long_header_text():
    """A #CHROM line of thousands of sample names, longer than 19,999 bytes, whose tail has ten fields and parses as a row
    (the second fragment starts inside the names), then two rows."""
    head = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"
    names = []
    while len(head) + sum(len(n) + 1 for n in names) < 52000:
        names.append(b"HG%05d" % len(names))
    # the fragment that starts at byte 19999 must look like a row: put the right fields there
    line = head + b"\t" + b"\t".join(names)
    row_like = b"chr20\t77\t.\tA\tG\t60\tPASS\tDP=40\tGT\t"
    line = line[:FRAG] + row_like + line[FRAG + len(row_like):]
    return b"##x\n" + line + b"\n" + mk() + mk(chrom=b"chr1", pos=b"5")
