// tools/hap_check_fuzz.cpp -- the argument checks in front of the reference ingest and haplotype assembly kernels
// (simuscop_amd/csrc/sg_hap_check.h) against a brute-force restatement, for a sanitizer build on the CPU
// (tools/hap_check_sanitized.sh).  The restatement adds in 128 bits, where nothing wraps, and decides tiling by marking
// every byte of the (small) chains in an array: a list is legal when every byte is marked exactly once.  Hand-made cases
// for every clause with their legal neighbours, the values whose 64-bit sums wrap, then seeded random piece lists of
// which about half are legal -- that share is asserted, so refusing everything does not pass.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../simuscop_amd/csrc/sg_hap_check.h"

namespace chk = sg::hapcheck;
typedef unsigned __int128 u128;

namespace {

const uint64_t TOP = ~(uint64_t)0;   // 2^64 - 1
int failures = 0;

void expect(bool ok, const char* what, const std::string& detail = "") {
  if (ok) return;
  fprintf(stderr, "FAIL %s %s\n", what, detail.c_str());
  failures++;
}

// ---- the restatement -----------------------------------------------------------------------------------------------------
enum Why { LEGAL = 0, CHAIN, CONTIG, LITERAL, TILING, PATCH };

struct Build {
  std::vector<uint64_t> lens, contigs;
  std::vector<sg_hap_piece> pieces;
  std::vector<sg_hap_patch> patches;
  uint64_t n_lit = 0;
};

// the verdict of the rule, byte by byte; *at: the first piece (or patch) out of bounds
Why model(const Build& b, uint64_t* at, std::vector<std::vector<int>>* marks) {
  for (size_t i = 0; i < b.pieces.size(); i++) {
    const sg_hap_piece& p = b.pieces[i];
    *at = i;
    if (p.chain >= b.lens.size() || (u128)p.dst + p.len > b.lens[p.chain]) return CHAIN;
    if (p.kind == 0) {
      if (p.contig >= b.contigs.size() || (u128)p.src + p.len > b.contigs[p.contig]) return CONTIG;
    } else if ((u128)p.src + p.len > b.n_lit) {
      return LITERAL;
    }
  }
  marks->assign(b.lens.size(), std::vector<int>());
  for (size_t c = 0; c < b.lens.size(); c++) (*marks)[c].assign((size_t)b.lens[c], 0);   // (small chains only)
  for (const sg_hap_piece& p : b.pieces)
    for (uint32_t k = 0; k < p.len; k++) (*marks)[p.chain][(size_t)p.dst + k]++;
  for (const auto& m : *marks)
    for (int v : m)
      if (v != 1) return TILING;
  for (size_t i = 0; i < b.patches.size(); i++) {
    *at = i;
    if (b.patches[i].chain >= b.lens.size() || b.patches[i].dst >= b.lens[b.patches[i].chain]) return PATCH;
  }
  return LEGAL;
}

// the header's functions in the order sg_build_haplotypes calls them
chk::Verdict checked(const Build& b) {
  auto contig_length = [&](uint32_t k) { return b.contigs[k]; };
  const int32_t n = (int32_t)b.lens.size();
  for (size_t i = 0; i < b.pieces.size(); i++)
    if (auto v = chk::piece(b.pieces[i], i, n, b.lens.data(), contig_length, b.contigs.size(), b.n_lit)) return v;
  if (auto v = chk::tiling(n, b.lens.data(), b.pieces.data(), b.pieces.size())) return v;
  for (size_t i = 0; i < b.patches.size(); i++)
    if (auto v = chk::patch(b.patches[i], i, n, b.lens.data())) return v;
  return chk::Verdict();
}

bool has(const std::string& s, const std::string& part) { return s.find(part) != std::string::npos; }
uint64_t number_after(const std::string& s, const std::string& key) { return strtoull(s.c_str() + s.find(key) + key.size(), nullptr, 10); }

// both sides on one list; the message names what the restatement finds offending.  Returns the restatement's verdict.
Why compare(const Build& b, const char* what) {
  uint64_t at = 0;
  std::vector<std::vector<int>> marks;
  const Why w = model(b, &at, &marks);
  const chk::Verdict v = checked(b);
  const std::string d = std::string(what) + ": code " + std::to_string(v.code) + " '" + v.msg + "', restatement " + std::to_string((int)w);
  if (w == LEGAL) { expect(v.code == SG_OK && v.msg.empty(), "legal list refused", d); return w; }
  expect(v.code == SG_ERR_INVALID, "illegal list: code", d);
  if (v.code == SG_OK) return w;
  const std::string piece_at = "piece " + std::to_string(at) + " ", patch_at = "patch " + std::to_string(at) + " ";
  if (w == CHAIN) expect(has(v.msg, piece_at + "falls outside its chain"), "message", d);
  if (w == CONTIG) expect(has(v.msg, piece_at + "falls outside its contig"), "message", d);
  if (w == LITERAL) expect(has(v.msg, piece_at + "falls outside the literal bytes"), "message", d);
  if (w == PATCH) expect(has(v.msg, patch_at + "falls outside its chain"), "message", d);
  if (w == TILING) {
    if (has(v.msg, "overlaps")) {           // the named piece holds a byte that is marked twice
      const sg_hap_piece& p = b.pieces[number_after(v.msg, "piece ")];
      bool twice = false;
      for (uint32_t k = 0; k < p.len; k++) twice |= marks[p.chain][(size_t)p.dst + k] > 1;
      expect(twice && p.chain == number_after(v.msg, "chain "), "overlap names a piece without one", d);
    } else if (has(v.msg, "leave a gap in front of piece")) {   // the byte in front of the named piece is unmarked
      const sg_hap_piece& p = b.pieces[number_after(v.msg, "front of piece ")];
      expect(p.len && p.dst > 0 && marks[p.chain][(size_t)p.dst - 1] == 0 && p.chain == number_after(v.msg, "chain "), "gap names a piece without one", d);
    } else {                                // the named chain has an unmarked byte
      expect(has(v.msg, "do not add up to its length"), "message", d);
      const uint64_t c = number_after(v.msg, "chain ");
      bool unmarked = false;
      if (c < marks.size())
        for (int m : marks[c]) unmarked |= m == 0;
      expect(unmarked, "names a chain that is covered", d);
    }
  }
  return w;
}

sg_hap_piece P(uint64_t dst, uint64_t src, uint32_t len, uint32_t chain, uint32_t contig = 0, uint32_t kind = 0) {
  sg_hap_piece p;
  p.dst = dst; p.src = src; p.len = len; p.chain = chain; p.contig = contig; p.kind = kind;
  return p;
}
sg_hap_patch Q(uint64_t dst, uint32_t chain) {
  sg_hap_patch q;
  q.dst = dst; q.chain = chain; q.base = 'A';
  return q;
}
sg_contig K(uint64_t raw, uint64_t len, uint32_t lb, uint32_t lw) {
  sg_contig k;
  k.raw_offset = raw; k.length = len; k.line_bases = lb; k.line_width = lw;
  return k;
}

void want(Why w, const Build& b, const char* what) { expect(compare(b, what) == w, "the restatement's own verdict", what); }

// ---- hand-made: every clause with its legal neighbour, the wrapping values ---------------------------------------------------
void hand_made() {
  Build ok;
  ok.lens = {10, 0, 1};
  ok.contigs = {20, 5};
  ok.n_lit = 4;
  ok.pieces = {P(0, 15, 5, 0), P(5, 1, 3, 0, 0, 1), P(8, 3, 2, 0, 1), P(0, 3, 1, 2, 0, 1)};
  ok.patches = {Q(0, 0), Q(9, 0), Q(0, 2)};
  want(LEGAL, ok, "legal: source ranges reach the last base and the last literal byte");
  Build b = ok;
  b.pieces[2] = P(8, 3, 3, 0, 1);       want(CHAIN, b, "piece past its chain by one");
  b = ok; b.pieces[0] = P(0, 16, 5, 0);  want(CONTIG, b, "piece past its contig by one");
  b = ok; b.pieces[1] = P(5, 2, 3, 0, 0, 1);   want(LITERAL, b, "piece past the literals by one");
  b = ok; b.pieces[3].chain = 3;         want(CHAIN, b, "chain index out of range");
  b = ok; b.pieces[2].contig = 2;        want(CONTIG, b, "contig index out of range");
  b = ok; b.pieces[3].contig = 99;       want(LEGAL, b, "a literal piece's contig field is not read");
  b = ok; b.patches[1] = Q(10, 0);       want(PATCH, b, "patch at lens[c]");
  b = ok; b.patches[1] = Q(0, 1);        want(PATCH, b, "patch on an empty chain");
  b = ok; b.patches[1] = Q(0, 3);        want(PATCH, b, "patch's chain out of range");
  b = ok; b.patches[1] = Q(TOP, 0);      want(PATCH, b, "patch at 2^64 - 1");
  // wrapping sums
  b = ok; b.pieces[3] = P(TOP, 3, 1, 2, 0, 1);           want(CHAIN, b, "dst = 2^64 - 1, len 1");
  b = ok; b.pieces[0] = P(TOP - 4, 15, 5, 0);            want(CHAIN, b, "dst = 2^64 - len");
  b = ok; b.pieces[0] = P(0, TOP - 4, 5, 0);             want(CONTIG, b, "contig src = 2^64 - len");
  b = ok; b.pieces[0] = P(0, TOP, 5, 0);                 want(CONTIG, b, "contig src = 2^64 - 1");
  b = ok; b.pieces[1] = P(5, TOP - 2, 3, 0, 0, 1);       want(LITERAL, b, "literal src = 2^64 - len");
  b = ok; b.pieces[1] = P(5, TOP, 3, 0, 0, 1);           want(LITERAL, b, "literal src = 2^64 - 1");
  b = ok; b.lens[1] = 0; b.pieces.push_back(P(TOP, 0, 1, 1)); want(CHAIN, b, "dst + len == 2^64 on an empty chain");
  // tiling
  b = ok; b.pieces.pop_back();                           want(TILING, b, "a chain without pieces");
  b = ok; b.pieces[1].len = 2;                           want(TILING, b, "adds up short");
  b = ok; b.pieces[2] = P(7, 2, 3, 0, 1);                want(TILING, b, "adds up over");
  Build t;
  t.lens = {20};
  t.contigs = {20};
  t.pieces = {P(0, 0, 8, 0), P(5, 0, 7, 0), P(15, 0, 5, 0)};   // [0,8) [5,12) [15,20): 3 twice, 3 never, sum 20
  want(TILING, t, "overlap and gap of equal size");
  std::swap(t.pieces[0], t.pieces[2]);                   want(TILING, t, "the same, shuffled");
  std::swap(t.pieces[0], t.pieces[1]);                   want(TILING, t, "the same, shuffled again");
  t.pieces = {P(0, 0, 5, 0), P(15, 0, 5, 0), P(5, 0, 7, 0), P(8, 0, 7, 0)};   // gap [12,15) closed late, overlap [8,12)... sum 24
  want(TILING, t, "overlap in an unordered list");
  t.pieces = {P(12, 0, 8, 0), P(0, 0, 5, 0), P(5, 0, 7, 0)};   want(LEGAL, t, "a legal list out of order");
  t.pieces = {P(0, 0, 10, 0), P(0, 0, 10, 0)};           want(TILING, t, "the same piece twice");
  t.pieces = {P(0, 0, 0, 0), P(0, 0, 12, 0), P(7, 0, 0, 0), P(12, 0, 8, 0), P(20, 0, 0, 0)};
  want(LEGAL, t, "pieces of length 0 at a chain's start, middle and end");
  t.pieces.push_back(P(21, 0, 0, 0));                    want(CHAIN, t, "a piece of length 0 behind the chain's end");
  Build e;
  e.lens = {0, 0};
  want(LEGAL, e, "chains of length 0 without pieces, no contigs");
  e.lens.clear();
  want(LEGAL, e, "no chains");
  e.pieces = {P(0, 0, 0, 0)};                            want(CHAIN, e, "a piece without any chain");

  // ---- sg_reference_chunk ----
  expect(!chk::chunk(true, 100, 0, 100), "chunk: the whole image");
  expect(!chk::chunk(true, 100, 100, 0), "chunk: nothing at the end");
  expect(!chk::chunk(true, 0, 0, 0), "chunk: nothing of nothing");
  expect(!!chk::chunk(true, 100, 1, 100), "chunk: past the end by one");
  expect(!!chk::chunk(true, 100, 101, 0), "chunk: nothing behind the end");
  expect(!!chk::chunk(false, 100, 0, 1), "chunk: before begin");
  expect(!!chk::chunk(true, 100, TOP, 1), "chunk: offset + bytes == 2^64");
  expect(!!chk::chunk(true, 100, TOP - 49, 50), "chunk: offset = 2^64 - bytes");
  expect(!!chk::chunk(true, 100, 50, TOP - 49), "chunk: bytes = 2^64 - offset");
  expect(!!chk::chunk(true, TOP, TOP, 1), "chunk: image of 2^64 - 1 bytes, one past it");
  expect(!chk::chunk(true, TOP, TOP - 1, 1), "chunk: image of 2^64 - 1 bytes, its last byte");
  {
    const chk::Verdict v = chk::chunk(true, 100, TOP, 1);
    expect(v.code == SG_ERR_INVALID && v.msg == "sg_reference_chunk: range outside sg_reference_begin's size", "chunk: code and text");
  }
  // ---- call order ----
  expect(!chk::need_image(true, "sg_reference_scan"), "scan after begin");
  expect(chk::need_image(false, "sg_reference_scan").msg == "sg_reference_scan: call sg_reference_begin first", "scan before begin");
  expect(chk::need_image(false, "sg_reference_commit").msg == "sg_reference_commit: call sg_reference_begin first" &&
             chk::need_image(false, "sg_reference_commit").code == SG_ERR_INVALID, "commit before begin");
  expect(!chk::need_contigs(false, 0) && !chk::need_contigs(true, 5), "build: nothing to copy, or contigs committed");
  expect(chk::need_contigs(false, 1).msg == "sg_build_haplotypes: call sg_reference_commit first", "build before commit");
  // ---- sg_reference_commit: one contig ----
  // 130 bases in lines of 60 + 1: 2 breaks inside, extent 132
  expect(!chk::contig(K(10, 130, 60, 61), 0, 142), "contig ending exactly at the image's end");
  expect(has(chk::contig(K(10, 130, 60, 61), 3, 141).msg, "contig 3 runs past the end of the file"), "contig past the image by one");
  expect(!chk::contig(K(10, 120, 60, 61), 0, 131), "a full last line: its break is not part of the extent");
  expect(!!chk::contig(K(10, 120, 60, 61), 0, 130), "a full last line, one byte short");
  expect(!chk::contig(K(10, 120, 60, 62), 0, 132) && !!chk::contig(K(10, 120, 60, 62), 0, 131), "two-byte breaks");
  expect(!chk::contig(K(7, 0, 0, 0), 0, 7) && !chk::contig(K(0, 0, 0, 0), 0, 0), "an empty contig needs no line shape");
  expect(!!chk::contig(K(8, 0, 0, 0), 0, 7), "an empty contig behind the image's end");
  expect(has(chk::contig(K(0, 1, 0, 1), 2, 100).msg, "contig 2 has an impossible line shape"), "line_bases 0");
  expect(has(chk::contig(K(0, 1, 5, 4), 0, 100).msg, "impossible line shape"), "line_width < line_bases");
  expect(!chk::contig(K(0, 5, 5, 5), 0, 5), "line_width == line_bases");
  expect(chk::contig(K(0, 0xFFFFFFF1ull, 60, 61), 0, TOP).code == SG_ERR_UNSUPPORTED, "longer than the 32-bit limit");
  expect(!chk::contig(K(0, 0xFFFFFFF0ull, 60, 61), 0, TOP), "at the 32-bit limit");
  expect(!!chk::contig(K(TOP - 129, 130, 60, 61), 0, 1000), "raw_offset = 2^64 - length");
  expect(!!chk::contig(K(TOP - 131, 130, 60, 61), 0, 1000), "raw_offset + extent == 2^64");
  expect(!!chk::contig(K(TOP, 1, 1, 1), 0, 1000), "raw_offset = 2^64 - 1");
  expect(!!chk::contig(K(100, 0xFFFFFFF0ull, 1, 0xFFFFFFFFu), 0, 1000), "an extent near 2^64");
  // ---- sg_haplotype_codes ----
  const uint64_t cl[2] = {10, 0};
  expect(!chk::codes(true, cl, 2, 0, 0, 10) && !chk::codes(true, cl, 2, 0, 10, 0) && !chk::codes(true, cl, 2, 1, 0, 0), "codes: legal ranges");
  expect(chk::codes(true, cl, 2, 0, 1, 10).msg == "sg_haplotype_codes: range past the end of the chain", "codes: past the end by one");
  expect(!!chk::codes(true, cl, 2, 0, 11, 0) && !!chk::codes(true, cl, 2, 1, 0, 1), "codes: behind the end");
  expect(chk::codes(true, cl, 2, 2, 0, 0).msg == "sg_haplotype_codes: chain index out of range", "codes: chain out of range");
  expect(chk::codes(false, nullptr, 0, 0, 0, 0).msg == "sg_haplotype_codes: no haplotypes on the device", "codes: before any chains");
  expect(!!chk::codes(true, cl, 2, 0, TOP, 1) && !!chk::codes(true, cl, 2, 0, TOP - 4, 5) && !!chk::codes(true, cl, 2, 0, 5, TOP - 4),
         "codes: offset + n == 2^64");
}

// ---- random --------------------------------------------------------------------------------------------------------------
void random_ranges(std::mt19937_64& rng, int n) {
  auto value = [&]() -> uint64_t {   // small, or near 2^64, or anything
    switch (rng() % 4) {
      case 0: return rng() % 200;
      case 1: return TOP - rng() % 200;
      case 2: return rng();
      default: return rng() % 8;
    }
  };
  long legal = 0;
  for (int it = 0; it < n; it++) {
    const uint64_t off = value(), len = value(), limit = value();
    const bool w = (u128)off + len <= limit;
    legal += w;
    expect(chk::in_range(off, len, limit) == w, "in_range");
    expect(!chk::chunk(true, limit, off, len) == w, "chunk");
    const uint64_t cl[1] = {limit};
    expect(!chk::codes(true, cl, 1, 0, off, len) == w, "codes");
    // a contig: the extent in 128 bits
    const uint32_t lb = (uint32_t)(rng() % 3 ? rng() % 70 : rng()), lw = lb + (uint32_t)(rng() % 4 ? rng() % 3 : rng() % 1000) - (rng() % 16 == 0);
    const uint64_t length = rng() % 3 ? rng() % 300 : (rng() % 2 ? rng() % 0x180000000ull : 0xFFFFFFF0ull - rng() % 3);
    const sg_contig k = K(off, length, lb, lw);
    int wcode = SG_OK;
    if (length && (lb == 0 || lw < lb)) wcode = SG_ERR_INVALID;
    else if (length > 0xFFFFFFF0ull) wcode = SG_ERR_UNSUPPORTED;
    else {
      const u128 extent = (u128)length + (length ? (u128)((length - 1) / lb) * (lw - lb) : 0);
      if ((u128)off + extent > limit) wcode = SG_ERR_INVALID;
    }
    expect(chk::contig(k, 0, limit).code == wcode, "contig", std::to_string(off) + " " + std::to_string(length) + " " + std::to_string(lb) + " " + std::to_string(lw) + " in " + std::to_string(limit));
  }
  expect(legal > n / 10 && legal < n - n / 10, "random ranges: both verdicts occur");
}

long random_lists(std::mt19937_64& rng, int n) {
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  long legal = 0;
  for (int it = 0; it < n; it++) {
    Build b;
    const int n_chains = (int)pick(1, 3);
    for (int c = 0; c < n_chains; c++) b.lens.push_back(rng() % 6 == 0 ? 0 : pick(1, 64));
    for (int c = (int)pick(1, 3); c > 0; c--) b.contigs.push_back(pick(1, 80));
    b.n_lit = pick(0, 40);
    // a legal tiling: cuts at random places, now and then a piece of length 0, sources that fit
    size_t budget = 12;
    for (int c = 0; c < n_chains; c++) {
      uint64_t at = 0;
      const size_t share = budget / (size_t)(n_chains - c);
      size_t used = 0;
      while (at < b.lens[c] || (used < share && rng() % 8 == 0)) {
        const bool last = used + 1 >= share;
        uint64_t len = at < b.lens[c] ? (last ? b.lens[c] - at : pick(rng() % 5 == 0 ? 0 : 1, b.lens[c] - at)) : 0;
        const uint32_t kind = (uint32_t)(rng() & 1), contig = (uint32_t)(rng() % b.contigs.size());
        uint64_t room = kind ? b.n_lit : b.contigs[contig];
        if (len > room) len = last ? len : room;           // (a last piece longer than its source: an illegal list, so be it)
        const uint64_t src = len <= room ? pick(0, room - len) : 0;
        b.pieces.push_back(P(at, src, (uint32_t)len, (uint32_t)c, contig, kind));
        at += len;
        used++;
        if (used >= share) break;
      }
      budget -= used;
    }
    for (int q = (int)pick(0, 3); q > 0; q--) {
      const uint32_t c = (uint32_t)(rng() % n_chains);
      if (b.lens[c]) b.patches.push_back(Q(pick(0, b.lens[c] - 1), c));
    }
    if (rng() % 2)   // out of order: the sorting path
      for (size_t i = b.pieces.size(); i > 1; i--) std::swap(b.pieces[i - 1], b.pieces[rng() % i]);
    if (rng() % 2 && !b.pieces.empty()) {   // one thing wrong (now and then a change that leaves the list legal)
      sg_hap_piece& p = b.pieces[rng() % b.pieces.size()];
      switch (rng() % 10) {
        case 0: p.dst += pick(1, 3); break;
        case 1: p.dst -= p.dst ? pick(1, p.dst < 3 ? p.dst : 3) : 0; break;
        case 2: p.len += (uint32_t)pick(1, 3); break;
        case 3: p.len -= p.len ? 1 : 0; break;
        case 4: b.pieces.push_back(p); break;
        case 5: p = b.pieces.back(); b.pieces.pop_back(); break;
        case 6: p.dst = rng() % 2 ? TOP : TOP - p.len + 1; break;
        case 7: p.src = rng() % 2 ? TOP : TOP - p.len + 1; break;
        case 8: (rng() % 2 ? p.chain : p.contig) += (uint32_t)pick(1, 3); break;
        default: {   // an overlap here, a gap of the same size there: the sum stays right
          sg_hap_piece& q = b.pieces[rng() % b.pieces.size()];
          if (&q != &p && q.chain == p.chain && p.len > 1 && q.len > 1) { p.len--; q.len++; if (rng() % 2) q.dst--; }
          else if (!b.patches.empty()) b.patches[0].dst = b.lens[b.patches[0].chain];
        }
      }
    }
    legal += compare(b, "random list") == LEGAL;
  }
  return legal;
}

}  // namespace

int main(int argc, char** argv) {
  const int n_lists = argc > 1 ? atoi(argv[1]) : 4000;
  std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 12345);
  hand_made();
  random_ranges(rng, 20000);
  const long legal = random_lists(rng, n_lists);
  printf("hap_check_fuzz: %d random lists, %ld legal by the byte-marking restatement, %d failures\n", n_lists, legal, failures);
  if (legal * 10 < (long)n_lists * 3 || legal * 10 > (long)n_lists * 7) {
    fprintf(stderr, "FAIL the share of legal lists is not about a half\n");
    return 1;
  }
  if (failures) return 1;
  printf("hap_check_fuzz: every verdict as the restatement has it\n");
  return 0;
}
