// sg_hap_check.h -- the argument checks in front of the reference ingest and haplotype assembly kernels
// (sg_api_haplotypes.cpp calls them; sg_haplotypes.hip trusts them).  Plain functions over the public structs of
// simuscop_amd.h, a code and a message each; no HIP header is reached from here, so tools/hap_check_fuzz.cpp runs them on
// the CPU under the sanitizers against a byte-marking restatement.
//
// Every "range inside limit" test has the form  len <= limit && off <= limit - len  (in_range): no sum is formed that
// could wrap at 2^64.  The tiling of a chain is checked as tiling, not as a sum of lengths.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "simuscop_amd.h"

namespace sg {
namespace hapcheck {

struct Verdict {
  int code = SG_OK;
  std::string msg;
  explicit operator bool() const { return code != SG_OK; }   // true: refused
};
inline Verdict refuse(int code, std::string msg) { Verdict v; v.code = code; v.msg = std::move(msg); return v; }

// [off, off + len) lies inside [0, limit); nothing is added before it is compared
inline bool in_range(uint64_t off, uint64_t len, uint64_t limit) { return len <= limit && off <= limit - len; }

// ---- sg_reference_* ----------------------------------------------------------------------------------------------------
// scan and commit need the image of sg_reference_begin (a commit releases it)
inline Verdict need_image(bool have_image, const char* who) {
  if (!have_image) return refuse(SG_ERR_INVALID, std::string(who) + ": call sg_reference_begin first");
  return Verdict();
}

inline Verdict chunk(bool have_image, uint64_t image_bytes, uint64_t offset, uint64_t bytes) {
  if (!have_image || !in_range(offset, bytes, image_bytes))
    return refuse(SG_ERR_INVALID, "sg_reference_chunk: range outside sg_reference_begin's size");
  return Verdict();
}

// the bytes a contig takes in the image, from its first base to its last: bases and the line breaks between them;
// false: not a number of 64 bits
inline bool contig_extent(const sg_contig& k, uint64_t* extent) {
  const uint64_t lines = k.length ? (k.length - 1) / k.line_bases : 0;   // line breaks inside the contig
  uint64_t breaks = 0;
  if (__builtin_mul_overflow(lines, (uint64_t)(k.line_width - k.line_bases), &breaks)) return false;
  return !__builtin_add_overflow(k.length, breaks, extent);
}

// contig c of sg_reference_commit against an image of image_bytes
inline Verdict contig(const sg_contig& k, uint32_t c, uint64_t image_bytes) {
  if (k.length && (k.line_bases == 0 || k.line_width < k.line_bases))
    return refuse(SG_ERR_INVALID, "sg_reference_commit: contig " + std::to_string(c) + " has an impossible line shape");
  if (k.length > 0xFFFFFFF0ull)   // (the ingest kernel's line / column arithmetic is 32-bit; the host says the same, fasta.cpp)
    return refuse(SG_ERR_UNSUPPORTED, "sg_reference_commit: contig " + std::to_string(c) + " is longer than 4 Gbp");
  uint64_t extent = 0;
  if (!contig_extent(k, &extent) || !in_range(k.raw_offset, extent, image_bytes))
    return refuse(SG_ERR_INVALID, "sg_reference_commit: contig " + std::to_string(c) + " runs past the end of the file");
  return Verdict();
}

// ---- sg_build_haplotypes -----------------------------------------------------------------------------------------------
inline Verdict need_contigs(bool have_contigs, uint64_t n_pieces) {
  if (!have_contigs && n_pieces) return refuse(SG_ERR_INVALID, "sg_build_haplotypes: call sg_reference_commit first");
  return Verdict();
}

// piece i: inside its chain and inside its source (contig_length(k): the bases of committed contig k < n_contigs)
template <class ContigLength>
inline Verdict piece(const sg_hap_piece& p, uint64_t i, int32_t n_chains, const uint64_t* lens, ContigLength&& contig_length,
                     uint64_t n_contigs, uint64_t n_literal_bytes) {
  if ((int64_t)p.chain >= n_chains || !in_range(p.dst, p.len, lens[p.chain]))
    return refuse(SG_ERR_INVALID, "sg_build_haplotypes: piece " + std::to_string(i) + " falls outside its chain");
  if (p.kind == 0) {
    if (p.contig >= n_contigs || !in_range(p.src, p.len, contig_length(p.contig)))
      return refuse(SG_ERR_INVALID, "sg_build_haplotypes: piece " + std::to_string(i) + " falls outside its contig");
  } else if (!in_range(p.src, p.len, n_literal_bytes)) {
    return refuse(SG_ERR_INVALID, "sg_build_haplotypes: piece " + std::to_string(i) + " falls outside the literal bytes");
  }
  return Verdict();
}

// The pieces (each one already inside its chain) tile every chain: ordered by dst they follow one another without gap or
// overlap from 0 to lens[c].  Pieces of length 0 cover nothing and are accepted wherever they lie.  Pieces usually arrive
// in dst order chain by chain (chains may interleave): then one linear pass decides.  Only a list that is out of order
// is sorted, and the walk over the sorted list names the first piece that overlaps its predecessor or leaves a gap in
// front of itself, or the first chain that ends short.
inline Verdict tiling(int32_t n_chains, const uint64_t* lens, const sg_hap_piece* pieces, uint64_t n_pieces) {
  std::vector<uint64_t> next((size_t)n_chains, 0);
  bool in_order = true;
  for (uint64_t i = 0; i < n_pieces && in_order; i++) {
    const sg_hap_piece& p = pieces[i];
    if (!p.len) continue;
    if (p.dst == next[p.chain]) next[p.chain] += p.len;   // (<= lens[p.chain]: the piece lies inside its chain)
    else in_order = false;
  }
  if (!in_order) {
    std::vector<uint64_t> order;
    order.reserve((size_t)n_pieces);
    for (uint64_t i = 0; i < n_pieces; i++)
      if (pieces[i].len) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
      const sg_hap_piece &x = pieces[a], &y = pieces[b];
      return x.chain != y.chain ? x.chain < y.chain : x.dst != y.dst ? x.dst < y.dst : a < b;
    });
    std::fill(next.begin(), next.end(), 0);
    for (uint64_t i : order) {
      const sg_hap_piece& p = pieces[i];
      if (p.dst < next[p.chain])
        return refuse(SG_ERR_INVALID, "sg_build_haplotypes: piece " + std::to_string(i) + " overlaps another piece of chain " + std::to_string(p.chain));
      if (p.dst > next[p.chain])
        return refuse(SG_ERR_INVALID, "sg_build_haplotypes: the pieces of chain " + std::to_string(p.chain) + " leave a gap in front of piece " + std::to_string(i));
      next[p.chain] += p.len;
    }
  }
  for (int32_t c = 0; c < n_chains; c++)
    if (next[c] != lens[c]) return refuse(SG_ERR_INVALID, "sg_build_haplotypes: the pieces of chain " + std::to_string(c) + " do not add up to its length");
  return Verdict();
}

inline Verdict patch(const sg_hap_patch& q, uint64_t i, int32_t n_chains, const uint64_t* lens) {
  if ((int64_t)q.chain >= n_chains || q.dst >= lens[q.chain])
    return refuse(SG_ERR_INVALID, "sg_build_haplotypes: patch " + std::to_string(i) + " falls outside its chain");
  return Verdict();
}

// ---- sg_haplotype_codes ------------------------------------------------------------------------------------------------
inline Verdict codes(bool have_haps, const uint64_t* chain_len, uint64_t n_chains, uint32_t chain, uint64_t offset, uint64_t n) {
  if (!have_haps) return refuse(SG_ERR_INVALID, "sg_haplotype_codes: no haplotypes on the device");
  if (chain >= n_chains) return refuse(SG_ERR_INVALID, "sg_haplotype_codes: chain index out of range");
  if (!in_range(offset, n, chain_len[chain])) return refuse(SG_ERR_INVALID, "sg_haplotype_codes: range past the end of the chain");
  return Verdict();
}

}  // namespace hapcheck
}  // namespace sg
