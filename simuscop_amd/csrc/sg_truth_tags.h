// sg_truth_tags.h -- the tag rule of sg_truth.h (truth_tags_walk, truth_xe) as one wave walks it: the operations and
// the events are taken one after the other by the whole wave, the bases of a run 64 at a time, lane = base.  What both
// tag kernels share: truth_tag_size_kernel (sg_truth_tags.hip) counts the MD text's bytes, the tagged record kernel
// (sg_truth.hip) writes them into its image.  Device code only.
#pragma once
#include "sg_truth.h"

namespace sg {

// SEQ as the record shows it, over the read's bases in FASTQ orientation (global memory or the record kernel's text stage)
struct WaveSeq {
  const uint8_t* bases;
  uint32_t np;
  bool flip;   // the record is turned round: letter i is the complement of base np - 1 - i
};
__device__ __forceinline__ uint32_t wave_seq_letter(const WaveSeq& S, uint32_t i) {
  return S.flip ? truth_complement(S.bases[S.np - 1u - i]) : (uint32_t)S.bases[i];
}

// truth_tags_walk by a wave.  `ref` are the contig's codes from POS on, `room` of them; a base outside SEQ or outside
// the contig is not loaded (the caller compares q_end and r_end with what the record has and fails the call).  With
// kWrite the text's bytes below `cap` go to `out`; without, nothing is written and a D run costs no loop.
template <bool kWrite>
__device__ __forceinline__ TagWalk wave_tags_walk(const uint32_t* ops, uint32_t n_ops, const WaveSeq& S, const uint8_t* ref, uint64_t room,
                                                  uint32_t lane, uint8_t* out, uint32_t cap) {
  TagWalk W = {0u, 0u, 0u, 0u};
  uint32_t m = 0;
  auto number = [&]() {
    const uint32_t n = truth_digits(m);
    if (kWrite && lane < n && W.md_len + lane < cap) out[W.md_len + lane] = (uint8_t)truth_digit(m, n, lane);
    W.md_len += n;
    m = 0;
  };
  for (uint32_t k = 0; k < n_ops; k++) {
    const uint32_t len = ops[k] >> 4, op = ops[k] & 15u;
    if (op == kOpM) {
      for (uint32_t c = 0; c < len; c += 64u) {
        const uint32_t i = c + lane;
        const bool valid = i < len;
        uint32_t code = 5u, letter = 0u;
        if (valid && W.q_end + i < S.np && W.r_end + i < room) {
          code = ref[W.r_end + i];
          letter = wave_seq_letter(S, W.q_end + i);
        }
        unsigned long long mask = __ballot(valid && !truth_base_matches(letter, code));
        const uint32_t nv = len - c < 64u ? len - c : 64u;
        uint32_t base = 0;
        W.nm += (uint32_t)__popcll(mask);
        while (mask) {   // the mismatches are few: one after the other, the whole wave
          const uint32_t b = (uint32_t)__ffsll((long long)mask) - 1u;
          mask &= mask - 1ull;
          m += b - base;
          number();
          if (kWrite && lane == b && W.md_len < cap) out[W.md_len] = (uint8_t)truth_ref_letter(code);
          W.md_len++;
          base = b + 1u;
        }
        m += nv - base;
      }
      W.q_end += len;
      W.r_end += len;
    } else if (op == kOpD) {
      number();
      if (kWrite) {
        if (lane == 0u && W.md_len < cap) out[W.md_len] = (uint8_t)'^';
        for (uint32_t i = lane; i < len && W.md_len + 1u + i < cap; i += 64u)
          out[W.md_len + 1u + i] = (uint8_t)truth_ref_letter(W.r_end + i < room ? (uint32_t)ref[W.r_end + i] : 5u);
      }
      W.md_len += 1u + len;
      W.nm += len;
      W.r_end += len;
    } else if (op == kOpN) {
      W.r_end += len;
    } else {
      if (op == kOpI) W.nm += len;
      W.q_end += len;
    }
  }
  number();
  return W;
}

// truth_xe by a wave: `chain` is the template's first base code in chain direction, `bases` the read in FASTQ orientation
__device__ __forceinline__ uint32_t wave_xe(const uint32_t* events, uint32_t n_events, uint32_t L, uint32_t np, bool reverse,
                                            const uint8_t* chain, const uint8_t* bases, uint32_t lane) {
  if (errtab_walk(events, n_events, L, [](uint32_t, uint32_t, uint32_t, uint32_t) {}) != np) return kErrWalkBad;
  uint32_t mine = 0, indel = 0;
  errtab_walk(events, n_events, L, [&](uint32_t kind, uint32_t j, uint32_t r, uint32_t n) {
    if (kind != 0u) { indel += n; return; }
    for (uint32_t i = lane; i < n; i += 64u) {
      const uint32_t tc = errtab_tmpl_code(chain[reverse ? L - 1u - (j + i) : j + i], reverse);
      if (tc < 4u && errtab_read_code(bases[r + i]) != tc) mine++;
    }
  });
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d, 64);
  return mine + indel;
}

// which tags a record gets: NM and MD when it is mapped (MD unless its text was dropped), XE when its template lies in its chain
__device__ __forceinline__ uint32_t tags_present(uint32_t tags, bool mapped, bool inside, uint32_t md_len) {
  return (mapped ? tags & kTagNM : 0u) | (mapped && md_len != kMdDropped ? tags & kTagMD : 0u) | (inside ? tags & kTagXE : 0u);
}

}  // namespace sg
