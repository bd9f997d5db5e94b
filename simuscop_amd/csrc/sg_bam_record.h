// sg_bam_record.h -- one BAM record of an inflated stream on the device (SAMv1 section 4.2): its fixed fields and the checks every
// kernel that takes records makes first (sg_bam.hip: the lines of the training input; sg_eval.hip: the rows of truthEval).
// Device code only.  A record is read once its block_size says the stream holds it whole.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sg_bam.h"

namespace sg {

__device__ __forceinline__ uint32_t rd32(const uint8_t* d, uint64_t o) {
  return (uint32_t)d[o] | ((uint32_t)d[o + 1] << 8) | ((uint32_t)d[o + 2] << 16) | ((uint32_t)d[o + 3] << 24);
}
__device__ __forceinline__ uint32_t rd16(const uint8_t* d, uint64_t o) { return (uint32_t)d[o] | ((uint32_t)d[o + 1] << 8); }

// ---- one record: its fields, the checks (kBamOk or the error code) ----
struct Rec {
  uint32_t bs, lname, mapq, ncig, flag;
  int32_t ref, pos, lseq, nref, npos, tlen;
  uint64_t name, cig, seq, qual, aux, end;   // offsets in the stream
  uint64_t ops;                              // where the CIGAR operations are read (the record's or its CG tag's)
  uint32_t nops;
};

__device__ inline uint32_t aux_size(uint8_t ty) {
  switch (ty) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    case 'd': return 8;
    default: return 0;
  }
}

__device__ inline uint32_t parse(const BamJob& J, uint64_t o, Rec& R) {
  const uint8_t* d = J.d;
  R.bs = rd32(d, o);
  if (R.bs < 32) return kBamShort;
  R.end = o + 4 + R.bs;
  R.ref = (int32_t)rd32(d, o + 4);
  R.pos = (int32_t)rd32(d, o + 8);
  R.lname = d[o + 12];
  R.mapq = d[o + 13];
  R.ncig = rd16(d, o + 16);
  R.flag = rd16(d, o + 18);
  R.lseq = (int32_t)rd32(d, o + 20);
  R.nref = (int32_t)rd32(d, o + 24);
  R.npos = (int32_t)rd32(d, o + 28);
  R.tlen = (int32_t)rd32(d, o + 32);
  if (R.lname < 1 || R.lseq < 0) return kBamLengths;
  if (32ull + R.lname + 4ull * R.ncig + ((uint64_t)R.lseq + 1) / 2 + (uint64_t)R.lseq > R.bs) return kBamShort;
  if (R.ref < -1 || R.ref >= (int32_t)J.n_ref || R.nref < -1 || R.nref >= (int32_t)J.n_ref) return kBamRefId;
  R.name = o + 36;
  R.cig = R.name + R.lname;
  R.seq = R.cig + 4ull * R.ncig;
  R.qual = R.seq + ((uint64_t)R.lseq + 1) / 2;
  R.aux = R.qual + (uint64_t)R.lseq;
  for (uint32_t i = 0; i < R.ncig; i++)
    if ((d[R.cig + 4ull * i] & 15u) > 8) return kBamOpCode;
  R.ops = R.cig;
  R.nops = R.ncig;
  // htslib's bam_tag2cigar: a first operation kS with k = l_seq stands for the real CIGAR in CG:B:I
  if (R.ncig > 0 && R.ref >= 0 && R.pos >= 0 && (d[R.cig] & 15u) == 4 && (rd32(d, R.cig) >> 4) == (uint32_t)R.lseq) {
    uint64_t p = R.aux;
    while (p + 3 <= R.end) {
      const uint8_t t0 = d[p], t1 = d[p + 1], ty = d[p + 2];
      p += 3;
      if (ty == 'Z' || ty == 'H') {
        while (p < R.end && d[p]) p++;
        p++;
      } else if (ty == 'B') {
        if (p + 5 > R.end) break;
        const uint8_t sub = d[p];
        const uint32_t n = rd32(d, p + 1), es = aux_size(sub);
        if (!es) break;
        if (t0 == 'C' && t1 == 'G' && (sub == 'I' || sub == 'i')) {
          if (n >= R.ncig && n < (1u << 29) && p + 5 + 4ull * n <= R.end) {
            R.ops = p + 5;
            R.nops = n;
            for (uint32_t i = 0; i < n; i++)
              if ((d[R.ops + 4ull * i] & 15u) > 8) return kBamOpCode;
          }
          break;
        }
        p += 5 + (uint64_t)n * es;
      } else {
        const uint32_t es = aux_size(ty);
        if (!es) break;
        p += es;
      }
    }
  }
  return kBamOk;
}

}  // namespace sg
