// sg_inflate.hip -- BGZF members inflated on the device (RFC 1951 / 1952, SAMv1 section 4.1): the reverse of sg_deflate.hip.
//
//   inflate_kernel  workgroup = one wave = one member.  The member's output (at most 64 KiB) is staged in LDS, so a match
//                   copy reads bytes of the same wave's LDS and never bytes it has just stored to global memory.  The
//                   bit stream is decoded by all 64 lanes in lockstep (every lane holds the same bit buffer and the same
//                   symbol, so the decode costs one lane's time); a literal is stored by lane 0, a match is copied by all
//                   lanes at once (lane k takes byte k, k + 64, ... of the copy; an overlapping copy of distance d < length
//                   reads byte k mod d of the source, which lies before the copy).  Decode tables: a 10-bit look-up
//                   table filled by all lanes, longer codes by the canonical walk (count / symbol lists).  Then the
//                   CRC-32 of the output, 1 KiB per lane combined by a tree of "advance by 1024 * 2^k zero bytes" operators
//                   (the output is right-aligned in 64 KiB; the standard register start of ~0 is folded into the first four
//                   bytes), the check against the trailer, and one copy out.
// A member that is not a well-formed DEFLATE stream gets a verdict (sg_bam.h) and writes nothing; every read stays inside
// the batch and every write inside the member's own 64 KiB of LDS / its ISIZE bytes of output.
// Bytes left over between the final block and the trailer are accepted, as zlib's inflate() accepts them (it returns
// Z_STREAM_END with input left): the member is taken when its output has the trailer's ISIZE and CRC-32.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "sg_bam.h"

namespace sg {

namespace {

constexpr uint32_t kFastBits = 10;

struct Huff {
  uint16_t fast[1u << kFastBits];   // (symbol << 4) | length for codes of up to kFastBits bits, 0: longer code
  uint16_t count[16];               // codes of each length
  uint16_t first_code[16], start[16], next[16];
  uint16_t sym[320];                // symbols in canonical order
};
struct InflLds {
  uint8_t out[kBgzfMaxIsize];
  Huff lit, dist;
  uint32_t crc_tab[256];
  uint32_t crcs[64];
  uint8_t lens[352];                // fixed codes: [0, 320); dynamic: the code-length code at [0, 19), the codes at [32, 348)
  int32_t verdict;
};

__constant__ uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
                                       6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t kClenOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// LSB-first bit reader, the same in every lane.  Bytes past the batch read as zero; running past the member's DEFLATE data
// is found by the bit count.
struct Bits {
  const uint8_t* p;
  uint64_t pos, lim;   // next byte to load; bytes of the batch
  uint64_t bb;
  uint32_t bc;
  __device__ __forceinline__ void refill() {
    if (bc <= 32) {
      uint32_t v = 0;
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) v |= (uint32_t)(pos + k < lim ? p[pos + k] : 0) << (8 * k);
      bb |= (uint64_t)v << bc;
      bc += 32;
      pos += 4;
    }
  }
  __device__ __forceinline__ uint32_t take(uint32_t n) {   // n <= 32 bits, refill() before
    const uint32_t v = (uint32_t)(bb & ((1ull << n) - 1));
    bb >>= n;
    bc -= n;
    return v;
  }
};

__device__ __forceinline__ int decode(const Huff& h, Bits& b) {
  b.refill();
  const uint32_t e = h.fast[b.bb & ((1u << kFastBits) - 1)];
  if (e) { b.take(e & 15u); return (int)(e >> 4); }
  int code = 0, first = 0, index = 0;
  for (uint32_t len = 1; len <= 15; len++) {   // canonical walk (RFC 1951 3.2.2), one code bit at a time
    code |= (int)((b.bb >> (len - 1)) & 1u);
    const int count = h.count[len];
    if (code - count < first) { b.take(len); return h.sym[index + (code - first)]; }
    index += count;
    first = (first + count) << 1;
    code <<= 1;
  }
  return -1;
}

// Decode tables from code lengths lens[0, n).  kind 0: code-length code (must be complete), 1: literal / length and
// distance codes (an incomplete code only as a single code of length 1, as zlib allows).  All lanes call it; 0 or a verdict.
__device__ uint32_t build(Huff& h, const uint8_t* lens, uint32_t n, int kind, InflLds& S) {
  const uint32_t lane = threadIdx.x;
  if (lane == 0) {
    for (int l = 0; l < 16; l++) h.count[l] = 0;
    for (uint32_t s = 0; s < n; s++) h.count[lens[s]]++;
    int left = 1, max_len = 0;
    for (int l = 1; l < 16; l++) {
      left = (left << 1) - h.count[l];
      if (h.count[l]) max_len = l;
      if (left < 0) break;
    }
    int verdict = 0;
    if (left < 0) verdict = kInflBadCode;
    else if (left > 0 && (kind == 0 || max_len > 1) && max_len > 0) verdict = kInflBadCode;
    else if (kind == 0 && max_len == 0) verdict = kInflBadCode;
    uint32_t code = 0, at = 0;
    h.count[0] = 0;
    for (int l = 1; l < 16; l++) {
      code = (code + h.count[l - 1]) << 1;
      h.first_code[l] = (uint16_t)code;
      h.start[l] = (uint16_t)at;
      at += h.count[l];
    }
    for (int l = 1; l < 16; l++) h.next[l] = h.start[l];
    for (uint32_t s = 0; s < n; s++)
      if (lens[s]) h.sym[h.next[lens[s]]++] = (uint16_t)s;
    S.verdict = verdict;
  }
  for (uint32_t i = lane; i < (1u << kFastBits); i += 64) h.fast[i] = 0;
  __syncthreads();
  if (S.verdict) return (uint32_t)S.verdict;
  uint32_t total = 0;
  for (int l = 1; l < 16; l++) total += h.count[l];
  for (uint32_t i = lane; i < total; i += 64) {
    uint32_t l = 1;
    while (l < 15 && i >= (uint32_t)h.start[l] + h.count[l]) l++;
    if (l > kFastBits) continue;
    const uint32_t code = h.first_code[l] + (i - h.start[l]);
    uint32_t rev = 0;
    for (uint32_t k = 0; k < l; k++) rev |= ((code >> k) & 1u) << (l - 1 - k);
    const uint16_t e = (uint16_t)((h.sym[i] << 4) | l);
    for (uint32_t f = rev; f < (1u << kFastBits); f += 1u << l) h.fast[f] = e;
  }
  __syncthreads();
  return 0;
}

__global__ __launch_bounds__(64) void inflate_kernel(InflateJob J) {
  extern __shared__ __align__(16) uint8_t lds_raw[];
  InflLds& S = *reinterpret_cast<InflLds*>(lds_raw);
  const uint32_t lane = threadIdx.x;
  const InflateMember m = J.members[blockIdx.x];
  const uint8_t* src = J.src;
  for (uint32_t i = lane; i < 256; i += 64) S.crc_tab[i] = J.crc_tab[i];
  uint32_t err = 0;
  const uint64_t dend = m.src + m.bytes - 8;   // the trailer: CRC32, ISIZE
  const uint32_t xlen = (uint32_t)src[m.src + 10] | ((uint32_t)src[m.src + 11] << 8);
  const uint64_t dstart = m.src + 12 + xlen;
  if (dstart > dend) err = kInflHeader;
  Bits b{src, dstart, J.src_bytes, 0, 0};
  uint32_t op = 0;
  bool last = false;
  while (!err && !last) {
    b.refill();
    last = b.take(1) != 0;
    const uint32_t type = b.take(2);
    if (type == 0) {   // stored
      b.take(b.bc & 7u);
      b.refill();
      const uint32_t len = b.take(16), nlen = b.take(16);
      if (len != (~nlen & 0xFFFFu)) { err = kInflStoredLen; break; }
      if (op + len > kBgzfMaxIsize) { err = kInflTooLong; break; }
      uint32_t k = 0;
      for (; k < len && b.bc; k++) {
        const uint32_t v = b.take(8);
        if (lane == 0) S.out[op + k] = (uint8_t)v;
      }
      const uint32_t rest = len - k;
      if (rest && b.pos + rest > dend) { err = kInflOverrun; break; }   // (with rest > 0 the bit buffer is empty: b.pos is the next byte)
      for (uint32_t i = lane; i < rest; i += 64) S.out[op + k + i] = src[b.pos + i];
      b.pos += rest;
      op += len;
      continue;
    }
    if (type == 3) { err = kInflBlockType; break; }
    if (type == 1) {   // fixed codes (RFC 1951 3.2.6); distance codes 30 and 31 take part in the code but are refused below
      for (uint32_t i = lane; i < 320; i += 64) S.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
      __syncthreads();
      if ((err = build(S.lit, S.lens, 288, 1, S))) break;
      if ((err = build(S.dist, S.lens + 288, 32, 1, S))) break;
    } else {           // dynamic codes (3.2.7)
      b.refill();
      const uint32_t hlit = b.take(5) + 257, hdist = b.take(5) + 1, hclen = b.take(4) + 4;
      if (hlit > 286 || hdist > 30) { err = kInflBadCode; break; }
      for (uint32_t i = lane; i < 19; i += 64) S.lens[i] = 0;
      __syncthreads();
      for (uint32_t i = 0; i < hclen; i++) {
        b.refill();
        const uint32_t v = b.take(3);
        if (lane == 0) S.lens[kClenOrder[i]] = (uint8_t)v;
      }
      __syncthreads();
      if ((err = build(S.dist, S.lens, 19, 0, S))) break;   // (the distance slot holds the code-length code for a while)
      uint32_t idx = 0, prev = 0;
      const uint32_t want = hlit + hdist;
      while (idx < want) {
        const int sym = decode(S.dist, b);
        if (sym < 0) { err = kInflBadCode; break; }
        uint32_t rep = 1, v = (uint32_t)sym;
        if (sym == 16) {
          if (idx == 0) { err = kInflBadCode; break; }
          v = prev; rep = 3 + b.take(2);
        } else if (sym == 17) {
          v = 0; rep = 3 + b.take(3);
        } else if (sym == 18) {
          v = 0; rep = 11 + b.take(7);
        }
        if (idx + rep > want) { err = kInflBadCode; break; }
        for (uint32_t i = lane; i < rep; i += 64) S.lens[32 + idx + i] = (uint8_t)v;   // (behind the 19 code-length lengths)
        idx += rep;
        prev = v;
        if (b.pos > dend + 8) { err = kInflOverrun; break; }
      }
      __syncthreads();
      if (err) break;
      if (S.lens[32 + 256] == 0) { err = kInflBadCode; break; }   // no end-of-block code
      if ((err = build(S.lit, S.lens + 32, hlit, 1, S))) break;
      if ((err = build(S.dist, S.lens + 32 + hlit, hdist, 1, S))) break;
    }
    for (;;) {   // the block's symbols
      const int sym = decode(S.lit, b);
      if (sym < 256) {
        if (sym < 0) { err = kInflBadCode; break; }
        if (op >= kBgzfMaxIsize) { err = kInflTooLong; break; }
        if (lane == 0) S.out[op] = (uint8_t)sym;
        op++;
        continue;
      }
      if (sym == 256) break;
      const uint32_t ls = (uint32_t)sym - 257;
      if (ls >= 29) { err = kInflBadCode; break; }
      const uint32_t len = kLenBase[ls] + b.take(kLenExtra[ls]);
      const int ds = decode(S.dist, b);
      if (ds < 0 || ds >= 30) { err = ds < 0 ? kInflBadCode : kInflDistance; break; }
      const uint32_t dist = kDistBase[ds] + b.take(kDistExtra[ds]);
      if (dist > op) { err = kInflDistance; break; }
      if (op + len > kBgzfMaxIsize) { err = kInflTooLong; break; }
      const uint32_t from = op - dist;
      for (uint32_t k = lane; k < len; k += 64) S.out[op + k] = S.out[dist >= len ? from + k : from + k % dist];
      op += len;
      if (b.pos > dend + 8) { err = kInflOverrun; break; }
    }
    if (!err && b.pos > dend + 8) err = kInflOverrun;
  }
  if (!err && (b.pos - dstart) * 8 - b.bc > (dend - dstart) * 8) err = kInflOverrun;
  const uint32_t want_crc = (uint32_t)src[dend] | ((uint32_t)src[dend + 1] << 8) | ((uint32_t)src[dend + 2] << 16) | ((uint32_t)src[dend + 3] << 24);
  const uint32_t want_isize = (uint32_t)src[dend + 4] | ((uint32_t)src[dend + 5] << 8) | ((uint32_t)src[dend + 6] << 16) | ((uint32_t)src[dend + 7] << 24);
  if (!err && (op != want_isize || op != m.isize)) err = kInflIsize;
  __syncthreads();
  if (!err) {
    // ---- CRC-32: lane l takes bytes [l * 1024, (l + 1) * 1024) of the output right-aligned in 64 KiB ----
    uint32_t crc;
    if (op >= 4) {
      const int64_t j0 = (int64_t)lane * kCrcLaneBytes - (int64_t)(kBgzfMaxIsize - op);
      uint32_t c = 0;
      for (int64_t j = j0 < 0 ? 0 : j0; j < j0 + (int64_t)kCrcLaneBytes; j++) {
        const uint32_t v = S.out[j] ^ (j < 4 ? 0xFFu : 0u);
        c = (c >> 8) ^ S.crc_tab[(c ^ v) & 0xFFu];
      }
      S.crcs[lane] = c;
      for (uint32_t k = 0; k < kCrcLevels; k++) {
        __syncthreads();
        if ((lane & ((2u << k) - 1)) == 0) {
          const uint32_t x = S.crcs[lane], y = S.crcs[lane + (1u << k)];
          uint32_t r = y;
          for (uint32_t i = 0; i < 8; i++) r ^= J.crc_shift[k * 128u + i * 16u + ((x >> (4 * i)) & 15u)];
          S.crcs[lane] = r;
        }
      }
      __syncthreads();
      crc = ~S.crcs[0];
    } else {
      uint32_t c = 0xFFFFFFFFu;
      for (uint32_t j = 0; j < op; j++) c = (c >> 8) ^ S.crc_tab[(c ^ S.out[j]) & 0xFFu];
      crc = ~c;
    }
    if (crc != want_crc) err = kInflCrc;
  }
  if (!err) {
    uint8_t* dst = J.out + m.dst;
    for (uint32_t k = lane; k < op; k += 64) dst[k] = S.out[k];
  }
  if (lane == 0) J.status[blockIdx.x] = err;
}

struct CrcTables {
  uint32_t tab[256];
  uint32_t shift[kCrcLevels][8][16];
  CrcTables() {
    for (uint32_t i = 0; i < 256; i++) {
      uint32_t c = i;
      for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      tab[i] = c;
    }
    for (uint32_t k = 0; k < kCrcLevels; k++) {
      uint32_t col[32];
      for (int j = 0; j < 32; j++) {
        uint32_t s = 1u << j;
        for (uint64_t n = 0; n < ((uint64_t)kCrcLaneBytes << k); n++) s = (s >> 8) ^ tab[s & 0xFFu];
        col[j] = s;
      }
      for (int i = 0; i < 8; i++)
        for (uint32_t v = 0; v < 16; v++) {
          uint32_t r = 0;
          for (int t = 0; t < 4; t++)
            if (v & (1u << t)) r ^= col[4 * i + t];
          shift[k][i][v] = r;
        }
    }
  }
};
const CrcTables& crc_tables() {
  static const CrcTables* t = new CrcTables;
  return *t;
}

}  // namespace

const uint32_t* inflate_crc_tab() { return crc_tables().tab; }
const uint32_t* inflate_crc_shift() { return &crc_tables().shift[0][0][0]; }

void launch_inflate(const InflateJob& J, hipStream_t s) {
  if (!J.n) return;
  const size_t lds = sizeof(InflLds);
  (void)hipFuncSetAttribute((const void*)inflate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(inflate_kernel, dim3(J.n), dim3(64), lds, s, J);
}

}  // namespace sg
