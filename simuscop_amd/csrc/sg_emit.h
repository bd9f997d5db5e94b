// sg_emit.h -- what the emit kernels of sg_kernels.hip (generic, slow, header), the straight-line kernel of
// sg_emit_fast.hip and fragment_kernel of sg_pass_front.hip as the rows' writer share: the workgroup shape, the read row,
// the straight-line kernel's LDS layout, the read-group runs and the few device helpers these files call.  Device code
// (.hip files only).
#pragma once
#include "sg_device.h"
#include "sg_philox.h"

namespace sg {

#define EMIT_THREADS 1024
#define EMIT_WAVES (EMIT_THREADS / 64)
#define META_ROW 32  // bytes of LDS metadata per read

// ------------------------------------------------------------------------------------------------
// The read row: DevBatch::meta holds 48 bytes per read, written by fragment_kernel (m0 and m1 through ReadRow::make_m0 and
// ReadRow::make_m1, then the name's text), read by every emit kernel and by header_kernel.
//   m0 (bytes 0..15)   x, y  offset of the fragment's first base in the chains buffer (low, high word)
//                      z     namepos   } the two numbers of the read's name "@popu#chr#pos%segsize#fragCount[/m]"
//                      w     fragcount }
//   m1 (bytes 16..31)  x     flen (bits 0..29: fragment length, 0 = unused slot) | bad_block << 30 (the read touches a
//                            64-base block holding a non-ACGT base: straight-line kernel only) | rev << 31
//                      y     np (bits 0..15: bases of the read, n') | nev << 16 (6 bits: sequencing indels) |
//                            hdr_len << 22 (10 bits: bytes of the name line, line break included)
//                      z     inv = ceil(2^32 / np): bin = (i * bins * inv) >> 32
//                      w     the event itself (ev_pack) when nev == 1, else 0
//   text (bytes 32..47) the name's own part "pos#count[/m]\n" when it fits 16 bytes (zero beyond its end)
// A read is `active` when word m1.x has any of its low 31 bits set.
//
// The generic kernels keep m0, m1 in registers or LDS and put the record's 64-bit offset in the text into m0.z, m0.w
// (set_out64 / out64: the name's numbers are header_kernel's business, not theirs).
//
// The straight-line kernel keeps the two words in LDS (32 bytes per read, FastRow below) and reuses four of them from
// phase 0 on, for what its plain and clean steps need of a read:
//   m0.y  src_m5: base index of output position -5 in the 2-bit copy the read walks (bits 0..30; the kernel runs on
//         buffers < 2^31 bases) | copy_is_rc << 31 (that copy is the reverse complement)
//   m0.z  out_off: offset of the record from the read group's first record (32 bits)
//   m0.w  base_off: out_off + hdr_len, the offset of the read's first base
// m0.x (the fragment offset's low word) stays: the general steps compute their windows from it (fast_src).
// When the general steps have sampled a read's LAST item and that item is partial (or the read goes to the slow queue),
// the item is parked in the row over fields no lane needs once the last item has been sampled:
//   m0.x, m0.y  the item's eight base characters (m0.x = 0xFFFFFFFF: the read's last item went to emit_slow_kernel;
//               base characters are never 0xFF)
//   m1.z, m1.w  its eight quality characters (over inv and the event: the fix-up pass computes inv again)
// So nothing of a read may follow its last item in the general stream, and an idle lane must not follow a row's fragment
// offset, reciprocal or event.  m0.z, m0.w, m1.x and m1.y stay valid until the group ends.
// ------------------------------------------------------------------------------------------------
namespace row {
constexpr uint32_t kFlenMask = 0x3FFFFFFFu, kNpMax = 0xFFFFu, kNevMax = 63u, kHdrMax = 1023u;
constexpr uint32_t pack_x(uint32_t flen, uint32_t bad_block, uint32_t rev) { return flen | (bad_block << 30) | (rev << 31); }
constexpr uint32_t pack_y(uint32_t np, uint32_t nev, uint32_t hdr_len) { return np | (nev << 16) | (hdr_len << 22); }
constexpr uint32_t flen(uint32_t x) { return x & kFlenMask; }
constexpr uint32_t bad_block(uint32_t x) { return (x >> 30) & 1u; }
constexpr bool rev(uint32_t x) { return (x >> 31) != 0u; }
constexpr bool active(uint32_t x) { return (x & 0x7FFFFFFFu) != 0u; }
constexpr uint32_t np(uint32_t y) { return y & kNpMax; }
constexpr uint32_t nev(uint32_t y) { return (y >> 16) & kNevMax; }
constexpr uint32_t hdr_len(uint32_t y) { return y >> 22; }
// ceil(2^32 / np) = floor((2^32-1)/np) + 1: bin = (i*bins*inv) >> 32 is exact while i*bins*np < 2^32 (sg_load_profile
// rejects profiles that could violate the bound)
constexpr uint32_t inv_of(uint32_t np) { return 0xFFFFFFFFu / np + 1u; }
// the straight-line kernel's word m0.y
constexpr uint32_t pack_src(uint32_t src_m5, bool rc) { return src_m5 | (rc ? 0x80000000u : 0u); }
constexpr uint32_t src_m5(uint32_t w) { return w & 0x7FFFFFFFu; }
constexpr bool copy_is_rc(uint32_t w) { return (w >> 31) != 0u; }

static_assert(np(pack_y(kNpMax, kNevMax, kHdrMax)) == kNpMax && nev(pack_y(kNpMax, kNevMax, kHdrMax)) == kNevMax &&
              hdr_len(pack_y(kNpMax, kNevMax, kHdrMax)) == kHdrMax, "m1.y: extreme values of all three fields");
static_assert(np(pack_y(kNpMax, 0, 0)) == kNpMax && nev(pack_y(kNpMax, 0, 0)) == 0 && hdr_len(pack_y(0, kNevMax, 0)) == 0 &&
              nev(pack_y(0, 0, kHdrMax)) == 0 && np(pack_y(0, kNevMax, kHdrMax)) == 0, "m1.y: no field leaks into a neighbour");
static_assert(flen(pack_x(kFlenMask, 1, 1)) == kFlenMask && bad_block(pack_x(kFlenMask, 1, 1)) == 1 && rev(pack_x(kFlenMask, 1, 1)),
              "m1.x: flen = 2^30 - 1 with both flag bits");
static_assert(bad_block(pack_x(kFlenMask, 0, 1)) == 0 && !rev(pack_x(kFlenMask, 1, 0)) && active(pack_x(1, 0, 0)) &&
              active(pack_x(0, 1, 0)) && !active(pack_x(0, 0, 1)), "m1.x: the flags are independent; rev alone is not active");
static_assert(src_m5(pack_src(0x7FFFFFFFu, true)) == 0x7FFFFFFFu && copy_is_rc(pack_src(0, true)) && !copy_is_rc(pack_src(0x7FFFFFFFu, false)),
              "m0.y of the straight-line kernel's row");
static_assert(inv_of(1) == 0u && inv_of(151) == 28443493u && inv_of(kNpMax) == 65538u, "ceil(2^32 / np) in 32 bits");
}  // namespace row

struct ReadRow {
  uint4 m0, m1;
  __device__ __forceinline__ static ReadRow load(const uint4* meta, size_t idx) { return ReadRow{meta[idx * 3], meta[idx * 3 + 1]}; }
  __device__ __forceinline__ static ReadRow none() { return ReadRow{make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)}; }
  // the writer's side (fragment_kernel): the two words of a live read; an unused slot's are all zero
  __device__ __forceinline__ static uint4 make_m0(uint64_t foff, uint32_t namepos, uint32_t fragcount) {
    return make_uint4((uint32_t)foff, (uint32_t)(foff >> 32), namepos, fragcount);
  }
  // (event: the event of a read with exactly one, else 0)
  __device__ __forceinline__ static uint4 make_m1(uint32_t flen, uint32_t bad_block, uint32_t rev, uint32_t np, uint32_t nev,
                                                  uint32_t hdr_len, uint32_t event) {
    return make_uint4(row::pack_x(flen, bad_block, rev), row::pack_y(np, nev, hdr_len), row::inv_of(np), event);
  }
  __device__ __forceinline__ uint32_t flen() const { return row::flen(m1.x); }
  __device__ __forceinline__ bool rev() const { return row::rev(m1.x); }
  __device__ __forceinline__ uint32_t bad_block() const { return row::bad_block(m1.x); }
  __device__ __forceinline__ bool active() const { return row::active(m1.x); }
  __device__ __forceinline__ uint32_t np() const { return row::np(m1.y); }
  __device__ __forceinline__ uint32_t nev() const { return row::nev(m1.y); }
  __device__ __forceinline__ uint32_t hdr_len() const { return row::hdr_len(m1.y); }
  __device__ __forceinline__ uint32_t inv() const { return m1.z; }
  __device__ __forceinline__ uint32_t event() const { return m1.w; }
  __device__ __forceinline__ uint32_t items() const { return (np() + 7u) / 8u; }   // 8-base items of the read's bases
  __device__ __forceinline__ uint32_t rec_len() const { return hdr_len() + 2u * np() + 4u; }  // name line + 2 lines + "\n+\n", '\n'
  __device__ __forceinline__ uint64_t frag_off() const { return ((uint64_t)m0.y << 32) | m0.x; }
  __device__ __forceinline__ uint32_t frag_lo() const { return m0.x; }
  __device__ __forceinline__ uint32_t namepos() const { return m0.z; }
  __device__ __forceinline__ uint32_t fragcount() const { return m0.w; }
  // generic kernels: the record's offset in the mate's text, over the name's numbers
  __device__ __forceinline__ void set_out64(uint64_t off) { m0.z = (uint32_t)off; m0.w = (uint32_t)(off >> 32); }
  __device__ __forceinline__ uint64_t out64() const { return ((uint64_t)m0.w << 32) | m0.z; }
};

// The straight-line kernel's LDS row (layout above): a ReadRow whose words m0.y, m0.z, m0.w have been rewritten.
struct FastRow : ReadRow {
  // rc: the read walks the reverse-complement 2-bit copy, where the fragment [A, A + n) starts at total - A - n
  __device__ __forceinline__ static FastRow for_steps(const ReadRow& g, bool rc, uint32_t chains_total, uint32_t out_off) {
    FastRow r;
    r.m0 = g.m0; r.m1 = g.m1;
    r.m0.y = row::pack_src((rc ? chains_total - g.m0.x - g.flen() : g.m0.x) - 5u, rc);
    r.m0.z = out_off;
    r.m0.w = out_off + g.hdr_len();
    return r;
  }
  __device__ __forceinline__ uint32_t src_m5() const { return row::src_m5(m0.y); }
  __device__ __forceinline__ bool copy_is_rc() const { return row::copy_is_rc(m0.y); }
  __device__ __forceinline__ uint32_t out_off() const { return m0.z; }
  __device__ __forceinline__ uint32_t base_off() const { return m0.w; }
  // the parked last item, as the per-read pass reads it back
  __device__ __forceinline__ bool parked_slow() const { return m0.x == 0xFFFFFFFFu; }
  __device__ __forceinline__ uint64_t parked_bases() const { return ((uint64_t)m0.y << 32) | m0.x; }
  __device__ __forceinline__ uint64_t parked_quals() const { return ((uint64_t)m1.w << 32) | m1.z; }
};

// One wave's 64 rows in LDS.
struct FastRows {
  uint4* rows;
  __device__ __forceinline__ FastRow load(uint32_t r) const { FastRow f; f.m0 = rows[r * 2]; f.m1 = rows[r * 2 + 1]; return f; }
  __device__ __forceinline__ void store(uint32_t r, const FastRow& f) const { rows[r * 2] = f.m0; rows[r * 2 + 1] = f.m1; }
  // single words, for the plain steps (one 4-byte LDS read each instead of the row's two 16-byte ones)
  __device__ __forceinline__ uint32_t src_word(uint32_t r) const { return ((const uint32_t*)(rows + r * 2))[1]; }   // m0.y
  __device__ __forceinline__ uint32_t base_off(uint32_t r) const { return ((const uint32_t*)(rows + r * 2))[3]; }   // m0.w
  __device__ __forceinline__ uint32_t np(uint32_t r) const { return row::np(rows[r * 2 + 1].y); }
  // the read's last item, parked (slow: it went to emit_slow_kernel, the characters do not matter)
  __device__ __forceinline__ void park(uint32_t r, bool slow, const uint32_t (&sw)[2], const uint32_t (&qw)[2]) const {
    uint4* tail_row = rows + r * 2;
    tail_row[0].x = slow ? 0xFFFFFFFFu : sw[0];
    tail_row[0].y = sw[1];
    tail_row[1].z = qw[0];
    tail_row[1].w = qw[1];
  }
  // base h of a parked item redone by the fix-up pass: characters in words 0, 1, qualities in words 6, 7 of the row
  __device__ __forceinline__ void patch_parked(uint32_t r, uint32_t h, uint32_t ch, uint32_t sym) const {
    uint8_t* row8 = (uint8_t*)(rows + r * 2);
    row8[h] = (uint8_t)ch;
    row8[24u + h] = (uint8_t)sym;
  }
};

// ------------------------------------------------------------------------------------------------
// The straight-line kernel's dynamic LDS, stated once for the kernel (which takes its pointers from it) and the host
// (which takes the launch's byte count and the clean list's head-room from it).  Byte offsets; every region but the
// first three is per wave, EMIT_WAVES of them back to back.
// ------------------------------------------------------------------------------------------------
#define LUT_ROW 12u    // dwords per item in the look-up row: so[0..7], qo[0..1], 2 unused
#define SLOW_CAP 128  // per-wave queue of items deferred to the generic code
#define OVF_CAP 192   // per-wave list of single items: the plain reads' last items (<= 63) + appended items (<= 126)
#define FIX_CAP 128   // per-wave list of flagged bases waiting for the group's fix-up pass
#define CLEAN_CAP 256 // per-wave list of the one-indel reads' clean items (~10 such reads of 19 items in a group at XTen rates)

struct FastLds {
  uint32_t img;     // table image: bins x fast_stride words, rounded up to 16 bytes
  uint32_t lut;     // look-up rows: TI x LUT_ROW words
  uint32_t code4;   // 256 words: four 2-bit codes -> bytes code * 4
  uint32_t rows;    // per wave: 64 read rows of META_ROW bytes (FastRows)
  uint32_t slow;    // per wave: SLOW_CAP words, items for the slow queue (read | item << 8)
  uint32_t fix;     // per wave: FIX_CAP uint2, flagged items waiting for the fix-up pass
  uint32_t perm;    // per wave: 64 bytes, the general stream's reads in step order
  uint32_t permp;   // per wave: 64 bytes, the plain reads of a group, in lane order
  uint32_t ovf;     // per wave: OVF_CAP uint16, single items of the general stream (read | item << 8)
  uint32_t clean;   // per wave: clean_cap uint16, clean items of one-indel reads (read | after << 6 | item << 7)
  uint32_t total;
  __host__ __device__ FastLds(uint32_t bins, uint32_t fast_stride, uint32_t TI, uint32_t clean_cap) {
    img = 0;
    lut = img + ((bins * fast_stride + 3u) & ~3u) * 4u;
    code4 = lut + TI * LUT_ROW * 4u;
    rows = code4 + 256u * 4u;
    slow = rows + EMIT_WAVES * 64u * META_ROW;
    fix = slow + EMIT_WAVES * SLOW_CAP * 4u;
    perm = fix + EMIT_WAVES * FIX_CAP * 8u;
    permp = perm + EMIT_WAVES * 64u;
    ovf = permp + EMIT_WAVES * 64u;
    clean = ovf + EMIT_WAVES * OVF_CAP * 2u;
    total = clean + EMIT_WAVES * clean_cap * 2u;
  }
  // the largest clean list (entries per wave, whole 64s, at most CLEAN_CAP) that fits `room` bytes behind the other regions
  __host__ __device__ static uint32_t clean_cap_in(size_t room) {
    const size_t n = (room / (EMIT_WAVES * 2u)) & ~(size_t)63;
    return n < (size_t)CLEAN_CAP ? (uint32_t)n : (uint32_t)CLEAN_CAP;
  }
};

// Orders one wave's LDS writes before its later LDS reads by other lanes (wave-private staging rows).  Wavefront scope:
// the LDS executes one wave's operations in issue order, so only the compiler has to be held back -- a workgroup-scope
// fence would also wait for every global store the wave has in flight (s_waitcnt vmcnt(0)), several times per read group.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A workgroup barrier for what its waves hand each other through LDS only: their LDS operations are ordered, their
// global loads and stores stay in flight across it (__syncthreads() waits for those too: s_waitcnt vmcnt(0)).
__device__ __forceinline__ void block_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Byte offset of read t's record in its mate's text: base of its segment of 2^seg_shift blocks + base of its block of
// 256 reads inside the segment + prefix inside the block (fragment_kernel, block_base_kernel)
__device__ __forceinline__ uint64_t rec_offset(const DevBatch& B, uint32_t m, uint32_t t) {
  const uint32_t blk = t >> 8;
  const uint64_t* segbase = (const uint64_t*)((const uint8_t*)B.totals + kTotalsSegBase);
  return segbase[m * 16u + (blk >> B.seg_shift)] + B.blkbase[(size_t)m * ((B.n_slots + 255u) >> 8) + blk] +
         B.recloc[(size_t)m * B.n_slots + t];
}

// The window that owns slot t: the last one that starts at or before it (empty windows share their slot_base with the
// next window that owns slots), over win_slot[0 .. n_windows].  `from`: a window known to start at or before t --
// fragment_kernel looks among 257 staged first slots block-wise and comes here from the last of them.
__device__ __forceinline__ uint32_t slot_window(const DevBatch& B, uint32_t t, uint32_t from = 0u) {
  uint64_t lo = from, hi = B.n_windows;  // win_slot[lo] <= t < win_slot[hi]
  while (lo + 1u < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (B.win_slot[mid] <= t) lo = mid; else hi = mid;
  }
  return (uint32_t)lo;
}

__device__ __forceinline__ uint32_t aux_draw(const DevBatch& B, uint32_t slot, uint32_t j, uint32_t f, uint32_t mate) {
  uint32_t x[4];
  philox4x32_10(slot + B.slot_offset, j, f >> 2, dev_ctx(KIND_AUX, mate, B.batch_id), B.k0, B.k1, x);
  uint32_t l = f & 3;
  return l == 0 ? x[0] : l == 1 ? x[1] : l == 2 ? x[2] : x[3];
}

__device__ __forceinline__ uint32_t ndigits(uint32_t v) {
  return v < 10 ? 1 : v < 100 ? 2 : v < 1000 ? 3 : v < 10000 ? 4 : v < 100000 ? 5 : v < 1000000 ? 6
       : v < 10000000 ? 7 : v < 100000000 ? 8 : v < 1000000000 ? 9 : 10;
}

// ------------------------------------------------------------------------------------------------
// Read names "@popu#chr#pos%segsize#fragCount[/m]\n" (Segment.cpp:780,809,824).  emit_fast_kernel stores the names of
// its reads itself (phase 0: the batch's prefix from the kernel arguments + the read's part from its row) when the
// prefix fits 16 bytes; header_kernel (one lane per read, after the offset scan) serves the generic emit kernel and
// longer prefixes.
// ------------------------------------------------------------------------------------------------
// any name, byte stream -> unaligned dword stores (7 instead of 27 byte stores per record)
// (out of line in each of the two files that call it: device code is not linked across files)
__device__ __attribute__((noinline)) inline void write_name(uint8_t* hp, const uint8_t* __restrict__ prefix, uint32_t prefix_len,
                                                            uint32_t namepos, uint32_t fragcount, uint32_t paired, uint32_t m) {
  uint32_t w = 0, nb = 0;
  auto push = [&](uint32_t b) {
    w |= b << (nb * 8u);
    if (++nb == 4u) { __builtin_memcpy(hp, &w, 4); hp += 4; w = 0; nb = 0; }
  };
  auto push_dec = [&](uint32_t v) {  // digits generated least-significant first into a byte queue
    const uint32_t nd = ndigits(v);
    uint64_t lo = 0;  // last (up to 8) digits, most significant in byte 0
    uint32_t hi = 0;  // leading digits of 9- and 10-digit numbers
    for (uint32_t k = 0; k < nd; k++) {
      const uint32_t qd = v / 10u, d = '0' + (v - qd * 10u);
      if (k < 8u) lo = (lo << 8) | d; else hi = (hi << 8) | d;
      v = qd;
    }
    for (uint32_t k = 8; k < nd; k++) { push(hi & 0xFFu); hi >>= 8; }
    for (uint32_t k = 0; k < (nd < 8u ? nd : 8u); k++) { push((uint32_t)lo & 0xFFu); lo >>= 8; }
  };
  for (uint32_t i = 0; i < prefix_len; i++) push(prefix[i]);
  push_dec(namepos);
  push('#');
  push_dec(fragcount);
  if (paired) { push('/'); push('1' + m); }
  push('\n');
  for (uint32_t i = 0; i < nb; i++) hp[i] = (uint8_t)(w >> (8u * i));
}

// Which read groups a wave does.  The groups of a mate are cut into eight contiguous partitions, one per XCD (workgroups
// go to the XCDs round-robin by their linear id: x % 8; a grid that is not a multiple of eight gets one partition): the
// workgroups of an XCD work through ONE eighth of the haplotype and of the text, whose lines then live in that XCD's L2.
// Inside its partition a wave takes its first group by position and every further one from the partition's counter
// (CUs and waves do not run at one speed; with a static stride the grid drained 18 % late), then from the other
// partitions' counters.  One counter per partition,
// each in a cache line of its own, because one address serves ~85 M atomics per second: a single counter per mate was
// the ceiling of the whole kernel for 75-base reads (410 k groups per C2 pass = 4.8 ms whatever the groups cost).
struct GroupRuns {
  uint32_t* counters;        // this kernel's and mate's eight counters, 32 words apart
  uint32_t ngroups, P, part, tried, waves_per_part;
  uint32_t g;                // the wave's current group (uniform); valid while more()
  bool ok;
  __device__ __forceinline__ uint32_t lo(uint32_t p) const { return (uint32_t)((uint64_t)ngroups * p / P); }
  __device__ __forceinline__ GroupRuns(uint64_t* totals, uint32_t kernel, uint32_t mate, uint32_t n, uint32_t wv, uint32_t waves_per_wg) {
    ngroups = n;
    P = (gridDim.x & 7u) == 0u ? 8u : 1u;
    part = P == 8u ? blockIdx.x & 7u : 0u;
    tried = 0;
    waves_per_part = (gridDim.x / P) * waves_per_wg;
    counters = (uint32_t*)((uint8_t*)totals + 128) + (kernel * 2u + mate) * 8u * 32u;
    g = lo(part) + (P == 8u ? blockIdx.x >> 3 : blockIdx.x) * waves_per_wg + wv;
    ok = g < lo(part + 1u);
  }
  __device__ __forceinline__ bool more() const { return ok; }
  // the next group: from the own partition's counter; when that is exhausted, from the next partition's (the XCDs do not
  // finish together either), until all eight have been tried
  __device__ __forceinline__ void next(uint32_t lane) {
    for (;;) {
      uint32_t nx = 0;
      if (lane == 0u) nx = atomicAdd(counters + part * 32u, 1u);
      nx = (uint32_t)__builtin_amdgcn_readfirstlane((int)nx);
      const uint32_t first_dyn = lo(part) + waves_per_part, end = lo(part + 1u);
      g = first_dyn + nx;
      if (first_dyn < end && nx < end - first_dyn) { ok = true; return; }
      part = part + 1u == P ? 0u : part + 1u;
      if (++tried >= P) { ok = false; return; }
    }
  }
};

// the straight-line kernel's TI: 8-base items per read of the profile's own length that its lane map holds
inline uint32_t fast_items_per_read(const DevProfile& P) {
  const uint32_t TI = ((uint32_t)P.L + 7u) / 8u;
  return TI > 64u ? 64u : TI;  // longer reads finish in steps of their own
}
// sg_emit_fast.hip: the straight-line kernel's launch (grid, lane map reciprocal, the four instantiations)
void launch_emit_fast(const DevProfile& P, const DevBatch& B, const EmitPath& path, hipStream_t s);

}  // namespace sg
