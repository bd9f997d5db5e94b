// sg_emit_fast.hip -- emit_fast_kernel, the straight-line emit kernel of the common profile shape, and its launch.
// The generic and slow emit kernels, which share sg_emit.h with it, are in sg_kernels.hip.
//
// ------------------------------------------------------------------------------------------------
// emit, straight-line variant for the common profile shape (kmer == 3, tables in LDS).  Same results as
// emit_kernel, far fewer instructions.  Cost model (tools/valu_microbench.hip, 4 waves per SIMD): only
// add / sub / and / or / xor / right shift / mov issue at 2.3 cycles per wave instruction (v_bitop3_b32 2.8);
// compares, selects, left shifts, bit-field extracts, multiplies and every other three-operand integer op take
// 4.2.  The 8-base block is therefore written in subtractions, right shifts and three-input boolean ops:
//   * the 13 source codes of an item are packed 2 bits each (natural order A0 C1 T2 G3) into one word, so a
//     k-mer context is a shift and a mask; the tables are laid out for that digit order on the host;
//   * per base ONE 32-bit draw (the "heads" word): 12 bits decide "no substitution" against the context row's
//     keep count (identity-first rows: one subtraction, the sign is the answer), 20 bits pick an alias column of
//     the (reference == called) quality row and the side of its threshold (again a subtraction; the sign,
//     extended over the high bits, selects the symbol through a three-input boolean op);
//   * a base the heads cannot decide -- a substitution (0.35 % of the bases), a head equal to a threshold's --
//     sets a flag bit; flagged bases are redone exactly by the fix-up loop after the block (full rows from L2,
//     the "tails" Philox call only for a head on a threshold);
//   * table addresses come from a per-item look-up row (bin offsets of the item's eight positions; the short
//     contexts of a read's first two bases are table regions of their own, selected by that row);
//   * a group's reads walk three loops of steps, 64 items per step: the plain reads (no indel, the profile's own length)
//     their own stream, the items of one-indel reads that lie wholly before or behind the indel a list of their own
//     (the plain step with computed bins and a shifted template), everything else one general stream ordered by
//     event class;
//   * what is per read rather than per item: the name goes out at phase 0 (lane = read; prefix from the kernel
//     arguments, the read's own part from its row), the partial last item, "\n+\n" and '\n' are stored by a per-read
//     pass once per group (the last item waits in the read's own LDS row);
//   * windows holding a non-ACGT base and items two sequencing indels reach into (both rare) go to a global
//     queue for emit_slow_kernel.
//
// The file, top to bottom: the 8-base block (sample1, sample8); the workgroup's constants and the wave's context
// (FastBlock, FastWave); the pieces every step shares (window fetch and decode, heads8, pipelined_steps); the two
// flushes and push_fix; phase 0 (stage_tables, store_name, open_group); the group's classification and lists
// (split_one_indel_reads, classify_group, compose_lists); the plain16, plain8 and clean steps; the general step
// (item_events, item_codes, item_bins, store_item, fast_item, general_step) with its loop and the loop past the map;
// the per-read tail pass; emit_fast_kernel, which calls them in that order; launch_emit_fast.
// The read row and the LDS layout are stated in sg_emit.h (ReadRow, FastRow, FastRows, FastLds).
// ------------------------------------------------------------------------------------------------
#include "sg_emit.h"

namespace sg {

__device__ __forceinline__ uint32_t pack4(uint32_t w) {  // four code bytes (0..3) -> 8 bits
  return (w | (w >> 6) | (w >> 12) | (w >> 18)) & 0xFFu;
}

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define FAST_CTX 192u  // context rows per bin: [0,64) three bases, [64,128) two bases (x4), [128,192) one base (x16)

// v_bitop3_b32 truth tables, f(a, b, c) evaluated on a = 0xF0, b = 0xCC, c = 0xAA
#define BITOP_OR_AND 0xF8       // a | (b & c)
#define BITOP_XOR_AND 0x78      // a ^ (b & c)
#define BITOP_ANDN_OR 0xBA      // (a & ~b) | c

// "tails" word of output position i0 + h (KIND_BASE call (2c + h/4, 1)); rare, kept out of line
__device__ __noinline__ uint32_t tail_word(uint32_t slot, uint32_t c, uint32_t h, uint32_t c3b, uint32_t k0, uint32_t k1) {
  uint32_t y[4];
  philox_base(slot, 2u * c + (h >> 2), 1u, c3b, k0, k1, y);
  const uint32_t l = h & 3u;
  return l == 0u ? y[0] : l == 1u ? y[1] : l == 2u ? y[2] : y[3];
}

// one base of the 8-base block (sample8 below)
template <int H>
__device__ __forceinline__ void sample1(uint32_t col_sh, uint32_t col_mask, uint32_t cw, uint32_t wh, uint32_t so_h, uint32_t qo_h, uint32_t cd4_w,
                                        uint32_t& acc, uint32_t& sy) {
  // so_h, qo_h are absolute LDS byte addresses (the image's own address is part of them: the look-up rows hold it, the
  // arithmetic paths add it), read through integer-made LDS pointers: with a pointer base in the expression every
  // address cost an instruction more (an add of the base, a constant the compiler only learns at link time)
  typedef const __attribute__((address_space(3))) uint32_t* lds_word;
  // substitution: sure "none" iff the 16-bit head (high half) is below the row's keep count: d_s = keep_h - 1 - head >= 0
  const uint32_t kv4 = (cw >> (2 * H + 4)) & 0xFCu;   // the context's row word, as a byte offset
  const uint32_t keepm1 = *(lds_word)(uintptr_t)(so_h + kv4);
  const uint32_t d_s = keepm1 - (wh >> 16);
  // quality: alias column (col, cd) of the diagonal row; its low half holds col : thr_head, so the draw's low half minus
  // it is d_q = u_head - thr_head: negative -> lo, positive -> hi, zero -> the tail decides (fix-up)
  // (column * 16 by a right shift and a mask: both issue at the full rate, a bit-field extract and a left shift do not)
  const uint32_t col16 = (wh >> col_sh) & col_mask;
  const uint32_t qa = qo_h + ((cd4_w >> (8 * (H & 3))) & 0xFFu);
  const uint32_t e = *(lds_word)(uintptr_t)(qa + col16 + FAST_CTX * 4u);
  const uint32_t d_q = (wh & 0xFFFFu) - (e & 0xFFFFu);
  // flag (bits 17.. are copies of it): substitution possible (d_s < 0) or head on the threshold (d_q == 0)
  const uint32_t z = __builtin_amdgcn_bitop3_b32(d_q - 1u, d_q, d_s, BITOP_ANDN_OR);
  acc = __builtin_amdgcn_bitop3_b32(acc, z, 1u << (17 + H), BITOP_OR_AND);
  // symbol = hi ^ ((lo ^ hi) & (d_q < 0)), fields at bits 24.. and 16..: lands in byte 2 (the image holds the symbols as
  // characters: the profile's lowest quality character is added on the host)
  sy = __builtin_amdgcn_bitop3_b32(e >> 8, e, d_q, BITOP_XOR_AND);
}

// The 8-base block of the straight-line kernels: eight positions' substitution and quality decisions from their heads
// words.  Written for few instructions and, where there is a choice, for the ones that issue at the full rate (add, sub,
// and/or/xor, right shifts: 2.3 cycles against 4.2, tools/valu_microbench.hip): 16-bit fields that operand selects (SDWA)
// pick for free, byte permutes for packing, shift + mask instead of bit-field extract + left shift.
//   cw   13 source codes, 2 bits each (output positions i0-5 .. i0+7)      x[h]  heads word of position i0 + h
//   so[h] LDS byte address of position h's bin in the table image (+ the short-context region of a read's first two bases),
//   qo0/qo1 the plain bin addresses of positions 0 and 1
// Out: sw = the eight called characters (= the reference bases), qw = the eight quality characters, acc bit 17 + h = the
// head could not decide base h (possible substitution, or a head equal to a threshold's): the fix-up pass redoes it.
__device__ __forceinline__ void sample8(const uint32_t* code4, uint32_t lgW, uint32_t cw, const uint32_t (&x)[8],
                                        const uint32_t (&so)[8], uint32_t qo0, uint32_t qo1, uint32_t (&sw)[2], uint32_t (&qw)[2],
                                        uint32_t& acc_out) {
  // the items's eight reference codes as bytes code * 4 (alias column offset, and >> 2 the character selector)
  const uint32_t cd4[2] = {code4[(cw >> 10) & 0xFFu], code4[(cw >> 18) & 0xFFu]};
  const uint32_t col_sh = 12u - lgW, col_mask = ((1u << lgW) - 1u) << 4;   // (lgW <= 7)
  uint32_t acc = 0, sy[8];
  sample1<0>(col_sh, col_mask, cw, x[0], so[0], qo0, cd4[0], acc, sy[0]);
  sample1<1>(col_sh, col_mask, cw, x[1], so[1], qo1, cd4[0], acc, sy[1]);
  sample1<2>(col_sh, col_mask, cw, x[2], so[2], so[2], cd4[0], acc, sy[2]);
  sample1<3>(col_sh, col_mask, cw, x[3], so[3], so[3], cd4[0], acc, sy[3]);
  sample1<4>(col_sh, col_mask, cw, x[4], so[4], so[4], cd4[1], acc, sy[4]);
  sample1<5>(col_sh, col_mask, cw, x[5], so[5], so[5], cd4[1], acc, sy[5]);
  sample1<6>(col_sh, col_mask, cw, x[6], so[6], so[6], cd4[1], acc, sy[6]);
  sample1<7>(col_sh, col_mask, cw, x[7], so[7], so[7], cd4[1], acc, sy[7]);
  // byte 2 of four symbols words -> one word (selector bytes: 0-3 from the second operand, 4-7 from the first)
#pragma unroll
  for (int g = 0; g < 2; g++) {
    const uint32_t p01 = __builtin_amdgcn_perm(sy[4 * g + 1], sy[4 * g], 0x0C0C0602u);
    const uint32_t p23 = __builtin_amdgcn_perm(sy[4 * g + 3], sy[4 * g + 2], 0x06020C0Cu);
    qw[g] = p01 | p23;
    // called bases = reference bases: code -> character
    sw[g] = __builtin_amdgcn_perm(0u, 0x47544341u, cd4[g] >> 2);  // "ACTG"
  }
  acc_out = acc;
}

// n (< 16) bytes of the 128-bit value (lo, hi) to q, as TWO overlapping pieces of the largest power of two <= n: its
// first bytes and its last (one piece when n is that power).  (Lane = record here: every store instruction touches 64 different lines, so the number of
// pieces is what these stores cost; 8/4/2/1-byte pieces made three or four of a 15-byte name.)
__device__ __forceinline__ void store_var(uint8_t* q, uint64_t lo, uint64_t hi, uint32_t n) {
  if (n >= 8u) {
    __builtin_memcpy(q, &lo, 8);
    if (n > 8u) {
      const uint32_t k = 8u * (n - 8u);   // bit offset of the last eight bytes (8 .. 56)
      const uint64_t v = (lo >> k) | (hi << (64u - k));
      __builtin_memcpy(q + n - 8u, &v, 8);
    }
  } else if (n >= 4u) {
    const uint32_t a = (uint32_t)lo, b = (uint32_t)(lo >> (8u * (n - 4u)));
    __builtin_memcpy(q, &a, 4);
    if (n > 4u) __builtin_memcpy(q + n - 4u, &b, 4);
  } else if (n >= 2u) {
    const uint16_t a = (uint16_t)lo, b = (uint16_t)(lo >> (8u * (n - 2u)));
    __builtin_memcpy(q, &a, 2);
    if (n > 2u) __builtin_memcpy(q + n - 2u, &b, 2);
  } else if (n == 1u) {
    *q = (uint8_t)lo;
  }
}

// ------------------------------------------------------------------------------------------------
// The workgroup's constants and the wave's context
// ------------------------------------------------------------------------------------------------
// Lane -> (read, item) map over the first TI = ceil(L / 8) items of a group's G = 63 reads: their items form one
// stream, 64 per step: lane l of step s does stream item i = 64 s + l = item i % TI of the (i / TI)-th read in step
// order; every lane busy whatever TI is (63 reads, so that TI steps hold the 63 TI map items plus up to TI appended
// ones).  inv_TI = ceil-reciprocal of TI.
constexpr uint32_t FAST_G = 63u;

// What is the same for every wave and group of a workgroup.
template <bool PAIRED, bool DIAG>
struct FastBlock {
  const DevProfile& P;
  const DevBatch& B;
  uint32_t m, tm;        // mate; the mate whose tables are sampled
  uint32_t dg;           // SG_FDIAG timing ablations: compiled out of the production kernel
  uint32_t bins, TI, inv_TI, clean_cap;
  uint32_t img_at;       // the table image's LDS byte address
  const uint32_t* lut;
  const uint32_t* code4;
  // Items per plain read that run through the plain steps: all but the last one, whose store is partial and followed by the
  // record separators -- unless the last item holds seven bases (L % 8 == 7, the 151-base profile): with the line break as
  // its eighth byte it is a whole item like the others, plus the two bytes of the "+" line.  (No fewer instructions that
  // way, but the record's last bytes leave with their neighbours instead of fifteen steps later, when the line has left
  // L2: WRITE_SIZE 6.43 -> see profiles/r03_final.)
  bool tail_whole;
  uint32_t TIp;
  // 16-base items per plain read (the plain16 steps below).  A whole last item of seven bases (tail_whole) carries the line
  // break and the "+" line and only the 8-base steps write those: it stays out of the pairs (L = 303: 38 items, 18 pairs +
  // items 36 and 37 on their own; found by fuzz seeds 222 / 224, whose 303-base reads lost their line break to a sixteenth base)
  uint32_t TI16, inv_TI16;   // inv_TI16: ceil-reciprocal (i / TI16 exact while i * TI16 < 2^20)

  __device__ __forceinline__ FastBlock(const DevProfile& P_, const DevBatch& B_, uint32_t m_, uint32_t TI_, uint32_t inv_TI_,
                                       uint32_t clean_cap_, uint32_t img_at_, const uint32_t* lut_, const uint32_t* code4_)
      : P(P_), B(B_), m(m_), tm(PAIRED ? m_ : 0u), dg(DIAG ? B_.diag : 0u), bins((uint32_t)P_.bins), TI(TI_), inv_TI(inv_TI_),
        clean_cap(clean_cap_), img_at(img_at_), lut(lut_), code4(code4_) {
    tail_whole = ((uint32_t)P.L & 7u) == 7u && ((uint32_t)P.L + 7u) / 8u == TI;
    TIp = tail_whole ? TI : TI - 1u;
    TI16 = (tail_whole ? TIp - 1u : TIp) >> 1;
    inv_TI16 = TI16 ? (1u << 20) / TI16 + 1u : 0u;
  }
  // does a read walk the reverse-complement 2-bit copy?  (paired: mate 2; single end: the row's own bit)
  __device__ __forceinline__ bool rc(bool row_bit) const { return PAIRED ? m == 1u : row_bit; }
  // ---- window fetch: the eight bytes of the 2-bit copy (forward or reverse complement) that hold base index idx ----
  __device__ __forceinline__ uint2 fetch_window(bool row_bit, uint32_t idx) const {
    uint2 v;
    fetch_window(row_bit, idx, v);
    return v;
  }
  // (over a window at hand, for item_codes' conditional refetch.  The window stays a uint2 filled by memcpy: as a 64-bit
  // scalar, or refetched by assigning the value above, the compiler read it through a pointer that was either the step's
  // prefetched window or the copy, and the prefetched window then lived in scratch memory in the SG_FDIAG instantiations
  // -- private segment 64 -> 80 bytes)
  __device__ __forceinline__ void fetch_window(bool row_bit, uint32_t idx, uint2& into) const {
    __builtin_memcpy(&into, (rc(row_bit) ? B.chains2_rc : B.chains2_fwd) + (idx >> 2), 8);
  }
  __device__ __forceinline__ uint32_t c3b() const { return dev_ctx(KIND_BASE, m, B.batch_id); }
};

// ---- window decode: the codes from base index idx on, 2 bits each, lowest first (an item uses 26 bits: positions
// 8c - 5 .. 8c + 7; a 16-base item 42) ----
__device__ __forceinline__ uint64_t window_codes(uint2 w, uint32_t idx) { return (((uint64_t)w.y << 32) | w.x) >> (2u * (idx & 3u)); }

// One wave's view of its current read group.
struct FastWave {
  uint32_t lane;
  FastRows rows;           // the group's read rows
  uint32_t* slow_list;     // items for emit_slow_kernel's queue (read | item << 8), nslow of them
  uint2* fix_list;         // flagged items (read | flags << 6 | item << 17, packed codes), nfix of them
  uint8_t* perm;           // the general stream's reads in step order
  uint8_t* permp;          // the plain reads, in lane order
  uint16_t* ovf;           // single items of the general stream (read | item << 8)
  uint16_t* clean;         // clean items of one-indel reads (read | after << 6 | item << 7)
  uint32_t g;              // the group (wave-uniform)
  uint8_t* gout;           // the group's first record in the mate's text
  __amdgpu_buffer_rsrc_t out_rsrc;   // buffer descriptor on gout: the records at 32-bit offsets (FastRow::out_off)
  uint32_t nslow, nfix;    // wave-uniform
  __device__ __forceinline__ unsigned long long lanes_below() const { return (1ull << lane) - 1ull; }
};

// ---- heads draws: two Philox calls, the heads words of an item's eight positions (call = i/4, word = i%4).
// slot: the read's Philox address (batch slot + DevBatch::slot_offset) ----
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void heads8(const FastBlock<PAIRED, DIAG>& k, uint32_t slot, uint32_t c, uint32_t (&x)[8]) {
  const uint32_t c3b = k.c3b();
  if (k.dg & 8u) {  // ablation: no Philox
#pragma unroll
    for (int z = 0; z < 8; z++) x[z] = (slot * 2654435761u) ^ (c * 40503u + z * 0x9E3779B9u);
  } else {
    philox_base(slot, 2u * c, 0, c3b, k.B.k0, k.B.k1, x);
    philox_base(slot, 2u * c + 1u, 0, c3b, k.B.k0, k.B.k1, x + 4);
  }
}

// A step loop.  A step's lane -> (read, item) map, its read rows and its haplotype window are fetched ONE STEP AHEAD (the
// chain LDS -> LDS -> L2 is ~1000 cycles; issued before the previous step's sampling it is covered by it).  The caller
// fetches step `first` into `cur` and issues its dropped stores behind that fetch, so that the loop is entered with the
// same vector-memory operations behind the first prefetch as every later iteration has behind its own.
// (the last step fetches itself again: an unconditional fetch keeps the loaded registers free of copies until
// the end of the iteration, so the wait for them sits after this step's sampling)
template <class S, class Fetch, class Run>
__device__ __forceinline__ void pipelined_steps(S cur, uint32_t first, uint32_t last, Fetch fetch, Run run) {
  for (uint32_t step = first; step < last; step++) {
    const S nxt = fetch(min(step + 1u, last - 1u));
    run(cur);
    cur = nxt;
  }
}

// ------------------------------------------------------------------------------------------------
// The two flushes and the fix-up list's push
// ------------------------------------------------------------------------------------------------
// Items the straight-line code cannot do (non-ACGT window, >= 2 indels) go to the batch's global
// queue: one atomic per flush reserves the range; emit_slow_kernel runs the generic code on them
// afterwards.  Keeping that code out of this kernel is worth ~14 % (SGPR spills, I-cache).
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void flush_slow(const FastBlock<PAIRED, DIAG>& k, FastWave& w) {
  const DevBatch& B = k.B;
  const uint32_t m = k.m, lane = w.lane;
  wave_lds_sync();
  uint32_t base = 0;
  if (lane == 0u) base = atomicAdd(B.slowq_count + m, w.nslow);
  base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
  for (uint32_t b0 = 0; b0 < w.nslow; b0 += 64u) {
    const uint32_t i = b0 + lane;
    if (i < w.nslow && base + i < B.slowq_cap) {
      const uint32_t e = w.slow_list[i];
      B.slowq[(size_t)m * B.slowq_cap + base + i] = make_uint2(w.g * FAST_G + (e & 0xFFu), e >> 8);
    }
  }
  if (lane == 0u && base + w.nslow > B.slowq_cap) atomicOr((unsigned long long*)(B.totals + 3), 2ull);
  w.nslow = 0;
  wave_lds_sync();
}

// The fix-up pass, lane = flagged base: the bases the heads could not decide (a possible substitution, a head equal
// to a threshold's) are sampled again exactly -- full identity-first row and alias column from L2, the tails call
// only when a head sits on a threshold -- and patched into the text already stored (or into the parked last item).
// Run once per read group (and whenever the list fills): one pass serves ~40 flagged bases, where a loop inside the
// step would run for one or two lanes in five steps out of six.
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void flush_fix(const FastBlock<PAIRED, DIAG>& k, FastWave& w) {
  const DevProfile& P = k.P;
  const DevBatch& B = k.B;
  const uint32_t bins = k.bins, lane = w.lane;
  wave_lds_sync();
  // the items' own stores must have landed before single bytes of them are rewritten
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  const uint32_t lgW = P.lgW, u_mask = (1u << (16u - lgW)) - 1u;
  const uint4* gsub = P.fast_sub + (size_t)k.tm * bins * FAST_CTX;
  const uint32_t c3b = k.c3b();
  for (uint32_t b0 = 0; b0 < w.nfix; b0 += 64u) {
    // lane = flagged item: read | flags of its eight bases << 6 | item << 17, packed codes; its bases one after the
    // other (nine items in ten have one flagged base, so the loop body nearly always runs once per 64 items)
    const uint2 fe = w.fix_list[b0 + lane < w.nfix ? b0 + lane : 0u];
    uint32_t todo = b0 + lane < w.nfix ? (fe.x >> 6) & 0xFFu : 0u;
    const uint32_t r = fe.x & 63u, c = fe.x >> 17, cw = fe.y;
    const uint32_t slot = w.g * FAST_G + r + B.slot_offset;
    const FastRow rr = w.rows.load(r);
    const uint32_t np = rr.np(), hl = rr.hdr_len();
    // stored like a whole item (a last item of seven bases included), or the read's parked last item?
    const bool whole = 8u * c + 8u <= np + (uint32_t)((np & 7u) == 7u);
    // ceil(2^32 / n') again (fragment_kernel's row word): a read's parked last item has overwritten it in the row
    const uint32_t inv = row::inv_of(max(np, 1u));
    while (__ballot(todo != 0u) != 0ull) {
      const bool on = todo != 0u;
      const uint32_t h = on ? (uint32_t)__builtin_ctz(todo) : 0u;
      todo &= todo - 1u;
      const uint32_t i = 8u * c + h;
      const uint32_t bin = __umulhi(__umul24(i, bins), inv);
      uint32_t xw[4];
      philox_base(slot, 2u * c + (h >> 2), 0, c3b, B.k0, B.k1, xw);
      const uint32_t l = h & 3u;
      const uint32_t wh = l == 0u ? xw[0] : l == 1u ? xw[1] : l == 2u ? xw[2] : xw[3];
      const uint32_t region = c == 0u ? (h == 0u ? 128u : h == 1u ? 64u : 0u) : 0u;
      const uint32_t cdn = (cw >> (2u * h + 10u)) & 3u;
      const uint4 row = gsub[(size_t)bin * FAST_CTX + region + ((cw >> (2u * h + 6u)) & 63u)];
      // identity-first row on the 16-bit head: certain unless the head equals a threshold's
      const uint32_t sh = wh >> 16, h0 = row.x >> 16, h1 = row.y >> 16, h2 = row.z >> 16;
      const uint32_t jj = (uint32_t)(sh > h0) + (uint32_t)(sh > h1) + (uint32_t)(sh > h2);
      const bool amb_s = on && jj != (uint32_t)(sh >= h0) + (uint32_t)(sh >= h1) + (uint32_t)(sh >= h2);
      uint32_t kn = 0;
      uint2 e2 = make_uint2(0, 0);
      const uint32_t col = (wh & 0xFFFFu) >> (16u - lgW), uh = wh & u_mask;
      auto column = [&](uint32_t j_) {
        const uint32_t jm = max(j_, row.w & 3u);
        kn = (row.w >> (2u * jm + 2u)) & 3u;
        e2 = P.fast_alias[((((size_t)cdn * 4u + kn) * bins + bin) << lgW) + col];
      };
      if (!amb_s) column(jj);
      const bool need_tail = amb_s || (on && uh == (e2.x >> 16) && (e2.y & 0xFFu) != (e2.y >> 8));
      uint32_t wt = 0;
      if (__ballot(need_tail) != 0ull) {
        if (need_tail) wt = tail_word(slot, c, h, c3b, B.k0, B.k1);
      }
      if (__ballot(amb_s) != 0ull) {
        if (amb_s) {
          const uint32_t xs = (wh & 0xFFFF0000u) | (wt >> 16);
          column((uint32_t)(xs > row.x) + (uint32_t)(xs > row.y) + (uint32_t)(xs > row.z));
        }
      }
      // side of the column: the head decides unless it sits on the threshold's (then the 16-bit tail does)
      const uint32_t th = e2.x >> 16;
      const bool lo_side = uh != th ? uh < th : ((uh << 16) | (wt & 0xFFFFu)) < e2.x;
      const uint32_t sym = (lo_side ? (e2.y & 0xFFu) : (e2.y >> 8)) + (uint32_t)P.min_qual;
      const uint32_t ch = (0x47544341u >> (8u * kn)) & 0xFFu;  // "ACTG"[kn]: natural code -> character
      if (on) {
        if (whole) {
          uint8_t* rec = w.gout + rr.out_off() + hl + i;
          rec[0] = (uint8_t)ch;
          rec[np + 3u] = (uint8_t)sym;
        } else if (!rr.parked_slow()) {
          w.rows.patch_parked(r, h, ch, sym);   // the read's parked last item
        }
      }
    }
  }
  w.nfix = 0;
  wave_lds_sync();
}

// flagged items -> the group's fix-up list: read | flags of the eight bases << 6 | item << 17 (items < 2^15), packed
// codes.  One entry per item whatever the number of its flagged bases: no loop in the step.
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void push_fix(const FastBlock<PAIRED, DIAG>& k, FastWave& w, uint32_t r, uint32_t c, uint32_t fix, uint32_t cw) {
  const unsigned long long fm = __ballot(fix != 0u);
  if (fm) {
    if (w.nfix + 64u > FIX_CAP) flush_fix(k, w);
    if (fix != 0u) w.fix_list[w.nfix + (uint32_t)__popcll(fm & w.lanes_below())] = make_uint2(r | (fix << 6) | (c << 17), cw);
    w.nfix += (uint32_t)__popcll(fm);
  }
}

// ------------------------------------------------------------------------------------------------
// Phase 0: the workgroup's tables, then per group lane = read: names, the group's descriptor, the rows
// ------------------------------------------------------------------------------------------------
// the table image, the look-up rows and the code table into LDS, by the whole workgroup
__device__ __forceinline__ void stage_tables(const DevProfile& P, uint32_t tm, uint32_t TI, uint32_t* img, uint32_t img_at,
                                             uint32_t* lut, uint32_t* code4) {
  const uint32_t tid = threadIdx.x, bins = (uint32_t)P.bins, img_words = bins * P.fast_stride;
  const uint4* src = (const uint4*)(P.fast_lds + (size_t)tm * P.fast_mate_words);  // 16-byte aligned on the host
  for (uint32_t i = tid; i < (img_words + 3u) / 4u; i += EMIT_THREADS) ((uint4*)img)[i] = src[i];
  // look-up rows for reads of the profile's own length: bin = i * binCount / L (Profile.cpp:1672)
  const uint32_t blk_bytes = P.fast_stride * 4u;
  for (uint32_t i = tid; i < TI * LUT_ROW; i += EMIT_THREADS) {
    const uint32_t c = i / LUT_ROW, f = i - c * LUT_ROW;
    const uint32_t h = f < 8u ? f : f - 8u;
    const uint32_t pos = 8u * c + h;
    const uint32_t bin = min(pos * bins / (uint32_t)P.L, bins - 1u);
    uint32_t v = bin * blk_bytes;
    if (f < 8u && c == 0u) v += f == 0u ? 128u * 4u : f == 1u ? 64u * 4u : 0u;
    lut[i] = f < 10u ? v + img_at : 0u;
  }
  for (uint32_t i = tid; i < 256u; i += EMIT_THREADS) {
    uint32_t v = 0;
    for (uint32_t z = 0; z < 4u; z++) v |= (((i >> (2u * z)) & 3u) * 4u) << (8u * z);
    code4[i] = v;
  }
}

// The read's name, stored in front of where the step loop will put the bases: the batch's prefix, then the
// read's own part from its row (fragment_kernel made the text), two pieces of <= 16 bytes.  (B.prefix_len <= 16)
template <bool PAIRED>
__device__ __forceinline__ void store_name(const DevBatch& B, uint32_t m, const ReadRow& my, size_t idx, uint8_t* rec) {
  const uint32_t nv = my.hdr_len() - B.prefix_len;
  if (__builtin_expect(nv > 16u, 0)) {
    write_name(rec, B.prefix, B.prefix_len, my.namepos(), my.fragcount(), PAIRED ? 1u : 0u, m);
    return;
  }
  const uint64_t p_lo = ((uint64_t)B.prefix_w[1] << 32) | B.prefix_w[0], p_hi = ((uint64_t)B.prefix_w[3] << 32) | B.prefix_w[2];
  const uint4 tx = B.meta[idx * 3 + 2];
  const uint64_t b0 = ((uint64_t)tx.y << 32) | tx.x, b1 = ((uint64_t)tx.w << 32) | tx.z;
  const uint32_t plen = B.prefix_len, hb = plen + nv;   // the name's bytes: prefix, then the read's own text
  if (plen < 16u && hb >= 16u && hb <= 24u) {
    // the usual case ("@sim#20#" + "592246#30000/1\n"): the name as ONE string (both parts are zero beyond their
    // ends), its first sixteen bytes and its last eight -- two stores where prefix + two text pieces were three
    // (lane = record: every store instruction touches 64 lines, and on the 75-base profiles the names and tails
    // are a quarter of the kernel's time)
    const uint32_t sh = 8u * plen;
    uint64_t w0, w1, w2;
    if (sh < 64u) {
      w0 = p_lo | (b0 << sh);
      w1 = p_hi | (b1 << sh) | (sh ? b0 >> (64u - sh) : 0ull);
      w2 = sh ? b1 >> (64u - sh) : 0ull;
    } else {
      const uint32_t t2 = sh - 64u;
      w0 = p_lo;
      w1 = p_hi | (b0 << t2);
      w2 = (b1 << t2) | (t2 ? b0 >> (64u - t2) : 0ull);
    }
    struct { uint64_t a, b; } first = {w0, w1};
    __builtin_memcpy(rec, &first, 16);
    const uint32_t n2 = hb - 16u;
    if (n2) {
      const uint32_t k = 8u * n2;
      const uint64_t v = k == 64u ? w2 : (w1 >> k) | (w2 << (64u - k));
      __builtin_memcpy(rec + hb - 8u, &v, 8);
    }
  } else {
    if (plen == 16u) { __builtin_memcpy(rec, &p_lo, 8); __builtin_memcpy(rec + 8, &p_hi, 8); }
    else store_var(rec, p_lo, p_hi, plen);
    uint8_t* q = rec + plen;
    if (nv == 16u) __builtin_memcpy(q, &tx, 16);
    else store_var(q, b0, b1, nv);
  }
}

// The group's text is one contiguous range starting at its first record: a buffer descriptor on that address, the
// records at 32-bit offsets from it (row word 2).  Offsets past 2^31 are the "no store" value of idle lanes.
// ooff: the lane's record offset in the mate's text; returns the group's.
__device__ __forceinline__ uint64_t open_group(FastWave& w, uint8_t* out, uint64_t ooff) {
  const uint64_t gbase = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(ooff >> 32)) << 32) |
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ooff);
  w.gout = out + gbase;
  w.out_rsrc = __builtin_amdgcn_make_buffer_rsrc(w.gout, 0, 0x80000000u, 0x00020000);
  return gbase;
}

// ------------------------------------------------------------------------------------------------
// The group's classification and lists
//
// The group's items go through two loops.
//  * PLAIN steps: items 0 .. TI-2 of the plain reads -- no sequencing indel, the profile's own length, no non-ACGT
//    block (84 % of the reads at XTen rates).  Every such item is eight bases stored whole, its bin offsets come from
//    the look-up row, nothing about it is conditional: the step is the 8-base block, two Philox calls and ~50
//    instructions around them (the general step: ~250).
//  * GENERAL steps: everything else as one item stream -- all items of the other reads (reads with one indel before
//    those with several, so that the two-window code and the event-list walk run in few steps), then single items: the
//    plain reads' last items (partial or followed by the separators: the per-read pass and the parked-item logic
//    belong to the general code) and the one or two items an insertion appended to a read.
//  * CLEAN steps: a read with ONE sequencing indel is, item by item, a plain read nearly everywhere -- the items wholly
//    before the event read the template unshifted, those wholly after it read it shifted by the event's length; what
//    differs from a plain item is the bin arithmetic (n' != L: no look-up row) and that shift.  Only the one to
//    three items the event reaches into, and the last, partial one, need the general code.  (Measured before this
//    split, SQ_INSTS_VALU with either loop compiled out: the general steps took 34 % of the kernel's instructions for
//    16 % of the reads -- every item of a one-indel read paid the two-window code and its insertion loop.)
// ------------------------------------------------------------------------------------------------
struct GroupPlan {
  // lane = read
  uint32_t items;          // its 8-base items (0: no read)
  bool plain_l, split_l;   // a plain read; a one-indel read whose clean items go to the clean list
  bool small;              // an insertion appended one or two items to the read
  uint32_t extra;          // items past the map (unsplit reads)
  // one-indel reads, item ranges: 0 .. kb-1 wholly before the event, ca0 .. n_whole-1 wholly after it (ka of them),
  // n_gen left for the general steps; vscan = (clean items << 16 | general items) of the candidates up to and including
  // this lane
  uint32_t kb, ca0, n_whole, ka, n_gen, vscan;
  // wave-uniform: the reads by class, the item counts of the lists
  unsigned long long m_plain, m_rest, m_one, m_multi, b1, b2;
  uint32_t n_plain, n_psingle, n_rest, n_one, n_fast, n_single, n_gen_all, n_moved;
  uint32_t n_clean, n_ovf;       // entries of the clean list and of ovf, once compose_lists has run
  unsigned long long more;       // reads with items past the map and the appended ones
};

// one-indel reads: item ranges.  fc = first output position that is not the unshifted template's, fs = first one that
// reads the shifted template (an insertion's own bases lie between the two); an item's codes span positions
// 8c - 5 .. 8c + 7
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void split_one_indel_reads(const FastBlock<PAIRED, DIAG>& k, const FastWave& w, const ReadRow& my, GroupPlan& gp) {
  const uint32_t TI = k.TI, lane = w.lane, items = gp.items, np_l = my.np();
  const bool act_l = items > 0u, plain_l = gp.plain_l;
  gp.kb = 0; gp.ca0 = 0; gp.n_whole = 0; gp.ka = 0; gp.n_gen = 0; gp.vscan = 0;
  gp.split_l = false;
  // (only where a group has enough one-indel reads for about two clean steps: with fewer the split cannot pay, see below,
  // and the other profiles' groups -- a third to a twentieth of XTen's one-indel reads -- skip its bookkeeping)
  const bool cand0_l = act_l && my.nev() == 1u && !my.bad_block();
  if (k.clean_cap != 0u && (uint32_t)__popcll(__ballot(cand0_l)) * (TI - 2u) >= 96u) {
    const uint32_t ew = my.event();
    const uint32_t ej = ew & 0xFFFFu, elen = (ew >> 16) & 0x7FFFu;
    const bool del = (ew >> 31) != 0u;
    const uint32_t fc = del ? ej : ej + 1u, fs = del ? ej : ej + elen + 1u;
    gp.n_whole = np_l >> 3;
    gp.kb = min(fc >> 3, gp.n_whole);                 // items 0 .. kb-1: wholly before
    gp.ca0 = (fs + 12u) >> 3;                         // items ca0 .. n_whole-1: wholly after (8c - 5 >= fs)
    gp.ka = gp.n_whole > gp.ca0 ? gp.n_whole - gp.ca0 : 0u;
    gp.n_gen = gp.ka ? (gp.ca0 - gp.kb) + (items - gp.n_whole) : items - gp.kb;   // what is left for the general steps
    const bool cand_l = cand0_l && items <= 255u && gp.kb + gp.ka != 0u;
    // as many of them, in lane order, as the two lists hold (behind the other single items, counted below)
    uint32_t v = cand_l ? ((gp.kb + gp.ka) << 16) | gp.n_gen : 0u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(v, d, 64);
      if ((int)lane >= d) v += up;
    }
    gp.vscan = v;   // (clean items << 16 | general items) of the candidates up to and including this lane
    const uint32_t extra_l = items > TI ? items - TI : 0u;
    const uint32_t others = (k.tail_whole ? 0u : (uint32_t)__popcll(__ballot(plain_l))) +
                            (uint32_t)__popcll(__ballot(extra_l == 1u || extra_l == 2u)) + (uint32_t)__popcll(__ballot(extra_l == 2u));
    bool split_l = cand_l && (v >> 16) <= k.clean_cap && others + (v & 0xFFFFu) <= OVF_CAP;
    // (a prefix in lane order: the sums only grow)
    // Does the split pay in this group?  Steps are whole: a few clean items make a clean step of their own, and what
    // they leave behind may still need as many general steps as before (the 125-base profile: one read in ten has one
    // indel, and every plain read sends its partial last item through the general steps anyway -- with the split
    // unconditional its launch ran 3.6 % MORE instructions).  Step counts either way from the sums at hand, priced at
    // the loops' measured instructions per step (general 390-590 by profile: 480, clean 260, composing the lists ~250).
    const unsigned long long ms = __ballot(split_l);
    if (ms) {
      const uint32_t tot_s = (uint32_t)__shfl((int)v, 63 - __builtin_clzll(ms), 64);
      const uint32_t n_cl = tot_s >> 16, n_gn = tot_s & 0xFFFFu;
      const uint32_t whole = (uint32_t)__popcll(__ballot(act_l && !plain_l && !split_l));   // reads that stay whole in the general steps
      const uint32_t s0 = (whole + (uint32_t)__popcll(ms)) * TI + others, s1 = whole * TI + others + n_gn;
      const uint32_t rem = n_cl & 63u, mv = (rem != 0u && rem <= ((0u - s1) & 63u)) ? rem : 0u;   // (the partial clean step that moves, below)
      const uint32_t before = 48u * ((s0 + 63u) >> 6);
      const uint32_t after = 26u * ((n_cl - mv + 63u) >> 6) + 48u * ((s1 + mv + 63u) >> 6) + 25u;
      if (after >= before) split_l = false;
    }
    gp.split_l = split_l;
    gp.kb = split_l ? gp.kb : 0u;
    gp.ka = split_l ? gp.ka : 0u;
    gp.n_gen = split_l ? gp.n_gen : 0u;
  }
}

// The group's reads by class and the sizes of its lists.  my, items: the lane's read (phase 0).
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ GroupPlan classify_group(const FastBlock<PAIRED, DIAG>& k, const FastWave& w, const ReadRow& my, uint32_t items) {
  GroupPlan gp;
  const uint32_t TI = k.TI;
  const uint32_t nev_l = my.nev();
  const bool act_l = items > 0u;
  gp.items = items;
  gp.plain_l = act_l && nev_l == 0u && my.np() == (uint32_t)k.P.L && items == TI && !my.bad_block() && k.TIp != 0u;
  split_one_indel_reads(k, w, my, gp);
  const bool plain_l = gp.plain_l, split_l = gp.split_l;
  const unsigned long long m_split = __ballot(split_l);
  gp.m_plain = __ballot(plain_l);
  gp.m_multi = __ballot(act_l && nev_l >= 2u);
  gp.m_one = __ballot(act_l && nev_l == 1u && !split_l);
  gp.m_rest = __ballot(act_l && !plain_l && nev_l == 0u);
  gp.n_plain = (uint32_t)__popcll(gp.m_plain);
  gp.n_psingle = k.tail_whole ? 0u : gp.n_plain;   // plain reads' last items left to the general steps
  gp.n_rest = (uint32_t)__popcll(gp.m_rest);
  gp.n_one = (uint32_t)__popcll(gp.m_one);
  gp.n_fast = gp.n_rest + gp.n_one + (uint32_t)__popcll(gp.m_multi);  // reads whose items all walk the general steps
  // TI = ceil(L / 8) exactly; a read that an insertion grew by one or two items appends them to the end of
  // the stream (they fill lanes of the last step that would idle anyway); only reads longer than that take
  // steps of their own below.
  gp.extra = (items > TI && !split_l) ? items - TI : 0u;
  gp.small = gp.extra == 1u || gp.extra == 2u;
  gp.b1 = __ballot(gp.small);
  gp.b2 = __ballot(gp.extra == 2u);
  gp.n_single = gp.n_psingle + (uint32_t)__popcll(gp.b1) + (uint32_t)__popcll(gp.b2);
  // the split reads' totals (they are the first candidates in lane order: the scan above holds their sums and offsets)
  const uint32_t tot = m_split ? (uint32_t)__shfl((int)gp.vscan, 63 - __builtin_clzll(m_split), 64) : 0u;
  gp.n_clean = tot >> 16;
  gp.n_gen_all = tot & 0xFFFFu;
  // The clean list's last, partial step: if the general stream's last step has that many idle lanes, the items go there
  // as single items (the general code does them as well) and the step is saved.  They go FIRST among the single items:
  // a read's last item is parked in its LDS row over fields its other items need (store_item), so nothing of a read may
  // follow its last item in the stream.
  gp.n_moved = 0;
  {
    const uint32_t rem = gp.n_clean & 63u, idle = (0u - (gp.n_fast * TI + gp.n_single + gp.n_gen_all)) & 63u;
    if (rem != 0u && rem <= idle && gp.n_single + gp.n_gen_all + rem <= OVF_CAP) gp.n_moved = rem;
  }
  gp.n_ovf = gp.n_moved + gp.n_single + gp.n_gen_all;
  gp.more = (k.dg & 256u) ? 0ull : __ballot(gp.extra > 2u);
  return gp;
}

// perm / permp / ovf / clean from the plan, each lane its own read's entries
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void compose_lists(const FastBlock<PAIRED, DIAG>& k, const FastWave& w, GroupPlan& gp) {
  const uint32_t TI = k.TI, lane = w.lane, items = gp.items, n_moved = gp.n_moved;
  const unsigned long long lt = w.lanes_below();
  if (items > 0u && !gp.split_l) {
    if (gp.plain_l) {
      const uint32_t pos = (uint32_t)__popcll(gp.m_plain & lt);
      w.permp[pos] = (uint8_t)lane;
      if (!k.tail_whole) w.ovf[n_moved + pos] = (uint16_t)(lane | (k.TIp << 8));   // its last item: a single item of the general stream
    } else {
      uint32_t pos;
      if ((gp.m_rest >> lane) & 1ull) pos = (uint32_t)__popcll(gp.m_rest & lt);
      else if ((gp.m_one >> lane) & 1ull) pos = gp.n_rest + (uint32_t)__popcll(gp.m_one & lt);
      else pos = gp.n_rest + gp.n_one + (uint32_t)__popcll(gp.m_multi & lt);
      w.perm[pos] = (uint8_t)lane;
    }
  }
  if (gp.n_fast == 0u && lane == 0u) w.perm[0] = 0;   // (what idle lanes of a step look at)
  if (gp.small) {
    const uint32_t o = n_moved + gp.n_psingle + (uint32_t)__popcll(gp.b1 & lt) + (uint32_t)__popcll(gp.b2 & lt);
    w.ovf[o] = (uint16_t)(lane | (TI << 8));
    if (gp.extra == 2u) w.ovf[o + 1u] = (uint16_t)(lane | ((TI + 1u) << 8));
  }
  if (gp.split_l) {
    // the split reads' items into the two lists, each lane its own ranges (one loop over both clean ranges: the wave runs
    // as many iterations as its longest lane needs, and every split read has about TI - 2 clean items however they fall
    // before and after its indel)
    const uint32_t kb = gp.kb, ka = gp.ka, ca0 = gp.ca0;
    const uint32_t oc = (gp.vscan >> 16) - (kb + ka);
    uint32_t og = n_moved + gp.n_single + (gp.vscan & 0xFFFFu) - gp.n_gen;
    const uint32_t kt = kb + ka, behind = ((ca0 - kb) << 7) | 64u;
    for (uint32_t q = 0; q < kt; q++) w.clean[oc + q] = (uint16_t)((lane | (q << 7)) + (q >= kb ? behind : 0u));
    const uint32_t mid_end = ka ? ca0 : items;
    for (uint32_t c = kb; c < mid_end; c++) w.ovf[og++] = (uint16_t)(lane | (c << 8));
    if (ka) for (uint32_t c = gp.n_whole; c < items; c++) w.ovf[og++] = (uint16_t)(lane | (c << 8));
  }
  wave_lds_sync();
  if (n_moved) {
    gp.n_clean -= n_moved;
    if (lane < n_moved) {
      const uint32_t e = w.clean[gp.n_clean + lane];
      w.ovf[lane] = (uint16_t)((e & 63u) | ((e >> 7) << 8));
    }
    wave_lds_sync();
  }
}

// ------------------------------------------------------------------------------------------------
// The plain reads' steps
//
// The plain reads' items walk two loops (round 4).  PLAIN16 steps: lane = SIXTEEN bases, items 2c and 2c + 1 of one read
// -- one map, one row fetch, one 8-byte window of the 2-bit copy (21 codes = 42 bits), two 16-byte stores for what were
// two of each; only WHOLE steps run that way.  What is left -- the 16-base items of the last, partial step, as their two
// halves, and the reads' odd last 8-base item (cnt8 = TIp mod 2) -- goes through the 8-base plain steps as one stream,
// so that neither loop ends in a step with idle lanes of its own.
// Reads of fewer than 18 whole items keep the 8-base steps alone: with four to seven pairs per read the whole 16-base steps
// cover 70 % of a group's items and the rest pays two loops' prologues -- the 125-, 75- and 74-base profiles ran 6-7 %
// SLOWER in pairs (2.75 / 3.36 / 3.41 ms against 2.59 / 3.14 / 3.18, profiles/r04_mid_all_profiles vs r03_final).
// ------------------------------------------------------------------------------------------------
struct PlainSteps {
  bool use16;
  uint32_t n_plain, np16steps, cnt8, c8_base, n_pitems, npsteps;
};
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ PlainSteps plan_plain_steps(const FastBlock<PAIRED, DIAG>& k, uint32_t n_plain) {
  PlainSteps ps;
  const uint32_t dg = k.dg, TIp = k.TIp, TI16 = k.TI16;
  ps.n_plain = n_plain;
  ps.use16 = !(dg & 512u) && TIp >= 18u;                 // (SG_FDIAG 512: no 16-base steps)
  const uint32_t n_p16 = ps.use16 ? n_plain * TI16 : 0u;
  ps.np16steps = (dg & 128u) ? 0u : n_p16 >> 6;
  const uint32_t rem16 = n_p16 - (ps.np16steps << 6);
  ps.cnt8 = ps.use16 ? TIp - 2u * TI16 : TIp;
  ps.c8_base = ps.use16 ? 2u * TI16 : 0u;
  ps.n_pitems = 2u * rem16 + n_plain * ps.cnt8;
  ps.npsteps = (dg & 128u) ? 0u : (ps.n_pitems + 63u) / 64u;   // (ablations: no general / no plain steps)
  return ps;
}

// The lookup row's table addresses of item c of a read of the profile's own length
__device__ __forceinline__ void lut_bins(const uint32_t* lut, uint32_t c, uint32_t (&so)[8], uint32_t& qo0, uint32_t& qo1) {
  const uint4* lrow = (const uint4*)(lut + c * LUT_ROW);
  const uint4 r0 = lrow[0], r1 = lrow[1], r2 = lrow[2];
  so[0] = r0.x; so[1] = r0.y; so[2] = r0.z; so[3] = r0.w; so[4] = r1.x; so[5] = r1.y; so[6] = r1.z; so[7] = r1.w;
  qo0 = r2.x; qo1 = r2.y;
}

// ---- plain16 steps: whole steps of 16-base items ----
struct P16 { uint32_t r, c, src, out; uint2 w; };

template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void plain16_step(const FastBlock<PAIRED, DIAG>& k, FastWave& w, const P16& st, uint32_t qual_at) {
  const uint32_t dg = k.dg;
  const uint32_t c8 = 2u * st.c;   // the lane's two 8-base items: c8, c8 + 1
  // 21 source codes (positions 16c - 5 .. 16c + 15): 42 bits from bit 2 (src mod 4) of the eight bytes on
  const uint64_t w64 = window_codes(st.w, st.src);
  uint32_t cwa = (uint32_t)w64, cwb = (uint32_t)(w64 >> 16);
  const uint32_t slot = w.g * FAST_G + st.r + k.B.slot_offset;
  if (dg & 4u) { cwa = (w.g * FAST_G + st.r) * 2654435761u + c8; cwb = cwa * 40503u + 1u; }  // ablation: no haplotype fetch
  uint32_t sw[4], qw[4], fixv[2];
#pragma unroll
  for (int hf = 0; hf < 2; hf++) {
    uint32_t x[8];
    const uint32_t c = c8 + (uint32_t)hf, cw = hf ? cwb : cwa;
    heads8(k, slot, c, x);
    uint32_t so[8], qo0, qo1;
    lut_bins(k.lut, c, so, qo0, qo1);
    uint32_t s2[2], q2[2], acc;
    sample8(k.code4, k.P.lgW, cw, x, so, qo0, qo1, s2, q2, acc);
    sw[2 * hf] = s2[0]; sw[2 * hf + 1] = s2[1];
    qw[2 * hf] = q2[0]; qw[2 * hf + 1] = q2[1];
    fixv[hf] = (dg & 16u) ? 0u : (acc >> 17) & 0xFFu;
  }
  const uint32_t so_ = (dg & 1u) ? 0xFFFFFFFFu : st.out;
  const uint32_t qo_ = (dg & 1u) ? 0xFFFFFFFFu : st.out + qual_at;
  __builtin_amdgcn_raw_buffer_store_b128(u32x4{sw[0], sw[1], sw[2], sw[3]}, w.out_rsrc, so_, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b128(u32x4{qw[0], qw[1], qw[2], qw[3]}, w.out_rsrc, qo_, 0, 0);
#pragma unroll
  for (int hf = 0; hf < 2; hf++) push_fix(k, w, st.r, c8 + (uint32_t)hf, fixv[hf], hf ? cwb : cwa);
}

template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void plain16_steps(const FastBlock<PAIRED, DIAG>& k, FastWave& w, uint32_t a16, uint32_t b16) {
  uint32_t TI16_v = k.TI16, inv_TI16_v = k.inv_TI16, qual_at = (uint32_t)k.P.L + 3u;
  asm volatile("" : "+v"(TI16_v), "+v"(inv_TI16_v), "+v"(qual_at));   // (as scalars they were spilled, see the 8-base loop)
  auto fetch16 = [&](uint32_t step) -> P16 {
    P16 st;
    const uint32_t i = step * 64u + w.lane;                // < n_p16: whole steps only, every lane has an item
    const uint32_t ri = __umul24(i, inv_TI16_v) >> 20;    // i / TI16
    st.c = i - __umul24(ri, TI16_v);
    st.r = w.permp[ri];
    const uint32_t A = w.rows.src_word(st.r);
    st.src = row::src_m5(A) + 16u * st.c;
    st.out = w.rows.base_off(st.r) + 16u * st.c;
    st.w = k.fetch_window(row::copy_is_rc(A), st.src);
    return st;
  };
  P16 cur = fetch16(a16);
  // (two dropped stores: every iteration then has the same vector-memory operations behind its prefetch, see below)
  __builtin_amdgcn_raw_buffer_store_b128(u32x4{0u, 0u, 0u, 0u}, w.out_rsrc, 0xFFFFFFFFu, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b128(u32x4{0u, 0u, 0u, 0u}, w.out_rsrc, 0xFFFFFFF0u, 0, 0);
  pipelined_steps(cur, a16, b16, fetch16, [&](const P16& st) { plain16_step(k, w, st, qual_at); });
}

// What the plain8 and the clean step share, once each has made its item's table addresses: decode, draws, the 8-base
// block, the two stores, the push.  An item of read r at output offset `out`, its qualities qual_at bytes behind;
// ok: the lane has an item (idle lanes redo their stream's last one, their stores are dropped).  tail_patch (plain
// steps of a tail_whole profile, wave-uniform): the read's last item, whose eighth byte is the line break.
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void sample_store8(const FastBlock<PAIRED, DIAG>& k, FastWave& w, uint32_t r, uint32_t c, bool ok, uint2 win,
                                              uint32_t src, const uint32_t (&so)[8], uint32_t qo0, uint32_t qo1, uint32_t out,
                                              uint32_t qual_at, bool tail_patch) {
  const uint32_t dg = k.dg;
  uint32_t cw;
  if (dg & 4u) cw = (w.g * FAST_G + r) * 2654435761u + c;  // ablation: no haplotype fetch
  else cw = (uint32_t)window_codes(win, src);
  uint32_t x[8];
  heads8(k, w.g * FAST_G + r + k.B.slot_offset, c, x);
  uint32_t sw[2], qw[2], acc;
  sample8(k.code4, k.P.lgW, cw, x, so, qo0, qo1, sw, qw, acc);
  const bool st_ok = ok && !(dg & 1u);
  const uint32_t so_ = st_ok ? out : 0xFFFFFFFFu;
  const uint32_t qo_ = st_ok ? out + qual_at : 0xFFFFFFFFu;
  uint32_t fix_mask = 0xFFu;
  if (tail_patch) {  // (wave-uniform) the read's last item: its eighth byte is the line break, then "+\n"
    const bool last = c + 1u == k.TI;
    const uint32_t sel = last ? 0x04020100u : 0x03020100u;   // v_perm: byte 3 = the first operand's byte 0 / the second's own
    sw[1] = __builtin_amdgcn_perm(0x0Au, sw[1], sel);
    qw[1] = __builtin_amdgcn_perm(0x0Au, qw[1], sel);
    __builtin_amdgcn_raw_buffer_store_b16((unsigned short)0x0A2Bu, w.out_rsrc, st_ok && last ? so_ + 8u : 0xFFFFFFFFu, 0, 0);
    fix_mask = last ? 0x7Fu : 0xFFu;
  }
  __builtin_amdgcn_raw_buffer_store_b64(u32x2{sw[0], sw[1]}, w.out_rsrc, so_, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b64(u32x2{qw[0], qw[1]}, w.out_rsrc, qo_, 0, 0);
  const uint32_t fix = (ok && !(dg & 16u)) ? (acc >> 17) & fix_mask : 0u;
  push_fix(k, w, r, c, fix, cw);
}

// ---- plain steps (8-base items): the reads' own odd last items, then the halves of the 16-base items the whole steps
// above left over ----
struct PStage { uint32_t r, c, src, out; bool ok; uint2 w; };

template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void plain8_steps(const FastBlock<PAIRED, DIAG>& k, FastWave& w, const PlainSteps& ps, uint32_t a8, uint32_t b8) {
  const uint32_t cnt8 = ps.cnt8, c8_base = ps.c8_base, n_pitems = ps.n_pitems, TI16 = k.TI16, inv_TI16 = k.inv_TI16;
  // (wave-uniform values of every step held in vector registers: as scalars they were spilled and came back
  // through a v_readlane_b32 in every step)
  uint32_t qual_at = (uint32_t)k.P.L + 3u, n_single = ps.n_plain * cnt8, i16_base = ps.np16steps << 6;
  asm volatile("" : "+v"(qual_at), "+v"(n_single), "+v"(i16_base));
  const uint32_t inv_cnt8 = cnt8 ? (1u << 20) / cnt8 + 1u : 0u;
  auto fetch_plain = [&](uint32_t step) -> PStage {
    PStage st;
    const uint32_t i_raw = step * 64u + w.lane;
    st.ok = i_raw < n_pitems;
    const uint32_t i = min(i_raw, n_pitems - 1u);     // idle lanes redo the stream's last item, their stores are dropped
    const bool half = i >= n_single;                  // a read's own 8-base item / a half of a left-over 16-base item
    const uint32_t j = i - n_single;
    const uint32_t q = half ? i16_base + (j >> 1) : i;
    const uint32_t d = half ? TI16 : cnt8;
    const uint32_t ri = __umul24(q, half ? inv_TI16 : inv_cnt8) >> 20;  // q / d
    const uint32_t rem = q - __umul24(ri, d);
    st.c = half ? 2u * rem + (j & 1u) : c8_base + rem;
    st.r = w.permp[ri];
    const uint32_t A = w.rows.src_word(st.r);
    st.src = row::src_m5(A) + 8u * st.c;
    st.out = w.rows.base_off(st.r) + 8u * st.c;
    st.w = k.fetch_window(row::copy_is_rc(A), st.src);
    return st;
  };
  auto run_plain = [&](const PStage& st) {
    uint32_t so[8], qo0, qo1;
    lut_bins(k.lut, st.c, so, qo0, qo1);
    sample_store8(k, w, st.r, st.c, st.ok, st.w, st.src, so, qo0, qo1, st.out, qual_at, k.tail_whole);
  };
  PStage cur = fetch_plain(a8);
  // (two dropped stores: every iteration then has the same vector-memory operations behind its prefetch, see below)
  __builtin_amdgcn_raw_buffer_store_b64(u32x2{0u, 0u}, w.out_rsrc, 0xFFFFFFFFu, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b64(u32x2{0u, 0u}, w.out_rsrc, 0xFFFFFFF0u, 0, 0);
  if (k.tail_whole) __builtin_amdgcn_raw_buffer_store_b16((unsigned short)0u, w.out_rsrc, 0xFFFFFFE0u, 0, 0);
  pipelined_steps(cur, a8, b8, fetch_plain, run_plain);
}

// The odd items leave in the MIDDLE of their reads' pairs (round 4): a read's last bytes written nine steps behind its
// pairs met the line gone from L2 (WRITE_SIZE 5.80 -> 6.99 M KiB per launch, profiles/r04_start); with the singles' step
// between the two halves of the 16-base steps no instalment of a read is more than ~four steps from the other.
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void plain_steps(const FastBlock<PAIRED, DIAG>& k, FastWave& w, uint32_t n_plain) {
  const PlainSteps ps = plan_plain_steps(k, n_plain);
  const uint32_t h16 = ps.np16steps >> 1, s8_first = (ps.use16 && ps.cnt8 && ps.npsteps) ? 1u : 0u;   // (8-base steps alone: one loop, phase 1)
#pragma unroll 1
  for (uint32_t ph = 0; ph < 2u; ph++) {
    const uint32_t a16 = ph ? h16 : 0u, b16 = ph ? ps.np16steps : h16;
    const uint32_t a8 = ph ? s8_first : 0u, b8 = ph ? ps.npsteps : s8_first;
    if (a16 < b16) plain16_steps(k, w, a16, b16);
    if (a8 < b8) plain8_steps(k, w, ps, a8, b8);
  }
}

// ---- clean steps: the plain step with the read's own bins, length and (behind the indel) shifted template ----
struct CStage { uint32_t r, c, src, out, np, inv; bool ok; uint2 w; };

template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void clean_steps(const FastBlock<PAIRED, DIAG>& k, FastWave& w, uint32_t n_clean) {
  if (!n_clean) return;
  const uint32_t ncsteps = (k.dg & 128u) ? 0u : (n_clean + 63u) / 64u;
  auto fetch_clean = [&](uint32_t step) -> CStage {
    CStage st;
    const uint32_t i_raw = step * 64u + w.lane;
    st.ok = i_raw < n_clean;
    const uint32_t e = w.clean[min(i_raw, n_clean - 1u)];   // idle lanes redo the list's last item, their stores are dropped
    st.r = e & 63u;
    st.c = e >> 7;
    const FastRow q = w.rows.load(st.r);
    const uint32_t elen = (q.event() >> 16) & 0x7FFFu;
    const uint32_t delta = (e & 64u) ? ((q.event() >> 31) ? elen : 0u - elen) : 0u;
    st.src = q.src_m5() + 8u * st.c + delta;
    st.out = q.base_off() + 8u * st.c;
    st.np = q.np();
    st.inv = q.inv();
    st.w = k.fetch_window(q.copy_is_rc(), st.src);
    return st;
  };
  const uint32_t bins = k.bins, blk_bytes = k.P.fast_stride * 4u;
  auto run_clean = [&](const CStage& st) {
    // bin = i * binCount / n' (Profile.cpp:1672) by the row's reciprocal
    uint32_t so[8];
    const uint32_t ib0 = __umul24(8u * st.c, bins);
#pragma unroll
    for (int h = 0; h < 8; h++) so[h] = __umul24(__umulhi(ib0 + (uint32_t)h * bins, st.inv), blk_bytes) + k.img_at;
    const uint32_t qo0 = so[0], qo1 = so[1];
    if (st.c == 0u) { so[0] += 128u * 4u; so[1] += 64u * 4u; }
    sample_store8(k, w, st.r, st.c, st.ok, st.w, st.src, so, qo0, qo1, st.out, st.np + 3u, false);
  };
  if (ncsteps) {
    CStage cur = fetch_clean(0);
    __builtin_amdgcn_raw_buffer_store_b64(u32x2{0u, 0u}, w.out_rsrc, 0xFFFFFFFFu, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b64(u32x2{0u, 0u}, w.out_rsrc, 0xFFFFFFF0u, 0, 0);
    pipelined_steps(cur, 0u, ncsteps, fetch_clean, run_clean);
  }
}

// ------------------------------------------------------------------------------------------------
// The general step
// ------------------------------------------------------------------------------------------------
// One item per lane, with what the step fetches one step ahead: the read's row and its un-shifted window.
struct Stage { uint32_t r, c; bool active; FastRow row; uint32_t src; uint2 w; };

// Base index of an item's un-shifted template window in the 2-bit copy the read walks forwards -- the forward copy, or
// for a reverse read the reverse-complement copy, where the fragment [A, A + n) starts at total - A - n: output
// position p of the read is base `index + p - 8c + 5` of that copy.  Idle lanes read a harmless in-bounds index.
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ uint32_t fast_src(const FastBlock<PAIRED, DIAG>& k, const FastRow& row, uint32_t c, bool active) {
  const uint32_t a = k.rc(row.rev()) ? (uint32_t)k.B.chains_total - row.frag_lo() - row.flen() : row.frag_lo();  // the straight-line kernel runs on buffers < 2^31 bases
  return active ? a + 8u * c - 5u : 128u;
}

template <bool PAIRED, bool DIAG>
__device__ __forceinline__ Stage fetch_item(const FastBlock<PAIRED, DIAG>& k, const FastWave& w, uint32_t r, uint32_t c, bool ok, uint32_t c_idle) {
  Stage st;
  st.r = r;
  st.row = w.rows.load(r);
  st.active = ok && st.row.active() && c < st.row.items();
  st.c = st.active ? c : c_idle;
  st.src = fast_src(k, st.row, st.c, st.active);
  st.w = k.fetch_window(st.row.rev(), st.src);
  return st;
}

// the item stream, 64 items per step: n_items map items (n_fast reads of TI items), then the single items of ovf
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ Stage fetch_step(const FastBlock<PAIRED, DIAG>& k, const FastWave& w, uint32_t n_items, uint32_t n_stream, uint32_t step) {
  const uint32_t i = step * 64u + w.lane;
  const bool ok = i < n_stream, in_map = i < n_items;
  const uint32_t ri = __umul24(i, k.inv_TI) >> 20;  // i / TI (exact: i * TI < 2^20)
  const uint32_t e = w.ovf[(ok && !in_map) ? i - n_items : 0u];
  const uint32_t r = in_map ? w.perm[ri] : (ok ? (e & 0xFFu) : w.perm[0]);
  const uint32_t c = in_map ? i - __umul24(ri, k.TI) : (ok ? e >> 8 : 1u);
  return fetch_item(k, w, r, c, ok, c);
}

// What the read's sequencing indels mean for one item: d0 = template index minus output index at the item's first
// position (events before it), n_in = events reaching into it (0, 1, or 2 = too many for the two-window code), ew_in =
// that event with its OUTPUT position, tj_in = its template position (the address of its draws).
struct ItemEvents { int d0; uint32_t n_in, ew_in, tj_in; };

template <bool PAIRED, bool DIAG>
__device__ __forceinline__ ItemEvents item_events(const FastBlock<PAIRED, DIAG>& k, const FastWave& w, const Stage& st) {
  const uint32_t nev_r = st.active ? st.row.nev() : 0u;
  const uint32_t c = st.c;
  ItemEvents ie;
  ie.d0 = 0;
  ie.n_in = nev_r == 1u ? 1u : 0u;
  ie.ew_in = st.row.event();
  ie.tj_in = st.row.event() & 0xFFFFu;
  if (__ballot(nev_r >= 2u) != 0ull) {
    if (nev_r >= 2u) {
      // walk the event list like slow_codes does: shift = output index - template index so far
      const uint32_t* ev = k.B.events + ((size_t)k.m * k.B.n_slots + (w.g * FAST_G + st.r)) * SG_MAX_EVENTS;
      const int p_lo = (int)(8u * c) - 2, p_hi = (int)(8u * c) + 7;  // positions whose source bases the item uses
      int shift = 0;
      ie.n_in = 0;
      for (uint32_t q = 0; q < nev_r; q++) {
        const uint32_t e = ev[q];
        const int j = (int)(e & 0xFFFFu), len = (int)((e >> 16) & 0x7FFFu);
        const bool del = (e >> 31) != 0;
        const int pe = j + shift;  // output position of template base j
        if (del ? pe <= p_lo : pe + len < p_lo) { shift += del ? -len : len; continue; }  // wholly before the item
        if (del ? pe > p_hi : pe >= p_hi) break;                                              // this and the rest: after it
        if (ie.n_in == 0u) { ie.d0 = -shift; ie.ew_in = (e & 0xFFFF0000u) | (uint32_t)pe; ie.tj_in = (uint32_t)j; }
        ie.n_in++;
        shift += del ? -len : len;
      }
      if (ie.n_in == 0u) ie.d0 = -shift;
    }
  }
  return ie;
}

// 13 source codes, 2 bits each, for output positions i0-5 .. i0+7: 26 bits of the 2-bit copy starting at base index
// src (st.src = the un-shifted window, fast_src, already loaded into st.w by the caller one step ahead; events before
// the item shift it by d0).  Reads touching a non-ACGT block never get here with valid codes: they are queued whole.
// nev: the events reaching into the item (0 for an idle lane), slot: the read's slot in the batch.
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ uint32_t item_codes(const FastBlock<PAIRED, DIAG>& k, const Stage& st, uint2 wpre, const ItemEvents& ie, uint32_t nev, uint32_t slot) {
  const uint32_t c = st.c, i0 = 8u * c;
  const bool row_rev = st.row.rev();
  const uint32_t src = st.src + (uint32_t)ie.d0;
  if (__ballot(ie.d0 != 0) != 0ull) {
    if (ie.d0 != 0) k.fetch_window(row_rev, src, wpre);
  }
  uint32_t cw;
  if (k.dg & 4u) cw = slot * 2654435761u + c;  // ablation: no haplotype fetch
  else cw = (uint32_t)window_codes(wpre, src);

  // reads with exactly one sequencing indel: past the event the window is shifted by +-len
  if (__ballot(nev == 1u) != 0ull) {
    int q_ins = 1, q_end = 0;  // an insertion's own positions inside the item's window
    if (nev == 1u) {
      const uint32_t ew = ie.ew_in;
      const int ej = (int)(ew & 0xFFFFu), elen = (int)((ew >> 16) & 0x7FFFu);
      const bool del = (ew >> 31) != 0;
      const int delta = del ? elen : -elen;
      const uint32_t src2 = src + (uint32_t)delta;
      const uint32_t cw2 = (uint32_t)window_codes(k.fetch_window(row_rev, src2), src2);
      const int first_shifted = del ? ej : ej + elen + 1;       // first output position reading the shifted window
      const int q0 = first_shifted - ((int)i0 - 5);               // its index in the item window
      const uint32_t keep = q0 <= 0 ? 0u : (q0 >= 13 ? 0xFFFFFFFFu : ((1u << (2 * q0)) - 1u));
      cw = (cw & keep) | (cw2 & ~keep);
      if (!del) {
        // inserted run = output positions ej+1 .. ej+elen: randomInteger(0, N-1), never the last base
        // (Profile.cpp:1564); flat draw f = p - ej of stream (slot, ej); codes are `bases` indexes
        // (window indexes q = p - (i0 - 5) in 3 .. 12 of those positions; the wave loops as often as its longest run needs)
        q_ins = max(3, ej + 1 - ((int)i0 - 5));
        q_end = min(12, ej + elen - ((int)i0 - 5));
      }
    }
#pragma unroll 1
    for (; __ballot(q_ins <= q_end) != 0ull; q_ins++) {
      if (q_ins <= q_end) {
        const int p = (int)i0 - 5 + q_ins, ej = (int)(ie.ew_in & 0xFFFFu);
        const uint32_t prof = __umulhi(aux_draw(k.B, slot, ie.tj_in, (uint32_t)(p - ej), k.m), 3u);
        const uint32_t nat = (k.P.inv_remap_packed >> (2u * prof)) & 3u;
        cw = (cw & ~(3u << (2 * q_ins))) | (nat << (2 * q_ins));
      }
    }
  }
  return cw;
}

// ---- table offsets of the eight positions: bin * block bytes (+ the short-context region of a read's first two
// bases).  Reads of the profile's own length take them from the item's look-up row; reads that a sequencing indel
// changed (their bins are i * binCount / n') and items past the row compute them. ----
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void item_bins(const FastBlock<PAIRED, DIAG>& k, const Stage& st, uint32_t (&so)[8], uint32_t& qo0, uint32_t& qo1) {
  const uint32_t c = st.c, bins = k.bins, blk_bytes = k.P.fast_stride * 4u;
  const bool active = st.active;
  const bool lut_ok = st.row.np() == (uint32_t)k.P.L && c < k.TI;
  if (__ballot(active && !lut_ok) == 0ull) {
    lut_bins(k.lut, lut_ok ? c : 0u, so, qo0, qo1);
  } else {
    const uint32_t ib0 = __umul24(8u * c, bins), inv = st.row.inv();
#pragma unroll
    for (int h = 0; h < 8; h++) {
      // idle lanes may compute a bin past the table: LDS reads beyond the allocation return 0, results unused
      const uint32_t bin = __umulhi(ib0 + (uint32_t)h * bins, inv);
      so[h] = __umul24(active ? bin : 0u, blk_bytes) + k.img_at;
    }
    qo0 = so[0]; qo1 = so[1];
    if (c == 0u) { so[0] += 128u * 4u; so[1] += 64u * 4u; }
  }
}

// A whole item is two 8-byte stores.  They are buffer stores through the read group's descriptor (base = the group's
// first record, offsets 32-bit), issued by EVERY lane on every path: a lane with nothing to store gives an offset past
// the descriptor's range and the hardware drops it.  The step loop so holds a fixed number of vector-memory
// operations, and the wait for the next step's prefetched window is a counted s_waitcnt (vmcnt(3)) instead of one
// that also drains these stores (with the stores under a branch the compiler had to assume the path without them:
// vmcnt(1), a full store round trip exposed in every step).  The read's last, partial item (np % 8 bases) is parked
// in the read's own LDS row: the per-read pass after the step loop merges it with the record separators, so the
// byte-granular stores run once per read group rather than in every step.
// A last item of exactly seven bases (np % 8 == 7: every read without an indel of the 151-base profile) is a whole
// item too -- its eighth byte is the line break that follows the bases / the qualities -- so it leaves with the steps,
// next to its neighbours, instead of coming back to half-written lines from the per-read pass.
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void store_item(const FastBlock<PAIRED, DIAG>& k, const FastWave& w, const Stage& st, bool slow,
                                           const uint32_t (&sw)[2], const uint32_t (&qw)[2]) {
  const uint32_t np = st.row.np(), i0 = 8u * st.c;
  const bool active = st.active, go = active && !slow;
  const bool last7 = i0 + 7u == np;
  const bool whole = i0 + 8u <= np || last7;
  const bool sto = go && whole && !(k.dg & 1u);
  const uint32_t so_ = sto ? st.row.out_off() + st.row.hdr_len() + i0 : 0xFFFFFFFFu;
  const uint32_t qo_ = sto ? so_ + np + 3u : 0xFFFFFFFFu;
  const uint32_t s1 = last7 ? (sw[1] & 0x00FFFFFFu) | 0x0A000000u : sw[1];
  const uint32_t q1 = last7 ? (qw[1] & 0x00FFFFFFu) | 0x0A000000u : qw[1];
  __builtin_amdgcn_raw_buffer_store_b64(u32x2{sw[0], s1}, w.out_rsrc, so_, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b64(u32x2{qw[0], q1}, w.out_rsrc, qo_, 0, 0);
  // ... and the "+\n" between the two line breaks, by the same lane (a third store on every path, dropped elsewhere)
  __builtin_amdgcn_raw_buffer_store_b16((unsigned short)0x0A2Bu, w.out_rsrc, sto && last7 ? so_ + 8u : 0xFFFFFFFFu, 0, 0);
  // parked over the fields no lane needs once the last item has been sampled (fragment offset, 2^32/n',
  // event): base characters are never 0xFF
  if (active && i0 + 8u > np && !(last7 && !slow)) w.rows.park(st.r, slow, sw, qw);
}

// One item of the general stream: codes, draws, table addresses, the 8-base block, the stores.  Returns whether the item
// is left to the generic code (the caller queues it); fix = its flagged bases, cw_out = its codes.
// An idle lane may be looking at a row whose read is finished; its fragment offset, reciprocal and event word then
// hold the parked last item (sg_emit.h), so an idle lane must not follow them -- it reads a harmless in-bounds
// window and has no event.  The caller has reduced the read's sequencing indels to what this item sees (item_events).
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ bool fast_item(const FastBlock<PAIRED, DIAG>& k, const FastWave& w, const Stage& st, const ItemEvents& ie,
                                          uint32_t& fix, uint32_t& cw_out) {
  const bool active = st.active;
  const uint32_t c = st.c, slot = w.g * FAST_G + st.r;
  const uint32_t np = st.row.np(), nev = active ? ie.n_in : 0u;
  const uint32_t bad = st.row.bad_block();
  const uint32_t cw = item_codes(k, st, st.w, ie, nev, slot);
  uint32_t x[8];
  heads8(k, slot + k.B.slot_offset, c, x);
  uint32_t so[8], qo0, qo1;
  item_bins(k, st, so, qo0, qo1);
  uint32_t qw[2], sw[2], acc;
  sample8(k.code4, k.P.lgW, cw, x, so, qo0, qo1, sw, qw, acc);
  const bool slow = active && (bad != 0u || nev >= 2u);  // queued for the generic item code by the caller
  // flagged bases are redone exactly by the group's fix-up pass (the flags of a queued item do not matter)
  fix = (active && !slow && !(k.dg & 16u)) ? (acc >> 17) & 0xFFu & ((1u << min(8u, np - 8u * c)) - 1u) : 0u;
  cw_out = cw;
  store_item(k, w, st, slow, sw, qw);
  return slow;
}

// windows with a non-ACGT base are queued for the generic code
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void general_step(const FastBlock<PAIRED, DIAG>& k, FastWave& w, const Stage& st) {
  const ItemEvents ie = item_events(k, w, st);
  uint32_t fix, cw;
  const bool slow = fast_item(k, w, st, ie, fix, cw);
  const unsigned long long sm = __ballot(slow);
  if (sm) {
    if (slow) w.slow_list[w.nslow + (uint32_t)__popcll(sm & w.lanes_below())] = st.r | (st.c << 8);
    w.nslow += (uint32_t)__popcll(sm);
  }
  push_fix(k, w, st.r, st.c, fix, cw);
}

// ---- general steps ----
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void general_steps(const FastBlock<PAIRED, DIAG>& k, FastWave& w, const GroupPlan& gp) {
  const uint32_t n_items = gp.n_fast * k.TI, n_stream = n_items + gp.n_ovf;
  const uint32_t nmain = (k.dg & 256u) ? 0u : (n_stream + 63u) / 64u;   // (ablations: no general / no plain steps)
  if (!nmain) return;
  Stage cur = fetch_step(k, w, n_items, n_stream, 0u);
  // three (dropped) stores: the loop is then entered with the same vector-memory operations behind the first
  // prefetch as every later iteration has behind its own (three item stores + the next prefetch), and the wait for a
  // prefetched window stays a counted one instead of falling back to the entry path's vmcnt(1)
  __builtin_amdgcn_raw_buffer_store_b64(u32x2{0u, 0u}, w.out_rsrc, 0xFFFFFFFFu, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b64(u32x2{0u, 0u}, w.out_rsrc, 0xFFFFFFF0u, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b16((unsigned short)0u, w.out_rsrc, 0xFFFFFFE0u, 0, 0);
  pipelined_steps(
      cur, 0u, nmain,
      [&](uint32_t step) {   // (every step begins by making room in the slow list, in front of its prefetch)
        if (w.nslow > SLOW_CAP - 64u) flush_slow(k, w);
        return fetch_step(k, w, n_items, n_stream, step);
      },
      [&](const Stage& st) { general_step(k, w, st); });
}

// items past the map (reads grown by insertions, reads of more than 64 items): never a first item
template <bool PAIRED, bool DIAG>
__device__ __forceinline__ void past_map_steps(const FastBlock<PAIRED, DIAG>& k, FastWave& w, unsigned long long more) {
  uint32_t cb = k.TI;
  while (more) {
    if (w.nslow > SLOW_CAP - 64u) flush_slow(k, w);
    const uint32_t r = (uint32_t)__builtin_ctzll(more);
    const uint32_t c = cb + w.lane;
    const uint32_t nitems = (w.rows.np(r) + 7u) / 8u;
    cb += 64u;
    if (cb >= nitems) { more &= more - 1ull; cb = k.TI; }
    const Stage st = fetch_item(k, w, r, c, true, 1u);
    general_step(k, w, st);
  }
}

// ---- per-read pass, lane = read: last partial item, record separators ----
// These byte-granular stores touch lines the steps above have just written from this wave, so
// they merge in L2.  Reads whose last item went to the generic code (0xFFFFFFFF row) get only the
// separators here; emit_slow_kernel writes the same separator bytes again (benign).
__device__ __forceinline__ void tail_pass(const FastWave& w) {
  const FastRow r = w.rows.load(w.lane);
  if (!r.active()) return;
  const uint32_t np = r.np(), hl = r.hdr_len();
  uint8_t* rec = w.gout + r.out_off();
  if ((np & 7u) == 7u && !r.parked_slow()) {
    // the last item went out with the steps, line breaks and the "+" line included
  } else {
    const uint32_t d = !r.parked_slow() ? (np & 7u) : 0u;  // bases (and qualities) of the partial item
    const uint64_t S = r.parked_bases(), Q = r.parked_quals();
    const uint64_t keep = (1ull << (8u * d)) - 1ull;
    uint8_t* so = rec + hl + (np - d);
    // d bases + "\n+\n" (3..10 bytes), d qualities + '\n' (1..8 bytes)
    const uint64_t s_lo = (S & keep) | (0x0A2B0Aull << (8u * d));
    const uint64_t s_hi = d > 5u ? (0x0A2B0Aull >> (8u * (8u - d))) : 0ull;
    store_var(so, s_lo, s_hi, d + 3u);
    store_var(so + np + 3u, (Q & keep) | (0x0Aull << (8u * d)), 0ull, d + 1u);
  }
}

// ------------------------------------------------------------------------------------------------
// The kernel: a wave takes read groups of 63 consecutive reads of one mate (GroupRuns) and takes each through
//   phase 0 (lane = read): row, name, the group's descriptor, the row as the steps want it;
//   the classification of its reads and the lists of its items;
//   the plain, clean and general steps and the steps past the map (lane = item);
//   the two flushes; the per-read tail pass (lane = read).
// ------------------------------------------------------------------------------------------------
template <bool PAIRED, bool DIAG>
__global__ __launch_bounds__(EMIT_THREADS) void emit_fast_kernel(DevProfile P, DevBatch B, uint32_t TI, uint32_t inv_TI, uint32_t clean_cap) {
  extern __shared__ uint4 smem[];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t m = blockIdx.y;
  // launched before the host knew the text size (sg_api.cpp run_pass): a text that does not fit the buffers is left to
  // a second launch into larger ones
  if (B.totals[m] + 64u > B.out_cap[m]) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr((unsigned long long*)&B.totals[3], 4ull);
    return;
  }
  const FastLds lds((uint32_t)P.bins, P.fast_stride, TI, clean_cap);
  uint8_t* const base = (uint8_t*)smem;
  uint32_t* img = (uint32_t*)(base + lds.img);
  const uint32_t img_at = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)img;  // its LDS byte address
  uint32_t* lut = (uint32_t*)(base + lds.lut);
  uint32_t* code4 = (uint32_t*)(base + lds.code4);
  stage_tables(P, PAIRED ? m : 0u, TI, img, img_at, lut, code4);
  __syncthreads();
  const FastBlock<PAIRED, DIAG> k(P, B, m, TI, inv_TI, clean_cap, img_at, lut, code4);
  FastWave w;
  w.lane = lane;
  w.rows.rows = (uint4*)(base + lds.rows) + (size_t)wv * 64 * (META_ROW / 16);
  w.slow_list = (uint32_t*)(base + lds.slow) + wv * SLOW_CAP;
  w.fix_list = (uint2*)(base + lds.fix) + wv * FIX_CAP;
  w.perm = base + lds.perm + wv * 64;
  w.permp = base + lds.permp + wv * 64;
  w.ovf = (uint16_t*)(base + lds.ovf) + wv * OVF_CAP;
  w.clean = (uint16_t*)(base + lds.clean) + wv * clean_cap;

  const uint32_t ngroups = (B.n_slots + FAST_G - 1u) / FAST_G;
  GroupRuns runs(B.totals, 0u, m, ngroups, wv, EMIT_WAVES);
  for (; runs.more(); runs.next(lane)) {
    w.g = runs.g;
    // ---- phase 0, lane = read ----
    const uint32_t t = w.g * FAST_G + lane;
    const bool have = lane < FAST_G && t < B.n_slots;
    uint32_t items = 0;
    ReadRow my = ReadRow::none();
    uint64_t ooff = 0;
    if (have) {
      const size_t idx = (size_t)m * B.n_slots + t;
      my = ReadRow::load(B.meta, idx);
      ooff = rec_offset(B, m, t);
      if (my.active()) {
        items = my.items();  // separators: per-read pass below
        if (B.prefix_len <= 16u && !(k.dg & 2u)) store_name<PAIRED>(B, m, my, idx, B.out[m] + ooff);
      }
    }
    const uint64_t gbase = open_group(w, B.out[m], ooff);
    // what the plain steps need of the read, in the row words nothing else uses (FastRow)
    w.rows.store(lane, FastRow::for_steps(my, k.rc(my.rev()), (uint32_t)B.chains_total, (uint32_t)(ooff - gbase)));
    wave_lds_sync();
    w.nslow = 0;
    w.nfix = 0;
    // ---- the group's reads by class, its items into the lists ----
    GroupPlan gp = classify_group(k, w, my, items);
    compose_lists(k, w, gp);
    // ---- the steps, lane = item ----
    plain_steps(k, w, gp.n_plain);
    clean_steps(k, w, gp.n_clean);
    general_steps(k, w, gp);
    past_map_steps(k, w, gp.more);
    if (w.nslow) flush_slow(k, w);
    if (w.nfix) flush_fix(k, w);
    // ---- per-read pass, lane = read ----
    wave_lds_sync();
    if (have && !(k.dg & 2u)) tail_pass(w);
    wave_lds_sync();
  }
}

// ------------------------------------------------------------------------------------------------
// launch: one 1024-thread workgroup per CU, persistent over read groups; item-stream map, 63 reads per group
// ------------------------------------------------------------------------------------------------
// The runtime puts a file's device code on the device when one of its kernels is first used.  While this kernel shared
// a file with the pass's first kernel that happened at the pass's first launch; in a file of its own it happened inside the first
// emit launch's event pair (measured: 0.45 ms on `emit` of a one-pass run's --stats line, 0.3 ms off `plan`,
// profiles/r14_emit_files/times.txt).  The engine asks for it when a profile that takes this kernel is loaded.
void preload_emit_fast() {
  hipFuncAttributes attr;
  (void)hipFuncGetAttributes(&attr, (const void*)emit_fast_kernel<true, false>);
}

void launch_emit_fast(const DevProfile& P, const DevBatch& B, const EmitPath& path, hipStream_t s) {
  int dev = 0, cus = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const uint32_t nm = B.paired ? 2 : 1;
  const uint32_t TIf = fast_items_per_read(P);
  const uint32_t fneed = ((B.n_slots + FAST_G - 1u) / FAST_G + EMIT_WAVES - 1) / EMIT_WAVES;
  uint32_t fgx = (uint32_t)cus / nm;
  if (fgx < 1) fgx = 1;
  if (fgx > fneed) fgx = fneed;
  const dim3 fgrid(fgx, nm);
  const uint32_t inv_TI = (1u << 20) / TIf + 1u;
  // the list of the one-indel reads' clean items, where the table image leaves room for it (else those reads stay whole
  // in the general steps: same output)
  const uint32_t clean_cap = path.clean_cap;
  const size_t lds_fast = path.lds_bytes;
  auto launch_fast = [&](auto kern) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_fast);
    hipLaunchKernelGGL(kern, fgrid, dim3(EMIT_THREADS), lds_fast, s, P, B, TIf, inv_TI, clean_cap);
  };
  if (B.diag) {  // timing ablations (SG_FDIAG)
    if (B.paired) launch_fast(emit_fast_kernel<true, true>);
    else launch_fast(emit_fast_kernel<false, true>);
  } else {
    if (B.paired) launch_fast(emit_fast_kernel<true, false>);
    else launch_fast(emit_fast_kernel<false, false>);
  }
}

}  // namespace sg
