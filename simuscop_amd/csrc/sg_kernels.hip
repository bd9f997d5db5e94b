// sg_kernels.hip -- the generic emit side of the read-sampling pass, hand-written for gfx950 (CDNA4): header_kernel (the
// reads' names), emit_kernel and emit_slow_kernel over emit_item (Profile::predict sampling loop, Profile.cpp:1636-1700,
// + FASTQ formatting, Segment.cpp:803-832), encode_kernel, mail_kernel, the choice of the emit path and the launchers.
// One lane = one read, then 8 bases of one: a wave's reads are consecutive fragment slots of the same 1 kbp window(s), so
// their haplotype bytes share a few cache lines and their FASTQ records form one contiguous ~21 KB output range.
// The kernels in front of these (they write the reads' rows and the record offsets) are in sg_pass_front.hip, the
// straight-line emit kernel (emit_fast_kernel) in sg_emit_fast.hip; what they share -- the read row, the read-group runs,
// write_name -- in sg_emit.h.  The window planner's kernels are in sg_windows.hip, the general u32 scan in sg_scan.hip.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "sg_emit.h"

namespace sg {

__global__ __launch_bounds__(256) void header_kernel(DevBatch B) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t m = blockIdx.y;
  if (t >= B.n_slots) return;
  const size_t idx = (size_t)m * B.n_slots + t;
  ReadRow row;
  row.m1 = B.meta[idx * 3 + 1];
  if (!row.active()) return;
  row.m0 = B.meta[idx * 3];
  const uint64_t ooff = rec_offset(B, m, t);
  if (ooff + row.rec_len() > B.out_cap[m]) return;  // (the record's length: header + 2 lines + 4 line breaks and '+')
  if (!(B.diag & 4u)) write_name(B.out[m] + ooff, B.prefix, B.prefix_len, row.namepos(), row.fragcount(), B.paired, m);
}

// ------------------------------------------------------------------------------------------------
// emit: Profile::predict's sampling loop (Profile.cpp:1636-1700) + FASTQ formatting
// (Segment.cpp:803-832).
//
// Mapping (v3).  A wave owns G consecutive reads of one mate (one contiguous ~21 KB output range).
//   phase 0  lane = read: words m0, m1 of its 48-byte row (ReadRow, sg_emit.h; written by fragment_kernel) with the
//            record's offset, 32 bytes, into LDS.
//   phase 1  lane = 8 consecutive bases.  The lane -> (read-in-iteration, item) map is FIXED:
//            TI = ceil((L+3)/8) items per read, RPI = 64/TI reads per wave iteration, so there is no
//            search, no division and no shuffle in the loop; read metadata comes from two LDS b128
//            reads.  Consecutive lanes write consecutive 8-byte runs: whole cache lines per store.
//            Reads grown by insertions beyond 8*TI-3 bases finish in a short clean-up loop.
// Haplotypes arrive pre-encoded (encode_kernel: A0 C1 T2 G3, N=4, other=5), thresholds live in LDS,
// sampling is branch-free integer compares.  v1 (lane per read) wrote each line in 32 partial
// stores (35.8 GB fabric writes for 4.2 GB of FASTQ); v2 fixed the traffic but spent ~1100
// instructions per 4 bases on bookkeeping (profiles/README.md).
// ------------------------------------------------------------------------------------------------

// A template byte of the chains (A0 C1 T2 G3, N = 4, X = 6, anything else = 5) as the sampling loop sees it: a base code in
// read orientation (reverse reads: complemented, A0 <-> T2, C1 <-> G3, Segment.cpp:81-103), 4 = unknown, 6 = a literal 'X'.
// The reference's k-mer trie holds the place-holder contexts "XXb" and "Xbb" of a read's first bases under the character
// 'X' (Profile.cpp:94-101), so a literal X in the genome -- on a forward read: the complement of anything but A/C/G/T is
// 'N' (Segment.cpp:99) -- is the same place holder in the middle of a read.  `x_known` false (--strict-bases): an X is an
// unknown base like any other.
__device__ __forceinline__ uint32_t template_code(uint32_t raw, bool rev, bool x_known) {
  return raw < 4u ? (rev ? raw ^ 2u : raw) : ((raw == 6u && !rev && x_known) ? 6u : 4u);
}

// Source codes of a read that carries sequencing-indel events (rare path, kept OUT OF LINE and
// un-unrolled: inlined it pushed the kernel past the 64 KB instruction cache and cost 2x).
// Walks the events of Profile::predict's first loop (Profile.cpp:1607-1658) with a forward cursor and
// returns 13 nibbles, one per output position p = i0-5+q: base code 0..3 (template bases complemented
// for reverse reads), 4/5 = not in `bases`, bit 3 set = inserted base (already a profile code).
__device__ __noinline__ uint64_t slow_codes(const uint8_t* frag, uint32_t flen, uint32_t rev, const uint32_t* ev,
                                            uint32_t nev, uint32_t np, uint32_t i0, uint32_t K, uint32_t slot,
                                            uint32_t ctx_aux, uint32_t k0, uint32_t k1, bool x_known) {
  uint64_t out = 0;
  uint32_t e = 0;
  int shift = 0;  // output index - template index of the template bases after the consumed events
  uint32_t nextw = nev ? ev[0] : 0xFFFFFFFFu;
#pragma unroll 1
  for (int q = 0; q < 13; q++) {
    const int p = (int)i0 - 5 + q;
    uint32_t v = 4u;
    if (p >= 0 && (uint32_t)p < np && q >= 6 - (int)K) {
      // consume the events that end before p
#pragma unroll 1
      while (nextw != 0xFFFFFFFFu) {
        const int j = (int)(nextw & 0xFFFFu), len = (int)((nextw >> 16) & 0x7FFFu);
        const int pe = j + shift;  // output position of template base j / where it would have been
        if (nextw >> 31) { if (p < pe) break; shift -= len; }
        else { if (p <= pe + len) break; shift += len; }
        e++;
        nextw = e < nev ? ev[e] : 0xFFFFFFFFu;
      }
      bool inserted = false;
      if (nextw != 0xFFFFFFFFu && !(nextw >> 31)) {
        const int j = (int)(nextw & 0xFFFFu);
        const int pe = j + shift;
        if (p > pe) {  // inserted base number p-pe: randomInteger(0, N-1), never the last base (Profile.cpp:1564)
          const uint32_t f = (uint32_t)(p - pe);
          uint32_t x[4];
          philox4x32_10(slot, (uint32_t)j, f >> 2, ctx_aux, k0, k1, x);
          const uint32_t l = f & 3u;
          const uint32_t xv = l == 0 ? x[0] : l == 1 ? x[1] : l == 2 ? x[2] : x[3];
          v = 8u | __umulhi(xv, 3u);
          inserted = true;
        }
      }
      if (!inserted) {
        const uint32_t jt = (uint32_t)(p - shift);
        v = template_code(frag[rev ? flen - 1u - jt : jt], rev != 0u, x_known);
      }
    }
    out |= (uint64_t)v << (4 * q);
  }
  return out;
}

// One item = output positions [8c, 8c+8) of one read: sample and store bases + qualities.
//   rd: the read's row (sg_emit.h) with the record's offset in the text in place of the name's numbers (set_out64)
template <int KT, bool SUB_LDS>
__device__ __forceinline__ void emit_item(const DevProfile& P, const DevBatch& B, const uint4* lds_sub, const uint4* gsub,
                                          uint32_t m, const ReadRow rd, uint32_t slot, uint32_t c, bool active) {
  const uint32_t K = KT ? (uint32_t)KT : (uint32_t)P.kmer;
  const uint32_t bins = (uint32_t)P.bins;
  const uint32_t ctxmask = (1u << (2 * K)) - 1u;
  const uint32_t flen = rd.flen();
  const bool rev = rd.rev();
  const uint32_t np = rd.np(), nev = (B.diag & 32u) ? 0u : rd.nev(), hdr = rd.hdr_len();
  const uint32_t inv = rd.inv();
  const uint8_t* frag = B.chains + rd.frag_off();
  const uint32_t i0 = 8u * c;
  const bool x_known = B.strict_bases == 0u;  // a literal X of the genome is the trie's place holder (template_code)

  // ---- source codes for positions i0-5 .. i0+7 (index q = p - i0 + 5); >= 4 means "not in bases" ----
  // Every lane loads the un-shifted template window: 16 encoded haplotype bytes; after the conditional
  // byte reversal position p sits at byte p-i0+5.  Unused slots (flen == 0: last partial group,
  // abandoned windows) read a harmless in-bounds address.
  uint32_t code[13];
  const uint8_t* src = flen == 0u ? B.chains + 128 : (rev ? frag + (int)flen - (int)i0 - 11 : frag + (int)i0 - 5);
  auto load_window = [&](const uint8_t* p16, uint32_t (&w)[4]) {
    __builtin_memcpy(w, p16, 16);
    if (rev) {
      const uint32_t t0 = __builtin_bswap32(w[3]), t1 = __builtin_bswap32(w[2]);
      const uint32_t t2 = __builtin_bswap32(w[1]), t3 = __builtin_bswap32(w[0]);
      w[0] = t0; w[1] = t1; w[2] = t2; w[3] = t3;
    }
  };
  {
    uint32_t w[4] = {0x00010203u + i0, 0x03020100u, 0x01000302u, 0x02030001u};
    if (!(B.diag & 2u)) load_window(src, w);
#pragma unroll
    for (int q = 0; q < 13; q++) code[q] = template_code((w[q >> 2] >> ((q & 3) * 8)) & 0xFFu, rev, x_known);
  }
  // Reads with exactly one sequencing indel (most event reads): past the event the template window is
  // the same window shifted by +-len; inserted bases are redrawn from their addressed Philox stream.
  if (__ballot(nev == 1u) != 0ull) {
    if (nev == 1u) {
      const uint32_t ew = rd.event();
      const int ej = (int)(ew & 0xFFFFu), elen = (int)((ew >> 16) & 0x7FFFu);
      const bool del = (ew >> 31) != 0;
      const int delta = del ? elen : -elen;  // template index shift past the event
      uint32_t w2[4];
      load_window(rev ? src - delta : src + delta, w2);
      const int first_shifted = del ? ej : ej + elen + 1;  // first output position that reads the shifted window
#pragma unroll
      for (int q = 0; q < 13; q++) {
        const int p = (int)i0 - 5 + q;
        const uint32_t c2 = template_code((w2[q >> 2] >> ((q & 3) * 8)) & 0xFFu, rev, x_known);
        if (p >= first_shifted) code[q] = c2;
      }
      if (!del) {
        // inserted run occupies output positions ej+1 .. ej+elen: randomInteger(0, N-1), never the last
        // base (Profile.cpp:1564); flat draw f = p - ej of stream (slot, ej)
#pragma unroll 1
        for (int q = 0; q < 13; q++) {
          const int p = (int)i0 - 5 + q;
          const bool ins = p > ej && p <= ej + elen && p >= 0;
          if (__ballot(ins) == 0ull) continue;
          if (ins) {
            const uint32_t v = 0x100u | __umulhi(aux_draw(B, slot, (uint32_t)ej, (uint32_t)(p - ej), m), 3u);
            // q is a loop variable: select through a mask instead of indexing registers dynamically
#pragma unroll
            for (int z = 0; z < 13; z++) if (z == q) code[z] = v;
          }
        }
      }
    }
  }
  if (__ballot(nev >= 2u) != 0ull) {
    if (nev >= 2u) {
      const uint32_t* ev = B.events + ((size_t)m * B.n_slots + slot) * SG_MAX_EVENTS;
      const uint64_t packed = slow_codes(frag, flen, rev ? 1u : 0u, ev, nev, np, i0, K, slot + B.slot_offset,
                                         dev_ctx(KIND_AUX, m, B.batch_id), B.k0, B.k1, x_known);
#pragma unroll
      for (int q = 0; q < 13; q++) {
        const uint32_t v = (uint32_t)(packed >> (4 * q)) & 0xFu;
        code[q] = (v & 8u) ? (0x100u | (v & 3u)) : v;
      }
    }
  }
  // natural index (A0 C1 T2 G3) -> profile base code; inserted bases (0x100 flag) already are profile codes
  const bool identity = P.remap_packed == 0xE4u;
#pragma unroll
  for (int q = 0; q < 13; q++) {
    uint32_t v = code[q];
    if (v & 0x100u) v &= 3u;
    else if (!identity && v < 4u) v = (P.remap_packed >> (2u * v)) & 3u;
    code[q] = v;
  }
  // ---- k-mer context (Profile::initKmers order, Profile.cpp:70-124).  The reference looks the K characters ending at a
  // position up in a trie that holds b^K and the place-holder forms X^a b^(K-a) (Profile.cpp:94-101, 220-226); the
  // characters before a read's first base are 'X' (Profile.cpp:1660-1663), and so is a literal X of the genome.  A position
  // has a context iff its window is a run of X (xr of them) followed by vc >= 1 bases; the context then has min(vc, K)
  // bases.  State: vc = bases at the end of what was seen, xr = the X run right before them, xc = the X run at the end.
  uint32_t ctxv = 0, vc = 0, xr = 0, xc = 0;
  auto ctx_step = [&](uint32_t c) {
    const bool valid = c < 4u;
    ctxv = ((ctxv << 2) | (c & 3u)) & ctxmask;
    if (valid) { if (vc == 0u) xr = xc; vc = min(vc + 1u, K); xc = 0u; }
    else { vc = 0u; xr = 0u; xc = c == 6u ? min(xc + 1u, K) : 0u; }
  };
#pragma unroll
  for (int q = 0; q < 5; q++)
    if (q >= 6 - (int)K) ctx_step((int)i0 - 5 + q >= 0 ? code[q] : 6u);   // the K-1 positions before i0
  // ---- four Philox calls: heads and tails of output positions i0 .. i0+7 (call = i/4, c2 = 0 heads / 1 tails, word = i%4):
  //   substitution draw = heads[31:16] << 16 | tails[31:16],  quality draw = heads[15:0] << 16 | tails[15:0]
  uint32_t xh[8], xt[8];
  const uint32_t c3b = dev_ctx(KIND_BASE, m, B.batch_id);
#pragma unroll
  for (int g = 0; g < 2; g++) {
    if (B.diag & 8u) {
      for (int z = 0; z < 4; z++) { xh[4 * g + z] = (slot * 2654435761u) ^ (c * 40503u + (4 * g + z) * 0x9E3779B9u); xt[4 * g + z] = ~xh[4 * g + z]; }
    } else {
      philox_base(slot + B.slot_offset, 2u * c + (uint32_t)g, 0, c3b, B.k0, B.k1, xh + 4 * g);
      philox_base(slot + B.slot_offset, 2u * c + (uint32_t)g, 1, c3b, B.k0, B.k1, xt + 4 * g);
    }
  }
  const uint32_t lgW = P.lgW;
  uint32_t sw[2] = {0, 0}, qw[2] = {0, 0};
#pragma unroll
  for (int h = 0; h < 8; h++) {
    const uint32_t i = i0 + (uint32_t)h;
    const uint32_t cd = code[5 + h];
    const bool valid = cd < 4u;
    ctx_step(cd);
    const uint32_t xs = (xh[h] & 0xFFFF0000u) | (xt[h] >> 16), xq = (xh[h] << 16) | (xt[h] & 0xFFFFu);
    const uint32_t bin = min(__umulhi(i * bins, inv), bins - 1u);  // i*binCount/n' (clamp only guards idle lanes)
    const uint32_t mlen = max(vc, 1u);
    const uint32_t mmask = (1u << (2u * mlen)) - 1u;
    const bool ctx_ok = vc >= 1u && vc + xr >= K && !(B.diag & 16u);
    // contexts with m real bases start at (4^m-4)/3 = (0x55555555 & (4^m-1)) - 1
    const uint32_t kidx = ctx_ok ? ((0x55555555u & mmask) - 1u) + (ctxv & mmask) : 0u;
    const uint4 row = SUB_LDS ? lds_sub[kidx * bins + bin] : gsub[(size_t)kidx * bins + bin];
    // identity-first row: j = max(j0, #{xs > D_i}), called base = o_j (o_0 = the reference base)
    const uint32_t j = max((uint32_t)(xs > row.x) + (uint32_t)(xs > row.y) + (uint32_t)(xs > row.z), row.w & 3u);
    const uint32_t k = ctx_ok ? ((row.w >> (2u * j + 2u)) & 3u) : cd;  // unknown context: the base is copied (Profile.cpp:1531-1533)
    const bool kvalid = k < 4u;
    const uint32_t kk = kvalid ? k : 0u;
    // alias column of row (reference base, called base, bin)
    const uint2 e = P.alias[(((size_t)((valid ? cd : 0u) * 4u + kk) * bins + bin) << lgW) + (xq >> (32u - lgW))];
    const uint32_t u = xq & ((1u << (32u - lgW)) - 1u);
    const uint32_t qi = (B.diag & 16u) ? 7u + (xq >> 29) : (u < e.x ? (e.y & 0xFFu) : ((e.y >> 8) & 0xFFu));
    uint32_t ch = kvalid ? ((P.bases_packed >> (8u * kk)) & 0xFFu) : (uint32_t)'N';
    uint32_t q = (uint32_t)P.min_qual + (kvalid ? qi : __umulhi(xq, 20u));  // getRandBaseQuality, Profile.cpp:1582-1584
    if (i >= np) {  // "\n+\n" after the bases, '\n' after the qualities
      ch = (i - np == 1u) ? '+' : '\n';
      q = '\n';
    }
    sw[h >> 2] |= ch << (8 * (h & 3));
    qw[h >> 2] |= q << (8 * (h & 3));
  }
  if (active && !(B.diag & 1u)) {
    uint8_t* so = B.out[m] + rd.out64() + hdr + i0;
    uint8_t* qo = so + np + 3u;
    const uint32_t ns = min(8u, np + 3u - i0);                  // bases + "\n+\n"
    const uint32_t nq = i0 <= np ? min(8u, np + 1u - i0) : 0u;  // qualities + '\n'
    if (ns == 8) __builtin_memcpy(so, sw, 8);
    else for (uint32_t b2 = 0; b2 < ns; b2++) so[b2] = (uint8_t)(sw[b2 >> 2] >> (8 * (b2 & 3)));
    if (nq == 8) __builtin_memcpy(qo, qw, 8);
    else for (uint32_t b2 = 0; b2 < nq; b2++) qo[b2] = (uint8_t)(qw[b2 >> 2] >> (8 * (b2 & 3)));
  }
}

template <int KT, bool SUB_LDS>
__global__ __launch_bounds__(EMIT_THREADS) void emit_kernel(DevProfile P, DevBatch B, uint32_t sub_rows, uint32_t TI, uint32_t RPI) {
  extern __shared__ uint4 smem[];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t m = blockIdx.y;
  // launched before the host knew the text size (sg_api.cpp run_pass): a text that does not fit the buffers is left to
  // a second launch into larger ones
  if (B.totals[m] + 64u > B.out_cap[m]) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr((unsigned long long*)&B.totals[3], 4ull);
    return;
  }
  const uint32_t tm = B.paired ? m : 0u;  // SE always samples from the mate-1 tables (Segment.cpp:770,777)
  // ---- LDS carve-up: [sub rows][per-wave metadata rows]; the alias columns are read through L2 ----
  uint4* lds_sub = smem;
  uint4* lds_meta_all = smem + (SUB_LDS ? sub_rows : 0u);
  const uint4* gsub = P.sub + (size_t)tm * P.sub_mate_rows;
  if (SUB_LDS)
    for (uint32_t i = tid; i < sub_rows; i += EMIT_THREADS) lds_sub[i] = gsub[i];
  __syncthreads();
  uint4* meta_rows = lds_meta_all + (size_t)wv * 64 * (META_ROW / 16);

  const uint32_t G = RPI * (64u / RPI);             // reads per wave group
  const uint32_t ngroups = (B.n_slots + G - 1u) / G;
  const uint32_t sub = lane / TI, c_lane = lane - sub * TI;  // fixed lane -> (read in iteration, item)
  const bool lane_ok = sub < RPI;

  // groups from a counter of its own: this kernel also re-emits a batch after emit_fast_kernel has run (sg_result)
  GroupRuns runs(B.totals, 1u, m, ngroups, wv, EMIT_WAVES);
  for (; runs.more(); runs.next(lane)) {
    const uint32_t g = runs.g;
    // ================= phase 0: lane = read: its 32-byte row (coalesced) into LDS =================
    const uint32_t t = g * G + lane;
    uint32_t items = 0;
    ReadRow my = ReadRow::none();
    if (lane < G && t < B.n_slots) {
      my = ReadRow::load(B.meta, (size_t)m * B.n_slots + t);
      my.set_out64(rec_offset(B, m, t));
      if (my.active()) items = (my.np() + 10u) / 8u;  // ceil((np + 3) / 8): bases + "\n+\n"
    }
    meta_rows[lane * 2] = my.m0;
    meta_rows[lane * 2 + 1] = my.m1;
    wave_lds_sync();

    // ================= phase 1: lane = 8 consecutive bases, fixed lane -> (read, item) map =================
    if (!(B.diag & 64u)) {
      // main steps: RPI reads per step through the fixed map; then the reads grown by insertions past
      // the TI items of the map (rare) finish one read at a time.  One call site keeps the loop small.
      const uint32_t nmain = (G + RPI - 1u) / RPI;
      unsigned long long more = __ballot(items > TI);
      uint32_t cb = TI;
      for (uint32_t step = 0;; step++) {
        uint32_t r, c;
        bool ok;
        if (step < nmain) {
          r = step * RPI + sub;
          c = c_lane;
          ok = lane_ok && r < G;
          if (!ok) r = step * RPI;
        } else {
          if (!more) break;
          r = (uint32_t)__builtin_ctzll(more);
          c = cb + lane;
          ok = true;
        }
        const ReadRow rd{meta_rows[r * 2], meta_rows[r * 2 + 1]};
        const uint32_t np = rd.np();
        const uint32_t nitems = (np + 10u) / 8u;
        if (step >= nmain) {
          cb += 64u;
          if (cb >= nitems) { more &= more - 1ull; cb = TI; }
        }
        const bool active = ok && rd.active() && c < nitems;
        emit_item<KT, SUB_LDS>(P, B, lds_sub, gsub, m, rd, g * G + r, active ? c : 0u, active);
      }
    }

    wave_lds_sync();  // the next group's phase 0 rewrites the metadata rows
  }
}

// The queued items of emit_fast_kernel, one lane each, through the generic item code; the tables are
// staged in LDS like in emit_kernel when they fit (persistent workgroup per CU, grid-stride over the queue).
template <int KT, bool SUB_LDS>
__global__ __launch_bounds__(EMIT_THREADS) void emit_slow_kernel(DevProfile P, DevBatch B, uint32_t sub_rows) {
  extern __shared__ uint4 smem[];
  const uint32_t m = blockIdx.y, tid = threadIdx.x, lane = tid & 63u;
  const uint32_t tm = B.paired ? m : 0u;
  uint32_t n = B.slowq_count[m];
  if (n > B.slowq_cap) n = B.slowq_cap;  // overflow: the host reruns the batch through emit_kernel
  if ((blockIdx.x * EMIT_THREADS) >= n) return;  // nothing for this workgroup: skip the staging too
  uint4* lds_sub = smem;
  const uint4* gsub = P.sub + (size_t)tm * P.sub_mate_rows;
  if (SUB_LDS)
    for (uint32_t i = tid; i < sub_rows; i += EMIT_THREADS) lds_sub[i] = gsub[i];
  __syncthreads();
  const uint2* q = B.slowq + (size_t)m * B.slowq_cap;
  for (uint32_t b0 = (blockIdx.x * EMIT_THREADS + tid) & ~63u; b0 < n; b0 += gridDim.x * EMIT_THREADS) {
    const uint32_t i = b0 + lane;
    const bool act = i < n;
    const uint2 e = q[act ? i : b0];
    ReadRow rd = ReadRow::load(B.meta, (size_t)m * B.n_slots + e.x);
    rd.set_out64(rec_offset(B, m, e.x));
    emit_item<KT, SUB_LDS>(P, B, lds_sub, gsub, m, rd, e.x, e.y, act);
  }
}

// ------------------------------------------------------------------------------------------------
// haplotype encoding: ASCII -> base code, in place (A0 C1 T2 G3, 'N' = 4, 'X' = 6, anything else = 5)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t encode4(uint32_t w) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t b = (w >> (8 * i)) & 0xDFu;   // letters in either case, as encode_base of sg_haplotypes.hip has them
    const bool acgt = (b == 'A') | (b == 'C') | (b == 'G') | (b == 'T');
    const uint32_t v = acgt ? ((b >> 1) & 3u) : (b == 'N' ? 4u : (b == 'X' ? 6u : 5u));
    o |= v << (8 * i);
  }
  return o;
}
__global__ __launch_bounds__(256) void encode_kernel(uint4* __restrict__ buf, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) {
    uint4 v = buf[i];
    v.x = encode4(v.x); v.y = encode4(v.y); v.z = encode4(v.z); v.w = encode4(v.w);
    buf[i] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// launchers (declared in sg_device.h)
// ------------------------------------------------------------------------------------------------
// a pass's sizes and flags (totals[0..4]) to the context's pinned mailbox: a kernel of five lanes writing host memory
// reaches the host sooner than a copy command of 40 bytes through the DMA engine
__global__ void mail_kernel(const uint64_t* __restrict__ totals, uint64_t* __restrict__ mail) {
  if (threadIdx.x < 5u) mail[threadIdx.x] = totals[threadIdx.x];
}
void launch_mail(const uint64_t* totals, uint64_t* mail, hipStream_t s) {
  hipLaunchKernelGGL(mail_kernel, dim3(1), dim3(64), 0, s, totals, mail);
}
void launch_header(const DevProfile& P, const DevBatch& B, hipStream_t s) {
  if (!B.n_slots) return;
  const bool fast = emit_uses_fast_kernel(P, B);
  if (fast && B.prefix_len <= 16u) return;  // the straight-line kernel writes the names of its reads itself
  dim3 grid((B.n_slots + 255) / 256, B.paired ? 2 : 1);
  hipLaunchKernelGGL(header_kernel, grid, dim3(256), 0, s, B);
}
// LDS budget: the generic kernels stage the substitution rows when they fit (the alias columns are read through L2);
// the straight-line kernel needs its whole table image.
static const size_t kLdsBytes = 160 * 1024;
template <int KT, bool SL>
static void launch_emit_variant(const DevProfile& P, const DevBatch& B, dim3 grid, size_t lds, uint32_t sub_rows, uint32_t TI,
                                uint32_t RPI, hipStream_t s) {
  (void)hipFuncSetAttribute((const void*)emit_kernel<KT, SL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((emit_kernel<KT, SL>), grid, dim3(EMIT_THREADS), lds, s, P, B, sub_rows, TI, RPI);
}
struct EmitLds { uint32_t sub_rows, fast_TI; size_t lds, lds_fast; bool sub_lds, fast_fits; };
static EmitLds emit_lds(const DevProfile& P) {
  EmitLds e;
  uint32_t kmer_count = 0;
  for (int m = 1, p = 1; m <= P.kmer; m++) { p *= 4; kmer_count += p; }
  e.sub_rows = kmer_count * (uint32_t)P.bins;
  const size_t meta_b = (size_t)EMIT_WAVES * 64 * META_ROW;
  const size_t sub_b = (size_t)e.sub_rows * 16;
  e.sub_lds = meta_b + sub_b <= kLdsBytes;
  e.lds = meta_b + (e.sub_lds ? sub_b : 0);
  // straight-line kernel: everything of its layout (FastLds, sg_emit.h) but the clean list
  e.fast_TI = fast_items_per_read(P);
  e.lds_fast = FastLds((uint32_t)P.bins, P.fast_stride, e.fast_TI, 0u).total;
  e.fast_fits = P.kmer == 3 && P.fast_lds != nullptr && e.lds_fast <= kLdsBytes && P.bins < 256;
  return e;
}
// 0: generic kernel, 1: straight-line kernel
static int emit_fast_mode(const DevProfile& P) {
  if (getenv("SG_DIAG") != nullptr) return 0;
  return emit_lds(P).fast_fits ? 1 : 0;
}
int emit_variant(const DevProfile& P) { return emit_fast_mode(P); }
bool emit_uses_fast_kernel(const DevProfile& P, const DevBatch& B) {
  // the straight-line kernel addresses the 2-bit haplotype copies with 32-bit base indexes
  return emit_fast_mode(P) != 0 && B.chains_total < (1ull << 31);
}
// (clean_cap: CLEAN_CAP entries per wave, or as many 64s as fit beside a large image: the 41-symbol profiles leave 6.9 KB)
EmitPath emit_path(const DevProfile& P, const DevBatch& B, bool force_generic) {
  const EmitLds e = emit_lds(P);
  EmitPath r;
  if (!force_generic && emit_uses_fast_kernel(P, B)) {
    uint32_t clean_cap = FastLds::clean_cap_in(kLdsBytes - e.lds_fast);
    if (getenv("SG_NO_CLEAN_STEPS") != nullptr) clean_cap = 0;
    if (const char* c = getenv("SG_CLEAN_CAP")) clean_cap = std::min(clean_cap, (uint32_t)strtoul(c, nullptr, 10) & ~63u);  // (tests: a list that overflows)
    r.main_kernel = SG_EMIT_STRAIGHT_LINE;
    r.slow_rows_lds = e.sub_lds ? 1 : 0;
    r.lds_bytes = FastLds((uint32_t)P.bins, P.fast_stride, e.fast_TI, clean_cap).total;
    r.clean_cap = clean_cap;
  } else {
    r.main_kernel = !e.sub_lds ? SG_EMIT_GENERIC_GLOBAL : P.kmer == 3 ? SG_EMIT_GENERIC_K3_LDS : SG_EMIT_GENERIC_LDS;
    r.slow_rows_lds = -1;
    r.lds_bytes = (uint32_t)e.lds;
    r.clean_cap = 0;
  }
  return r;
}
void launch_emit(const DevProfile& P, const DevBatch& B, hipStream_t s, bool force_generic, hipEvent_t after_main) {
  if (!B.n_slots) {
    if (after_main) (void)hipEventRecord(after_main, s);
    return;
  }
  const EmitLds e = emit_lds(P);
  const EmitPath path = emit_path(P, B, force_generic);
  int dev = 0, cus = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const uint32_t nm = B.paired ? 2 : 1;
  // generic kernel, fixed lane map: TI items of 8 bases per read, RPI reads per wave iteration
  uint32_t TI = ((uint32_t)P.L + 3u + 7u) / 8u;
  if (TI > 64u) TI = 64u;  // longer reads finish in the clean-up loop
  const uint32_t RPI = 64u / TI;
  const uint32_t G = RPI * (64u / RPI);
  uint32_t gx = (uint32_t)cus / nm;  // one 1024-thread workgroup per CU, persistent over read groups
  if (gx < 1) gx = 1;
  const uint32_t need = ((B.n_slots + G - 1u) / G + EMIT_WAVES - 1) / EMIT_WAVES;
  if (gx > need) gx = need;
  const dim3 grid(gx, nm);
  if (path.main_kernel == SG_EMIT_STRAIGHT_LINE) {
    launch_emit_fast(P, B, path, s);  // the straight-line kernel (sg_emit_fast.hip)
    if (after_main) (void)hipEventRecord(after_main, s);
    // the queued items through the generic code (reference-order tables)
    const size_t slow_sub = path.slow_rows_lds ? (size_t)e.sub_rows * 16 : 0;
    auto launch_slow = [&](auto kern) {
      (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)slow_sub);
      hipLaunchKernelGGL(kern, grid, dim3(EMIT_THREADS), slow_sub, s, P, B, e.sub_rows);
    };
    if (slow_sub) launch_slow(emit_slow_kernel<3, true>);
    else launch_slow(emit_slow_kernel<3, false>);
  } else {
    if (path.main_kernel == SG_EMIT_GENERIC_K3_LDS) launch_emit_variant<3, true>(P, B, grid, e.lds, e.sub_rows, TI, RPI, s);
    else if (path.main_kernel == SG_EMIT_GENERIC_LDS) launch_emit_variant<0, true>(P, B, grid, e.lds, e.sub_rows, TI, RPI, s);
    else launch_emit_variant<0, false>(P, B, grid, e.lds, e.sub_rows, TI, RPI, s);
    if (after_main) (void)hipEventRecord(after_main, s);
  }
}
void launch_encode(uint8_t* buf, size_t bytes, hipStream_t s) {  // bytes is a multiple of 16
  if (!bytes) return;
  const size_t n16 = bytes / 16;
  uint32_t grid = (uint32_t)std::min<size_t>((n16 + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(encode_kernel, dim3(grid), dim3(256), 0, s, (uint4*)buf, n16);
}

}  // namespace sg
