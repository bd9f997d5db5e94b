// sg_kernels.hip -- hand-written gfx950 (CDNA4) kernels of the read-sampling pass.
//
// Mapping: one lane = one fragment slot (fragment_kernel) / one read (emit).  A wave's 64 reads are
// consecutive fragment slots of the same 1 kbp window(s), so their haplotype bytes share a few
// cache lines and their FASTQ records form one contiguous ~21 KB output range.  All sampling is
// integer work on u32 thresholds (sg_tables.h); the only fp64 is the window-start draw, which must
// round exactly like the reference's `start+(end-start)*(x/2^32)` (ThreadPool.cpp:208-212).
//
//   batch_map_kernel  when a batch is planned: slot -> window tables, edge windows, segments that hold one
//   edge_kernel      Segment::yieldReads draw loop of the windows whose attempts can fail (lib/segment/Segment.cpp:735-762,
//                    848) and the fragment numbers of their segments (Segment.cpp:732,763); clears the pass's counters
//   fragment_kernel  the draw of every other fragment, its number (slot order), and Profile::predict's indel pass
//                    (lib/profile/Profile.cpp:1607-1634, 1556-1574); writes the reads' rows
//   block_base_kernel  record offsets: in-block prefix by fragment_kernel, block and segment bases here (replaces the
//                    50 MB per-worker buffers + SeqWriter mutex, Segment.cpp:695-707,834-846;
//                    lib/seqwriter/SeqWriter.cpp:49-54)
//   emit_slow_kernel, emit_kernel (generic) + header_kernel
//                    Profile::predict sampling loop  (Profile.cpp:1636-1700) + FASTQ formatting
//                    (Segment.cpp:803-832)
// The straight-line emit kernel (emit_fast_kernel) is in sg_emit_fast.hip; what the emit kernels share -- the read row,
// the read-group runs, write_name -- in sg_emit.h.  The window planner's kernels are in sg_windows.hip, the general u32
// scan in sg_scan.hip.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "sg_emit.h"

namespace sg {

// lower bound over a {k0, T...} row (sg_tables.h)
__device__ __forceinline__ uint32_t row_search(const uint32_t* __restrict__ row, uint32_t lg, uint32_t x) {
  const uint32_t* T = row + 1;
  uint32_t pos = 0;
  for (uint32_t step = lg ? (1u << (lg - 1)) : 0; step; step >>= 1)
    if (x > T[pos + step - 1]) pos += step;
  return row[0] + pos;
}

// ------------------------------------------------------------------------------------------------
// plan draws.  The reference draws (start, insert size) attempts one after the other and counts failures per window
// (fragment shorter than a read: Segment.cpp:753-762); attempt t of window w has the address (w, t).  Interior ("safe")
// windows cannot fail -- every start leaves at least the largest insert size before the chain end -- so attempt t IS
// fragment t, and fragment_kernel draws it in the lane that owns the fragment's slot.  Windows near a chain end ("edge"
// windows) keep the attempt loop, in edge_kernel.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t planned_of(const sg_window& win, int32_t paired) {
  const int n = win.n_reads;
  return n <= 0 ? 0u : (paired ? ((uint32_t)n + 1u) / 2u : (uint32_t)n);
}

// can no attempt of this window fail?
__device__ __forceinline__ bool window_safe(const DevProfile& P, const DevBatch& B, const sg_window& win, uint64_t clen) {
  const uint64_t last_start = win.hap_base + win.spos + win.len - 1u;
  const uint64_t need = B.paired ? (uint64_t)P.isz_hi : (uint64_t)win.len;
  const uint32_t shortest = B.paired ? (uint32_t)P.isz_lo : win.len;
  return last_start + need <= clen && shortest >= (uint32_t)P.L;
}

// the part of a WinRow that a draw needs, from the window itself
__device__ __forceinline__ WinRow win_row_of(const sg_window& win, uint64_t clen, uint64_t chain_off, uint32_t seg_size) {
  WinRow wr = {};
  wr.hap_off = chain_off + win.hap_base;
  wr.room = clen - win.hap_base;
  wr.spos = win.spos; wr.len = win.len;
  wr.slot_base = win.slot_base; wr.seg_size = seg_size;
  return wr;
}

__device__ __forceinline__ bool plan_attempt(const DevProfile& P, const DevBatch& B, const WinRow& win, uint64_t w,
                                             uint32_t attempt, uint32_t c3, PairRec& r, const uint32_t* isz_row) {
  uint32_t x[4];
  philox4x32_10((uint32_t)w + B.win_offset, attempt, 0, c3, B.k0, B.k1, x);
  // threadPool->randomInteger(spos, epos+1): (long)(start + (end-start)*(x/2^32)) in fp64
  const double frac = __dmul_rn((double)x[0], 1.0 / 4294967296.0);
  const double v = __dadd_rn((double)win.spos, __dmul_rn((double)win.len, frac));
  const uint32_t pos = (uint32_t)(long long)v;
  uint32_t isz;
  if (B.paired) isz = isz_row ? (uint32_t)P.isz_min + row_search(isz_row, P.isz_lg, x[1]) : (uint32_t)P.fixed_isz;
  else isz = win.len;
  const uint64_t avail = win.room - pos;
  const uint32_t flen = avail < (uint64_t)isz ? (uint32_t)avail : isz;
  const uint32_t strand = B.paired ? 0u : (x[2] >> 31);  // randomInteger(0,2)
  r.win = (uint32_t)w; r.fl = flen | (strand << 31);
  r.namepos = pos % win.seg_size;
  r.foff = win.hap_off + pos;
  r.pad = 0;
  return flen >= (uint32_t)P.L;
}

// A batch's tables, made once when it is planned (finish_plan), one lane per window: the windows' first slots side by
// side (win_slot, [n_windows] = n_slots); their rows (WinRow); win_flag = is it an edge window | its segment << 1 (the
// one whose run of seg_first_window holds it: the segment of the fragment numbers); which segments hold an edge window;
// and for every block of 256 slots the window that owns its first slot.  seg_flag and seg_lost arrive cleared;
// batch_flag_kernel then tells every window of a flagged segment.
__global__ __launch_bounds__(256) void batch_map_kernel(DevProfile P, DevBatch B) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w > B.n_windows) return;
  if (w == B.n_windows) { B.win_slot[w] = B.n_slots; return; }
  const sg_window win = B.windows[w];
  const uint32_t planned = planned_of(win, B.paired);
  B.win_slot[w] = win.slot_base;
  const bool edge = planned != 0u && !window_safe(P, B, win, B.chain_len[win.chain]);
  uint32_t seg = 0;  // the last segment that starts at or before w
  for (uint32_t lo = 0, hi = B.n_segs; lo + 1u < hi;) {
    const uint32_t mid = (lo + hi) >> 1;
    if (B.seg_first_window[mid] <= w) seg = lo = mid; else hi = mid;
  }
  B.win_flag[w] = (edge ? 1u : 0u) | (seg << 1);
  if (edge) B.seg_flag[seg] = 1u;
  WinRow wr = win_row_of(win, B.chain_len[win.chain], B.chain_off[win.chain], B.seg_size[win.seg]);
  wr.name0 = win.slot_base - B.windows[B.seg_first_window[seg]].slot_base;
  wr.flags = edge ? 1u : 0u;
  B.win_rows[w] = wr;
  const uint64_t first = win.slot_base, end = first + planned, nblk = ((uint64_t)B.n_slots + 255u) >> 8;
  for (uint64_t b = (first + 255u) >> 8; b < nblk && (b << 8) < end; b++) B.blk_win[b] = (uint32_t)w;
}

__global__ __launch_bounds__(256) void batch_flag_kernel(DevBatch B) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w < B.n_windows && B.seg_flag[B.win_flag[w] >> 1]) B.win_rows[w].flags |= 2u;
}

// inclusive sum scan over the 256 lanes of a workgroup
__device__ __forceinline__ uint32_t block_scan256(uint32_t v, uint32_t* wave_part /* [4], LDS */, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(v, d, 64);
    if ((int)lane >= d) v += up;
  }
  __syncthreads();  // (wave_part may still be read from the call before)
  if (lane == 63u) wave_part[wv] = v;
  __syncthreads();
  uint32_t all = 0;
#pragma unroll
  for (uint32_t i = 0; i < 4u; i++) {
    const uint32_t p = wave_part[i];
    if (i < wv) v += p;
    all += p;
  }
  if (total) *total = all;
  return v;
}

// ------------------------------------------------------------------------------------------------
// edge windows: the pass's first kernel, one workgroup per segment; a segment without an edge window has nothing to do.
// An edge window's attempts are drawn 64 at a time by one wave: attempt a counts iff fewer than `planned` earlier
// attempts succeeded and at most 1000 earlier ones failed -- the sequential loop's `done < planned` and `++fail > 1000`
// -- and its fragment number is the count of the successes before it.  Then the segment's name bases: the exclusive
// scan of the fragments its windows produced (a safe window: what was planned).  What the segment gave up goes to
// seg_lost; fragment_kernel's first workgroup takes the sum from n_slots.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void edge_kernel(DevProfile P, DevBatch B) {
  __shared__ uint32_t isz_lds[1025];
  __shared__ uint32_t wave_part[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  // the pass's first kernel also clears its counters and results (nothing here uses them; one command less in the stream)
  if (blockIdx.x == 0)
    for (uint32_t i = tid; i < kTotalsBytes / 4u; i += blockDim.x) ((uint32_t*)B.totals)[i] = 0u;
  const uint32_t s = blockIdx.x;
  if (s >= B.n_segs || !B.seg_flag[s]) return;
  const uint32_t* isz_row = P.isz_row;
  if (P.isz_row && P.isz_lg <= 10u) {
    for (uint32_t i = tid; i < (1u << P.isz_lg) + 1u; i += blockDim.x) isz_lds[i] = P.isz_row[i];
    isz_row = isz_lds;
  }
  __syncthreads();
  const uint32_t c3 = dev_ctx(KIND_PLAN, 0, B.batch_id);
  const uint32_t w0 = B.seg_first_window[s], w1 = B.seg_first_window[s + 1];
  uint32_t carry = 0, lost = 0;
  for (uint32_t base = w0; base < w1; base += 256u) {
    const uint32_t wl = base + tid;
    sg_window mine = {};
    uint32_t produced = 0, planned_mine = 0;
    bool edge = false;
    if (wl < w1) {
      mine = B.windows[wl];
      produced = planned_mine = planned_of(mine, B.paired);
      edge = (B.win_flag[wl] & 1u) != 0u;
    }
    // the wave's edge windows, one after the other
    for (unsigned long long em = __ballot(edge); em; em &= em - 1ull) {
      const uint32_t src = (uint32_t)__builtin_ctzll(em);
      const uint32_t w = base + (tid & ~63u) + src;
      const sg_window sgw = B.windows[w];
      const uint32_t planned = planned_of(sgw, B.paired);
      const WinRow win = win_row_of(sgw, B.chain_len[sgw.chain], B.chain_off[sgw.chain], B.seg_size[sgw.seg]);
      uint32_t done = 0, fail = 0, first = 0;
      while (done < planned && fail <= 1000u) {
        PairRec r;
        const bool ok = plan_attempt(P, B, win, w, first + lane, c3, r, isz_row);
        const unsigned long long okm = __ballot(ok), below = (1ull << lane) - 1ull;
        const uint32_t ok_before = done + (uint32_t)__popcll(okm & below), fail_before = fail + (uint32_t)__popcll(~okm & below);
        const bool counts = ok_before < planned && fail_before <= 1000u;
        if (counts && ok) {
          r.k = ok_before;
          B.pairs[win.slot_base + ok_before] = r;
        }
        const unsigned long long cm = __ballot(counts);
        done += (uint32_t)__popcll(okm & cm);
        fail += (uint32_t)__popcll(~okm & cm);
        first += 64u;
      }
      for (uint32_t k = done + lane; k < planned; k += 64u) {  // given up: unused slots
        PairRec r;
        r.win = w; r.namepos = 0; r.fl = 0; r.k = k; r.foff = 0; r.pad = 0;
        B.pairs[win.slot_base + k] = r;
      }
      if (lane == src) produced = done;
    }
    uint32_t all = 0;
    const uint32_t incl = block_scan256(produced, wave_part, &all);
    if (wl < w1) B.win_namebase[wl] = carry + incl - produced;
    carry += all;
    lost += planned_mine - produced;
  }
  uint32_t all_lost = 0;
  block_scan256(lost, wave_part, &all_lost);
  if (tid == 0u) B.seg_lost[s] = all_lost;
}

// ------------------------------------------------------------------------------------------------
// fragment_kernel: one lane per fragment slot, 256 consecutive slots per workgroup -- the fragment's plan draw, its
// number, the indel pass of both of its reads (Profile::predict's first loop) and the reads' rows.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fragment_kernel(DevProfile P, DevBatch B) {
  // lane = fragment, both of its reads: what the two share -- the plan draw, the window's name base, the digits of the
  // name -- is made once.
  // The reads' 48-byte rows leave through LDS: written by their lanes (16 bytes and single characters at a stride of 48:
  // straight to memory every store instruction touched 64 cache lines), stored by the wave as 3 KB in one piece; mate 2's
  // rows reuse the space (its rows differ from mate 1's in the middle 16 bytes and in one character).
  // Before the rows are written the space serves the kernel's front: the insert-size row (words [0, 1028)) for the plan
  // draws, and behind it the first draws of the listed reads for their walk (cand_xy) and then what the walks found;
  // the reads' lanes take that into registers, and a barrier lies between that and the rows.
  __shared__ uint4 row_lds[256 * 3 + 2];
  uint32_t* const isz_lds = (uint32_t*)row_lds;
  ulonglong2* const cand_xy = (ulonglong2*)(row_lds + 257);
  // reads with at least one indel candidate (16 % at XTen rates), as local index | mate << 8.  A wave in which every lane
  // walks its own read's candidates pays for its unluckiest lane with most lanes idle; the listed reads are walked 64 to
  // a wave instead, and what a walk found -- events, length change, first event -- goes back in the place of the draw.
  __shared__ uint16_t cand[512];
  __shared__ uint32_t cand_n;
  __shared__ uint32_t wave_len[2][4];
  __shared__ uint32_t slot_lds[257];  // the first slots of the windows from the owner of the block's first slot on
  __shared__ uint32_t wave_part[4];
  __shared__ uint32_t indel_lds[2][65];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t s0 = blockIdx.x * blockDim.x;  // the block's first slot
  const uint32_t t = s0 + tid;
  const uint32_t nm = B.paired ? 2u : 1u;
  uint4* const wave_rows = row_lds + (tid & ~63u) * 3u;
  uint4* const my_row = wave_rows + lane * 3u;
  const uint32_t t_wave = t - lane;  // the wave's first slot
  const uint32_t L = (uint32_t)P.L;
  const bool in_batch = t < B.n_slots;
  // ---- tables staged by the whole block: indel distances (see below), indel lengths, insert sizes ----
  __shared__ uint64_t gap_lds[256];
  const uint64_t* gap = P.gap_row;
  if (L + 1u <= 256u) {  // (longer reads: from L2)
    for (uint32_t i = tid; i <= L; i += blockDim.x) gap_lds[i] = P.gap_row[i];
    gap = gap_lds;
  }
  const uint32_t* ins_row = P.ins_row;
  const uint32_t* del_row = P.del_row;
  if (P.ins_lg <= 6u) {
    if (tid < (1u << P.ins_lg) + 1u) indel_lds[0][tid] = P.ins_row[tid];
    ins_row = indel_lds[0];
  }
  if (P.del_lg <= 6u) {
    if (tid >= 128u && tid - 128u < (1u << P.del_lg) + 1u) indel_lds[1][tid - 128u] = P.del_row[tid - 128u];
    del_row = indel_lds[1];
  }
  const uint32_t* isz_row = P.isz_row;
  if (P.isz_row && P.isz_lg <= 10u) {
    for (uint32_t i = tid; i < (1u << P.isz_lg) + 1u; i += blockDim.x) isz_lds[i] = P.isz_row[i];
    isz_row = isz_lds;
  }
  // slot -> window: the block's windows are the owner of its first slot and the ones behind it
  const uint32_t first_win = B.blk_win[blockIdx.x];
  for (uint32_t i = tid; i < 257u; i += blockDim.x) {
    const uint64_t wi = (uint64_t)first_win + i;
    slot_lds[i] = wi <= B.n_windows ? B.win_slot[wi] : 0xFFFFFFFFu;
  }
  if (tid == 0u) cand_n = 0u;
  // fragments produced = planned - what the edge windows gave up (edge_kernel)
  if (blockIdx.x == 0u) {
    uint32_t lost = 0;
    for (uint32_t s = tid; s < B.n_segs; s += blockDim.x) lost += B.seg_lost[s];
    uint32_t all_lost = 0;
    block_scan256(lost, wave_part, &all_lost);
    if (tid == 0u) B.totals[2] = (uint64_t)B.n_slots - all_lost;
  }
  // ---- the reads' first indel test: needs the slot alone, covers the staging loads ----
  // Sequencing indels by skipping ahead (DevProfile::gap_row): every template position is an indel candidate with
  // probability evB / 2^64, independently, so the distance to the next one is geometric and is drawn directly -- call
  // (slot, e, 0) of the read's e-th candidate: x = words (1, 0) against the table P(no candidate in k positions),
  // y = words (3, 2): an insertion iff floor(y evB / 2^64) < evA.  A read without indels (84 % at XTen rates) costs ONE
  // call and ONE compare (x < gap[L]); testing every position took 19 calls per 151-base read.
  uint64_t x0[2] = {0, 0}, y0[2] = {0, 0};
#pragma unroll
  for (uint32_t m = 0; m < 2u; m++) {
    if (m >= nm) break;
    uint32_t x4[4];
    philox4x32_10(t + B.slot_offset, 0u, 0, dev_ctx(KIND_INDEL, m, B.batch_id), B.k0, B.k1, x4);
    x0[m] = ((uint64_t)x4[1] << 32) | x4[0];
    y0[m] = ((uint64_t)x4[3] << 32) | x4[2];
  }
  block_lds_sync();  // the staged tables, cand_n
  // ---- the fragment: a safe window's lane draws it, an edge window's takes what edge_kernel left ----
  PairRec rec = {};
  uint32_t fragcount = 0;
  if (in_batch) {
    // The slot's window is the last one that starts at or before it (empty windows share their first slot with the next
    // window that owns slots): among the 257 staged ones, or -- behind a run of more than 256 windows that start inside
    // the block -- further on.
    uint32_t at = 0;
#pragma unroll
    for (uint32_t step = 256u; step; step >>= 1)
      if (at + step <= 256u && slot_lds[at + step] <= t) at += step;
    uint32_t w = first_win + at;
    if (at == 256u) {
      uint64_t lo = w, hi = B.n_windows;  // win_slot[lo] <= t < win_slot[hi]
      while (lo + 1u < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (B.win_slot[mid] <= t) lo = mid; else hi = mid;
      }
      w = (uint32_t)lo;
    }
    const WinRow win = B.win_rows[w];
    const uint32_t k = t - win.slot_base;
    if (win.flags & 1u) rec = B.pairs[t];
    else {
      plan_attempt(P, B, win, w, k, dev_ctx(KIND_PLAN, 0, B.batch_id), rec, isz_row);
      rec.k = k;
    }
    fragcount = ((win.flags & 2u) ? B.win_namebase[w] : win.name0) + k + 1u;
  }
  const uint32_t flen = rec.fl & 0x7FFFFFFFu;
  const bool live = flen != 0u;
  if (!live) fragcount = 0;
  // What the reads' rows need beyond that: the bad-block bits.
  uint32_t touches_bad[2] = {0, 0};
  const uint64_t foff = rec.foff;
  const uint32_t rev1 = rec.fl >> 31;  // SE: the read's strand (PE: mate 1 forward, mate 2 reverse)
  if (live) {
    // A read's template is the first (forward) / last (reverse) L bases of the fragment; does it -- with the two context
    // bases before it and the slack of the emit kernel's last item -- touch a 64-base block holding a non-ACGT base?
    // Such reads go through the generic item code (the straight-line kernel reads 2-bit codes).  Up to 17 blocks (reads
    // of up to 1000 bases: L + 24 <= 1024) lie in one or two neighbouring 16-bit words and fit a 32-bit mask behind
    // the first block's bit; longer reads test their blocks one by one.
#pragma unroll
    for (uint32_t m = 0; m < 2u; m++) {
      if (m >= nm) break;
      const bool rev = B.paired ? (m == 1u) : (rev1 != 0u);
      const uint64_t t0 = (rev ? foff + flen - L : foff) - 8u, t1 = t0 + L + 24u;  // inside the guard bytes
      const uint64_t b0 = t0 >> 6, b1 = t1 >> 6, i0 = b0 >> 4, i1 = b1 >> 4;
      uint32_t bad = 0;
      if (b1 - b0 <= 16u) {  // then i1 <= i0 + 1 and (b0 & 15) + nb <= 32
        uint32_t bits = B.chains_bad[i0];
        if (i1 != i0) bits |= (uint32_t)B.chains_bad[i1] << 16;
        const uint32_t nb = (uint32_t)(b1 - b0) + 1u;  // 1 .. 17
        bad = ((bits >> (b0 & 15u)) & ((1u << nb) - 1u)) != 0u ? 1u : 0u;
      } else {
        for (uint64_t b = b0; b <= b1; b++) bad |= (B.chains_bad[b >> 4] >> (b & 15u)) & 1u;
      }
      touches_bad[m] = bad;
    }
  }
  // ---- the reads with a candidate, listed with their first draw ----
  uint32_t listed_at[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
#pragma unroll
  for (uint32_t m = 0; m < 2u; m++) {
    if (m >= nm) break;
    const bool has = live && !(x0[m] < gap[L]);
    const unsigned long long hm = __ballot(has);
    if (hm) {
      uint32_t base = 0;
      if (lane == (uint32_t)__builtin_ctzll(hm)) base = atomicAdd(&cand_n, (uint32_t)__popcll(hm));
      base = __shfl(base, __builtin_ctzll(hm), 64);
      if (has) {
        const uint32_t at = base + (uint32_t)__popcll(hm & ((1ull << lane) - 1ull));
        cand[at] = (uint16_t)(tid | (m << 8));
        cand_xy[at] = make_ulonglong2(x0[m], y0[m]);
        listed_at[m] = at;
      }
    }
  }
  block_lds_sync();
  {
    const uint32_t nc = cand_n;
#pragma unroll 1
    for (uint32_t i = tid; i < nc; i += blockDim.x) {
      const uint32_t e16 = cand[i], lt = e16 & 255u, m = e16 >> 8;
      const uint32_t tt = s0 + lt;
      uint32_t* ev = B.events + ((size_t)m * B.n_slots + tt) * SG_MAX_EVENTS;
      const uint32_t c3 = dev_ctx(KIND_INDEL, m, B.batch_id);
      int j = 0, dl = 0;
      uint32_t nev = 0, first_ev = 0, e = 1;
      // call e = 0 is the draw of the first test, made by the read's own lane
      const ulonglong2 xy = cand_xy[i];
      uint64_t x = xy.x, y = xy.y;
#pragma unroll 1
      for (;;) {
        const int room = (int)L - j;
        if (x < gap[room]) break;                 // no candidate before the read's end
        int lo = 0, hi = room - 1;                // g = #{k in [1, room): x < gap[k]} (gap decreases)
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (x < gap[mid]) lo = mid; else hi = mid - 1;
        }
        const int jj = j + lo;
        const bool is_ins = __umul64hi(y, P.evB) < P.evA;
        j = jj + 1;
        if (is_ins) {
          uint32_t len = row_search(ins_row, P.ins_lg, aux_draw(B, tt, (uint32_t)jj, 0, m));
          if (len > 0) {
            if (nev < SG_MAX_EVENTS) ev[nev] = ev_pack((uint32_t)jj, len, 0);
            if (nev == 0) first_ev = ev_pack((uint32_t)jj, len, 0);
            nev++;
            dl += (int)len;
          }
        } else {
          uint32_t len = row_search(del_row, P.del_lg, aux_draw(B, tt, (uint32_t)jj, 0, m));
          if (len > 0) {
            uint32_t k = min((uint32_t)((int)L - jj), len);
            if (nev < SG_MAX_EVENTS) ev[nev] = ev_pack((uint32_t)jj, k, 1);
            if (nev == 0) first_ev = ev_pack((uint32_t)jj, k, 1);
            nev++;
            dl -= (int)k;
            j = jj + (int)k;
          }
        }
        if (j >= (int)L) break;
        uint32_t x4[4];
        philox4x32_10(tt + B.slot_offset, e++, 0, c3, B.k0, B.k1, x4);
        x = ((uint64_t)x4[1] << 32) | x4[0];
        y = ((uint64_t)x4[3] << 32) | x4[2];
      }
      ((uint4*)cand_xy)[i] = make_uint4(nev, (uint32_t)dl, first_ev, 0u);
    }
  }
  block_lds_sync();
  uint4 found[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};  // {events, length change, first event}
#pragma unroll
  for (uint32_t m = 0; m < 2u; m++)
    if (m < nm && listed_at[m] != 0xFFFFFFFFu) found[m] = ((const uint4*)cand_xy)[listed_at[m]];
  block_lds_sync();  // the rows go where the walks' results were
  // ---- the reads' rows, their record lengths and the prefix of those inside the block ----
  // Per-read 48-byte row for the emit kernels (ReadRow, sg_emit.h): m0 = fragment offset + the two numbers of the read's
  // name "@popu#chr#pos%segsize#fragCount[/m]" (Segment.cpp:780,809,824), m1 = lengths, reciprocal, event, then the
  // name's own part "pos#count[/m]\n" as text when it fits 16 bytes (emit_fast_kernel stores it behind the batch's
  // constant prefix; this kernel has the VALU time for the digits, that one has not).
  const uint32_t namepos = rec.namepos;
  const uint32_t hdr = B.prefix_len + ndigits(namepos) + 1u + ndigits(fragcount) + (B.paired ? 2u : 0u) + 1u;
  uint32_t mate_at = 0;  // where the name's mate digit sits in the text
  my_row[0] = live ? ReadRow::make_m0(foff, namepos, fragcount) : make_uint4(0, 0, 0, 0);
  my_row[2] = make_uint4(0, 0, 0, 0);
  if (live && hdr - B.prefix_len <= 16u) {
    uint8_t* hb = (uint8_t*)(my_row + 2);
    uint32_t o = 0;
    auto put_dec = [&](uint32_t v) {  // the digits of a number from its last one backwards
      const uint32_t nd = ndigits(v);
      for (uint32_t k = nd; k-- > 0u;) {
        const uint32_t qd = v / 10u;
        hb[o + k] = (uint8_t)('0' + (v - qd * 10u));
        v = qd;
      }
      o += nd;
    };
    put_dec(namepos);
    hb[o++] = '#';
    put_dec(fragcount);
    if (B.paired) { hb[o++] = '/'; mate_at = o; hb[o++] = '1'; }
    hb[o] = '\n';
  }
  uint32_t rl[2] = {0, 0};
#pragma unroll
  for (uint32_t m = 0; m < 2u; m++) {
    if (m >= nm) break;
    if (m == 1u) {
      wave_lds_sync();  // mate 1's rows have been read
      if (mate_at) ((uint8_t*)(my_row + 2))[mate_at] = '2';
    }
    uint4 mid = make_uint4(0, 0, 0, 0);
    if (live) {
      const uint4 f = found[m];
      uint32_t nev = f.x;
      int dl = (int)f.y;
      if ((int)L + dl < 50) { nev = 0; dl = 0; }  // Profile.cpp:1627-1634
      if (nev > SG_MAX_EVENTS) { atomicOr((unsigned long long*)&B.totals[3], 1ull); nev = 0; dl = 0; }
      const uint32_t np = (uint32_t)((int)L + dl);
      rl[m] = hdr + 2u * np + 4u;
      const uint32_t rev = B.paired ? m : rev1;
      // (the reciprocal of np is made there; the event itself goes into the row for single-event reads, which the emit
      // kernels handle inline)
      mid = ReadRow::make_m1(flen, touches_bad[m], rev, np, nev, hdr, nev == 1u ? f.z : 0u);
    }
    my_row[1] = mid;
    if (t_wave < B.n_slots) {
      wave_lds_sync();
      uint4* dst = B.meta + ((size_t)m * B.n_slots + t_wave) * 3;
      const uint32_t n_pieces = min(B.n_slots - t_wave, 64u) * 3u;  // 16-byte pieces of the wave's rows that exist
#pragma unroll
      for (uint32_t i = 0; i < 3u; i++) {
        const uint32_t q = i * 64u + lane;
        if (q < n_pieces) dst[q] = wave_rows[q];
      }
    }
  }
  // Record offsets: exclusive prefix of the record lengths inside the block of 256 reads, here; the blocks' bases by
  // one small kernel afterwards (block_base_kernel).  offset = base[block] + prefix (rec_offset()).
  uint32_t incl[2];
#pragma unroll
  for (uint32_t m = 0; m < 2u; m++) {
    if (m >= nm) break;
    uint32_t v = rl[m];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(v, d, 64);
      if ((int)lane >= d) v += up;
    }
    incl[m] = v;
    if (lane == 63u) wave_len[m][wv] = v;
  }
  block_lds_sync();
#pragma unroll
  for (uint32_t m = 0; m < 2u; m++) {
    if (m >= nm) break;
    uint32_t base = 0, all = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) {
      const uint32_t w = wave_len[m][i];
      if (i < wv) base += w;
      all += w;
    }
    if (in_batch) B.recloc[(size_t)m * B.n_slots + t] = base + incl[m] - rl[m];
    if (tid == 0u) B.blkbase[(size_t)m * gridDim.x + blockIdx.x] = all;
  }
}

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

// Record offsets, middle level: the block sums fragment_kernel left in blkbase, cut into <= 16 segments of 2^seg_shift
// blocks; workgroup j scans segment j in place (thread i owns a run of consecutive sums), the workgroup that arrives
// last turns the 16 segment totals into segment bases and the mate's text size (totals[m]).  One launch, 16 CUs per
// mate busy instead of one.
__global__ __launch_bounds__(1024) void block_base_kernel(DevBatch B) {
  __shared__ uint64_t buf[1024];
  __shared__ uint32_t ticket;
  const uint32_t m = blockIdx.y, j = blockIdx.x;
  const uint32_t nblk = (B.n_slots + 255u) >> 8;
  uint64_t* b = B.blkbase + (size_t)m * nblk;
  uint64_t* segbase = (uint64_t*)((uint8_t*)B.totals + kTotalsSegBase) + m * 16u;
  uint32_t* arrived = (uint32_t*)((uint8_t*)B.totals + kTotalsSegBase + 2 * 16 * 8) + m;
  const uint32_t s0 = min(j << B.seg_shift, nblk), s1 = min((j + 1u) << B.seg_shift, nblk);
  const uint32_t run = ((s1 - s0) + 1023u) / 1024u;
  const uint32_t lo = min(s0 + threadIdx.x * run, s1), hi = min(lo + run, s1);
  uint64_t mine = 0;
  for (uint32_t i = lo; i < hi; i++) mine += b[i];
  buf[threadIdx.x] = mine;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint64_t t = threadIdx.x >= d ? buf[threadIdx.x - d] : 0;
    __syncthreads();
    buf[threadIdx.x] += t;
    __syncthreads();
  }
  uint64_t carry = buf[threadIdx.x] - mine;
  for (uint32_t i = lo; i < hi; i++) {
    const uint64_t v = b[i];
    b[i] = carry;
    carry += v;
  }
  if (threadIdx.x == 0) {
    __hip_atomic_store(&segbase[j], buf[1023], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    ticket = atomicAdd(arrived, 1u);
  }
  __syncthreads();
  if (ticket + 1u == gridDim.x && threadIdx.x == 0) {  // every segment total is in: bases, text size
    __threadfence();
    uint64_t acc = 0;
    for (uint32_t i = 0; i < gridDim.x; i++) {
      const uint64_t v = __hip_atomic_load(&segbase[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&segbase[i], acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      acc += v;
    }
    B.totals[m] = acc;
  }
}

// ------------------------------------------------------------------------------------------------
// emit: Profile::predict's sampling loop (Profile.cpp:1636-1700) + FASTQ formatting
// (Segment.cpp:803-832).
//
// Mapping (v3).  A wave owns G consecutive reads of one mate (one contiguous ~21 KB output range).
//   phase 0  lane = read: its 32-byte metadata row (written by fragment_kernel / header_kernel) into LDS.
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
void launch_batch_map(const DevProfile& P, const DevBatch& B, hipStream_t s) {  // (seg_flag, seg_lost: cleared by the caller)
  if (!B.n_windows) return;
  hipLaunchKernelGGL(batch_map_kernel, dim3((uint32_t)((B.n_windows + 1 + 255) / 256)), dim3(256), 0, s, P, B);
  hipLaunchKernelGGL(batch_flag_kernel, dim3((uint32_t)((B.n_windows + 255) / 256)), dim3(256), 0, s, B);
}
void launch_edge(const DevProfile& P, const DevBatch& B, hipStream_t s) {
  if (!B.n_windows) return;
  hipLaunchKernelGGL(edge_kernel, dim3(std::max(B.n_segs, 1u)), dim3(256), 0, s, P, B);
}
void launch_fragment(const DevProfile& P, const DevBatch& B, hipStream_t s) {
  if (!B.n_slots) return;
  hipLaunchKernelGGL(fragment_kernel, dim3((B.n_slots + 255) / 256), dim3(256), 0, s, P, B);
}
void launch_header(const DevProfile& P, const DevBatch& B, hipStream_t s) {
  if (!B.n_slots) return;
  const bool fast = emit_uses_fast_kernel(P, B);
  if (fast && B.prefix_len <= 16u) return;  // the straight-line kernel writes the names of its reads itself
  dim3 grid((B.n_slots + 255) / 256, B.paired ? 2 : 1);
  hipLaunchKernelGGL(header_kernel, grid, dim3(256), 0, s, B);
}
uint32_t record_seg_shift(uint32_t n_slots) {  // smallest shift with at most 16 segments of 2^shift blocks of 256 reads
  const uint32_t nblk = (n_slots + 255u) >> 8;
  uint32_t k = 0;
  while (((nblk + (1u << k) - 1u) >> k) > 16u) k++;
  return k;
}
void launch_scan(const DevBatch& B, hipStream_t s) {  // block sums of fragment_kernel -> block / segment bases, text sizes
  if (!B.n_slots) return;
  hipLaunchKernelGGL(block_base_kernel, dim3(16, B.paired ? 2 : 1), dim3(1024), 0, s, B);
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
