// sg_pass_front.hip -- the front of a sampling pass: the gfx950 (CDNA4) kernels in front of the emit kernels (sg_kernels.hip,
// sg_emit_fast.hip).  One lane = one fragment slot.  All sampling is integer work on u32 thresholds (sg_tables.h); the only
// fp64 is the window-start draw, which must round exactly like the reference's `start+(end-start)*(x/2^32)`
// (ThreadPool.cpp:208-212).
//   batch_map_kernel (+ batch_flag_kernel)  when a batch is planned: slot -> window tables, edge windows, their segments
//   edge_kernel      Segment::yieldReads draw loop of the windows whose attempts can fail (lib/segment/Segment.cpp:735-762,
//                    848) and the fragment numbers of their segments (Segment.cpp:732,763); clears the pass's counters
//   fragment_kernel  the draw of every other fragment, its number (slot order), and Profile::predict's indel pass
//                    (lib/profile/Profile.cpp:1607-1634, 1556-1574); writes the reads' rows (ReadRow, sg_emit.h)
//   block_base_kernel  record offsets: in-block prefix by fragment_kernel, block and segment bases here (replaces the
//                    50 MB per-worker buffers + SeqWriter mutex, Segment.cpp:695-707,834-846;
//                    lib/seqwriter/SeqWriter.cpp:49-54)
#include <algorithm>

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

// The insert-size row in LDS (isz_lds: (1 << 10) + 1 words) when it fits, for a workgroup's plan draws; the caller's barrier
// comes before the first draw.  No row: a fixed insert size.  (`&`: one branch, as when each kernel had this loop itself.)
__device__ __forceinline__ const uint32_t* stage_isz_row(const DevProfile& P, uint32_t* isz_lds, uint32_t tid) {
  const uint32_t* isz_row = P.isz_row;
  if ((P.isz_row != nullptr) & (P.isz_lg <= 10u)) {
    for (uint32_t i = tid; i < (1u << P.isz_lg) + 1u; i += blockDim.x) isz_lds[i] = P.isz_row[i];
    isz_row = isz_lds;
  }
  return isz_row;
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

// inclusive sum scan over the 64 lanes of a wave
__device__ __forceinline__ uint32_t wave_scan64(uint32_t v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(v, d, 64);
    if ((int)lane >= d) v += up;
  }
  return v;
}

// inclusive sum scan over the 256 lanes of a workgroup
__device__ __forceinline__ uint32_t block_scan256(uint32_t v, uint32_t* wave_part /* [4], LDS */, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  v = wave_scan64(v, lane);
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
// One wave draws edge window w, 64 attempts per round under the sequential loop's stopping rule, and leaves its
// fragments in B.pairs; returns how many it produced.
__device__ __forceinline__ uint32_t draw_edge_window(const DevProfile& P, const DevBatch& B, uint32_t w, uint32_t lane, uint32_t c3,
                                                     const uint32_t* isz_row) {
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
  return done;
}

// The name bases of 256 windows of a segment (lane's window: wl, if `have`): the fragments produced before them, `carry`
// of them by the segment's earlier windows.  Returns what the 256 produced.
__device__ __forceinline__ uint32_t store_name_bases(const DevBatch& B, uint32_t wl, bool have, uint32_t produced, uint32_t carry,
                                                     uint32_t* wave_part) {
  uint32_t all = 0;
  const uint32_t incl = block_scan256(produced, wave_part, &all);
  if (have) B.win_namebase[wl] = carry + incl - produced;
  return all;
}

__global__ __launch_bounds__(256) void edge_kernel(DevProfile P, DevBatch B) {
  __shared__ uint32_t isz_lds[1025];
  __shared__ uint32_t wave_part[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  // the pass's first kernel also clears its counters and results (nothing here uses them; one command less in the stream)
  if (blockIdx.x == 0)
    for (uint32_t i = tid; i < kTotalsBytes / 4u; i += blockDim.x) ((uint32_t*)B.totals)[i] = 0u;
  const uint32_t s = blockIdx.x;
  if (s >= B.n_segs || !B.seg_flag[s]) return;
  const uint32_t* isz_row = stage_isz_row(P, isz_lds, tid);
  __syncthreads();  // the insert-size row is staged
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
      const uint32_t done = draw_edge_window(P, B, base + (tid & ~63u) + src, lane, c3, isz_row);
      if (lane == src) produced = done;
    }
    carry += store_name_bases(B, wl, wl < w1, produced, carry, wave_part);
    lost += planned_mine - produced;
  }
  uint32_t all_lost = 0;
  block_scan256(lost, wave_part, &all_lost);
  if (tid == 0u) B.seg_lost[s] = all_lost;
}

// ------------------------------------------------------------------------------------------------
// fragment_kernel: one lane per fragment slot, 256 consecutive slots per workgroup -- the fragment's plan draw, its
// number, the indel pass of both of its reads (Profile::predict's first loop) and the reads' rows.
// lane = fragment, both of its reads: what the two share -- the plan draw, the window's name base, the digits of the
// name -- is made once.
//
// The kernel's LDS, all of it.  `space` (16-byte pieces) serves the kernel's front and then the rows:
//   the insert-size row for the plan draws, words [0, kIszWords): inside pieces [0, kCandAt);
//   from piece kCandAt on cand_xy, the first draws (x, y) of the listed reads for their walk, and IN THE DRAW'S PLACE
//   what the walk found, {events, length change, first event, 0}; the reads' lanes take that into registers, and a
//   barrier lies between that and the rows;
//   the rows, pieces [0, kRowPieces): three per lane (m0, m1, name text), a wave's 64 rows 3 KB in one piece.
// The reads' 48-byte rows leave through LDS: written by their lanes (16 bytes and single characters at a stride of 48:
// straight to memory every store instruction touched 64 cache lines), stored by the wave as 3 KB in one piece; mate 2's
// rows reuse the space (its rows differ from mate 1's in the middle 16 bytes and in one character).
// ------------------------------------------------------------------------------------------------
struct FrontLds {
  static constexpr uint32_t kIszWords = (1u << 10) + 1u, kCandAt = 257u, kCandMax = 2u * 256u, kRowPieces = 256u * 3u, kPieces = 770u;
  uint4 space[kPieces];
  uint64_t gap[256];        // DevProfile::gap_row of reads of up to 255 bases
  uint32_t wave_len[2][4];  // per mate: the record lengths of each wave's reads  } (16-byte aligned: read in one piece)
  uint32_t wave_part[4];    // block_scan256                                       }
  uint32_t slot[257];       // the first slots of the windows from the owner of the block's first slot on
  uint32_t indel[2][65];    // the insertion and the deletion length rows (ins_lg, del_lg <= 6)
  uint32_t cand_n;
  // reads with at least one indel candidate (16 % at XTen rates), as local index | mate << 8.  A wave in which every lane
  // walks its own read's candidates pays for its unluckiest lane with most lanes idle; the listed reads are walked 64 to
  // a wave instead, and what a walk found -- events, length change, first event -- goes back in the place of the draw.
  uint16_t cand[kCandMax];
  __device__ __forceinline__ uint32_t* isz() { return (uint32_t*)space; }
  __device__ __forceinline__ ulonglong2* cand_xy() { return (ulonglong2*)(space + kCandAt); }
  __device__ __forceinline__ uint4* found() { return space + kCandAt; }
  __device__ __forceinline__ uint4* wave_rows(uint32_t tid) { return space + (tid & ~63u) * 3u; }
};
static_assert(FrontLds::kIszWords * 4u <= FrontLds::kCandAt * 16u, "the insert-size row ends where cand_xy begins");
static_assert(FrontLds::kCandAt + FrontLds::kCandMax <= FrontLds::kPieces && sizeof(ulonglong2) == 16, "a draw, then a result, for both reads of every lane");
static_assert(FrontLds::kRowPieces <= FrontLds::kPieces, "three pieces per lane");
static_assert(sizeof(FrontLds) == 16992, "17 KB: eight waves per SIMD take at most 20 KB a workgroup");

// What the phases of fragment_kernel share: the lane's place and the tables (in LDS when they fit).
struct FrontBlock {
  const DevProfile& P;
  const DevBatch& B;
  FrontLds& lds;
  uint32_t tid, lane, wv;
  uint32_t s0, t, t_wave;  // the block's first slot, the lane's slot, the wave's first slot
  uint32_t nm, L;          // reads per fragment, bases per read
  bool in_batch;
  uint32_t first_win;      // the window that owns slot s0  } set by stage_tables_and_slots
  const uint64_t* gap;     // DevProfile::gap_row           }
  const uint32_t *ins_row, *del_row, *isz_row;
  __device__ __forceinline__ FrontBlock(const DevProfile& P_, const DevBatch& B_, FrontLds& lds_)
      : P(P_), B(B_), lds(lds_), tid(threadIdx.x), lane(threadIdx.x & 63u), wv(threadIdx.x >> 6), s0(blockIdx.x * blockDim.x),
        t(s0 + tid), t_wave(t - lane), nm(B_.paired ? 2u : 1u), L((uint32_t)P_.L), in_batch(t < B_.n_slots) {}
};

// the (x, y) of an indel draw: call (slot, e, 0) of the read's stream c3, x = words (1, 0), y = words (3, 2)
__device__ __forceinline__ ulonglong2 indel_draw(const DevBatch& B, uint32_t slot, uint32_t e, uint32_t c3) {
  uint32_t x4[4];
  philox4x32_10(slot + B.slot_offset, e, 0, c3, B.k0, B.k1, x4);
  return make_ulonglong2(((uint64_t)x4[1] << 32) | x4[0], ((uint64_t)x4[3] << 32) | x4[2]);
}

// ---- tables staged by the whole block: indel distances (first_indel_draws), indel lengths, insert sizes; the slot map;
// the empty list; and in the first workgroup the pass's count of fragments ----
__device__ __forceinline__ void stage_tables_and_slots(FrontBlock& k) {
  const DevProfile& P = k.P;
  const DevBatch& B = k.B;
  const uint32_t tid = k.tid, nt = blockDim.x;  // (read once: under `blockIdx.x == 0` it became a load of its own)
  k.gap = P.gap_row;
  if (k.L + 1u <= 256u) {  // (longer reads: from L2)
    for (uint32_t i = tid; i <= k.L; i += nt) k.lds.gap[i] = P.gap_row[i];
    k.gap = k.lds.gap;
  }
  k.ins_row = P.ins_row;
  k.del_row = P.del_row;
  if (P.ins_lg <= 6u) {
    if (tid < (1u << P.ins_lg) + 1u) k.lds.indel[0][tid] = P.ins_row[tid];
    k.ins_row = k.lds.indel[0];
  }
  if (P.del_lg <= 6u) {
    if (tid >= 128u && tid - 128u < (1u << P.del_lg) + 1u) k.lds.indel[1][tid - 128u] = P.del_row[tid - 128u];
    k.del_row = k.lds.indel[1];
  }
  k.isz_row = stage_isz_row(P, k.lds.isz(), tid);
  // slot -> window: the block's windows are the owner of its first slot and the ones behind it
  k.first_win = B.blk_win[blockIdx.x];
  for (uint32_t i = tid; i < 257u; i += nt) {
    const uint64_t wi = (uint64_t)k.first_win + i;
    k.lds.slot[i] = wi <= B.n_windows ? B.win_slot[wi] : 0xFFFFFFFFu;
  }
  if (tid == 0u) k.lds.cand_n = 0u;
  // fragments produced = planned - what the edge windows gave up (edge_kernel)
  if (blockIdx.x == 0u) {
    uint32_t lost = 0;
    for (uint32_t s = tid; s < B.n_segs; s += nt) lost += B.seg_lost[s];
    uint32_t all_lost = 0;
    block_scan256(lost, k.lds.wave_part, &all_lost);
    if (tid == 0u) B.totals[2] = (uint64_t)B.n_slots - all_lost;
  }
}

// ---- the reads' first indel test: needs the slot alone, covers the staging loads ----
// Sequencing indels by skipping ahead (DevProfile::gap_row): every template position is an indel candidate with
// probability evB / 2^64, independently, so the distance to the next one is geometric and is drawn directly -- call
// (slot, e, 0) of the read's e-th candidate: x = words (1, 0) against the table P(no candidate in k positions),
// y = words (3, 2): an insertion iff floor(y evB / 2^64) < evA.  A read without indels (84 % at XTen rates) costs ONE
// call and ONE compare (x < gap[L]); testing every position took 19 calls per 151-base read.
// (x0, y0 stay two arrays of scalars: handed on as one array of pairs, the compiler moved the calls behind the barrier.)
__device__ __forceinline__ void first_indel_draws(const FrontBlock& k, uint64_t (&x0)[2], uint64_t (&y0)[2]) {
#pragma unroll
  for (uint32_t m = 0; m < 2u; m++) {
    if (m >= k.nm) break;
    const ulonglong2 xy = indel_draw(k.B, k.t, 0u, dev_ctx(KIND_INDEL, m, k.B.batch_id));
    x0[m] = xy.x; y0[m] = xy.y;
  }
}

// The slot's window is the last one that starts at or before it (empty windows share their first slot with the next
// window that owns slots): among the 257 staged ones, or -- behind a run of more than 256 windows that start inside
// the block -- further on.
__device__ __forceinline__ uint32_t window_of_slot(const FrontBlock& k) {
  uint32_t at = 0;
#pragma unroll
  for (uint32_t step = 256u; step; step >>= 1)
    if (at + step <= 256u && k.lds.slot[at + step] <= k.t) at += step;
  const uint32_t w = k.first_win + at;
  return at == 256u ? slot_window(k.B, k.t, w) : w;
}

// ---- the fragment: a safe window's lane draws it, an edge window's takes what edge_kernel left.  Returns its number
// (0: the slot holds none) ----
__device__ __forceinline__ uint32_t fragment_of_slot(const FrontBlock& k, PairRec& rec) {
  const DevBatch& B = k.B;
  uint32_t fragcount = 0;
  if (k.in_batch) {
    const uint32_t w = window_of_slot(k);
    const WinRow win = B.win_rows[w];
    const uint32_t n = k.t - win.slot_base;
    if (win.flags & 1u) rec = B.pairs[k.t];
    else {
      plan_attempt(k.P, B, win, w, n, dev_ctx(KIND_PLAN, 0, B.batch_id), rec, k.isz_row);
      rec.k = n;
    }
    fragcount = ((win.flags & 2u) ? B.win_namebase[w] : win.name0) + n + 1u;
  }
  return (rec.fl & 0x7FFFFFFFu) != 0u ? fragcount : 0u;
}

// What the reads' rows need beyond that: the bad-block bits.
// A read's template is the first (forward) / last (reverse) L bases of the fragment; does it -- with the two context
// bases before it and the slack of the emit kernel's last item -- touch a 64-base block holding a non-ACGT base?
// Such reads go through the generic item code (the straight-line kernel reads 2-bit codes).  Up to 17 blocks (reads
// of up to 1000 bases: L + 24 <= 1024) lie in one or two neighbouring 16-bit words and fit a 32-bit mask behind
// the first block's bit; longer reads test their blocks one by one.
__device__ __forceinline__ void bad_block_bits(const FrontBlock& k, const PairRec& rec, uint32_t (&touches_bad)[2]) {
  const DevBatch& B = k.B;
  const uint32_t flen = rec.fl & 0x7FFFFFFFu, L = k.L;
  const uint64_t foff = rec.foff;
  if (flen == 0u) return;
#pragma unroll
  for (uint32_t m = 0; m < 2u; m++) {
    if (m >= k.nm) break;
    const bool rev = B.paired ? (m == 1u) : ((rec.fl >> 31) != 0u);
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
__device__ __forceinline__ void list_candidates(const FrontBlock& k, bool live, const uint64_t (&x0)[2], const uint64_t (&y0)[2], uint32_t (&listed_at)[2]) {
#pragma unroll
  for (uint32_t m = 0; m < 2u; m++) {
    if (m >= k.nm) break;
    const bool has = live && !(x0[m] < k.gap[k.L]);
    const unsigned long long hm = __ballot(has);
    if (hm) {
      uint32_t base = 0;
      if (k.lane == (uint32_t)__builtin_ctzll(hm)) base = atomicAdd(&k.lds.cand_n, (uint32_t)__popcll(hm));
      base = __shfl(base, __builtin_ctzll(hm), 64);
      if (has) {
        const uint32_t at = base + (uint32_t)__popcll(hm & ((1ull << k.lane) - 1ull));
        k.lds.cand[at] = (uint16_t)(k.tid | (m << 8));
        k.lds.cand_xy()[at] = make_ulonglong2(x0[m], y0[m]);
        listed_at[m] = at;
      }
    }
  }
}

// ---- the walk of the listed reads, one lane each: the read's events to B.events, what it found in the draw's place ----
__device__ __forceinline__ void walk_listed(const FrontBlock& k) {
  const DevProfile& P = k.P;
  const DevBatch& B = k.B;
  const uint32_t L = k.L, nc = k.lds.cand_n;
#pragma unroll 1
  for (uint32_t i = k.tid; i < nc; i += blockDim.x) {
    const uint32_t e16 = k.lds.cand[i], lt = e16 & 255u, m = e16 >> 8;
    const uint32_t tt = k.s0 + lt;
    uint32_t* ev = B.events + ((size_t)m * B.n_slots + tt) * SG_MAX_EVENTS;
    const uint32_t c3 = dev_ctx(KIND_INDEL, m, B.batch_id);
    int j = 0, dl = 0;
    uint32_t nev = 0, first_ev = 0, e = 1;
    auto record_event = [&](uint32_t at, uint32_t len, uint32_t del) {
      if (nev < SG_MAX_EVENTS) ev[nev] = ev_pack(at, len, del);
      if (nev == 0) first_ev = ev_pack(at, len, del);
      nev++;
    };
    // call e = 0 is the draw of the first test, made by the read's own lane
    ulonglong2 xy = k.lds.cand_xy()[i];
#pragma unroll 1
    for (;;) {
      const int room = (int)L - j;
      if (xy.x < k.gap[room]) break;            // no candidate before the read's end
      int lo = 0, hi = room - 1;                // g = #{k in [1, room): x < gap[k]} (gap decreases)
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (xy.x < k.gap[mid]) lo = mid; else hi = mid - 1;
      }
      const int jj = j + lo;
      const bool is_ins = __umul64hi(xy.y, P.evB) < P.evA;
      j = jj + 1;
      if (is_ins) {
        uint32_t len = row_search(k.ins_row, P.ins_lg, aux_draw(B, tt, (uint32_t)jj, 0, m));
        if (len > 0) {
          record_event((uint32_t)jj, len, 0);
          dl += (int)len;
        }
      } else {
        uint32_t len = row_search(k.del_row, P.del_lg, aux_draw(B, tt, (uint32_t)jj, 0, m));
        if (len > 0) {
          uint32_t n = min((uint32_t)((int)L - jj), len);  // clipped at the read's end
          record_event((uint32_t)jj, n, 1);
          dl -= (int)n;
          j = jj + (int)n;
        }
      }
      if (j >= (int)L) break;
      xy = indel_draw(B, tt, e++, c3);
    }
    k.lds.found()[i] = make_uint4(nev, (uint32_t)dl, first_ev, 0u);
  }
}

// ---- the walks' results back to their reads' lanes: {events, length change, first event} ----
__device__ __forceinline__ void take_results(const FrontBlock& k, const uint32_t (&listed_at)[2], uint4 (&found)[2]) {
#pragma unroll
  for (uint32_t m = 0; m < 2u; m++)
    if (m < k.nm && listed_at[m] != 0xFFFFFFFFu) found[m] = k.lds.found()[listed_at[m]];
}

// ---- the reads' rows ----
// Per-read 48-byte row for the emit kernels (ReadRow, sg_emit.h): m0 = fragment offset + the two numbers of the read's
// name "@popu#chr#pos%segsize#fragCount[/m]" (Segment.cpp:780,809,824), m1 = lengths, reciprocal, event, then the
// name's own part "pos#count[/m]\n" as text when it fits 16 bytes (emit_fast_kernel stores it behind the batch's
// constant prefix; this kernel has the VALU time for the digits, that one has not).
// Here: m0 and the text into the lane's row in LDS.  Returns the name line's length; mate_at: where the name's mate digit
// sits in the text (0: no text).
__device__ __forceinline__ uint32_t name_into_row(const FrontBlock& k, const PairRec& rec, uint32_t fragcount, uint32_t& mate_at) {
  const DevBatch& B = k.B;
  uint4* const my_row = k.lds.wave_rows(k.tid) + k.lane * 3u;
  const bool live = (rec.fl & 0x7FFFFFFFu) != 0u;
  const uint32_t namepos = rec.namepos;
  const uint32_t hdr = B.prefix_len + ndigits(namepos) + 1u + ndigits(fragcount) + (B.paired ? 2u : 0u) + 1u;
  my_row[0] = live ? ReadRow::make_m0(rec.foff, namepos, fragcount) : make_uint4(0, 0, 0, 0);
  my_row[2] = make_uint4(0, 0, 0, 0);
  if (live && hdr - B.prefix_len <= 16u) {
    uint8_t* hb = (uint8_t*)(my_row + 2);
    uint32_t o = 0;
    auto put_dec = [&](uint32_t v) {  // the digits of a number from its last one backwards
      const uint32_t nd = ndigits(v);
      for (uint32_t d = nd; d-- > 0u;) {
        const uint32_t qd = v / 10u;
        hb[o + d] = (uint8_t)('0' + (v - qd * 10u));
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
  return hdr;
}

// Each mate's m1 into the rows, and the wave's rows from LDS to B.meta; rl: the reads' record lengths.
__device__ __forceinline__ void store_rows(const FrontBlock& k, const PairRec& rec, const uint32_t (&touches_bad)[2], const uint4 (&found)[2],
                                           uint32_t hdr, uint32_t mate_at, uint32_t (&rl)[2]) {
  const DevBatch& B = k.B;
  uint4* const wave_rows = k.lds.wave_rows(k.tid);
  uint4* const my_row = wave_rows + k.lane * 3u;
  const uint32_t flen = rec.fl & 0x7FFFFFFFu, L = k.L;
#pragma unroll
  for (uint32_t m = 0; m < 2u; m++) {
    if (m >= k.nm) break;
    if (m == 1u) {
      wave_lds_sync();  // mate 1's rows have been read
      if (mate_at) ((uint8_t*)(my_row + 2))[mate_at] = '2';
    }
    uint4 mid = make_uint4(0, 0, 0, 0);
    if (flen != 0u) {
      const uint4 f = found[m];
      uint32_t nev = f.x;
      int dl = (int)f.y;
      if ((int)L + dl < 50) { nev = 0; dl = 0; }  // Profile.cpp:1627-1634
      if (nev > SG_MAX_EVENTS) { atomicOr((unsigned long long*)&B.totals[3], 1ull); nev = 0; dl = 0; }
      const uint32_t np = (uint32_t)((int)L + dl);
      rl[m] = hdr + 2u * np + 4u;
      const uint32_t rev = B.paired ? m : rec.fl >> 31;  // SE: the read's strand (PE: mate 1 forward, mate 2 reverse)
      // (the reciprocal of np is made there; the event itself goes into the row for single-event reads, which the emit
      // kernels handle inline)
      mid = ReadRow::make_m1(flen, touches_bad[m], rev, np, nev, hdr, nev == 1u ? f.z : 0u);
    }
    my_row[1] = mid;
    if (k.t_wave < B.n_slots) {
      wave_lds_sync();  // the wave's rows are whole
      uint4* dst = B.meta + ((size_t)m * B.n_slots + k.t_wave) * 3;
      const uint32_t n_pieces = min(B.n_slots - k.t_wave, 64u) * 3u;  // 16-byte pieces of the wave's rows that exist
#pragma unroll
      for (uint32_t i = 0; i < 3u; i++) {
        const uint32_t q = i * 64u + k.lane;
        if (q < n_pieces) dst[q] = wave_rows[q];
      }
    }
  }
}

// Record offsets: exclusive prefix of the record lengths inside the block of 256 reads, here; the blocks' bases by
// one small kernel afterwards (block_base_kernel).  offset = base[block] + prefix (rec_offset()).
// First the prefix inside the wave and the waves' sums ...
__device__ __forceinline__ void scan_record_lengths(const FrontBlock& k, const uint32_t (&rl)[2], uint32_t (&incl)[2]) {
#pragma unroll
  for (uint32_t m = 0; m < 2u; m++) {
    if (m >= k.nm) break;
    incl[m] = wave_scan64(rl[m], k.lane);
    if (k.lane == 63u) k.lds.wave_len[m][k.wv] = incl[m];
  }
}

// ... then, with the sums of the waves before: the reads' prefixes and the block's sum.
__device__ __forceinline__ void store_record_prefix(const FrontBlock& k, const uint32_t (&rl)[2], const uint32_t (&incl)[2]) {
  const DevBatch& B = k.B;
#pragma unroll
  for (uint32_t m = 0; m < 2u; m++) {
    if (m >= k.nm) break;
    uint32_t base = 0, all = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) {
      const uint32_t w = k.lds.wave_len[m][i];
      if (i < k.wv) base += w;
      all += w;
    }
    if (k.in_batch) B.recloc[(size_t)m * B.n_slots + k.t] = base + incl[m] - rl[m];
    if (k.tid == 0u) B.blkbase[(size_t)m * gridDim.x + blockIdx.x] = all;
  }
}

__global__ __launch_bounds__(256) void fragment_kernel(DevProfile P, DevBatch B) {
  __shared__ FrontLds lds;
  FrontBlock k(P, B, lds);
  stage_tables_and_slots(k);
  uint64_t x0[2] = {0, 0}, y0[2] = {0, 0};
  first_indel_draws(k, x0, y0);
  block_lds_sync();  // staging | the plan draws and the list: the tables, the slot map, cand_n
  PairRec rec = {};
  const uint32_t fragcount = fragment_of_slot(k, rec);
  uint32_t touches_bad[2] = {0, 0};
  bad_block_bits(k, rec, touches_bad);
  uint32_t listed_at[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
  list_candidates(k, (rec.fl & 0x7FFFFFFFu) != 0u, x0, y0, listed_at);
  block_lds_sync();  // listing | the walks: the list is whole
  walk_listed(k);
  block_lds_sync();  // the walks | their reads' lanes: the results are in the draws' place
  uint4 found[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
  take_results(k, listed_at, found);
  block_lds_sync();  // results taken | the rows, which go where the results were
  uint32_t mate_at = 0, rl[2] = {0, 0}, incl[2];
  const uint32_t hdr = name_into_row(k, rec, fragcount, mate_at);
  store_rows(k, rec, touches_bad, found, hdr, mate_at, rl);
  scan_record_lengths(k, rl, incl);
  block_lds_sync();  // the waves' sums | the prefixes over them
  store_record_prefix(k, rl, incl);
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
// launchers (declared in sg_device.h)
// ------------------------------------------------------------------------------------------------
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

}  // namespace sg
