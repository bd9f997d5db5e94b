// sg_windows.hip -- hand-written gfx950 (CDNA4) kernels of the device window planner (sg_api_windows.cpp): GC% and
// GC-bias weight of the sampling windows, their tiling from generators, and the batch table of a sampling plan.
//
//   gc_kernel          calculateGCPercent            (lib/mydefine/MyDefine.cpp:279-303)
//   gc_weight_kernel   Profile::getGCFactor          (lib/profile/Profile.cpp:1507-1517; Segment.cpp:576,586,615)
//   tile_kernel        Segment::getWeightedLength's tiles (Segment.cpp:566-590), seg_sum_kernel its sum (:627-630)
//   window_reads_kernel, seg_remainder_kernel        Segment::setReadCount (Segment.cpp:462-476)
//   planned_kernel, slot_base_kernel, seg_slots_kernel, slice_kernel   the sg_window rows of a batch and of a run of it
#include "sg_philox.h"
#include "sg_scan.h"
#include "sg_windows.h"

namespace sg {

// ------------------------------------------------------------------------------------------------
// GC% per window: one wave per window, 16 B per lane per step
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t count_eq_bytes(uint32_t w, uint32_t c) {
  uint32_t x = w ^ (c * 0x01010101u);
  uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
  t = ~(t | x | 0x7F7F7F7Fu);  // 0x80 in every byte of x that is zero
  return __popc(t);
}

__global__ __launch_bounds__(256) void gc_kernel(const uint8_t* __restrict__ chains, const uint64_t* __restrict__ chain_off,
                                                 const sg_gc_window* __restrict__ wins, uint64_t n, int32_t* __restrict__ out) {
  const uint64_t w = (uint64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (w >= n) return;
  const sg_gc_window win = wins[w];
  const uint8_t* p = chains + chain_off[win.chain] + win.start;
  uint32_t gc = 0, nn = 0;
  for (uint32_t b = lane * 16; b < win.len; b += 64 * 16) {
    uint32_t v[4];
    __builtin_memcpy(v, p + b, 16);
    const uint32_t rem = win.len - b;  // bytes of this 16-byte group inside the window
#pragma unroll
    for (int i = 0; i < 4; i++) {
      uint32_t x = v[i];
      const int left = (int)rem - 4 * i;
      if (left <= 0) x = 0;
      else if (left < 4) x &= (1u << (8 * left)) - 1u;  // masked-off bytes read as 0 = 'A': neither GC nor N
      gc += count_eq_bytes(x, 1u) + count_eq_bytes(x, 3u);  // encoded C, G
      nn += count_eq_bytes(x, 4u);                           // encoded N
    }
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    gc += __shfl_xor(gc, d);
    nn += __shfl_xor(nn, d);
  }
  if (lane == 0) out[w] = win.len == 0 ? 0 : (nn > 0 ? -1 : (int32_t)(100u * gc / win.len));
}

// GC factor and weight of a window (Profile::getGCFactor, Profile.cpp:1507-1517; Segment.cpp:576,586,615): one lane
// per window, the normal variate interpolated from the quantile table in three rounded fp64 operations (no fused
// multiply-add: the host / oracle evaluation of the same table must give the same bits)
__global__ __launch_bounds__(256) void gc_weight_kernel(const int32_t* __restrict__ gc, const sg_gc_window* __restrict__ wins,
                                                        const uint32_t* __restrict__ seg_ord, const uint32_t* __restrict__ win_ord,
                                                        uint64_t n, const double* __restrict__ means, double std,
                                                        const double* __restrict__ Q, uint32_t lg_cells, uint32_t frag,
                                                        int32_t full_tile_form, uint32_t c3, uint32_t k0, uint32_t k1,
                                                        double* __restrict__ out) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  const int32_t g = gc[w];
  double f = 0.0;
  if (g >= 0 && g <= 100) {
    const double mean = means[g];
    const uint32_t tail_bits = 32u - lg_cells;
    const double scale = 1.0 / (double)(1ull << (tail_bits + 1u));
    for (uint32_t a = 0;; a++) {
      uint32_t x[4];
      philox4x32_10(win_ord[w], a, seg_ord[w], c3, k0, k1, x);
      const uint32_t k = x[0] >> tail_bits, fr = x[0] & ((1u << tail_bits) - 1u);
      const double t = __dmul_rn((double)(2u * fr + 1u), scale);
      const double d = __dsub_rn(Q[k + 1], Q[k]);
      const double z = __dadd_rn(Q[k], __dmul_rn(d, t));
      f = __dadd_rn(mean, __dmul_rn(std, z));
      if (f >= 0.0) break;
    }
  }
  const uint32_t len = wins[w].len;
  out[w] = (full_tile_form && len == frag) ? __ddiv_rn(f, (double)frag)
                                           : __ddiv_rn(__dmul_rn(f, (double)len), (double)((uint64_t)frag * frag));
}

// ------------------------------------------------------------------------------------------------
// sampling plan on the device (sg_windows_build / sg_plan_windows / sg_plan_range)
// ------------------------------------------------------------------------------------------------
// generator of window w: the last one whose prefix (first window) is <= w
__device__ __forceinline__ uint32_t gen_of(const uint64_t* __restrict__ prefix, uint32_t n_gens, uint64_t w) {
  uint32_t lo = 0, hi = n_gens - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= w) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// lane = window: geometry of the tile (Segment.cpp:566-590), its segment and its ordinal inside the segment
__global__ __launch_bounds__(256) void tile_kernel(const sg_window_gen* __restrict__ gens, const uint64_t* __restrict__ prefix,
                                                   uint32_t n_gens, uint64_t n, uint32_t frag, const uint64_t* __restrict__ seg_first,
                                                   sg_gc_window* __restrict__ out, uint32_t* __restrict__ seg_ord, uint32_t* __restrict__ win_ord) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  const uint32_t g = gen_of(prefix, n_gens, w);
  const sg_window_gen G = gens[g];
  const uint64_t t = w - prefix[g], off = t * frag;
  sg_gc_window o;
  o.start = G.hap_base + off;
  o.chain = G.chain;
  o.len = (uint32_t)(G.hap_len - off < frag ? G.hap_len - off : frag);
  out[w] = o;
  seg_ord[w] = G.seg;
  win_ord[w] = (uint32_t)(w - seg_first[G.seg]);
}
// workgroup = segment: weight sum in window order (the reference's summation order, Segment.cpp:627-630; fp64 addition
// does not reassociate).  The whole workgroup stages tiles of the weights in LDS (coalesced), its first lane adds them
// one after the other: the chain of dependent adds is all that is serial (one lane per segment reading its weights
// from memory itself took 0.27 ms for 65 segments of 2000 windows).
#define SEG_SUM_TILE 4096
__global__ __launch_bounds__(256) void seg_sum_kernel(const double* __restrict__ wt, const uint64_t* __restrict__ seg_first, uint32_t n_segs,
                                                      double* __restrict__ out) {
  __shared__ double tile[SEG_SUM_TILE];
  const uint32_t k = blockIdx.x;
  const uint64_t w0 = seg_first[k], w1 = seg_first[k + 1];
  double acc = 0.0;
  for (uint64_t base = w0; base < w1; base += SEG_SUM_TILE) {
    const uint32_t n = (uint32_t)(w1 - base < SEG_SUM_TILE ? w1 - base : SEG_SUM_TILE);
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) tile[i] = wt[base + i];
    __syncthreads();
    if (threadIdx.x == 0u)
      for (uint32_t i = 0; i < n; i++) acc = __dadd_rn(acc, tile[i]);
    __syncthreads();
  }
  if (threadIdx.x == 0u) out[k] = acc;
}
// lane = window of an active segment: fragRCs[i] = (long)(fragWeights[i] * readCount / totalWL), Segment.cpp:466-470
__global__ __launch_bounds__(256) void window_reads_kernel(const sg_window_gen* __restrict__ gens, const uint64_t* __restrict__ prefix,
                                                           uint32_t n_gens, uint64_t n, uint32_t frag, const double* __restrict__ wt,
                                                           const sg_active_seg* __restrict__ act, sg_window* __restrict__ rows,
                                                           unsigned long long* __restrict__ seg_sum) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = w < n;
  uint32_t seg = 0xFFFFFFFFu;
  long long rc = 0;
  if (valid) {
    const uint32_t g = gen_of(prefix, n_gens, w);
    const sg_window_gen G = gens[g];
    const uint64_t t = w - prefix[g], off = t * frag;
    const sg_active_seg A = act[G.seg];
    const double total = __dadd_rn(A.weight, 2.2204e-16);
    rc = (long long)__ddiv_rn(__dmul_rn(wt[G.first_window + t], (double)A.reads), total);
    sg_window o;
    o.hap_base = G.hap_base;
    o.chain = G.chain;
    o.spos = (uint32_t)off;
    o.len = (uint32_t)(G.hap_len - off < frag ? G.hap_len - off : frag);
    o.n_reads = (int32_t)rc;
    o.seg = G.seg;
    o.slot_base = 0;
    rows[w] = o;
    seg = G.seg;
  }
  // The segment's sum (an integer: any order): a wave's windows are nearly always of ONE segment -- one atomic for the
  // wave then, not 64 on the same address (64 k single-address atomics were 0.37 ms of this kernel's 0.38).
  const uint32_t seg0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg);  // (the first lane of a wave that has one is valid)
  if (__ballot(valid && seg != seg0) == 0ull) {
    unsigned long long sum = (unsigned long long)rc;  // 0 on the lanes past n
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_down(sum, d, 64);
    if ((threadIdx.x & 63u) == 0u && valid) atomicAdd(seg_sum + seg0, sum);
  } else if (valid) {
    atomicAdd(seg_sum + seg, (unsigned long long)rc);
  }
}
// lane = active segment: the remainder goes to the segment's first window (Segment.cpp:472-474)
__global__ __launch_bounds__(64) void seg_remainder_kernel(const sg_active_seg* __restrict__ act, const uint32_t* __restrict__ seg_first,
                                                           uint32_t n_act, const unsigned long long* __restrict__ seg_sum,
                                                           sg_window* __restrict__ rows) {
  const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n_act) return;
  const long long sum = (long long)seg_sum[a];
  if (sum < act[a].reads) rows[seg_first[a]].n_reads += (int32_t)(act[a].reads - sum);
}
__global__ __launch_bounds__(256) void planned_kernel(const sg_window* __restrict__ rows, uint64_t n, int32_t paired, uint32_t* __restrict__ planned) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  const int32_t r = rows[w].n_reads;
  planned[w] = r <= 0 ? 0u : (paired ? ((uint32_t)r + 1u) / 2u : (uint32_t)r);
}
__global__ __launch_bounds__(256) void slot_base_kernel(sg_window* __restrict__ rows, uint64_t n, const uint64_t* __restrict__ off) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w < n) rows[w].slot_base = (uint32_t)off[w];
}
// planned fragments before each active segment's first window (and the total in [n_act])
__global__ __launch_bounds__(64) void seg_slots_kernel(const uint64_t* __restrict__ off, const uint32_t* __restrict__ seg_first, uint32_t n_act,
                                                       const uint64_t* __restrict__ total, uint64_t* __restrict__ out) {
  const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a < n_act) out[a] = off[seg_first[a]];
  if (a == n_act) out[a] = *total;
}
// rows [w_lo, w_lo + n) of the batch table as a batch of their own: segment ordinals and slots relative to the run
__global__ __launch_bounds__(256) void slice_kernel(const sg_window* __restrict__ all, uint64_t w_lo, uint64_t n, uint32_t a0, uint32_t slot_lo,
                                                    sg_window* __restrict__ out) {
  const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  sg_window o = all[w_lo + w];
  o.seg -= a0;
  o.slot_base -= slot_lo;
  out[w] = o;
}
// ------------------------------------------------------------------------------------------------
// launchers (declared in sg_windows.h)
// ------------------------------------------------------------------------------------------------
static inline uint32_t blocks256(uint64_t n) { return (uint32_t)((n + 255) / 256); }
void launch_gc(const uint8_t* chains, const uint64_t* chain_off, const sg_gc_window* wins, uint64_t n, int32_t* out, hipStream_t s) {
  if (n) hipLaunchKernelGGL(gc_kernel, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, s, chains, chain_off, wins, n, out);
}
void launch_weights(const uint8_t* chains, const uint64_t* chain_off, const WindowList& w, uint64_t n, const sg_gc_model& m, uint64_t seed,
                    double* out, hipStream_t s) {
  if (!n) return;
  launch_gc(chains, chain_off, w.win, n, w.gc, s);
  hipLaunchKernelGGL(gc_weight_kernel, dim3(blocks256(n)), dim3(256), 0, s, w.gc, w.win, w.seg_ord, w.win_ord, n, m.means, m.std, m.quantiles,
                     m.lg_cells, m.frag_size, m.full_tile_form, KIND_GC | (m.ctx24 << 8), (uint32_t)seed, (uint32_t)(seed >> 32), out);
}
void launch_tile(const BuildWork& b, uint64_t n, uint32_t frag, hipStream_t s) {
  if (n) hipLaunchKernelGGL(tile_kernel, dim3(blocks256(n)), dim3(256), 0, s, b.g.gens, b.g.prefix, b.g.n_gens, n, frag, b.seg_first, b.w.win,
                            b.w.seg_ord, b.w.win_ord);
}
void launch_seg_sum(const double* wt, const uint64_t* seg_first, uint32_t n_segs, double* out, hipStream_t s) {
  if (n_segs) hipLaunchKernelGGL(seg_sum_kernel, dim3(n_segs), dim3(256), 0, s, wt, seg_first, n_segs, out);
}
void launch_plan_rows(const PlanWork& p, uint64_t n, uint32_t frag, const double* wt, uint32_t n_act, sg_window* rows, int32_t paired,
                      hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(window_reads_kernel, dim3(blocks256(n)), dim3(256), 0, s, p.g.gens, p.g.prefix, p.g.n_gens, n, frag, wt, p.act, rows, p.seg_sum);
  hipLaunchKernelGGL(seg_remainder_kernel, dim3((n_act + 63) / 64), dim3(64), 0, s, p.act, p.seg_first, n_act, p.seg_sum, rows);
  hipLaunchKernelGGL(planned_kernel, dim3(blocks256(n)), dim3(256), 0, s, rows, n, paired, p.planned);
  launch_scan_u32(p.planned, (uint32_t)n, p.bsum, p.off, p.total, s);
  hipLaunchKernelGGL(slot_base_kernel, dim3(blocks256(n)), dim3(256), 0, s, rows, n, p.off);
  hipLaunchKernelGGL(seg_slots_kernel, dim3((n_act + 64) / 64), dim3(64), 0, s, p.off, p.seg_first, n_act, p.total, p.seg_slots);
}
void launch_slice(const sg_window* all, uint64_t w_lo, uint64_t n, uint32_t a0, uint32_t slot_lo, sg_window* out, hipStream_t s) {
  if (n) hipLaunchKernelGGL(slice_kernel, dim3(blocks256(n)), dim3(256), 0, s, all, w_lo, n, a0, slot_lo, out);
}

}  // namespace sg
