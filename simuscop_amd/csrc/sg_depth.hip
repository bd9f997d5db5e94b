// sg_depth.hip -- the reads' true coverage (simuReads --truth-depth), gfx950.
//
// Coverage adds up, so it needs no sort: every M run [a, b) of every read's true alignment (truth_walk, sg_truth.h) adds
// +1 at slot a and -1 at slot b of one int32 difference array over the reference (DepthJob), pass after pass.  At the end
// a prefix sum gives the depth.
//   depth_add_kernel     lane = read (index = slot * mates + mate, as truth_size_kernel): the walk, its M runs staged in
//                        LDS until the walk has told where the alignment starts, then two atomics per run;
//   depth_spans_kernel   lane = span: the same two atomics for spans the host gives (sg_depth_add_spans);
//   the finishing pass, per contig, wave = tile of kDepthTile bases, 16 bytes per lane and load:
//     depth_tiles_kernel   the tile's sum of differences and its number of run starts (launch_scan_u32 scans both);
//     depth_bins_kernel    the running depth rebuilt in registers (wave scan), its 64-bit prefix sums through the wave's
//                          LDS: the last base of every bin inside the wave's 256 bases adds the bin's part to the bin's
//                          sum, one atomic per bin and wave; no per-base depth is written;
//     depth_runs_kernel    the same depth; the run starts leave as (start, depth) rows compacted by the scanned counts;
//     depth_fetch_kernel   per-base depths of a range (tests, small regions).
#include "sg_truth.h"

namespace sg {
namespace {

constexpr uint32_t kStageRuns = kDepthStageRuns;
constexpr uint32_t kAddThreads = 256;

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// +1 at the run's first slot, -1 behind its last; a run outside its contig is reported, not written
__device__ __forceinline__ uint32_t add_run(const DepthJob& J, int64_t contig, int64_t start, uint64_t len) {
  if (!len) return 0u;
  if (contig < 0 || contig >= (int64_t)J.n_contigs || start < 0 || (uint64_t)start > J.contig_len[contig] ||
      len > J.contig_len[contig] - (uint64_t)start)
    return 1u;
  int32_t* const d = J.diff + J.contig_off[contig] + (uint64_t)start;
  atomicAdd(d, 1);
  atomicAdd(d + len, -1);
  return 0u;
}

__device__ __forceinline__ void count_and_flag(const DepthJob& J, uint64_t bases, uint32_t flags) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) bases += __shfl_xor((unsigned long long)bases, d, 64);
  if ((threadIdx.x & 63u) == 0u && bases) atomicAdd(&J.counters[0], (unsigned long long)bases);
  if (flags) atomicOr(&J.counters[1], (unsigned long long)flags);
}

__global__ __launch_bounds__(kAddThreads) void depth_add_kernel(DevProfile P, DevBatch B, DepthJob J) {
  __shared__ uint32_t st_rel[kStageRuns * kAddThreads], st_len[kStageRuns * kAddThreads];   // [run][lane]: no bank conflict
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  const PassRead R = pass_read(B, idx, J.map.n_reads);
  ReadGeom g = {};
  if (R.in_range) g = read_geom(P, B, R.t, R.m);
  uint64_t bases = 0;
  uint32_t flags = 0;
  if (g.live && g.inside && g.chain < J.map.n_chains) {
    const uint64_t last = J.map.chain_first[g.chain + 1];
    const uint64_t pi = truth_find_piece(J.map.pieces, J.map.chain_first[g.chain], last, g.tmpl_off);
    // `put` is told lengths, not positions, and the alignment's start only comes back with the walk: the M runs are kept
    // as offsets from that start (M, D and N move along the reference).  What the end of the walk withdraws is never M.
    uint32_t n_runs = 0, rel = 0, m_end = 0;
    const uint32_t tid = threadIdx.x;
    const TruthAln A = truth_walk(J.map.pieces, last, pi, g.tmpl_off, (uint32_t)P.L, g.reverse != 0u, g.events, g.nev, [&](uint32_t, uint32_t v) {
      const uint32_t op = v & 15u, len = v >> 4;
      if (op == kOpM) {
        if (n_runs < J.stage_runs) { st_rel[n_runs * kAddThreads + tid] = rel; st_len[n_runs * kAddThreads + tid] = len; }
        n_runs++;
        rel += len;
        m_end = rel;
      } else if (op == kOpD || op == kOpN) {
        rel += len;
      }
    });
    if (A.n_ops) {
      if (A.pos0 + (int64_t)m_end != A.end) flags |= 2u;
      if (n_runs <= J.stage_runs) {
        for (uint32_t r = 0; r < n_runs; r++) {
          const uint32_t len = st_len[r * kAddThreads + tid];
          const uint32_t f = add_run(J, A.contig, A.pos0 + st_rel[r * kAddThreads + tid], len);
          flags |= f;
          if (!f) bases += len;
        }
      } else {   // more runs than the stage holds: the walk again, now that its start is known
        uint32_t rel2 = 0;
        truth_walk(J.map.pieces, last, pi, g.tmpl_off, (uint32_t)P.L, g.reverse != 0u, g.events, g.nev, [&](uint32_t, uint32_t v) {
          const uint32_t op = v & 15u, len = v >> 4;
          if (op == kOpM) {
            const uint32_t f = add_run(J, A.contig, A.pos0 + rel2, len);
            flags |= f;
            if (!f) bases += len;
            rel2 += len;
          } else if (op == kOpD || op == kOpN) {
            rel2 += len;
          }
        });
      }
    }
  }
  count_and_flag(J, bases, flags);
}

__global__ __launch_bounds__(256) void depth_spans_kernel(DepthJob J, const uint32_t* __restrict__ contig, const uint64_t* __restrict__ start,
                                                          const uint64_t* __restrict__ end, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t bases = 0;
  uint32_t flags = 0;
  if (i < n) {
    const uint64_t a = start[i], b = end[i];
    if (b < a || a > 0x7FFFFFFFFFFFFFFFull) flags = 1u;
    else {
      flags = add_run(J, contig[i], (int64_t)a, b - a);
      if (!flags) bases = b - a;
    }
  }
  count_and_flag(J, bases, flags);
}

// ---- the finishing pass ----
// Step k of a tile: lane l holds the four differences of bases e .. e + 3, e = tile * kDepthTile + k * 256 + l * 4; what lies
// behind the contig's last base reads as 0.  (A contig's slots end at a multiple of 4 behind slot len: the load stays inside.)
constexpr uint32_t kTileSteps = kDepthTile / 256u;

__device__ __forceinline__ uint4 load_diffs(const DepthView& V, uint32_t e) {
  uint4 x = make_uint4(0u, 0u, 0u, 0u);
  if (e < V.len) {
    x = *(const uint4*)(V.diff + e);
    const uint32_t left = V.len - e;
    if (left < 4u) { x.w = 0u; if (left < 3u) x.z = 0u; if (left < 2u) x.y = 0u; }
  }
  return x;
}
__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t v, uint32_t lane) {   // inclusive
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(v, d, 64);
    if ((int)lane >= d) v += up;
  }
  return v;
}
__device__ __forceinline__ unsigned long long wave_scan_u64(unsigned long long v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long up = __shfl_up(v, d, 64);
    if ((int)lane >= d) v += up;
  }
  return v;
}
// the four depths of a lane's bases from their differences; `carry` (the depth in front of the step) moves on
__device__ __forceinline__ uint4 step_depths(const uint4 x, uint32_t lane, uint32_t& carry) {
  const uint32_t p0 = x.x, p1 = p0 + x.y, p2 = p1 + x.z, p3 = p2 + x.w;
  const uint32_t incl = wave_scan_u32(p3, lane);
  const uint32_t base = carry + incl - p3;
  carry += __shfl(incl, 63, 64);
  return make_uint4(base + p0, base + p1, base + p2, base + p3);
}

__global__ __launch_bounds__(64) void depth_tiles_kernel(DepthView V, uint32_t* __restrict__ tile_sum, uint32_t* __restrict__ tile_starts) {
  const uint32_t lane = threadIdx.x, tile = blockIdx.x;
  uint32_t sum = 0, starts = 0;
#pragma unroll
  for (uint32_t k = 0; k < kTileSteps; k++) {
    const uint32_t e = tile * kDepthTile + k * 256u + lane * 4u;
    const uint4 x = load_diffs(V, e);
    sum += x.x + x.y + x.z + x.w;
    starts += (x.x != 0u || (e == 0u && V.len != 0u) ? 1u : 0u) + (x.y != 0u ? 1u : 0u) + (x.z != 0u ? 1u : 0u) + (x.w != 0u ? 1u : 0u);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    sum += __shfl_xor(sum, d, 64);
    starts += __shfl_xor(starts, d, 64);
  }
  if (lane == 0u) {
    tile_sum[tile] = sum;
    tile_starts[tile] = starts;
  }
}

__global__ __launch_bounds__(64) void depth_bins_kernel(DepthView V, const uint64_t* __restrict__ tile_base, uint32_t bin,
                                                        unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long pre[256];   // prefix sums of the step's 256 depths
  const uint32_t lane = threadIdx.x, tile = blockIdx.x;
  uint32_t carry = (uint32_t)tile_base[tile];
  for (uint32_t k = 0; k < kTileSteps; k++) {
    const uint32_t e = tile * kDepthTile + k * 256u + lane * 4u;
    if (tile * kDepthTile + k * 256u >= V.len) break;   // (the whole wave)
    const uint4 x = load_diffs(V, e);
    const uint4 d = step_depths(x, lane, carry);
    const uint32_t dv[4] = {d.x, d.y, d.z, d.w};
    unsigned long long q[4];
    unsigned long long acc = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (e + (uint32_t)j < V.len) acc += dv[j];
      q[j] = acc;
    }
    const unsigned long long excl = wave_scan_u64(acc, lane) - acc;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      q[j] += excl;
      pre[lane * 4u + (uint32_t)j] = q[j];
    }
    wave_lds_sync();
    if (e < V.len) {
      uint32_t b = e / bin, r = e - b * bin;   // bin of the lane's first base and the base's place in it
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t pos = e + (uint32_t)j, i = lane * 4u + (uint32_t)j;
        if (pos < V.len && (r == bin - 1u || pos == V.len - 1u || i == 255u)) {
          const uint32_t i0 = i > r ? i - r : 0u;   // where the bin begins inside this step
          atomicAdd(&sums[b], q[j] - (i0 ? pre[i0 - 1u] : 0ull));
        }
        if (++r == bin) { r = 0u; b++; }
      }
    }
    wave_lds_sync();
  }
}

__global__ __launch_bounds__(64) void depth_runs_kernel(DepthView V, const uint64_t* __restrict__ tile_base, const uint64_t* __restrict__ start_base,
                                                        DepthRun* __restrict__ rows, uint64_t cap) {
  const uint32_t lane = threadIdx.x, tile = blockIdx.x;
  uint32_t carry = (uint32_t)tile_base[tile];
  uint64_t at = start_base[tile];
  for (uint32_t k = 0; k < kTileSteps; k++) {
    const uint32_t e = tile * kDepthTile + k * 256u + lane * 4u;
    if (tile * kDepthTile + k * 256u >= V.len) break;
    const uint4 x = load_diffs(V, e);
    const uint4 d = step_depths(x, lane, carry);
    const uint32_t xv[4] = {x.x, x.y, x.z, x.w}, dv[4] = {d.x, d.y, d.z, d.w};
    bool is_start[4];
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t pos = e + (uint32_t)j;
      is_start[j] = pos < V.len && (pos == 0u || xv[j] != 0u);
      mine += is_start[j] ? 1u : 0u;
    }
    const uint32_t incl = wave_scan_u32(mine, lane);
    uint64_t w = at + (incl - mine);
    at += __shfl(incl, 63, 64);
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (is_start[j]) {
        if (w < cap) rows[w] = DepthRun{e + (uint32_t)j, dv[j]};
        w++;
      }
  }
}

__global__ __launch_bounds__(64) void depth_fetch_kernel(DepthView V, const uint64_t* __restrict__ tile_base, uint32_t first, uint32_t n,
                                                         uint32_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x, tile = first / kDepthTile + blockIdx.x;
  uint32_t carry = (uint32_t)tile_base[tile];
  for (uint32_t k = 0; k < kTileSteps; k++) {
    const uint32_t e = tile * kDepthTile + k * 256u + lane * 4u;
    if (tile * kDepthTile + k * 256u >= V.len) break;
    const uint4 x = load_diffs(V, e);
    const uint4 d = step_depths(x, lane, carry);
    const uint32_t dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t pos = e + (uint32_t)j;
      if (pos < V.len && pos >= first && pos - first < n) out[pos - first] = dv[j];
    }
  }
}

}  // namespace

void launch_depth_add(const DevProfile& P, const DevBatch& B, const DepthJob& J, hipStream_t s) {
  if (!J.map.n_reads) return;
  hipLaunchKernelGGL(depth_add_kernel, dim3((J.map.n_reads + kAddThreads - 1u) / kAddThreads), dim3(kAddThreads), 0, s, P, B, J);
}
void launch_depth_spans(const DepthJob& J, const uint32_t* contig, const uint64_t* start, const uint64_t* end, uint64_t n, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(depth_spans_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, s, J, contig, start, end, n);
}
void launch_depth_tiles(const DepthView& V, uint32_t* tile_sum, uint32_t* tile_starts, hipStream_t s) {
  if (!V.n_tiles) return;
  hipLaunchKernelGGL(depth_tiles_kernel, dim3(V.n_tiles), dim3(64), 0, s, V, tile_sum, tile_starts);
}
void launch_depth_bins(const DepthView& V, const uint64_t* tile_base, uint32_t bin, unsigned long long* sums, hipStream_t s) {
  if (!V.n_tiles) return;
  hipLaunchKernelGGL(depth_bins_kernel, dim3(V.n_tiles), dim3(64), 0, s, V, tile_base, bin, sums);
}
void launch_depth_runs(const DepthView& V, const uint64_t* tile_base, const uint64_t* start_base, DepthRun* rows, uint64_t cap, hipStream_t s) {
  if (!V.n_tiles) return;
  hipLaunchKernelGGL(depth_runs_kernel, dim3(V.n_tiles), dim3(64), 0, s, V, tile_base, start_base, rows, cap);
}
void launch_depth_fetch(const DepthView& V, const uint64_t* tile_base, uint32_t first, uint32_t n, uint32_t* out, hipStream_t s) {
  if (!n || !V.n_tiles) return;
  const uint32_t t0 = first / kDepthTile, t1 = (first + n - 1u) / kDepthTile;
  hipLaunchKernelGGL(depth_fetch_kernel, dim3(t1 - t0 + 1u), dim3(64), 0, s, V, tile_base, first, n, out);
}

}  // namespace sg
