// sg_scan.hip -- exclusive scan of u32 values into u64 offsets, for every subsystem that turns lengths or counts into
// offsets (sg_scan.h).
#include "sg_scan.h"

namespace sg {

// ------------------------------------------------------------------------------------------------
// exclusive scan u32 -> u64 (three passes, 2048 items per block), one grid row per mate
// ------------------------------------------------------------------------------------------------
#define SCAN_ITEMS 8
#define SCAN_BLOCK 256
#define SCAN_TILE (SCAN_ITEMS * SCAN_BLOCK)

__device__ __forceinline__ uint64_t block_exclusive_scan(uint64_t v, uint64_t* total) {
  __shared__ uint64_t wsum[SCAN_BLOCK / 64];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint64_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint64_t t = __shfl_up(incl, d);
    if ((int)lane >= d) incl += t;
  }
  if (lane == 63) wsum[wid] = incl;
  __syncthreads();
  uint64_t woff = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < SCAN_BLOCK / 64; i++) {
    if (i < (int)wid) woff += wsum[i];
    tot += wsum[i];
  }
  __syncthreads();
  *total = tot;
  return woff + incl - v;
}

__global__ __launch_bounds__(SCAN_BLOCK) void scan_reduce_kernel(const uint32_t* __restrict__ in, uint32_t n,
                                                                uint64_t* __restrict__ bsum, uint32_t nblk) {
  const uint32_t m = blockIdx.y;
  const uint32_t* src = in + (size_t)m * n;
  const uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  uint64_t s = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++)
    if (base + i < n) s += src[base + i];
  uint64_t tot;
  block_exclusive_scan(s, &tot);
  if (threadIdx.x == 0) bsum[(size_t)m * nblk + blockIdx.x] = tot;
}

__global__ __launch_bounds__(1024) void scan_sums_kernel(uint64_t* __restrict__ bsum, uint32_t nblk,
                                                        uint64_t* __restrict__ totals) {
  // one block per row (mate): thread i owns a run of ceil(nblk / 1024) consecutive sums -- adds them up, the 1024 run
  // totals are scanned in LDS (one Hillis-Steele pass), then every thread writes the exclusive prefixes of its run
  __shared__ uint64_t buf[1024];
  const uint32_t m = blockIdx.x;
  uint64_t* b = bsum + (size_t)m * nblk;
  const uint32_t run = (nblk + 1023u) / 1024u;
  const uint32_t lo = threadIdx.x * run, hi = min(lo + run, nblk);
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
  if (threadIdx.x == 1023u) totals[m] = buf[1023];
}

__global__ __launch_bounds__(SCAN_BLOCK) void scan_apply_kernel(const uint32_t* __restrict__ in, uint32_t n,
                                                               const uint64_t* __restrict__ bsum, uint32_t nblk,
                                                               uint64_t* __restrict__ out) {
  const uint32_t m = blockIdx.y;
  const uint32_t* src = in + (size_t)m * n;
  uint64_t* dst = out + (size_t)m * n;
  const uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS];
  uint64_t s = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++) {
    v[i] = base + i < n ? src[base + i] : 0u;
    s += v[i];
  }
  uint64_t tot;
  uint64_t off = block_exclusive_scan(s, &tot) + bsum[(size_t)m * nblk + blockIdx.x];
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++) {
    if (base + i < n) dst[base + i] = off;
    off += v[i];
  }
}

uint32_t scan_blocks(uint32_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }
// exclusive scan of n u32 values into u64 offsets (one row); total -> *total
void launch_scan_u32(const uint32_t* in, uint32_t n, uint64_t* bsum, uint64_t* out, uint64_t* total, hipStream_t s) {
  if (!n) return;
  const uint32_t nblk = scan_blocks(n);
  hipLaunchKernelGGL(scan_reduce_kernel, dim3(nblk, 1), dim3(SCAN_BLOCK), 0, s, in, n, bsum, nblk);
  hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(1024), 0, s, bsum, nblk, total);
  hipLaunchKernelGGL(scan_apply_kernel, dim3(nblk, 1), dim3(SCAN_BLOCK), 0, s, in, n, bsum, nblk, out);
}

}  // namespace sg
