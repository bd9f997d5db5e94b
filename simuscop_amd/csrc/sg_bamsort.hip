// sg_bamsort.hip -- the truth BAM in coordinate order (simuReads --truth-sort), gfx950.  The order: sg_bamsort.h.
//
//   bamsort_count_kernel / bamsort_key_kernel   a pass's (key, read index) pairs, live records only, in record order: the
//                       key is the refID / POS the pack kernel will write (the mate's row for an unmapped read)
//   bamsort_hist_kernel / bamsort_scatter_kernel   one digit of a stable LSD radix sort of (u64 key, u32 payload): per-block
//                       digit histograms in LDS, scanned digit-major by launch_scan_u32, then a scatter whose ranks
//                       within a block follow the keys' order in it
//   bamsort_lens_kernel / bamsort_offsets_kernel   the lengths in sorted order, and their scan handed back by read index:
//                       rec_off of the pack kernels, which so write a sorted stream unchanged
//   bamsort_gather_kernel   the merge: one wave per record, 16 bytes per lane through registers
#include "sg_bamsort.h"

namespace sg {
namespace {

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void bamsort_count_kernel(const uint32_t* __restrict__ rec_len, uint32_t n, uint32_t* __restrict__ blk_count) {
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  const int live = idx < n && rec_len[idx] != 0u;
  const int c = __syncthreads_count(live);
  if (threadIdx.x == 0u) blk_count[blockIdx.x] = (uint32_t)c;
}

__global__ __launch_bounds__(256) void bamsort_key_kernel(const TruthRow* __restrict__ rows, const uint32_t* __restrict__ rec_len, uint32_t n,
                                                          uint32_t paired, const uint64_t* __restrict__ blk_off, uint64_t* __restrict__ keys,
                                                          uint32_t* __restrict__ vals, unsigned long long* counters) {
  __shared__ uint32_t wave_live[4];
  __shared__ uint64_t wave_or[4], wave_and[4];
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const bool live = idx < n && rec_len[idx] != 0u;
  uint64_t key = 0;
  if (live) {
    const TruthRow row = rows[idx];
    int32_t ref = row.contig, pos = row.pos;
    if (row.n_ops == 0u) {   // unmapped: at its mate's place, as truth_pack_kernel puts it
      TruthRow mate = {-1, -1, -1, 0u};
      if (paired && (idx ^ 1u) < n && rec_len[idx ^ 1u] != 0u) mate = rows[idx ^ 1u];
      const bool mate_mapped = mate.n_ops != 0u;
      ref = mate_mapped ? mate.contig : -1;
      pos = mate_mapped ? mate.pos : -1;
    }
    key = bamsort_key(ref, pos);
  }
  const unsigned long long lm = __ballot(live);
  uint64_t k_or = live ? key : 0ull, k_and = live ? key : ~0ull;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    k_or |= __shfl_xor(k_or, d, 64);
    k_and &= __shfl_xor(k_and, d, 64);
  }
  if (lane == 0u) {
    wave_live[wid] = (uint32_t)__popcll(lm);
    wave_or[wid] = k_or;
    wave_and[wid] = k_and;
  }
  __syncthreads();
  if (threadIdx.x == 0u) {   // one pair of atomics a block, and none when the block has no bit to add or to take
    const uint64_t b_or = wave_or[0] | wave_or[1] | wave_or[2] | wave_or[3], b_and = wave_and[0] & wave_and[1] & wave_and[2] & wave_and[3];
    if (b_or & ~__atomic_load_n(&counters[1], __ATOMIC_RELAXED)) atomicOr(&counters[1], (unsigned long long)b_or);
    if (~b_and & __atomic_load_n(&counters[2], __ATOMIC_RELAXED)) atomicAnd(&counters[2], (unsigned long long)b_and);
  }
  if (!live) return;
  uint64_t at = blk_off[blockIdx.x] + (uint64_t)__popcll(lm & ((1ull << lane) - 1ull));
  for (uint32_t w = 0; w < wid; w++) at += wave_live[w];
  keys[at] = key;
  vals[at] = idx;
}

__global__ __launch_bounds__(256) void bamsort_iota_kernel(uint32_t* __restrict__ vals, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) vals[i] = i;
}

// A sort block's keys: wave w owns [256 w, 256 w + 256) of the tile, lane l takes 64 i + l of them in round i.
__device__ __forceinline__ uint32_t tile_index(uint32_t i) { return blockIdx.x * kSortTile + (threadIdx.x >> 6) * 256u + i * 64u + (threadIdx.x & 63u); }

__global__ __launch_bounds__(kSortBlock) void bamsort_hist_kernel(const uint64_t* __restrict__ keys, uint32_t n, uint32_t shift,
                                                                  uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[kSortDigits];
  h[threadIdx.x] = 0u;
  __syncthreads();
#pragma unroll
  for (uint32_t i = 0; i < kSortItems; i++) {
    const uint32_t e = tile_index(i);
    if (e < n) atomicAdd(&h[(uint32_t)(keys[e] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(kSortBlock) void bamsort_scatter_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t n,
                                                                     uint32_t shift, const uint64_t* __restrict__ hist_off,
                                                                     uint64_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out) {
  __shared__ uint32_t cnt[kSortBlock / 64][kSortDigits];   // per wave: keys of each digit so far, then where its first one goes
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t w = 0; w < kSortBlock / 64; w++) cnt[w][threadIdx.x] = 0u;
  __syncthreads();
  uint64_t k[kSortItems];
  uint32_t v[kSortItems], dig[kSortItems], rank[kSortItems];
  bool valid[kSortItems];
#pragma unroll
  for (uint32_t i = 0; i < kSortItems; i++) {
    const uint32_t e = tile_index(i);
    valid[i] = e < n;
    k[i] = valid[i] ? keys[e] : 0ull;
    v[i] = valid[i] ? vals[e] : 0u;
    dig[i] = (uint32_t)(k[i] >> shift) & 255u;
    // the lanes of this round with my digit; my rank among them is the number in front of me
    unsigned long long peers = __ballot(valid[i]);
#pragma unroll
    for (uint32_t b = 0; b < 8u; b++) {
      const bool bit = (dig[i] >> b) & 1u;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const uint32_t ahead = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
    const uint32_t before = cnt[wid][dig[i]];
    wave_lds_sync();
    if (valid[i] && ahead == 0u) cnt[wid][dig[i]] = before + (uint32_t)__popcll(peers);
    wave_lds_sync();
    rank[i] = before + ahead;
  }
  __syncthreads();
  {   // thread = digit: the block's keys of this digit start at hist_off, wave after wave
    uint32_t at = (uint32_t)hist_off[(size_t)threadIdx.x * gridDim.x + blockIdx.x];   // (fewer than 2^32 keys)
#pragma unroll
    for (uint32_t w = 0; w < kSortBlock / 64; w++) {
      const uint32_t c = cnt[w][threadIdx.x];
      cnt[w][threadIdx.x] = at;
      at += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t i = 0; i < kSortItems; i++) {
    if (!valid[i]) continue;
    const uint32_t p = cnt[wid][dig[i]] + rank[i];
    if (p < n) {
      keys_out[p] = k[i];
      vals_out[p] = v[i];
    }
  }
}

__global__ __launch_bounds__(256) void bamsort_lens_kernel(const uint32_t* __restrict__ len, const uint32_t* __restrict__ vals, uint32_t n,
                                                           uint32_t* __restrict__ sorted_len) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j < n) sorted_len[j] = len[vals[j]];
}

__global__ __launch_bounds__(256) void bamsort_offsets_kernel(const uint64_t* __restrict__ sorted_off, const uint32_t* __restrict__ vals, uint32_t n,
                                                              uint64_t* __restrict__ by_index) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j < n) by_index[vals[j]] = sorted_off[j];
}

// One wave per record.  The destination decides the pieces: up to 15 single bytes to its first 16-byte boundary, whole
// 16-byte pieces, up to 15 single bytes behind them.  A piece's source has any residue: the two aligned 16-byte loads
// around it, shifted together in registers (the residue is the same for the whole wave).
__global__ __launch_bounds__(256) void bamsort_gather_kernel(const uint8_t* __restrict__ src, uint64_t src_bytes, const uint64_t* __restrict__ src_off,
                                                             const uint32_t* __restrict__ vals, const uint32_t* __restrict__ sorted_len,
                                                             const uint64_t* __restrict__ dst_off, uint32_t n, uint8_t* __restrict__ dst,
                                                             uint64_t dst_bytes, unsigned long long* flags) {
  const uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (j >= n) return;
  const uint32_t len = sorted_len[j];
  const uint64_t so = src_off[vals[j]], d_o = dst_off[j];
  if (so > src_bytes || len > src_bytes - so || d_o > dst_bytes || len > dst_bytes - d_o) {
    if (lane == 0u) atomicOr(flags, 1ull);
    return;
  }
  const uint8_t* const sp = src + so;
  uint8_t* const dp = dst + d_o;
  const uint32_t head = min((uint32_t)((16u - (uint32_t)((uintptr_t)dp & 15u)) & 15u), len);
  const uint32_t n16 = (len - head) >> 4, tail_at = head + n16 * 16u;
  if (lane < head) dp[lane] = sp[lane];
  if (lane >= 32u && tail_at + (lane - 32u) < len && lane - 32u < 16u) dp[tail_at + (lane - 32u)] = sp[tail_at + (lane - 32u)];
  const uint8_t* const body = sp + head;
  const uint32_t sh = (uint32_t)((uintptr_t)body & 15u), ws = sh >> 2, bs = sh & 3u;
  const uint4* const a16 = (const uint4*)(body - sh);
  uint4* const d16 = (uint4*)(dp + head);
  for (uint32_t q = lane; q < n16; q += 64u) {
    const uint4 A = a16[q], B = a16[q + 1u];   // (B reaches at most 31 bytes past the record: src's padding)
    const uint32_t w0 = A.x, w1 = A.y, w2 = A.z, w3 = A.w, w4 = B.x, w5 = B.y, w6 = B.z, w7 = B.w;
    const uint32_t c0 = ws == 0u ? w0 : ws == 1u ? w1 : ws == 2u ? w2 : w3;
    const uint32_t c1 = ws == 0u ? w1 : ws == 1u ? w2 : ws == 2u ? w3 : w4;
    const uint32_t c2 = ws == 0u ? w2 : ws == 1u ? w3 : ws == 2u ? w4 : w5;
    const uint32_t c3 = ws == 0u ? w3 : ws == 1u ? w4 : ws == 2u ? w5 : w6;
    const uint32_t c4 = ws == 0u ? w4 : ws == 1u ? w5 : ws == 2u ? w6 : w7;
    uint4 o;
    o.x = __builtin_amdgcn_alignbyte(c1, c0, bs);
    o.y = __builtin_amdgcn_alignbyte(c2, c1, bs);
    o.z = __builtin_amdgcn_alignbyte(c3, c2, bs);
    o.w = __builtin_amdgcn_alignbyte(c4, c3, bs);
    d16[q] = o;
  }
}

}  // namespace

void launch_bamsort_count(const uint32_t* rec_len, uint32_t n_reads, uint32_t* blk_count, hipStream_t s) {
  if (!n_reads) return;
  hipLaunchKernelGGL(bamsort_count_kernel, dim3((n_reads + 255u) / 256u), dim3(256), 0, s, rec_len, n_reads, blk_count);
}
void launch_bamsort_keys(const TruthRow* rows, const uint32_t* rec_len, uint32_t n_reads, uint32_t paired, const uint64_t* blk_off, uint64_t* keys,
                         uint32_t* vals, unsigned long long* counters, hipStream_t s) {
  if (!n_reads) return;
  hipLaunchKernelGGL(bamsort_key_kernel, dim3((n_reads + 255u) / 256u), dim3(256), 0, s, rows, rec_len, n_reads, paired, blk_off, keys, vals, counters);
}
void launch_bamsort_iota(uint32_t* vals, uint32_t n, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(bamsort_iota_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, vals, n);
}
void launch_bamsort_hist(const uint64_t* keys, uint32_t n, uint32_t shift, uint32_t* hist, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(bamsort_hist_kernel, dim3(bamsort_blocks(n)), dim3(kSortBlock), 0, s, keys, n, shift, hist);
}
void launch_bamsort_scatter(const uint64_t* keys, const uint32_t* vals, uint32_t n, uint32_t shift, const uint64_t* hist_off, uint64_t* keys_out,
                            uint32_t* vals_out, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(bamsort_scatter_kernel, dim3(bamsort_blocks(n)), dim3(kSortBlock), 0, s, keys, vals, n, shift, hist_off, keys_out, vals_out);
}
void launch_bamsort_lens(const uint32_t* len, const uint32_t* vals, uint32_t n, uint32_t* sorted_len, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(bamsort_lens_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, len, vals, n, sorted_len);
}
void launch_bamsort_offsets(const uint64_t* sorted_off, const uint32_t* vals, uint32_t n, uint64_t* by_index, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(bamsort_offsets_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, sorted_off, vals, n, by_index);
}
void launch_bamsort_gather(const uint8_t* src, uint64_t src_bytes, const uint64_t* src_off, const uint32_t* vals, const uint32_t* sorted_len,
                           const uint64_t* dst_off, uint32_t n, uint8_t* dst, uint64_t dst_bytes, unsigned long long* flags, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(bamsort_gather_kernel, dim3((n + 3u) / 4u), dim3(256), 0, s, src, src_bytes, src_off, vals, sorted_len, dst_off, n, dst, dst_bytes,
                     flags);
}

}  // namespace sg
