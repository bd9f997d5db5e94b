// sg_bamindex.hip -- the BAI index of the sorted truth BAM (simuReads --truth-index), gfx950.  The index: sg_bamindex.h.
//
//   bamindex_rows_kernel      lane = record: the fixed fields and the CIGAR from the record's bytes -> {refID, beg, end,
//                             bin, 0x4} and the start offset; the stem's linear index (64-bit atomicMin, the first
//                             window only where the lane in front is in another one) and per-reference counts (one
//                             set of atomics per block where the block holds one refID)
//   bamindex_heads_kernel / bamindex_compact_kernel   where (refID, bin) changes; after launch_scan_u32 the chunk
//                             rows at their ranks, the last one left open
//   bamindex_gather_kernel    the chunk rows in the order the sort of (key, chunk number) gave
#include "sg_bamindex.h"

namespace sg {
namespace {

// four bytes at any residue: the two aligned words around them (reaches at most 7 bytes past p: the buffer's padding)
__device__ __forceinline__ uint32_t load_u32(const uint8_t* p) {
  const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
  const uint32_t* a = (const uint32_t*)(p - sh);
  return __builtin_amdgcn_alignbyte(a[1], a[0], sh);
}

__device__ __forceinline__ uint64_t chunk_key(const BaiRow& r, uint32_t n_ref) {
  return r.ref < 0 ? (uint64_t)n_ref << 32 : ((uint64_t)(uint32_t)r.ref << 32) | (uint64_t)(r.bin_unmapped & 0x7FFFFFFFu);
}

__global__ __launch_bounds__(256) void bamindex_rows_kernel(const BaiJob J, BaiRow* __restrict__ rows, uint64_t* __restrict__ voff_out,
                                                            unsigned long long* __restrict__ linear, unsigned long long* __restrict__ counts,
                                                            unsigned long long* __restrict__ flags) {
  __shared__ int32_t s_ref0;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  const bool in = i < J.m;
  bool ok = false;
  int32_t ref = -1, beg = 0, end = 1;
  uint32_t unm = 0, bin = 0;
  uint64_t voff = 0;
  unsigned long long bad = 0;
  if (in) {
    const uint8_t* rec = nullptr;
    uint32_t len = 0;
    if (i < J.carried) {
      rec = J.carry;
      len = J.carry_len;
      voff = J.carry_voff;
    } else {
      const uint32_t j = i - J.carried;
      const uint64_t u = J.skip + J.off[j];
      len = J.len[j];
      if (len < 36u || u > J.bytes || len > J.bytes - u) bad = kBaiBadOffset;
      else {
        rec = J.text + u;
        voff = ((J.file_off + J.moff[u >> 15]) << 16) | (u & 32767u);
      }
    }
    if (!bad && len < 36u) bad = kBaiBadRecord;
    if (!bad) {
      const uint32_t block_size = load_u32(rec), w3 = load_u32(rec + 12), w4 = load_u32(rec + 16);
      ref = (int32_t)load_u32(rec + 4);
      beg = (int32_t)load_u32(rec + 8);
      const uint32_t l_name = w3 & 255u, n_cigar = w4 & 0xFFFFu;
      unm = (w4 >> 18) & 1u;
      if (block_size != len - 4u || 36u + l_name + 4u * n_cigar > len) bad = kBaiBadRecord;
      else {
        uint64_t ref_len = 0;
        const uint8_t* cig = rec + 36u + l_name;
        for (uint32_t k = 0; k < n_cigar; k++) {
          const uint32_t op = load_u32(cig + 4u * k);
          if ((0x18Du >> (op & 15u)) & 1u) ref_len += op >> 4;   // M D N = X
        }
        if (ref < 0) ref = -1;
        else {
          const uint64_t e = (uint64_t)(uint32_t)beg + ((unm || !ref_len) ? 1ull : ref_len);
          if ((uint32_t)ref >= J.n_ref || beg < 0 || e > kBaiMaxLen || e > J.refs[ref].len) bad = kBaiBadPlace;
          else {
            end = (int32_t)e;
            bin = truth_reg2bin((uint32_t)beg, (uint32_t)end);
          }
        }
      }
    }
    if (bad) {
      atomicOr(flags, bad);
      ref = -1;
    } else ok = true;
    BaiRow row;
    row.ref = ref;
    row.beg = beg;
    row.end = end;
    row.bin_unmapped = bin | (unm << 31);
    rows[i] = row;
    voff_out[i] = voff;
  }
  // linear index: the records come in file order, so within a wave a lane whose predecessor is in the same window of the
  // same reference has nothing to add to that window
  const bool co = ok && ref >= 0;
  const int32_t w0 = co ? beg >> kBaiShift : -1, w1 = co ? (end - 1) >> kBaiShift : -1;
  const int32_t p_ref = __shfl_up(co ? ref : -1, 1, 64), p_w0 = __shfl_up(w0, 1, 64);
  if (co) {
    unsigned long long* const lin = linear + J.refs[ref].win_first;
    if (lane == 0u || p_ref != ref || p_w0 != w0) atomicMin(&lin[w0], (unsigned long long)voff);
    for (int32_t w = w0 + 1; w <= w1; w++) atomicMin(&lin[w], (unsigned long long)voff);
  }
  // counts: one set of atomics for a block of one reference (thread 0 holds its smallest offset), per lane otherwise
  const int32_t my = ok ? ref : -2;
  if (threadIdx.x == 0u) s_ref0 = my;
  __syncthreads();
  const int32_t r0 = s_ref0;
  const int one = __syncthreads_and(!in || my == r0);
  const int n_map = __syncthreads_count(ok && !unm), n_unm = __syncthreads_count(ok && unm);
  if (one) {
    if (threadIdx.x == 0u && r0 >= 0) {
      if (n_map) atomicAdd(&counts[3u * r0], (unsigned long long)n_map);
      if (n_unm) atomicAdd(&counts[3u * r0 + 1u], (unsigned long long)n_unm);
      atomicMin(&counts[3u * r0 + 2u], (unsigned long long)voff);
    } else if (threadIdx.x == 0u && r0 == -1) atomicAdd(&counts[3u * J.n_ref], (unsigned long long)(n_map + n_unm));
  } else if (ok) {
    if (ref >= 0) {
      atomicAdd(&counts[3u * ref + unm], 1ull);
      atomicMin(&counts[3u * ref + 2u], (unsigned long long)voff);
    } else atomicAdd(&counts[3u * J.n_ref], 1ull);
  }
}

__global__ __launch_bounds__(256) void bamindex_heads_kernel(const BaiRow* __restrict__ rows, uint32_t m, uint32_t n_ref, uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= m) return;
  head[i] = (i == 0u || chunk_key(rows[i], n_ref) != chunk_key(rows[i - 1u], n_ref)) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void bamindex_compact_kernel(const BaiRow* __restrict__ rows, const uint64_t* __restrict__ voff,
                                                               const uint32_t* __restrict__ head, const uint64_t* __restrict__ rank,
                                                               const uint64_t* __restrict__ total, uint32_t m, uint32_t n_ref,
                                                               uint64_t* __restrict__ ckey, uint64_t* __restrict__ cbeg, uint64_t* __restrict__ cend,
                                                               uint32_t* __restrict__ pay, unsigned long long* __restrict__ no_coor) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= m || !head[i]) return;
  const uint64_t r = rank[i], v = voff[i];
  if (r >= m) return;
  const BaiRow row = rows[i];
  ckey[r] = chunk_key(row, n_ref);
  cbeg[r] = v;
  pay[r] = (uint32_t)r;
  if (r) cend[r - 1u] = v;
  if (r + 1u == *total) cend[r] = ~0ull;
  if (row.ref < 0) atomicAdd(no_coor, 1ull);
}

__global__ __launch_bounds__(256) void bamindex_gather_kernel(const uint64_t* __restrict__ key, const uint32_t* __restrict__ pay,
                                                              const uint64_t* __restrict__ cbeg, const uint64_t* __restrict__ cend, uint32_t n,
                                                              uint64_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const uint32_t c = pay[j];
  if (c >= n) return;
  out[3u * (size_t)j] = key[j];
  out[3u * (size_t)j + 1u] = cbeg[c];
  out[3u * (size_t)j + 2u] = cend[c];
}

__global__ __launch_bounds__(256) void bamindex_fill_kernel(unsigned long long* __restrict__ p, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) p[i] = ~0ull;
}

}  // namespace

void launch_bamindex_rows(const BaiJob& J, BaiRow* rows, uint64_t* voff, unsigned long long* linear, unsigned long long* counts,
                          unsigned long long* flags, hipStream_t s) {
  if (!J.m) return;
  hipLaunchKernelGGL(bamindex_rows_kernel, dim3((J.m + 255u) / 256u), dim3(256), 0, s, J, rows, voff, linear, counts, flags);
}
void launch_bamindex_heads(const BaiRow* rows, uint32_t m, uint32_t n_ref, uint32_t* head, hipStream_t s) {
  if (!m) return;
  hipLaunchKernelGGL(bamindex_heads_kernel, dim3((m + 255u) / 256u), dim3(256), 0, s, rows, m, n_ref, head);
}
void launch_bamindex_compact(const BaiRow* rows, const uint64_t* voff, const uint32_t* head, const uint64_t* rank, const uint64_t* total, uint32_t m,
                             uint32_t n_ref, uint64_t* ckey, uint64_t* cbeg, uint64_t* cend, uint32_t* pay, unsigned long long* no_coor, hipStream_t s) {
  if (!m) return;
  hipLaunchKernelGGL(bamindex_compact_kernel, dim3((m + 255u) / 256u), dim3(256), 0, s, rows, voff, head, rank, total, m, n_ref, ckey, cbeg, cend, pay,
                     no_coor);
}
void launch_bamindex_gather(const uint64_t* key, const uint32_t* pay, const uint64_t* cbeg, const uint64_t* cend, uint32_t n, uint64_t* out,
                            hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(bamindex_gather_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, key, pay, cbeg, cend, n, out);
}
void launch_bamindex_fill(unsigned long long* p, uint64_t n, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(bamindex_fill_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, s, p, n);
}

}  // namespace sg
