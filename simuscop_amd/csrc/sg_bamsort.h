// sg_bamsort.h -- coordinate order for the truth BAM (simuReads --truth-sort; kernels: sg_bamsort.hip, entry points:
// sg_api_bamsort.cpp).
//
// The order, stated once (DESIGN.md 10g quotes it):
//   key of a record = (refID as u32) << 32 | (POS as u32), taken from the record's own fields -- an unmapped read placed
//   at its mate sorts at its mate's place, an unplaced one (-1 / -1) has the largest key and sorts last;
//   ties keep the order of the unsorted file (pass order, then record order within the pass): a stable sort.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sg_truth.h"

namespace sg {

constexpr uint32_t kSortBlock = 256;                       // threads of a sort block
constexpr uint32_t kSortItems = 4;                         // keys per thread
constexpr uint32_t kSortTile = kSortBlock * kSortItems;    // keys per sort block (SG_BAMSORT_TILE of the ABI header)
constexpr uint32_t kSortDigits = 256;                      // 8-bit digits, least significant first

__host__ __device__ inline uint64_t bamsort_key(int32_t ref, int32_t pos) { return ((uint64_t)(uint32_t)ref << 32) | (uint64_t)(uint32_t)pos; }
inline uint32_t bamsort_blocks(uint32_t n) { return (n + kSortTile - 1) / kSortTile; }

// counters of the key kernel (u64 each): [1] OR of the keys, [2] AND of the keys (starts as ~0); the number of live
// records is the total of the scan of blk_count
// ---- keys of a pass: live records only, in record order ----
// blk_count[b] = live records among reads [256 b, 256 b + 256)
void launch_bamsort_count(const uint32_t* rec_len, uint32_t n_reads, uint32_t* blk_count, hipStream_t s);
// blk_off = exclusive scan of blk_count; (key, read index) of every live record at its rank
void launch_bamsort_keys(const TruthRow* rows, const uint32_t* rec_len, uint32_t n_reads, uint32_t paired, const uint64_t* blk_off, uint64_t* keys,
                         uint32_t* vals, unsigned long long* counters, hipStream_t s);
// vals[i] = i
void launch_bamsort_iota(uint32_t* vals, uint32_t n, hipStream_t s);
// ---- one digit pass of the stable LSD radix sort ----
// hist[d * n_blocks + b] = keys of sort block b whose digit at `shift` is d
void launch_bamsort_hist(const uint64_t* keys, uint32_t n, uint32_t shift, uint32_t* hist, hipStream_t s);
// hist_off = exclusive scan of hist: where the keys of (digit, block) start.  Stable within a block.
void launch_bamsort_scatter(const uint64_t* keys, const uint32_t* vals, uint32_t n, uint32_t shift, const uint64_t* hist_off, uint64_t* keys_out,
                            uint32_t* vals_out, hipStream_t s);
// ---- after the sort ----
// sorted_len[j] = len[vals[j]]
void launch_bamsort_lens(const uint32_t* len, const uint32_t* vals, uint32_t n, uint32_t* sorted_len, hipStream_t s);
// the offsets kernel: by_index[vals[j]] = sorted_off[j] (rec_off of the pack kernels)
void launch_bamsort_offsets(const uint64_t* sorted_off, const uint32_t* vals, uint32_t n, uint64_t* by_index, hipStream_t s);
// the gather kernel, one wave per output record j: sorted_len[j] bytes from src + src_off[vals[j]] to dst + dst_off[j].
// A record outside [0, src_bytes) or [0, dst_bytes) is not copied and sets bit 0 of *flags.  `src` is followed by 64
// readable bytes.
void launch_bamsort_gather(const uint8_t* src, uint64_t src_bytes, const uint64_t* src_off, const uint32_t* vals, const uint32_t* sorted_len,
                           const uint64_t* dst_off, uint32_t n, uint8_t* dst, uint64_t dst_bytes, unsigned long long* flags, hipStream_t s);

}  // namespace sg
