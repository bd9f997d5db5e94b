// sg_scan.h -- the general exclusive scan (sg_scan.hip): u32 values in, u64 offsets out, three kernels on one stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sg {

// blocks of the scan over n values: `bsum` of launch_scan_u32 holds one u64 each
uint32_t scan_blocks(uint32_t n);
// exclusive scan of n u32 values into u64 offsets (one row); total -> *total
void launch_scan_u32(const uint32_t* in, uint32_t n, uint64_t* bsum, uint64_t* out, uint64_t* total, hipStream_t s);

}  // namespace sg
