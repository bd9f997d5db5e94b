// sg_philox.h -- the counter-based generator of every device draw (device code only: sg_pass_front.hip, sg_kernels.hip, sg_emit_fast.hip, sg_windows.hip).
// The stream kinds and kBaseRounds are in sg_device.h.
#pragma once
#include "sg_device.h"

namespace sg {

// ------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11), one call = four 32-bit draws
// ------------------------------------------------------------------------------------------------
template <int ROUNDS>
__device__ __forceinline__ void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                           uint32_t k0, uint32_t k1, uint32_t out[4]) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
  for (int r = 0; r < ROUNDS; r++) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;  // one v_mad_u64_u32 each
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c0 = __builtin_amdgcn_bitop3_b32(hi1, c1, k0, 0x96);  // three-input xor in one v_bitop3_b32
    c1 = lo1;
    c2 = __builtin_amdgcn_bitop3_b32(hi0, c3, k1, 0x96);
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
  philox4x32<10>(c0, c1, c2, c3, k0, k1, out);
}
// the per-base draws (KIND_BASE): kBaseRounds rounds (sg_device.h)
__device__ __forceinline__ void philox_base(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
  philox4x32<kBaseRounds>(c0, c1, c2, c3, k0, k1, out);
}

__device__ __forceinline__ uint32_t dev_ctx(uint32_t kind, uint32_t mate, uint32_t batch) {
  return kind | ((((mate & 1u) << 23) | (batch & 0xFFFFu)) << 8);
}

}  // namespace sg
