// The block rule of the project's fp8 format, on registers: OCP e4m3fn codes under one power-of-two scale per
// block.  What a block is belongs to the including code: 32 elements of a window on the K7 fp8 wire
// (csrc/probe/peer_q8.h, where the format is described in full), one 128-element K or V row of the fp8 paged KV
// cache (csrc/ops/attention_decode_paged_fp8.hip).  Both take e from the block's amax by q8_block_exp, scale by
// the exact 2^-e and convert with v_cvt_pk_fp8_f32, so one rule gives both their codes.
//
// Device code only and free of torch: csrc/probe includes it too.
#pragma once
#include <hip/hip_runtime.h>

namespace gtk_q8 {

constexpr int kQ8ExpMin = -100, kQ8ExpMax = 120;
constexpr int kQ8Bias = 127;                    // the stored byte is e + 127

__device__ __forceinline__ float q8_pow2(int n) { return __uint_as_float((unsigned int)(n + 127) << 23); }

// amax = m * 2^E with m in [1, 2): e = E - 8 when m <= 1.75 (448 = 1.75 * 2^8), else E - 7.  A zero or
// subnormal amax lands below the clamp, an infinite one above it.
__device__ __forceinline__ int q8_block_exp(float amax) {
  const unsigned int a = __float_as_uint(amax);
  const int e = (int)(a >> 23) - 127 - 8 + (int)((a & 0x7fffffu) > 0x600000u);
  return min(max(e, kQ8ExpMin), kQ8ExpMax);
}

// Two scaled values to two codes, the first in the low byte.
__device__ __forceinline__ unsigned int q8_codes2(float a, float b) {
  return (unsigned int)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xffffu;
}

}  // namespace gtk_q8
