// What the kernels over the fp8 paged KV cache share (gfx950): the exact widening of e4m3 codes to bf16, the
// power-of-two scale of an exponent byte, and the row quantiser of the appends.  The cache format is described at the
// head of attention_decode_paged_fp8.hip; its rule on registers is csrc/common/q8_block.h.  Included by
// attention_decode_paged_fp8.hip (decode, the append of up to 32 rows) and attention_prefill_paged_fp8.hip (prefill,
// the append of a ragged chunk).
#pragma once
#include "../common/q8_block.h"
#include "attention_decode_body.h"

namespace gtk_decode {

typedef unsigned char u8;
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// 8 codes (two dwords, element j in byte j) to their 8 fp32 values, exactly
__device__ __forceinline__ void cvt8(uint32_t a, uint32_t b, float (&f)[8]) {
  const f32x2 a0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a, false), a1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)a, true);
  const f32x2 b0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b, false), b1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)b, true);
  f[0] = a0[0], f[1] = a0[1], f[2] = a1[0], f[3] = a1[1], f[4] = b0[0], f[5] = b0[1], f[6] = b1[0], f[7] = b1[1];
}

// the high halves of 8 fp32 as 8 bf16: truncation, exact where the values have at most 8 significant bits
__device__ __forceinline__ bf16x8 pack_hi8(const float (&f)[8]) {
  u32x4 u;
#pragma unroll
  for (int d = 0; d < 4; ++d) u[d] = (__float_as_uint(f[2 * d]) >> 16) | (__float_as_uint(f[2 * d + 1]) & 0xffff0000u);
  return __builtin_bit_cast(bf16x8, u);
}

// 8 codes to the 8 bf16 of an MFMA operand, exactly
__device__ __forceinline__ bf16x8 widen8(uint32_t a, uint32_t b) {
  float f[8];
  cvt8(a, b, f);
  return pack_hi8(f);
}

// 2^e of byte b of an exponent dword
__device__ __forceinline__ float exp_scale(uint32_t w, int b) { return __uint_as_float(((w >> (8 * b)) & 0xffu) << 23); }

// one lane's 8 elements of a row held by 16 lanes: the row's exponent, and the lane's 8 codes
__device__ __forceinline__ u32x2 quantize_row8(const uint4& x, int& e) {
  using namespace gtk_q8;
  const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
  float f[8];
#pragma unroll
  for (int d = 0; d < 4; ++d) f[2 * d] = __uint_as_float(xs[d] << 16), f[2 * d + 1] = __uint_as_float(xs[d] & 0xffff0000u);
  float amax = 0.f;  // over the elements that are not NaN: fmaxf drops a quieted one
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) amax = fmaxf(amax, fabsf(__builtin_canonicalizef(f[jj])));
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) amax = fmaxf(amax, __shfl_xor(amax, d));
  e = q8_block_exp(amax);
  const float down = q8_pow2(-e);
  u32x2 cw;
  cw[0] = q8_codes2(f[0] * down, f[1] * down) | (q8_codes2(f[2] * down, f[3] * down) << 16);
  cw[1] = q8_codes2(f[4] * down, f[5] * down) | (q8_codes2(f[6] * down, f[7] * down) << 16);
  return cw;
}

}  // namespace gtk_decode
