// What every source of the _fused module starts from: bf16 values travel as raw 16-bit words (u16),
// eight to a 16-B vector; the math is fp32.  Each source pulls these names into its own namespace
// with `using namespace gtk;`.
#pragma once

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <cstdint>

namespace gtk {

typedef unsigned short u16;
typedef u16 u16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf2f(u16 v) { return __uint_as_float((uint32_t)v << 16); }
__device__ __forceinline__ u16 f2bf(float f) { return __builtin_bit_cast(u16, (__bf16)f); }

// all 64 lanes of a wave get the sum / the maximum of their values
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

inline hipStream_t cur_stream() { return at::hip::getCurrentHIPStream().stream(); }
inline const u16* bp(const at::Tensor& t) { return reinterpret_cast<const u16*>(t.data_ptr()); }
inline u16* bpm(at::Tensor& t) { return reinterpret_cast<u16*>(t.data_ptr()); }

// blocks of `per_block` threads for `work` items, grid-stride beyond 16 blocks per CU (256 CUs)
inline int grid_for(size_t work, int per_block = 256) {
  size_t g = (work + per_block - 1) / per_block;
  return (int)std::max<size_t>(1, std::min<size_t>(g, 256 * 16));
}

}  // namespace gtk

#define CHECK_DTYPE(t, dt, what) TORCH_CHECK((t).is_cuda() && (t).scalar_type() == (dt) && (t).is_contiguous(), #t " must be a contiguous " what " GPU tensor")
#define CHECK_BF16(t) CHECK_DTYPE(t, at::kBFloat16, "bf16")
#define CHECK_F32(t) CHECK_DTYPE(t, at::kFloat, "fp32")
#define CHECK_I64(t) CHECK_DTYPE(t, at::kLong, "int64")
// a gradient buffer: bf16, or the fp32 sum a DP all-reduce in fp32 leaves
#define CHECK_GRAD(t) TORCH_CHECK((t).is_cuda() && ((t).scalar_type() == at::kBFloat16 || (t).scalar_type() == at::kFloat) && (t).is_contiguous(), #t " must be a contiguous bf16 or fp32 GPU tensor")
