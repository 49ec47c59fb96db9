// What every source of the _fused module starts from: bf16 values travel as raw 16-bit words (u16),
// eight to a 16-B vector; the math is fp32.  Each source pulls these names into its own namespace
// with `using namespace gtk;`.
#pragma once

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <cstdint>

namespace gtk {

typedef unsigned short u16;
typedef u16 u16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf2f(u16 v) { return __uint_as_float((uint32_t)v << 16); }
__device__ __forceinline__ u16 f2bf(float f) { return __builtin_bit_cast(u16, (__bf16)f); }

inline hipStream_t cur_stream() { return at::hip::getCurrentHIPStream().stream(); }
inline const u16* bp(const at::Tensor& t) { return reinterpret_cast<const u16*>(t.data_ptr()); }
inline u16* bpm(at::Tensor& t) { return reinterpret_cast<u16*>(t.data_ptr()); }

}  // namespace gtk

#define CHECK_BF16(t) TORCH_CHECK((t).is_cuda() && (t).scalar_type() == at::kBFloat16 && (t).is_contiguous(), #t " must be a contiguous bf16 GPU tensor")
