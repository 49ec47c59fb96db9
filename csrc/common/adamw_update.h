// The one AdamW update body (decoupled weight decay), on registers: eight master/m/v values and eight
// gradient values in, the eight new master/m/v values and the eight new bf16 weights out.  Every kernel
// that updates a weight instantiates adam8_update, so master/m/v/W get the same expressions whichever
// kernel touches them: the flat, range and tile kernels of csrc/ops/adamw.hip, and the ZeRO-1 epilogue of
// the peer push reduce (csrc/probe/peer_zero1.h), whose gradient is a sum it holds in registers.
//
// Device code only and free of torch: csrc/probe includes it too.  Loads, stores and where the
// hyper-parameters come from are the including kernel's.
#pragma once
#include <hip/hip_runtime.h>

namespace gtk_adamw {

typedef unsigned short adam_u16x8 __attribute__((ext_vector_type(8)));  // gtk::u16x8: eight bf16 as raw words

// [lr, beta1, beta2, eps, weight_decay, grad_scale, bias_c1, bias_c2]: the host form's hp in its order
// (bias_c = 1 - beta^t), so eight floats read as a Hyper.
struct Hyper {
  float lr, b1, b2, eps, wd, gs, bc1, bc2;
};

__device__ __forceinline__ unsigned short f2bf(float f) {  // round to nearest even, as gtk::f2bf of ops/bf16.h
  return __builtin_bit_cast(unsigned short, (__bf16)f);
}

// p, mm, vv: master, m and v, updated in place; gf: the gradient before grad_scale; wo: the new weights.
__device__ __forceinline__ void adam8_update(float (&p)[8], float (&mm)[8], float (&vv)[8], const float (&gf)[8], const Hyper& h,
                                             adam_u16x8& wo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {  // the AdamW update: every kernel's bits come from these expressions
    const float gr = gf[j] * h.gs;
    mm[j] = h.b1 * mm[j] + (1.f - h.b1) * gr;
    vv[j] = h.b2 * vv[j] + (1.f - h.b2) * gr * gr;
    const float upd = (mm[j] / h.bc1) / (sqrtf(vv[j] / h.bc2) + h.eps);
    p[j] = p[j] - h.lr * (upd + h.wd * p[j]);
    wo[j] = f2bf(p[j]);
  }
}

}  // namespace gtk_adamw
