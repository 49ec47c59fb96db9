// K7 ZeRO-1 step: the push reduce with the AdamW update as its epilogue.  Device code only, in the style of
// peer_allreduce.h.
//
// Rank r owns slice r of the parameters: their fp32 master, m and v are rank-local memory that no peer ever
// reads.  Every rank's window holds the bf16 gradient of all parameters.  One launch per rank
//   sums slice r of every window in member order in fp32 and multiplies once by `scale`, as peer_reduce_vecs
//   does (on the fp8 wire: the dequantised packed forms, as peer_q8_sum_vecs does);
//   applies adam8_update (common/adamw_update.h, the body of every AdamW kernel of csrc/ops/adamw.hip) to
//   that gradient and the rank's master/m/v, and stores the three back;
//   pushes the new bf16 weights into slice r of every rank's out through PeerPushDst, own out first.
// The gradient shard never reaches memory and the weights are written once, where an all-gather would read
// and write them again: against reduce-scatter (fp32 out), AdamW and all-gather that is one launch for three,
// 8 bytes per slice element of gradient not written and re-read, and 2 bytes per element of weights not re-read.
//
// Both kernels are the reduce's own loads, sum and walk (peer_reduce_range, peer_q8_sum_range) with
// PeerAdamwEpi in place of the store epilogue, so the sum has the reduce's bits.  The epilogue's state loads
// of all U positions are issued with the members' loads, ahead of the first state store: through the same
// master/m/v pointers the compiler cannot hoist a later position's loads above an earlier position's stores
// (the note on Adam8In in csrc/ops/adamw.hip).  The hyper-parameters are the host form's eight floats, passed
// by value.  Padding: a slice is whole vectors (fp8: whole blocks); past the count the gradient is zero, and
// zero master/m/v stay zero under the update, so the padding of out is written as zero.
//
// fp32 windows have no kernel here: four lanes would give half a weight vector, and the wide bf16-to-fp32
// mean is what the fusion makes unnecessary.  No kernel waits for another kernel; vector stores only; no LDS.
#pragma once
#include "../common/adamw_update.h"
#include "peer_allreduce.h"
#include "peer_q8.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The epilogue of a position of E summed elements (8: a window vector of bf16; 16: a code vector): unit o of
// the launch's range, which starts at unit `first`, holds floats [E (o - first), E (o - first) + E) of the
// rank's master, m and v, and becomes E / 8 weight vectors at E / 8 * o of every destination.
template <int KB, int E>
struct PeerAdamwEpi {
  PeerPushDst<KB> sink;  // its first destination, the rank's own out, is the range's `dst`
  float scale;
  float* __restrict__ master;
  float* __restrict__ m;
  float* __restrict__ v;
  size_t first;
  gtk_adamw::Hyper h;

  template <int U>
  struct Pre {
    f32x4 s[U][3][E / 4];  // master, m, v
  };
  template <int U>
  __device__ __forceinline__ void load(Pre<U>& pre, int u, size_t o) const {
    const size_t e = (size_t)E * (o - first);
    const float* src[3] = {master + e, m + e, v + e};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int q = 0; q < E / 4; ++q) pre.s[u][a][q] = reinterpret_cast<const f32x4*>(src[a])[q];
  }
  template <int U>
  __device__ __forceinline__ void operator()(const Pre<U>& pre, int u, float (&acc)[E], u32x4* __restrict__ dst, size_t o) const {
    const size_t e = (size_t)E * (o - first);
#pragma unroll
    for (int j = 0; j < E; ++j) acc[j] = acc[j] * scale;
    u32x4 w[E / 8];
#pragma unroll
    for (int half = 0; half < E / 8; ++half) {
      float p[8], mm[8], vv[8], g[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int q = 2 * half + j / 4;
        p[j] = pre.s[u][0][q][j % 4];
        mm[j] = pre.s[u][1][q][j % 4];
        vv[j] = pre.s[u][2][q][j % 4];
        g[j] = acc[8 * half + j];
      }
      gtk_adamw::adam_u16x8 wo;
      gtk_adamw::adam8_update(p, mm, vv, g, h, wo);
      float* out[3] = {master + e, m + e, v + e};
      const float* val[3] = {p, mm, vv};
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          f32x4 t;
#pragma unroll
          for (int j = 0; j < 4; ++j) t[j] = val[a][4 * q + j];
          reinterpret_cast<f32x4*>(out[a])[2 * half + q] = t;
        }
      w[half] = __builtin_bit_cast(u32x4, wo);  // element 2 j is the low half of word j, as peer_narrow packs
    }
    sink(w, dst, o * (E / 8));
  }
};

// Vectors [v0, v1) of every member's bf16 window: master/m/v floats [0, 8 (v1 - v0)) updated with scale * their
// sum, the new weights to vectors [v0, v1) of every dsts.p[d], d < k.
template <int KB, int U>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_reduce_adamw_push_kernel(SrcSet srcs, DstSet dsts, int k, size_t v0,
                                                                                   size_t v1, float scale, float* __restrict__ master,
                                                                                   float* __restrict__ m, float* __restrict__ v,
                                                                                   gtk_adamw::Hyper h) {
  peer_reduce_range<uint16_t, KB, U>(srcs, k, v0, v1,
                                     PeerAdamwEpi<KB, 8>{PeerPushDst<KB>{dsts, k}, scale, master, m, v, v0, h}, dsts.p[0]);
}

// Blocks [b0, b1) of every member's packed buffer: master/m/v floats [0, 32 (b1 - b0)) updated with scale * the
// sum of the dequantised blocks, the new weights to blocks [b0, b1) of every dsts.p[d], d < k: four vectors a
// block, two from each of its code vectors.
template <int KB, int U>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_q8_sum_adamw_push_kernel(SrcSet srcs, DstSet dsts, int k, size_t exp_vec,
                                                                                   size_t b0, size_t b1, float scale,
                                                                                   float* __restrict__ master, float* __restrict__ m,
                                                                                   float* __restrict__ v, gtk_adamw::Hyper h) {
  peer_q8_sum_range<KB, U>(srcs, k, exp_vec, b0, b1,
                           PeerAdamwEpi<KB, 16>{PeerPushDst<KB>{dsts, k}, scale, master, m, v, 2 * b0, h}, dsts.p[0]);
}

// The member buckets of the reduce, with fewer positions per lane: a position holds its six (fp8: twelve)
// state vectors next to the members' loads, and no instantiation may spill.
void launch_peer_reduce_adamw_push(const SrcSet& set, const DstSet& dsts, int k, size_t v0, size_t v1, float scale, float* master,
                                   float* m, float* v, const gtk_adamw::Hyper& h, int grid, hipStream_t s) {
  const dim3 g(grid), b(kBlock);
  if (k <= 2)
    peer_reduce_adamw_push_kernel<2, 4><<<g, b, 0, s>>>(set, dsts, k, v0, v1, scale, master, m, v, h);
  else if (k <= 4)
    peer_reduce_adamw_push_kernel<4, 2><<<g, b, 0, s>>>(set, dsts, k, v0, v1, scale, master, m, v, h);
  else if (k <= 8)
    peer_reduce_adamw_push_kernel<8, 2><<<g, b, 0, s>>>(set, dsts, k, v0, v1, scale, master, m, v, h);
  else
    peer_reduce_adamw_push_kernel<16, 1><<<g, b, 0, s>>>(set, dsts, k, v0, v1, scale, master, m, v, h);
  HIP_CHECK(hipGetLastError());
}

void launch_peer_q8_sum_adamw_push(const SrcSet& packed, const DstSet& dsts, int k, size_t exp_vec, size_t b0, size_t b1, float scale,
                                   float* master, float* m, float* v, const gtk_adamw::Hyper& h, int grid, hipStream_t s) {
  const dim3 g(grid), b(kBlock);
  if (k <= 2)
    peer_q8_sum_adamw_push_kernel<2, 2><<<g, b, 0, s>>>(packed, dsts, k, exp_vec, b0, b1, scale, master, m, v, h);
  else if (k <= 4)
    peer_q8_sum_adamw_push_kernel<4, 2><<<g, b, 0, s>>>(packed, dsts, k, exp_vec, b0, b1, scale, master, m, v, h);
  else if (k <= 8)
    peer_q8_sum_adamw_push_kernel<8, 1><<<g, b, 0, s>>>(packed, dsts, k, exp_vec, b0, b1, scale, master, m, v, h);
  else
    peer_q8_sum_adamw_push_kernel<16, 1><<<g, b, 0, s>>>(packed, dsts, k, exp_vec, b0, b1, scale, master, m, v, h);
  HIP_CHECK(hipGetLastError());
}

}  // namespace
