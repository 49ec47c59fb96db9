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
// mean is what the fusion makes unnecessary.  No kernel waits for another kernel; vector stores only; no LDS in the fused
// kernels (the clipped step's first launch, further down, keeps four floats there for its block sum).
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

// -- the clipped step: two launches, the global norm between them ---------------------------------------------
// Clipping by the global norm needs the norm of the summed gradient before any element is updated, and the fused
// kernels above never write that sum.  The clipped step keeps every gradient byte to one trip over a link:
//   launch 1 (peer_reduce_sqnorm_stash_kernel, peer_q8_sum_sqnorm_stash_kernel) is the reduce's loads, sum and walk
//     with PeerSqnormStashEpi: the scaled fp32 sum goes to a rank-local fp32 *stash* (a fourth array next to master,
//     m and v, its owner's alone) and its squares into a per-lane accumulator, one partial per block at the end;
//   the host adds the partials in float64, the ranks exchange their totals at a barrier and derive one factor;
//   launch 2 (peer_adamw_push_kernel) walks the stash, rank-local memory only, and runs PeerAdamwEpi on it with
//     scale = 1 and that factor as grad_scale: the update and the push of the fused step, unchanged.
// The stash is stored plainly, not non-temporally: launch 2 reads it back at once, and the cache is where it should
// be found.  No kernel waits for another kernel; vector stores only.

// The sum of s over the block's 256 lanes, in lane 0: six exchanges inside a wave, two adds across the four waves.
__device__ __forceinline__ float peer_block_sum(float s) {
  __shared__ float red[kBlock / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// The epilogue of launch 1 for a position of E summed elements: unit o of a range that starts at unit `first`
// becomes floats [E (o - first), E (o - first) + E) of the stash, which is the range's `dst`, after the one
// multiply by `scale` that peer_store and PeerAdamwEpi make, so these are the bits the update would have seen.
// `sq` is the lane's sum of their squares so far.  The epilogue is handed down as const, hence `mutable`: the
// kernel owns the one object, a local that ends up in a register, and reads the sum back after the walk.
template <int E>
struct PeerSqnormStashEpi {
  float scale;
  size_t first;
  mutable float sq;

  template <int U>
  struct Pre {};
  template <int U>
  __device__ __forceinline__ void load(Pre<U>&, int, size_t) const {}
  template <int U>
  __device__ __forceinline__ void operator()(const Pre<U>&, int, float (&acc)[E], u32x4* __restrict__ dst, size_t o) const {
    u32x4* out = dst + (size_t)(E / 4) * (o - first);
#pragma unroll
    for (int j = 0; j < E; ++j) acc[j] = acc[j] * scale;
#pragma unroll
    for (int q = 0; q < E / 4; ++q) {
      u32x4 t;
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = __float_as_uint(acc[4 * q + j]);
      out[q] = t;
    }
    float s = 0.f;  // the position's own sum first: one add per position on the chain that runs through the walk
#pragma unroll
    for (int j = 0; j < E; ++j) s = s + acc[j] * acc[j];
    sq = sq + s;
  }
};

// Vectors [v0, v1) of every member's bf16 window: stash floats [0, 8 (v1 - v0)) = scale * their sum, and
// parts[blockIdx.x] = the sum of the squares of what this block stored (0 for a block with no work: every slot of
// parts[0, gridDim.x) is written, so nothing needs a memset).
template <int KB, int U>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_reduce_sqnorm_stash_kernel(SrcSet srcs, int k, size_t v0, size_t v1, float scale,
                                                                                     u32x4* __restrict__ stash, float* __restrict__ parts) {
  const PeerSqnormStashEpi<8> epi{scale, v0, 0.f};
  peer_reduce_range<uint16_t, KB, U>(srcs, k, v0, v1, epi, stash);
  const float total = peer_block_sum(epi.sq);
  if (threadIdx.x == 0) parts[blockIdx.x] = total;
}

// Blocks [b0, b1) of every member's packed buffer: stash floats [0, 32 (b1 - b0)) = scale * the sum of the
// dequantised blocks, parts as above.
template <int KB, int U>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_q8_sum_sqnorm_stash_kernel(SrcSet srcs, int k, size_t exp_vec, size_t b0,
                                                                                     size_t b1, float scale, u32x4* __restrict__ stash,
                                                                                     float* __restrict__ parts) {
  const PeerSqnormStashEpi<16> epi{scale, 2 * b0, 0.f};
  peer_q8_sum_range<KB, U>(srcs, k, exp_vec, b0, b1, epi, stash);
  const float total = peer_block_sum(epi.sq);
  if (threadIdx.x == 0) parts[blockIdx.x] = total;
}

// -- gradient accumulation: launch 1 adds to the stash ------------------------------------------------------------
// A batch split into micro-batches keeps its gradient in the stash between calls: the first micro-batch's launch 1
// (above) stores its scaled sum there, and every later one runs the same loads, sum and walk with PeerSqnormAccumEpi,
// which adds the scaled sum to what the stash holds and stores the total back: an fp32 accumulator split over the
// ranks, never rounded to bf16.  The total's squares go into the lane's `sq` as above, so the last micro-batch's launch
// is launch 1 of a step on the accumulated gradient, and launch 2 (peer_adamw_push_kernel) follows unchanged.
//
// The epilogue of the adding launch for a position of E summed elements: unit o of a range that starts at unit `first`
// is floats [E (o - first), E (o - first) + E) of the accumulator.  They are read and written through the one pointer
// `acc` the epilogue holds, as PeerAdamwEpi reads and writes master, m and v, and the loads of all U positions are
// issued with the members' loads, ahead of the first store, for the reason given at the top of this file.  The range's
// `dst` is not used: it is a __restrict__ parameter, and what is stored through it must not be read through a member.
// Per element: the sum, one multiply by `scale`, one add to the accumulator, each rounded to fp32.  The multiply is
// not contracted into the add: the reference rounds twice, and the accumulator has its bits.
template <int E>
struct PeerSqnormAccumEpi {
  float scale;
  float* __restrict__ acc;
  size_t first;
  mutable float sq;

  template <int U>
  struct Pre {
    f32x4 a[U][E / 4];
  };
  template <int U>
  __device__ __forceinline__ void load(Pre<U>& pre, int u, size_t o) const {
    const f32x4* src = reinterpret_cast<const f32x4*>(acc + (size_t)E * (o - first));
#pragma unroll
    for (int q = 0; q < E / 4; ++q) pre.a[u][q] = src[q];
  }
  template <int U>
  __device__ __forceinline__ void operator()(const Pre<U>& pre, int u, float (&sum)[E], u32x4* __restrict__, size_t o) const {
    f32x4* out = reinterpret_cast<f32x4*>(acc + (size_t)E * (o - first));
    {
#pragma clang fp contract(off)
#pragma unroll
      for (int j = 0; j < E; ++j) {
        const float piece = sum[j] * scale;
        sum[j] = pre.a[u][j / 4][j % 4] + piece;
      }
    }
#pragma unroll
    for (int q = 0; q < E / 4; ++q) {
      f32x4 t;
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = sum[4 * q + j];
      out[q] = t;
    }
    float s = 0.f;  // as PeerSqnormStashEpi: the position's own sum first
#pragma unroll
    for (int j = 0; j < E; ++j) s = s + sum[j] * sum[j];
    sq = sq + s;
  }
};

// Vectors [v0, v1) of every member's bf16 window: accumulator floats [0, 8 (v1 - v0)) += scale * their sum, and
// parts[blockIdx.x] = the sum of the squares of the totals this block stored (0 for a block with no work).
template <int KB, int U>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_reduce_sqnorm_accum_kernel(SrcSet srcs, int k, size_t v0, size_t v1, float scale,
                                                                                     float* __restrict__ acc, float* __restrict__ parts) {
  const PeerSqnormAccumEpi<8> epi{scale, acc, v0, 0.f};
  peer_reduce_range<uint16_t, KB, U>(srcs, k, v0, v1, epi, nullptr);
  const float total = peer_block_sum(epi.sq);
  if (threadIdx.x == 0) parts[blockIdx.x] = total;
}

// Blocks [b0, b1) of every member's packed buffer: accumulator floats [0, 32 (b1 - b0)) += scale * the sum of the
// dequantised blocks, parts as above.
template <int KB, int U>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_q8_sum_sqnorm_accum_kernel(SrcSet srcs, int k, size_t exp_vec, size_t b0,
                                                                                     size_t b1, float scale, float* __restrict__ acc,
                                                                                     float* __restrict__ parts) {
  const PeerSqnormAccumEpi<16> epi{scale, acc, 2 * b0, 0.f};
  peer_q8_sum_range<KB, U>(srcs, k, exp_vec, b0, b1, epi, nullptr);
  const float total = peer_block_sum(epi.sq);
  if (threadIdx.x == 0) parts[blockIdx.x] = total;
}

// U positions of launch 2 per lane, `stride` apart from `i`: a position is one weight vector, eight stash floats
// and eight floats each of master, m and v.  The 2 U gradient loads and the 6 U state loads are issued before the
// first state store, for the reason given at the top of this file.
template <int KB, int U>
__device__ __forceinline__ void peer_adamw_push_vecs(const f32x4* __restrict__ stash, const PeerAdamwEpi<KB, 8>& epi,
                                                     u32x4* __restrict__ dst, size_t i, size_t stride) {
  f32x4 g[U][2];
  typename PeerAdamwEpi<KB, 8>::template Pre<U> pre;
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int q = 0; q < 2; ++q) g[u][q] = stash[2 * (i + (size_t)u * stride - epi.first) + q];
#pragma unroll
  for (int u = 0; u < U; ++u) epi.load(pre, u, i + (size_t)u * stride);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = g[u][j / 4][j % 4];
    epi(pre, u, acc, dst, i + (size_t)u * stride);
  }
}

// Weight vectors [v0, v1) of every dsts.p[d], d < k, from stash and state floats [0, 8 (v1 - v0)): AdamW with the
// stash as the gradient, which launch 1 has scaled already, so the epilogue's own scale is 1 and changes no bit.
// The walk is the reduce's: whole tiles in one contiguous run per block, the rest one position per lane.
template <int KB, int U>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_adamw_push_kernel(DstSet dsts, int k, size_t v0, size_t v1,
                                                                            const f32x4* __restrict__ stash, float* __restrict__ master,
                                                                            float* __restrict__ m, float* __restrict__ v,
                                                                            gtk_adamw::Hyper h) {
  const PeerAdamwEpi<KB, 8> epi{PeerPushDst<KB>{dsts, k}, 1.0f, master, m, v, v0, h};
  const size_t tile = (size_t)gtk::kStreamBlock * U;
  const size_t n_tiles = (v1 - v0) / tile;
  const size_t per = (n_tiles + gridDim.x - 1) / gridDim.x;
  const size_t t0 = (size_t)blockIdx.x * per;
  const size_t t1 = std::min(n_tiles, t0 + per);
  for (size_t t = t0; t < t1; ++t) peer_adamw_push_vecs<KB, U>(stash, epi, dsts.p[0], v0 + t * tile + threadIdx.x, gtk::kStreamBlock);
  for (size_t i = v0 + n_tiles * tile + (size_t)blockIdx.x * gtk::kStreamBlock + threadIdx.x; i < v1;
       i += (size_t)gridDim.x * gtk::kStreamBlock)
    peer_adamw_push_vecs<KB, 1>(stash, epi, dsts.p[0], i, 0);
}

// Launch 1 has no state loads, so it starts from the reduce's own buckets (peer_driver.h).
void launch_peer_reduce_sqnorm_stash(const SrcSet& set, int k, size_t v0, size_t v1, float scale, float* stash, float* parts, int grid,
                                     hipStream_t s) {
  const dim3 g(grid), b(kBlock);
  u32x4* st = reinterpret_cast<u32x4*>(stash);
  if (k <= 2)
    peer_reduce_sqnorm_stash_kernel<2, 4><<<g, b, 0, s>>>(set, k, v0, v1, scale, st, parts);
  else if (k <= 4)
    peer_reduce_sqnorm_stash_kernel<4, 4><<<g, b, 0, s>>>(set, k, v0, v1, scale, st, parts);
  else if (k <= 8)
    peer_reduce_sqnorm_stash_kernel<8, 2><<<g, b, 0, s>>>(set, k, v0, v1, scale, st, parts);
  else
    peer_reduce_sqnorm_stash_kernel<16, 1><<<g, b, 0, s>>>(set, k, v0, v1, scale, st, parts);
  HIP_CHECK(hipGetLastError());
}

void launch_peer_q8_sum_sqnorm_stash(const SrcSet& packed, int k, size_t exp_vec, size_t b0, size_t b1, float scale, float* stash,
                                     float* parts, int grid, hipStream_t s) {
  const dim3 g(grid), b(kBlock);
  u32x4* st = reinterpret_cast<u32x4*>(stash);
  if (k <= 2)
    peer_q8_sum_sqnorm_stash_kernel<2, 4><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, scale, st, parts);
  else if (k <= 4)
    peer_q8_sum_sqnorm_stash_kernel<4, 4><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, scale, st, parts);
  else if (k <= 8)
    peer_q8_sum_sqnorm_stash_kernel<8, 2><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, scale, st, parts);
  else
    peer_q8_sum_sqnorm_stash_kernel<16, 1><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, scale, st, parts);
  HIP_CHECK(hipGetLastError());
}

// The adding launch holds a position's two (fp8: four) accumulator vectors next to the members' loads; the reduce's
// own buckets still leave no instantiation with scratch.
void launch_peer_reduce_sqnorm_accum(const SrcSet& set, int k, size_t v0, size_t v1, float scale, float* acc, float* parts, int grid,
                                     hipStream_t s) {
  const dim3 g(grid), b(kBlock);
  if (k <= 2)
    peer_reduce_sqnorm_accum_kernel<2, 4><<<g, b, 0, s>>>(set, k, v0, v1, scale, acc, parts);
  else if (k <= 4)
    peer_reduce_sqnorm_accum_kernel<4, 4><<<g, b, 0, s>>>(set, k, v0, v1, scale, acc, parts);
  else if (k <= 8)
    peer_reduce_sqnorm_accum_kernel<8, 2><<<g, b, 0, s>>>(set, k, v0, v1, scale, acc, parts);
  else
    peer_reduce_sqnorm_accum_kernel<16, 1><<<g, b, 0, s>>>(set, k, v0, v1, scale, acc, parts);
  HIP_CHECK(hipGetLastError());
}

void launch_peer_q8_sum_sqnorm_accum(const SrcSet& packed, int k, size_t exp_vec, size_t b0, size_t b1, float scale, float* acc,
                                     float* parts, int grid, hipStream_t s) {
  const dim3 g(grid), b(kBlock);
  if (k <= 2)
    peer_q8_sum_sqnorm_accum_kernel<2, 4><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, scale, acc, parts);
  else if (k <= 4)
    peer_q8_sum_sqnorm_accum_kernel<4, 4><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, scale, acc, parts);
  else if (k <= 8)
    peer_q8_sum_sqnorm_accum_kernel<8, 2><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, scale, acc, parts);
  else
    peer_q8_sum_sqnorm_accum_kernel<16, 1><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, scale, acc, parts);
  HIP_CHECK(hipGetLastError());
}

// Launch 2 holds no member loads: a position is eight vectors whatever k is, and KB sizes the push alone.
void launch_peer_adamw_push(const DstSet& dsts, int k, size_t v0, size_t v1, const float* stash, float* master, float* m, float* v,
                            const gtk_adamw::Hyper& h, int grid, hipStream_t s) {
  const dim3 g(grid), b(kBlock);
  const f32x4* st = reinterpret_cast<const f32x4*>(stash);
  if (k <= 2)
    peer_adamw_push_kernel<2, 2><<<g, b, 0, s>>>(dsts, k, v0, v1, st, master, m, v, h);
  else if (k <= 4)
    peer_adamw_push_kernel<4, 2><<<g, b, 0, s>>>(dsts, k, v0, v1, st, master, m, v, h);
  else if (k <= 8)
    peer_adamw_push_kernel<8, 2><<<g, b, 0, s>>>(dsts, k, v0, v1, st, master, m, v, h);
  else
    peer_adamw_push_kernel<16, 2><<<g, b, 0, s>>>(dsts, k, v0, v1, st, master, m, v, h);
  HIP_CHECK(hipGetLastError());
}

}  // namespace
