// K7: all-reduce (sum) over peer pointers, device side, over SrcSet / kMaxSrc of probe_common.h.
// Device code only, in the style of csrc/common/stream_copy.h: blocks of gtk::kStreamBlock threads,
// 64-bit indices, 16-byte vectors.
//
// Every member's buffers are padded with zeros to a whole number of vectors by the host driver, so
// no kernel sees a scalar tail.  The sum of one element is fp32, taken in member order
// ((x0 + x1) + x2) + ... with no tree and no reassociation, multiplied once by the call's scale (1 for
// a sum, 1/k for a mean) and rounded once: every member computes the same bits, and a sequential CPU
// sum reproduces them (ops/peer_ref.py).  The output may be wider than the input: bf16 read over the
// link, fp32 written, which halves the link traffic of reducing a widened copy.
//
// The inputs may hold anything.  The adds, the multiply and the rounding are IEEE: subnormals of fp32
// and of bf16 are kept, never flushed; Inf + -Inf and anything with a NaN give NaN; -0 + -0 = -0; a sum
// that reaches 0x7F7F8000 rounds to a bf16 Inf.  Which NaN comes out (sign, payload) is the hardware's
// choice, the same on every member; tests/test_gpu_peer_nonfinite.py compares the rest bit for bit.
//
// The push form (peer_reduce_push_kernel) is the same body with another sink for the stores: every result
// vector goes to every member's `out`, so what is said above about the bits holds for it unchanged.  What
// follows a position's sum is an epilogue (PeerStoreEpi: scale, round, store); the ZeRO-1 step of peer_zero1.h
// is the same loads, sum and walk with the AdamW update as the epilogue.
//
// No kernel here waits for another running kernel: the all-reduce's cross-member ordering is stream
// events between launches (the host driver in peer_driver.h), visibility rests on kernel boundaries.
#pragma once
#include "probe_common.h"

namespace {

// fp32 lanes of one 16-byte vector: 4 of float, 8 of bf16 (raw u16; element 2j is the low half of word j).
template <typename T>
constexpr int kPeerLanes = 16 / (int)sizeof(T);

__device__ __forceinline__ void peer_widen(const u32x4& v, float (&f)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) f[j] = __uint_as_float(v[j]);
}
__device__ __forceinline__ void peer_widen(const u32x4& v, float (&f)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = __uint_as_float(v[j] << 16);
    f[2 * j + 1] = __uint_as_float(v[j] & 0xffff0000u);
  }
}
__device__ __forceinline__ u32x4 peer_narrow(const float (&f)[4]) {
  u32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = __float_as_uint(f[j]);
  return v;
}
__device__ __forceinline__ unsigned int peer_bf16_bits(float x) {  // round to nearest even
  return (unsigned int)__builtin_bit_cast(unsigned short, (__bf16)x);
}
__device__ __forceinline__ u32x4 peer_narrow(const float (&f)[8]) {
  u32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = peer_bf16_bits(f[2 * j]) | (peer_bf16_bits(f[2 * j + 1]) << 16);
  return v;
}

// Where a position's rounded result goes: `sink(v, dst, o)` stores the N vectors v[] at vector offsets
// o, o + 1, ... of `dst`, the launch's first (PeerOneDst: only) destination, non-temporally.  PeerPushDst is the push form:
// after `dst`, which is dsts.p[0], the same vectors go to dsts.p[d] + o for every 0 < d < k, in the set's order
// (the host chooses it) and destination by destination, so the adjacent vectors of one position reach each
// destination back to back; KB is the member bucket as in peer_reduce_vecs, so p[] is indexed by constants only.
struct PeerOneDst {
  template <int N>
  __device__ __forceinline__ void operator()(const u32x4 (&v)[N], u32x4* __restrict__ dst, size_t o) const {
#pragma unroll
    for (int j = 0; j < N; ++j) __builtin_nontemporal_store(v[j], dst + o + j);
  }
};
template <int KB>
struct PeerPushDst {
  const DstSet& dsts;
  int k;
  template <int N>
  __device__ __forceinline__ void operator()(const u32x4 (&v)[N], u32x4* __restrict__ dst, size_t o) const {
#pragma unroll
    for (int j = 0; j < N; ++j) __builtin_nontemporal_store(v[j], dst + o + j);
#pragma unroll
    for (int d = 1; d < KB; ++d)
      if (d < k) {
#pragma unroll
        for (int j = 0; j < N; ++j) __builtin_nontemporal_store(v[j], dsts.p[d] + o + j);
      }
  }
};

// One position's result: `scale` applied to the fp32 sum, then a bf16 output rounds once and stores one
// vector at `o`; an fp32 output of bf16 inputs (the wide form) stores two, at 2 * o and 2 * o + 1, so its
// offsets and slice bounds are twice the input's.  scale == 1.0f changes no bit of the sum.
template <typename TO, int L, typename Sink>
__device__ __forceinline__ void peer_store(float (&acc)[L], float scale, const Sink& sink, u32x4* __restrict__ dst, size_t o) {
#pragma unroll
  for (int j = 0; j < L; ++j) acc[j] = acc[j] * scale;
  if constexpr (L == kPeerLanes<TO>) {
    const u32x4 v[1] = {peer_narrow(acc)};
    sink(v, dst, o);
  } else {
    static_assert(L == 8 && kPeerLanes<TO> == 4, "the wide form is bf16 in, fp32 out");
    u32x4 v[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[0][j] = __float_as_uint(acc[j]);
      v[1][j] = __float_as_uint(acc[4 + j]);
    }
    sink(v, dst, 2 * o);
  }
}

// What follows a position's sum is an epilogue, `epi`:
//   typename Epi::template Pre<U>   what it holds of its own per lane for U positions (PeerStoreEpi: nothing);
//   epi.load(pre, u, o)             issues position u's own loads, at unit offset o, next to the members' loads;
//   epi(pre, u, acc, dst, o)        takes the position's fp32 sum, not yet scaled, and stores what becomes of it;
//                                   `dst` is the launch's first destination, handed down as a __restrict__
//                                   parameter so that the members' loads may pass the stores to it.
// PeerStoreEpi is the reduce itself: peer_store through a sink into `dst`, element type TO.  The fp8 wire's sum
// (peer_q8.h) runs the same epilogues on sixteen sums per position, and peer_zero1.h has the AdamW one.
template <typename TO, typename Sink>
struct PeerStoreEpi {
  Sink sink;
  float scale;
  template <int U>
  struct Pre {};
  template <int U>
  __device__ __forceinline__ void load(Pre<U>&, int, size_t) const {}
  template <int U, int L>
  __device__ __forceinline__ void operator()(const Pre<U>&, int, float (&acc)[L], u32x4* __restrict__ dst, size_t o) const {
    peer_store<TO>(acc, scale, sink, dst, o);
  }
};

// U vectors per lane, `stride` apart from `i`: the k x U loads (member-major, all in flight before the
// first add) and the epilogue's own, then per position the sum in member order and the epilogue: for the
// reduce one multiply by `scale`, one rounding and the store.  TI is the input element type.  KB is the
// member bucket the registers are sized for (k <= KB): r[] is indexed by constants only.
template <typename TI, int KB, int U, typename Epi>
__device__ __forceinline__ void peer_reduce_vecs(const SrcSet& srcs, int k, const Epi& epi, u32x4* __restrict__ dst, size_t i,
                                                 size_t stride) {
  u32x4 r[KB][U];
  typename Epi::template Pre<U> pre;
#pragma unroll
  for (int m = 0; m < KB; ++m)
    if (m < k) {
#pragma unroll
      for (int u = 0; u < U; ++u) r[m][u] = __builtin_nontemporal_load(srcs.p[m] + i + (size_t)u * stride);
    }
#pragma unroll
  for (int u = 0; u < U; ++u) epi.load(pre, u, i + (size_t)u * stride);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    float acc[kPeerLanes<TI>];
    peer_widen(r[0][u], acc);
#pragma unroll
    for (int m = 1; m < KB; ++m)
      if (m < k) {
        float x[kPeerLanes<TI>];
        peer_widen(r[m][u], x);
#pragma unroll
        for (int j = 0; j < kPeerLanes<TI>; ++j) acc[j] = acc[j] + x[j];
      }
    epi(pre, u, acc, dst, i + (size_t)u * stride);
  }
}

// The epilogue of the sum over members m < k of srcs.p[m][v0, v1), vectors of the input type TI (float, or
// bf16 as raw u16), position by position.  With PeerStoreEpi: dst[v0, v1), and the same vectors of what else
// the sink stores to, = scale * that sum; the wide form (bf16 in, float out) writes [2 * v0, 2 * v1).  Whole
// tiles (kStreamBlock x U vectors) are cut into one contiguous run per block, as gtk::stream_slices
// does; what is left of the range, under one tile, goes one vector per lane over the whole grid.
template <typename TI, int KB, int U, typename Epi>
__device__ __forceinline__ void peer_reduce_range(const SrcSet& srcs, int k, size_t v0, size_t v1, const Epi& epi,
                                                  u32x4* __restrict__ dst) {
  const size_t tile = (size_t)gtk::kStreamBlock * U;
  const size_t n_tiles = (v1 - v0) / tile;
  const size_t per = (n_tiles + gridDim.x - 1) / gridDim.x;
  const size_t t0 = (size_t)blockIdx.x * per;
  const size_t t1 = std::min(n_tiles, t0 + per);
  for (size_t t = t0; t < t1; ++t) peer_reduce_vecs<TI, KB, U>(srcs, k, epi, dst, v0 + t * tile + threadIdx.x, gtk::kStreamBlock);
  for (size_t i = v0 + n_tiles * tile + (size_t)blockIdx.x * gtk::kStreamBlock + threadIdx.x; i < v1;
       i += (size_t)gridDim.x * gtk::kStreamBlock)
    peer_reduce_vecs<TI, KB, 1>(srcs, k, epi, dst, i, 0);
}

// The reduce into the launching member's own `dst`.
template <typename TI, typename TO, int KB, int U>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_reduce_kernel(SrcSet srcs, int k, size_t v0, size_t v1,
                                                                        u32x4* __restrict__ dst, float scale) {
  peer_reduce_range<TI, KB, U>(srcs, k, v0, v1, PeerStoreEpi<TO, PeerOneDst>{PeerOneDst{}, scale}, dst);
}

// The push form: the same range, sum and rounding, every result vector stored to the same offset of every
// dsts.p[d], d < k: all members' `out`, the launching member's among them.  No member reads an `out`, and
// vectors [v0, v1) of every `out` are written by this launch alone, so a round needs no second phase.
template <typename TI, typename TO, int KB, int U>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_reduce_push_kernel(SrcSet srcs, DstSet dsts, int k, size_t v0,
                                                                             size_t v1, float scale) {
  peer_reduce_range<TI, KB, U>(srcs, k, v0, v1, PeerStoreEpi<TO, PeerPushDst<KB>>{PeerPushDst<KB>{dsts, k}, scale}, dsts.p[0]);
}

// Slice i of an all-gather: `count` vectors from vector `first` of p[i], to the same offset of dst.
struct SliceSet {
  const u32x4* p[kMaxSrc];
  size_t first[kMaxSrc];
  size_t count[kMaxSrc];
};

// Block b serves slice b % nsrc with gridDim / nsrc blocks (the grid is a multiple of nsrc), as the
// K5 gather does; slices differ in length and may be empty.
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_allgather_kernel(SliceSet sl, int nsrc,
                                                                           u32x4* __restrict__ dst) {
  const int s = blockIdx.x % nsrc;
  const size_t blk = blockIdx.x / nsrc, nblk = gridDim.x / nsrc;
  const u32x4* src = sl.p[s] + sl.first[s];
  u32x4* out = dst + sl.first[s];
  const size_t first = gtk::stream_slices<4>(src, out, sl.count[s], blk, nblk);
  gtk::stream_vec_tail(src, out, sl.count[s], first, blk, nblk);
}

// Test inputs: element i of the member with seed `seed` is a small integer in [-8, 7], so a sum over
// up to 16 members lies in [-128, 112] and is exact in bf16 as in fp32.  `narrow` keeps the integer's
// lowest bit alone, a value in {-1, 0}: a sum over up to 16 members is then an integer in [-16, 0], which
// has at most four significant bits and so survives a packing into e4m3 under any block scale.
__device__ __forceinline__ int peer_pattern(size_t i, unsigned int seed, bool narrow = false) {
  const int p = (int)((((unsigned int)i * 2654435761u + seed * 40503u) >> 16) & 15u) - 8;
  return narrow ? -(p & 1) : p;
}
__device__ __forceinline__ void peer_put(float* p, float x) { *p = x; }
__device__ __forceinline__ void peer_put(uint16_t* p, float x) { *p = (uint16_t)(__float_as_uint(x) >> 16); }
__device__ __forceinline__ float peer_get(const float* p) { return *p; }
__device__ __forceinline__ float peer_get(const uint16_t* p) { return __uint_as_float((unsigned int)*p << 16); }

// p[0, count) = pattern(seed); p[count, padded) = 0.
template <typename T>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_fill_kernel(T* __restrict__ p, size_t count, size_t padded,
                                                                      unsigned int seed, bool narrow = false) {
  for (size_t i = (size_t)blockIdx.x * gtk::kStreamBlock + threadIdx.x; i < padded;
       i += (size_t)gridDim.x * gtk::kStreamBlock)
    peer_put(p + i, i < count ? (float)peer_pattern(i, seed, narrow) : 0.f);
}

struct SeedSet {
  unsigned int s[kMaxSrc];
};

// Counts the elements of p[0, count) that differ from the sum of the k members' patterns, and the
// padding elements p[count, padded) that are not zero.
template <typename T>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_check_kernel(const T* __restrict__ p, size_t count,
                                                                       size_t padded, SeedSet seeds, int k,
                                                                       unsigned long long* bad, bool narrow = false) {
  unsigned long long local = 0;
  for (size_t i = (size_t)blockIdx.x * gtk::kStreamBlock + threadIdx.x; i < padded;
       i += (size_t)gridDim.x * gtk::kStreamBlock) {
    int want = 0;
    if (i < count)
      for (int m = 0; m < k; ++m) want += peer_pattern(i, seeds.s[m], narrow);
    local += (peer_get(p + i) != (float)want);
  }
  if (local) atomicAdd(bad, local);
}

}  // namespace
