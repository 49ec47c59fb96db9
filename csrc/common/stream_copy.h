// Device-side pieces of a streaming copy in 16-byte vectors, shared by the link probe's copy kernels
// (csrc/probe/probe.hip) and the one-rank all-reduce's copy kernel (csrc/rccl/self_copy.h).
// Device code only.  Every kernel built from these runs blocks of kStreamBlock threads; all indices
// are 64-bit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

namespace gtk {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kStreamBlock = 256;

// Body of whole tiles (kStreamBlock x U vectors each), cut into contiguous slices: block `blk` of
// `nblk` streams tiles [blk*per, min(n_tiles, (blk+1)*per)), so each workgroup walks one DRAM region
// instead of the whole grid sweeping one window together.  Every lane keeps U independent
// non-temporal 16-byte loads in flight, then stores them non-temporally.  Returns the number of
// vectors the body covers over all blocks, which is where the tail starts.
template <int U>
__device__ __forceinline__ size_t stream_slices(const u32x4* __restrict__ src, u32x4* __restrict__ dst, size_t n_vec,
                                                size_t blk, size_t nblk) {
  const size_t tile = (size_t)kStreamBlock * U;
  const size_t n_tiles = n_vec / tile;
  const size_t per = (n_tiles + nblk - 1) / nblk;
  const size_t t0 = blk * per;
  const size_t t1 = std::min(n_tiles, t0 + per);
  for (size_t t = t0; t < t1; ++t) {
    const size_t base = t * tile + threadIdx.x;
    u32x4 r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) r[u] = __builtin_nontemporal_load(src + base + (size_t)u * kStreamBlock);
#pragma unroll
    for (int u = 0; u < U; ++u) __builtin_nontemporal_store(r[u], dst + base + (size_t)u * kStreamBlock);
  }
  return n_tiles * tile;
}

// Tail of under one tile of whole vectors, [first, n_vec): a grid-stride per-thread copy.
__device__ __forceinline__ void stream_vec_tail(const u32x4* __restrict__ src, u32x4* __restrict__ dst, size_t n_vec,
                                                size_t first, size_t blk, size_t nblk) {
  for (size_t i = first + blk * kStreamBlock + threadIdx.x; i < n_vec; i += nblk * kStreamBlock) dst[i] = src[i];
}

}  // namespace gtk
