// K8: link latency by a dependent-load chase, device side.  A fragment of csrc/probe/probe.hip,
// included there at file scope like peer_allreduce.h; the code below joins its unnamed namespace.
//
// The chain: a buffer of n = ws_bytes / stride nodes, n and stride powers of two, stride >= 4,
// ws_bytes <= 4 GiB.  Node i is a uint32 at byte i * stride and holds the BYTE OFFSET of its successor
// next(i) = (A * i + C) mod n, so a hop is one load, one mask and the address add of the next load.
// C is odd and A = 1 (mod 4), so by Hull-Dobell the map is one cycle through all n nodes for every
// power-of-two n, and it walks the buffer in no order a prefetcher or an open DRAM page could follow.
// n divides 2^32, so the map is computed in wrapping uint32 arithmetic and masked.  The successor after
// any number of hops has a closed form (the affine map composed by doubling), which the host driver
// and ops/chase_ref.py use to know where every lane must stand after every launch.
//
// No kernel here waits for another kernel, and nothing spins: a launch ends after `hops` loads.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../common/stream_copy.h"

namespace {

constexpr unsigned int kChainA = 1664525u;
constexpr unsigned int kChainC = 1013904223u;
constexpr int kChaseUnroll = 8;
constexpr int kChaseMaxChains = 64;  // one wave: a lane per chain

// Node i (at byte i << log2_stride) = next(i) << log2_stride, for every i < n.  The bytes between the
// nodes are never read and stay as they were allocated.
__global__ __launch_bounds__(gtk::kStreamBlock) void chase_fill_kernel(unsigned char* __restrict__ base, size_t n,
                                                                       unsigned int log2_stride) {
  const unsigned int node_mask = (unsigned int)(n - 1);
  for (size_t i = (size_t)blockIdx.x * gtk::kStreamBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * gtk::kStreamBlock) {
    const unsigned int next = ((unsigned int)i * kChainA + kChainC) & node_mask;
    *reinterpret_cast<unsigned int*>(base + (i << log2_stride)) = next << log2_stride;
  }
}

// One hop: a plain 4-byte vector load (no nt / sc bits, what ordinary code issues), and the loaded
// value masked to a node's offset before it may become an address: a corrupted node cannot send the
// next load outside the allocation.
__device__ __forceinline__ unsigned int chase_hop(const unsigned char* __restrict__ base, unsigned int off,
                                                  unsigned int off_mask) {
  return *reinterpret_cast<const unsigned int*>(base + off) & off_mask;
}

// One wave.  Lane l < chains follows its own chain for `hops` dependent loads from byte offset pos[l]
// and leaves the offset it reached in pos[l], so the next launch continues where this one ended; the
// other lanes exit.  Lane 0 stores the wall-clock ticks (hipDeviceAttributeWallClockRate) the loop took.
//
// `off` is made opaque in a VGPR first: with the start a kernel argument the compiler proves the
// address uniform and would walk the chain through the scalar cache (s_load_dword), which is not the
// path a kernel's loads take.  The first clock read is waited for before the first load issues, and the
// second is ordered after the last loaded value has arrived: both asm statements take `off`.
__global__ __launch_bounds__(64) void chase_kernel(const unsigned char* __restrict__ base, unsigned int off_mask,
                                                   unsigned int* __restrict__ pos, int chains, int hops,
                                                   unsigned long long* __restrict__ ticks) {
  const int lane = threadIdx.x;
  if (lane >= chains) return;
  unsigned int off = pos[lane] & off_mask;
  asm volatile("" : "+v"(off));
  unsigned long long t0 = wall_clock64();
  asm volatile("" : "+v"(off), "+s"(t0));
  int h = 0;
  for (; h + kChaseUnroll <= hops; h += kChaseUnroll) {
#pragma unroll
    for (int u = 0; u < kChaseUnroll; ++u) off = chase_hop(base, off, off_mask);
  }
  for (; h < hops; ++h) off = chase_hop(base, off, off_mask);
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(off)::"memory");
  const unsigned long long t1 = wall_clock64();
  pos[lane] = off;
  if (lane == 0) *ticks = t1 - t0;
}

// f^hops of the chain's map f(x) = A x + C (mod 2^32), as (a, c): f^hops(x) = a x + c.  O(log hops).
struct ChainMap {
  unsigned int a = 1u, c = 0u;
  unsigned int operator()(unsigned int x) const { return a * x + c; }
};
inline ChainMap chain_power(unsigned long long hops) {
  ChainMap r, f{kChainA, kChainC};
  for (; hops; hops >>= 1) {
    if (hops & 1) r = ChainMap{f.a * r.a, f.a * r.c + f.c};
    f = ChainMap{f.a * f.a, f.a * f.c + f.c};
  }
  return r;
}
// The node reached from `start` after `hops` hops in a chain of n nodes (n a power of two <= 2^30).
inline unsigned int chain_skip(unsigned int start, unsigned long long hops, size_t n) {
  return chain_power(hops)(start) & (unsigned int)(n - 1);
}

}  // namespace
