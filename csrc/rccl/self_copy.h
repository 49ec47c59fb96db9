// Streaming device copy for the one-rank all-reduce (included by rccl_core.h).
//
// On a one-rank communicator an out-of-place sum is an identity copy of the message from `send` to
// `recv`.  RCCL hands that to the HIP runtime's blit kernel, which moved the headline's 2 GiB at
// 2.38-2.50 TB/s in six bench.py runs on an MI355X; the kernel below moved it at 2.73-2.87 TB/s in six
// runs alternating with those (profiles/k1_self_copy/SUMMARY.md has every measured row).
//
// Shape: 256 threads per block, every lane keeps kSelfCopyUnroll independent 16-byte loads in flight
// and writes them back; loads and stores are non-temporal, since neither buffer is read again within
// a step and together they exceed the 256 MiB Infinity Cache at every size routed here.  The grid is
// capped at CUs x kSelfCopyBlocksPerCU blocks, and block b streams its own contiguous 1/grid slice of
// the message tile by tile.  The other candidate, the whole grid striding over the message together
// (the best arm of profiles/r06_prof/hbm_copy_sweep.log at 1 GiB), is as fast up to 1 GiB but falls off
// above it, to below the runtime's copy at 8 GiB: there every block meets a new page on every tile.
// The kernel works on bytes: a body of whole tiles, a tail of 16-byte vectors of under one tile, and
// a last tail of under 16 bytes copied in 2-byte units (every element type is a multiple of 2 bytes
// wide).  All indices are 64-bit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../common/stream_copy.h"

namespace gtk {

// Equal to the probe's kBlock / kUnroll / kBlocksPerCU today, but tuned on their own (these on the
// 2 GiB headline, the probe's on its LDS budget): kept separate on purpose.
constexpr int kSelfCopyBlock = 256;
constexpr int kSelfCopyUnroll = 4;
constexpr int kSelfCopyBlocksPerCU = 8;
constexpr size_t kSelfCopyTileVec = (size_t)kSelfCopyBlock * kSelfCopyUnroll;  // 16-byte vectors per tile
constexpr size_t kSelfCopyTileBytes = kSelfCopyTileVec * sizeof(u32x4);        // 16 KiB
static_assert(kSelfCopyBlock == kStreamBlock, "stream_copy.h indexes blocks of kStreamBlock threads");

// Messages below this many bytes stay with ncclAllReduce (RankState::self_copy_min's default).
// Measured from Comm.step() with bench/allreduce_k1_ab.py, GB/s copied, median of 5 alternating runs,
// runtime's copy / this kernel (profiles/k1_self_copy/allreduce_k1_ab.log).  While source and
// destination fit the 256 MiB Infinity Cache together the runtime's copy wins: 1 MiB 296 / 276,
// 16 MiB 3931 / 2948, 64 MiB 3458 / 3126, 128 MiB 3599 / 3030 (64 KiB, 18.5 / 17.6, is within the
// spread).  Once they do not, the kernel wins: 256 MiB 2700 / 2762, 512 MiB 2687 / 2816,
// 1 GiB 2416 / 2759, 2 GiB 2379 / 2743, 4 GiB 2414 / 2696, 8 GiB 2464 / 2741, 16 GiB 2371 / 2601.  In
// every row that names a winner the two arms' min-max ranges do not overlap.  The cutoff is the
// smallest measured size that wins; nothing between 128 and 256 MiB was measured.
constexpr size_t kSelfCopyMinBytes = (size_t)256 << 20;

// `src` and `dst` are 16-byte aligned and do not overlap; `bytes` is a multiple of 2.
__global__ __launch_bounds__(kSelfCopyBlock) void gtk_self_copy_kernel(const void* __restrict__ src_,
                                                                        void* __restrict__ dst_, size_t bytes) {
  const u32x4* __restrict__ src = static_cast<const u32x4*>(src_);
  u32x4* __restrict__ dst = static_cast<u32x4*>(dst_);
  const size_t n_vec = bytes / sizeof(u32x4);
  const size_t first = stream_slices<kSelfCopyUnroll>(src, dst, n_vec, blockIdx.x, gridDim.x);
  stream_vec_tail(src, dst, n_vec, first, blockIdx.x, gridDim.x);
  // under one vector, in 2-byte units
  if (blockIdx.x == 0) {
    const size_t done = n_vec * sizeof(u32x4);
    const size_t units = (bytes - done) / sizeof(uint16_t);
    if (threadIdx.x < units) {
      const uint16_t* s = reinterpret_cast<const uint16_t*>(static_cast<const char*>(src_) + done);
      uint16_t* d = reinterpret_cast<uint16_t*>(static_cast<char*>(dst_) + done);
      d[threadIdx.x] = s[threadIdx.x];
    }
  }
}

// Blocks for a message of `bytes`: one per tile (the last one partial), at most `max_blocks`.
inline unsigned self_copy_grid(size_t bytes, int max_blocks) {
  const size_t tiles = (bytes + kSelfCopyTileBytes - 1) / kSelfCopyTileBytes;
  return (unsigned)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)max_blocks));
}

}  // namespace gtk
