// HIP/CDNA4 link-cost probe kernels (gfx950) + pybind11 bindings.
//
// Reference: design.md:23-59 obtains the GPU-pair link class from NVML and leaves the bandwidth
// weight as a TODO (design.md:47).  On MI355X every GPU pair is a direct xGMI link, so the link
// class alone cannot rank placements; instead the device plugin measures the real link-cost matrix
// at node start with the kernels below:
//   K1 p2p read  : kernel on the reader GPU pulls a peer buffer over xGMI, staged through LDS by
//                  LDS-DMA (global_load_lds_dwordx4) and stored to local HBM.
//   K2 p2p write : kernel on the source GPU pushes local HBM into the peer buffer.
//   K3 hbm copy  : self pair (k=1 baseline), same kernel with both pointers local.
//   K4 mfma warm : v_mfma_f32_32x32x16_bf16 loop to lift clocks before timing, also reporting the
//                  achieved dense bf16 rate.
//   K5 gather    : one kernel on the reader pulls from all of its peers at once -> aggregate xGMI
//                  ingress per GPU with every other GPU idle.
//   K6 ring      : every member of a subset runs the K5 gather from its peers at the same time
//                  (ingress and egress of every GPU loaded together, as under a ring all-reduce):
//                  the slowest member's ingress is the bound a ring all-reduce's busBW is measured
//                  against.
//   K7 allreduce : the sum of every member's buffer, in every member's output, by kernels over peer
//                  pointers (peer_allreduce.h, peer_driver.h): a fixed summation order, so it is exact
//                  against a CPU sum; the repository's own collective, next to RCCL's.  On the fp8 wire
//                  (peer_q8.h) every member packs its input into block-scaled e4m3 first and the members
//                  read that, 33 bytes per 32 elements, with the same fixed order and exactness; on the
//                  fp8x2 wire a two-shot packs its sums again and gathers the packed form too; the push
//                  algorithm stores each member's slice of the sum into every member's out in one launch.  PeerRank
//                  (peer_rank.h) launches the same kernels for one rank of the peer communicator.
//   K8 latency   : one wave follows a chain of dependent loads through a buffer of another device
//                  (chase_latency.h): nanoseconds per access over the link, next to K1's GB/s.
//   IPC read     : the K1 kernel on a buffer another process exported with hipIpcGetMemHandle (the
//                  mapping RCCL's P2P transport gives a rank of its peers' buffers).
// The copy kernel exists in two staging forms (LDS-DMA and plain register staging) so the
// rocprofv3 counter profile can show what LDS staging costs/buys on a pure stream (profiles/).
//
// Geometry (CDNA4): 256-thread blocks (4 wave64), each wave moves 64 lanes x 16 B = 1 KiB per
// instruction; UNROLL=4 instructions in flight per lane -> 16 KiB LDS image per block, so up to
// 8 blocks (32 waves, the CU maximum) are resident per CU inside the 160 KiB LDS.  Grid = CUs x 8
// with a grid-stride loop: >>256 workgroups fills all 8 XCDs; a streaming copy has no reuse so no
// XCD remap is needed (each byte is touched once).
// This file is the one translation unit of _probe; every header includes what it needs.
#include "chase_latency.h"   // K8 kernels and the chain's closed form
#include "peer_allreduce.h"  // K7 kernels
#include "peer_driver.h"     // K7 launch plan, PeerAllreduce and its entry points
#include "peer_q8.h"         // K7 fp8 wire: block-scaled e4m3 quantize, sum, repack and unpack kernels
#include "peer_rank.h"       // one rank of the peer communicator's device backend
#include "peer_zero1.h"      // K7 ZeRO-1 step: the push reduce with the AdamW update as its epilogue
#include "probe_common.h"    // geometry, SrcSet, pattern fill and verifier, guards, grids, timers

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

using gptr_t = const __attribute__((address_space(1))) void*;
using lptr_t = __attribute__((address_space(3))) void*;

// ---------------------------------------------------------------------------------------------
// K1/K2/K3: LDS-DMA staged copy.  Each wave issues kUnroll global_load_lds_dwordx4 into its own
// 1 KiB LDS slices (wave-uniform base + lane*16: the DMA's lane-linear rule), drains vmcnt, then
// each lane stores back the 16 B its own lane fetched, so no cross-wave barrier is needed.
// `blk`/`nblk` let one launch split its grid over several streams (K5 gather below).
template <bool kNonTemporal>
__device__ __forceinline__ void copy_lds_stream(const u32x4* __restrict__ src, u32x4* __restrict__ dst, size_t n_vec,
                                                u32x4* lds, size_t blk, size_t nblk) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const size_t n_full = (n_vec / kTileVec) * kTileVec;
  for (size_t base = blk * kTileVec; base < n_full; base += nblk * kTileVec) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const size_t off = base + (size_t)u * kBlock + wave * 64;
      __builtin_amdgcn_global_load_lds((gptr_t)(src + off + lane), (lptr_t)(lds + u * kBlock + wave * 64), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const size_t off = base + (size_t)u * kBlock + wave * 64 + lane;
      u32x4 v = lds[u * kBlock + wave * 64 + lane];
      if (kNonTemporal)
        __builtin_nontemporal_store(v, dst + off);
      else
        dst[off] = v;
    }
  }
  gtk::stream_vec_tail(src, dst, n_vec, n_full, blk, nblk);
}

template <bool kNonTemporal>
__global__ __launch_bounds__(kBlock) void copy_lds_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst,
                                                          size_t n_vec) {
  __shared__ u32x4 lds[kTileVec];
  copy_lds_stream<kNonTemporal>(src, dst, n_vec, lds, blockIdx.x, gridDim.x);
}

// K5 gather: one launch on the reader pulls from up to kMaxSrc peers at once (ingress over all of
// its xGMI links together).  Block b serves source b % nsrc, so every source gets gridDim/nsrc
// blocks spread over all XCDs; source s lands in dst[s * n_vec ...].
__global__ __launch_bounds__(kBlock) void gather_lds_kernel(SrcSet srcs, int nsrc, u32x4* __restrict__ dst,
                                                            size_t n_vec) {
  __shared__ u32x4 lds[kTileVec];
  const int s = blockIdx.x % nsrc;
  copy_lds_stream<true>(srcs.p[s], dst + (size_t)s * n_vec, n_vec, lds, blockIdx.x / nsrc, gridDim.x / nsrc);
}

// Register-staged variant of the same stream (kUnroll independent 16-B loads in flight per lane).
template <bool kNonTemporal>
__global__ __launch_bounds__(kBlock) void copy_reg_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst,
                                                          size_t n_vec) {
  const size_t n_full = (n_vec / kTileVec) * kTileVec;
  for (size_t base = (size_t)blockIdx.x * kTileVec; base < n_full; base += (size_t)gridDim.x * kTileVec) {
    u32x4 r[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) r[u] = src[base + (size_t)u * kBlock + threadIdx.x];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (kNonTemporal)
        __builtin_nontemporal_store(r[u], dst + base + (size_t)u * kBlock + threadIdx.x);
      else
        dst[base + (size_t)u * kBlock + threadIdx.x] = r[u];
    }
  }
  gtk::stream_vec_tail(src, dst, n_vec, n_full, blockIdx.x, gridDim.x);
}

// Contiguous-chunk variant: block b streams its own 1/grid slice of the buffer, U independent 16-B
// loads in flight per lane, non-temporal loads and stores (the body the one-rank all-reduce uses).
template <int U>
__global__ __launch_bounds__(kBlock) void copy_chunk_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst,
                                                            size_t n_vec) {
  const size_t first = gtk::stream_slices<U>(src, dst, n_vec, blockIdx.x, gridDim.x);
  gtk::stream_vec_tail(src, dst, n_vec, first, blockIdx.x, gridDim.x);
}

// K4: MFMA warm-up.  Each wave keeps 4 independent 32x32 accumulators so back-to-back
// v_mfma_f32_32x32x16_bf16 issue is not serialised on the dependent-accumulator latency.
__global__ __launch_bounds__(kBlock) void mfma_warmup_kernel(float* __restrict__ out, int iters) {
  bf16x8 a, b;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    a[i] = (__bf16)((threadIdx.x & 7) * 0.125f - 0.5f);
    b[i] = (__bf16)(i * 0.0625f - 0.25f);
  }
  f32x16 acc0 = {}, acc1 = {}, acc2 = {}, acc3 = {};
  for (int it = 0; it < iters; ++it) {
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc1, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc2, 0, 0, 0);
    acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc3, 0, 0, 0);
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += acc0[i] + acc1[i] + acc2[i] + acc3[i];
  out[(size_t)blockIdx.x * kBlock + threadIdx.x] = s;
}

// K4r: the same loop on random operands.  Eight distinct pseudo-random A and B fragments per lane
// (uniform in [-1, 1), from a hash of lane and index) are cycled, so consecutive MFMAs see new
// operand bits as a GEMM's do.  The bit toggling draws more power than K4's near-constant operands;
// the rate it reaches is the MFMA ceiling a GEMM or an attention kernel on real data can approach.
__device__ __forceinline__ __bf16 rand_bf16(unsigned int x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return (__bf16)((float)(x >> 8) * (1.0f / 8388608.0f) - 1.0f);
}

__global__ __launch_bounds__(kBlock) void mfma_warmup_random_kernel(float* __restrict__ out, int iters) {
  bf16x8 a[8], b[8];
  const unsigned int seed = (blockIdx.x * kBlock + threadIdx.x) * 131u;
#pragma unroll
  for (int f = 0; f < 8; ++f)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      a[f][i] = rand_bf16(seed + 16u * f + i);
      b[f][i] = rand_bf16(~(seed + 16u * f + i));
    }
  f32x16 acc0 = {}, acc1 = {}, acc2 = {}, acc3 = {};
  for (int it = 0; it < iters; it += 2) {
#pragma unroll
    for (int f = 0; f < 8; f += 4) {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[f], b[f + 1], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[f + 1], b[f + 2], acc1, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[f + 2], b[f + 3], acc2, 0, 0, 0);
      acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[f + 3], b[f], acc3, 0, 0, 0);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += acc0[i] + acc1[i] + acc2[i] + acc3[i];
  out[(size_t)blockIdx.x * kBlock + threadIdx.x] = s;
}

// Where a workgroup runs: its XCD (HW_REG_XCC_ID[3:0]) and the low half of HW_REG_HW_ID (wave, SIMD,
// CU, SH, SE).  Lane 0 writes one word per workgroup with an ordinary vector store.  Shows how a queue
// CU mask (HSA_CU_MASK, time-sliced shares in topology/shares.py) spreads over the 8 XCDs.
__global__ __launch_bounds__(64) void xcc_census_kernel(unsigned int* __restrict__ out) {
  const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xFu;  // hwreg(HW_REG_XCC_ID, 0, 4)
  const unsigned hw = __builtin_amdgcn_s_getreg((15 << 11) | 4);          // hwreg(HW_REG_HW_ID, 0, 16)
  if (threadIdx.x == 0) out[blockIdx.x] = (xcc << 16) | (hw & 0xFFFFu);
}

void launch_copy(const std::string& kind, bool nt, const void* src, void* dst, size_t n_vec, int grid, hipStream_t s) {
  auto* S = reinterpret_cast<const u32x4*>(src);
  auto* D = reinterpret_cast<u32x4*>(dst);
  if (kind == "lds") {
    if (nt)
      hipLaunchKernelGGL(copy_lds_kernel<true>, dim3(grid), dim3(kBlock), 0, s, S, D, n_vec);
    else
      hipLaunchKernelGGL(copy_lds_kernel<false>, dim3(grid), dim3(kBlock), 0, s, S, D, n_vec);
  } else if (kind == "reg") {
    if (nt)
      hipLaunchKernelGGL(copy_reg_kernel<true>, dim3(grid), dim3(kBlock), 0, s, S, D, n_vec);
    else
      hipLaunchKernelGGL(copy_reg_kernel<false>, dim3(grid), dim3(kBlock), 0, s, S, D, n_vec);
  } else if (kind == "chunk") {
    hipLaunchKernelGGL(copy_chunk_kernel<8>, dim3(grid), dim3(kBlock), 0, s, S, D, n_vec);
  } else if (kind == "chunk4") {
    hipLaunchKernelGGL(copy_chunk_kernel<4>, dim3(grid), dim3(kBlock), 0, s, S, D, n_vec);
  } else if (kind == "sdma") {
    HIP_CHECK(hipMemcpyAsync(dst, src, n_vec * 16, hipMemcpyDeviceToDevice, s));
    return;
  } else {
    throw std::invalid_argument("kind must be lds|reg|chunk|chunk4|sdma");
  }
  HIP_CHECK(hipGetLastError());
}

struct CopyResult {
  int src, dst, exec, iters, grid;
  size_t bytes;
  std::string kind;
  bool nontemporal, ok, dry_run;
  double ms_per_iter, gbps;
};

CopyResult copy_bw_impl(int src_dev, int dst_dev, int exec_dev, size_t bytes, int iters, int warmup,
                        const std::string& kind, bool nontemporal, int blocks_per_cu, bool dry_run = false) {
  check_bytes_iters(bytes, iters);
  if (exec_dev != src_dev && exec_dev != dst_dev) throw std::invalid_argument("exec_dev must be src or dst");
  check_devs({src_dev, dst_dev});
  if (src_dev != dst_dev) enable_peer(exec_dev, exec_dev == src_dev ? dst_dev : src_dev);

  DevBuf src(src_dev, bytes), dst(dst_dev, bytes);
  const size_t n_vec = bytes / 16;
  const unsigned int seed = 0x9e3779b9u ^ (unsigned)(src_dev * 131 + dst_dev);
  fill_pattern(src_dev, src.p, bytes, seed);
  poison_pattern(dst_dev, dst.p, bytes, seed);
  const int grid = num_cus(exec_dev) * std::max(1, blocks_per_cu);
  float ms = 0.f;
  {
    DeviceGuard g(exec_dev);
    ms = time_launches([&](hipStream_t s) {
      if (!dry_run) launch_copy(kind, nontemporal, src.p, dst.p, n_vec, grid, s);
    }, iters, warmup);
  }
  const bool ok = holds_pattern(dst_dev, dst.p, bytes / 4, seed);
  // gbps = bytes copied per second (one direction over the link; for a self copy HBM moves 2x)
  return CopyResult{src_dev, dst_dev, exec_dev, iters, grid, bytes, kind, nontemporal, ok, dry_run, (double)ms / iters,
                    gbps((double)bytes, ms, iters)};
}

// K5: aggregate ingress of `dst_dev` reading `bytes` from every device in `srcs` concurrently.
// A source equal to dst_dev is a local stream (one buffer per entry); on a node the sources are the
// peers.  Every source is seeded by its slot in `srcs`, not by its device, and segment i is checked
// against slot i's seed (`seeds` in the result): with a device repeated, the only form a 1-GPU box
// can run, a gather that read one source for every segment or swapped two segments still fails.
py::dict gather_bw(int dst_dev, const std::vector<int>& srcs, size_t bytes, int iters, int warmup, int blocks_per_cu,
                   bool dry_run) {
  if (srcs.empty() || srcs.size() > (size_t)kMaxSrc) throw std::invalid_argument("1..16 source devices");
  check_bytes_iters(bytes, iters);
  check_dev(dst_dev);
  check_devs(srcs);
  auto seed_of = [](int slot) { return 0x51ed27u ^ (unsigned)(slot * 977 + 1); };
  float ms = 0.f;
  bool ok = true;
  const int nsrc = (int)srcs.size();
  std::vector<unsigned int> seeds(nsrc);
  for (int i = 0; i < nsrc; ++i) seeds[i] = seed_of(i);
  {
    py::gil_scoped_release nogil;
    for (int d : srcs) enable_peer(dst_dev, d);
    std::vector<std::unique_ptr<DevBuf>> src_bufs;
    SrcSet set{};
    for (int i = 0; i < nsrc; ++i) {
      src_bufs.emplace_back(new DevBuf(srcs[i], bytes));
      fill_pattern(srcs[i], src_bufs.back()->p, bytes, seeds[i]);
      set.p[i] = reinterpret_cast<const u32x4*>(src_bufs.back()->p);
    }
    DevBuf dst(dst_dev, bytes * (size_t)nsrc);
    for (int i = 0; i < nsrc; ++i) poison_pattern(dst_dev, (char*)dst.p + (size_t)i * bytes, bytes, seeds[i]);
    DeviceGuard g(dst_dev);
    const int grid = gather_grid(dst_dev, blocks_per_cu, nsrc);
    ms = time_launches([&](hipStream_t s) {
      if (dry_run) return;
      hipLaunchKernelGGL(gather_lds_kernel, dim3(grid), dim3(kBlock), 0, s, set, nsrc, (u32x4*)dst.p, bytes / 16);
    }, iters, warmup);
    // every segment holds its source's pattern
    for (int i = 0; i < nsrc && ok; ++i)
      ok = holds_pattern(dst_dev, (const char*)dst.p + (size_t)i * bytes, bytes / 4, seeds[i]);
  }
  py::dict r;
  r["dst"] = dst_dev;
  r["srcs"] = srcs;
  r["seeds"] = seeds;
  r["bytes_per_src"] = bytes;
  put_rate(r, (double)bytes * nsrc, ms, iters);
  r["ok"] = ok;
  r["dry_run"] = dry_run;
  return r;
}

// K6 ring: every member of a subset gathers from its peers AT THE SAME TIME, so each GPU's xGMI
// ingress and egress are loaded together, as they are under a ring all-reduce (K1 loads one
// direction of one idle link; K5 loads one GPU's ingress with every other GPU idle).  Member m runs
// the K5 gather kernel on its own stream of devs[m], pulling the source buffer of every member in
// peers[m] into its own inbox; launches are interleaved across members so they overlap from the
// first iteration.  A member's rate is the bytes it received / its own stream time; the subset's
// ring bound is the slowest member (a ring all-reduce's busBW is every member's ingress rate, so
// the slowest one caps it).  Members may repeat a device: on one GPU that checks the indexing.
py::dict ring_bw(const std::vector<int>& devs, const std::vector<std::vector<int>>& peers, size_t bytes, int iters,
                 int warmup, int blocks_per_cu, bool dry_run) {
  const int k = (int)devs.size();
  if (k < 2 || k > kMaxSrc + 1) throw std::invalid_argument("2..17 ring members");
  if ((int)peers.size() != k) throw std::invalid_argument("one peer list per member");
  check_bytes_iters(bytes, iters);
  check_devs(devs);
  for (int m = 0; m < k; ++m) {
    if (peers[m].empty() || peers[m].size() > (size_t)kMaxSrc) throw std::invalid_argument("1..16 peers per member");
    for (int p : peers[m])
      if (p < 0 || p >= k || p == m) throw std::invalid_argument("peers are other members' indices");
  }
  auto seed_of = [](int m) { return 0x6a09e667u ^ (unsigned)(m * 7919 + 1); };
  MemberTimes t;
  bool ok = true;
  {
    py::gil_scoped_release nogil;
    for (int m = 0; m < k; ++m)
      for (int p : peers[m]) enable_peer(devs[m], devs[p]);
    std::vector<std::unique_ptr<DevBuf>> src, inbox;
    for (int m = 0; m < k; ++m) {
      src.emplace_back(new DevBuf(devs[m], bytes));
      inbox.emplace_back(new DevBuf(devs[m], bytes * peers[m].size()));
      fill_pattern(devs[m], src[m]->p, bytes, seed_of(m));
      for (size_t i = 0; i < peers[m].size(); ++i)
        poison_pattern(devs[m], (char*)inbox[m]->p + i * bytes, bytes, seed_of(peers[m][i]));
    }
    std::vector<SrcSet> sets(k);
    std::vector<int> grid(k);
    MemberStreams ts;
    for (int m = 0; m < k; ++m) {
      const int ns = (int)peers[m].size();
      for (int i = 0; i < ns; ++i) sets[m].p[i] = reinterpret_cast<const u32x4*>(src[peers[m][i]]->p);
      grid[m] = gather_grid(devs[m], blocks_per_cu, ns, device_share(devs, devs[m]));
      DeviceGuard g(devs[m]);
      ts.emplace_back(new TimedStream());
    }
    t = time_member_rounds(devs, ts, warmup, iters, [&](int) {
      for (int m = 0; m < k && !dry_run; ++m) {
        DeviceGuard g(devs[m]);
        hipLaunchKernelGGL(gather_lds_kernel, dim3(grid[m]), dim3(kBlock), 0, ts[m]->s, sets[m], (int)peers[m].size(),
                           (u32x4*)inbox[m]->p, bytes / 16);
        HIP_CHECK(hipGetLastError());
      }
    });
    ts.clear();
    // every inbox segment holds its peer's pattern
    for (int m = 0; m < k && ok; ++m)
      for (size_t i = 0; i < peers[m].size() && ok; ++i)
        ok = holds_pattern(devs[m], (const char*)inbox[m]->p + i * bytes, bytes / 4, seed_of(peers[m][i]));
  }
  py::dict r;
  std::vector<double> gbps(k);
  double bound = 0.0;
  for (int m = 0; m < k; ++m) {
    gbps[m] = (double)bytes * peers[m].size() * iters / (t.ms_member[m] / 1e3) / 1e9;
    bound = (m == 0) ? gbps[m] : std::min(bound, gbps[m]);
  }
  std::vector<unsigned int> seeds(k);
  for (int m = 0; m < k; ++m) seeds[m] = seed_of(m);
  r["devs"] = devs;
  r["peers"] = peers;
  r["seeds"] = seeds;
  r["bytes_per_peer"] = bytes;
  r["iters"] = iters;
  r["ms_member"] = t.ms_member;
  r["wall_ms"] = t.wall_ms;
  r["ingress_gbps"] = gbps;
  r["bound_gbps"] = bound;
  r["ok"] = ok;
  r["dry_run"] = dry_run;
  return r;
}

// K8 link latency: one wave on `exec_dev` follows a chain of dependent loads (chase_latency.h) that
// lives in the memory of the chain's device, the orientation of copy_bw in read mode: the number for
// (src, exec) sits where K1's GB/s for (src, dst) sits.  Time is taken inside the kernel (wall clock
// around the loop), so launch and completion overheads are outside it; the hipEvent time of the same
// launch is reported next to it.  Lane l starts (l * n) / chains hops from node 0, so lanes are spread
// evenly over the cycle, and launch j + 1 continues where launch j ended: no line is visited twice
// until hops x launches reaches n / chains.  After every launch the host compares every lane's
// position with the chain's closed form.
//   evict   : before the first launch a 512 MiB scratch buffer of the owning device is streamed with
//             fill_pattern, so the 256 MiB Infinity Cache does not hold freshly written chain lines.
//   !evict  : one untimed lap over all n nodes first (up to 64 lanes, each its own n / lanes stretch),
//             so that a small working set is resident before it is timed.
struct ChaseResult {
  std::vector<double> kernel_ns, event_ms;  // per timed launch
  std::vector<unsigned int> end;            // node index per lane after the last launch
  bool ok = true;
  int rate_khz = 0;
};

class ChaseChain {
 public:
  static constexpr size_t kMaxBytes = (size_t)4 << 30;
  static constexpr size_t kEvictBytes = (size_t)512 << 20;
  static constexpr int kMaxHops = 1 << 18, kMaxLaunches = 64;

  static void check_chain(size_t ws_bytes, size_t stride) {
    auto pow2 = [](size_t x) { return x != 0 && (x & (x - 1)) == 0; };
    if (!pow2(stride) || stride < 4) throw std::invalid_argument("stride: a power of two >= 4");
    if (!pow2(ws_bytes) || ws_bytes > kMaxBytes) throw std::invalid_argument("ws_bytes: a power of two <= 4 GiB");
    if (ws_bytes / stride < 2) throw std::invalid_argument("ws_bytes / stride: at least 2 nodes");
  }
  static void check_run(int hops, int chains, int iters, int warmup) {
    if (chains < 1 || chains > kChaseMaxChains) throw std::invalid_argument("1 <= chains <= 64");
    if (hops < 1 || hops > kMaxHops) throw std::invalid_argument("1 <= hops <= 2^18");
    if (warmup < 0 || iters + warmup > kMaxLaunches) throw std::invalid_argument("warmup >= 0, iters + warmup <= 64");
    check_bytes_iters(kEvictBytes, iters);
  }

  // Allocates the chain on `dev` and writes it there, once for every run() that follows.
  ChaseChain(int dev, size_t ws_bytes, size_t stride) : dev_(dev), ws_(ws_bytes), stride_(stride) {
    check_chain(ws_bytes, stride);
    check_dev(dev);
    n_ = ws_bytes / stride;
    while (((size_t)1 << log2_stride_) < stride) ++log2_stride_;
    py::gil_scoped_release nogil;
    buf_.reset(new DevBuf(dev, ws_bytes));
    DeviceGuard g(dev);
    const int grid = (int)std::min<size_t>((size_t)num_cus(dev) * 4, (n_ + kBlock - 1) / kBlock);
    chase_fill_kernel<<<dim3(grid), dim3(kBlock)>>>((unsigned char*)buf_->p, n_, log2_stride_);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
  }
  ChaseChain(const ChaseChain&) = delete;
  ChaseChain& operator=(const ChaseChain&) = delete;

  ChaseResult run(int exec_dev, int hops, int chains, int iters, int warmup, bool evict) {
    check_run(hops, chains, iters, warmup);
    check_dev(exec_dev);
    enable_peer(exec_dev, dev_);
    if (evict) {
      if (!scratch_) scratch_.reset(new DevBuf(dev_, kEvictBytes));
      fill_pattern(dev_, scratch_->p, kEvictBytes, 0xe71c7u);
    }
    ChaseResult r;
    DeviceGuard g(exec_dev);
    HIP_CHECK(hipDeviceGetAttribute(&r.rate_khz, hipDeviceAttributeWallClockRate, exec_dev));
    if (r.rate_khz <= 0) throw std::runtime_error("hipDeviceAttributeWallClockRate is not positive");
    DevBuf pos(exec_dev, kChaseMaxChains * sizeof(unsigned int)), ticks(exec_dev, sizeof(unsigned long long));
    TimedStream t;
    const unsigned int off_mask = (unsigned int)(n_ - 1) << log2_stride_;
    std::vector<unsigned int> host(kChaseMaxChains, 0u);
    // every lane's node index, to the device as byte offsets and back
    auto put = [&](const std::vector<unsigned int>& nodes) {
      for (size_t l = 0; l < nodes.size(); ++l) host[l] = nodes[l] << log2_stride_;
      HIP_CHECK(hipMemcpyAsync(pos.p, host.data(), host.size() * sizeof(unsigned int), hipMemcpyHostToDevice, t.s));
      HIP_CHECK(hipStreamSynchronize(t.s));
    };
    auto starts = [&](int lanes) {
      std::vector<unsigned int> s(lanes);
      for (int l = 0; l < lanes; ++l) s[l] = chain_skip(0u, (unsigned long long)l * n_ / lanes, n_);
      return s;
    };
    auto launch = [&](int lanes, int h) {
      chase_kernel<<<dim3(1), dim3(64), 0, t.s>>>((const unsigned char*)buf_->p, off_mask, (unsigned int*)pos.p, lanes, h,
                                                  (unsigned long long*)ticks.p);
      HIP_CHECK(hipGetLastError());
    };
    if (!evict) {
      const int lanes = (int)std::min<size_t>(kChaseMaxChains, n_);
      put(starts(lanes));
      for (size_t left = n_ / lanes; left;) {
        const int h = (int)std::min<size_t>(left, kMaxHops);
        launch(lanes, h);
        HIP_CHECK(hipStreamSynchronize(t.s));
        left -= h;
      }
    }
    std::vector<unsigned int> want = starts(chains);
    put(want);
    const ChainMap step = chain_power((unsigned long long)hops);
    for (int j = 0; j < warmup + iters; ++j) {
      t.begin();
      launch(chains, hops);
      const float ms = t.end_ms();
      unsigned long long tk = 0;
      HIP_CHECK(hipMemcpyAsync(&tk, ticks.p, sizeof(tk), hipMemcpyDeviceToHost, t.s));
      HIP_CHECK(hipMemcpyAsync(host.data(), pos.p, host.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, t.s));
      HIP_CHECK(hipStreamSynchronize(t.s));
      for (int l = 0; l < chains; ++l) {
        want[l] = step(want[l]) & (unsigned int)(n_ - 1);
        r.ok = r.ok && host[l] == (want[l] << log2_stride_);
      }
      if (j >= warmup) {
        r.kernel_ns.push_back((double)tk * 1e6 / r.rate_khz);
        r.event_ms.push_back((double)ms);
      }
    }
    r.end.resize(chains);
    for (int l = 0; l < chains; ++l) r.end[l] = host[l] >> log2_stride_;
    return r;
  }

  py::dict run_py(int exec_dev, int hops, int chains, int iters, int warmup, bool evict) {
    ChaseResult c;
    {
      py::gil_scoped_release nogil;
      c = run(exec_dev, hops, chains, iters, warmup, evict);
    }
    std::vector<double> per(c.kernel_ns);
    for (double& x : per) x /= hops;
    std::vector<double> sorted(per);
    std::sort(sorted.begin(), sorted.end());
    const size_t m = sorted.size();
    py::dict r;
    r["src"] = dev_;
    r["exec"] = exec_dev;
    r["ns_per_hop"] = m % 2 ? sorted[m / 2] : 0.5 * (sorted[m / 2 - 1] + sorted[m / 2]);
    r["ns_min"] = sorted.front();
    r["ns_max"] = sorted.back();
    r["ns_launches"] = per;
    r["kernel_ns"] = c.kernel_ns;
    r["event_ms"] = c.event_ms;
    r["end"] = c.end;
    r["ok"] = c.ok;
    r["n_nodes"] = n_;
    r["hops"] = hops;
    r["chains"] = chains;
    r["iters"] = iters;
    r["stride"] = stride_;
    r["ws_bytes"] = ws_;
    r["evicted"] = evict;
    r["clock_khz"] = c.rate_khz;
    return r;
  }

 private:
  int dev_;
  size_t ws_, stride_, n_ = 0;
  unsigned int log2_stride_ = 0;
  std::unique_ptr<DevBuf> buf_, scratch_;
};

py::dict chase_latency(int src_dev, int exec_dev, size_t ws_bytes, size_t stride, int hops, int chains, int iters, int warmup,
                       bool evict) {
  // every argument is checked before the chain is allocated or anything is launched
  ChaseChain::check_chain(ws_bytes, stride);
  ChaseChain::check_run(hops, chains, iters, warmup);
  check_devs({src_dev, exec_dev});
  ChaseChain chain(src_dev, ws_bytes, stride);
  return chain.run_py(exec_dev, hops, chains, iters, warmup, evict);
}

py::dict to_dict(const CopyResult& c) {
  py::dict r;
  r["src"] = c.src;
  r["dst"] = c.dst;
  r["exec"] = c.exec;
  r["bytes"] = c.bytes;
  r["iters"] = c.iters;
  r["kind"] = c.kind;
  r["nontemporal"] = c.nontemporal;
  r["grid"] = c.grid;
  r["ms_per_iter"] = c.ms_per_iter;
  r["gbps"] = c.gbps;
  r["ok"] = c.ok;
  r["dry_run"] = c.dry_run;
  return r;
}

py::dict copy_bw(int src_dev, int dst_dev, int exec_dev, size_t bytes, int iters, int warmup, const std::string& kind,
                 bool nontemporal, int blocks_per_cu, bool dry_run) {
  CopyResult c;
  {
    py::gil_scoped_release nogil;
    c = copy_bw_impl(src_dev, dst_dev, exec_dev, bytes, iters, warmup, kind, nontemporal, blocks_per_cu, dry_run);
  }
  return to_dict(c);
}

// On the null stream, which every other stream of the device waits for: lifts the whole device's clocks.
py::dict mfma_warmup(int dev, double target_ms, int iters_per_launch, bool random_operands) {
  py::gil_scoped_release nogil_outer;
  DeviceGuard g(dev);
  if (iters_per_launch < 2 || iters_per_launch % 2) throw std::invalid_argument("iters_per_launch: a positive even number");
  auto* kern = random_operands ? mfma_warmup_random_kernel : mfma_warmup_kernel;
  const int grid = num_cus(dev) * 4;  // 16 waves per CU = 4 per SIMD
  DevBuf out(dev, (size_t)grid * kBlock * sizeof(float));
  hipEvent_t e0, e1;
  for (hipEvent_t* e : {&e0, &e1}) HIP_CHECK(hipEventCreate(e));
  int launches = 0;
  float total_ms = 0.f;
  auto t0 = std::chrono::steady_clock::now();
  do {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, 0, (float*)out.p, iters_per_launch);
    HIP_CHECK(hipGetLastError());
    ++launches;
    HIP_CHECK(hipDeviceSynchronize());
    total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  } while (total_ms < target_ms && launches < 100000);
  // timed launch, clocks now lifted
  HIP_CHECK(hipEventRecord(e0, 0));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, 0, (float*)out.p, iters_per_launch);
  HIP_CHECK(hipEventRecord(e1, 0));
  HIP_CHECK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  HIP_CHECK(hipEventDestroy(e0));
  HIP_CHECK(hipEventDestroy(e1));
  const double flops = 2.0 * 32 * 32 * 16 * 4.0 * (double)iters_per_launch * (grid * (kBlock / 64));
  py::gil_scoped_acquire gil;
  py::dict r;
  r["device"] = dev;
  r["launches"] = launches;
  r["warm_ms"] = total_ms;
  r["timed_ms"] = ms;
  r["tflops"] = flops / (ms / 1e3) / 1e12;
  r["random_operands"] = random_operands;
  return r;
}

py::dict device_props(int dev) {
  hipDeviceProp_t p;
  HIP_CHECK(hipGetDeviceProperties(&p, dev));
  char bus[64] = {0};
  HIP_CHECK(hipDeviceGetPCIBusId(bus, sizeof(bus), dev));
  py::dict r;
  r["index"] = dev;
  r["name"] = std::string(p.name);
  r["gcn_arch"] = std::string(p.gcnArchName);
  r["cus"] = p.multiProcessorCount;
  r["total_mem"] = (size_t)p.totalGlobalMem;
  r["lds_per_block"] = (size_t)p.sharedMemPerBlock;
  r["clock_khz"] = p.clockRate;
  r["mem_clock_khz"] = p.memoryClockRate;
  r["mem_bus_width"] = p.memoryBusWidth;
  r["l2_bytes"] = p.l2CacheSize;
  r["pci_bus_id"] = std::string(bus);
  r["warp_size"] = p.warpSize;
  return r;
}

int device_count() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

bool can_access_peer(int a, int b) {
  if (a == b) return true;
  int can = 0;
  HIP_CHECK(hipDeviceCanAccessPeer(&can, a, b));
  return can != 0;
}

// Full ordered-pair matrix: entry [i][j] = GB/s of moving data from device i to device j.
// "read" executes on j (pull over the link), "write" on i (push).  Diagonal = local HBM copy.
std::vector<std::vector<double>> probe_matrix(const std::vector<int>& devs, size_t bytes, int iters, int warmup,
                                              const std::string& mode, const std::string& kind, bool nontemporal,
                                              int blocks_per_cu) {
  const size_t n = devs.size();
  std::vector<std::vector<double>> m(n, std::vector<double>(n, 0.0));
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j) {
      int s = devs[i], d = devs[j];
      int ex = (mode == "write") ? s : d;
      CopyResult r = copy_bw_impl(s, d, ex, bytes, iters, warmup, kind, nontemporal, blocks_per_cu);
      if (!r.ok)
        throw std::runtime_error("probe copy verification failed for pair " + std::to_string(s) + "->" + std::to_string(d));
      m[i][j] = r.gbps;
    }
  return m;
}

// XCDs the workgroups of one census launch ran on (on the null stream: the process's own CU mask,
// e.g. HSA_CU_MASK), as {xcc: workgroups}.
py::dict xcc_census(int dev, int blocks) {
  std::vector<unsigned int> host(blocks);
  {
    py::gil_scoped_release nogil;
    DeviceGuard g(dev);
    DevBuf out(dev, (size_t)blocks * sizeof(unsigned int));
    hipLaunchKernelGGL(xcc_census_kernel, dim3(blocks), dim3(64), 0, 0, (unsigned int*)out.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(host.data(), out.p, (size_t)blocks * sizeof(unsigned int), hipMemcpyDeviceToHost));
  }
  py::dict r;
  for (unsigned int w : host) {
    py::int_ k((int)(w >> 16));
    r[k] = (r.contains(k) ? r[k].cast<int>() : 0) + 1;
  }
  return r;
}

// ---------------------------------------------------------------------------------------------
// Cross-process reads through HIP IPC: the mapping RCCL's P2P transport gives a rank of its peers'
// buffers (hipIpcGetMemHandle in the owner, hipIpcOpenMemHandle in the reader).  One process
// exports a patterned buffer; another opens the handle and streams it into a buffer of its own with
// the K1 LDS-DMA kernel, then verifies the pattern.  On one GPU both sides share the device, which
// runs the IPC export / import path (the HSA_ENABLE_IPC_MODE_LEGACY=0 dma-buf handles) and the
// kernel on an imported mapping; on a node the reader is a peer GPU.
class IpcBuffer {
 public:
  IpcBuffer(int dev, size_t bytes, unsigned int seed) : buf_(dev, bytes), seed_(seed) {
    check_bytes_iters(bytes);
    fill_pattern(dev, buf_.p, bytes, seed);
    DeviceGuard g(dev);
    HIP_CHECK(hipIpcGetMemHandle(&h_, buf_.p));
  }
  py::bytes handle() const { return py::bytes(reinterpret_cast<const char*>(&h_), sizeof(h_)); }
  size_t bytes() const { return buf_.bytes; }
  unsigned int seed() const { return seed_; }
  // After a peer wrote into this buffer through its mapping (K2 over IPC): does it hold pattern(seed)?
  bool holds(unsigned int seed) const {
    py::gil_scoped_release nogil;
    return holds_pattern(buf_.dev, buf_.p, buf_.bytes / 4, seed);
  }
  // The count holds() compares with 0: words that differ from pattern(seed).
  unsigned long long mismatches(unsigned int seed) const {
    py::gil_scoped_release nogil;
    return pattern_mismatches(buf_.dev, buf_.p, buf_.bytes / 4, seed);
  }
  // One word of the buffer overwritten from the host (tests of the verifier: a single wrong word is counted).
  void poke(size_t word_index, unsigned int value) {
    if (word_index >= buf_.bytes / 4) throw std::out_of_range("poke: word index outside the buffer");
    DeviceGuard g(buf_.dev);
    HIP_CHECK(hipMemcpy((unsigned int*)buf_.p + word_index, &value, sizeof(value), hipMemcpyHostToDevice));
  }

 private:
  DevBuf buf_;
  unsigned int seed_;
  hipIpcMemHandle_t h_{};
};

// Opens another process's buffers by handle for the lifetime of the object.
struct IpcMappings {
  std::vector<void*> p;
  IpcMappings(const std::vector<py::bytes>& handles, int dev) {
    DeviceGuard g(dev);
    for (const py::bytes& hb : handles) {
      const std::string raw = hb;
      if (raw.size() != sizeof(hipIpcMemHandle_t)) throw std::invalid_argument("not a hipIpcMemHandle_t");
      hipIpcMemHandle_t h;
      std::memcpy(&h, raw.data(), sizeof(h));
      void* q = nullptr;
      HIP_CHECK(hipIpcOpenMemHandle(&q, h, hipIpcMemLazyEnablePeerAccess));
      p.push_back(q);
    }
  }
  ~IpcMappings() {
    for (void* q : p) (void)hipIpcCloseMemHandle(q);
  }
  IpcMappings(const IpcMappings&) = delete;
  IpcMappings& operator=(const IpcMappings&) = delete;
};

// One imported buffer and one local buffer of `dev`, the K1 LDS-DMA kernel between them.
//   write (K2 over IPC): the kernel pushes a local patterned buffer into another process's buffer
//     through the imported mapping (remote stores, the direction RCCL's P2P write protocol uses).  The
//     owner checks the result (IpcBuffer.holds), since only it knows the write has landed in its memory;
//     the destination holds the owner's own pattern, so the caller pushes another seed (`gtk ipc` does).
//   read: the imported buffer is streamed into the local one, which is then verified against `seed`.
py::dict ipc_copy_bw(bool write, const py::bytes& handle, int dev, size_t bytes, unsigned int seed, int iters, int warmup,
                     int blocks_per_cu) {
  check_bytes_iters(bytes, iters);
  IpcMappings map({handle}, dev);
  float ms = 0.f;
  bool ok = true;
  {
    py::gil_scoped_release nogil;
    DeviceGuard g(dev);
    DevBuf local(dev, bytes);
    if (write)
      fill_pattern(dev, local.p, bytes, seed);
    else
      poison_pattern(dev, local.p, bytes, seed);
    const void* src = write ? local.p : map.p[0];
    void* dst = write ? map.p[0] : local.p;
    const int grid = num_cus(dev) * std::max(1, blocks_per_cu);
    ms = time_launches([&](hipStream_t s) { launch_copy("lds", true, src, dst, bytes / 16, grid, s); }, iters, warmup);
    if (!write) ok = holds_pattern(dev, local.p, bytes / 4, seed);
  }
  py::dict d;
  d["dev"] = dev;
  d["bytes"] = bytes;
  put_rate(d, (double)bytes, ms, iters);
  if (!write) d["ok"] = ok;
  return d;
}

py::dict ipc_write_bw(const py::bytes& handle, int dev, size_t bytes, unsigned int seed, int iters, int warmup,
                      int blocks_per_cu) {
  return ipc_copy_bw(true, handle, dev, bytes, seed, iters, warmup, blocks_per_cu);
}

py::dict ipc_read_bw(const py::bytes& handle, int dev, size_t bytes, unsigned int seed, int iters, int warmup,
                     int blocks_per_cu) {
  return ipc_copy_bw(false, handle, dev, bytes, seed, iters, warmup, blocks_per_cu);
}

// K5 over IPC: one gather launch pulls every imported buffer at once (segment i of the inbox from
// handle i, as a rank's ingress from all of its peers); each segment is verified against seeds[i].
py::dict ipc_gather_bw(const std::vector<py::bytes>& handles, int dev, size_t bytes, const std::vector<unsigned int>& seeds,
                       int iters, int warmup, int blocks_per_cu) {
  const int nsrc = (int)handles.size();
  if (nsrc < 1 || nsrc > kMaxSrc) throw std::invalid_argument("1..16 handles");
  if (seeds.size() != handles.size()) throw std::invalid_argument("one seed per handle");
  check_bytes_iters(bytes, iters);
  IpcMappings map(handles, dev);
  float ms = 0.f;
  bool ok = true;
  {
    py::gil_scoped_release nogil;
    DeviceGuard g(dev);
    SrcSet set{};
    for (int i = 0; i < nsrc; ++i) set.p[i] = reinterpret_cast<const u32x4*>(map.p[i]);
    DevBuf inbox(dev, bytes * (size_t)nsrc);
    for (int i = 0; i < nsrc; ++i) poison_pattern(dev, (char*)inbox.p + (size_t)i * bytes, bytes, seeds[i]);
    const int grid = gather_grid(dev, blocks_per_cu, nsrc);
    ms = time_launches([&](hipStream_t s) {
      hipLaunchKernelGGL(gather_lds_kernel, dim3(grid), dim3(kBlock), 0, s, set, nsrc, (u32x4*)inbox.p, bytes / 16);
    }, iters, warmup);
    for (int i = 0; i < nsrc && ok; ++i)
      ok = holds_pattern(dev, (const char*)inbox.p + (size_t)i * bytes, bytes / 4, seeds[i]);
  }
  py::dict d;
  d["dev"] = dev;
  d["segments"] = nsrc;
  d["bytes_per_segment"] = bytes;
  put_rate(d, (double)bytes * nsrc, ms, iters);
  d["ok"] = ok;
  return d;
}

}  // namespace

PYBIND11_MODULE(_probe, m) {
  m.doc() = "HIP/CDNA4 (gfx950) link probe kernels: LDS-DMA staged p2p/HBM copy, MFMA warm-up";
  m.def("device_count", &device_count);
  m.def("device_props", &device_props, py::arg("dev"));
  m.def("can_access_peer", &can_access_peer, py::arg("a"), py::arg("b"));
  m.def("copy_bw", &copy_bw, py::arg("src_dev"), py::arg("dst_dev"), py::arg("exec_dev"), py::arg("bytes"),
        py::arg("iters") = 10, py::arg("warmup") = 2, py::arg("kind") = "lds", py::arg("nontemporal") = false,
        py::arg("blocks_per_cu") = kBlocksPerCU, py::arg("dry_run") = false,
        "K1/K2/K3; dry_run (tests only): everything but the copy launches, so ok says what the check makes of an idle kernel");
  m.def("gather_bw", &gather_bw, py::arg("dst_dev"), py::arg("srcs"), py::arg("bytes") = (size_t)64 << 20,
        py::arg("iters") = 3, py::arg("warmup") = 1, py::arg("blocks_per_cu") = kBlocksPerCU, py::arg("dry_run") = false);
  m.def("ring_bw", &ring_bw, py::arg("devs"), py::arg("peers"), py::arg("bytes") = (size_t)64 << 20, py::arg("iters") = 3,
        py::arg("warmup") = 1, py::arg("blocks_per_cu") = kBlocksPerCU, py::arg("dry_run") = false);
  m.def("peer_allreduce", &peer_allreduce, py::arg("devs"), py::arg("count"), py::arg("dtype") = "bf16",
        py::arg("algo") = "twoshot", py::arg("iters") = 3, py::arg("warmup") = 1, py::arg("blocks_per_cu") = kBlocksPerCU,
        py::arg("wire") = "native", py::arg("dry_run") = false,
        "K7: timed all-reduce (sum) of device-made inputs over peer pointers; every member's result checked; "
        "wire=\"fp8\": members read each other's block-scaled e4m3 form (peer_q8.h); wire=\"fp8x2\" (twoshot): the "
        "gather phase reads packed sums too; algo=\"push\": one launch per member stores its slice of the sum into every "
        "member's out (native and fp8 wires); dry_run (tests only): everything but the kernels of the rounds");
  m.def("peer_allreduce_arrays", &peer_allreduce_arrays, py::arg("devs"), py::arg("inputs"), py::arg("dtype") = "bf16",
        py::arg("algo") = "twoshot", py::arg("rounds") = 1, py::arg("out_dtype") = py::none(), py::arg("scale") = 1.0f,
        py::arg("wire") = "native",
        "K7 on the caller's arrays (uint16 bit patterns for bf16, float32 for fp32): the k members' results, "
        "scale x sum, in out_dtype (none: dtype; fp32 of bf16 inputs is the wide reduce)");
  m.def("peer_q8_quantize", &peer_q8_quantize, py::arg("dev"), py::arg("array"), py::arg("dtype") = "bf16",
        py::arg("count") = py::none(), py::arg("residual") = py::none(),
        "the fp8 wire's quantize kernel on one array: (codes uint8, block exponents int32) in logical order; "
        "count (none: all): the elements that are data, the rest lies in the window after them; residual (float32, "
        "one value per element of the count's whole blocks): the feedback form, and the new residual as a third array");
  m.def("peer_reduce_grid", &peer_reduce_grid, py::arg("cus"), py::arg("blocks_per_cu"), py::arg("share"), py::arg("n_vec"),
        "blocks of a K7 reduce or quantize of n_vec vectors on a device of `cus` CUs that `share` members split");
  bind_peer_rank(m);
  m.def("chase_latency", &chase_latency, py::arg("src_dev"), py::arg("exec_dev"), py::arg("ws_bytes") = (size_t)1 << 30,
        py::arg("stride") = (size_t)128, py::arg("hops") = 4096, py::arg("chains") = 1, py::arg("iters") = 5,
        py::arg("warmup") = 1, py::arg("evict") = true,
        "K8: ns per dependent load of exec_dev through a chain in src_dev's memory; every launch's end is checked");
  py::class_<ChaseChain>(m, "ChaseChain", "K8: a chain written once on its device, for run() from several devices")
      .def(py::init<int, size_t, size_t>(), py::arg("dev"), py::arg("ws_bytes") = (size_t)1 << 30, py::arg("stride") = (size_t)128)
      .def("run", &ChaseChain::run_py, py::arg("exec_dev"), py::arg("hops") = 4096, py::arg("chains") = 1, py::arg("iters") = 5,
           py::arg("warmup") = 1, py::arg("evict") = true);
  m.def("mfma_warmup", &mfma_warmup, py::arg("dev"), py::arg("target_ms") = 50.0, py::arg("iters_per_launch") = 4096,
        py::arg("random_operands") = false);
  m.def("probe_matrix", &probe_matrix, py::arg("devs"), py::arg("bytes") = (size_t)256 << 20, py::arg("iters") = 5,
        py::arg("warmup") = 1, py::arg("mode") = "read", py::arg("kind") = "lds", py::arg("nontemporal") = false,
        py::arg("blocks_per_cu") = kBlocksPerCU, py::call_guard<py::gil_scoped_release>());
  m.def("xcc_census", &xcc_census, py::arg("dev"), py::arg("blocks") = 4096);
  py::class_<IpcBuffer>(m, "IpcBuffer")
      .def(py::init<int, size_t, unsigned int>(), py::arg("dev"), py::arg("bytes"), py::arg("seed") = 0x5eedu)
      .def("handle", &IpcBuffer::handle)
      .def("holds", &IpcBuffer::holds, py::arg("seed"), "does the buffer hold pattern(seed)? (after a peer's IPC write)")
      .def("mismatches", &IpcBuffer::mismatches, py::arg("seed"), "words that differ from pattern(seed)")
      .def("poke", &IpcBuffer::poke, py::arg("word_index"), py::arg("value"), "overwrite one 32-bit word")
      .def_property_readonly("bytes", &IpcBuffer::bytes)
      .def_property_readonly("seed", &IpcBuffer::seed);
  m.def("ipc_write_bw", &ipc_write_bw, py::arg("handle"), py::arg("dev"), py::arg("bytes"), py::arg("seed"),
        py::arg("iters") = 5, py::arg("warmup") = 1, py::arg("blocks_per_cu") = kBlocksPerCU,
        "K2 over IPC: push pattern(seed) into another process's buffer through its handle (owner verifies)");
  m.def("ipc_gather_bw", &ipc_gather_bw, py::arg("handles"), py::arg("dev"), py::arg("bytes"), py::arg("seeds"),
        py::arg("iters") = 5, py::arg("warmup") = 1, py::arg("blocks_per_cu") = kBlocksPerCU,
        "K5 over IPC: one gather launch over every imported buffer; each segment verified");
  m.def("ipc_read_bw", &ipc_read_bw, py::arg("handle"), py::arg("dev"), py::arg("bytes"), py::arg("seed"),
        py::arg("iters") = 5, py::arg("warmup") = 1, py::arg("blocks_per_cu") = kBlocksPerCU,
        "open another process's buffer by its IPC handle and stream it into a local one (K1 kernel); verified");
  m.attr("BLOCK") = kBlock;
  m.attr("UNROLL") = kUnroll;
  m.attr("BLOCKS_PER_CU") = kBlocksPerCU;
}
