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
//                  pointers (peer_allreduce.h): a fixed summation order, so the result is exact
//                  against a CPU sum; the repository's own collective, next to RCCL's.  PeerRank
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
#include <hip/hip_runtime.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../common/stream_copy.h"

namespace py = pybind11;

using gtk::u32x4;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define HIP_CHECK(expr)                                                                          \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess)                                                                        \
      throw std::runtime_error(std::string(#expr " failed: ") + hipGetErrorString(_e) + " at " + \
                               __FILE__ + ":" + std::to_string(__LINE__));                       \
  } while (0)

namespace {

// Equal to the all-reduce's kSelfCopy* (csrc/rccl/self_copy.h) today, but tuned on their own (these
// on the LDS budget above, those on the 2 GiB headline): kept separate on purpose.
constexpr int kBlock = 256;
constexpr int kUnroll = 4;
constexpr int kTileVec = kBlock * kUnroll;  // 16-byte vectors per block-iteration (16 KiB)
constexpr int kBlocksPerCU = 8;
static_assert(kBlock == gtk::kStreamBlock, "stream_copy.h indexes blocks of kStreamBlock threads");

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
constexpr int kMaxSrc = 16;
struct SrcSet {
  const u32x4* p[kMaxSrc];
};

__global__ __launch_bounds__(kBlock) void gather_lds_kernel(SrcSet srcs, int nsrc, u32x4* __restrict__ dst,
                                                            size_t n_vec) {
  __shared__ u32x4 lds[kTileVec];
  const int s = blockIdx.x % nsrc;
  copy_lds_stream<true>(srcs.p[s], dst + (size_t)s * n_vec, n_vec, lds, blockIdx.x / nsrc, gridDim.x / nsrc);
}

}  // namespace
#include "peer_allreduce.h"  // K7 kernels, over SrcSet / kMaxSrc above
#include "chase_latency.h"   // K8 kernels and the chain's closed form
namespace {

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

__global__ __launch_bounds__(kBlock) void fill_pattern_kernel(unsigned int* __restrict__ p, size_t n_words,
                                                              unsigned int seed) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_words; i += (size_t)gridDim.x * kBlock)
    p[i] = (unsigned int)(i * 2654435761u) ^ seed;
}

// Counts the words of p[0, n_words) that differ from what fill_pattern_kernel(seed) writes.
__global__ __launch_bounds__(kBlock) void pattern_mismatch_kernel(const unsigned int* __restrict__ p, size_t n_words,
                                                                  unsigned int seed, unsigned long long* bad) {
  unsigned long long local = 0;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_words; i += (size_t)gridDim.x * kBlock)
    local += (p[i] != ((unsigned int)(i * 2654435761u) ^ seed));
  if (local) atomicAdd(bad, local);
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

// ---------------------------------------------------------------------------------------------
struct DeviceGuard {
  int prev = 0;
  explicit DeviceGuard(int dev) {
    HIP_CHECK(hipGetDevice(&prev));
    HIP_CHECK(hipSetDevice(dev));
  }
  ~DeviceGuard() { (void)hipSetDevice(prev); }
};

struct DevBuf {
  void* p = nullptr;
  int dev = -1;
  size_t bytes = 0;
  DevBuf(int d, size_t b) : dev(d), bytes(b) {
    DeviceGuard g(d);
    HIP_CHECK(hipMalloc(&p, b));
  }
  ~DevBuf() {
    if (p) {
      int prev = 0;
      (void)hipGetDevice(&prev);
      (void)hipSetDevice(dev);
      (void)hipFree(p);
      (void)hipSetDevice(prev);
    }
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};

int num_cus(int dev) {
  int cus = 0;
  HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  return std::max(cus, 1);
}

void enable_peer(int from, int to) {
  if (from == to) return;
  int can = 0;
  HIP_CHECK(hipDeviceCanAccessPeer(&can, from, to));
  if (!can) throw std::runtime_error("device " + std::to_string(from) + " cannot access peer " + std::to_string(to));
  DeviceGuard g(from);
  hipError_t e = hipDeviceEnablePeerAccess(to, 0);
  if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
    throw std::runtime_error(std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
  (void)hipGetLastError();
}

void check_bytes_iters(size_t bytes, int iters = 1) {
  if (bytes < 16 || bytes % 16) throw std::invalid_argument("bytes must be a positive multiple of 16");
  if (iters < 1) throw std::invalid_argument("iters >= 1");
}

// Blocks of a gather launch on `dev`: a multiple of nsrc, so every source gets the same block count.
// Members of a ring that share a device (`share` of them) split its CUs.
int gather_grid(int dev, int blocks_per_cu, int nsrc, int share = 1) {
  const int per = std::max(1, num_cus(dev) * std::max(1, blocks_per_cu) / (nsrc * share));
  return per * nsrc;
}

// GB/s of `bytes` moved per iteration, `iters` iterations in `ms`.
double gbps(double bytes, double ms, int iters) { return bytes / (ms / 1e3 / iters) / 1e9; }

// A non-blocking stream of the current device with the two events that bracket a timed section.
struct TimedStream {
  int dev = 0;
  hipStream_t s = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  TimedStream() {
    try {
      HIP_CHECK(hipGetDevice(&dev));
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      for (hipEvent_t* e : {&e0, &e1}) HIP_CHECK(hipEventCreate(e));
    } catch (...) {
      release();
      throw;
    }
  }
  ~TimedStream() { release(); }
  TimedStream(const TimedStream&) = delete;
  TimedStream& operator=(const TimedStream&) = delete;
  void begin() { HIP_CHECK(hipEventRecord(e0, s)); }
  void end() { HIP_CHECK(hipEventRecord(e1, s)); }
  float ms() {  // of begin() .. end(), once the stream has reached end()
    float t = 0.f;
    HIP_CHECK(hipEventSynchronize(e1));
    HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
    return t;
  }
  float end_ms() {
    end();
    return ms();
  }

 private:
  void release() noexcept {
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(dev);
    if (s) (void)hipStreamSynchronize(s);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (s) (void)hipStreamDestroy(s);
    (void)hipSetDevice(prev);
  }
};

// Event-timed `iters` launches of `launch` on a fresh non-blocking stream (after `warmup` untimed).
template <class F>
float time_launches(F launch, int iters, int warmup) {
  TimedStream t;
  for (int i = 0; i < warmup; ++i) launch(t.s);
  HIP_CHECK(hipGetLastError());
  t.begin();
  for (int i = 0; i < iters; ++i) launch(t.s);
  HIP_CHECK(hipGetLastError());
  return t.end_ms();
}

void fill_pattern(int dev, void* p, size_t bytes, unsigned int seed) {
  DeviceGuard g(dev);
  hipLaunchKernelGGL(fill_pattern_kernel, dim3(num_cus(dev) * 4), dim3(kBlock), 0, 0, (unsigned int*)p, bytes / 4, seed);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
}

// Does p[0, n_words), memory of `dev`, hold pattern(seed) in every word?  One pass on the device.
bool holds_pattern(int dev, const void* p, size_t n_words, unsigned int seed) {
  DeviceGuard g(dev);
  DevBuf bad(dev, sizeof(unsigned long long));
  HIP_CHECK(hipMemset(bad.p, 0, sizeof(unsigned long long)));
  hipLaunchKernelGGL(pattern_mismatch_kernel, dim3(num_cus(dev) * kBlocksPerCU), dim3(kBlock), 0, 0,
                     (const unsigned int*)p, n_words, seed, (unsigned long long*)bad.p);
  HIP_CHECK(hipGetLastError());
  unsigned long long n = 0;
  HIP_CHECK(hipMemcpy(&n, bad.p, sizeof(n), hipMemcpyDeviceToHost));
  return n == 0;
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
  bool nontemporal, ok;
  double ms_per_iter, gbps;
};

CopyResult copy_bw_impl(int src_dev, int dst_dev, int exec_dev, size_t bytes, int iters, int warmup,
                        const std::string& kind, bool nontemporal, int blocks_per_cu) {
  check_bytes_iters(bytes, iters);
  if (exec_dev != src_dev && exec_dev != dst_dev) throw std::invalid_argument("exec_dev must be src or dst");
  int ndev = 0;
  HIP_CHECK(hipGetDeviceCount(&ndev));
  for (int d : {src_dev, dst_dev})
    if (d < 0 || d >= ndev) throw std::invalid_argument("device index out of range");
  if (src_dev != dst_dev) enable_peer(exec_dev, exec_dev == src_dev ? dst_dev : src_dev);

  DevBuf src(src_dev, bytes), dst(dst_dev, bytes);
  const size_t n_vec = bytes / 16;
  const unsigned int seed = 0x9e3779b9u ^ (unsigned)(src_dev * 131 + dst_dev);
  fill_pattern(src_dev, src.p, bytes, seed);
  const int grid = num_cus(exec_dev) * std::max(1, blocks_per_cu);
  float ms = 0.f;
  {
    DeviceGuard g(exec_dev);
    ms = time_launches([&](hipStream_t s) { launch_copy(kind, nontemporal, src.p, dst.p, n_vec, grid, s); }, iters, warmup);
  }
  const bool ok = holds_pattern(dst_dev, dst.p, bytes / 4, seed);
  // gbps = bytes copied per second (one direction over the link; for a self copy HBM moves 2x)
  return CopyResult{src_dev, dst_dev, exec_dev, iters, grid, bytes, kind, nontemporal, ok, (double)ms / iters,
                    gbps((double)bytes, ms, iters)};
}

// K5: aggregate ingress of `dst_dev` reading `bytes` from every device in `srcs` concurrently.
// A source equal to dst_dev is a local stream (one buffer per entry), which lets a 1-GPU box check
// the kernel's segment indexing; on a node the sources are the peers.
py::dict gather_bw(int dst_dev, const std::vector<int>& srcs, size_t bytes, int iters, int warmup, int blocks_per_cu) {
  if (srcs.empty() || srcs.size() > (size_t)kMaxSrc) throw std::invalid_argument("1..16 source devices");
  check_bytes_iters(bytes, iters);
  int ndev = 0;
  HIP_CHECK(hipGetDeviceCount(&ndev));
  if (dst_dev < 0 || dst_dev >= ndev) throw std::invalid_argument("device index out of range");
  for (int d : srcs) {
    if (d < 0 || d >= ndev) throw std::invalid_argument("source device index out of range");
  }
  auto seed_of = [](int dev) { return 0x51ed27u ^ (unsigned)(dev * 977); };
  float ms = 0.f;
  bool ok = true;
  const int nsrc = (int)srcs.size();
  {
    py::gil_scoped_release nogil;
    for (int d : srcs) enable_peer(dst_dev, d);
    std::vector<std::unique_ptr<DevBuf>> src_bufs;
    SrcSet set{};
    for (int i = 0; i < nsrc; ++i) {
      src_bufs.emplace_back(new DevBuf(srcs[i], bytes));
      fill_pattern(srcs[i], src_bufs.back()->p, bytes, seed_of(srcs[i]));
      set.p[i] = reinterpret_cast<const u32x4*>(src_bufs.back()->p);
    }
    DevBuf dst(dst_dev, bytes * (size_t)nsrc);
    DeviceGuard g(dst_dev);
    const int grid = gather_grid(dst_dev, blocks_per_cu, nsrc);
    ms = time_launches([&](hipStream_t s) {
      hipLaunchKernelGGL(gather_lds_kernel, dim3(grid), dim3(kBlock), 0, s, set, nsrc, (u32x4*)dst.p, bytes / 16);
    }, iters, warmup);
    // every segment holds its source's pattern
    for (int i = 0; i < nsrc && ok; ++i)
      ok = holds_pattern(dst_dev, (const char*)dst.p + (size_t)i * bytes, bytes / 4, seed_of(srcs[i]));
  }
  py::dict r;
  r["dst"] = dst_dev;
  r["srcs"] = srcs;
  r["bytes_per_src"] = bytes;
  r["iters"] = iters;
  r["ms_per_iter"] = (double)ms / iters;
  r["gbps"] = gbps((double)bytes * nsrc, ms, iters);
  r["ok"] = ok;
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
                 int warmup, int blocks_per_cu) {
  const int k = (int)devs.size();
  if (k < 2 || k > kMaxSrc + 1) throw std::invalid_argument("2..17 ring members");
  if ((int)peers.size() != k) throw std::invalid_argument("one peer list per member");
  check_bytes_iters(bytes, iters);
  int ndev = 0;
  HIP_CHECK(hipGetDeviceCount(&ndev));
  for (int d : devs)
    if (d < 0 || d >= ndev) throw std::invalid_argument("device index out of range");
  for (int m = 0; m < k; ++m) {
    if (peers[m].empty() || peers[m].size() > (size_t)kMaxSrc) throw std::invalid_argument("1..16 peers per member");
    for (int p : peers[m])
      if (p < 0 || p >= k || p == m) throw std::invalid_argument("peers are other members' indices");
  }
  auto seed_of = [](int m) { return 0x6a09e667u ^ (unsigned)(m * 7919 + 1); };
  std::vector<double> ms_member(k, 0.0);
  double wall_ms = 0.0;
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
    }
    std::vector<SrcSet> sets(k);
    std::vector<int> grid(k);
    std::vector<std::unique_ptr<TimedStream>> ts;
    for (int m = 0; m < k; ++m) {
      const int ns = (int)peers[m].size();
      for (int i = 0; i < ns; ++i) sets[m].p[i] = reinterpret_cast<const u32x4*>(src[peers[m][i]]->p);
      // members sharing a device split its CUs, so the self-test does not oversubscribe one GPU
      int share = 0;
      for (int d : devs) share += (d == devs[m]);
      grid[m] = gather_grid(devs[m], blocks_per_cu, ns, share);
      DeviceGuard g(devs[m]);
      ts.emplace_back(new TimedStream());
    }
    auto launch_round = [&]() {
      for (int m = 0; m < k; ++m) {
        DeviceGuard g(devs[m]);
        hipLaunchKernelGGL(gather_lds_kernel, dim3(grid[m]), dim3(kBlock), 0, ts[m]->s, sets[m], (int)peers[m].size(),
                           (u32x4*)inbox[m]->p, bytes / 16);
        HIP_CHECK(hipGetLastError());
      }
    };
    auto sync_all = [&]() {
      for (int m = 0; m < k; ++m) {
        DeviceGuard g(devs[m]);
        HIP_CHECK(hipStreamSynchronize(ts[m]->s));
      }
    };
    for (int i = 0; i < warmup; ++i) launch_round();
    sync_all();
    auto t0 = std::chrono::steady_clock::now();
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      ts[m]->begin();
    }
    for (int i = 0; i < iters; ++i) launch_round();
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      ts[m]->end();
    }
    sync_all();
    wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      ms_member[m] = ts[m]->ms();
    }
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
    gbps[m] = (double)bytes * peers[m].size() * iters / (ms_member[m] / 1e3) / 1e9;
    bound = (m == 0) ? gbps[m] : std::min(bound, gbps[m]);
  }
  r["devs"] = devs;
  r["peers"] = peers;
  r["bytes_per_peer"] = bytes;
  r["iters"] = iters;
  r["ms_member"] = ms_member;
  r["wall_ms"] = wall_ms;
  r["ingress_gbps"] = gbps;
  r["bound_gbps"] = bound;
  r["ok"] = ok;
  return r;
}

// K7 peer all-reduce: the sum of k members' buffers, left in every member's `out`, by this
// repository's own kernels over peer pointers (peer_allreduce.h): no RCCL.  One process, one stream
// per member as in K6, and members may repeat a device, so a 1-GPU box runs the k-member indexing
// and ordering.  The sum is taken in member order in fp32 and rounded once, so every member's result
// is bit-identical and equals a sequential CPU sum (ops/peer_ref.py).
//   oneshot: member m reduces every member's whole `in` into its own `out`; k x N read per member,
//            one launch, no dependency between members.
//   twoshot: phase 1, member m reduces slice m of every `in` into slice m of its `out`; phase 2, it
//            copies slice p from out[p] for every p != m.  Ingress per member 2(k-1)/k x N.
// Members are ordered by stream events alone (no kernel waits for a running kernel): e1[m] follows
// m's phase 1 and every member's phase 2 waits for all of them; e2[m] follows m's phase 2 and every
// member's next phase 1 waits for all of them, since phase 2 of p reads the slice m then overwrites.
struct PeerSlice {
  size_t first, count;  // in 16-byte vectors
};

// Slice s of k: vectors [s*per, min(n_vec, (s+1)*per)), per = ceil(n_vec / k); trailing ones may be empty.
std::vector<PeerSlice> peer_slices(size_t n_vec, int k) {
  const size_t per = (n_vec + k - 1) / k;
  std::vector<PeerSlice> out(k);
  for (int s = 0; s < k; ++s) {
    const size_t a = std::min(n_vec, (size_t)s * per), b = std::min(n_vec, (size_t)(s + 1) * per);
    out[s] = PeerSlice{a, b - a};
  }
  return out;
}

// Member buckets of peer_reduce_kernel: k x U loads of 16 bytes per lane stay within 64 VGPRs.
// The wide form (bf16 in, fp32 out) holds the same loads and eight accumulators, so it keeps the same U.
template <typename TI, typename TO>
void launch_peer_reduce(const SrcSet& set, int k, size_t v0, size_t v1, u32x4* dst, float scale, int grid, hipStream_t s) {
  const dim3 g(grid), b(kBlock);
  if (k <= 2)
    peer_reduce_kernel<TI, TO, 2, 4><<<g, b, 0, s>>>(set, k, v0, v1, dst, scale);
  else if (k <= 4)
    peer_reduce_kernel<TI, TO, 4, 4><<<g, b, 0, s>>>(set, k, v0, v1, dst, scale);
  else if (k <= 8)
    peer_reduce_kernel<TI, TO, 8, 2><<<g, b, 0, s>>>(set, k, v0, v1, dst, scale);
  else
    peer_reduce_kernel<TI, TO, 16, 1><<<g, b, 0, s>>>(set, k, v0, v1, dst, scale);
  HIP_CHECK(hipGetLastError());
}

// The element types of a reduce: bf16 -> bf16, fp32 -> fp32 and the wide bf16 -> fp32.
struct PeerTypes {
  bool in_bf16 = true, out_bf16 = true;
  size_t in_elem() const { return in_bf16 ? 2 : 4; }
  size_t out_elem() const { return out_bf16 ? 2 : 4; }
  size_t ratio() const { return out_elem() / in_elem(); }  // output vectors per input vector
};

PeerTypes peer_types(const std::string& dtype, const std::string& out_dtype) {
  if (dtype != "bf16" && dtype != "fp32") throw std::invalid_argument("dtype must be bf16|fp32");
  const std::string& o = out_dtype.empty() ? dtype : out_dtype;
  if (o != "bf16" && o != "fp32") throw std::invalid_argument("out_dtype must be bf16|fp32");
  if (dtype == "fp32" && o == "bf16") throw std::invalid_argument("fp32 inputs reduce to fp32 only");
  return PeerTypes{dtype == "bf16", o == "bf16"};
}

void launch_peer_reduce(PeerTypes t, const SrcSet& set, int k, size_t v0, size_t v1, u32x4* dst, float scale, int grid,
                        hipStream_t s) {
  if (!t.in_bf16)
    launch_peer_reduce<float, float>(set, k, v0, v1, dst, scale, grid, s);
  else if (t.out_bf16)
    launch_peer_reduce<uint16_t, uint16_t>(set, k, v0, v1, dst, scale, grid, s);
  else
    launch_peer_reduce<uint16_t, float>(set, k, v0, v1, dst, scale, grid, s);
}

struct PeerAllreduce {
  static constexpr size_t kMaxCount = (size_t)64 << 20;  // elements, through the array entry point

  std::vector<int> devs;
  int k = 0, nsets = 1;
  bool bf16 = true, twoshot = false;
  PeerTypes types;
  float scale = 1.0f;
  size_t count = 0, elem = 2, n_vec = 0;
  std::vector<std::unique_ptr<DevBuf>> in[2], out;  // in[set][m]: rounds alternate between the sets
  SrcSet srcs[2]{};
  std::vector<PeerSlice> plan;
  std::vector<SliceSet> gather;  // member m's phase 2: slice p of out[p], every p != m
  std::vector<int> reduce_grid, gather_grid_;
  std::vector<std::unique_ptr<TimedStream>> ts;
  std::vector<hipEvent_t> e1, e2;
  size_t rounds_done = 0;

  static void check_args(const std::vector<int>& devs, size_t count, const std::string& dtype, const std::string& algo) {
    if (devs.size() < 2 || devs.size() > (size_t)kMaxSrc) throw std::invalid_argument("2..16 members");
    int ndev = 0;
    HIP_CHECK(hipGetDeviceCount(&ndev));
    for (int d : devs)
      if (d < 0 || d >= ndev) throw std::invalid_argument("device index out of range");
    if (count < 1) throw std::invalid_argument("count >= 1");
    if (dtype != "bf16" && dtype != "fp32") throw std::invalid_argument("dtype must be bf16|fp32");
    if (algo != "oneshot" && algo != "twoshot") throw std::invalid_argument("algo must be oneshot|twoshot");
  }

  PeerAllreduce(const std::vector<int>& devs_, size_t count_, const std::string& dtype, const std::string& algo,
                int nsets_, int blocks_per_cu, const std::string& out_dtype = "", float scale_ = 1.0f)
      : devs(devs_), k((int)devs_.size()), nsets(nsets_), bf16(dtype == "bf16"), twoshot(algo == "twoshot"),
        types(peer_types(dtype, out_dtype)), scale(scale_), count(count_), elem(dtype == "bf16" ? 2 : 4), n_vec((count_ * (dtype == "bf16" ? 2 : 4) + 15) / 16),
        plan(peer_slices(n_vec, k)), gather(k), reduce_grid(k), gather_grid_(k), e1(k, nullptr), e2(k, nullptr) {
    for (int m = 0; m < k; ++m)
      for (int p = 0; p < k; ++p) enable_peer(devs[m], devs[p]);
    for (int m = 0; m < k; ++m) {
      for (int s = 0; s < nsets; ++s) {
        in[s].emplace_back(new DevBuf(devs[m], n_vec * 16));
        srcs[s].p[m] = reinterpret_cast<const u32x4*>(in[s][m]->p);
      }
      out.emplace_back(new DevBuf(devs[m], n_vec * 16 * types.ratio()));
    }
    try {
      for (int m = 0; m < k; ++m) {
        int share = 0;  // members sharing a device split its CUs, as in K6
        for (int d : devs) share += (d == devs[m]);
        const size_t mine = twoshot ? plan[m].count : n_vec;  // no more blocks than vectors to reduce
        const size_t cap = std::max(1, num_cus(devs[m]) * std::max(1, blocks_per_cu) / share);
        reduce_grid[m] = (int)std::max<size_t>(1, std::min(cap, (mine + kBlock - 1) / kBlock));
        gather_grid_[m] = gather_grid(devs[m], blocks_per_cu, k - 1, share);
        int i = 0;
        for (int p = 0; p < k; ++p) {
          if (p == m) continue;
          gather[m].p[i] = reinterpret_cast<const u32x4*>(out[p]->p);
          gather[m].first[i] = plan[p].first * types.ratio();  // slices of the output type
          gather[m].count[i] = plan[p].count * types.ratio();
          ++i;
        }
        DeviceGuard g(devs[m]);
        ts.emplace_back(new TimedStream());
        HIP_CHECK(hipEventCreateWithFlags(&e1[m], hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&e2[m], hipEventDisableTiming));
      }
    } catch (...) {
      release();
      throw;
    }
  }
  ~PeerAllreduce() { release(); }
  PeerAllreduce(const PeerAllreduce&) = delete;
  PeerAllreduce& operator=(const PeerAllreduce&) = delete;

  size_t padded() const { return n_vec * 16 / elem; }  // elements of a buffer, zero padding included

  void reduce(int m, int set, size_t v0, size_t v1) {
    if (v0 == v1) return;
    launch_peer_reduce(types, srcs[set], k, v0, v1, reinterpret_cast<u32x4*>(out[m]->p), scale, reduce_grid[m], ts[m]->s);
  }

  // One all-reduce of input set `set`, enqueued on every member's stream.  Every e1 / e2 is recorded
  // before any stream is made to wait for it (a wait for an event never recorded is no wait).
  void round(int set) {
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      if (!twoshot) {
        reduce(m, set, 0, n_vec);
        continue;
      }
      if (rounds_done)
        for (int p = 0; p < k; ++p)
          if (p != m) HIP_CHECK(hipStreamWaitEvent(ts[m]->s, e2[p], 0));
      reduce(m, set, plan[m].first, plan[m].first + plan[m].count);
      HIP_CHECK(hipEventRecord(e1[m], ts[m]->s));
    }
    for (int m = 0; twoshot && m < k; ++m) {
      DeviceGuard g(devs[m]);
      for (int p = 0; p < k; ++p)
        if (p != m) HIP_CHECK(hipStreamWaitEvent(ts[m]->s, e1[p], 0));
      peer_allgather_kernel<<<dim3(gather_grid_[m]), dim3(kBlock), 0, ts[m]->s>>>(gather[m], k - 1, (u32x4*)out[m]->p);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipEventRecord(e2[m], ts[m]->s));
    }
    ++rounds_done;
  }

  void sync_all() {
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      HIP_CHECK(hipStreamSynchronize(ts[m]->s));
    }
  }

  // in[set][m] = pattern(seed_of(set, m)), padding zero.
  static unsigned int seed_of(int set, int m) { return 0x243f6a88u ^ (unsigned)(set * 0x9e3779b9u) ^ (unsigned)(m * 7919 + 1); }
  void fill(int set) {
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      const dim3 grid(num_cus(devs[m]) * 4), block(kBlock);
      if (bf16)
        peer_fill_kernel<uint16_t><<<grid, block>>>((uint16_t*)in[set][m]->p, count, padded(), seed_of(set, m));
      else
        peer_fill_kernel<float><<<grid, block>>>((float*)in[set][m]->p, count, padded(), seed_of(set, m));
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipDeviceSynchronize());
    }
  }

  // Elements of every member's `out` (padding included) that are not the sum of set `set`'s patterns.
  unsigned long long wrong(int set) {
    SeedSet seeds{};
    for (int m = 0; m < k; ++m) seeds.s[m] = seed_of(set, m);
    unsigned long long total = 0;
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      DevBuf bad(devs[m], sizeof(unsigned long long));
      HIP_CHECK(hipMemset(bad.p, 0, sizeof(unsigned long long)));
      const dim3 grid(num_cus(devs[m]) * kBlocksPerCU), block(kBlock);
      if (bf16)
        peer_check_kernel<uint16_t><<<grid, block>>>((const uint16_t*)out[m]->p, count, padded(), seeds, k,
                                                     (unsigned long long*)bad.p);
      else
        peer_check_kernel<float><<<grid, block>>>((const float*)out[m]->p, count, padded(), seeds, k,
                                                  (unsigned long long*)bad.p);
      HIP_CHECK(hipGetLastError());
      unsigned long long n = 0;
      HIP_CHECK(hipMemcpy(&n, bad.p, sizeof(n), hipMemcpyDeviceToHost));
      total += n;
    }
    return total;
  }

 private:
  void release() noexcept {
    ts.clear();  // synchronises every stream first
    for (int m = 0; m < k; ++m) {
      int prev = 0;
      (void)hipGetDevice(&prev);
      (void)hipSetDevice(devs[m]);
      if (e1[m]) (void)hipEventDestroy(e1[m]);
      if (e2[m]) (void)hipEventDestroy(e2[m]);
      e1[m] = e2[m] = nullptr;
      (void)hipSetDevice(prev);
    }
  }
};

py::dict peer_allreduce(const std::vector<int>& devs, size_t count, const std::string& dtype, const std::string& algo,
                        int iters, int warmup, int blocks_per_cu) {
  PeerAllreduce::check_args(devs, count, dtype, algo);
  if (iters < 1 || warmup < 0) throw std::invalid_argument("iters >= 1, warmup >= 0");
  const int k = (int)devs.size();
  std::vector<double> ms_member(k, 0.0);
  double wall_ms = 0.0;
  unsigned long long wrong = 0;
  size_t bytes = 0;
  {
    py::gil_scoped_release nogil;
    // with more than one round, consecutive rounds alternate between two input sets and the check uses
    // the last round's: a round that ran ahead of the one before it leaves a mix of the two sums
    const int total = warmup + iters;
    PeerAllreduce ar(devs, count, dtype, algo, total >= 2 ? 2 : 1, blocks_per_cu);
    bytes = count * ar.elem;
    for (int s = 0; s < ar.nsets; ++s) ar.fill(s);
    int r = 0;
    for (; r < warmup; ++r) ar.round(r % ar.nsets);
    ar.sync_all();
    auto t0 = std::chrono::steady_clock::now();
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      ar.ts[m]->begin();
    }
    for (; r < total; ++r) ar.round(r % ar.nsets);
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      ar.ts[m]->end();
    }
    ar.sync_all();
    wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      ms_member[m] = ar.ts[m]->ms();
    }
    wrong = ar.wrong((total - 1) % ar.nsets);
  }
  const double time_us = *std::max_element(ms_member.begin(), ms_member.end()) * 1e3 / iters;
  py::dict r;
  r["devs"] = devs;
  r["dtype"] = dtype;
  r["algo"] = algo;
  r["iters"] = iters;
  r["bytes"] = bytes;
  r["count"] = count;
  r["time_us"] = time_us;
  r["algbw_gbps"] = (double)bytes / (time_us * 1e-6) / 1e9;
  r["busbw_gbps"] = (double)bytes / (time_us * 1e-6) / 1e9 * (2.0 * (k - 1) / k);
  r["ms_member"] = ms_member;
  r["wall_ms"] = wall_ms;
  r["wrong"] = wrong;
  r["ok"] = wrong == 0;
  return r;
}

// The same all-reduce on the caller's data: k one-dimensional arrays of equal length (uint16 bit
// patterns for bf16, float32 for fp32) in, the k members' results out, after `rounds` all-reduces of
// the same inputs.  `out_dtype` (none: the inputs') and `scale` select the wide and the scaled reduce.
py::list peer_allreduce_arrays(const std::vector<int>& devs, const std::vector<py::array>& inputs, const std::string& dtype,
                               const std::string& algo, int rounds, const std::optional<std::string>& out_dtype, float scale) {
  if (inputs.size() != devs.size()) throw std::invalid_argument("one input array per member");
  const size_t count = inputs.empty() ? 0 : (size_t)inputs[0].size();
  PeerAllreduce::check_args(devs, count, dtype, algo);
  if (count > PeerAllreduce::kMaxCount) throw std::invalid_argument("count <= 64 Mi elements");
  if (rounds < 1) throw std::invalid_argument("rounds >= 1");
  const PeerTypes types = peer_types(dtype, out_dtype.value_or(""));
  const py::dtype want = dtype == "bf16" ? py::dtype::of<uint16_t>() : py::dtype::of<float>();
  const py::dtype give = types.out_bf16 ? py::dtype::of<uint16_t>() : py::dtype::of<float>();
  const int k = (int)devs.size();
  std::vector<py::array> src, dst;
  for (const py::array& a : inputs) {
    if (a.ndim() != 1 || (size_t)a.size() != count || !a.dtype().is(want))
      throw std::invalid_argument("inputs: one-dimensional arrays of one length, uint16 (bf16) or float32 (fp32)");
    src.push_back(py::array::ensure(a, py::array::c_style));
    dst.push_back(py::array(give, std::vector<py::ssize_t>{(py::ssize_t)count}));
  }
  std::vector<const void*> from(k);
  std::vector<void*> to(k);
  for (int m = 0; m < k; ++m) {
    from[m] = src[m].data();
    to[m] = dst[m].mutable_data();
  }
  {
    py::gil_scoped_release nogil;
    PeerAllreduce ar(devs, count, dtype, algo, 1, kBlocksPerCU, out_dtype.value_or(""), scale);
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      HIP_CHECK(hipMemset(ar.in[0][m]->p, 0, ar.n_vec * 16));
      HIP_CHECK(hipMemcpy(ar.in[0][m]->p, from[m], count * ar.elem, hipMemcpyHostToDevice));
      HIP_CHECK(hipDeviceSynchronize());
    }
    for (int r = 0; r < rounds; ++r) ar.round(0);
    ar.sync_all();
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      HIP_CHECK(hipMemcpy(to[m], ar.out[m]->p, count * types.out_elem(), hipMemcpyDeviceToHost));
    }
  }
  py::list r;
  for (py::array& a : dst) r.append(a);
  return r;
}

}  // namespace
#include "peer_rank.h"  // one rank of the peer communicator's device backend, over the K7 launches above
namespace {

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
  static void check_dev(int dev) {
    int ndev = 0;
    HIP_CHECK(hipGetDeviceCount(&ndev));
    if (dev < 0 || dev >= ndev) throw std::invalid_argument("device index out of range");
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
  ChaseChain::check_dev(src_dev);
  ChaseChain::check_dev(exec_dev);
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
  return r;
}

py::dict copy_bw(int src_dev, int dst_dev, int exec_dev, size_t bytes, int iters, int warmup, const std::string& kind,
                 bool nontemporal, int blocks_per_cu) {
  CopyResult c;
  {
    py::gil_scoped_release nogil;
    c = copy_bw_impl(src_dev, dst_dev, exec_dev, bytes, iters, warmup, kind, nontemporal, blocks_per_cu);
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

// K2 over IPC: the writer's kernel pushes a local patterned buffer into another process's buffer
// through the imported mapping (remote stores, the direction RCCL's P2P write protocol uses).  The
// owner checks the result (IpcBuffer.holds), since only it knows the write has landed in its memory.
py::dict ipc_write_bw(const py::bytes& handle, int dev, size_t bytes, unsigned int seed, int iters, int warmup,
                      int blocks_per_cu) {
  check_bytes_iters(bytes, iters);
  IpcMappings map({handle}, dev);
  float ms = 0.f;
  {
    py::gil_scoped_release nogil;
    DeviceGuard g(dev);
    DevBuf src(dev, bytes);
    fill_pattern(dev, src.p, bytes, seed);
    const int grid = num_cus(dev) * std::max(1, blocks_per_cu);
    ms = time_launches([&](hipStream_t s) { launch_copy("lds", true, src.p, map.p[0], bytes / 16, grid, s); }, iters, warmup);
  }
  py::dict d;
  d["dev"] = dev;
  d["bytes"] = bytes;
  d["iters"] = iters;
  d["ms_per_iter"] = ms / iters;
  d["gbps"] = gbps((double)bytes, ms, iters);
  return d;
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
  d["iters"] = iters;
  d["ms_per_iter"] = ms / iters;
  d["gbps"] = gbps((double)bytes * nsrc, ms, iters);
  d["ok"] = ok;
  return d;
}

py::dict ipc_read_bw(const py::bytes& handle, int dev, size_t bytes, unsigned int seed, int iters, int warmup,
                     int blocks_per_cu) {
  check_bytes_iters(bytes, iters);
  IpcMappings map({handle}, dev);
  float ms = 0.f;
  bool ok = true;
  {
    py::gil_scoped_release nogil;
    DeviceGuard g(dev);
    DevBuf dst(dev, bytes);
    const int grid = num_cus(dev) * std::max(1, blocks_per_cu);
    ms = time_launches([&](hipStream_t s) { launch_copy("lds", true, map.p[0], dst.p, bytes / 16, grid, s); }, iters, warmup);
    ok = holds_pattern(dev, dst.p, bytes / 4, seed);
  }
  py::dict d;
  d["dev"] = dev;
  d["bytes"] = bytes;
  d["iters"] = iters;
  d["ms_per_iter"] = ms / iters;
  d["gbps"] = gbps((double)bytes, ms, iters);
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
        py::arg("blocks_per_cu") = kBlocksPerCU);
  m.def("gather_bw", &gather_bw, py::arg("dst_dev"), py::arg("srcs"), py::arg("bytes") = (size_t)64 << 20,
        py::arg("iters") = 3, py::arg("warmup") = 1, py::arg("blocks_per_cu") = kBlocksPerCU);
  m.def("ring_bw", &ring_bw, py::arg("devs"), py::arg("peers"), py::arg("bytes") = (size_t)64 << 20, py::arg("iters") = 3,
        py::arg("warmup") = 1, py::arg("blocks_per_cu") = kBlocksPerCU);
  m.def("peer_allreduce", &peer_allreduce, py::arg("devs"), py::arg("count"), py::arg("dtype") = "bf16",
        py::arg("algo") = "twoshot", py::arg("iters") = 3, py::arg("warmup") = 1, py::arg("blocks_per_cu") = kBlocksPerCU,
        "K7: timed all-reduce (sum) of device-made inputs over peer pointers; every member's result checked");
  m.def("peer_allreduce_arrays", &peer_allreduce_arrays, py::arg("devs"), py::arg("inputs"), py::arg("dtype") = "bf16",
        py::arg("algo") = "twoshot", py::arg("rounds") = 1, py::arg("out_dtype") = py::none(), py::arg("scale") = 1.0f,
        "K7 on the caller's arrays (uint16 bit patterns for bf16, float32 for fp32): the k members' results, "
        "scale x sum, in out_dtype (none: dtype; fp32 of bf16 inputs is the wide reduce)");
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
