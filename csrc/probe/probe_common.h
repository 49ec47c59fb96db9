// What every file of csrc/probe/ uses: the launch geometry, the source set of a gather, the pattern
// fill and verifier, and the host helpers around a launch (device guard and buffer, argument checks,
// grids, the single-stream and the per-member timers).  All of it joins the unnamed namespace of the
// one translation unit, csrc/probe/probe.hip.
#pragma once
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

#define HIP_CHECK(expr)                                                                          \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess)                                                                        \
      throw std::runtime_error(std::string(#expr " failed: ") + hipGetErrorString(_e) + " at " + \
                               __FILE__ + ":" + std::to_string(__LINE__));                       \
  } while (0)

namespace {

// Equal to the all-reduce's kSelfCopy* (csrc/rccl/self_copy.h) today, but tuned on their own (these
// on the LDS budget of probe.hip's geometry, those on the 2 GiB headline): kept separate on purpose.
constexpr int kBlock = 256;
constexpr int kUnroll = 4;
constexpr int kTileVec = kBlock * kUnroll;  // 16-byte vectors per block-iteration (16 KiB)
constexpr int kBlocksPerCU = 8;
static_assert(kBlock == gtk::kStreamBlock, "stream_copy.h indexes blocks of kStreamBlock threads");

// The sources of one gather (K5) or the members of one reduce (K7): up to kMaxSrc peers at once.
constexpr int kMaxSrc = 16;
struct SrcSet {
  const u32x4* p[kMaxSrc];
};
// The destinations of one push reduce (K7): every member's `out`, in the order a lane stores to them.
struct DstSet {
  u32x4* p[kMaxSrc];
};

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

// Every entry of `devs` is a device index of this process.
void check_devs(const std::vector<int>& devs) {
  int ndev = 0;
  HIP_CHECK(hipGetDeviceCount(&ndev));
  for (int d : devs)
    if (d < 0 || d >= ndev) throw std::invalid_argument("device index out of range");
}
void check_dev(int dev) { check_devs({dev}); }

// How many entries of `devs` are `dev`: members that share a device split its CUs, so a self-test
// with repeated members does not oversubscribe one GPU.
int device_share(const std::vector<int>& devs, int dev) { return (int)std::count(devs.begin(), devs.end(), dev); }

// Blocks of a gather launch on a device of `cus` CUs: a multiple of nsrc, so every source gets the
// same block count.  Members of a ring that share a device (`share` of them) split its CUs.
int gather_grid_cus(int cus, int blocks_per_cu, int nsrc, int share) {
  const int per = std::max(1, cus * std::max(1, blocks_per_cu) / (nsrc * share));
  return per * nsrc;
}
int gather_grid(int dev, int blocks_per_cu, int nsrc, int share = 1) {
  return gather_grid_cus(num_cus(dev), blocks_per_cu, nsrc, share);
}

// GB/s of `bytes` moved per iteration, `iters` iterations in `ms`.
double gbps(double bytes, double ms, int iters) { return bytes / (ms / 1e3 / iters) / 1e9; }

// The timing keys of a bandwidth result, from the same three numbers.
void put_rate(py::dict& r, double bytes, float ms, int iters) {
  r["iters"] = iters;
  r["ms_per_iter"] = (double)ms / iters;
  r["gbps"] = gbps(bytes, ms, iters);
}

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

// Member m's stream is ts[m], a stream of devs[m] (K6, K7).
using MemberStreams = std::vector<std::unique_ptr<TimedStream>>;

void sync_streams(const std::vector<int>& devs, const MemberStreams& ts) {
  for (size_t m = 0; m < ts.size(); ++m) {
    DeviceGuard g(devs[m]);
    HIP_CHECK(hipStreamSynchronize(ts[m]->s));
  }
}

struct MemberTimes {
  std::vector<double> ms_member;  // every member's own stream time of the timed rounds
  double wall_ms = 0.0;           // host time over the same rounds, all members together
};

// time_launches for one stream per member: `round(r)` enqueues round number r on every member's
// stream, `warmup` rounds untimed, then `iters` between every member's begin() and end().
template <class F>
MemberTimes time_member_rounds(const std::vector<int>& devs, const MemberStreams& ts, int warmup, int iters, F round) {
  auto each = [&](auto f) {
    for (size_t m = 0; m < ts.size(); ++m) {
      DeviceGuard g(devs[m]);
      f(m);
    }
  };
  MemberTimes t{std::vector<double>(ts.size(), 0.0), 0.0};
  int r = 0;
  for (; r < warmup; ++r) round(r);
  sync_streams(devs, ts);
  auto t0 = std::chrono::steady_clock::now();
  each([&](size_t m) { ts[m]->begin(); });
  for (; r < warmup + iters; ++r) round(r);
  each([&](size_t m) { ts[m]->end(); });
  sync_streams(devs, ts);
  t.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  each([&](size_t m) { t.ms_member[m] = ts[m]->ms(); });
  return t;
}

void fill_pattern(int dev, void* p, size_t bytes, unsigned int seed) {
  DeviceGuard g(dev);
  hipLaunchKernelGGL(fill_pattern_kernel, dim3(num_cus(dev) * 4), dim3(kBlock), 0, 0, (unsigned int*)p, bytes / 4, seed);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
}

// A destination that will be checked against pattern(seed), before anything is launched into it:
// pattern(~seed), which differs from pattern(seed) in every bit of every word.  hipMalloc may hand back
// a block that an earlier call freed holding the very pattern the check looks for; after this only the
// launches under test can make a word right.  Synchronised, so none of it falls into a timed section.
void poison_pattern(int dev, void* p, size_t bytes, unsigned int seed) { fill_pattern(dev, p, bytes, ~seed); }

// What one kernel on `dev` counts: `launch(counter)` starts it on the null stream with a cleared
// 8-byte counter of that device, which is then copied back.
template <class F>
unsigned long long count_on_device(int dev, F launch) {
  DeviceGuard g(dev);
  DevBuf bad(dev, sizeof(unsigned long long));
  HIP_CHECK(hipMemset(bad.p, 0, sizeof(unsigned long long)));
  launch((unsigned long long*)bad.p);
  HIP_CHECK(hipGetLastError());
  unsigned long long n = 0;
  HIP_CHECK(hipMemcpy(&n, bad.p, sizeof(n), hipMemcpyDeviceToHost));
  return n;
}

// Words of p[0, n_words), memory of `dev`, that differ from pattern(seed).  One pass on the device.
unsigned long long pattern_mismatches(int dev, const void* p, size_t n_words, unsigned int seed) {
  return count_on_device(dev, [&](unsigned long long* bad) {
    hipLaunchKernelGGL(pattern_mismatch_kernel, dim3(num_cus(dev) * kBlocksPerCU), dim3(kBlock), 0, 0,
                       (const unsigned int*)p, n_words, seed, bad);
  });
}

bool holds_pattern(int dev, const void* p, size_t n_words, unsigned int seed) {
  return 0 == pattern_mismatches(dev, p, n_words, seed);
}

}  // namespace
