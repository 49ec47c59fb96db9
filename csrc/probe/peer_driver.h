// K7 host side: the launch plan (slices, element types, reduce and gather launches and their grids)
// that PeerAllreduce below and PeerRank (peer_rank.h) share, and PeerAllreduce's two entry points.
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
#pragma once
#include "peer_allreduce.h"
#include "probe_common.h"

namespace {

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

// Blocks of a reduce of `n_vec` vectors on a device of `cus` CUs that `share` members split: no more
// blocks than vectors to reduce.
int peer_reduce_grid(int cus, int blocks_per_cu, int share, size_t n_vec) {
  const size_t cap = std::max(1, cus * std::max(1, blocks_per_cu) / share);
  return (int)std::max<size_t>(1, std::min(cap, (n_vec + kBlock - 1) / kBlock));
}

// Phase 2 of a two-shot for rank `skip`: slice p (vectors of the output type) of outs[p], every p != skip.
SliceSet peer_gather_slices(const std::vector<const u32x4*>& outs, const std::vector<PeerSlice>& slices, int skip) {
  SliceSet sl{};
  int i = 0;
  for (int p = 0; p < (int)outs.size(); ++p) {
    if (p == skip) continue;
    sl.p[i] = outs[p];
    sl.first[i] = slices[p].first;
    sl.count[i] = slices[p].count;
    ++i;
  }
  return sl;
}

void launch_peer_gather(const SliceSet& sl, int nsrc, u32x4* dst, int grid, hipStream_t s) {
  peer_allgather_kernel<<<dim3(grid), dim3(kBlock), 0, s>>>(sl, nsrc, dst);
  HIP_CHECK(hipGetLastError());
}

struct PeerAllreduce {
  static constexpr size_t kMaxCount = (size_t)64 << 20;  // elements, through the array entry point

  std::vector<int> devs;
  int k = 0, nsets = 1;
  bool twoshot = false;
  PeerTypes types;
  float scale = 1.0f;
  size_t count = 0, n_vec = 0;
  std::vector<std::unique_ptr<DevBuf>> in[2], out;  // in[set][m]: rounds alternate between the sets
  SrcSet srcs[2]{};
  std::vector<PeerSlice> plan;
  std::vector<SliceSet> gather;  // member m's phase 2: slice p of out[p], every p != m
  std::vector<int> reduce_grid, gather_grid_;
  MemberStreams ts;
  std::vector<hipEvent_t> e1, e2;
  size_t rounds_done = 0;

  // The dtypes are peer_types' to check, which the caller has passed before it comes here.
  static void check_args(const std::vector<int>& devs, size_t count, const std::string& algo) {
    if (devs.size() < 2 || devs.size() > (size_t)kMaxSrc) throw std::invalid_argument("2..16 members");
    check_devs(devs);
    if (count < 1) throw std::invalid_argument("count >= 1");
    if (algo != "oneshot" && algo != "twoshot") throw std::invalid_argument("algo must be oneshot|twoshot");
  }

  PeerAllreduce(const std::vector<int>& devs_, size_t count_, PeerTypes types_, const std::string& algo, int nsets_,
                int blocks_per_cu, float scale_ = 1.0f)
      : devs(devs_), k((int)devs_.size()), nsets(nsets_), twoshot(algo == "twoshot"), types(types_), scale(scale_),
        count(count_), n_vec((count_ * types_.in_elem() + 15) / 16), plan(peer_slices(n_vec, k)), gather(k),
        reduce_grid(k), gather_grid_(k), e1(k, nullptr), e2(k, nullptr) {
    for (int m = 0; m < k; ++m)
      for (int p = 0; p < k; ++p) enable_peer(devs[m], devs[p]);
    std::vector<const u32x4*> outs(k);
    std::vector<PeerSlice> out_plan(k);  // slices of the output type
    for (int m = 0; m < k; ++m) {
      for (int s = 0; s < nsets; ++s) {
        in[s].emplace_back(new DevBuf(devs[m], n_vec * 16));
        srcs[s].p[m] = reinterpret_cast<const u32x4*>(in[s][m]->p);
      }
      out.emplace_back(new DevBuf(devs[m], n_vec * 16 * types.ratio()));
      outs[m] = reinterpret_cast<const u32x4*>(out[m]->p);
      out_plan[m] = PeerSlice{plan[m].first * types.ratio(), plan[m].count * types.ratio()};
    }
    try {
      for (int m = 0; m < k; ++m) {
        const int share = device_share(devs, devs[m]);  // as in K6
        reduce_grid[m] = peer_reduce_grid(num_cus(devs[m]), blocks_per_cu, share, twoshot ? plan[m].count : n_vec);
        gather_grid_[m] = gather_grid(devs[m], blocks_per_cu, k - 1, share);
        gather[m] = peer_gather_slices(outs, out_plan, m);
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

  size_t padded() const { return n_vec * 16 / types.in_elem(); }  // elements of a buffer, zero padding included

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
      launch_peer_gather(gather[m], k - 1, (u32x4*)out[m]->p, gather_grid_[m], ts[m]->s);
      HIP_CHECK(hipEventRecord(e2[m], ts[m]->s));
    }
    ++rounds_done;
  }

  // in[set][m] = pattern(seed_of(set, m)), padding zero.
  static unsigned int seed_of(int set, int m) { return 0x243f6a88u ^ (unsigned)(set * 0x9e3779b9u) ^ (unsigned)(m * 7919 + 1); }
  void fill(int set) {
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      const dim3 grid(num_cus(devs[m]) * 4), block(kBlock);
      if (types.in_bf16)
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
    for (int m = 0; m < k; ++m)
      total += count_on_device(devs[m], [&](unsigned long long* bad) {
        const dim3 grid(num_cus(devs[m]) * kBlocksPerCU), block(kBlock);
        if (types.in_bf16)
          peer_check_kernel<uint16_t><<<grid, block>>>((const uint16_t*)out[m]->p, count, padded(), seeds, k, bad);
        else
          peer_check_kernel<float><<<grid, block>>>((const float*)out[m]->p, count, padded(), seeds, k, bad);
      });
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
  const PeerTypes types = peer_types(dtype, "");
  PeerAllreduce::check_args(devs, count, algo);
  if (iters < 1 || warmup < 0) throw std::invalid_argument("iters >= 1, warmup >= 0");
  const int k = (int)devs.size();
  MemberTimes t;
  unsigned long long wrong = 0;
  const size_t bytes = count * types.in_elem();
  {
    py::gil_scoped_release nogil;
    // with more than one round, consecutive rounds alternate between two input sets and the check uses
    // the last round's: a round that ran ahead of the one before it leaves a mix of the two sums
    const int total = warmup + iters;
    PeerAllreduce ar(devs, count, types, algo, total >= 2 ? 2 : 1, blocks_per_cu);
    for (int s = 0; s < ar.nsets; ++s) ar.fill(s);
    t = time_member_rounds(devs, ar.ts, warmup, iters, [&](int r) { ar.round(r % ar.nsets); });
    wrong = ar.wrong((total - 1) % ar.nsets);
  }
  const double time_us = *std::max_element(t.ms_member.begin(), t.ms_member.end()) * 1e3 / iters;
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
  r["ms_member"] = t.ms_member;
  r["wall_ms"] = t.wall_ms;
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
  const PeerTypes types = peer_types(dtype, out_dtype.value_or(""));
  PeerAllreduce::check_args(devs, count, algo);
  if (count > PeerAllreduce::kMaxCount) throw std::invalid_argument("count <= 64 Mi elements");
  if (rounds < 1) throw std::invalid_argument("rounds >= 1");
  const py::dtype want = types.in_bf16 ? py::dtype::of<uint16_t>() : py::dtype::of<float>();
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
    PeerAllreduce ar(devs, count, types, algo, 1, kBlocksPerCU, scale);
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      HIP_CHECK(hipMemset(ar.in[0][m]->p, 0, ar.n_vec * 16));
      HIP_CHECK(hipMemcpy(ar.in[0][m]->p, from[m], count * types.in_elem(), hipMemcpyHostToDevice));
      HIP_CHECK(hipDeviceSynchronize());
    }
    for (int r = 0; r < rounds; ++r) ar.round(0);
    sync_streams(devs, ar.ts);
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
