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
//   push:    member m reduces slice m of every `in` and stores the result into slice m of every member's
//            `out` (peer_reduce_push_kernel), its own first and the others in ring order: (k-1)/k x N read
//            in and (k-1)/k x N written out per member, one launch, no second phase, the two-shot's bits.
// Members are ordered by stream events alone (no kernel waits for a running kernel): e1[m] follows
// m's phase 1 and every member's phase 2 waits for all of them; e2[m] follows m's phase 2 and every
// member's next phase 1 waits for all of them, since phase 2 of p reads the slice m then overwrites.
// A push takes none of those events: slice m of every `out` is written by member m alone, on m's stream,
// and no kernel of a round reads an `out`, so consecutive rounds of a member are ordered by its stream.
// On the fp8 wire it takes the one-shot's: eq before the sum, e1 before the next quantize.
//   wire fp8: a round starts with every member packing its own `in` into its own packed buffer
//            (peer_q8.h), phase 1 reads the packed buffers, blocks of 32 elements in place of vectors,
//            and phase 2 is unchanged.  eq[m] follows m's quantize and every member's phase 1 waits for
//            all of them; e1[m] follows m's phase 1 in one-shot too, and every member's next quantize
//            waits for all of them, since phase 1 of p still reads the packed buffer m then overwrites.
//   wire fp8x2: a two-shot on the fp8 wire whose phase 1 packs its sums again into member m's second packed
//            buffer (peer_q8_repack_kernel) and whose phase 2 unpacks all k slices, m's own included, from
//            those buffers into out[m] (peer_q8_unpack_kernel): no member reads another's `out`.  The events
//            are the two-shot's: the e2 wait before phase 1 holds back the overwrite of the second packed
//            buffer m until every member's last phase 2 has read it, as it held back the overwrite of slice m
//            of out[m]; the e1 wait before phase 2 lets a slice be read once its owner has packed it.
#pragma once
#include "peer_allreduce.h"
#include "peer_q8.h"
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

// The push form: the reduce's buckets and U, the stores of every position going to every dsts.p[d], d < k.
template <typename TI, typename TO>
void launch_peer_reduce_push(const SrcSet& set, const DstSet& dsts, int k, size_t v0, size_t v1, float scale, int grid, hipStream_t s) {
  const dim3 g(grid), b(kBlock);
  if (k <= 2)
    peer_reduce_push_kernel<TI, TO, 2, 4><<<g, b, 0, s>>>(set, dsts, k, v0, v1, scale);
  else if (k <= 4)
    peer_reduce_push_kernel<TI, TO, 4, 4><<<g, b, 0, s>>>(set, dsts, k, v0, v1, scale);
  else if (k <= 8)
    peer_reduce_push_kernel<TI, TO, 8, 2><<<g, b, 0, s>>>(set, dsts, k, v0, v1, scale);
  else
    peer_reduce_push_kernel<TI, TO, 16, 1><<<g, b, 0, s>>>(set, dsts, k, v0, v1, scale);
  HIP_CHECK(hipGetLastError());
}

void launch_peer_reduce_push(PeerTypes t, const SrcSet& set, const DstSet& dsts, int k, size_t v0, size_t v1, float scale, int grid,
                             hipStream_t s) {
  if (!t.in_bf16)
    launch_peer_reduce_push<float, float>(set, dsts, k, v0, v1, scale, grid, s);
  else if (t.out_bf16)
    launch_peer_reduce_push<uint16_t, uint16_t>(set, dsts, k, v0, v1, scale, grid, s);
  else
    launch_peer_reduce_push<uint16_t, float>(set, dsts, k, v0, v1, scale, grid, s);
}

// The destinations of member m's push: every member's `out`, m's own first and the others in ring order
// after it, so the k members of a round do not all store to member 0 first.
DstSet peer_push_dsts(const std::vector<u32x4*>& outs, int m) {
  DstSet d{};
  const int k = (int)outs.size();
  for (int j = 0; j < k; ++j) d.p[j] = outs[(m + j) % k];
  return d;
}

// The fp8 wire's two launches.  The sum keeps the reduce's member buckets and U: k x U code vectors and as
// many exponent words per lane, 80 VGPRs of loads, and sixteen accumulators.
template <typename TO>
void launch_peer_q8_sum(const SrcSet& packed, int k, size_t exp_vec, size_t b0, size_t b1, u32x4* dst, float scale, int grid,
                        hipStream_t s) {
  const dim3 g(grid), b(kBlock);
  if (k <= 2)
    peer_q8_sum_kernel<TO, 2, 4><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, dst, scale);
  else if (k <= 4)
    peer_q8_sum_kernel<TO, 4, 4><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, dst, scale);
  else if (k <= 8)
    peer_q8_sum_kernel<TO, 8, 2><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, dst, scale);
  else
    peer_q8_sum_kernel<TO, 16, 1><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, dst, scale);
  HIP_CHECK(hipGetLastError());
}

void launch_peer_q8_sum(bool out_bf16, const SrcSet& packed, int k, size_t exp_vec, size_t b0, size_t b1, u32x4* dst,
                        float scale, int grid, hipStream_t s) {
  if (out_bf16)
    launch_peer_q8_sum<uint16_t>(packed, k, exp_vec, b0, b1, dst, scale, grid, s);
  else
    launch_peer_q8_sum<float>(packed, k, exp_vec, b0, b1, dst, scale, grid, s);
}

template <typename TO>
void launch_peer_q8_sum_push(const SrcSet& packed, const DstSet& dsts, int k, size_t exp_vec, size_t b0, size_t b1, float scale,
                             int grid, hipStream_t s) {
  const dim3 g(grid), b(kBlock);
  if (k <= 2)
    peer_q8_sum_push_kernel<TO, 2, 4><<<g, b, 0, s>>>(packed, dsts, k, exp_vec, b0, b1, scale);
  else if (k <= 4)
    peer_q8_sum_push_kernel<TO, 4, 4><<<g, b, 0, s>>>(packed, dsts, k, exp_vec, b0, b1, scale);
  else if (k <= 8)
    peer_q8_sum_push_kernel<TO, 8, 2><<<g, b, 0, s>>>(packed, dsts, k, exp_vec, b0, b1, scale);
  else
    peer_q8_sum_push_kernel<TO, 16, 1><<<g, b, 0, s>>>(packed, dsts, k, exp_vec, b0, b1, scale);
  HIP_CHECK(hipGetLastError());
}

void launch_peer_q8_sum_push(bool out_bf16, const SrcSet& packed, const DstSet& dsts, int k, size_t exp_vec, size_t b0, size_t b1,
                             float scale, int grid, hipStream_t s) {
  if (out_bf16)
    launch_peer_q8_sum_push<uint16_t>(packed, dsts, k, exp_vec, b0, b1, scale, grid, s);
  else
    launch_peer_q8_sum_push<float>(packed, dsts, k, exp_vec, b0, b1, scale, grid, s);
}

void launch_peer_q8_quantize(bool in_bf16, const u32x4* win, u32x4* packed, size_t exp_vec, size_t b0, size_t b1, size_t count,
                             int grid, hipStream_t s) {
  if (in_bf16)
    peer_q8_quantize_kernel<uint16_t><<<dim3(grid), dim3(kBlock), 0, s>>>(win, packed, exp_vec, b0, b1, count);
  else
    peer_q8_quantize_kernel<float><<<dim3(grid), dim3(kBlock), 0, s>>>(win, packed, exp_vec, b0, b1, count);
  HIP_CHECK(hipGetLastError());
}

// The quantize with error feedback: `residual`, the member's own fp32 buffer (one float per element of the
// window), is added before the packing and rewritten with what the packing dropped, in blocks [b0, b1).
void launch_peer_q8_quantize_ef(bool in_bf16, const u32x4* win, u32x4* packed, size_t exp_vec, size_t b0, size_t b1, size_t count,
                                u32x4* residual, int grid, hipStream_t s) {
  if (in_bf16)
    peer_q8_quantize_ef_kernel<uint16_t><<<dim3(grid), dim3(kBlock), 0, s>>>(win, packed, exp_vec, b0, b1, count, residual);
  else
    peer_q8_quantize_ef_kernel<float><<<dim3(grid), dim3(kBlock), 0, s>>>(win, packed, exp_vec, b0, b1, count, residual);
  HIP_CHECK(hipGetLastError());
}

// The fp8x2 wire's two launches.  The repack keeps the sum's member buckets and U: its loads are the sum's,
// and where the sum narrows and stores sixteen results it scales and converts them in place.
void launch_peer_q8_repack(const SrcSet& packed, int k, size_t exp_vec, size_t b0, size_t b1, u32x4* packed_out, float scale,
                           int grid, hipStream_t s) {
  const dim3 g(grid), b(kBlock);
  if (k <= 2)
    peer_q8_repack_kernel<2, 4><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, packed_out, scale);
  else if (k <= 4)
    peer_q8_repack_kernel<4, 4><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, packed_out, scale);
  else if (k <= 8)
    peer_q8_repack_kernel<8, 2><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, packed_out, scale);
  else
    peer_q8_repack_kernel<16, 1><<<g, b, 0, s>>>(packed, k, exp_vec, b0, b1, packed_out, scale);
  HIP_CHECK(hipGetLastError());
}

// `sl` holds blocks, not vectors: slice p is blocks [first, first + count) of rank p's second packed buffer.
void launch_peer_q8_unpack(bool out_bf16, const SliceSet& sl, int nsrc, size_t exp_vec, u32x4* dst, int grid, hipStream_t s) {
  if (out_bf16)
    peer_q8_unpack_kernel<uint16_t><<<dim3(grid), dim3(kBlock), 0, s>>>(sl, nsrc, exp_vec, dst);
  else
    peer_q8_unpack_kernel<float><<<dim3(grid), dim3(kBlock), 0, s>>>(sl, nsrc, exp_vec, dst);
  HIP_CHECK(hipGetLastError());
}

// The wire of a call: native, fp8 (phase 1 reads packed buffers) or fp8x2 (phase 2 of a two-shot does too).
struct PeerWire {
  bool fp8 = false, x2 = false;
};

PeerWire peer_wire(const std::string& wire, const std::string& algo) {
  if (wire != "native" && wire != "fp8" && wire != "fp8x2") throw std::invalid_argument("wire must be native|fp8|fp8x2");
  if (wire == "fp8x2" && algo == "oneshot")
    throw std::invalid_argument("wire fp8x2 packs the gather phase of a twoshot: a oneshot has none");
  if (wire == "fp8x2" && algo == "push")
    throw std::invalid_argument("wire fp8x2 packs the gather phase of a twoshot: a push has none");
  return PeerWire{wire != "native", wire == "fp8x2"};
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
  bool push = false;                // phase 1 stores slice m of the sum into every member's `out`; no phase 2
  PeerTypes types;
  float scale = 1.0f;
  bool fp8 = false;                 // the wire: members read each other's packed buffers, not their `in`
  bool x2 = false;                  // fp8x2: phase 2 reads the members' second packed buffers, not their `out`
  bool dry = false;                 // tests: a round records and waits for its events but launches no kernel
  size_t count = 0, n_vec = 0;      // n_vec: vectors of an `in`
  size_t n_blocks = 0;              // fp8: blocks of 32 elements, and `out` holds whole blocks
  std::vector<std::unique_ptr<DevBuf>> in[2], out;  // in[set][m]: rounds alternate between the sets
  std::vector<std::unique_ptr<DevBuf>> packed;      // fp8: packed[m], member m's `in` of the current round
  std::vector<std::unique_ptr<DevBuf>> packed_out;  // fp8x2: packed_out[m], slice m of the round's sum, packed by m
  SrcSet srcs[2]{}, packs{};
  std::vector<DstSet> push_dsts;    // push: member m's destinations, every `out` from its own on
  SliceSet unpack_set{};            // fp8x2: every member's phase 2, slice p (blocks) of packed_out[p] for every p
  std::vector<PeerSlice> plan;      // phase 1 of a two-shot or a push: vectors of an `in`; fp8: blocks
  std::vector<SliceSet> gather;  // member m's phase 2: slice p of out[p], every p != m
  std::vector<int> reduce_grid, gather_grid_, quantize_grid;
  MemberStreams ts;
  std::vector<hipEvent_t> e1, e2, eq;
  size_t rounds_done = 0;

  // The dtypes are peer_types' to check, which the caller has passed before it comes here.
  static void check_args(const std::vector<int>& devs, size_t count, const std::string& algo) {
    if (devs.size() < 2 || devs.size() > (size_t)kMaxSrc) throw std::invalid_argument("2..16 members");
    check_devs(devs);
    if (count < 1) throw std::invalid_argument("count >= 1");
    if (algo != "oneshot" && algo != "twoshot" && algo != "push") throw std::invalid_argument("algo must be oneshot|twoshot|push");
  }

  PeerAllreduce(const std::vector<int>& devs_, size_t count_, PeerTypes types_, const std::string& algo, int nsets_,
                int blocks_per_cu, float scale_ = 1.0f, PeerWire wire = PeerWire{})
      : devs(devs_), k((int)devs_.size()), nsets(nsets_), twoshot(algo == "twoshot"), push(algo == "push"), types(types_), scale(scale_), fp8(wire.fp8),
        x2(wire.x2), count(count_), n_vec((count_ * types_.in_elem() + 15) / 16), n_blocks((count_ + kQ8Block - 1) / kQ8Block),
        plan(peer_slices(wire.fp8 ? n_blocks : n_vec, k)), gather(k), reduce_grid(k), gather_grid_(k), quantize_grid(k),
        e1(k, nullptr), e2(k, nullptr), eq(k, nullptr) {
    for (int m = 0; m < k; ++m)
      for (int p = 0; p < k; ++p) enable_peer(devs[m], devs[p]);
    std::vector<const u32x4*> outs(k);
    std::vector<u32x4*> outs_w(k);
    std::vector<PeerSlice> out_plan(k);  // slices of the output type
    // output vectors per unit of the plan, and of a whole `out`
    const size_t per_unit = fp8 ? kQ8Block * types.out_elem() / 16 : types.ratio();
    const size_t out_vec = fp8 ? n_blocks * per_unit : n_vec * per_unit;
    for (int m = 0; m < k; ++m) {
      for (int s = 0; s < nsets; ++s) {
        in[s].emplace_back(new DevBuf(devs[m], n_vec * 16));
        srcs[s].p[m] = reinterpret_cast<const u32x4*>(in[s][m]->p);
      }
      if (fp8) {
        packed.emplace_back(new DevBuf(devs[m], q8_packed_vecs(n_blocks) * 16));
        packs.p[m] = reinterpret_cast<const u32x4*>(packed[m]->p);
      }
      if (x2) {
        packed_out.emplace_back(new DevBuf(devs[m], q8_packed_vecs(n_blocks) * 16));
        unpack_set.p[m] = reinterpret_cast<const u32x4*>(packed_out[m]->p);
        unpack_set.first[m] = plan[m].first;
        unpack_set.count[m] = plan[m].count;
      }
      out.emplace_back(new DevBuf(devs[m], out_vec * 16));
      outs[m] = reinterpret_cast<const u32x4*>(out[m]->p);
      outs_w[m] = reinterpret_cast<u32x4*>(out[m]->p);
      out_plan[m] = PeerSlice{plan[m].first * per_unit, plan[m].count * per_unit};
    }
    for (int m = 0; push && m < k; ++m) push_dsts.push_back(peer_push_dsts(outs_w, m));
    try {
      for (int m = 0; m < k; ++m) {
        const int share = device_share(devs, devs[m]);  // as in K6
        const size_t units = twoshot || push ? plan[m].count : (fp8 ? n_blocks : n_vec);
        reduce_grid[m] = peer_reduce_grid(num_cus(devs[m]), blocks_per_cu, share, fp8 ? 2 * units : units);
        quantize_grid[m] = peer_reduce_grid(num_cus(devs[m]), blocks_per_cu, share, n_blocks * 64 / types.in_elem());
        gather_grid_[m] = gather_grid(devs[m], blocks_per_cu, x2 ? k : k - 1, share);
        gather[m] = peer_gather_slices(outs, out_plan, m);
        DeviceGuard g(devs[m]);
        ts.emplace_back(new TimedStream());
        HIP_CHECK(hipEventCreateWithFlags(&e1[m], hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&e2[m], hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&eq[m], hipEventDisableTiming));
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

  // Phase 1 of member m over [v0, v1) of the plan's units: vectors of `in`, or blocks of the packed buffers.
  void reduce(int m, int set, size_t v0, size_t v1) {
    if (v0 == v1 || dry) return;
    u32x4* dst = reinterpret_cast<u32x4*>(out[m]->p);
    if (push && fp8)
      launch_peer_q8_sum_push(types.out_bf16, packs, push_dsts[m], k, q8_exp_vec(n_blocks), v0, v1, scale, reduce_grid[m], ts[m]->s);
    else if (push)
      launch_peer_reduce_push(types, srcs[set], push_dsts[m], k, v0, v1, scale, reduce_grid[m], ts[m]->s);
    else if (x2)
      launch_peer_q8_repack(packs, k, q8_exp_vec(n_blocks), v0, v1, reinterpret_cast<u32x4*>(packed_out[m]->p), scale,
                            reduce_grid[m], ts[m]->s);
    else if (fp8)
      launch_peer_q8_sum(types.out_bf16, packs, k, q8_exp_vec(n_blocks), v0, v1, dst, scale, reduce_grid[m], ts[m]->s);
    else
      launch_peer_reduce(types, srcs[set], k, v0, v1, dst, scale, reduce_grid[m], ts[m]->s);
  }

  void quantize(int m, int set) {
    if (dry) return;
    launch_peer_q8_quantize(types.in_bf16, srcs[set].p[m], reinterpret_cast<u32x4*>(packed[m]->p), q8_exp_vec(n_blocks), 0,
                            n_blocks, count, quantize_grid[m], ts[m]->s);
  }

  // Phase 2 of member m: the other members' slices of their `out`; fp8x2: every slice of the second packed buffers.
  void gather_phase(int m) {
    if (dry) return;
    u32x4* dst = reinterpret_cast<u32x4*>(out[m]->p);
    if (x2)
      launch_peer_q8_unpack(types.out_bf16, unpack_set, k, q8_exp_vec(n_blocks), dst, gather_grid_[m], ts[m]->s);
    else
      launch_peer_gather(gather[m], k - 1, dst, gather_grid_[m], ts[m]->s);
  }

  // One all-reduce of input set `set`, enqueued on every member's stream.  Every e1 / e2 is recorded
  // before any stream is made to wait for it (a wait for an event never recorded is no wait).
  void round(int set) {
    auto wait_others = [&](int m, const std::vector<hipEvent_t>& ev) {
      for (int p = 0; p < k; ++p)
        if (p != m) HIP_CHECK(hipStreamWaitEvent(ts[m]->s, ev[p], 0));
    };
    for (int m = 0; fp8 && m < k; ++m) {
      DeviceGuard g(devs[m]);
      if (rounds_done) wait_others(m, e1);  // last round's phase 1 of every member has read packed[m]
      quantize(m, set);
      HIP_CHECK(hipEventRecord(eq[m], ts[m]->s));
    }
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      if (fp8) wait_others(m, eq);
      if (push) {  // slice m of every `out` is this member's alone and nothing reads an `out`: no event of its own
        reduce(m, set, plan[m].first, plan[m].first + plan[m].count);
        if (fp8) HIP_CHECK(hipEventRecord(e1[m], ts[m]->s));
        continue;
      }
      if (!twoshot) {
        reduce(m, set, 0, fp8 ? n_blocks : n_vec);
        if (fp8) HIP_CHECK(hipEventRecord(e1[m], ts[m]->s));
        continue;
      }
      if (rounds_done) wait_others(m, e2);
      reduce(m, set, plan[m].first, plan[m].first + plan[m].count);
      HIP_CHECK(hipEventRecord(e1[m], ts[m]->s));
    }
    for (int m = 0; twoshot && m < k; ++m) {
      DeviceGuard g(devs[m]);
      wait_others(m, e1);
      gather_phase(m);
      HIP_CHECK(hipEventRecord(e2[m], ts[m]->s));
    }
    ++rounds_done;
  }

  // in[set][m] = pattern(seed_of(set, m)), padding zero.  fp8x2 narrows the pattern: the sum of k patterns in
  // [-8, 7] needs more than the 4 bits a second packing keeps, a sum of values in {-1, 0} does not.
  static unsigned int seed_of(int set, int m) { return 0x243f6a88u ^ (unsigned)(set * 0x9e3779b9u) ^ (unsigned)(m * 7919 + 1); }
  void fill(int set) {
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      const dim3 grid(num_cus(devs[m]) * 4), block(kBlock);
      if (types.in_bf16)
        peer_fill_kernel<uint16_t><<<grid, block>>>((uint16_t*)in[set][m]->p, count, padded(), seed_of(set, m), x2);
      else
        peer_fill_kernel<float><<<grid, block>>>((float*)in[set][m]->p, count, padded(), seed_of(set, m), x2);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipDeviceSynchronize());
    }
  }

  // Every byte the rounds write before anything reads it, set to 0xFF: each member's `out` (NaN in every
  // element as bf16 and as fp32) and the packed buffers of the fp8 wires (NaN codes, the largest exponent).
  // None of them is written between hipMalloc and the first round, and the allocator may hand back a block
  // that an earlier call freed holding the very sums the check looks for.  Before the rounds, synchronised.
  void poison() {
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      HIP_CHECK(hipMemset(out[m]->p, 0xFF, out[m]->bytes));
      if (fp8) HIP_CHECK(hipMemset(packed[m]->p, 0xFF, packed[m]->bytes));
      if (x2) HIP_CHECK(hipMemset(packed_out[m]->p, 0xFF, packed_out[m]->bytes));
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
          peer_check_kernel<uint16_t><<<grid, block>>>((const uint16_t*)out[m]->p, count, padded(), seeds, k, bad, x2);
        else
          peer_check_kernel<float><<<grid, block>>>((const float*)out[m]->p, count, padded(), seeds, k, bad, x2);
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
      if (eq[m]) (void)hipEventDestroy(eq[m]);
      e1[m] = e2[m] = eq[m] = nullptr;
      (void)hipSetDevice(prev);
    }
  }
};

py::dict peer_allreduce(const std::vector<int>& devs, size_t count, const std::string& dtype, const std::string& algo,
                        int iters, int warmup, int blocks_per_cu, const std::string& wire, bool dry_run) {
  const PeerTypes types = peer_types(dtype, "");
  PeerAllreduce::check_args(devs, count, algo);
  const PeerWire w = peer_wire(wire, algo);
  const bool fp8 = w.fp8;
  if (iters < 1 || warmup < 0) throw std::invalid_argument("iters >= 1, warmup >= 0");
  const int k = (int)devs.size();
  MemberTimes t;
  unsigned long long wrong = 0;
  const size_t bytes = count * types.in_elem();
  double quantize_us = 0.0, sum_us = 0.0, gather_us = 0.0;
  {
    py::gil_scoped_release nogil;
    // with more than one round, consecutive rounds alternate between two input sets and the check uses
    // the last round's: a round that ran ahead of the one before it leaves a mix of the two sums
    const int total = warmup + iters;
    PeerAllreduce ar(devs, count, types, algo, total >= 2 ? 2 : 1, blocks_per_cu, 1.0f, w);
    ar.dry = dry_run;
    for (int s = 0; s < ar.nsets; ++s) ar.fill(s);
    ar.poison();
    t = time_member_rounds(devs, ar.ts, warmup, iters, [&](int r) { ar.round(r % ar.nsets); });
    wrong = ar.wrong((total - 1) % ar.nsets);
    if (fp8) {
      // member 0's kernels alone on an idle device, after the check: the same set as the last round,
      // so `out` (fp8x2: its slice of the second packed buffer, then `out`) is rewritten with the same bits
      const int set = (total - 1) % ar.nsets;
      const bool sliced = ar.twoshot || ar.push;
      const size_t a = sliced ? ar.plan[0].first : 0, b = sliced ? a + ar.plan[0].count : ar.n_blocks;
      DeviceGuard g(devs[0]);
      ar.ts[0]->begin();
      for (int i = 0; i < iters; ++i) ar.quantize(0, set);
      quantize_us = ar.ts[0]->end_ms() * 1e3 / iters;
      ar.ts[0]->begin();
      for (int i = 0; i < iters; ++i) ar.reduce(0, set, a, b);
      sum_us = ar.ts[0]->end_ms() * 1e3 / iters;
      if (w.x2) {
        ar.ts[0]->begin();
        for (int i = 0; i < iters; ++i) ar.gather_phase(0);
        gather_us = ar.ts[0]->end_ms() * 1e3 / iters;
      }
    }
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
  r["wire"] = wire;
  r["dry_run"] = dry_run;
  if (fp8) {
    r["quantize_us"] = quantize_us;
    r["sum_us"] = sum_us;
    if (w.x2) r["gather_us"] = gather_us;
  }
  return r;
}

// The same all-reduce on the caller's data: k one-dimensional arrays of equal length (uint16 bit
// patterns for bf16, float32 for fp32) in, the k members' results out, after `rounds` all-reduces of
// the same inputs.  `out_dtype` (none: the inputs') and `scale` select the wide and the scaled reduce.
py::list peer_allreduce_arrays(const std::vector<int>& devs, const std::vector<py::array>& inputs, const std::string& dtype,
                               const std::string& algo, int rounds, const std::optional<std::string>& out_dtype, float scale,
                               const std::string& wire) {
  if (inputs.size() != devs.size()) throw std::invalid_argument("one input array per member");
  const size_t count = inputs.empty() ? 0 : (size_t)inputs[0].size();
  const PeerTypes types = peer_types(dtype, out_dtype.value_or(""));
  PeerAllreduce::check_args(devs, count, algo);
  const PeerWire w = peer_wire(wire, algo);
  const bool fp8 = w.fp8;
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
    PeerAllreduce ar(devs, count, types, algo, 1, kBlocksPerCU, scale, w);
    for (int m = 0; m < k; ++m) {
      DeviceGuard g(devs[m]);
      // the fp8 wire masks what lies past the count itself: its padding is made non-zero on purpose
      HIP_CHECK(hipMemset(ar.in[0][m]->p, fp8 ? 0x7b : 0, ar.n_vec * 16));
      HIP_CHECK(hipMemcpy(ar.in[0][m]->p, from[m], count * types.in_elem(), hipMemcpyHostToDevice));
      HIP_CHECK(hipDeviceSynchronize());
    }
    ar.poison();
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

// The quantize kernel alone on one array (uint16 bit patterns for bf16, float32 for fp32): the codes
// (uint8, 32 per block, element order) and the block exponents (int32, unbiased) it wrote, in logical
// order.  The window is filled with a non-zero byte first, so what lies past the count is not zero.
// `count` (none: the array's size) is the call's element count: the array's elements at and past it
// lie in the window after the count, as far as the count's last block reaches.
// `residual` (none: the plain kernel, and a 2-tuple): float32, one value per element of the count's whole
// blocks; the feedback form then runs on it and the residual it left comes back as a third array.
py::tuple peer_q8_quantize(int dev, const py::array& array, const std::string& dtype, const py::object& count_arg,
                           const py::object& residual_arg) {
  const PeerTypes types = peer_types(dtype, "");
  check_dev(dev);
  const py::dtype want = types.in_bf16 ? py::dtype::of<uint16_t>() : py::dtype::of<float>();
  if (array.ndim() != 1 || array.size() < 1 || !array.dtype().is(want))
    throw std::invalid_argument("a one-dimensional, non-empty array, uint16 (bf16) or float32 (fp32)");
  const size_t count = count_arg.is_none() ? (size_t)array.size() : count_arg.cast<size_t>();
  if (count < 1 || count > (size_t)array.size()) throw std::invalid_argument("1 <= count <= the array's size");
  if (count > PeerAllreduce::kMaxCount) throw std::invalid_argument("count <= 64 Mi elements");
  const py::array src = py::array::ensure(array, py::array::c_style);
  const size_t n_blocks = (count + kQ8Block - 1) / kQ8Block, in_bytes = n_blocks * kQ8Block * types.in_elem();
  const bool ef = !residual_arg.is_none();
  const size_t res_bytes = n_blocks * kQ8Block * sizeof(float);
  py::array res_in;
  if (ef) {
    const py::array given = residual_arg.cast<py::array>();
    if (given.ndim() != 1 || (size_t)given.size() != n_blocks * kQ8Block || !given.dtype().is(py::dtype::of<float>()))
      throw std::invalid_argument("residual: a one-dimensional float32 array, one value per element of the count's whole blocks");
    res_in = py::array::ensure(given, py::array::c_style);
  }
  py::array_t<uint8_t> codes((py::ssize_t)(n_blocks * kQ8Block));
  py::array_t<int32_t> exps((py::ssize_t)n_blocks);
  py::array_t<float> res_out((py::ssize_t)(ef ? n_blocks * kQ8Block : 0));
  std::vector<uint8_t> biased(n_blocks);
  const void* from = src.data();
  const void* res_from = ef ? res_in.data() : nullptr;
  void* to = codes.mutable_data();
  void* res_to = res_out.mutable_data();
  {
    py::gil_scoped_release nogil;
    DeviceGuard g(dev);
    DevBuf win(dev, in_bytes), packed(dev, q8_packed_vecs(n_blocks) * 16);
    std::unique_ptr<DevBuf> residual;
    HIP_CHECK(hipMemset(win.p, 0x7b, in_bytes));
    HIP_CHECK(hipMemcpy(win.p, from, std::min((size_t)array.size() * types.in_elem(), in_bytes), hipMemcpyHostToDevice));
    const int grid = peer_reduce_grid(num_cus(dev), kBlocksPerCU, 1, in_bytes / 16);
    if (ef) {
      residual.reset(new DevBuf(dev, res_bytes));
      HIP_CHECK(hipMemcpy(residual->p, res_from, res_bytes, hipMemcpyHostToDevice));
      launch_peer_q8_quantize_ef(types.in_bf16, (const u32x4*)win.p, (u32x4*)packed.p, q8_exp_vec(n_blocks), 0, n_blocks, count,
                                 (u32x4*)residual->p, grid, nullptr);
    } else {
      launch_peer_q8_quantize(types.in_bf16, (const u32x4*)win.p, (u32x4*)packed.p, q8_exp_vec(n_blocks), 0, n_blocks, count, grid,
                              nullptr);
    }
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(to, packed.p, n_blocks * kQ8Block, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(biased.data(), (const char*)packed.p + q8_exp_vec(n_blocks) * 16, n_blocks, hipMemcpyDeviceToHost));
    if (ef) HIP_CHECK(hipMemcpy(res_to, residual->p, res_bytes, hipMemcpyDeviceToHost));
  }
  int32_t* e = exps.mutable_data();
  for (size_t b = 0; b < n_blocks; ++b) e[b] = (int32_t)biased[b] - kQ8Bias;
  if (ef) return py::make_tuple(codes, exps, res_out);
  return py::make_tuple(codes, exps);
}

}  // namespace
