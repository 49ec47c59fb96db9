// One rank's device state for the peer communicator (parallel/peer_comm.py, backend="device").
// Host code only: it launches the K7 kernels of peer_allreduce.h and peer_q8.h through the launch plan of
// peer_driver.h, as PeerAllreduce does, and the ZeRO-1 kernels of peer_zero1.h, and adds no kernel of its own.
// The push launches (reduce_push, reduce_q8_push, reduce_adamw_push, reduce_q8_adamw_push) store into the
// peers' outs, which is why those are held mutable.
//
// A rank owns a window (inputs, `capacity` bytes), an out (results, twice that: the wide form writes
// two vectors per input vector), a packed buffer (the fp8 wire's form of the window, sized for a window
// full of bf16: capacity / 64 blocks), a second packed buffer of that size (the fp8x2 wire's form of the rank's
// slice of a sum, which its peers gather from) and one non-blocking stream on its device.  A rank that packs with
// error feedback also owns a residual (fp32, one value per element of a window full of bf16: twice the capacity),
// allocated on its first feedback call; it is the rank's alone, never published and no part of open_peers.
// The same holds for the ZeRO-1 optimizer state (zero1_alloc): master, m and v, fp32, of the rank's slice of the
// parameters alone, read and written by the rank's own fused step (reduce_adamw_push, reduce_q8_adamw_push), and
// for the stash of the clipped step (zero1_stash_alloc): the scaled gradient sum that reduce_sqnorm_stash or
// reduce_q8_sqnorm_stash leaves for adamw_push, with the sum-of-squares partials the host adds up in between.
// reduce_sqnorm_accum and reduce_q8_sqnorm_accum add to that stash instead of overwriting it: between the first
// micro-batch of an accumulation and the step that ends it the stash is the rank's fp32 gradient accumulator.
// Ranks are threads of one
// process, so a peer's buffer is reached through its plain device address and, across devices,
// hipDeviceEnablePeerAccess: no IPC call.  A PeerRank is used by one thread.  Nothing here waits on
// the GPU for another rank: no event is shared between ranks and no kernel spins, so ordering between
// ranks is the caller's (synchronize(), then a host barrier).  Every HIP call is made with the GIL
// released, since a rank blocked in hipStreamSynchronize must not keep another from its barrier.
#pragma once
#include <array>
#include <mutex>

#include "peer_driver.h"
#include "peer_zero1.h"

namespace {

// Allocation, free and peer enabling of every rank, one at a time.
std::mutex& peer_rank_mutex() {
  static std::mutex m;
  return m;
}

class PeerRank {
 public:
  // `max_ctas` (0: no cap) bounds the grid of every launch that peer_reduce_grid sizes: the reduce, the push, the fp8
  // sum and its push, the repack, the quantize with and without feedback, the two fused ZeRO-1 kernels and both
  // launches of the clipped step, the adding launch of an accumulation among them.  Those kernels walk their range with any grid, and every element is computed by one
  // lane from the same operands whichever block holds it, so the cap changes no result bit (the clipped step's norm
  // excepted: its summation order follows the grid).  The gather and unpack launches keep their grids, which must stay
  // a multiple of the source count.
  PeerRank(int dev, int rank, int world, size_t capacity_bytes, int blocks_per_cu, int max_ctas = 0)
      : dev_(dev), rank_(rank), world_(world), cap_(capacity_bytes), blocks_per_cu_(std::max(1, blocks_per_cu)), max_ctas_(max_ctas) {
    if (max_ctas < 0) throw std::invalid_argument("max_ctas >= 0 (0: no cap)");
    if (world < 2 || world > kMaxSrc) throw std::invalid_argument("2..16 ranks");
    if (rank < 0 || rank >= world) throw std::invalid_argument("rank out of range");
    if (capacity_bytes < 16 || capacity_bytes % 16) throw std::invalid_argument("capacity_bytes must be a positive multiple of 16");
    py::gil_scoped_release nogil;
    check_dev(dev);
    cus_ = num_cus(dev);
    try {
      {
        std::lock_guard<std::mutex> lock(peer_rank_mutex());
        window_.reset(new DevBuf(dev, cap_));
        out_.reset(new DevBuf(dev, 2 * cap_));
        packed_.reset(new DevBuf(dev, packed_bytes()));
        packed_out_.reset(new DevBuf(dev, packed_bytes()));
      }
      DeviceGuard g(dev);
      HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
      HIP_CHECK(hipMemsetAsync(window_->p, 0, cap_, stream_));
      HIP_CHECK(hipMemsetAsync(out_->p, 0, 2 * cap_, stream_));
      HIP_CHECK(hipMemsetAsync(packed_->p, 0, packed_bytes(), stream_));
      HIP_CHECK(hipMemsetAsync(packed_out_->p, 0, packed_bytes(), stream_));
      HIP_CHECK(hipStreamSynchronize(stream_));
    } catch (...) {
      release_locked();
      throw;
    }
  }
  ~PeerRank() {
    if (released_) return;
    if (Py_IsInitialized() && PyGILState_Check()) {
      py::gil_scoped_release nogil;
      release_locked();
    } else {
      release_locked();
    }
  }
  PeerRank(const PeerRank&) = delete;
  PeerRank& operator=(const PeerRank&) = delete;

  uintptr_t window_ptr() const { return reinterpret_cast<uintptr_t>(live().window_->p); }
  uintptr_t out_ptr() const { return reinterpret_cast<uintptr_t>(live().out_->p); }
  uintptr_t packed_ptr() const { return reinterpret_cast<uintptr_t>(live().packed_->p); }
  uintptr_t packed_out_ptr() const { return reinterpret_cast<uintptr_t>(live().packed_out_->p); }
  size_t capacity_bytes() const { return cap_; }
  size_t max_blocks() const { return cap_ / (kQ8Block * 2); }  // blocks of 32 bf16 elements the window holds
  size_t packed_bytes() const { return std::max<size_t>(16, q8_packed_vecs(max_blocks()) * 16); }
  size_t residual_bytes() const { return residual_ ? 2 * cap_ : 0; }  // 0 until the first feedback call
  size_t zero1_elems() const { return zero1_n_; }  // floats of each of master, m and v; 0 until zero1_alloc
  size_t stash_elems() const { return stash_ ? zero1_n_ : 0; }  // floats of the clipped step's stash; 0 until zero1_stash_alloc
  size_t zero1_bytes() const { return (3 * zero1_n_ + stash_elems()) * sizeof(float); }  // the partials, a few KiB, are not counted
  size_t launches() const { return launches_; }
  int last_grid() const { return last_grid_; }  // blocks of the most recent launch; 0 before any
  bool released() const { return released_; }

  // Every rank's device and buffer addresses, this rank's own included (and checked to be its own).
  // A peer's address must be the base of a device allocation of this process on the device it names,
  // at least as large as this rank's buffers: the kernels index a peer's buffer as they index their own,
  // and a push (reduce_push, reduce_q8_push) stores into the peers' outs.
  // `packeds` is optional: without the peers' packed buffers the fp8 phases stay unavailable; so is
  // `packed_outs`, the peers' second packed buffers, without which the fp8x2 phases stay unavailable.
  void open_peers(const std::vector<int>& devices, const std::vector<uintptr_t>& windows, const std::vector<uintptr_t>& outs,
                  const std::optional<std::vector<uintptr_t>>& packeds = std::nullopt,
                  const std::optional<std::vector<uintptr_t>>& packed_outs = std::nullopt) {
    live();
    const size_t k = (size_t)world_;
    if (devices.size() != k || windows.size() != k || outs.size() != k) throw std::invalid_argument("one device, window and out per rank");
    if ((packeds && packeds->size() != k) || (packed_outs && packed_outs->size() != k))
      throw std::invalid_argument("one packed buffer per rank");
    if (packed_outs && !packeds) throw std::invalid_argument("the second packed buffers come with the first");
    if (devices[rank_] != dev_ || windows[rank_] != window_ptr() || outs[rank_] != out_ptr() ||
        (packeds && (*packeds)[rank_] != packed_ptr()) || (packed_outs && (*packed_outs)[rank_] != packed_out_ptr()))
      throw std::invalid_argument("this rank's own entry is not its device and buffers");
    check_devs(devices);
    for (size_t p = 0; p < k; ++p) {
      check_allocation(windows[p], devices[p], cap_);
      check_allocation(outs[p], devices[p], 2 * cap_);
      if (packeds) check_allocation((*packeds)[p], devices[p], packed_bytes());
      if (packed_outs) check_allocation((*packed_outs)[p], devices[p], packed_bytes());
    }
    {
      std::lock_guard<std::mutex> lock(peer_rank_mutex());
      for (size_t p = 0; p < k; ++p) enable_peer(dev_, devices[p]);
    }
    share_ = device_share(devices, dev_);  // as the members of PeerAllreduce do
    outs_.resize(k);
    packed_outs_.assign(k, nullptr);
    for (size_t p = 0; p < k; ++p) {
      windows_.p[p] = reinterpret_cast<const u32x4*>(windows[p]);
      outs_[p] = reinterpret_cast<u32x4*>(outs[p]);
      packeds_.p[p] = packeds ? reinterpret_cast<const u32x4*>((*packeds)[p]) : nullptr;
      if (packed_outs) packed_outs_[p] = reinterpret_cast<const u32x4*>((*packed_outs)[p]);
    }
    open_ = true;
    open_q8_ = packeds.has_value();
    open_q8x2_ = packed_outs.has_value();
  }

  void close_peers() {
    windows_ = packeds_ = SrcSet{};
    outs_.clear();
    packed_outs_.clear();
    open_ = open_q8_ = open_q8x2_ = false;
  }

  // out[v0, v1) of this rank = scale x the sum over ranks of window[v0, v1), vectors of the input type
  // (the wide form writes out[2 * v0, 2 * v1)).
  void reduce(size_t v0, size_t v1, const std::string& in_dtype, const std::string& out_dtype, float scale) {
    const PeerTypes t = peer_types(in_dtype, out_dtype);
    need_peers();
    if (v0 > v1 || v1 > cap_ / 16) throw std::invalid_argument("reduce: vectors past the end of the window");
    if (v1 * t.ratio() > 2 * cap_ / 16) throw std::invalid_argument("reduce: vectors past the end of out");
    if (v0 == v1) return;
    const int grid = reduce_grid(v1 - v0);
    DeviceGuard g(dev_);
    launch_peer_reduce(t, windows_, world_, v0, v1, reinterpret_cast<u32x4*>(out_->p), scale, grid, stream_);
    ++launches_;
  }

  // The push form of reduce: the same sum of window[v0, v1) of every rank, stored to vectors [v0, v1) of
  // every rank's out (the wide form: [2 * v0, 2 * v1)), this rank's own first and the others in ring order.
  // One launch.  The caller gives every rank a range of its own: the ranges of one epoch must not overlap.
  void reduce_push(size_t v0, size_t v1, const std::string& in_dtype, const std::string& out_dtype, float scale) {
    const PeerTypes t = peer_types(in_dtype, out_dtype);
    need_peers();
    if (v0 > v1 || v1 > cap_ / 16) throw std::invalid_argument("reduce_push: vectors past the end of the window");
    if (v1 * t.ratio() > 2 * cap_ / 16) throw std::invalid_argument("reduce_push: vectors past the end of out");
    if (v0 == v1) return;
    const int grid = reduce_grid(v1 - v0);
    DeviceGuard g(dev_);
    launch_peer_reduce_push(t, windows_, peer_push_dsts(outs_, rank_), world_, v0, v1, scale, grid, stream_);
    ++launches_;
  }

  // The fp8 wire's first phase: blocks [b0, b1) of this rank's window (32 elements of `in_dtype` each,
  // elements at or past `count` taken as zero) to the same blocks of its packed buffer.  With
  // `error_feedback` the rank's residual of those blocks is added first and rewritten with what the packing
  // dropped (element i of the window has float i of the residual); the first such call allocates it, zeroed.
  // One launch either way.
  void quantize(size_t b0, size_t b1, size_t count, const std::string& in_dtype, bool error_feedback = false) {
    const PeerTypes t = peer_types(in_dtype, "");
    need_q8();
    if (b0 > b1 || b1 * kQ8Block * t.in_elem() > cap_) throw std::invalid_argument("quantize: blocks past the end of the window");
    if (b1 > max_blocks()) throw std::invalid_argument("quantize: blocks past the end of the packed buffer");  // and of the residual
    if (b0 == b1) return;
    const int grid = reduce_grid((b1 - b0) * kQ8Block * t.in_elem() / 16);
    DeviceGuard g(dev_);
    if (error_feedback) {
      need_residual();
      launch_peer_q8_quantize_ef(t.in_bf16, reinterpret_cast<const u32x4*>(window_->p), reinterpret_cast<u32x4*>(packed_->p),
                                 q8_exp_vec(max_blocks()), b0, b1, count, reinterpret_cast<u32x4*>(residual_->p), grid, stream_);
    } else {
      launch_peer_q8_quantize(t.in_bf16, reinterpret_cast<const u32x4*>(window_->p), reinterpret_cast<u32x4*>(packed_->p),
                              q8_exp_vec(max_blocks()), b0, b1, count, grid, stream_);
    }
    ++launches_;
  }

  // The residual back to zero: one memset on the stream, nothing if it was never allocated.
  void reset_residual() {
    live();
    if (!residual_) return;
    DeviceGuard g(dev_);
    HIP_CHECK(hipMemsetAsync(residual_->p, 0, 2 * cap_, stream_));
  }

  // Floats [first_elem, first_elem + n) of the residual to `dst`, after everything on the stream; zeros
  // while it is unallocated, which is what it then stands for.
  void read_residual(float* dst, size_t first_elem, size_t n) {
    live();
    if (first_elem > cap_ / 2 || n > cap_ / 2 - first_elem) throw std::invalid_argument("read_residual: past the end of the residual");
    DeviceGuard g(dev_);
    if (!residual_)
      std::fill(dst, dst + n, 0.f);
    else if (n)
      HIP_CHECK(hipMemcpyAsync(dst, static_cast<const float*>(residual_->p) + first_elem, n * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  // Host floats into the residual from `first_elem` on (a restored checkpoint; the tests' starting state),
  // allocating it if need be.  On the rank's stream; returns once the host floats have been read.
  void write_residual(const float* src, size_t n, size_t first_elem) {
    live();
    if (first_elem > cap_ / 2 || n > cap_ / 2 - first_elem) throw std::invalid_argument("write_residual: past the end of the residual");
    if (!n) return;
    DeviceGuard g(dev_);
    need_residual();
    HIP_CHECK(hipMemcpyAsync(static_cast<float*>(residual_->p) + first_elem, src, n * sizeof(float), hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  // The ZeRO-1 optimizer state of this rank's slice: master, m and v, `n_elems` floats each (whole vectors of
  // eight; 0 frees it), zero-filled on the stream.  A second call replaces what the first allocated.
  void zero1_alloc(size_t n_elems) {
    live();
    if (n_elems % 8) throw std::invalid_argument("zero1_alloc: whole vectors of 8 elements");
    if (n_elems > cap_ / 2) throw std::invalid_argument("zero1_alloc: more elements than a window full of bf16");
    DeviceGuard g(dev_);
    HIP_CHECK(hipStreamSynchronize(stream_));  // no launch still uses the state this call frees
    {
      std::lock_guard<std::mutex> lock(peer_rank_mutex());
      zero1_.reset();
      stash_.reset();  // the stash has the state's size: the next clipped step makes a new one
      zero1_n_ = 0;
      if (n_elems) zero1_.reset(new DevBuf(dev_, 3 * n_elems * sizeof(float)));
    }
    zero1_n_ = n_elems;
    if (n_elems) HIP_CHECK(hipMemsetAsync(zero1_->p, 0, 3 * n_elems * sizeof(float), stream_));
  }

  // Host floats into floats [first, first + n) of master (which = 0), m (1) or v (2): the initial weights, a
  // restored checkpoint.  On the rank's stream; returns once the host floats have been read.
  void zero1_write_state(int which, const float* src, size_t first, size_t n) {
    float* dst = zero1_ptr(which, first, n, "zero1_write_state");
    if (!n) return;
    DeviceGuard g(dev_);
    HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyHostToDevice, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  // Floats [first, first + n) of master, m or v (which = 3: of the stash, once it exists) to `dst`, after
  // everything on the stream.
  void zero1_read_state(int which, float* dst, size_t first, size_t n) {
    const float* src = which == 3 ? stash_ptr(first, n) : zero1_ptr(which, first, n, "zero1_read_state");
    DeviceGuard g(dev_);
    if (n) HIP_CHECK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  // The ZeRO-1 step on the native wire: scale x the sum over ranks of vectors [v0, v1) of their bf16 windows is
  // the gradient of state floats [0, 8 (v1 - v0)); AdamW with `hyper` (the host form's eight: lr, beta1, beta2,
  // eps, weight_decay, grad_scale, bias_c1, bias_c2) updates them, and the new bf16 weights go to vectors
  // [v0, v1) of every rank's out, in reduce_push's order.  One launch; ranges of one epoch must not overlap.
  void reduce_adamw_push(size_t v0, size_t v1, float scale, const std::array<float, 8>& hyper) {
    need_peers();
    if (v0 > v1 || v1 > cap_ / 16) throw std::invalid_argument("reduce_adamw_push: vectors past the end of the window");
    if (8 * (v1 - v0) > zero1_n_) throw std::invalid_argument("reduce_adamw_push: more vectors than zero1_alloc made state for");
    if (v0 == v1) return;
    const int grid = reduce_grid(v1 - v0);
    DeviceGuard g(dev_);
    launch_peer_reduce_adamw_push(windows_, peer_push_dsts(outs_, rank_), world_, v0, v1, scale, zero1_state(0), zero1_state(1),
                                  zero1_state(2), zero1_hyper(hyper), grid, stream_);
    ++launches_;
  }

  // The same step on the fp8 wire: blocks [b0, b1) of every rank's packed buffer, state floats
  // [0, 32 (b1 - b0)), the weights to blocks [b0, b1) of every rank's out.
  void reduce_q8_adamw_push(size_t b0, size_t b1, float scale, const std::array<float, 8>& hyper) {
    need_q8();
    if (b0 > b1 || b1 > max_blocks()) throw std::invalid_argument("reduce_q8_adamw_push: blocks past the end of the packed buffer");
    if (kQ8Block * (b1 - b0) > zero1_n_) throw std::invalid_argument("reduce_q8_adamw_push: more blocks than zero1_alloc made state for");
    if (b0 == b1) return;
    const int grid = reduce_grid(2 * (b1 - b0));
    DeviceGuard g(dev_);
    launch_peer_q8_sum_adamw_push(packeds_, peer_push_dsts(outs_, rank_), world_, q8_exp_vec(max_blocks()), b0, b1, scale, zero1_state(0),
                                  zero1_state(1), zero1_state(2), zero1_hyper(hyper), grid, stream_);
    ++launches_;
  }

  // The clipped ZeRO-1 step's stash: one float per float of master, the scaled gradient sum between the step's two
  // launches, with one sum-of-squares partial per block of the first.  Allocated on first call, zeroed on the
  // stream; nothing for an empty state.  zero1_alloc frees it.  The caller makes this call outside a barrier epoch.
  void zero1_stash_alloc() {
    live();
    if (stash_ || !zero1_n_) return;
    DeviceGuard g(dev_);
    {
      std::lock_guard<std::mutex> lock(peer_rank_mutex());
      stash_.reset(new DevBuf(dev_, zero1_n_ * sizeof(float)));
      if (!parts_) parts_.reset(new DevBuf(dev_, max_grid() * sizeof(float)));
    }
    HIP_CHECK(hipMemsetAsync(stash_->p, 0, zero1_n_ * sizeof(float), stream_));
  }

  // Launch 1 of the clipped step on the native wire: stash floats [0, 8 (v1 - v0)) = scale x the sum over ranks of
  // vectors [v0, v1) of their bf16 windows.  Returns the sum of their squares: the blocks' fp32 partials, copied to
  // the host after the launch and added in float64 in index order, so the call synchronises the stream.  An empty
  // range launches nothing and returns 0.
  double reduce_sqnorm_stash(size_t v0, size_t v1, float scale) {
    need_peers();
    if (v0 > v1 || v1 > cap_ / 16) throw std::invalid_argument("reduce_sqnorm_stash: vectors past the end of the window");
    if (8 * (v1 - v0) > stash_elems()) throw std::invalid_argument("reduce_sqnorm_stash: more vectors than the stash holds");
    if (v0 == v1) return 0.0;
    const int grid = reduce_grid(v1 - v0);
    DeviceGuard g(dev_);
    launch_peer_reduce_sqnorm_stash(windows_, world_, v0, v1, scale, static_cast<float*>(stash_->p), static_cast<float*>(parts_->p), grid,
                                    stream_);
    ++launches_;
    return sum_parts(grid);
  }

  // The same on the fp8 wire: blocks [b0, b1) of every rank's packed buffer, stash floats [0, 32 (b1 - b0)).
  double reduce_q8_sqnorm_stash(size_t b0, size_t b1, float scale) {
    need_q8();
    if (b0 > b1 || b1 > max_blocks()) throw std::invalid_argument("reduce_q8_sqnorm_stash: blocks past the end of the packed buffer");
    if (kQ8Block * (b1 - b0) > stash_elems()) throw std::invalid_argument("reduce_q8_sqnorm_stash: more blocks than the stash holds");
    if (b0 == b1) return 0.0;
    const int grid = reduce_grid(2 * (b1 - b0));
    DeviceGuard g(dev_);
    launch_peer_q8_sum_sqnorm_stash(packeds_, world_, q8_exp_vec(max_blocks()), b0, b1, scale, static_cast<float*>(stash_->p),
                                    static_cast<float*>(parts_->p), grid, stream_);
    ++launches_;
    return sum_parts(grid);
  }

  // The adding form of launch 1, for a gradient accumulated over micro-batches: stash floats [0, 8 (v1 - v0)) +=
  // scale x the sum over ranks of vectors [v0, v1) of their bf16 windows, one fp32 multiply and one fp32 add per
  // element.  Returns the sum of the squares of the totals it stored, as reduce_sqnorm_stash does.
  double reduce_sqnorm_accum(size_t v0, size_t v1, float scale) {
    need_peers();
    if (v0 > v1 || v1 > cap_ / 16) throw std::invalid_argument("reduce_sqnorm_accum: vectors past the end of the window");
    if (8 * (v1 - v0) > stash_elems()) throw std::invalid_argument("reduce_sqnorm_accum: more vectors than the stash holds");
    if (v0 == v1) return 0.0;
    const int grid = reduce_grid(v1 - v0);
    DeviceGuard g(dev_);
    launch_peer_reduce_sqnorm_accum(windows_, world_, v0, v1, scale, static_cast<float*>(stash_->p), static_cast<float*>(parts_->p), grid,
                                    stream_);
    ++launches_;
    return sum_parts(grid);
  }

  // The same on the fp8 wire: blocks [b0, b1) of every rank's packed buffer, stash floats [0, 32 (b1 - b0)).
  double reduce_q8_sqnorm_accum(size_t b0, size_t b1, float scale) {
    need_q8();
    if (b0 > b1 || b1 > max_blocks()) throw std::invalid_argument("reduce_q8_sqnorm_accum: blocks past the end of the packed buffer");
    if (kQ8Block * (b1 - b0) > stash_elems()) throw std::invalid_argument("reduce_q8_sqnorm_accum: more blocks than the stash holds");
    if (b0 == b1) return 0.0;
    const int grid = reduce_grid(2 * (b1 - b0));
    DeviceGuard g(dev_);
    launch_peer_q8_sum_sqnorm_accum(packeds_, world_, q8_exp_vec(max_blocks()), b0, b1, scale, static_cast<float*>(stash_->p),
                                    static_cast<float*>(parts_->p), grid, stream_);
    ++launches_;
    return sum_parts(grid);
  }

  // Launch 2 of the clipped step, either wire: AdamW with `hyper` on state floats [0, 8 (v1 - v0)), the stash as the
  // gradient, the new bf16 weights to vectors [v0, v1) of every rank's out, in reduce_push's order.  It reads
  // rank-local memory only.  One launch; ranges of one epoch must not overlap.
  void adamw_push(size_t v0, size_t v1, const std::array<float, 8>& hyper) {
    need_peers();
    if (v0 > v1 || v1 > cap_ / 16) throw std::invalid_argument("adamw_push: vectors past the end of a window's worth of out");
    if (8 * (v1 - v0) > stash_elems()) throw std::invalid_argument("adamw_push: more vectors than the stash holds");
    if (v0 == v1) return;
    const int grid = reduce_grid(v1 - v0);
    DeviceGuard g(dev_);
    launch_peer_adamw_push(peer_push_dsts(outs_, rank_), world_, v0, v1, static_cast<const float*>(stash_->p), zero1_state(0),
                           zero1_state(1), zero1_state(2), zero1_hyper(hyper), grid, stream_);
    ++launches_;
  }

  // Blocks [b0, b1) of this rank's out (whole blocks of `out_dtype`) = scale x the sum over ranks of the
  // same blocks of their packed buffers.
  void reduce_q8(size_t b0, size_t b1, const std::string& out_dtype, float scale) {
    const PeerTypes t = peer_types("bf16", out_dtype);  // the packed form carries no input type: any output is allowed
    need_q8();
    if (b0 > b1 || b1 > max_blocks()) throw std::invalid_argument("reduce_q8: blocks past the end of the packed buffer");
    if (b1 * kQ8Block * t.out_elem() > 2 * cap_) throw std::invalid_argument("reduce_q8: blocks past the end of out");
    if (b0 == b1) return;
    const int grid = reduce_grid(2 * (b1 - b0));
    DeviceGuard g(dev_);
    launch_peer_q8_sum(t.out_bf16, packeds_, world_, q8_exp_vec(max_blocks()), b0, b1, reinterpret_cast<u32x4*>(out_->p), scale, grid,
                       stream_);
    ++launches_;
  }

  // The push form of reduce_q8: the same sum, stored to blocks [b0, b1) of every rank's out, in reduce_push's order.
  void reduce_q8_push(size_t b0, size_t b1, const std::string& out_dtype, float scale) {
    const PeerTypes t = peer_types("bf16", out_dtype);  // as reduce_q8
    need_q8();
    if (b0 > b1 || b1 > max_blocks()) throw std::invalid_argument("reduce_q8_push: blocks past the end of the packed buffer");
    if (b1 * kQ8Block * t.out_elem() > 2 * cap_) throw std::invalid_argument("reduce_q8_push: blocks past the end of out");
    if (b0 == b1) return;
    const int grid = reduce_grid(2 * (b1 - b0));
    DeviceGuard g(dev_);
    launch_peer_q8_sum_push(t.out_bf16, packeds_, peer_push_dsts(outs_, rank_), world_, q8_exp_vec(max_blocks()), b0, b1, scale, grid,
                            stream_);
    ++launches_;
  }

  // Phase 1 of the fp8x2 two-shot: blocks [b0, b1) of this rank's second packed buffer = the packed form of
  // scale x the sum over ranks of the same blocks of their packed buffers.
  void repack_q8(size_t b0, size_t b1, float scale) {
    need_q8x2();
    if (b0 > b1 || b1 > max_blocks()) throw std::invalid_argument("repack_q8: blocks past the end of the packed buffers");
    if (b0 == b1) return;
    const int grid = reduce_grid(2 * (b1 - b0));
    DeviceGuard g(dev_);
    launch_peer_q8_repack(packeds_, world_, q8_exp_vec(max_blocks()), b0, b1, reinterpret_cast<u32x4*>(packed_out_->p), scale, grid,
                          stream_);
    ++launches_;
  }

  // Phase 2 of the fp8x2 two-shot: blocks [a, b) of the second packed buffer of rank p, widened to the same
  // blocks of this rank's out (whole blocks of `out_dtype`), for every p, this rank included.  One launch;
  // slices may be empty.
  void unpack_q8(const std::vector<std::pair<size_t, size_t>>& slices, const std::string& out_dtype) {
    const PeerTypes t = peer_types("bf16", out_dtype);  // as reduce_q8: the packed form carries no input type
    need_q8x2();
    if (slices.size() != (size_t)world_) throw std::invalid_argument("unpack_q8: one slice per rank");
    SliceSet sl{};
    for (int p = 0; p < world_; ++p) {
      const size_t a = slices[p].first, b = slices[p].second;
      if (a > b || b > max_blocks()) throw std::invalid_argument("unpack_q8: blocks past the end of the packed buffers");
      if (b * kQ8Block * t.out_elem() > 2 * cap_) throw std::invalid_argument("unpack_q8: blocks past the end of out");
      sl.p[p] = packed_outs_[p];
      sl.first[p] = a;
      sl.count[p] = b - a;
    }
    DeviceGuard g(dev_);
    last_grid_ = gather_grid_cus(cus_, blocks_per_cu_, world_, share_);
    launch_peer_q8_unpack(t.out_bf16, sl, world_, q8_exp_vec(max_blocks()), reinterpret_cast<u32x4*>(out_->p), last_grid_, stream_);
    ++launches_;
  }

  // Phase 2 of a two-shot: vectors [a, b) of out of rank p, to the same vectors of this rank's out, for
  // every p but this rank.  One launch; slices may be empty.
  void gather(const std::vector<std::pair<size_t, size_t>>& slices) {
    need_peers();
    if (slices.size() != (size_t)world_) throw std::invalid_argument("gather: one slice per rank");
    std::vector<PeerSlice> plan(world_);
    for (int p = 0; p < world_; ++p) {
      const size_t a = slices[p].first, b = slices[p].second;
      if (a > b || b > 2 * cap_ / 16) throw std::invalid_argument("gather: slice past the end of out");
      plan[p] = PeerSlice{a, b - a};
    }
    launch_gather(peer_gather_slices(std::vector<const u32x4*>(outs_.begin(), outs_.end()), plan, rank_), world_ - 1);
  }

  // All-gather: vectors [p * n_vec, (p + 1) * n_vec) of rank p's window to the same vectors of this
  // rank's out, for every p, this rank included.  One launch.
  void gather_windows(size_t n_vec) {
    need_peers();
    if (n_vec > cap_ / 16 / (size_t)world_) throw std::invalid_argument("gather_windows: slices past the end of the window");
    SliceSet sl{};
    for (int p = 0; p < world_; ++p) {
      sl.p[p] = windows_.p[p];
      sl.first[p] = (size_t)p * n_vec;
      sl.count[p] = n_vec;
    }
    launch_gather(sl, world_);
  }

  // Host bytes into the window from `first_byte` on, the rest of the last 16-byte vector zeroed (the
  // kernels assume zero padding).  On the rank's stream; returns once the host bytes have been read.
  void write_host(const void* src, size_t nbytes, size_t first_byte) {
    live();
    const size_t padded = (nbytes + 15) / 16 * 16;
    if (first_byte % 16 || first_byte > cap_ || padded > cap_ - first_byte)
      throw std::invalid_argument("write_host: past the end of the window, or first_byte is no multiple of 16");
    if (!nbytes) return;
    DeviceGuard g(dev_);
    char* dst = static_cast<char*>(window_->p) + first_byte;
    HIP_CHECK(hipMemcpyAsync(dst, src, nbytes, hipMemcpyHostToDevice, stream_));
    if (padded > nbytes) HIP_CHECK(hipMemsetAsync(dst + nbytes, 0, padded - nbytes, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  // Bytes [first_byte, first_byte + nbytes) of out to `dst`, after everything on the stream.
  void read_host(void* dst, size_t first_byte, size_t nbytes) {
    live();
    if (first_byte > 2 * cap_ || nbytes > 2 * cap_ - first_byte) throw std::invalid_argument("read_host: past the end of out");
    DeviceGuard g(dev_);
    if (nbytes) HIP_CHECK(hipMemcpyAsync(dst, static_cast<const char*>(out_->p) + first_byte, nbytes, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  void synchronize() {
    live();
    DeviceGuard g(dev_);
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  // Synchronises, destroys the stream, frees the buffers.  Idempotent.  The caller must know that no
  // peer still reads this rank's buffers.
  void release() { release_locked(); }

 private:
  const PeerRank& live() const {
    if (released_) throw std::runtime_error("the PeerRank is released");
    return *this;
  }
  void need_peers() const {
    live();
    if (!open_) throw std::runtime_error("open_peers first");
  }
  void need_q8() const {
    need_peers();
    if (!open_q8_) throw std::runtime_error("the fp8 phases need open_peers with the peers' packed buffers");
  }

  void need_q8x2() const {
    need_q8();
    if (!open_q8x2_) throw std::runtime_error("the fp8x2 phases need open_peers with the peers' second packed buffers");
  }

  // The residual, allocated like the other buffers and zeroed on the stream, ahead of its first use there.
  // The caller holds a DeviceGuard of dev_.
  void need_residual() {
    if (residual_) return;
    {
      std::lock_guard<std::mutex> lock(peer_rank_mutex());
      residual_.reset(new DevBuf(dev_, 2 * cap_));
    }
    HIP_CHECK(hipMemsetAsync(residual_->p, 0, 2 * cap_, stream_));
  }

  float* zero1_state(int which) const { return static_cast<float*>(zero1_->p) + (size_t)which * zero1_n_; }
  float* zero1_ptr(int which, size_t first, size_t n, const char* what) const {
    live();
    if (which < 0 || which > 2) throw std::invalid_argument(std::string(what) + ": which is 0 (master), 1 (m) or 2 (v)");
    if (first > zero1_n_ || n > zero1_n_ - first) throw std::invalid_argument(std::string(what) + ": past the end of the state");
    return zero1_ ? zero1_state(which) + first : nullptr;
  }
  const float* stash_ptr(size_t first, size_t n) const {
    live();
    if (first > stash_elems() || n > stash_elems() - first) throw std::invalid_argument("zero1_read_state: past the end of the stash");
    return stash_ ? static_cast<const float*>(stash_->p) + first : nullptr;
  }
  // The grid of a launch over `n_vec` units that is about to be made: peer_reduce_grid, under the cap where one is set.
  int reduce_grid(size_t n_vec) {
    const int grid = peer_reduce_grid(cus_, blocks_per_cu_, share_, n_vec);
    return last_grid_ = max_ctas_ > 0 ? std::min(grid, max_ctas_) : grid;
  }
  size_t max_grid() const { return (size_t)std::max(1, cus_ * blocks_per_cu_); }  // no peer_reduce_grid exceeds it
  // parts[0, grid) of the launch just made, added in float64 in index order; synchronises the stream.
  double sum_parts(int grid) {
    std::vector<float> host((size_t)grid);
    HIP_CHECK(hipMemcpyAsync(host.data(), parts_->p, host.size() * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    double total = 0.0;
    for (float x : host) total += (double)x;
    return total;
  }
  static gtk_adamw::Hyper zero1_hyper(const std::array<float, 8>& a) {
    return gtk_adamw::Hyper{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]};
  }

  static void check_allocation(uintptr_t addr, int dev, size_t bytes) {
    void* p = reinterpret_cast<void*>(addr);
    hipPointerAttribute_t attr{};
    hipError_t e = addr ? hipPointerGetAttributes(&attr, p) : hipErrorInvalidValue;
    if (e != hipSuccess) {
      (void)hipGetLastError();
      throw std::invalid_argument("open_peers: an address is no device allocation of this process");
    }
    if (attr.type != hipMemoryTypeDevice || attr.device != dev)
      throw std::invalid_argument("open_peers: an address is not device memory of the device it is given with");
    void* base = nullptr;
    size_t size = 0;
    HIP_CHECK(hipMemGetAddressRange(reinterpret_cast<hipDeviceptr_t*>(&base), &size, reinterpret_cast<hipDeviceptr_t>(p)));
    if (base != p || size < bytes) throw std::invalid_argument("open_peers: an allocation is smaller than this rank's buffers");
  }

  void launch_gather(const SliceSet& sl, int nsrc) {
    DeviceGuard g(dev_);
    last_grid_ = gather_grid_cus(cus_, blocks_per_cu_, nsrc, share_);
    launch_peer_gather(sl, nsrc, reinterpret_cast<u32x4*>(out_->p), last_grid_, stream_);
    ++launches_;
  }

  void release_locked() noexcept {
    if (released_) return;
    released_ = true;
    close_peers();
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(dev_);
    if (stream_) {
      (void)hipStreamSynchronize(stream_);
      (void)hipStreamDestroy(stream_);
      stream_ = nullptr;
    }
    (void)hipSetDevice(prev);
    std::lock_guard<std::mutex> lock(peer_rank_mutex());
    window_.reset();
    out_.reset();
    packed_.reset();
    packed_out_.reset();
    residual_.reset();
    zero1_.reset();
    stash_.reset();
    parts_.reset();
    zero1_n_ = 0;
  }

  int dev_, rank_, world_;
  size_t cap_;
  int blocks_per_cu_, max_ctas_, cus_ = 1, share_ = 1;
  int last_grid_ = 0;
  std::unique_ptr<DevBuf> window_, out_, packed_, packed_out_, residual_;
  std::unique_ptr<DevBuf> zero1_;  // master, m and v, zero1_n_ floats each, in that order
  std::unique_ptr<DevBuf> stash_;  // the clipped step's scaled gradient sum, zero1_n_ floats: scratch, no part of a checkpoint
  std::unique_ptr<DevBuf> parts_;  // max_grid() floats: one sum-of-squares partial per block of launch 1
  size_t zero1_n_ = 0;
  hipStream_t stream_ = nullptr;
  SrcSet windows_{}, packeds_{};
  std::vector<u32x4*> outs_;  // mutable: a push stores into every rank's out
  std::vector<const u32x4*> packed_outs_;
  bool open_ = false, open_q8_ = false, open_q8x2_ = false, released_ = false;
  size_t launches_ = 0;
};

void bind_peer_rank(py::module_& m) {
  using nogil = py::call_guard<py::gil_scoped_release>;
  py::class_<PeerRank>(m, "PeerRank",
                       "one rank of the peer communicator's device backend: a window, an out and a stream on one device, "
                       "the K7 kernels launched over the peers' addresses; used by one thread")
      .def(py::init<int, int, int, size_t, int, int>(), py::arg("dev"), py::arg("rank"), py::arg("world"), py::arg("capacity_bytes"),
           py::arg("blocks_per_cu") = kBlocksPerCU, py::arg("max_ctas") = 0)
      .def("window_ptr", &PeerRank::window_ptr)
      .def("out_ptr", &PeerRank::out_ptr)
      .def("packed_ptr", &PeerRank::packed_ptr)
      .def("packed_out_ptr", &PeerRank::packed_out_ptr)
      .def("open_peers", &PeerRank::open_peers, py::arg("devices"), py::arg("windows"), py::arg("outs"),
           py::arg("packeds") = py::none(), py::arg("packed_outs") = py::none(), nogil())
      .def("close_peers", &PeerRank::close_peers, nogil())
      .def("reduce", &PeerRank::reduce, py::arg("v0"), py::arg("v1"), py::arg("in_dtype"), py::arg("out_dtype"), py::arg("scale") = 1.0f,
           nogil())
      .def("quantize", &PeerRank::quantize, py::arg("b0"), py::arg("b1"), py::arg("count"), py::arg("in_dtype"),
           py::arg("error_feedback") = false, nogil())
      .def("reset_residual", &PeerRank::reset_residual, nogil())
      .def("read_residual",
           [](PeerRank& r, size_t first_elem, size_t n) {
             if (r.released()) throw std::runtime_error("the PeerRank is released");
             if (first_elem > r.capacity_bytes() / 2 || n > r.capacity_bytes() / 2 - first_elem)
               throw std::invalid_argument("read_residual: past the end of the residual");
             py::array_t<float> a((py::ssize_t)n);
             float* p = a.mutable_data();
             {
               py::gil_scoped_release nogil;
               r.read_residual(p, first_elem, n);
             }
             return a;
           },
           py::arg("first_elem"), py::arg("n"))
      .def("write_residual",
           [](PeerRank& r, const py::array_t<float, py::array::c_style | py::array::forcecast>& a, size_t first_elem) {
             const float* p = a.data();
             const size_t n = (size_t)a.size();
             py::gil_scoped_release nogil;
             r.write_residual(p, n, first_elem);
           },
           py::arg("floats"), py::arg("first_elem") = 0)
      .def("reduce_q8", &PeerRank::reduce_q8, py::arg("b0"), py::arg("b1"), py::arg("out_dtype"), py::arg("scale") = 1.0f, nogil())
      .def("reduce_push", &PeerRank::reduce_push, py::arg("v0"), py::arg("v1"), py::arg("in_dtype"), py::arg("out_dtype"),
           py::arg("scale") = 1.0f, nogil())
      .def("reduce_q8_push", &PeerRank::reduce_q8_push, py::arg("b0"), py::arg("b1"), py::arg("out_dtype"), py::arg("scale") = 1.0f,
           nogil())
      .def("zero1_alloc", &PeerRank::zero1_alloc, py::arg("n_elems"), nogil())
      .def("zero1_write_state",
           [](PeerRank& r, int which, const py::array_t<float, py::array::c_style | py::array::forcecast>& a, size_t first) {
             const float* p = a.data();
             const size_t n = (size_t)a.size();
             py::gil_scoped_release nogil;
             r.zero1_write_state(which, p, first, n);
           },
           py::arg("which"), py::arg("floats"), py::arg("first") = 0)
      .def("zero1_read_state",
           [](PeerRank& r, int which, size_t first, size_t n) {
             if (r.released()) throw std::runtime_error("the PeerRank is released");
             const size_t have = which == 3 ? r.stash_elems() : r.zero1_elems();
             if (first > have || n > have - first) throw std::invalid_argument("zero1_read_state: past the end of the state");
             py::array_t<float> a((py::ssize_t)n);
             float* p = a.mutable_data();
             {
               py::gil_scoped_release nogil;
               r.zero1_read_state(which, p, first, n);
             }
             return a;
           },
           py::arg("which"), py::arg("first"), py::arg("n"))
      .def("reduce_adamw_push", &PeerRank::reduce_adamw_push, py::arg("v0"), py::arg("v1"), py::arg("scale"), py::arg("hyper"), nogil())
      .def("reduce_q8_adamw_push", &PeerRank::reduce_q8_adamw_push, py::arg("b0"), py::arg("b1"), py::arg("scale"), py::arg("hyper"),
           nogil())
      .def("zero1_stash_alloc", &PeerRank::zero1_stash_alloc, nogil())
      .def("reduce_sqnorm_stash", &PeerRank::reduce_sqnorm_stash, py::arg("v0"), py::arg("v1"), py::arg("scale"), nogil())
      .def("reduce_q8_sqnorm_stash", &PeerRank::reduce_q8_sqnorm_stash, py::arg("b0"), py::arg("b1"), py::arg("scale"), nogil())
      .def("reduce_sqnorm_accum", &PeerRank::reduce_sqnorm_accum, py::arg("v0"), py::arg("v1"), py::arg("scale"), nogil())
      .def("reduce_q8_sqnorm_accum", &PeerRank::reduce_q8_sqnorm_accum, py::arg("b0"), py::arg("b1"), py::arg("scale"), nogil())
      .def("adamw_push", &PeerRank::adamw_push, py::arg("v0"), py::arg("v1"), py::arg("hyper"), nogil())
      .def("repack_q8", &PeerRank::repack_q8, py::arg("b0"), py::arg("b1"), py::arg("scale") = 1.0f, nogil())
      .def("unpack_q8", &PeerRank::unpack_q8, py::arg("slices"), py::arg("out_dtype"), nogil())
      .def("gather", &PeerRank::gather, py::arg("slices"), nogil())
      .def("gather_windows", &PeerRank::gather_windows, py::arg("n_vec"), nogil())
      .def("write_host",
           [](PeerRank& r, const py::buffer& b, size_t first_byte) {
             const py::buffer_info info = b.request();
             if (!PyBuffer_IsContiguous(info.view(), 'C')) throw std::invalid_argument("write_host: a contiguous buffer");
             const void* p = info.ptr;
             const size_t n = (size_t)info.size * (size_t)info.itemsize;
             py::gil_scoped_release nogil;
             r.write_host(p, n, first_byte);
           },
           py::arg("bytes_like"), py::arg("first_byte") = 0)
      .def("read_host",
           [](PeerRank& r, size_t first_byte, size_t nbytes) {
             if (r.released()) throw std::runtime_error("the PeerRank is released");
             if (first_byte > 2 * r.capacity_bytes() || nbytes > 2 * r.capacity_bytes() - first_byte)
               throw std::invalid_argument("read_host: past the end of out");
             py::array_t<uint8_t> a((py::ssize_t)nbytes);
             void* p = a.mutable_data();
             {
               py::gil_scoped_release nogil;
               r.read_host(p, first_byte, nbytes);
             }
             return a;
           },
           py::arg("first_byte"), py::arg("nbytes"))
      .def("synchronize", &PeerRank::synchronize, nogil())
      .def("release", &PeerRank::release, nogil())
      .def_property_readonly("launches", &PeerRank::launches)
      .def_property_readonly("last_grid", &PeerRank::last_grid)
      .def_property_readonly("capacity_bytes", &PeerRank::capacity_bytes)
      .def_property_readonly("packed_bytes", &PeerRank::packed_bytes)
      .def_property_readonly("residual_bytes", &PeerRank::residual_bytes)
      .def_property_readonly("zero1_bytes", &PeerRank::zero1_bytes)
      .def_property_readonly("released", &PeerRank::released);
}

}  // namespace
