// The optimizer: flat-buffer AdamW (decoupled weight decay) over bf16 weights with fp32 master/m/v,
// and the gradient's sum of squares for global-norm clipping.
//
//   adamw_flat_kernel    grid-stride over the whole buffer, 8 elements per thread per trip: two 16-B
//                        loads each of master/m/v, the gradient's 8 elements; writes master/m/v and
//                        the bf16 weight.  28 B in + out per element: HBM-bound by construction.
//   adamw_tiles_kernel   the same update that also writes the transposed bf16 weights (VERDICT r3
//                        next #3).  The Llama workload's backward GEMMs run in hipBLASLt's fastest
//                        ("NT") layout, whose input-gradient GEMM reads W^T (models/llama.py).  W changes
//                        only here, so the optimizer, which streams every weight anyway, writes W^T in
//                        the same pass: +2 B per element, and the backward finds W^T ready.  One
//                        64 x 256 tile of one projection matrix per loop trip (grid-stride over every
//                        matrix's tiles: the persistent grid ends when the tile index passes the total,
//                        so every wave exits).  The update walks 1 KiB row segments like the flat
//                        kernel, stages the new bf16 rows in the LDS tile of tile_t.h, and writes W^T
//                        from it.
//   adamw_ranges_kernel  the parameters that are not transposed (embedding, norms): blockIdx.y picks a
//                        range, grid-stride over its 16-B vectors.
//   sqnorm_kernel        sum of squares of the gradient -> per-block fp32 partials; optionally
//                        advances the device step counter.
// Every AdamW kernel updates its elements through adam8 with the hyper-parameters of hyper<DEV>, so
// master/m/v/W get the same bits whichever kernel touches them.  DEV = the graph-capturable form:
// bias corrections and the clipping factor are derived on the device.  The gradient is bf16, or the
// fp32 buffer a DP all-reduce in fp32 leaves (parallel/dp.py grad_reduce="fp32").
#include <type_traits>
#include <vector>

#include "../common/adamw_update.h"  // Hyper and adam8_update, the update body every kernel here instantiates
#include "tile_t.h"

namespace gtk_adamw {

using namespace gtk;

// the sum of s over the block's 256 threads (4 waves), in every thread
__device__ __forceinline__ float block_sum(float s) {
  __shared__ float red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// hp (host form) = [lr, beta1, beta2, eps, weight_decay, grad_scale, bias_c1, bias_c2]: a device
//   tensor, so a captured graph replays with updated hyper-parameters.
// hp (DEV form)  = [lr, beta1, beta2, eps, weight_decay, grad_scale, clip_norm (<= 0: off), -]:
//   everything the host used to compute per step is derived here, so one captured launch replays
//   correctly forever (``FlatAdamW(capturable=True)``).
//     part = the gradient's sum-of-squares partials (``sq_norm_parts``); every block sums them itself
//     tptr = optimizer step count AFTER this step (``sq_norm_parts`` advanced it in stream order)
//   Bias corrections 1 - beta^t and the clipping factor min(1, clip / ||g * grad_scale||) follow.
//   The gradient may hold anything.  A NaN norm gives a NaN factor, as torch.clamp(.., max=1) does in
//   the host form (models/optim.py), and with it a NaN in every element: a fminf would return 1 and
//   switch the clipping off quietly.  An infinite norm gives the factor 0.  Without clipping a NaN or
//   an Inf in the gradient reaches its own element of master, m, v and W alone.
template <bool DEV>
__device__ __forceinline__ Hyper hyper(const float* __restrict__ hp, const float* __restrict__ part, int nparts,
                                       const float* __restrict__ tptr) {
  Hyper h{hp[0], hp[1], hp[2], hp[3], hp[4], hp[5], 0.f, 0.f};
  if (!DEV) {
    h.bc1 = hp[6];
    h.bc2 = hp[7];
    return h;
  }
  const float clip = hp[6];
  if (nparts > 0 && clip > 0.f) {  // block-uniform
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
    const float norm = sqrtf(block_sum(s)) * h.gs;
    const float f = clip / (norm + 1e-6f);
    h.gs = h.gs * (f > 1.f ? 1.f : f);  // not fminf: a NaN passes
  }
  const float t = tptr[0];
  h.bc1 = 1.f - powf(h.b1, t);
  h.bc2 = 1.f - powf(h.b2, t);
  return h;
}

// 8 gradient elements at flat index i (a multiple of 8) as fp32
__device__ __forceinline__ void load_g8(const u16* __restrict__ g, size_t i, float (&out)[8]) {
  const u16x8 gv = *reinterpret_cast<const u16x8*>(g + i);
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = bf2f(gv[j]);
}
__device__ __forceinline__ void load_g8(const float* __restrict__ g, size_t i, float (&out)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(g + i), b = *reinterpret_cast<const f32x4*>(g + i + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = a[j], out[j + 4] = b[j];
}

// The update of 8 elements at flat index i (a multiple of 8) in two halves: the loads, then the
// arithmetic and the stores from those registers.  The tile kernel issues the loads of several passes
// before any store: through the same master/m/v pointers the compiler cannot hoist a later pass's
// loads above an earlier pass's stores.
struct Adam8In {
  f32x4 p0, p1, m0, m1, v0, v1;
  float gf[8];
};
template <typename G>
__device__ __forceinline__ void adam8_load(const float* __restrict__ master, const float* __restrict__ m, const float* __restrict__ v,
                                           const G* __restrict__ g, size_t i, Adam8In& in) {
  const f32x4* mp = reinterpret_cast<const f32x4*>(master + i);
  const f32x4* mm_ = reinterpret_cast<const f32x4*>(m + i);
  const f32x4* vp = reinterpret_cast<const f32x4*>(v + i);
  in.p0 = mp[0], in.p1 = mp[1], in.m0 = mm_[0], in.m1 = mm_[1], in.v0 = vp[0], in.v1 = vp[1];
  load_g8(g, i, in.gf);
}
// returns the 8 new bf16 weights it stored
__device__ __forceinline__ u16x8 adam8_store(float* __restrict__ master, float* __restrict__ m, float* __restrict__ v,
                                             u16* __restrict__ w, size_t i, const Adam8In& in, const Hyper& h) {
  u16x8 wo;
  float p[8], mm[8], vv[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    p[j] = in.p0[j], p[j + 4] = in.p1[j];
    mm[j] = in.m0[j], mm[j + 4] = in.m1[j];
    vv[j] = in.v0[j], vv[j + 4] = in.v1[j];
  }
  adam8_update(p, mm, vv, in.gf, h, wo);
  f32x4 p0, p1, m0, m1, v0, v1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    p0[j] = p[j], p1[j] = p[j + 4];
    m0[j] = mm[j], m1[j] = mm[j + 4];
    v0[j] = vv[j], v1[j] = vv[j + 4];
  }
  f32x4* mp = reinterpret_cast<f32x4*>(master + i);
  f32x4* mmp = reinterpret_cast<f32x4*>(m + i);
  f32x4* vp = reinterpret_cast<f32x4*>(v + i);
  mp[0] = p0, mp[1] = p1, mmp[0] = m0, mmp[1] = m1, vp[0] = v0, vp[1] = v1;
  *reinterpret_cast<u16x8*>(w + i) = wo;
  return wo;
}
template <typename G>
__device__ __forceinline__ u16x8 adam8(float* __restrict__ master, float* __restrict__ m, float* __restrict__ v,
                                       const G* __restrict__ g, u16* __restrict__ w, size_t i, const Hyper& h) {
  Adam8In in;
  adam8_load(master, m, v, g, i, in);
  return adam8_store(master, m, v, w, i, in, h);
}

template <bool DEV, typename G>
__global__ __launch_bounds__(256) void adamw_flat_kernel(float* __restrict__ master, float* __restrict__ m, float* __restrict__ v,
                                                         const G* __restrict__ g, u16* __restrict__ w, const float* __restrict__ hp,
                                                         const float* __restrict__ part, int nparts, const float* __restrict__ tptr,
                                                         size_t n) {
  const Hyper h = hyper<DEV>(hp, part, nparts, tptr);
  const size_t nv = n >> 3;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) adam8(master, m, v, g, w, 8 * i, h);
}

// one transposed matrix: rows R x cols C at flat element offset `off`, its W^T ([C, R]) at `toff` of
// the transposed buffer, tiles [tile_base, tile_base + (R/64)(C/64)) of the global tile index
struct Mat {
  int64_t off, toff, R, C, tile_base;
};

// Tile = 64 rows x 256 columns.  The fp32 master/m/v streams are read and written in 1 KiB
// contiguous row segments (a wave covers two rows: 64 lanes x 8 elements x 4 B), the access shape of
// the flat kernel; a 64 x 64 tile's 256-B segments ran the step at 5.45 TB/s against the flat
// kernel's 5.97 (profiles/r04_llama).  W^T leaves as 256 output rows x 128 B.
constexpr int kTR = 64, kTC = 256;

template <bool DEV, typename G, int kAhead = 1>
__global__ __launch_bounds__(256) void adamw_tiles_kernel(float* __restrict__ master, float* __restrict__ m, float* __restrict__ v,
                                                          const G* __restrict__ g, u16* __restrict__ w, u16* __restrict__ wt,
                                                          const Mat* __restrict__ mats, int nmats, int64_t total_tiles,
                                                          const float* __restrict__ hp, const float* __restrict__ part, int nparts,
                                                          const float* __restrict__ tptr) {
  __shared__ TileT<kTC / 8> tile;
  const Hyper h = hyper<DEV>(hp, part, nparts, tptr);
  const int t = threadIdx.x;
  for (int64_t ti = blockIdx.x; ti < total_tiles; ti += gridDim.x) {
    int lo = 0, hi = nmats - 1;  // last matrix whose tile_base <= ti (block-uniform)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (mats[mid].tile_base <= ti) lo = mid;
      else hi = mid - 1;
    }
    const Mat mt = mats[lo];
    const int64_t local = ti - mt.tile_base, tiles_c = mt.C / kTC;
    const int64_t r0 = (local / tiles_c) * kTR, c0 = (local % tiles_c) * kTC;
    // update: 8 passes of 8 rows; thread t takes vector t & 31 of row 8 * pass + t / 32
    if (kAhead == 1) {
#pragma unroll 4
      for (int pass = 0; pass < kTR / 8; ++pass) {
        const int r = 8 * pass + (t >> 5), vv = t & 31;
        tile.put(r, vv, adam8(master, m, v, g, w, (size_t)(mt.off + (r0 + r) * mt.C + c0 + 8 * vv), h));
      }
    } else {  // kAhead passes' loads in flight before their stores
#pragma unroll 1
      for (int p0 = 0; p0 < kTR / 8; p0 += kAhead) {
        Adam8In in[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          const int r = 8 * (p0 + u) + (t >> 5), vv = t & 31;
          adam8_load(master, m, v, g, (size_t)(mt.off + (r0 + r) * mt.C + c0 + 8 * vv), in[u]);
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          const int r = 8 * (p0 + u) + (t >> 5), vv = t & 31;
          tile.put(r, vv, adam8_store(master, m, v, w, (size_t)(mt.off + (r0 + r) * mt.C + c0 + 8 * vv), in[u], h));
        }
      }
    }
    __syncthreads();
    tile.store_t(wt + mt.toff, (size_t)mt.R, (size_t)c0, (size_t)r0);  // W^T: 256 output rows x 128 B
    __syncthreads();  // the tile is free for the next trip
  }
}

// ranges: [start, length] element pairs (multiples of 8)
template <bool DEV, typename G>
__global__ __launch_bounds__(256) void adamw_ranges_kernel(float* __restrict__ master, float* __restrict__ m, float* __restrict__ v,
                                                           const G* __restrict__ g, u16* __restrict__ w,
                                                           const int64_t* __restrict__ ranges, const float* __restrict__ hp,
                                                           const float* __restrict__ part, int nparts,
                                                           const float* __restrict__ tptr) {
  const Hyper h = hyper<DEV>(hp, part, nparts, tptr);
  const int64_t start = ranges[2 * blockIdx.y], nv = ranges[2 * blockIdx.y + 1] >> 3;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256)
    adam8(master, m, v, g, w, (size_t)(start + 8 * i), h);
}

// Sum of squares of n gradient elements -> one fp32 partial per block.  Each thread's grid-stride
// vectors are loaded kAhead at a time (four 16-B loads in flight per lane; one at a time ran the 16 GB
// bf16 gradient at 5.3 TB/s) and summed in ascending order into one accumulator.  The clip factor, and
// with it the training trajectory, is sensitive to the norm's last bits (profiles/r04_norm).  For a bf16
// gradient every square is exact in fp32, so a partial's bits depend on the grid alone; for an fp32
// gradient they also depend on which products the compiler fuses into the sum, which differs between
// the loop shapes (profiles/adamw_one_body): an entry point's kAhead is part of its result.
// tick, when given: block 0 adds 1 to the step counter -- nothing else in this kernel reads it; the
// AdamW kernel after it in stream order does.
template <typename G, int kAhead>
__global__ __launch_bounds__(256) void sqnorm_kernel(const G* __restrict__ g, float* __restrict__ part, size_t n,
                                                     float* __restrict__ tick) {
  float s = 0.f;
  const size_t nv = n >> 3, stride = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + (kAhead - 1) * stride < nv; i += kAhead * stride) {
    float x[kAhead][8];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) load_g8(g, 8 * (i + u * stride), x[u]);
#pragma unroll
    for (int u = 0; u < kAhead; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) s += x[u][j] * x[u][j];
  }
  for (; kAhead > 1 && i < nv; i += stride) {  // the last kAhead - 1 vectors at the most
    float x[8];
    load_g8(g, 8 * i, x);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += x[j] * x[j];
  }
  s = block_sum(s);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = s;
    if (tick != nullptr && blockIdx.x == 0) tick[0] = tick[0] + 1.f;
  }
}

// f(the gradient's data as const float*, or as const u16* for bf16)
template <typename F>
void with_grad(const at::Tensor& g, F&& f) {
  if (g.scalar_type() == at::kFloat) f(static_cast<const float*>(g.data_ptr<float>()));
  else f(bp(g));
}
template <typename P>
using elem_t = std::remove_cv_t<std::remove_pointer_t<P>>;

// the DEV form's device inputs; all null in the host form
struct DevIn {
  const float* part = nullptr;
  int nparts = 0;
  const float* t = nullptr;
};
DevIn dev_in(const c10::optional<at::Tensor>& part, const at::Tensor* t) {
  DevIn d;
  if (part.has_value()) {
    CHECK_F32(*part);
    d.part = part->data_ptr<float>();
    d.nparts = (int)part->numel();
  }
  if (t != nullptr) {
    CHECK_F32(*t);
    d.t = t->data_ptr<float>();
  }
  return d;
}

// checks the flat buffers; returns their common element count
size_t check_flat(const at::Tensor& master, const at::Tensor& m, const at::Tensor& v, const at::Tensor& g, const at::Tensor& w,
                  const at::Tensor& hp) {
  CHECK_F32(master);
  CHECK_F32(m);
  CHECK_F32(v);
  CHECK_GRAD(g);
  CHECK_BF16(w);
  CHECK_F32(hp);
  const size_t n = master.numel();
  TORCH_CHECK(n % 8 == 0 && (size_t)m.numel() == n && (size_t)v.numel() == n && (size_t)g.numel() == n && (size_t)w.numel() == n,
              "adamw: flat buffers must have equal sizes, a multiple of 8");
  return n;
}

template <bool DEV>
void launch_flat(at::Tensor& master, at::Tensor& m, at::Tensor& v, const at::Tensor& g, at::Tensor& w, const at::Tensor& hp,
                 const DevIn& d, size_t n) {
  if (!n) return;
  with_grad(g, [&](auto* gp) {
    hipLaunchKernelGGL((adamw_flat_kernel<DEV, elem_t<decltype(gp)>>), dim3(grid_for(n / 8)), dim3(256), 0, cur_stream(),
                       master.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), gp, bpm(w), hp.data_ptr<float>(), d.part,
                       d.nparts, d.t, n);
  });
}

void adamw_step(at::Tensor& master, at::Tensor& m, at::Tensor& v, const at::Tensor& g, at::Tensor& w, const at::Tensor& hp) {
  const size_t n = check_flat(master, m, v, g, w, hp);
  TORCH_CHECK(hp.numel() >= 8, "adamw: hp needs 8 entries");
  launch_flat<false>(master, m, v, g, w, hp, DevIn{}, n);
}

void adamw_step_dev(at::Tensor& master, at::Tensor& m, at::Tensor& v, const at::Tensor& g, at::Tensor& w, const at::Tensor& hp,
                    c10::optional<at::Tensor> part, const at::Tensor& t) {
  const size_t n = check_flat(master, m, v, g, w, hp);
  TORCH_CHECK(hp.numel() >= 7, "adamw_step_dev: hp needs 7 entries");
  launch_flat<true>(master, m, v, g, w, hp, dev_in(part, &t), n);
}

// `grid` partials of g's sum of squares into part
template <int kAhead>
void launch_sqnorm(const at::Tensor& g, at::Tensor& part, int grid, float* tick) {
  with_grad(g, [&](auto* gp) {
    hipLaunchKernelGGL((sqnorm_kernel<elem_t<decltype(gp)>, kAhead>), dim3(grid), dim3(256), 0, cur_stream(), gp, part.data_ptr<float>(),
                       (size_t)g.numel(), tick);
  });
}

// The number of partials determines the sum's bits: sq_norm always has 1024, sq_norm_parts one per
// 256 vectors up to 1024; so does kAhead for an fp32 gradient: 4 in sq_norm, 1 in sq_norm_parts.
at::Tensor sq_norm(const at::Tensor& g) {
  CHECK_GRAD(g);
  TORCH_CHECK(g.numel() % 8 == 0, "sq_norm: size must be a multiple of 8");
  const int grid = 1024;
  auto part = at::zeros({grid}, g.options().dtype(at::kFloat));
  if (g.numel()) launch_sqnorm<4>(g, part, grid, nullptr);
  return part.sum();
}

at::Tensor sq_norm_parts(const at::Tensor& g, c10::optional<at::Tensor> tick) {
  CHECK_GRAD(g);
  const size_t n = g.numel();
  TORCH_CHECK(n % 8 == 0, "sq_norm_parts: size must be a multiple of 8");
  float* tk = nullptr;
  if (tick.has_value()) {
    CHECK_F32(*tick);
    tk = tick->data_ptr<float>();
  }
  const int grid = (int)std::max<size_t>(1, std::min<size_t>((n / 8 + 255) / 256, 1024));
  auto part = at::empty({grid}, g.options().dtype(at::kFloat));  // every slot written
  launch_sqnorm<1>(g, part, grid, tk);
  return part;
}

// mats: int64 [N, 5] (off, toff, R, C, tile_base) on the device; ranges: int64 [M, 2] on the device.
// part / t present = the DEV form.  ahead: passes' loads in flight in the host form's tile kernel
// (1, 2 or 4; anything else = 1).
void adamw_step_t(at::Tensor& master, at::Tensor& m, at::Tensor& v, const at::Tensor& g, at::Tensor& w, at::Tensor& wt,
                  const at::Tensor& hp, const at::Tensor& mats, int64_t total_tiles, const at::Tensor& ranges,
                  int64_t max_range, c10::optional<at::Tensor> part, c10::optional<at::Tensor> t, int64_t ahead) {
  check_flat(master, m, v, g, w, hp);
  CHECK_BF16(wt);
  CHECK_I64(mats);
  CHECK_I64(ranges);
  TORCH_CHECK(mats.dim() == 2 && mats.size(1) == 5 && ranges.dim() == 2 && ranges.size(1) == 2, "adamw_step_t: bad descriptors");
  TORCH_CHECK(ranges.size(0) <= 65535, "adamw_step_t: too many ranges");
  const bool dev = t.has_value();
  const DevIn d = dev_in(part, dev ? &*t : nullptr);
  hipStream_t s = cur_stream();
  auto* mp = master.data_ptr<float>();
  auto* mmp = m.data_ptr<float>();
  auto* vp = v.data_ptr<float>();
  auto* hpp = hp.data_ptr<float>();
  with_grad(g, [&](auto* gp) {
    using G = elem_t<decltype(gp)>;
    if (mats.size(0) > 0 && total_tiles > 0) {
      const dim3 grid((unsigned)std::min<int64_t>(total_tiles, 4096));
      const Mat* md = reinterpret_cast<const Mat*>(mats.data_ptr<int64_t>());
      const int nm = (int)mats.size(0);
      auto tiles = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, mp, mmp, vp, gp, bpm(w), bpm(wt), md, nm, total_tiles, hpp, d.part, d.nparts,
                           d.t);
      };
      if (dev) tiles(adamw_tiles_kernel<true, G>);
      else if (ahead == 4) tiles(adamw_tiles_kernel<false, G, 4>);
      else if (ahead == 2) tiles(adamw_tiles_kernel<false, G, 2>);
      else tiles(adamw_tiles_kernel<false, G>);
    }
    if (ranges.size(0) > 0 && max_range > 0) {
      const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((max_range / 8 + 255) / 256, 2048));
      auto flat = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(gx, (unsigned)ranges.size(0)), dim3(256), 0, s, mp, mmp, vp, gp, bpm(w),
                           ranges.data_ptr<int64_t>(), hpp, d.part, d.nparts, d.t);
      };
      if (dev) flat(adamw_ranges_kernel<true, G>);
      else flat(adamw_ranges_kernel<false, G>);
    }
  });
}

}  // namespace gtk_adamw
