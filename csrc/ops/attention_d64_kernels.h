#pragma once
// Causal GQA flash attention at head dim 64 for gfx950 (MFMA 32x32x16 bf16), forward and backward, with
// and without the document mask of a packed batch.  bf16 I/O, fp32 accumulation and softmax; the same
// numerics and the same outputs as the head-dim-128 family of attention_kernels.h (lse2 = m + log2 l in
// log2 units with c = scale * log2 e folded into the exponent, raw v_exp_f32, the slack-8 running max,
// the finite initial max under the document mask, every document bound clamped).  Written beside that
// family, not as a parameter of it: the 128 kernels are not to move (see the comment at their top).
// New code, so one template over the mask (kDoc) instead of a header compiled twice.
//
// What head dim 64 changes, and what this design does with it:
//   * Per 64-key tile a wave has half the MFMAs of the 128 kernel (8 QK^T + 8 PV) and the same 32
//     exponentials per lane, so the forward leans on the VALU / transcendental pipe, not on the matrix
//     pipe.  The registers that 4 Q fragments and 2 O accumulators free are spent on occupancy: the
//     forward fits 168 VGPRs and runs THREE waves per SIMD (three 128-query workgroups per CU, 32 KiB of
//     LDS each), so one wave's softmax runs under the MFMAs of two others.  Tiles stay 128 queries x 64
//     keys: every S that is a multiple of 128 is served and the causal triangle keeps its balance.
//   * LDS rows are 128 B, two to a 256-B line of the 64 banks.  The image of a [rows][64 x bf16] tile
//     puts 16-B chunk ch of row r at 128 r + 16 (ch ^ g(r)), g(r) = 4 bit1(r) + bits32(r):
//       - ds_read_b128 row reads (K; Q and dO in dK/dV): 16 lanes read one chunk column of 16
//         consecutive rows.  Rows of one parity share a half line; g is a bijection of bits 1..3 of r,
//         so the 8 rows of a parity take the 8 chunk slots of their half: conflict-free.
//       - ds_read_b64_tr_b16 transposed reads (V; K in dQ; dO^T and Q^T in dK/dV): 32 lanes read 4
//         aligned chunks of rows 4j .. 4j+3.  Rows 4j and 4j+2 share a half line and differ in bit 1,
//         which g moves to bit 2 of the slot: the two rows take the two aligned groups of 4 slots.
//     The swizzle goes on the SOURCE offset of the LDS-DMA (1 KiB = 8 rows per wave instruction), so the
//     destination stays lane-linear.
//   * K/V tiles (forward, dQ) and query slices (dK/dV) are double-buffered in LDS, the next one staged
//     by buffer_load ... lds through wave-uniform descriptors under the current one's math, with one
//     explicit wait + barrier (dma_sync) per tile.
//   * "swapped" products as in the 128 family: the query (forward, dQ) or the key (dK/dV) sits on the
//     lane, so the score accumulator, rounded to bf16, IS the B operand of the next MFMA and the row
//     max / sum need one exchange with lane ^ 32.
//   * Grids: forward and dQ (B*H, S/128), heaviest query block first, heads XCD-grouped; dK/dV
//     (B*Hkv, S/128), one workgroup = 128 keys of one (batch, kv-head) sweeping every q-head of the GQA
//     group x 32-query slices: no cross-workgroup sums, no atomics.  dK/dV computes a slice's dV^T / dK^T
//     products right after its softmax (no deferral ring: at 64 accumulator registers per wave two
//     workgroups share a CU and cover each other's waits) and keeps -lse/c and -delta as the initial
//     accumulators of the S and dP chains.
//   * Document mask: the block's tile range starts at doc_start of its first query, a key block's
//     sweep ends at doc_end of its last key; per wave, a tile (slice) wholly outside the documents of
//     the wave's rows is skipped, and the per-lane compare runs on the tiles that can need it.
#include <cmath>

#include "bf16.h"

namespace gtk_attn64 {

using namespace gtk;

typedef u16 u16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int D = 64;
constexpr int ROWB = D * 2;        // bytes per LDS row
constexpr int BQ = 128;            // forward, dQ: queries per workgroup
constexpr int BK = 64;             // forward, dQ: keys per tile
constexpr int TILEB = BK * ROWB;   // one K or V image
constexpr int KB = 128;            // dK/dV: keys per workgroup
constexpr int QT = 32;             // dK/dV: queries per slice

#define GTK64_LDS __attribute__((address_space(3)))

// byte offset of 16-B chunk `ch` of row `row` in a [rows][64 x bf16] swizzled image
__device__ __forceinline__ int swz_slot(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }
__device__ __forceinline__ int swz(int row, int ch) { return row * ROWB + 16 * (ch ^ swz_slot(row)); }
// accumulator register -> row of a 32x32 MFMA tile (lane half hh)
__device__ __forceinline__ int crow(int reg, int hh) { return (reg & 3) + 8 * (reg >> 2) + 4 * hh; }

__device__ __forceinline__ bf16x8 lds_b128(const char* base, int off) { return *reinterpret_cast<const bf16x8*>(base + off); }

__device__ __forceinline__ s16x4 lds_tr(const char* base, int off) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((GTK64_LDS s16x4*)(base + off));
}

// whole-vector bit casts only (a per-element cast of the transposed read's result is miscompiled)
__device__ __forceinline__ bf16x8 cat8(s16x4 lo, s16x4 hi) {
  return __builtin_shufflevector(__builtin_bit_cast(bf16x4, lo), __builtin_bit_cast(bf16x4, hi), 0, 1, 2, 3, 4, 5, 6, 7);
}

// Transposed A fragment of a 32x32x16 MFMA whose k index walks ROWS of a swizzled image and whose
// output row walks COLUMNS: element j of lane (r, hh) = img[row_of(j)][col0 + r], rows r_lo + {0..3}
// (j < 4) and r_hi + {0..3} (j >= 4); the caller adds 4 * hh to both.
__device__ __forceinline__ bf16x8 tr_frag(const char* img, int lane, int r_lo, int r_hi, int col0) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int col = col0 + 16 * (g & 1);
  const int ch = (col >> 3) + (p >> 1);
  s16x4 lo = lds_tr(img, swz(r_lo + q, ch) + 8 * (p & 1));
  s16x4 hi = lds_tr(img, swz(r_hi + q, ch) + 8 * (p & 1));
  return cat8(lo, hi);
}

__device__ __forceinline__ bf16x8 pack8(const f32x16& acc, int base) {
  bf16x8 out;
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = (__bf16)acc[base + j];
  return out;
}

// raw v_exp_f32 (2^x): softmax terms below 2^-126 are 0 either way
__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// workgroups are dealt round-robin over the 8 XCDs: consecutive ids of one XCD -> consecutive heads
__device__ __forceinline__ int xcd_head(int id, int n) { return (n & 7) ? id : (id & 7) * (n >> 3) + (id >> 3); }

__device__ __forceinline__ float max3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

__device__ __forceinline__ float xhalf_max(float x) {  // max(x[lane], x[lane ^ 32])
  const auto p = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(p[0]), __uint_as_float(p[1]));
}

constexpr float kMaxSlack = 8.f;  // the running max moves only when a row's max exceeds it by more
constexpr float kMinM = -1e30f;   // finite initial max of the document build: fma(-inf, c, -kMinM) stays -inf

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// every wave's LDS-DMA has landed and every LDS read it issued has returned, then a barrier
__device__ __forceinline__ void dma_sync() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

// LDS-DMA staging of one [64][64] K tile and V tile into the swizzled images (K at img, V at img + 8 KiB)
// by a 4-wave workgroup: wave w fills rows 16w .. 16w+15 of each with 2 buffer_load_dwordx4 ... lds
// (1 KiB = 8 rows).  Lane (row R, slot p) fetches chunk p ^ g(R): swz(R, chunk) == 128 R + 16 p.
struct KVStage {
  __amdgpu_buffer_rsrc_t krs, vrs;
  uint32_t voff[2];
  int w;
  __device__ __forceinline__ KVStage(const u16* kbase, const u16* vbase, int S, int w_, int lane) : w(w_) {
    const uint32_t bytes = (uint32_t)((size_t)S * ROWB);
    krs = __builtin_amdgcn_make_buffer_rsrc((void*)kbase, 0, bytes, 0x00020000);
    vrs = __builtin_amdgcn_make_buffer_rsrc((void*)vbase, 0, bytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int R = 16 * w + 8 * i + (lane >> 3);
      voff[i] = (uint32_t)(R * ROWB + 16 * ((lane & 7) ^ swz_slot(R)));
    }
  }
  __device__ __forceinline__ void load(int kt, char* img) const {
    const uint32_t soff = (uint32_t)kt * TILEB;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(krs, (GTK64_LDS void*)(img + (16 * w + 8 * i) * ROWB), 16, voff[i], soff, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(vrs, (GTK64_LDS void*)(img + TILEB + (16 * w + 8 * i) * ROWB), 16, voff[i], soff,
                                               0, 0);
    }
  }
};

// What the forward and dQ kernels derive from doc_start (ds = the batch row), every bound clamped to
// [0, its query]: lo of the lane's query, the block's first tile, doc_start of the wave's first / last query.
struct DocTiles {
  int lo, kt0, wlo0, wlo1;
  __device__ __forceinline__ DocTiles() : lo(0), kt0(0), wlo0(0), wlo1(0) {}
  __device__ __forceinline__ DocTiles(const int* __restrict__ ds, int qb, int q0, int myq) {
    lo = clampi(ds[myq], 0, myq);
    kt0 = clampi(ds[qb * BQ], 0, qb * BQ) / BK;
    wlo0 = clampi(ds[q0], 0, q0);
    wlo1 = clampi(ds[q0 + 31], 0, q0 + 31);
  }
};

// 8 packed bf16 of two column groups -> 16 contiguous bytes per lane (lanes 0-31: group k, 32-63: k+1)
__device__ __forceinline__ uint4 widen(u16x4 va, u16x4 vb) {
  const auto a = __builtin_bit_cast(uint2, va), bb = __builtin_bit_cast(uint2, vb);
  const auto s0 = __builtin_amdgcn_permlane32_swap(a.x, bb.x, false, false);
  const auto s1 = __builtin_amdgcn_permlane32_swap(a.y, bb.y, false, false);
  return uint4{s0[0], s1[0], s0[1], s1[1]};
}

// ==================================================================================== forward
// One workgroup = 4 waves = 128 queries of one (batch, q-head), wave w the queries 32w .. 32w+31 (one per
// lane & 31); tiles of 64 keys.  Per tile and wave: S^T = K . Q^T (2 x 4 MFMAs), the next tile's DMA, the
// online softmax on the 32 scores of the lane, O^T += V^T . P^T (2 x 4 MFMAs, V^T by transposed reads).
// Only the block's last two tiles can need the causal mask or be invisible to a wave.  kDoc: query i
// sees key j iff doc_start[b, i] <= j <= i; a wave skips a tile that ends at or before doc_start of its
// first query and lower-masks a tile that begins before doc_start of its last query.
template <bool kDoc>
__global__ __launch_bounds__(256, 3) void attn64_fwd_kernel(const u16* __restrict__ q, const u16* __restrict__ k,
                                                            const u16* __restrict__ v, u16* __restrict__ o,
                                                            float* __restrict__ lse2, int H, int Hkv, int S, float c,
                                                            u16* __restrict__ ot, const int* __restrict__ doc_start) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILEB];  // [buf][K image | V image]
  const int t = threadIdx.x, lane = t & 63, r = lane & 31, hh = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nqb = gridDim.y;
  const int qb = nqb - 1 - blockIdx.y;  // heaviest first
  const int bh = xcd_head(blockIdx.x, gridDim.x), b = bh / H, hq = bh % H, hk = hq / (H / Hkv);
  const u16* qp = q + ((size_t)(b * H + hq) * S) * D;
  const size_t kvoff = ((size_t)(b * Hkv + hk) * S) * D;
  const int q0 = qb * BQ + w * 32;
  const int myq = q0 + r;

  bf16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qp + (size_t)myq * D + 16 * s + 8 * hh);

  f32x16 oacc[2];
  oacc[0] = oacc[1] = f32x16{};
  float m = kDoc ? kMinM : -INFINITY, l = 0.f;  // m in log2 units (score * c)

  const int ntiles = (qb * BQ + BQ) / BK;
  DocTiles dt_;
  if (kDoc) dt_ = DocTiles(doc_start + (size_t)b * S, qb, q0, myq);
  const int lo = dt_.lo, kt0 = kDoc ? dt_.kt0 : 0, wlo0 = dt_.wlo0, wlo1 = dt_.wlo1;
  const KVStage stage(k + kvoff, v + kvoff, S, w, lane);
  auto buf = [&](int kt) { return smem + (kt & 1) * (2 * TILEB); };

  auto tile = [&](int kt, bool masked, bool low) {
    const char* kimg = buf(kt);
    const char* vimg = kimg + TILEB;
    const int key0 = kt * BK;
    f32x16 s0 = f32x16{}, s1 = f32x16{};
    __builtin_amdgcn_s_setprio(1);
    {
      bf16x8 kf0[4], kf1[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        kf0[s] = lds_b128(kimg, swz(r, 2 * s + hh));
        kf1[s] = lds_b128(kimg, swz(32 + r, 2 * s + hh));
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        s0 = mfma(kf0[s], qf[s], s0);
        s1 = mfma(kf1[s], qf[s], s1);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    if (kt + 1 < ntiles) stage.load(kt + 1, buf(kt + 1));  // lands under softmax + PV
    if (masked) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k0i = key0 + crow(i, hh);
        if (k0i > myq) s0[i] = -INFINITY;
        if (k0i + 32 > myq) s1[i] = -INFINITY;
      }
    }
    if (kDoc && low) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k0i = key0 + crow(i, hh);
        if (k0i < lo) s0[i] = -INFINITY;
        if (k0i + 32 < lo) s1[i] = -INFINITY;
      }
    }
    float mx = max3(s0[0], s1[0], s0[1]);
#pragma unroll
    for (int i = 1; i < 16; ++i) mx = max3(mx, s1[i], i + 1 < 16 ? s0[i + 1] : s1[i]);
    const float mrow = xhalf_max(mx) * c;
    // per row: a row's frame depends on its own visible scores only; the wave-uniform `resc` only gates
    // the rescale branch, alpha == 1 exactly on unmoved rows
    const float mnew = mrow > m + kMaxSlack ? mrow : m;
    const bool resc = __any(mnew != m);
    float rs = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      s0[i] = fexp2(fmaf(s0[i], c, -mnew));
      s1[i] = fexp2(fmaf(s1[i], c, -mnew));
      rs += s0[i] + s1[i];
    }
    rs += __shfl_xor(rs, 32, 64);
    if (resc) {
      const float alpha = fexp2(m - mnew);
      l *= alpha;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[dt][i] *= alpha;
    }
    l += rs;
    m = mnew;
    const bf16x8 p00 = pack8(s0, 0), p01 = pack8(s0, 8), p10 = pack8(s1, 0), p11 = pack8(s1, 8);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const int col0 = 32 * dt;
      oacc[dt] = mfma(tr_frag(vimg, lane, 0 + 4 * hh, 8 + 4 * hh, col0), p00, oacc[dt]);
      oacc[dt] = mfma(tr_frag(vimg, lane, 16 + 4 * hh, 24 + 4 * hh, col0), p01, oacc[dt]);
      oacc[dt] = mfma(tr_frag(vimg, lane, 32 + 4 * hh, 40 + 4 * hh, col0), p10, oacc[dt]);
      oacc[dt] = mfma(tr_frag(vimg, lane, 48 + 4 * hh, 56 + 4 * hh, col0), p11, oacc[dt]);
    }
    __builtin_amdgcn_s_setprio(0);
  };

  stage.load(kt0, buf(kt0));
  dma_sync();
  int kt = kt0;
  // tiles up to ntiles-3 lie below every query of the block: no causal mask, no causal visibility test
  for (; kt < ntiles - 2; ++kt) {
    if (kDoc) {
      const int key0 = kt * BK;
      if (key0 + BK > wlo0)
        tile(kt, false, key0 < wlo1);
      else
        stage.load(kt + 1, buf(kt + 1));  // kt + 1 <= ntiles - 2
    } else {
      tile(kt, false, false);
    }
    dma_sync();
  }
  // the block's diagonal: tile ntiles-2 covers keys [128 qb, 128 qb + 64), ntiles-1 the next 64
  for (; kt < ntiles; ++kt) {
    const int key0 = kt * BK;
    if (key0 <= q0 + 31 && (!kDoc || key0 + BK > wlo0)) {
      tile(kt, key0 + BK - 1 > q0, kDoc && key0 < wlo1);
    } else if (kt + 1 < ntiles) {
      stage.load(kt + 1, buf(kt + 1));
    }
    dma_sync();
  }

  const float inv = 1.f / l;
  u16* orow = o + (((size_t)b * S + myq) * (size_t)(H) + hq) * D;
  // O^T [H*64, B*S] (ot != nullptr) from an LDS image of the block's [64 d][128 q] tile (the loop's last
  // dma_sync retired every LDS read, so the K/V buffers are free), written as 64-B row segments.  Same
  // bf16 values as O.  Row stride 136 elements (272 B) staggers the banks.
  constexpr int kOtStride = 136;
  u16* otl = reinterpret_cast<u16*>(smem);
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; g4 += 2) {
      u16x4 va, vb;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        va[e] = f2bf(oacc[dt][4 * g4 + e] * inv);
        vb[e] = f2bf(oacc[dt][4 * g4 + 4 + e] * inv);
      }
      if (ot) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          otl[(32 * dt + 8 * g4 + 4 * hh + e) * kOtStride + w * 32 + r] = va[e];
          otl[(32 * dt + 8 * g4 + 8 + 4 * hh + e) * kOtStride + w * 32 + r] = vb[e];
        }
      }
      *reinterpret_cast<uint4*>(orow + 32 * dt + 8 * g4 + 8 * hh) = widen(va, vb);
    }
  if (hh == 0) lse2[(size_t)(b * H + hq) * S + myq] = m + log2f(l);
  if (ot) {
    __syncthreads();
    const int d = t >> 2, part = t & 3;  // 4 threads per d row, 32 queries (64 B) each
    const size_t BS = (size_t)(gridDim.x / H) * S;
    u16* dst = ot + ((size_t)hq * D + d) * BS + (size_t)b * S + (size_t)qb * BQ + 32 * part;
    const u16* srcl = otl + d * kOtStride + 32 * part;
#pragma unroll
    for (int j = 0; j < 4; ++j) reinterpret_cast<u16x8*>(dst)[j] = reinterpret_cast<const u16x8*>(srcl)[j];
  }
}

// ==================================================================================== backward
// delta[b, h, q] = sum_d dO[b, q, h, d] * O[b, q, h, d] (one 8-lane group of 8 elements per row), plus
// what dK/dV starts its S / dP chains from: nls = -lse2 / c, ndl = -delta
__global__ __launch_bounds__(256) void attn64_bwd_pre_kernel(const u16* __restrict__ dout, const u16* __restrict__ out,
                                                              const float* __restrict__ lse2, float* __restrict__ delta,
                                                              float* __restrict__ nls, float* __restrict__ ndl, int B, int H,
                                                              int S, float inv_c) {
  const int row = blockIdx.x * 32 + (threadIdx.x >> 3);  // row = (b*S + s)*H + h
  const int i = threadIdx.x & 7;
  if (row >= B * S * H) return;
  const u16x8 a = reinterpret_cast<const u16x8*>(dout + (size_t)row * D)[i];
  const u16x8 bb = reinterpret_cast<const u16x8*>(out + (size_t)row * D)[i];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += bf2f(a[j]) * bf2f(bb[j]);
#pragma unroll
  for (int off = 4; off > 0; off >>= 1) s += __shfl_xor(s, off, 8);
  if (i == 0) {
    const int h = row % H, bs = row / H, sidx = bs % S, bidx = bs / S;
    const size_t o = ((size_t)bidx * H + h) * S + sidx;
    delta[o] = s;
    ndl[o] = -s;
    nls[o] = -lse2[o] * inv_c;
  }
}

// ============================================================================ backward dK/dV
// One workgroup = 128 keys of one (batch, kv-head), wave w the keys 32w .. 32w+31, one per lane & 31,
// whose K and V rows live in registers for the whole kernel.  It sweeps the q-heads of the GQA group x
// 32-query slices from the block's diagonal on.  A slice (Q and dO rows as swizzled images, -lse/c,
// -delta) arrives by LDS-DMA into the slot the previous slice left, one slice ahead, one dma_sync per
// slice.  Per slice and wave: S' = Q.K^T - lse/c and dP' = dO.V^T - delta (4 + 4 MFMAs, the negated
// values as initial accumulators), p = 2^(c S'), dS = p dP', both packed to bf16 as the B operands of
// dV^T += dO^T.P and dK^T += Q^T.dS (4 + 4 MFMAs, A by transposed reads of the same slice).
// Only the first KB/QT slices of each q-head touch the block's diagonal; a slice wholly above the
// wave's keys is skipped.  kDoc: seen from the key the mask is j <= i < doc_end[b, j], clamped to
// [key + 1, S]; the sweep ends at the slice that holds doc_end of the block's last key, a wave skips a
// slice that begins at or after doc_end of its last key and masks (query >= doc_end of the lane's key
// -> p = 0) a slice that ends after doc_end of its first key.
constexpr int SL_Q = 0, SL_DO = QT * ROWB, SL_LSE = 2 * QT * ROWB, SL_DEL = SL_LSE + 256, SL_BYTES = SL_DEL + 256;

template <bool kDoc>
__global__ __launch_bounds__(256, 2) void attn64_bwd_dkdv_kernel(const u16* __restrict__ q, const u16* __restrict__ k,
                                                                 const u16* __restrict__ v, const u16* __restrict__ dout,
                                                                 const float* __restrict__ nls, const float* __restrict__ ndl,
                                                                 u16* __restrict__ dk, u16* __restrict__ dv, int H, int Hkv,
                                                                 int S, float c, float scale,
                                                                 const int* __restrict__ doc_end) {
  __shared__ __attribute__((aligned(16))) char smem[2 * SL_BYTES];
  const int t = threadIdx.x, lane = t & 63, r = lane & 31, hh = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int kb = blockIdx.y;  // key block 0 has the longest sweep: heaviest first
  const int bk = xcd_head(blockIdx.x, gridDim.x), b = bk / Hkv, hk = bk % Hkv, G = H / Hkv;
  const size_t kvoff = ((size_t)(b * Hkv + hk) * S + (size_t)kb * KB) * D;
  const int krow = w * 32 + r, mykey = kb * KB + krow, kmin = kb * KB + w * 32;
  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    kf[s] = *reinterpret_cast<const bf16x8*>(k + kvoff + (size_t)krow * D + 16 * s + 8 * hh);
    vf[s] = *reinterpret_cast<const bf16x8*>(v + kvoff + (size_t)krow * D + 16 * s + 8 * hh);
  }
  f32x16 dvt[2], dkt[2];
  dvt[0] = dvt[1] = dkt[0] = dkt[1] = f32x16{};
  int qend = S, dmin = S, dmax = S, myend = S;  // sweep end; doc_end of the wave's first / last key, of the lane's
  if (kDoc) {
    const int* de = doc_end + (size_t)b * S;
    qend = clampi(de[kb * KB + KB - 1], kb * KB + KB, S);
    dmin = clampi(de[kmin], kmin + 1, S);
    dmax = clampi(de[kmin + 31], kmin + 32, S);
    myend = clampi(de[mykey], mykey + 1, S);
  }
  const int qt0 = (kb * KB) / QT, nqt = (kDoc ? (qend + QT - 1) / QT : S / QT) - qt0, nslice = G * nqt;

  const uint32_t qbytes = (uint32_t)((size_t)H * S * ROWB), dbytes = (uint32_t)((size_t)S * H * ROWB);
  const auto qrs = __builtin_amdgcn_make_buffer_rsrc((void*)(q + (size_t)b * H * S * D), 0, qbytes, 0x00020000);
  const auto drs = __builtin_amdgcn_make_buffer_rsrc((void*)(dout + (size_t)b * S * H * D), 0, dbytes, 0x00020000);
  const auto lrs = __builtin_amdgcn_make_buffer_rsrc((void*)((w == 0 ? nls : ndl) + (size_t)b * H * S), 0,
                                                     (uint32_t)((size_t)H * S * 4), 0x00020000);
  // wave w stages rows 8w .. 8w+7 of the slice's Q and dO (1 KiB each); waves 0 / 1 its -lse/c / -delta
  const int R = 8 * w + (lane >> 3);
  const uint32_t ch16 = 16 * ((lane & 7) ^ swz_slot(R));
  const uint32_t qv = (uint32_t)(R * ROWB) + ch16, dvo = (uint32_t)(R * H * ROWB) + ch16;
  auto sload = [&](int sh, int sj, char* buf) {
    const int hq = hk * G + sh, qbase = (qt0 + sj) * QT;
    const uint32_t qs = (uint32_t)(((size_t)hq * S + qbase) * ROWB), ds = (uint32_t)(((size_t)qbase * H + hq) * ROWB);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(qrs, (GTK64_LDS void*)(buf + SL_Q + 8 * w * ROWB), 16, qv, qs, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(drs, (GTK64_LDS void*)(buf + SL_DO + 8 * w * ROWB), 16, dvo, ds, 0, 0);
    if (w < 2)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(lrs, (GTK64_LDS void*)(buf + (w == 0 ? SL_LSE : SL_DEL)), 4, 4 * lane,
                                               (uint32_t)(((size_t)hq * S + qbase) * 4), 0, 0);
  };
  int cur_h = 0, cur_j = 0;  // this step's slice, walked in (q-head, query tile) order

  // buf: this slice, nbuf: the slot the next slice's DMA fills.  As __restrict__ parameters the two are
  // provably disjoint, so no read of buf waits for the DMA into nbuf, issued first.
  auto step = [&](int idx, const char* __restrict__ buf, char* __restrict__ nbuf) {
    const int nj = cur_j + 1 == nqt ? 0 : cur_j + 1, nh = cur_j + 1 == nqt ? cur_h + 1 : cur_h;
    if (idx + 1 < nslice) sload(nh, nj, nbuf);
    const int qbase = (qt0 + cur_j) * QT;
    const bool dead = qbase + QT - 1 < kmin || (kDoc && qbase >= dmax);  // wave-uniform: every score masked
    if (!dead) {
      f32x16 sacc, dpacc;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(buf + SL_LSE + 4 * (8 * g + 4 * hh));
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(buf + SL_DEL + 4 * (8 * g + 4 * hh));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sacc[4 * g + e] = l4[e];
          dpacc[4 * g + e] = d4[e];
        }
      }
      bf16x8 qa[4], da[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        qa[s] = lds_b128(buf + SL_Q, swz(r, 2 * s + hh));
        da[s] = lds_b128(buf + SL_DO, swz(r, 2 * s + hh));
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sacc = mfma(qa[s], kf[s], sacc);
        dpacc = mfma(da[s], vf[s], dpacc);
      }
      __builtin_amdgcn_s_setprio(0);
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[i] = fexp2(sacc[i] * c);
      if (qbase <= kmin + 31) {  // the wave's diagonal slice: query < key -> 0
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[i] = (mykey > qbase + crow(i, hh)) ? 0.f : sacc[i];
      }
      if (kDoc && qbase + QT > dmin) {  // some query of the slice is past some key's document
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[i] = (qbase + crow(i, hh) >= myend) ? 0.f : sacc[i];
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) dpacc[i] *= sacc[i];
      const bf16x8 p0 = pack8(sacc, 0), p1 = pack8(sacc, 8), d0 = pack8(dpacc, 0), d1 = pack8(dpacc, 8);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        dvt[dt] = mfma(tr_frag(buf + SL_DO, lane, 0 + 4 * hh, 8 + 4 * hh, 32 * dt), p0, dvt[dt]);
        dkt[dt] = mfma(tr_frag(buf + SL_Q, lane, 0 + 4 * hh, 8 + 4 * hh, 32 * dt), d0, dkt[dt]);
        dvt[dt] = mfma(tr_frag(buf + SL_DO, lane, 16 + 4 * hh, 24 + 4 * hh, 32 * dt), p1, dvt[dt]);
        dkt[dt] = mfma(tr_frag(buf + SL_Q, lane, 16 + 4 * hh, 24 + 4 * hh, 32 * dt), d1, dkt[dt]);
      }
      __builtin_amdgcn_s_setprio(0);
    }
    cur_h = nh, cur_j = nj;
    dma_sync();
  };

  sload(0, 0, smem);
  dma_sync();
  char* const s0 = smem;
  char* const s1 = smem + SL_BYTES;
  int idx = 0;
  for (; idx + 2 <= nslice; idx += 2) {
    step(idx, s0, s1);
    step(idx + 1, s1, s0);
  }
  if (idx < nslice) step(idx, s0, s1);

  u16* dkrow = dk + ((size_t)(b * Hkv + hk) * S + mykey) * D;
  u16* dvrow = dv + ((size_t)(b * Hkv + hk) * S + mykey) * D;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      u16x4 a4, b4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a4[e] = f2bf(dkt[dt][4 * g4 + e] * scale);
        b4[e] = f2bf(dvt[dt][4 * g4 + e]);
      }
      *reinterpret_cast<u16x4*>(dkrow + 32 * dt + 8 * g4 + 4 * hh) = a4;
      *reinterpret_cast<u16x4*>(dvrow + 32 * dt + 8 * g4 + 4 * hh) = b4;
    }
}

// ============================================================================ backward dQ
// Forward-shaped (query on the lane): per 64-key tile S^T = K.Q^T and dP^T = V.dO^T (2 x 4 MFMAs each),
// p = 2^(c s - lse2), dS = p (dP - delta) packed to bf16 as the B operand of dQ^T += K^T.dS^T (K^T by
// transposed reads of the K image).  The tile's LDS images are __restrict__ parameters, so the
// compiler's LDS-DMA wait tracking sees the reads and the next tile's DMA as disjoint.
// kMasked: the causal mask; kLow: the document's lower one (key < lo -> p = 0).
template <bool kMasked, bool kLow>
__device__ __forceinline__ void dq_tile(const char* __restrict__ kimg, const char* __restrict__ vimg, char* __restrict__ nimg,
                                        bool prefetch, const KVStage& stage, int kt, const bf16x8 (&qf)[4],
                                        const bf16x8 (&df)[4], f32x16 (&dqt)[2], float lse_q, float del_q, int lane, int r,
                                        int hh, int myq, float c, int lo) {
  const int key0 = kt * BK;
  f32x16 s0 = f32x16{}, s1 = f32x16{}, e0 = f32x16{}, e1 = f32x16{};
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const bf16x8 k0 = lds_b128(kimg, swz(r, 2 * s + hh)), k1 = lds_b128(kimg, swz(32 + r, 2 * s + hh));
    const bf16x8 v0 = lds_b128(vimg, swz(r, 2 * s + hh)), v1 = lds_b128(vimg, swz(32 + r, 2 * s + hh));
    s0 = mfma(k0, qf[s], s0);
    s1 = mfma(k1, qf[s], s1);
    e0 = mfma(v0, df[s], e0);
    e1 = mfma(v1, df[s], e1);
  }
  __builtin_amdgcn_s_setprio(0);
  if (prefetch) stage.load(kt + 1, nimg);  // lands under the dQ MFMAs
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float p0 = fexp2(fmaf(s0[i], c, -lse_q));
    float p1 = fexp2(fmaf(s1[i], c, -lse_q));
    if (kMasked) {
      const int kk = key0 + crow(i, hh);
      if (kk > myq) p0 = 0.f;
      if (kk + 32 > myq) p1 = 0.f;
    }
    if (kLow) {
      const int kk = key0 + crow(i, hh);
      if (kk < lo) p0 = 0.f;
      if (kk + 32 < lo) p1 = 0.f;
    }
    s0[i] = p0 * (e0[i] - del_q);
    s1[i] = p1 * (e1[i] - del_q);
  }
  const bf16x8 d00 = pack8(s0, 0), d01 = pack8(s0, 8), d10 = pack8(s1, 0), d11 = pack8(s1, 8);
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    dqt[dt] = mfma(tr_frag(kimg, lane, 0 + 4 * hh, 8 + 4 * hh, 32 * dt), d00, dqt[dt]);
    dqt[dt] = mfma(tr_frag(kimg, lane, 16 + 4 * hh, 24 + 4 * hh, 32 * dt), d01, dqt[dt]);
    dqt[dt] = mfma(tr_frag(kimg, lane, 32 + 4 * hh, 40 + 4 * hh, 32 * dt), d10, dqt[dt]);
    dqt[dt] = mfma(tr_frag(kimg, lane, 48 + 4 * hh, 56 + 4 * hh, 32 * dt), d11, dqt[dt]);
  }
  __builtin_amdgcn_s_setprio(0);
}

// kDoc: the forward's tile range and per-wave tests.  Two tile bodies: the unmasked one, and one with
// both masks for every edge tile (the diagonal pair, and under kDoc a tile that begins before doc_start
// of the wave's last query); a mask a tile does not need selects nothing.
template <bool kDoc>
__global__ __launch_bounds__(256, 2) void attn64_bwd_dq_kernel(const u16* __restrict__ q, const u16* __restrict__ k,
                                                               const u16* __restrict__ v, const u16* __restrict__ dout,
                                                               const float* __restrict__ lse2, const float* __restrict__ delta,
                                                               u16* __restrict__ dq, int H, int Hkv, int S, float c, float scale,
                                                               const int* __restrict__ doc_start) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILEB];  // [buf][K image | V image]
  const int t = threadIdx.x, lane = t & 63, r = lane & 31, hh = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nqb = gridDim.y, qb = nqb - 1 - blockIdx.y;
  const int bh = xcd_head(blockIdx.x, gridDim.x), b = bh / H, hq = bh % H, hk = hq / (H / Hkv);
  const size_t kvoff = ((size_t)(b * Hkv + hk) * S) * D;
  const int q0 = qb * BQ + w * 32, myq = q0 + r;
  const u16* qrow = q + ((size_t)(b * H + hq) * S + myq) * D;
  const u16* dorow = dout + (((size_t)b * S + myq) * H + hq) * D;
  bf16x8 qf[4], df[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8*>(qrow + 16 * s + 8 * hh);
    df[s] = *reinterpret_cast<const bf16x8*>(dorow + 16 * s + 8 * hh);
  }
  const float lse_q = lse2[(size_t)(b * H + hq) * S + myq], del_q = delta[(size_t)(b * H + hq) * S + myq];
  f32x16 dqt[2];
  dqt[0] = dqt[1] = f32x16{};
  const int ntiles = (qb * BQ + BQ) / BK;
  DocTiles dt_;
  if (kDoc) dt_ = DocTiles(doc_start + (size_t)b * S, qb, q0, myq);
  const KVStage stage(k + kvoff, v + kvoff, S, w, lane);
  auto buf = [&](int kt) { return smem + (kt & 1) * (2 * TILEB); };
  auto tile = [&](int kt, bool edge) {
    const char* kimg = buf(kt);
    if (edge)
      dq_tile<true, kDoc>(kimg, kimg + TILEB, buf(kt + 1), kt + 1 < ntiles, stage, kt, qf, df, dqt, lse_q, del_q, lane, r, hh, myq,
                          c, dt_.lo);
    else
      dq_tile<false, false>(kimg, kimg + TILEB, buf(kt + 1), kt + 1 < ntiles, stage, kt, qf, df, dqt, lse_q, del_q, lane, r, hh,
                            myq, c, 0);
  };
  const int kt0 = kDoc ? dt_.kt0 : 0;
  stage.load(kt0, buf(kt0));
  dma_sync();
  for (int kt = kt0; kt < ntiles; ++kt) {
    const int key0 = kt * BK;
    if (key0 <= q0 + 31 && (!kDoc || key0 + BK > dt_.wlo0)) {
      tile(kt, kt >= ntiles - 2 || (kDoc && key0 < dt_.wlo1));
    } else if (kt + 1 < ntiles) {
      stage.load(kt + 1, buf(kt + 1));
    }
    dma_sync();
  }
  u16* out = dq + ((size_t)(b * H + hq) * S + myq) * D;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; g4 += 2) {
      u16x4 va, vb;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        va[e] = f2bf(dqt[dt][4 * g4 + e] * scale);
        vb[e] = f2bf(dqt[dt][4 * g4 + 4 + e] * scale);
      }
      *reinterpret_cast<uint4*>(out + 32 * dt + 8 * g4 + 8 * hh) = widen(va, vb);
    }
}

}  // namespace gtk_attn64
