// Split-KV flash attention for a short query chunk against long K/V (gfx950, head dim 128).
//
// attn_fwd2_kernel and attn_bwd_dq2n_kernel launch one workgroup per (batch, q-head, 128 queries), and that
// workgroup walks all of its visible keys alone.  A context-parallel rank at B 1 or a prefill chunk against a
// long cache launches a few hundred such workgroups or fewer for the chip's 512 slots (256 CUs x 2), each with
// a long walk.  The kernels here add the missing parallelism, over the keys:
//
//   attn_fwd_split_kernel   grid (B*H, Sq/128, n).  Workgroup (., qb, z) runs the online softmax over split
//                           z of query block qb's key blocks (SplitRange, attention_splitkv.h) and writes its
//                           own normalised O in fp32 and its own lse2; an empty split writes lse2 = -inf and
//                           returns before it stages anything.
//   splitkv_merge_kernel<true>   one 32-lane group per output row: M = max_z lse2_z, w_z = 2^(lse2_z - M),
//                           O = sum_z w_z O_z / sum_z w_z in fp32, rounded once to bf16; lse2 = M + log2 sum_z w_z.
//   attn_dq_split_kernel    the same grid and ranges.  Given the merged lse2 and delta, dQ is linear in the
//                           key tiles: each split writes its fp32 partial of dQ / scale.
//   splitkv_merge_kernel<false>  sums the non-empty splits' partials, times scale, rounded once to bf16.
//
// Both merges take the splits in index order, so a result does not depend on which workgroup finished first,
// and neither reads an empty split's partial (the workspace is not cleared).  dK/dV is parallel over key
// blocks already and stays gtk_qoff::launch_dkdv.
//
// What is kept from attn_fwd2_kernel / attn_bwd_dq2n_kernel, through the helpers of attention_kernels.h: the
// swapped QK^T with the query on the lane, P and dS as the next MFMA's B operand, the XOR-swizzled K/V image,
// the LDS-DMA double buffer with one barrier per 64-key tile (KVStage, dma_sync), the slack-8 running max, the
// XCD head mapping and two workgroups per CU.  A split begins at an even 64-key tile, so the buffer parity is
// the tile's as before.  What differs:
//   * the diagonal tile pair lies in the last non-empty split only: every other split is the branch-free
//     unmasked loop and nothing else (no mask code is reached, no visibility test);
//   * launch order: blockIdx.y still walks the query blocks heaviest first, and z is the slowest grid
//     dimension, so the splits of one index are dispatched together.  The splits of a query block are equally
//     long but for the last, which is the shortest and is dispatched last;
//   * the epilogue stores fp32 accumulators as they lie in the registers (four consecutive columns, 16 B, per
//     accumulator quad): no bf16 pack, no lane exchange, no O^T.
//
// Built with attention_qoff.hip's flags (packed fp32 VALU off, the MFMA VGPR form).
#define GTK_ATTN_SPLITKV_TU 1
#include "attention_kernels.h"
#include "attention_splitkv.h"

namespace gtk_splitkv {

constexpr int kTileBytes = 2 * BK * D * 2;  // one LDS buffer: [K image | V image]

// What the forward and the dQ kernel share: who the workgroup is and which 64-key tiles it walks.
struct SplitBlock {
  int qb, z, b, hq, hk, q0, myq, qpos0, kt0, kte, ktu;
  bool empty;
  size_t kvoff, row;  // row: (b*H + hq)*Sq + myq, the index of lse2, delta and dQ
  __device__ __forceinline__ SplitBlock(int w, int r, int H, int Hkv, int Sq, int Sk, int q_offset) {
    qb = (int)gridDim.y - 1 - (int)blockIdx.y;  // heaviest first
    z = blockIdx.z;
    const int bh = xcd_head(blockIdx.x, gridDim.x);
    b = bh / H, hq = bh % H, hk = hq / (H / Hkv);
    q0 = qb * BQ + w * 32, myq = q0 + r, qpos0 = q_offset + q0;
    const SplitRange sr(q_offset, qb, gridDim.z);
    empty = sr.begin(z) >= sr.P;
    kt0 = 2 * sr.begin(z), kte = 2 * sr.end(z);       // 64-key tiles [kt0, kte)
    ktu = sr.end(z) == sr.P ? kte - 2 : kte;          // [kt0, ktu) unmasked; then the diagonal pair, if it is ours
    kvoff = ((size_t)(b * Hkv + hk) * Sk) * D;
    row = (size_t)(b * H + hq) * Sq + myq;
  }
};

__global__ __launch_bounds__(256, 2) void attn_fwd_split_kernel(const u16* __restrict__ q, const u16* __restrict__ k,
                                                                const u16* __restrict__ v, float* __restrict__ o_part,
                                                                float* __restrict__ lse_part, int H, int Hkv, int Sq, float c,
                                                                int Sk, int q_offset) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kTileBytes];
  const int t = threadIdx.x, lane = t & 63, r = lane & 31, hh = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const SplitBlock sb(w, r, H, Hkv, Sq, Sk, q_offset);
  const size_t nrows = (size_t)gridDim.x * Sq;  // B*H*Sq: rows of one split's partials
  float* lrow = lse_part + (size_t)sb.z * nrows + sb.row;
  if (sb.empty) {  // wave-uniform, the whole workgroup
    if (hh == 0) *lrow = -INFINITY;
    return;
  }
  const int myq = sb.myq, qpos = q_offset + myq, kte = sb.kte;
  const u16* qp = q + sb.row * D;
  bf16x8 qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qp + 16 * s + 8 * hh);

  f32x16 oacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x16{};
  float m = -INFINITY, l = 0.f;  // m in units of log2 (score * c)
  const KVStage stage(k + sb.kvoff, v + sb.kvoff, Sk, w, lane);

  // one KV tile, as attn_fwd2_kernel's: QK^T, DMA of the next tile, online softmax, PV
  auto tile = [&](int kt, bool masked) {
    char* kimg = smem + (kt & 1) * kTileBytes;
    char* vimg = kimg + BK * D * 2;
    const int key0 = kt * BK;
    f32x16 s0 = f32x16{}, s1 = f32x16{};
    __builtin_amdgcn_s_setprio(1);
    {
      bf16x8 kf0[8], kf1[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        kf0[s] = lds_b128(kimg, swz(r, 2 * s + hh));
        kf1[s] = lds_b128(kimg, swz(32 + r, 2 * s + hh));
      }
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        s0 = mfma(kf0[s], qf[s], s0);
        s1 = mfma(kf1[s], qf[s], s1);
      }
      __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);  // 8 reads ahead, then read/MFMA pairs
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x8, 8, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    if (kt + 1 < kte) stage.load(kt + 1, smem + ((kt + 1) & 1) * kTileBytes);  // lands under softmax + PV
    if (masked) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k0i = key0 + crow(i, hh);
        if (k0i > qpos) s0[i] = -INFINITY;
        if (k0i + 32 > qpos) s1[i] = -INFINITY;
      }
    }
    float mx = max3(s0[0], s1[0], s0[1]);
#pragma unroll
    for (int i = 1; i < 16; ++i) mx = max3(mx, s1[i], i + 1 < 16 ? s0[i + 1] : s1[i]);
    const float mrow = xhalf_max(mx) * c;
    const float mnew = mrow > m + kMaxSlack ? mrow : m;  // per row; `resc` only gates the branch
    const bool resc = __any(mnew != m);
    float rs = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      s0[i] = fexp2(fmaf(s0[i], c, -mnew));
      s1[i] = fexp2(fmaf(s1[i], c, -mnew));
      rs += s0[i] + s1[i];
    }
    rs += __shfl_xor(rs, 32, 64);
    if (resc) {  // alpha == 1 everywhere otherwise
      const float alpha = fexp2(m - mnew);
      l *= alpha;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[dt][i] *= alpha;
    }
    l += rs;
    m = mnew;
    const bf16x8 p00 = pack8(s0, 0), p01 = pack8(s0, 8), p10 = pack8(s1, 0), p11 = pack8(s1, 8);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const int col0 = 32 * dt;
      oacc[dt] = mfma(tr_frag(vimg, lane, 0 + 4 * hh, 8 + 4 * hh, col0), p00, oacc[dt]);
      oacc[dt] = mfma(tr_frag(vimg, lane, 16 + 4 * hh, 24 + 4 * hh, col0), p01, oacc[dt]);
      oacc[dt] = mfma(tr_frag(vimg, lane, 32 + 4 * hh, 40 + 4 * hh, col0), p10, oacc[dt]);
      oacc[dt] = mfma(tr_frag(vimg, lane, 48 + 4 * hh, 56 + 4 * hh, col0), p11, oacc[dt]);
    }
    __builtin_amdgcn_s_setprio(0);
  };
  stage.load(sb.kt0, smem + (sb.kt0 & 1) * kTileBytes);
  dma_sync();
  int kt = sb.kt0;
  // tiles that lie entirely below every query of the block: all of a split that is not the last
  for (; kt < sb.ktu; ++kt) {
    tile(kt, false);
    dma_sync();
  }
  // the last non-empty split ends with the block's diagonal pair: a wave skips a tile it cannot see
  for (; kt < kte; ++kt) {
    const int key0 = kt * BK;
    if (key0 <= sb.qpos0 + 31) {
      tile(kt, key0 + BK - 1 > sb.qpos0);
    } else if (kt + 1 < kte) {
      stage.load(kt + 1, smem + ((kt + 1) & 1) * kTileBytes);
    }
    dma_sync();
  }
  // every row has seen a key: all of an unmasked tile, or itself on the diagonal, so l > 0
  const float inv = 1.f / l;
  float* orow = o_part + ((size_t)sb.z * nrows + ((size_t)sb.b * Sq + myq) * H + sb.hq) * D;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 o4 = {oacc[dt][4 * g] * inv, oacc[dt][4 * g + 1] * inv, oacc[dt][4 * g + 2] * inv, oacc[dt][4 * g + 3] * inv};
      *reinterpret_cast<f32x4*>(orow + 32 * dt + 8 * g + 4 * hh) = o4;
    }
  if (hh == 0) *lrow = m + log2f(l);
}

__global__ __launch_bounds__(256, 2) void attn_dq_split_kernel(const u16* __restrict__ q, const u16* __restrict__ k,
                                                               const u16* __restrict__ v, const u16* __restrict__ dout,
                                                               const float* __restrict__ lse2, const float* __restrict__ delta,
                                                               float* __restrict__ dq_part, int H, int Hkv, int Sq, float c,
                                                               int Sk, int q_offset) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kTileBytes];
  const int t = threadIdx.x, lane = t & 63, r = lane & 31, hh = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const SplitBlock sb(w, r, H, Hkv, Sq, Sk, q_offset);
  if (sb.empty) return;  // the reduce does not read this split's partial
  const int myq = sb.myq, qpos = q_offset + myq, kte = sb.kte;
  const u16* qrow = q + sb.row * D;
  const u16* dorow = dout + (((size_t)sb.b * Sq + myq) * H + sb.hq) * D;
  bf16x8 qf[8], df[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    qf[s] = *reinterpret_cast<const bf16x8*>(qrow + 16 * s + 8 * hh);
    df[s] = *reinterpret_cast<const bf16x8*>(dorow + 16 * s + 8 * hh);
  }
  const float lse_q = lse2[sb.row], del_q = delta[sb.row];
  f32x16 dqt[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dqt[dt] = f32x16{};
  const KVStage stage(k + sb.kvoff, v + sb.kvoff, Sk, w, lane);
  stage.load(sb.kt0, smem + (sb.kt0 & 1) * kTileBytes);
  dma_sync();
  int kt = sb.kt0;
  for (; kt < sb.ktu; ++kt) {
    const char* kimg = smem + (kt & 1) * kTileBytes;
    dq_tile_na<false>(kimg, kimg + BK * D * 2, smem + ((kt + 1) & 1) * kTileBytes, kt + 1 < kte, stage, kt, qf, df, dqt, lse_q,
                      del_q, lane, r, hh, qpos, c);
    dma_sync();
  }
  // the diagonal pair, one masked tile body for both: the mask selects nothing on a tile that lies below
  // the wave's queries, so its values are the unmasked tile's
  for (; kt < kte; ++kt) {
    const char* kimg = smem + (kt & 1) * kTileBytes;
    char* nimg = smem + ((kt + 1) & 1) * kTileBytes;
    if (kt * BK <= sb.qpos0 + 31) {
      dq_tile_na<true>(kimg, kimg + BK * D * 2, nimg, kt + 1 < kte, stage, kt, qf, df, dqt, lse_q, del_q, lane, r, hh, qpos, c);
    } else if (kt + 1 < kte) {
      stage.load(kt + 1, nimg);
    }
    dma_sync();
  }
  const size_t nrows = (size_t)gridDim.x * Sq;
  float* out = dq_part + ((size_t)sb.z * nrows + sb.row) * D;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 d4 = {dqt[dt][4 * g], dqt[dt][4 * g + 1], dqt[dt][4 * g + 2], dqt[dt][4 * g + 3]};
      *reinterpret_cast<f32x4*>(out + 32 * dt + 8 * g + 4 * hh) = d4;
    }
}

// One 32-lane group per row of 128 columns, four columns a lane, the splits in index order.
//   kWeighted: part is o_part [n, B, Sq, H, 128] and the row (b*Sq + s)*H + h; the weights come from
//              lse_part [n, B, H, Sq].  A split with lse2 = -inf is empty: weight 0, its O not read (it may be
//              uninitialised memory, and 0 * NaN would be NaN).  Split 0 is never empty, so M is finite and
//              the sum of weights is at least 1.
//   else:      part is dq_part [n, B, H, Sq, 128] and the row (b*H + h)*Sq + s; the non-empty splits are the
//              first SplitRange::nonempty() of the row's query block, the others were never written.
template <bool kWeighted>
__global__ __launch_bounds__(256) void splitkv_merge_kernel(const float* __restrict__ part, const float* __restrict__ lse_part,
                                                            u16* __restrict__ out, float* __restrict__ lse2, int rows, int H,
                                                            int Sq, float scale, int q_offset, int n) {
  const int row = blockIdx.x * 8 + (threadIdx.x >> 5), c4 = threadIdx.x & 31;
  if (row >= rows) return;
  const float* p = part + (size_t)row * D + 4 * c4;
  const size_t zstride = (size_t)rows * D;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (kWeighted) {
    const int h = row % H, bs = row / H, s = bs % Sq, b = bs / Sq;
    const size_t li = ((size_t)b * H + h) * Sq + s;
    float M = -INFINITY;
    for (int z = 0; z < n; ++z) M = fmaxf(M, lse_part[(size_t)z * rows + li]);
    float wsum = 0.f;
    for (int z = 0; z < n; ++z) {
      const float lz = lse_part[(size_t)z * rows + li];
      if (lz == -INFINITY) continue;
      const float wz = fexp2(lz - M);
      const f32x4 x = *reinterpret_cast<const f32x4*>(p + z * zstride);
      wsum += wz;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(wz, x[e], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] /= wsum;
    if (c4 == 0) lse2[li] = M + log2f(wsum);
  } else {
    const int nz = SplitRange(q_offset, (row % Sq) / BQ, n).nonempty();
    for (int z = 0; z < nz; ++z) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(p + z * zstride);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += x[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] *= scale;
  }
  const u16x4 o4 = {f2bf(acc[0]), f2bf(acc[1]), f2bf(acc[2]), f2bf(acc[3])};
  *reinterpret_cast<u16x4*>(out + (size_t)row * D + 4 * c4) = o4;
}

void launch_fwd(dim3 grid, hipStream_t st, const u16* q, const u16* k, const u16* v, float* o_part, float* lse_part, int H,
                int Hkv, int Sq, float c, int Sk, int q_offset) {
  hipLaunchKernelGGL(attn_fwd_split_kernel, grid, dim3(256), 0, st, q, k, v, o_part, lse_part, H, Hkv, Sq, c, Sk, q_offset);
}
void launch_combine(hipStream_t st, const float* o_part, const float* lse_part, u16* o, float* lse2, int B, int H, int Sq,
                    int n) {
  const int rows = B * Sq * H;
  // rounded up: the decode kernel's rows need not be a multiple of 8 (the kernel guards row >= rows)
  hipLaunchKernelGGL(splitkv_merge_kernel<true>, dim3((rows + 7) / 8), dim3(256), 0, st, o_part, lse_part, o, lse2, rows, H, Sq,
                     1.f, 0, n);
}
void launch_dq(dim3 grid, hipStream_t st, const u16* q, const u16* k, const u16* v, const u16* dout, const float* lse2,
               const float* delta, float* dq_part, int H, int Hkv, int Sq, float c, int Sk, int q_offset) {
  hipLaunchKernelGGL(attn_dq_split_kernel, grid, dim3(256), 0, st, q, k, v, dout, lse2, delta, dq_part, H, Hkv, Sq, c, Sk,
                     q_offset);
}
void launch_dq_reduce(hipStream_t st, const float* dq_part, u16* dq, int B, int H, int Sq, float scale, int q_offset, int n) {
  const int rows = B * H * Sq;
  hipLaunchKernelGGL(splitkv_merge_kernel<false>, dim3(rows / 8), dim3(256), 0, st, dq_part, static_cast<const float*>(nullptr),
                     dq, static_cast<float*>(nullptr), rows, H, Sq, scale, q_offset, n);
}

}  // namespace gtk_splitkv
