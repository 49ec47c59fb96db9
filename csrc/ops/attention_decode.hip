// Decode attention over a ragged KV cache (gfx950, head dim 128): 1 to 8 new tokens per sequence against
// that sequence's own number of valid keys, read on the device.
//
// The other attention kernels give one workgroup 128 queries of one q-head.  A decode step has a handful of
// queries and is nothing but a K/V stream, so the work is laid out over the keys instead:
//
//   attn_decode_kernel   grid (B*Hkv, n), 256 threads.  One workgroup serves ALL G = H / Hkv q-heads and all Sq
//                        queries of one KV head over split z of that sequence's 64-key tiles: K/V leaves HBM
//                        once per GQA group, not G times.  MFMA query column r (the lane's r of the swapped
//                        QK^T) is row g * Sq + i of the group, G * Sq <= 32; the columns past it carry zeros
//                        and are never stored.
//   * The four waves split KEYS.  Wave w walks tiles t0 + w, t0 + w + 4, .. of the split with its own m, l and
//     oacc[4]: the 32x32x16 bf16 MFMA chain of the forward (P from the S accumulators as the next MFMA's B
//     operand, the slack-8 running max), and no barrier inside the walk.
//   * Split ranges are per sequence: T = ceil(kv_len[b] / 64) tiles in contiguous balanced ranges, the first
//     T % n splits one tile longer, so split 0 is never empty (the merge relies on it).  A split without a tile
//     writes lse2 = -inf for its rows and returns before it stages anything.
//   * K has no reuse: every byte is consumed by one lane of one wave, so it goes from global memory straight
//     into the A-operand registers, loaded for the wave's next tile right after QK^T of this one.  The dot
//     product over d is order-free: lane (r, hh) holds dims 64 hh + 8 s .. + 7 of its key for MFMA s (and of
//     its query), so a lane's eight 16-byte loads are one aligned 128-byte line.
//   * V needs the transposed fragment read (tr_frag), so it goes through LDS: each wave has its own LDS-DMA
//     double buffer of 64-key V tiles in the forward's swizzled image, 16 KiB x 2 x 4 waves = 128 KiB, the
//     next tile issued after QK^T.  That is one workgroup per CU and one wave per SIMD, which suits a kernel
//     that is memory-bound on a single stream per wave: 32 KiB of K/V in flight per wave is what hides the
//     HBM latency, not a second wave.
//   * Both buffer descriptors are built from wave-uniform values, the sequence's base address and num_records
//     = the clamped kv_len[b] rows, and the tile offset goes into the VGPR offset (the scalar offset is not
//     range-checked).  No content of kv_len moves an access outside the cache, and K rows past kv_len[b] read
//     as zero.  For V the tail tile does not rely on what an out-of-range LDS-DMA leaves in LDS: the masked
//     tile body selects zero into the V fragments' rows past kv_len[b], since p = 0 times a stale NaN is NaN.
//   * Only tiles that reach past position kv_len[b] - Sq take the masked body (the last tile, or the last two
//     when the chunk straddles a tile edge).  The running max starts from the finite kMinM, so a row whose
//     wave owns only keys it does not see ends with l = 0, O = 0 and a weight of exactly 0 in the merge.
//   * The four waves' (m, l, O) merge through LDS in wave order (the V buffers are free by then, 64 KiB + 1
//     KiB).  At n = 1 the workgroup rounds once to bf16 and writes o and lse2 itself; at n > 1 it writes its
//     normalised fp32 partial and lse2 in the layouts gtk_splitkv's weighted merge reads, which then combines
//     them in split order.  A row that sees no key of its split writes lse2 = -inf like an empty split.
//
// Built with attention_splitkv.hip's flags (packed fp32 VALU off, the MFMA VGPR form).
#define GTK_ATTN_SPLITKV_TU 1
#include "attention_kernels.h"

namespace gtk_decode {

using namespace gtk_splitkv;  // the helpers of attention_kernels.h

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kVTile = BK * D * 2;        // one 64-key V image
constexpr int kWaveLds = 2 * kVTile;      // a wave's double buffer
constexpr int kMergeO = 4 * 16 * 64 * 16; // [wave][accumulator quad][lane] f32x4

__device__ __forceinline__ bf16x8 load_b128(__amdgpu_buffer_rsrc_t rs, uint32_t voff) {
  return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, 0, 0));
}

// rows kb + {0..3} (elements 0..3) and kb + 8 + {0..3} (4..7) of a V fragment: those at or past len become 0
__device__ __forceinline__ bf16x8 zero_past(bf16x8 x, int kb, int len) {
  u32x4 u = __builtin_bit_cast(u32x4, x);
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int k0 = kb + 8 * (d >> 1) + 2 * (d & 1);
    u[d] &= (k0 < len ? 0xffffu : 0u) | (k0 + 1 < len ? 0xffff0000u : 0u);
  }
  return __builtin_bit_cast(bf16x8, u);
}

__global__ __launch_bounds__(256) void attn_decode_kernel(const u16* __restrict__ q, const u16* __restrict__ kc,
                                                          const u16* __restrict__ vc, const int* __restrict__ kv_len,
                                                          u16* __restrict__ o, float* __restrict__ lse2,
                                                          float* __restrict__ o_part, float* __restrict__ lse_part, int H,
                                                          int Hkv, int Sq, int Smax, float c) {
  __shared__ __attribute__((aligned(16))) char smem[4 * kWaveLds];
  const int t = threadIdx.x, lane = t & 63, r = lane & 31, hh = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int n = gridDim.y, z = blockIdx.y;
  const int bk = blockIdx.x, b = bk / Hkv, hk = bk % Hkv, G = H / Hkv;
  const int len = clampi(kv_len[b], Sq, Smax);
  const int T = (len + BK - 1) / BK, per = T / n, rem = T % n;
  const int t0 = z * per + (z < rem ? z : rem), t1 = t0 + per + (z < rem ? 1 : 0);  // this split's tiles
  const bool real = r < G * Sq;
  const int g = r / Sq, i = r - g * Sq;
  const size_t li = (size_t)(b * H + hk * G) * Sq + r;  // the row of q and of lse2 [B, H, Sq]
  const size_t ocol = ((size_t)(b * Sq + i) * H + hk * G + g) * D + 32 * w + 4 * hh;  // in o [B, Sq, H, D]: the merge's columns
  const size_t rows = (size_t)(gridDim.x / Hkv) * H * Sq;
  if (t0 == t1) {  // workgroup-uniform; only at n > 1
    if (real && t < 32) lse_part[z * rows + li] = -INFINITY;
    return;
  }
  const int qpos = real ? len - Sq + i : len - 1;  // the lane's query sees the keys j <= qpos

  bf16x8 qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) qf[s] = bf16x8{};
  if (real) {
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(q + li * D + 64 * hh + 8 * s);
  }

  const size_t kvoff = (size_t)bk * Smax * D;
  const uint32_t bytes = (uint32_t)len * (D * 2);
  const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc((void*)(kc + kvoff), 0, bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc((void*)(vc + kvoff), 0, bytes, 0x00020000);
  const uint32_t koff = (uint32_t)(r * (D * 2) + 128 * hh);
  uint32_t voff[4];  // KVStage's source swizzle: instruction ii stages rows 4 ii + (lane >> 4), voff[ii & 3] + 1024 (ii & ~3)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int R = 4 * j + (lane >> 4);
    voff[j] = (uint32_t)(R * D * 2 + 16 * ((lane & 15) ^ (((R & 3) << 2) | ((R >> 2) & 3))));
  }
  char* vbuf = smem + w * kWaveLds;

  bf16x8 kf0[8], kf1[8];
  auto load_k = [&](int kt) {
    const uint32_t o0 = koff + (uint32_t)kt * (BK * D * 2);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      kf0[s] = load_b128(krs, o0 + 16 * s);
      kf1[s] = load_b128(krs, o0 + 32 * D * 2 + 16 * s);
    }
  };
  auto load_v = [&](int kt, char* img) {
    const uint32_t o0 = (uint32_t)kt * (BK * D * 2);
#pragma unroll
    for (int ii = 0; ii < 16; ++ii)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(vrs, (LDS_AS void*)(img + ii * 1024), 16, voff[ii & 3] + 1024 * (ii & ~3) + o0, 0, 0,
                                               0);
  };

  f32x16 oacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x16{};
  float m = kMinM, l = 0.f;  // m in units of log2 (score * c)

  // one 64-key tile, the wave's j-th: QK^T from the registers, the next tile's loads, online softmax, PV
  auto tile = [&](int kt, int j, bool masked) {
    const char* vimg = vbuf + (j & 1) * kVTile;
    const int key0 = kt * BK;
    f32x16 s0 = f32x16{}, s1 = f32x16{};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      s0 = mfma(kf0[s], qf[s], s0);
      s1 = mfma(kf1[s], qf[s], s1);
    }
    if (kt + 4 < t1) {  // lands under softmax + PV
      load_k(kt + 4);
      load_v(kt + 4, vbuf + ((j + 1) & 1) * kVTile);
    }
    if (masked) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int k0e = key0 + crow(e, hh);
        if (k0e > qpos) s0[e] = -INFINITY;
        if (k0e + 32 > qpos) s1[e] = -INFINITY;
      }
    }
    float mx = max3(s0[0], s1[0], s0[1]);
#pragma unroll
    for (int e = 1; e < 16; ++e) mx = max3(mx, s1[e], e + 1 < 16 ? s0[e + 1] : s1[e]);
    const float mrow = xhalf_max(mx) * c;  // -inf where the row sees no key of the tile: m stays
    const float mnew = mrow > m + kMaxSlack ? mrow : m;
    const bool resc = __any(mnew != m);
    float rs = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      s0[e] = fexp2(fmaf(s0[e], c, -mnew));
      s1[e] = fexp2(fmaf(s1[e], c, -mnew));
      rs += s0[e] + s1[e];
    }
    rs += __shfl_xor(rs, 32, 64);
    if (resc) {  // alpha == 1 everywhere otherwise; from kMinM it is 0 on l = 0, O = 0
      const float alpha = fexp2(m - mnew);
      l *= alpha;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[dt][e] *= alpha;
    }
    l += rs;
    m = mnew;
    const bf16x8 p[4] = {pack8(s0, 0), pack8(s0, 8), pack8(s1, 0), pack8(s1, 8)};
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        bf16x8 vf = tr_frag(vimg, lane, 16 * f + 4 * hh, 16 * f + 8 + 4 * hh, 32 * dt);
        if (masked) vf = zero_past(vf, key0 + 16 * f + 4 * hh, len);
        oacc[dt] = mfma(vf, p[f], oacc[dt]);
      }
    // the next tile's K and V have landed and this tile's LDS reads have returned: the wave's own buffers
    // need no barrier, and the next DMA may overwrite the image just read
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  };

  int kt = t0 + w, j = 0;
  if (kt < t1) {
    load_k(kt);
    load_v(kt, vbuf);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  const int tm = (len - Sq + 1) / BK;  // the first tile that holds a key past some query's position
  for (; kt < t1 && kt < tm; kt += 4, ++j) tile(kt, j, false);
  for (; kt < t1; kt += 4, ++j) tile(kt, j, true);

  // ---- the four waves' (m, l, O) in wave order
  __syncthreads();  // every wave is past its last V read: the buffers become the merge area
  float* ml = reinterpret_cast<float*>(smem + kMergeO);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const f32x4 o4 = {oacc[dt][4 * gq], oacc[dt][4 * gq + 1], oacc[dt][4 * gq + 2], oacc[dt][4 * gq + 3]};
      *reinterpret_cast<f32x4*>(smem + (((w * 4 + dt) * 4 + gq) * 64 + lane) * 16) = o4;
    }
  if (hh == 0) {
    ml[2 * (w * 32 + r)] = m;
    ml[2 * (w * 32 + r) + 1] = l;
  }
  __syncthreads();
  float M = kMinM;
#pragma unroll
  for (int ws = 0; ws < 4; ++ws) M = fmaxf(M, ml[2 * (ws * 32 + r)]);
  float L = 0.f;
  f32x4 acc[4];
#pragma unroll
  for (int gq = 0; gq < 4; ++gq) acc[gq] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ws = 0; ws < 4; ++ws) {  // wave w sums columns 32 w .. 32 w + 31 of every row
    const float a = fexp2(ml[2 * (ws * 32 + r)] - M);  // 0 for a wave that saw no key of the row, unless none did
    L = fmaf(a, ml[2 * (ws * 32 + r) + 1], L);
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(smem + (((ws * 4 + w) * 4 + gq) * 64 + lane) * 16);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[gq][e] = fmaf(a, x[e], acc[gq][e]);
    }
  }
  if (!real) return;
  const float inv = L > 0.f ? 1.f / L : 0.f;          // L == 0: the row sees no key of this split (n > 1 only)
  const float lse = L > 0.f ? M + log2f(L) : -INFINITY;
  if (n == 1) {
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const u16x4 o4 = {f2bf(acc[gq][0] * inv), f2bf(acc[gq][1] * inv), f2bf(acc[gq][2] * inv), f2bf(acc[gq][3] * inv)};
      *reinterpret_cast<u16x4*>(o + ocol + 8 * gq) = o4;
    }
    if (t < 32) lse2[li] = lse;
  } else {
    float* op = o_part + (size_t)z * rows * D + ocol;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const f32x4 o4 = {acc[gq][0] * inv, acc[gq][1] * inv, acc[gq][2] * inv, acc[gq][3] * inv};
      *reinterpret_cast<f32x4*>(op + 8 * gq) = o4;
    }
    if (t < 32) lse_part[z * rows + li] = lse;
  }
}

void launch(hipStream_t st, const u16* q, const u16* kc, const u16* vc, const int* kv_len, u16* o, float* lse2, float* o_part,
            float* lse_part, int B, int H, int Hkv, int Sq, int Smax, float c, int n) {
  hipLaunchKernelGGL(attn_decode_kernel, dim3(B * Hkv, n), dim3(256), 0, st, q, kc, vc, kv_len, o, lse2, o_part, lse_part, H, Hkv,
                     Sq, Smax, c);
}

}  // namespace gtk_decode
