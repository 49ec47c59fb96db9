// The body the decode attention kernels share (gfx950, head dim 128): attn_decode_kernel of attention_decode.hip
// over a contiguous ragged cache and attn_paged_kernel of attention_decode_paged.hip over a block-table cache.
// Both give one workgroup the GQA group of one KV head over one split of a sequence's 64-key tiles, four waves
// that deal the tiles out, and differ only in where a tile's K and V are found: the buffer descriptor and the
// byte offset the loads below take.  What a tile computes (decode_tile) and how the four waves' (m, l, O) merge
// and leave the workgroup (decode_merge_store) is here once, so the two kernels agree bit for bit on the same
// keys.  The layout of the work is described at the head of attention_decode.hip.
#pragma once
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

// the lane's byte offset into a 64-key K tile: key r (and r + 32), dims 64 hh ..
__device__ __forceinline__ uint32_t k_lane_offset(int r, int hh) { return (uint32_t)(r * (D * 2) + 128 * hh); }

// KVStage's source swizzle: instruction ii stages rows 4 ii + (lane >> 4), voff[ii & 3] + 1024 (ii & ~3)
__device__ __forceinline__ void v_lane_offsets(int lane, uint32_t (&voff)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int R = 4 * j + (lane >> 4);
    voff[j] = (uint32_t)(R * D * 2 + 16 * ((lane & 15) ^ (((R & 3) << 2) | ((R >> 2) & 3))));
  }
}

// one 64-key K tile from global memory into the A-operand registers; o0 = the lane's offset + the tile's
__device__ __forceinline__ void load_k_tile(__amdgpu_buffer_rsrc_t krs, uint32_t o0, bf16x8 (&kf0)[8], bf16x8 (&kf1)[8]) {
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    kf0[s] = load_b128(krs, o0 + 16 * s);
    kf1[s] = load_b128(krs, o0 + 32 * D * 2 + 16 * s);
  }
}

// one 64-key V tile by LDS-DMA into the swizzled image img; o0 = the tile's byte offset under the descriptor
__device__ __forceinline__ void load_v_tile(__amdgpu_buffer_rsrc_t vrs, char* img, const uint32_t (&voff)[4], uint32_t o0) {
#pragma unroll
  for (int ii = 0; ii < 16; ++ii)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(vrs, (LDS_AS void*)(img + ii * 1024), 16, voff[ii & 3] + 1024 * (ii & ~3) + o0, 0, 0, 0);
}

// One 64-key tile whose first key is key0: QK^T from the registers, next() (the loads of the wave's next tile,
// which land under softmax + PV), online softmax, PV from the V image vimg.  qpos: the last key the lane's
// query sees; len: the sequence's keys.  Ends with every load of next() landed and this tile's LDS reads
// returned: the wave's own buffers need no barrier, and the next DMA may overwrite the image just read.
template <class Next>
__device__ __forceinline__ void decode_tile(const bf16x8 (&kf0)[8], const bf16x8 (&kf1)[8], const bf16x8 (&qf)[8], const char* vimg,
                                            int key0, bool masked, int qpos, int len, float c, int lane, int hh, float& m,
                                            float& l, f32x16 (&oacc)[4], Next&& next) {
  f32x16 s0 = f32x16{}, s1 = f32x16{};
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    s0 = mfma(kf0[s], qf[s], s0);
    s1 = mfma(kf1[s], qf[s], s1);
  }
  next();
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
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

// The four waves' (m, l, O) in wave order through smem (the V buffers, free once every wave is past its last V
// read: 64 KiB + 1 KiB), then the workgroup's rows: at n = 1 o (bf16, at ocol) and lse2 (at li), at n > 1 the
// normalised fp32 partial and lse2 of split z in the layouts gtk_splitkv's weighted merge reads.  A row that
// sees no key of its split writes lse2 = -inf like an empty split.
__device__ __forceinline__ void decode_merge_store(char* smem, const f32x16 (&oacc)[4], float m, float l, int t, int w, bool real,
                                                   int n, int z, size_t rows, size_t li, size_t ocol, u16* __restrict__ o,
                                                   float* __restrict__ lse2, float* __restrict__ o_part,
                                                   float* __restrict__ lse_part) {
  const int lane = t & 63, r = lane & 31, hh = lane >> 5;
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

}  // namespace gtk_decode
