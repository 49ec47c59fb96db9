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
#include "attention_decode_body.h"  // the tile body, the wave merge and the loads, shared with attention_decode_paged.hip

namespace gtk_decode {

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
  const uint32_t koff = k_lane_offset(r, hh);
  uint32_t voff[4];
  v_lane_offsets(lane, voff);
  char* vbuf = smem + w * kWaveLds;

  bf16x8 kf0[8], kf1[8];
  auto load_k = [&](int kt) { load_k_tile(krs, koff + (uint32_t)kt * (BK * D * 2), kf0, kf1); };
  auto load_v = [&](int kt, char* img) { load_v_tile(vrs, img, voff, (uint32_t)kt * (BK * D * 2)); };

  f32x16 oacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x16{};
  float m = kMinM, l = 0.f;  // m in units of log2 (score * c)

  // the wave's j-th tile; the next one's loads go out right after QK^T
  auto tile = [&](int kt, int j, bool masked) {
    decode_tile(kf0, kf1, qf, vbuf + (j & 1) * kVTile, kt * BK, masked, qpos, len, c, lane, hh, m, l, oacc, [&] {
      if (kt + 4 < t1) {
        load_k(kt + 4);
        load_v(kt + 4, vbuf + ((j + 1) & 1) * kVTile);
      }
    });
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

  decode_merge_store(smem, oacc, m, l, t, w, real, n, z, rows, li, ocol, o, lse2, o_part, lse_part);
}

void launch(hipStream_t st, const u16* q, const u16* kc, const u16* vc, const int* kv_len, u16* o, float* lse2, float* o_part,
            float* lse_part, int B, int H, int Hkv, int Sq, int Smax, float c, int n) {
  hipLaunchKernelGGL(attn_decode_kernel, dim3(B * Hkv, n), dim3(256), 0, st, q, kc, vc, kv_len, o, lse2, o_part, lse_part, H, Hkv,
                     Sq, Smax, c);
}

}  // namespace gtk_decode
