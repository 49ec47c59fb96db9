// Decode attention over a paged KV cache kept in 8 bits (gfx950, head dim 128), and the kernel that quantises the
// new tokens' K and V rows into the pages.
//
// Cache format.  Four pools over the pages of attention_decode_paged.hip (page_size a multiple of 64, the same
// block table int32 [B, max_pages] and kv_len int32 [B]):
//   k_codes, v_codes  uint8 [num_pages, Hkv, page_size, 128]   one OCP e4m3fn code per element
//   k_exp, v_exp      uint8 [num_pages, Hkv, page_size]        one byte per key row and KV head, e + 127
// 129 bytes per row against 256.  A block is one 128-element row, and its rule is the one of the K7 fp8 wire
// (csrc/common/q8_block.h, csrc/probe/peer_q8.h; ops/fused.py: kv_quantize_ref is the same rule in torch, and
// decides): e is the smallest integer with amax * 2^-e <= 448, clamped to [-100, 120] (amax == 0: -100), the amax
// taken over the row's elements that are not NaN; a code is x * 2^-e rounded to nearest even into e4m3fn, subnormal
// codes included; a NaN or an Inf gets a code with (code & 0x7f) == 0x7f.  value = float(code) * 2^e, which is exact
// in bf16: a code has at most 4 significant bits.  V is row-major like K: the append stays one launch of plain
// row stores, and the transposing LDS read below makes a transposed page unnecessary.
//
//   attn_decode_paged_fp8_kernel   grid (B*Hkv, n), 256 threads.  From attn_decode_paged_kernel it keeps the work
//                        split (one workgroup per KV head's GQA group and split, four waves dealing out the split's
//                        64-key tiles, the balanced split ranges), the masked-tile rule, the id-vector scheme (one
//                        vector load of page ids per 64 tiles, v_readlane into SGPR descriptors, no waterfall), the
//                        clamps, and decode_merge_store unchanged.  The MFMAs are the bf16 ones, fed in the same
//                        order, and the scales never touch K or V: a code widens exactly to bf16, 2^e_k[key] is
//                        multiplied onto the fp32 score after QK^T and 2^e_v[key] onto the fp32 probability before
//                        it is packed to bf16 for PV (the row sum l takes the unscaled probabilities).  Both
//                        multiplies are exact, and so is every product inside the MFMAs, so o and lse2 equal
//                        attn_decode_paged_kernel's on the dequantised pools at the same n bit for bit (fp32
//                        underflow of p * 2^e_v aside, which needs p < 2^-126-e_v).  The data path is its own:
//   * K.  A lane's half row is 64 bytes: 4 buffer_load_dwordx4 per key half, 8 per tile against 16, through a
//     per-tile descriptor with num_records = the rows of this page below kv_len[b] times 128, so rows at or past
//     kv_len[b] read as code 0 = +0.  The tile stays in registers as codes, 32 VGPRs against 64; each 8-code group
//     is widened just before its MFMA with v_cvt_pk_f32_fp8 and a pack of the two high halves (fp32 to bf16 by
//     truncation is exact for a widened code).  No scaling conversion is used.
//   * V.  A tile is 8 KiB and comes by LDS-DMA, 8 instructions of 16 bytes per lane against 16, into a per-wave
//     double buffer.  The PV A operand of lane (r, hh) is 8 keys of head dim col0 + r: one ds_read_b64_tr_b8.  In
//     each 16-lane group lane i' hands the read the address of 8 bytes and lane i receives byte i & 7 of lane
//     2 j + (i >> 3) as its byte j (a probe run on an MI355X confirmed this mapping): an 8 x 16 byte transpose whose
//     row j is addressed freely by lanes 2 j and 2 j + 1.  So row j is pointed at key 16 f + 4 hh + (j & 3) +
//     8 (j >> 2), the keys the lane's probabilities hold, and the fragment is tr_frag's of the bf16 kernel element
//     for element.  The image is row-major, 128 bytes a key, with the 32-byte unit u of key R at unit u ^ sw(R),
//     sw(R) = (R >> 1 & 1) | (R >> 3 & 1) << 1, put on the DMA's source offset (the destination is lane-linear): the
//     8 keys x 32 bytes a half wave reads then fall on 8 distinct bank groups of 8, free of conflicts.
//   * Scales.  A tile's 64 k_exp and 64 v_exp bytes come by two 4-byte LDS-DMAs next to its V image, through
//     descriptors bounded in rows (rounded up to 4), issued with the tile's other loads inside the previous tile.
//     A lane takes the 8 + 8 dwords that hold its 32 keys' bytes (dword hh + 2 m: keys 8 m + 4 hh ..) with LDS
//     reads under QK^T; 2^e is byte << 23.  In a masked tile the v_exp bytes of keys at or past kv_len[b] are
//     cleared in registers, so their probability 0 is multiplied by 0 whatever the pool holds there (a byte 0xff
//     would be Inf); a K score there is replaced by -inf by the mask, whatever its scale made of it.
//   * LDS 68 KiB (4 waves x 2 stages of 8 KiB + 512 B, the merge area of 65 KiB inside it) against 128 KiB: two
//     workgroups fit a CU.
//   * Safety, established by reading this code (no test hands the GPU an out-of-range id or length): kv_len[b] is
//     clamped into [Sq, max_pages * page_size]; a table index is clamped into [0, ceil(len / page_size) - 1], so
//     only entries the sequence needs are read and every read is inside row b of the table; every page id is
//     clamped into [0, num_pages) before it forms an address; num_records <= page_size rows bounds every access
//     under a descriptor to this head's part of that page, in each of the four pools.  An exponent byte is only
//     ever shifted into a float.  No content of block_table, kv_len or the exponent bytes moves an access outside
//     the four pools.
//
//   kv_append_paged_fp8_kernel   k_new, v_new bf16 [B, Hkv, Sq, 128]: the positions and the skip rules of
//                        kv_append_paged_kernel (a sequence whose kv_len[b] is outside [Sq, max_pages * page_size]
//                        is skipped whole, a row whose page id is outside [0, num_pages) is skipped, nothing is
//                        clamped onto another page).  16 lanes own a row: the amax is four lane exchanges, e is
//                        q8_block_exp's, the codes come from v_cvt_pk_fp8_f32 on exactly scaled values; each lane
//                        stores its 8 code bytes and the row's first lane the exponent byte, plain C++ stores.
//                        Quantising a new row reads nothing of the cache.
//
// Built with attention_decode_paged.hip's flags (packed fp32 VALU off, the MFMA VGPR form).
#include "attention_fp8.h"  // widen8, exp_scale, quantize_row8 and their typedefs

namespace gtk_decode {

constexpr int kVTile8 = BK * D;                  // one 64-key V image of codes
constexpr int kExpTile = 512;                    // a tile's exponent bytes as the two DMAs leave them: K at 0, V at 256
constexpr int kStage8 = kVTile8 + kExpTile;
constexpr int kWaveLds8 = 2 * kStage8;           // a wave's double buffer
constexpr int kSmem8 = 4 * kWaveLds8;
static_assert(kSmem8 >= kMergeO + 4 * 32 * 2 * 4, "the merge area must fit the V buffers");

// the lane's byte offset into a 64-key tile of K codes: key r (and r + 32), dims 64 hh ..
__device__ __forceinline__ uint32_t k8_lane_offset(int r, int hh) { return (uint32_t)(r * D + 64 * hh); }

// the DMA's source offsets: instruction ii stages keys 8 ii + (lane >> 3), voff[ii & 1] + 1024 ii, with the
// 16-byte chunk p of key R taken from chunk p ^ 2 sw(R)
__device__ __forceinline__ void v8_lane_offsets(int lane, uint32_t (&voff)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int sw = ((lane >> 4) & 1) | (j << 1);
    voff[j] = (uint32_t)((lane >> 3) * D + 16 * ((lane & 7) ^ (2 * sw)));
  }
}

// the lane's addresses for the transposed reads: rd[dt] + 2048 f is the 8 bytes it hands ds_read_b64_tr_b8 for
// the PV operand of keys 16 f .. and head dims 32 dt ..
__device__ __forceinline__ void v8_read_offsets(int lane, uint32_t (&rd)[4]) {
  const int g = lane >> 4, i = lane & 15, hh = g >> 1;
  const int row = 4 * hh + ((i >> 1) & 3) + 8 * (i >> 3), sw = (i >> 2) & 3;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) rd[dt] = (uint32_t)(row * D + 32 * (dt ^ sw) + 16 * (g & 1) + 8 * (i & 1));
}

__device__ __forceinline__ void load_k_codes(__amdgpu_buffer_rsrc_t krs, uint32_t o0, u32x4 (&kc0)[4], u32x4 (&kc1)[4]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    kc0[s] = __builtin_amdgcn_raw_buffer_load_b128(krs, (int)(o0 + 16 * s), 0, 0);
    kc1[s] = __builtin_amdgcn_raw_buffer_load_b128(krs, (int)(o0 + 32 * D + 16 * s), 0, 0);
  }
}

// One 64-key tile whose first key is key0, as decode_tile computes it, from the K codes in registers and the stage
// st (the V image, then the k_exp and the v_exp dwords).  Ends like decode_tile: every load of next() landed and
// this tile's LDS reads returned.
template <class Next>
__device__ __forceinline__ void decode_tile_fp8(const u32x4 (&kc0)[4], const u32x4 (&kc1)[4], const bf16x8 (&qf)[8], const char* st,
                                                const uint32_t (&rd)[4], int key0, bool masked, int qpos, int len, float c,
                                                int hh, float& m, float& l, f32x16 (&oacc)[4], Next&& next) {
  uint32_t ke[8], ve[8];  // dword mm: the bytes of keys key0 + 8 mm + 4 hh + {0..3}
  const uint32_t* ex = reinterpret_cast<const uint32_t*>(st + kVTile8) + hh;
#pragma unroll
  for (int mm = 0; mm < 8; ++mm) ke[mm] = ex[2 * mm], ve[mm] = ex[64 + 2 * mm];
  f32x16 s0 = f32x16{}, s1 = f32x16{};
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    s0 = mfma(widen8(kc0[s >> 1][2 * (s & 1)], kc0[s >> 1][2 * (s & 1) + 1]), qf[s], s0);
    s1 = mfma(widen8(kc1[s >> 1][2 * (s & 1)], kc1[s >> 1][2 * (s & 1) + 1]), qf[s], s1);
  }
  next();
#pragma unroll
  for (int e = 0; e < 16; ++e) {  // the keys' scales, exact: the scores of the dequantised K
    s0[e] *= exp_scale(ke[e >> 2], e & 3);
    s1[e] *= exp_scale(ke[4 + (e >> 2)], e & 3);
  }
  if (masked) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int k0e = key0 + crow(e, hh);
      if (k0e > qpos) s0[e] = -INFINITY;
      if (k0e + 32 > qpos) s1[e] = -INFINITY;
    }
#pragma unroll
    for (int mm = 0; mm < 8; ++mm) {  // no scale for a key at or past len, whatever byte the pool holds there
      const int k0 = key0 + 8 * mm + 4 * hh;
      ve[mm] &= (k0 < len ? 0xffu : 0u) | (k0 + 1 < len ? 0xff00u : 0u) | (k0 + 2 < len ? 0xff0000u : 0u) |
                (k0 + 3 < len ? 0xff000000u : 0u);
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
#pragma unroll
  for (int e = 0; e < 16; ++e) {  // the values' scales ride on the probabilities, after the row sum took them
    s0[e] *= exp_scale(ve[e >> 2], e & 3);
    s1[e] *= exp_scale(ve[4 + (e >> 2)], e & 3);
  }
  const bf16x8 p[4] = {pack8(s0, 0), pack8(s0, 8), pack8(s1, 0), pack8(s1, 8)};
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const i32x2 cv = __builtin_amdgcn_ds_read_tr8_b64_v2i32((LDS_AS i32x2*)(st + rd[dt] + 2048 * f));
      bf16x8 vf = widen8((uint32_t)cv[0], (uint32_t)cv[1]);
      if (masked) vf = zero_past(vf, key0 + 16 * f + 4 * hh, len);
      oacc[dt] = mfma(vf, p[f], oacc[dt]);
    }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

__global__ __launch_bounds__(256) void attn_decode_paged_fp8_kernel(const u16* __restrict__ q, const u8* __restrict__ kc,
                                                                    const u8* __restrict__ vc, const u8* __restrict__ kx,
                                                                    const u8* __restrict__ vx, const int* __restrict__ block_table,
                                                                    const int* __restrict__ kv_len, u16* __restrict__ o,
                                                                    float* __restrict__ lse2, float* __restrict__ o_part,
                                                                    float* __restrict__ lse_part, int H, int Hkv, int Sq,
                                                                    int page_size, int max_pages, int num_pages, float c) {
  __shared__ __attribute__((aligned(16))) char smem[kSmem8];
  const int t = threadIdx.x, lane = t & 63, r = lane & 31, hh = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int n = gridDim.y, z = blockIdx.y;
  const int bk = blockIdx.x, b = bk / Hkv, hk = bk % Hkv, G = H / Hkv;
  const int len = clampi(kv_len[b], Sq, max_pages * page_size);
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

  const int tpp = page_size / BK;                        // tiles per page
  const int np = (len + page_size - 1) / page_size;      // the sequence's pages: the table entries that may be read
  const int* __restrict__ tab = block_table + (size_t)b * max_pages;
  const uint32_t koff = k8_lane_offset(r, hh), xoff = (uint32_t)(4 * (lane & 15));
  uint32_t voff[2], rd[4];
  v8_lane_offsets(lane, voff);
  v8_read_offsets(lane, rd);
  char* vbuf = smem + w * kWaveLds8;

  // lane L: the table entry of the wave's tile j0 + L (tile t0 + w + 4 (j0 + L) of the sequence)
  auto load_ids = [&](int j0) {
    const int p = (t0 + w + 4 * (j0 + lane)) / tpp;
    return tab[p < np ? p : np - 1];
  };
  int ids = load_ids(0);

  int kt = t0 + w, j = 0;
  int pg = kt / tpp, tin = kt - pg * tpp;  // of the tile staged next: its page of the sequence, its tile of that page
  const int q4 = 4 / tpp, r4 = 4 - q4 * tpp;

  u32x4 kc0[4], kc1[4];
  // the loads of the wave's tile jn into the registers and the stage st, through descriptors over this head's part
  // of its page in each pool
  auto stage = [&](int jn, char* st) {
    const int id = clampi(__builtin_amdgcn_readlane(ids, jn & 63), 0, num_pages - 1);
    const size_t base = ((size_t)id * Hkv + hk) * page_size;  // the head's first row of the page, in rows
    const uint32_t nrow = (uint32_t)clampi(len - pg * page_size, 0, page_size);
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc((void*)(kc + base * D), 0, nrow * D, 0x00020000);
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc((void*)(vc + base * D), 0, nrow * D, 0x00020000);
    const __amdgpu_buffer_rsrc_t kxs = __builtin_amdgcn_make_buffer_rsrc((void*)(kx + base), 0, (nrow + 3) & ~3u, 0x00020000);
    const __amdgpu_buffer_rsrc_t vxs = __builtin_amdgcn_make_buffer_rsrc((void*)(vx + base), 0, (nrow + 3) & ~3u, 0x00020000);
    const uint32_t o0 = (uint32_t)tin * (BK * D);
    load_k_codes(krs, koff + o0, kc0, kc1);
#pragma unroll
    for (int ii = 0; ii < 8; ++ii)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(vrs, (LDS_AS void*)(st + ii * 1024), 16, voff[ii & 1] + 1024 * ii + o0, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(kxs, (LDS_AS void*)(st + kVTile8), 4, xoff + (uint32_t)tin * BK, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(vxs, (LDS_AS void*)(st + kVTile8 + 256), 4, xoff + (uint32_t)tin * BK, 0, 0, 0);
    pg += q4, tin += r4;
    if (tin >= tpp) tin -= tpp, ++pg;
  };

  f32x16 oacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x16{};
  float m = kMinM, l = 0.f;  // m in units of log2 (score * c)

  // the wave's j-th tile; the next one's loads go out right after QK^T, and after those of the last tile a
  // vector of ids covers, the next vector
  auto tile = [&](int kt, int j, bool masked) {
    decode_tile_fp8(kc0, kc1, qf, vbuf + (j & 1) * kStage8, rd, kt * BK, masked, qpos, len, c, hh, m, l, oacc, [&] {
      if (kt + 4 < t1) {
        stage(j + 1, vbuf + ((j + 1) & 1) * kStage8);
        if (((j + 1) & 63) == 63) ids = load_ids(j + 2);
      }
    });
  };

  if (kt < t1) {
    stage(0, vbuf);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  const int tm = (len - Sq + 1) / BK;  // the first tile that holds a key past some query's position
  for (; kt < t1 && kt < tm; kt += 4, ++j) tile(kt, j, false);
  for (; kt < t1; kt += 4, ++j) tile(kt, j, true);

  decode_merge_store(smem, oacc, m, l, t, w, real, n, z, rows, li, ocol, o, lse2, o_part, lse_part);
}

__global__ __launch_bounds__(256) void kv_append_paged_fp8_kernel(const u16* __restrict__ k_new, const u16* __restrict__ v_new,
                                                                  u8* __restrict__ kc, u8* __restrict__ vc, u8* __restrict__ kx,
                                                                  u8* __restrict__ vx, const int* __restrict__ block_table,
                                                                  const int* __restrict__ kv_len, int B, int Hkv, int Sq,
                                                                  int page_size, int max_pages, int num_pages) {
  const size_t row = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);  // of k_new [B, Hkv, Sq]; its 16 lanes leave together
  if (row >= (size_t)B * Hkv * Sq) return;
  const int i = (int)(row % Sq), hk = (int)(row / Sq % Hkv), b = (int)(row / Sq / Hkv);
  const int len = kv_len[b];
  if (len < Sq || len > max_pages * page_size) return;
  const int pos = len - Sq + i;  // in [0, max_pages * page_size)
  const int id = block_table[(size_t)b * max_pages + pos / page_size];
  if (id < 0 || id >= num_pages) return;
  const int sub = threadIdx.x & 15;
  const size_t src = row * D + 8 * sub;
  const size_t drow = ((size_t)id * Hkv + hk) * page_size + pos % page_size;
  const uint4 kn = *reinterpret_cast<const uint4*>(k_new + src), vn = *reinterpret_cast<const uint4*>(v_new + src);
  int ek, ev;
  const u32x2 kq = quantize_row8(kn, ek), vq = quantize_row8(vn, ev);
  *reinterpret_cast<u32x2*>(kc + drow * D + 8 * sub) = kq;
  *reinterpret_cast<u32x2*>(vc + drow * D + 8 * sub) = vq;
  if (sub == 0) {
    kx[drow] = (u8)(ek + gtk_q8::kQ8Bias);
    vx[drow] = (u8)(ev + gtk_q8::kQ8Bias);
  }
}

void launch_paged_fp8(hipStream_t st, const u16* q, const u8* kc, const u8* vc, const u8* kx, const u8* vx, const int* block_table,
                      const int* kv_len, u16* o, float* lse2, float* o_part, float* lse_part, int B, int H, int Hkv, int Sq,
                      int page_size, int max_pages, int num_pages, float c, int n) {
  hipLaunchKernelGGL(attn_decode_paged_fp8_kernel, dim3(B * Hkv, n), dim3(256), 0, st, q, kc, vc, kx, vx, block_table, kv_len, o, lse2,
                     o_part, lse_part, H, Hkv, Sq, page_size, max_pages, num_pages, c);
}

void launch_append_fp8(hipStream_t st, const u16* k_new, const u16* v_new, u8* kc, u8* vc, u8* kx, u8* vx, const int* block_table,
                       const int* kv_len, int B, int Hkv, int Sq, int page_size, int max_pages, int num_pages) {
  const size_t rows = (size_t)B * Hkv * Sq;
  hipLaunchKernelGGL(kv_append_paged_fp8_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, k_new, v_new, kc, vc, kx, vx,
                     block_table, kv_len, B, Hkv, Sq, page_size, max_pages, num_pages);
}

}  // namespace gtk_decode
