// Decode attention over a paged KV cache (gfx950, head dim 128), and the kernel that appends the new tokens' K
// and V rows to the pages.
//
// The cache is a pool of fixed-size pages, k_pool and v_pool bf16 [num_pages, Hkv, page_size, 128] with page_size
// a multiple of 64, and a block table int32 [B, max_pages]: entry [b, p] is the pool page that holds keys
// p * page_size .. (p + 1) * page_size - 1 of sequence b.  Sequences may share pages.
//
//   attn_decode_paged_kernel   grid (B*Hkv, n), 256 threads: the work split of attn_decode_kernel (one workgroup
//                        per KV head's GQA group and split, the four waves dealing out the split's 64-key tiles,
//                        the balanced per-sequence split ranges, the masked-tile rule, the wave merge), and its
//                        arithmetic: the tile body and the merge are the ones of attention_decode_body.h, fed the
//                        same keys in the same order, so o and lse2 equal attn_decode_kernel's on the gathered slab
//                        (Smax = max_pages * page_size, the same n) bit for bit.  What differs is where a tile's K and
//                        V come from:
//   * A 64-key tile never straddles a page.  The wave's tile kt lies in page kt / tpp of its sequence (tpp =
//     page_size / 64 tiles per page) at tile kt % tpp of it; the wave keeps that pair for the tile it stages next
//     and steps it by 4 tiles with precomputed 4 / tpp and 4 % tpp, no division in the walk.
//   * Both buffer descriptors are built per tile from wave-uniform scalars: base = pool + ((size_t)page * Hkv + hk)
//     * page_size * 128 in 64-bit arithmetic (the pool may exceed 4 GiB), num_records = the rows of this page
//     below kv_len[b] (0 .. page_size) times 256 bytes, and the tile's offset inside the page (< 256 KiB) in the
//     VGPR offset, which the hardware range-checks.  K rows at or past kv_len[b] read as zero and V rows there are
//     zeroed by the masked tile body, as in the contiguous kernel.  The descriptors live in SGPRs: the page id is
//     read out of a VGPR with v_readlane into an SGPR, so no waterfall loop is needed.
//   * The page ids stay off the critical path.  The K/V loads of the wave's tile j + 1 are issued inside tile j,
//     and a table read there would put a dependent memory latency in front of them once per tile.  Instead each
//     wave holds the ids of 64 of its tiles in one VGPR, lane L the id of its tile 64 k + L, fetched by ONE
//     vector load per 64 tiles (each lane divides its own tile index by tpp), and takes the id of the tile it is
//     about to stage with a lane read.  The next 64 ids are loaded right after the loads of tile 64 k + 63 have
//     gone out, inside tile 64 k + 62; that tile's closing s_waitcnt covers the load, and the first of the new ids
//     is used a whole tile later.  Only the first vector of a wave is loaded and used back to back, before there
//     is anything to overlap it with.
//   * Safety, established by reading this code (no test hands the GPU an out-of-range id or length): kv_len[b] is
//     clamped into [Sq, max_pages * page_size]; a table index is clamped into [0, ceil(len / page_size) - 1], so
//     only entries the sequence needs are read and every read is inside row b of the table; every page id is
//     clamped into [0, num_pages) before it forms an address; num_records <= page_size rows bounds every access
//     under the descriptor to this head's part of that page.  No content of block_table or kv_len moves an access
//     outside the pools.
//
//   kv_append_paged_kernel   k_new, v_new [B, Hkv, Sq, 128]: row i of sequence b goes to position pos = kv_len[b]
//                        - Sq + i (kv_len counts the new tokens), page block_table[b, pos / page_size], row pos %
//                        page_size.  One 256-byte row per 16 lanes, a 16-byte load and store per lane for K and
//                        for V, plain C++ stores.  A sequence whose kv_len[b] is outside [Sq, max_pages *
//                        page_size] is skipped whole and a row whose page id is outside [0, num_pages) is skipped:
//                        nothing is clamped onto another page, a wrong table overwrites nobody's keys.
//
// Built with attention_decode.hip's flags (packed fp32 VALU off, the MFMA VGPR form).
#include "attention_decode_body.h"

namespace gtk_decode {

__global__ __launch_bounds__(256) void attn_decode_paged_kernel(const u16* __restrict__ q, const u16* __restrict__ kp,
                                                                const u16* __restrict__ vp, const int* __restrict__ block_table,
                                                                const int* __restrict__ kv_len, u16* __restrict__ o,
                                                                float* __restrict__ lse2, float* __restrict__ o_part,
                                                                float* __restrict__ lse_part, int H, int Hkv, int Sq, int page_size,
                                                                int max_pages, int num_pages, float c) {
  __shared__ __attribute__((aligned(16))) char smem[4 * kWaveLds];
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
  const size_t head = (size_t)page_size * D;             // one KV head's part of a page, in elements
  const uint32_t koff = k_lane_offset(r, hh);
  uint32_t voff[4];
  v_lane_offsets(lane, voff);
  char* vbuf = smem + w * kWaveLds;

  // lane L: the table entry of the wave's tile j0 + L (tile t0 + w + 4 (j0 + L) of the sequence)
  auto load_ids = [&](int j0) {
    const int p = (t0 + w + 4 * (j0 + lane)) / tpp;
    return tab[p < np ? p : np - 1];
  };
  int ids = load_ids(0);

  int kt = t0 + w, j = 0;
  int pg = kt / tpp, tin = kt - pg * tpp;  // of the tile staged next: its page of the sequence, its tile of that page
  const int q4 = 4 / tpp, r4 = 4 - q4 * tpp;

  bf16x8 kf0[8], kf1[8];
  // the K and V loads of the wave's tile jn, through descriptors over this head's part of its pool page
  auto stage = [&](int jn, char* img) {
    const int id = clampi(__builtin_amdgcn_readlane(ids, jn & 63), 0, num_pages - 1);
    const size_t base = ((size_t)id * Hkv + hk) * head;
    const uint32_t bytes = (uint32_t)clampi(len - pg * page_size, 0, page_size) * (D * 2);
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc((void*)(kp + base), 0, bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc((void*)(vp + base), 0, bytes, 0x00020000);
    const uint32_t o0 = (uint32_t)tin * (BK * D * 2);
    load_k_tile(krs, koff + o0, kf0, kf1);
    load_v_tile(vrs, img, voff, o0);
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
    decode_tile(kf0, kf1, qf, vbuf + (j & 1) * kVTile, kt * BK, masked, qpos, len, c, lane, hh, m, l, oacc, [&] {
      if (kt + 4 < t1) {
        stage(j + 1, vbuf + ((j + 1) & 1) * kVTile);
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

__global__ __launch_bounds__(256) void kv_append_paged_kernel(const u16* __restrict__ k_new, const u16* __restrict__ v_new,
                                                              u16* __restrict__ kp, u16* __restrict__ vp,
                                                              const int* __restrict__ block_table, const int* __restrict__ kv_len,
                                                              int B, int Hkv, int Sq, int page_size, int max_pages, int num_pages) {
  const size_t row = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);  // of k_new [B, Hkv, Sq]
  if (row >= (size_t)B * Hkv * Sq) return;
  const int i = (int)(row % Sq), hk = (int)(row / Sq % Hkv), b = (int)(row / Sq / Hkv);
  const int len = kv_len[b];
  if (len < Sq || len > max_pages * page_size) return;
  const int pos = len - Sq + i;  // in [0, max_pages * page_size)
  const int id = block_table[(size_t)b * max_pages + pos / page_size];
  if (id < 0 || id >= num_pages) return;
  const size_t src = row * D + 8 * (threadIdx.x & 15);
  const size_t dst = (((size_t)id * Hkv + hk) * page_size + pos % page_size) * D + 8 * (threadIdx.x & 15);
  const uint4 kx = *reinterpret_cast<const uint4*>(k_new + src), vx = *reinterpret_cast<const uint4*>(v_new + src);
  *reinterpret_cast<uint4*>(kp + dst) = kx;
  *reinterpret_cast<uint4*>(vp + dst) = vx;
}

void launch_paged(hipStream_t st, const u16* q, const u16* kp, const u16* vp, const int* block_table, const int* kv_len, u16* o,
                  float* lse2, float* o_part, float* lse_part, int B, int H, int Hkv, int Sq, int page_size, int max_pages,
                  int num_pages, float c, int n) {
  hipLaunchKernelGGL(attn_decode_paged_kernel, dim3(B * Hkv, n), dim3(256), 0, st, q, kp, vp, block_table, kv_len, o, lse2, o_part,
                     lse_part, H, Hkv, Sq, page_size, max_pages, num_pages, c);
}

void launch_append(hipStream_t st, const u16* k_new, const u16* v_new, u16* kp, u16* vp, const int* block_table, const int* kv_len,
                   int B, int Hkv, int Sq, int page_size, int max_pages, int num_pages) {
  const size_t rows = (size_t)B * Hkv * Sq;
  hipLaunchKernelGGL(kv_append_paged_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, k_new, v_new, kp, vp, block_table,
                     kv_len, B, Hkv, Sq, page_size, max_pages, num_pages);
}

}  // namespace gtk_decode
