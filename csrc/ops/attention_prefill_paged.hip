// Prefill attention over a paged KV cache (gfx950, head dim 128, forward only): ragged query chunks straight over
// the block table, and the kernel that appends a chunk's K and V rows to the pages in one launch.
//
// The cache is the one of attention_decode_paged.hip: k_pool and v_pool bf16 [num_pages, Hkv, page_size, 128] with
// page_size a multiple of 64, a block table int32 [B, max_pages], kv_len int32 [B] counting the chunk's tokens.
// q is [B, H, Sq, 128], the batch padded to Sq rows, and q_len int32 [B] says how many of them are real.  With
// ql = clamp(q_len[b], 0, Sq) and len = clamp(kv_len[b], ql, max_pages * page_size), both read here on the device,
// query row i < ql sits at position qpos(i) = len - ql + i and sees the keys j <= qpos(i).  Rows i >= ql are not
// read and write o = 0, lse2 = -inf.
//
//   attn_prefill_paged_kernel   grid (B*H, ceil(Sq / 128)), 256 threads: attn_fwd2_kernel's work split (one workgroup
//                        = 4 waves = 128 query rows of one (batch, q head), 32 rows a wave, a query per lane; the
//                        last query block first, heads XCD-grouped by xcd_head so a GQA group shares an L2), its
//                        staging (K and V tiles of 64 keys double-buffered in 64 KiB of LDS by LDS-DMA, two workgroups
//                        a CU, each wave staging 16 rows, one barrier a tile) and its tile body (swapped QK^T, slack-8
//                        online softmax with the scale in the exponent, bf16 pack of P, PV through tr_frag) in its
//                        order: at Sq = q_len, Sq and len - Sq multiples of 128, o and lse2 equal attn_fwd_qoff's
//                        on the gathered slab bit for bit.  What differs:
//   * A block that lies wholly at or past ql writes its zeros and -inf and returns before any K/V traffic.
//   * Where a tile comes from.  A 64-key tile never straddles a page; the workgroup steps a (page of the sequence,
//     tile of the page) pair by one tile per DMA.  The descriptor pair is rebuilt per tile from wave-uniform scalars:
//     base = pool + ((size_t)page id * Hkv + hk) * page_size * 128 in 64-bit arithmetic (the pool may exceed
//     4 GiB), num_records = the rows of that page below len times 256 bytes, the tile's offset inside the page
//     (< 256 KiB) in the VGPR offset beside the lane's swizzled one.  Page ids are held 64 tiles to a VGPR, lane L
//     the id of tile 64 k + L, fetched by one vector load per 64 tiles and taken with a lane read into SGPRs.  The
//     next vector is loaded right after the DMA of tile 64 k + 63 went out (inside tile 64 k + 62); that tile's
//     closing s_waitcnt covers it and its first id is used a tile later.  Only the first vector is loaded and
//     used back to back.
//   * The diagonal is not aligned to tiles.  With wfirst / wlast the positions of a wave's first and last real row,
//     a wave-uniform choice per tile: skip if key0 > wlast (the wave still issues its share of the next DMA and
//     joins the barrier), masked if key0 + 63 > wfirst, plain otherwise.  A block walks ceil((qpos of its last real
//     row + 1) / 64) tiles.  The tiles that end at or before the block's first row are plain for every wave and run
//     in a branch-free main loop; at most three tiles remain for the peeled tail.  A wave with no real row (in a
//     partial last block) walks as a copy of the block's last real row with q = 0; a padded lane of a partial wave
//     likewise takes q = 0 and the wave's last real position.  Each lane is one query, so nothing of a padded lane
//     reaches another; its outputs are replaced by 0 and -inf at the store.
//   * The running max starts from kMinM, not -inf: a row may see no key of a tile its wave visits (the tile begins
//     past the row but not past the wave's last row).  Tile 0 holds key 0, which every row sees, so every real row's
//     max is finite from the first tile on, and the first rescale is alpha = 0 on l = 0, O = 0 as from -inf.
//   * Rows past len.  A tile that holds a row at or past len ends past every query's position (qpos < len), so it
//     is a masked tile for every wave that visits it and is never in the main loop; it is the sequence's last tile
//     and the last one of the walk of a block that reaches it, so no DMA is in flight while it is worked on.  K rows
//     there: their scores are replaced by -inf by the causal mask in the accumulator (key > qpos), whatever the LDS
//     image holds.  V rows there: set to zero by the workgroup, in the LDS image, after the tile's DMA has landed
//     and one more barrier before any wave reads it, so 0 * NaN cannot reach O.  (zero_past's masks on the 16 V
//     fragments cost 16 live VGPRs in a kernel that sits at the 256 of two workgroups a CU: that build spilled.)
//     The num_records bound carries neither claim; it only keeps the DMA from fetching rows no query can see.
//   * Safety, established by reading this code (no test hands the GPU an out-of-range id or length): q_len[b] is
//     clamped into [0, Sq], so q, o and lse2 are addressed by rows below Sq only; kv_len[b] is clamped into [ql,
//     max_pages * page_size] (the host refuses Sq > max_pages * page_size); a table index is clamped into [0,
//     ceil(len / page_size) - 1], inside row b of the table; every page id is clamped into [0, num_pages) before it
//     forms an address; a staged tile kt < ceil(len / 64) lies inside page kt / tpp < ceil(len / page_size) of the
//     sequence, so voffset + 16 <= page_size * 256, this head's part of that pool page, with or without the
//     hardware's range check.  No content of block_table, kv_len or q_len moves an access outside the pools, the
//     table row or q.
//
//   kv_append_paged_chunk_kernel   k_new, v_new [B, Hkv, Sq, 128], any Sq: row i < ql of sequence b goes to position
//                        kv_len[b] - ql + i; rows i >= ql are not read.  A grid over blocks of 16 rows, so a 4096-row
//                        chunk is one launch; one 256-byte row per 16 lanes, a 16-byte load and a plain vector store
//                        per lane for K and for V.  The skips are kv_append_paged_kernel's: a sequence whose
//                        kv_len[b] is outside [ql, max_pages * page_size] and a row whose page id is outside [0,
//                        num_pages) are left out, nothing is clamped onto another page.
//
// Not here: split-KV for a short chunk against a very long prefix, a backward, head dim 64.  The fp8 pools are served
// by attention_prefill_paged_fp8.hip.
// Built with attention_decode.hip's flags (packed fp32 VALU off, the MFMA VGPR form).
#include "attention_decode_body.h"

namespace gtk_decode {

// The lane's index from v_mbcnt, not from threadIdx: code that needs it once per 64 tiles or only in the epilogue
// (the page id loads, the store addresses) then holds no register through the loops for it
__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

__global__ __launch_bounds__(256, 2) void attn_prefill_paged_kernel(const u16* __restrict__ q, const u16* __restrict__ kp,
                                                                    const u16* __restrict__ vp, const int* __restrict__ block_table,
                                                                    const int* __restrict__ kv_len, const int* __restrict__ q_len,
                                                                    u16* __restrict__ o, float* __restrict__ lse2, int H, int Hkv,
                                                                    int Sq, int page_size, int max_pages, int num_pages, float c) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * BK * D * 2];  // [buf][K image | V image]
  const int t = threadIdx.x, lane = t & 63, r = lane & 31, hh = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int qb = gridDim.y - 1 - blockIdx.y;  // heaviest first
  const int bh = xcd_head(blockIdx.x, gridDim.x), b = bh / H, hq = bh % H, hk = hq / (H / Hkv);
  const int ql = clampi(q_len[b], 0, Sq);
  const int smax = max_pages * page_size;  // >= Sq >= ql (host)
  int len = kv_len[b];
  len = len < ql ? ql : len;
  len = len > smax ? smax : len;
  const size_t lrow = (size_t)(b * H + hq) * Sq;  // the head's first row of q and of lse2 [B, H, Sq]

  if (qb * BQ >= ql) {  // workgroup-uniform: no real row, 128 rows (those below Sq) of zeros and -inf
    for (int j = t; j < BQ * 16; j += 256) {
      const int row = qb * BQ + (j >> 4);
      if (row < Sq) *reinterpret_cast<uint4*>(o + (((size_t)b * Sq + row) * H + hq) * D + 8 * (j & 15)) = uint4{0u, 0u, 0u, 0u};
    }
    if (t < BQ && qb * BQ + t < Sq) lse2[lrow + qb * BQ + t] = -INFINITY;
    return;
  }

  const int off = len - ql;                                    // qpos(i) = off + i
  const int rl = (ql < qb * BQ + BQ ? ql : qb * BQ + BQ) - 1;  // the block's last real row
  const int q0 = qb * BQ + w * 32;
  const int wl = q0 + 31 < rl ? q0 + 31 : rl;                  // the wave's last real row (no real row: the block's)
  const int wfirst = off + (q0 < rl ? q0 : rl), wlast = off + wl;
  const int myq = q0 + r;
  const bool real = myq < ql;
  const int qpos = off + (real ? myq : wl);  // the lane's query sees the keys j <= qpos

  bf16x8 qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) qf[s] = bf16x8{};
  if (real) {
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(q + (lrow + myq) * D + 16 * s + 8 * hh);
  }

  f32x16 oacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x16{};
  float m = kMinM, l = 0.f;  // m in units of log2 (score * c)

  const int ntiles = (off + rl) / BK + 1;            // up to the tile of the block's last real position
  const int nplain = (off + qb * BQ + 1) / BK;       // tiles that end at or before the block's first position
  const int tpp = page_size / BK;                    // tiles per page
  const int np = (len + page_size - 1) / page_size;  // the sequence's pages: the table entries that may be read (>= 1)
  const int* __restrict__ tab = block_table + (size_t)b * max_pages;
  const size_t head = (size_t)page_size * D;         // one KV head's part of a page, in elements
  // KVStage's source swizzle: the wave's DMA i stages rows R = 16 w + 4 i + (lane >> 4), the lane fetching chunk (lane & 15)
  // ^ (((R & 3) << 2) | ((R >> 2) & 3)) = (lane & 15) ^ ((lane >> 4) << 2) ^ i.  One register carries the lane's part
  // through the loops; the xor with 16 i and the wave-uniform rest are formed per tile
  const uint32_t vbase = (uint32_t)((lane >> 4) * (D * 2) + 16 * ((lane & 15) ^ ((lane >> 4) << 2)));

  // lane L: the table entry of tile k0 + L
  auto load_ids = [&](int k0) {
    const int p = (k0 + lane_id()) / tpp;
    return tab[p < np ? p : np - 1];
  };
  int ids = load_ids(0);
  int pg = 0, tin = 0;  // of the tile staged next: its page of the sequence, its tile of that page

  // the wave's 16 rows of tile kt's K and V into img, through descriptors over this head's part of the tile's pool
  // page; tiles are staged in order, once each, by every wave
  auto gload = [&](int kt, char* img) {
    const int id = clampi(__builtin_amdgcn_readlane(ids, kt & 63), 0, num_pages - 1);
    const size_t base = ((size_t)id * Hkv + hk) * head;
    const uint32_t bytes = (uint32_t)clampi(len - pg * page_size, 0, page_size) * (D * 2);
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc((void*)(kp + base), 0, bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc((void*)(vp + base), 0, bytes, 0x00020000);
    const uint32_t o0 = (uint32_t)tin * (BK * D * 2) + 16 * w * (D * 2);  // the tile's offset in the page + the wave's rows
    uint32_t vb = vbase;
    asm volatile("" : "+v"(vb));  // keeps the four offsets below from being carried through the loops as well
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t vo = (vb ^ (16 * i)) + (o0 + 4 * i * (D * 2));
      __builtin_amdgcn_raw_ptr_buffer_load_lds(krs, (LDS_AS void*)(img + (16 * w + 4 * i) * 256), 16, vo, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(vrs, (LDS_AS void*)(img + BK * D * 2 + (16 * w + 4 * i) * 256), 16, vo, 0, 0, 0);
    }
    if (++tin == tpp) tin = 0, ++pg;
    if ((kt & 63) == 63) ids = load_ids(kt + 1);  // the next 64 ids, a whole tile before the first of them is used
  };

  // one KV tile, attn_fwd2_kernel's: QK^T, DMA of the next tile, online softmax, PV.  `masked` adds the causal mask
  auto tile = [&](int kt, bool masked) {
    char* kimg = smem + (kt & 1) * (2 * BK * D * 2);
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
    if (kt + 1 < ntiles) gload(kt + 1, smem + ((kt + 1) & 1) * (2 * BK * D * 2));  // lands under softmax + PV
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
    const float mrow = xhalf_max(mx) * c;  // -inf where the row sees no key of the tile: m stays
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
    if (resc) {  // alpha == 1 everywhere otherwise; from kMinM it is 0 on l = 0, O = 0
      const float alpha = fexp2(m - mnew);
      l *= alpha;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[dt][i] *= alpha;
    }
    l += rs;
    m = mnew;
    const bf16x8 p[4] = {pack8(s0, 0), pack8(s0, 8), pack8(s1, 0), pack8(s1, 8)};
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int f = 0; f < 4; ++f)
        oacc[dt] = mfma(tr_frag(vimg, lane, 16 * f + 4 * hh, 16 * f + 8 + 4 * hh, 32 * dt), p[f], oacc[dt]);
    __builtin_amdgcn_s_setprio(0);
  };

  gload(0, smem);
  dma_sync();
  int kt = 0;
  // tiles that lie entirely below every query of the block: no mask, no visibility test
  for (; kt < nplain; ++kt) {
    tile(kt, false);
    dma_sync();
  }
  // the block's diagonal, at most three tiles: per wave skipped, masked or plain
  for (; kt < ntiles; ++kt) {
    const int key0 = kt * BK;
    if (key0 + BK > len) {  // workgroup-uniform, the sequence's last tile only: its V rows at or past len become 0
      char* vimg = smem + (kt & 1) * (2 * BK * D * 2) + BK * D * 2;
      for (int R = len - key0 + 4 * w + (lane >> 4); R < BK; R += 16)
        *reinterpret_cast<uint4*>(vimg + R * 256 + 16 * (lane & 15)) = uint4{0u, 0u, 0u, 0u};
      __syncthreads();
    }
    if (key0 <= wlast) {
      tile(kt, key0 + BK - 1 > wfirst);
    } else if (kt + 1 < ntiles) {
      gload(kt + 1, smem + ((kt + 1) & 1) * (2 * BK * D * 2));
    }
    dma_sync();
  }

  // attn_fwd2_kernel's store (T21: one v_permlane32_swap per dword of a pair of column groups gives every lane 16
  // contiguous bytes); a padded row stores zeros and -inf, a row at or past Sq nothing
  const int el = lane_id(), row = q0 + (el & 31), eh = el >> 5;  // == myq, hh
  const bool keep = row < ql;
  const float inv = 1.f / l;
  u16* orow = o + (((size_t)b * Sq + row) * (size_t)(H) + hq) * D;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; g4 += 2) {
      u16x4 va, vb;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        va[e] = keep ? f2bf(oacc[dt][4 * g4 + e] * inv) : (u16)0;
        vb[e] = keep ? f2bf(oacc[dt][4 * g4 + 4 + e] * inv) : (u16)0;
      }
      const auto a = __builtin_bit_cast(uint2, va), bb = __builtin_bit_cast(uint2, vb);
      const auto x0 = __builtin_amdgcn_permlane32_swap(a.x, bb.x, false, false);
      const auto x1 = __builtin_amdgcn_permlane32_swap(a.y, bb.y, false, false);
      const uint4 out = {x0[0], x1[0], x0[1], x1[1]};
      if (row < Sq) *reinterpret_cast<uint4*>(orow + 32 * dt + 8 * g4 + 8 * eh) = out;
    }
  if (eh == 0 && row < Sq) lse2[lrow + row] = keep ? m + log2f(l) : -INFINITY;
}

__global__ __launch_bounds__(256) void kv_append_paged_chunk_kernel(const u16* __restrict__ k_new, const u16* __restrict__ v_new,
                                                                    u16* __restrict__ kp, u16* __restrict__ vp,
                                                                    const int* __restrict__ block_table,
                                                                    const int* __restrict__ kv_len, const int* __restrict__ q_len,
                                                                    int B, int Hkv, int Sq, int page_size, int max_pages,
                                                                    int num_pages) {
  const size_t row = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);  // of k_new [B, Hkv, Sq]
  if (row >= (size_t)B * Hkv * Sq) return;
  const int i = (int)(row % Sq), hk = (int)(row / Sq % Hkv), b = (int)(row / Sq / Hkv);
  const int ql = clampi(q_len[b], 0, Sq);
  if (i >= ql) return;
  const int len = kv_len[b];
  if (len < ql || len > max_pages * page_size) return;
  const int pos = len - ql + i;  // in [0, max_pages * page_size)
  const int id = block_table[(size_t)b * max_pages + pos / page_size];
  if (id < 0 || id >= num_pages) return;
  const size_t src = row * D + 8 * (threadIdx.x & 15);
  const size_t dst = (((size_t)id * Hkv + hk) * page_size + pos % page_size) * D + 8 * (threadIdx.x & 15);
  const uint4 kx = *reinterpret_cast<const uint4*>(k_new + src), vx = *reinterpret_cast<const uint4*>(v_new + src);
  *reinterpret_cast<uint4*>(kp + dst) = kx;
  *reinterpret_cast<uint4*>(vp + dst) = vx;
}

void launch_prefill_paged(hipStream_t st, const u16* q, const u16* kp, const u16* vp, const int* block_table, const int* kv_len,
                          const int* q_len, u16* o, float* lse2, int B, int H, int Hkv, int Sq, int page_size, int max_pages,
                          int num_pages, float c) {
  hipLaunchKernelGGL(attn_prefill_paged_kernel, dim3(B * H, (Sq + BQ - 1) / BQ), dim3(256), 0, st, q, kp, vp, block_table, kv_len,
                     q_len, o, lse2, H, Hkv, Sq, page_size, max_pages, num_pages, c);
}

void launch_append_chunk(hipStream_t st, const u16* k_new, const u16* v_new, u16* kp, u16* vp, const int* block_table,
                         const int* kv_len, const int* q_len, int B, int Hkv, int Sq, int page_size, int max_pages, int num_pages) {
  const size_t rows = (size_t)B * Hkv * Sq;
  hipLaunchKernelGGL(kv_append_paged_chunk_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, k_new, v_new, kp, vp,
                     block_table, kv_len, q_len, B, Hkv, Sq, page_size, max_pages, num_pages);
}

}  // namespace gtk_decode
