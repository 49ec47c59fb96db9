// Prefill attention over the paged KV cache kept in 8 bits (gfx950, head dim 128, forward only): ragged query chunks
// straight over the block table and the four fp8 pools, and the kernel that quantises a chunk's K and V rows into
// the pages in one launch.
//
// The cache is the one of attention_decode_paged_fp8.hip: k_codes, v_codes uint8 [num_pages, Hkv, page_size, 128] (one
// e4m3fn code an element), k_exp, v_exp uint8 [num_pages, Hkv, page_size] (e + 127 per row), value = float(code) * 2^e.
// q, q_len, kv_len, the clamps and the positions are those of attention_prefill_paged.hip: ql = clamp(q_len[b], 0, Sq),
// len = clamp(kv_len[b], ql, max_pages * page_size), row i < ql sits at len - ql + i and sees the keys up to it, rows
// i >= ql are not read and write o = 0, lse2 = -inf.
//
//   attn_prefill_paged_fp8_kernel   grid (B*H, ceil(Sq / 128)), 256 threads.  From attn_prefill_paged_kernel it keeps
//                        the grid and the work split (128 query rows a workgroup, 32 a wave, a query per lane, the
//                        heaviest block first, xcd_head), the (page, tile of the page) walk, the id vector (one vector
//                        load of page ids per 64 tiles, a lane read into scalar descriptors), the clamps, the
//                        skipped / masked / plain choice per wave with a branch-free main loop and at most three
//                        peeled tiles, the start from kMinM, the tile body's arithmetic in its order, and the store.
//                        The tile body reads a bf16 image of the tile that holds, element for element, what the bf16
//                        kernel's DMA puts there from the dequantised pools (rows at or past len aside, which no result
//                        depends on in either kernel), so o and lse2 equal attn_prefill_paged_kernel's on
//                        kv_dequantize_ref of the pools bit for bit: by construction, and tested on an MI355X on every
//                        case of tests/test_gpu_attention_prefill_paged_fp8.py.  The scales never ride on scores or
//                        probabilities.  The data path is its own:
//   * Staging.  A 64-key tile is 8 KiB of K codes and 8 KiB of V codes, half the bf16 kernel's DMA bytes.  Wave w
//     stages rows 16 w .. 16 w + 15 of both by two 16-byte LDS-DMAs each, and those rows' 16 + 16 exponent bytes by
//     two 4-byte LDS-DMAs (every lane group of 4 fetches the same 16 bytes; the wave reads back the first), into a
//     code stage that is double-buffered.  The descriptors are the fp8 decode kernel's: num_records = the rows of this
//     page below len times 128 for the codes, those rows rounded up to 4 for the exponent bytes.  A wave converts
//     only rows it staged itself, so the stages need no barrier: the wave's own s_waitcnt vmcnt(0) is enough before
//     it reads a stage, and its own lgkmcnt(0) before its next DMA overwrites one.
//   * Staging swizzle: none.  The code rows lie lane-linear, 128 bytes a row.  The converter gives 16 consecutive
//     lanes one row, lane i its codes 8 i .. 8 i + 7: the wave's 8-byte reads cover 512 consecutive bytes, and its
//     16-byte writes the four whole 256-byte rows of the image (swz permutes 16-byte chunks inside a row, and aligned
//     blocks of 8 chunks onto aligned blocks), so every group of 8, 16 or 32 consecutive lanes touches consecutive
//     bytes.  Free of bank conflicts by this reading of the layout; not measured with counters.
//   * Conversion, once per workgroup and tile (the decode kernel's per-wave widening would do it four times here, on
//     a VALU that is not idle).  Per 8 codes: one LDS read, the widening to fp32 (v_cvt_pk_f32_fp8), a multiply by
//     2^e = byte << 23 (exact in fp32 for every code and every e the format allows; Inf where kv_dequantize_ref gives
//     Inf), the high halves packed (truncation is exact: at most 4 significant bits), one 16-byte LDS write at swz(row,
//     chunk), the layout both lds_b128 (K) and tr_frag (V) read.  8 such units a lane and tile.
//   * Rows at or past len are written as +0 in both images whatever codes and exponent bytes the pool holds: the
//     converter ands the packed dwords with the row's mask, it does not multiply by 0.  This replaces the bf16 kernel's
//     zeroing of the last tile's V rows and its extra barrier.  K rows there: their scores are replaced by -inf by
//     the causal mask (key > qpos), as in the bf16 kernel.  Tested with NaN codes, 0x7f / 0xff and 0x38 / 0x80 there.
//   * One image, two barriers a tile, and the K and V handoffs split.  LDS: the K image and the V image (32 KiB), two
//     code stages (2 x 16 KiB), the exponent bytes (4 KiB): 68 KiB, two workgroups a CU.  Tile kt, per wave:
//         V codes of kt -> V image | QK^T from the K image | wait for the DMA of kt + 1, issue the DMA of kt + 2 |
//         barrier 1 | K codes of kt + 1 -> K image | softmax, PV from the V image | barrier 2
//     Barrier 1 says both "every wave has read the K image" and "the V image of kt is whole"; barrier 2 both "every
//     wave has read the V image" and "the K image of kt + 1 is whole".  So V's conversion sits beside the QK^T MFMAs
//     and K's beside the softmax and the PV MFMAs of the other waves, and no wave waits for a conversion alone.  A
//     DMA has a whole tile to land.  A wave that skips a tile still converts, stages and joins both barriers.
//     (Read from the code and the ISA; a trace of the overlap was not taken.)
//   * Safety, established by reading this code (no test hands the GPU an out-of-range id or length): q_len[b] is
//     clamped into [0, Sq], so q, o and lse2 are addressed by rows below Sq only; kv_len[b] is clamped into [ql,
//     max_pages * page_size] (the host refuses Sq > max_pages * page_size); a table index is clamped into [0,
//     ceil(len / page_size) - 1], inside row b of the table; every page id is clamped into [0, num_pages) before it
//     forms an address; a staged tile kt < ceil(len / 64) lies inside page kt / tpp < ceil(len / page_size) of the
//     sequence, so a code DMA ends at or before page_size * 128 and an exponent DMA at or before page_size bytes of this
//     head's part of that pool page, with or without the hardware's range check.  An exponent byte is only ever
//     shifted into a float.  No content of block_table, kv_len, q_len or the exponent bytes moves an access outside
//     the four pools, the table row or q.
//
//   kv_append_paged_chunk_fp8_kernel   k_new, v_new bf16 [B, Hkv, Sq, 128], any Sq: kv_append_paged_chunk_kernel's grid
//                        (16 rows a block, 16 lanes a row), positions (row i < ql to kv_len[b] - ql + i; rows i >= ql
//                        are not read) and skips (a sequence whose kv_len[b] is outside [ql, max_pages * page_size], a
//                        row whose page id is outside [0, num_pages)), with kv_append_paged_fp8_kernel's row: quantize_row8,
//                        8 code bytes a lane and the exponent byte from the row's first lane, plain vector stores.
//                        Nothing of the cache is read.  Tested byte for byte against kv_quantize_ref.
//
// Not here: split-KV for a short chunk against a very long prefix, a backward, head dim 64.
// Built with attention_prefill_paged.hip's flags (packed fp32 VALU off, the MFMA VGPR form).
#include "attention_fp8.h"

namespace gtk_decode {

constexpr int kImgBytes = 2 * BK * D * 2;            // the K image, then the V image, bf16
constexpr int kCodeTile = BK * D;                    // one tile's K codes (or V codes)
constexpr int kCodeStage = 2 * kCodeTile;            // a stage: K codes, then V codes
constexpr int kExpWave = 512;                        // a wave's exponent bytes of a stage: K at 0, V at 256, as the DMAs leave them
constexpr int kExpOff = kImgBytes + 2 * kCodeStage;  // [stage][wave] exponent areas
constexpr int kSmemP8 = kExpOff + 2 * 4 * kExpWave;
static_assert(kSmemP8 <= 80 * 1024, "two workgroups a CU");

__device__ __forceinline__ int lane_id8() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// The wave's 16 rows of one tile from codes (cs: the tile's code rows, 128 bytes a row; ex: the wave's 16 exponent
// bytes) to the bf16 image img.  key_w: the key index of the wave's first row; rows at or past len become +0
__device__ __forceinline__ void convert_rows(const char* cs, const char* ex, char* img, int w, int key_w, int len) {
  int el = lane_id8();
  asm volatile("" : "+v"(el));  // the addresses below are formed here, per call, not carried through the loops
  const int g = el >> 4, i = el & 15;
  const u32x4 eb = *reinterpret_cast<const u32x4*>(ex);  // wave-uniform address: dword u = rows 4 u .. 4 u + 3
  const char* src = cs + (16 * w + g) * D + 8 * i;
  char* dst = img + (16 * w + g) * 256;
  const int ch = i ^ (g << 2);  // swz(16 w + 4 u + g, i) = 256 row + 16 (i ^ (g << 2) ^ u)
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const u32x2 c = *reinterpret_cast<const u32x2*>(src + 4 * u * D);
    const float sc = __uint_as_float(((eb[u] >> (8 * g)) & 0xffu) << 23);
    float f[8];
    cvt8(c[0], c[1], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] *= sc;
    u32x4 x = __builtin_bit_cast(u32x4, pack_hi8(f));
    const uint32_t keep = key_w + 4 * u + g < len ? ~0u : 0u;
#pragma unroll
    for (int d = 0; d < 4; ++d) x[d] &= keep;
    *reinterpret_cast<u32x4*>(dst + 4 * u * 256 + 16 * (ch ^ u)) = x;
  }
}

__global__ __launch_bounds__(256, 2) void attn_prefill_paged_fp8_kernel(
    const u16* __restrict__ q, const u8* __restrict__ kc, const u8* __restrict__ vc, const u8* __restrict__ kx,
    const u8* __restrict__ vx, const int* __restrict__ block_table, const int* __restrict__ kv_len, const int* __restrict__ q_len,
    u16* __restrict__ o, float* __restrict__ lse2, int H, int Hkv, int Sq, int page_size, int max_pages, int num_pages, float c) {
  __shared__ __attribute__((aligned(16))) char smem[kSmemP8];
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
  char* const kimg = smem;
  char* const vimg = smem + BK * D * 2;

  // lane L: the table entry of tile k0 + L
  auto load_ids = [&](int k0) {
    const int p = (k0 + lane_id8()) / tpp;
    return tab[p < np ? p : np - 1];
  };
  int ids = load_ids(0);
  int pg = 0, tin = 0;  // of the tile staged next: its page of the sequence, its tile of that page

  // the wave's 16 rows of tile kt's K and V codes and their exponent bytes into stage kt & 1, through descriptors over
  // this head's part of the tile's page in each pool; tiles are staged in order, once each, by every wave
  auto gload = [&](int kt) {
    const int id = clampi(__builtin_amdgcn_readlane(ids, kt & 63), 0, num_pages - 1);
    const size_t base = ((size_t)id * Hkv + hk) * page_size;  // the head's first row of the page, in rows
    const uint32_t nrow = (uint32_t)clampi(len - pg * page_size, 0, page_size);
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc((void*)(kc + base * D), 0, nrow * D, 0x00020000);
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc((void*)(vc + base * D), 0, nrow * D, 0x00020000);
    const __amdgpu_buffer_rsrc_t kxs = __builtin_amdgcn_make_buffer_rsrc((void*)(kx + base), 0, (nrow + 3) & ~3u, 0x00020000);
    const __amdgpu_buffer_rsrc_t vxs = __builtin_amdgcn_make_buffer_rsrc((void*)(vx + base), 0, (nrow + 3) & ~3u, 0x00020000);
    int el = lane_id8();
    asm volatile("" : "+v"(el));  // keeps the two offsets below from being carried through the loops
    const uint32_t vo = (uint32_t)(16 * el) + (uint32_t)tin * kCodeTile + 16 * w * D;  // lane-linear: 8 rows an instruction
    const uint32_t xo = (uint32_t)(4 * (el & 3)) + (uint32_t)tin * BK + 16 * w;
    char* st = smem + kImgBytes + (kt & 1) * kCodeStage + 16 * w * D;
    char* ex = smem + kExpOff + ((kt & 1) * 4 + w) * kExpWave;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(krs, (LDS_AS void*)(st + 1024 * i), 16, vo + 1024 * i, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(vrs, (LDS_AS void*)(st + kCodeTile + 1024 * i), 16, vo + 1024 * i, 0, 0, 0);
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(kxs, (LDS_AS void*)ex, 4, xo, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(vxs, (LDS_AS void*)(ex + 256), 4, xo, 0, 0, 0);
    if (++tin == tpp) tin = 0, ++pg;
    if ((kt & 63) == 63) ids = load_ids(kt + 1);  // the next 64 ids, a whole tile before the first of them is used
  };
  auto conv_k = [&](int kt) {
    convert_rows(smem + kImgBytes + (kt & 1) * kCodeStage, smem + kExpOff + ((kt & 1) * 4 + w) * kExpWave, kimg, w, kt * BK + 16 * w, len);
  };
  auto conv_v = [&](int kt) {
    convert_rows(smem + kImgBytes + (kt & 1) * kCodeStage + kCodeTile, smem + kExpOff + ((kt & 1) * 4 + w) * kExpWave + 256, vimg, w,
                 kt * BK + 16 * w, len);
  };
  // the middle of a tile: the wave's DMA of kt + 1 has landed and its reads of stage kt & 1 have returned, so the DMA
  // of kt + 2 may overwrite that stage; barrier 1; the K image is free for tile kt + 1
  auto handoff = [&](int kt) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if (kt + 2 < ntiles) gload(kt + 2);
    __syncthreads();
    if (kt + 1 < ntiles) conv_k(kt + 1);
  };
  // the end of a tile: barrier 2
  auto tile_end = [&] {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
  };

  // one KV tile, attn_prefill_paged_kernel's on the bf16 image: QK^T, the handoff, online softmax, PV.  `masked` adds the causal mask
  auto tile = [&](int kt, bool masked) {
    const int key0 = kt * BK;
    conv_v(kt);
    __builtin_amdgcn_sched_barrier(0);  // the conversion's registers are free before the K fragments are loaded
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
    handoff(kt);
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
    tile_end();
  };

  gload(0);
  if (ntiles > 1) gload(1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  conv_k(0);
  tile_end();  // the K image of tile 0 is whole
  int kt = 0;
  // tiles that lie entirely below every query of the block: no mask, no visibility test
  for (; kt < nplain; ++kt) tile(kt, false);
  // the block's diagonal, at most three tiles: per wave skipped, masked or plain
  for (; kt < ntiles; ++kt) {
    const int key0 = kt * BK;
    if (key0 <= wlast) {
      tile(kt, key0 + BK - 1 > wfirst);
    } else {  // no row of the wave sees the tile: its share of the images, the DMA and both barriers
      conv_v(kt);
      handoff(kt);
      tile_end();
    }
  }

  // attn_prefill_paged_kernel's store; a padded row stores zeros and -inf, a row at or past Sq nothing
  const int el = lane_id8(), row = q0 + (el & 31), eh = el >> 5;  // == myq, hh
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

__global__ __launch_bounds__(256) void kv_append_paged_chunk_fp8_kernel(const u16* __restrict__ k_new, const u16* __restrict__ v_new,
                                                                        u8* __restrict__ kc, u8* __restrict__ vc, u8* __restrict__ kx,
                                                                        u8* __restrict__ vx, const int* __restrict__ block_table,
                                                                        const int* __restrict__ kv_len, const int* __restrict__ q_len,
                                                                        int B, int Hkv, int Sq, int page_size, int max_pages,
                                                                        int num_pages) {
  const size_t row = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);  // of k_new [B, Hkv, Sq]; its 16 lanes leave together
  if (row >= (size_t)B * Hkv * Sq) return;
  const int i = (int)(row % Sq), hk = (int)(row / Sq % Hkv), b = (int)(row / Sq / Hkv);
  const int ql = clampi(q_len[b], 0, Sq);
  if (i >= ql) return;
  const int len = kv_len[b];
  if (len < ql || len > max_pages * page_size) return;
  const int pos = len - ql + i;  // in [0, max_pages * page_size)
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

void launch_prefill_paged_fp8(hipStream_t st, const u16* q, const u8* kc, const u8* vc, const u8* kx, const u8* vx,
                              const int* block_table, const int* kv_len, const int* q_len, u16* o, float* lse2, int B, int H, int Hkv,
                              int Sq, int page_size, int max_pages, int num_pages, float c) {
  hipLaunchKernelGGL(attn_prefill_paged_fp8_kernel, dim3(B * H, (Sq + BQ - 1) / BQ), dim3(256), 0, st, q, kc, vc, kx, vx, block_table,
                     kv_len, q_len, o, lse2, H, Hkv, Sq, page_size, max_pages, num_pages, c);
}

void launch_append_chunk_fp8(hipStream_t st, const u16* k_new, const u16* v_new, u8* kc, u8* vc, u8* kx, u8* vx, const int* block_table,
                             const int* kv_len, const int* q_len, int B, int Hkv, int Sq, int page_size, int max_pages, int num_pages) {
  const size_t rows = (size_t)B * Hkv * Sq;
  hipLaunchKernelGGL(kv_append_paged_chunk_fp8_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, k_new, v_new, kc, vc, kx,
                     vx, block_table, kv_len, q_len, B, Hkv, Sq, page_size, max_pages, num_pages);
}

}  // namespace gtk_decode
