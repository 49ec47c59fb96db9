// K7 fp8 wire: a rank packs its window once, locally, into OCP e4m3fn codes with one power-of-two scale
// per 32 elements, and its peers read the packed form: 33 bytes per 32 elements over the link against 64
// for bf16 and 128 for fp32.  Device code only, in the style of peer_allreduce.h.
//
// Format (ops/peer_ref.py: q8_quantize_ref is the same rule in numpy, and decides):
//   block b  = elements [32 b, 32 b + 32) of the call; elements at or past `count` are zero and are masked
//              here, never trusted to be zero in the window.
//   e        = the smallest integer with amax * 2^-e <= 448, clamped to [-100, 120] (amax == 0: -100), so
//              2^e, 2^-e and every dequantised value are normal fp32 numbers and both scalings are exact.
//   code     = x * 2^-e rounded to nearest even into e4m3fn, subnormal codes (quantum 2^-9) included;
//              |x * 2^-e| <= 448, so nothing saturates.  value = float(code) * 2^e.
//   non-finite: the amax is taken over the block's elements that are not NaN (fmaxf drops a quieted NaN),
//              after the count's mask; an Inf counts, so its block has e = 120, and an all-NaN block e = -100.
//              A NaN or an Inf gets a code with (code & 0x7f) == 0x7f, the format's NaN (e4m3fn has no
//              infinity; the code's sign bit is unspecified), which widens to NaN; the block's finite
//              elements are coded by the ordinary rule with that e.  Under e = 120 a magnitude of at
//              least 248 * 2^120 rounds to the code of 256 and widens to 2^128 = Inf.
// The sum is taken over the dequantised values in member order in fp32, multiplied once by `scale` and
// rounded once, as peer_reduce_vecs does: every member computes the same bits, its own contribution
// being its packed form too.
//
// Layout of a packed buffer made for NB blocks, in 16-byte vectors:
//   vectors [0, 2 NB)                : the codes, one byte per element in element order, so block b is
//                                      vectors 2 b and 2 b + 1 and code vector v holds elements [16 v, 16 v + 16);
//   vectors [2 NB, 2 NB + ceil(NB/16)): one byte per block, e + 127 (the exponent field of 2^e in fp32),
//                                      in block order, the last vector's rest unused.
// That is 33 bytes per 32 elements, rounded up to a vector.  `exp_vec` = 2 NB is a property of the
// buffer, not of the call, and the same on every member.  A lane of the sum reads the aligned 4-byte
// word that holds its block's exponent: the 64 lanes of a wave cover 32 consecutive exponent bytes, two
// vectors, which reach the memory pipeline as one request next to the wave's 1 KiB of codes.
//
// A two-shot may pack its second phase too (wire fp8x2; ops/peer_ref.py: allreduce_q8x2_ref decides).  Phase 1
// then keeps the scaled fp32 sums of its slice in registers and packs them by the same block rule (the
// same e, clamp and NaN/Inf coding, blocks counted from element 0 of the call) into the rank's second
// packed buffer, of the layout above; phase 2 reads every rank's slice of those buffers, the rank's own
// included, widens it and stores it at the output precision.  Every member's result is then the
// dequantised form of one packing, so all hold the same bits, and the cast to the output type is exact:
// at most 4 significant bits and e in [-100, 120] fit bf16.  An Inf in the sum comes out as NaN (e4m3fn
// has no infinity), a magnitude of at least 248 * 2^120 as Inf.  Both phases then move 33 bytes per 32
// elements over the links.
//
// Error feedback (peer_q8_quantize_ef_kernel; ops/peer_ref.py: q8_quantize_ef_ref decides): the rank keeps an
// fp32 residual per element of its window, what its last packing dropped.  The feedback form packs
// y = x + residual (one fp32 add, x itself where the residual is zero; then the count's mask) by the rule above and leaves y - float(code) * 2^e,
// an exact difference, as the new residual: +0 where that is not finite (y NaN or Inf, or a code that
// widens to 2^128) and past the count.  The residual is the rank's own: no peer reads it, it costs no link
// byte, no launch and no barrier, and the plain form is the same code as without it.
//
// Conversions: v_cvt_pk_fp8_f32 and v_cvt_pk_f32_fp8 through their builtins, on values already scaled by
// an exact fp32 multiply; the scaling forms (cvt_scalef32_*) are not used, so which way they apply their
// scale operand plays no part here.  tests/test_gpu_peer_q8.py compares every code with the numpy rule.
#pragma once
#include "peer_allreduce.h"
#include "probe_common.h"

namespace {

constexpr int kQ8Block = 32;                    // elements that share one scale
constexpr int kQ8ExpMin = -100, kQ8ExpMax = 120;
constexpr int kQ8Bias = 127;                    // the stored byte is e + 127

// Vectors of a packed buffer for `n_blocks` blocks, and where its exponent bytes start.
constexpr size_t q8_exp_vec(size_t n_blocks) { return 2 * n_blocks; }
constexpr size_t q8_packed_vecs(size_t n_blocks) { return 2 * n_blocks + (n_blocks + 15) / 16; }

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float q8_pow2(int n) { return __uint_as_float((unsigned int)(n + 127) << 23); }

// amax = m * 2^E with m in [1, 2): e = E - 8 when m <= 1.75 (448 = 1.75 * 2^8), else E - 7.  A zero or
// subnormal amax lands below the clamp, an infinite one above it.
__device__ __forceinline__ int q8_block_exp(float amax) {
  const unsigned int a = __float_as_uint(amax);
  const int e = (int)(a >> 23) - 127 - 8 + (int)((a & 0x7fffffu) > 0x600000u);
  return min(max(e, kQ8ExpMin), kQ8ExpMax);
}

// Two scaled values to two codes, the first in the low byte.
__device__ __forceinline__ unsigned int q8_codes2(float a, float b) {
  return (unsigned int)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xffffu;
}

// One 16-byte vector `r` of the window, vector v of it (elements [v L, v L + L)), as one of the G
// consecutive lanes that hold a block (bf16: 4 lanes of 8 elements; fp32: 8 lanes of 4): the block's amax
// is log2(G) lane exchanges, with no memory and no other wave involved; every lane stores its own codes
// (8 or 4 bytes), the first lane of a block the exponent byte.
// EF, the feedback form: `res` holds the L residual floats of the lane's elements (zero for a vector wholly
// past the count), added before the count's mask; the codes just made are widened as q8_widen widens them
// and the new residual, what the packing dropped, goes to floats [v L, v L + L) of `residual` as vectors.
template <typename TI, bool EF>
__device__ __forceinline__ void q8_quantize_vec(const u32x4& r, const u32x4 (&res)[kPeerLanes<TI> / 4], size_t v, size_t count,
                                                u32x4* __restrict__ packed, unsigned char* __restrict__ exps,
                                                u32x4* __restrict__ residual) {
  constexpr int L = kPeerLanes<TI>;
  constexpr int G = kQ8Block / L;
  const size_t first = v * L;
  float f[L];
  peer_widen(r, f);
  if constexpr (EF) {
#pragma unroll
    for (int j = 0; j < L; ++j) {
      const float q = __uint_as_float(res[j / 4][j % 4]);
      f[j] = q == 0.f ? f[j] : f[j] + q;  // x + 0 would make +0 of -0: a zero residual leaves the plain rule's codes
    }
  }
  if (first + L > count) {  // the vector the count ends in, and those after it: every other one skips the mask
#pragma unroll
    for (int j = 0; j < L; ++j)
      if (first + j >= count) f[j] = 0.f;
  }
  // The amax leaves NaNs out.  fmaxf drops a quiet NaN, but a signalling one makes v_max_f32 return a
  // NaN (IEEE mode), and the window's bits reach it as they are: so every element is quieted first.
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < L; ++j) amax = fmaxf(amax, fabsf(__builtin_canonicalizef(f[j])));
#pragma unroll
  for (int d = 1; d < G; d <<= 1) amax = fmaxf(amax, __shfl_xor(amax, d));
  const int e = q8_block_exp(amax);
  const float down = q8_pow2(-e);
  unsigned int w[L / 4];
#pragma unroll
  for (int j = 0; j < L / 4; ++j)
    w[j] = q8_codes2(f[4 * j] * down, f[4 * j + 1] * down) | (q8_codes2(f[4 * j + 2] * down, f[4 * j + 3] * down) << 16);
  if constexpr (L == 8) {
    u32x2 c;
    c[0] = w[0];
    c[1] = w[1];
    __builtin_nontemporal_store(c, reinterpret_cast<u32x2*>(packed) + v);
  } else {
    __builtin_nontemporal_store(w[0], reinterpret_cast<unsigned int*>(packed) + v);
  }
  if (v % G == 0) exps[v / G] = (unsigned char)(e + kQ8Bias);
  if constexpr (EF) {
    // The subtraction must see the rounded product: contracted into one fma, 256 * 2^120 would not be Inf.
#pragma clang fp contract(off)
    const float up = q8_pow2(e);
#pragma unroll
    for (int j = 0; j < L / 4; ++j) {
      const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false);
      const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
      const float dq[4] = {lo[0] * up, lo[1] * up, hi[0] * up, hi[1] * up};
      u32x4 n;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned int d = __float_as_uint(f[4 * j + i] - dq[i]);
        n[i] = (d & 0x7f800000u) == 0x7f800000u ? 0u : d;  // NaN or Inf in, or 2^128 out: nothing is carried
      }
      __builtin_nontemporal_store(n, residual + v * (L / 4) + j);
    }
  }
}

// Blocks [b0, b1) of the window to the same blocks of the rank's own packed buffer, one window vector
// per lane and U of them per pass, a grid apart, all loaded before the first is converted.  b0 * G and
// the grid's stride are multiples of G, so the lanes of a block take every branch together.  EF: the
// residual vectors of those elements (two per bf16 window vector, one per fp32) are loaded with them and
// rewritten; a vector wholly past the count reads neither and writes a zero residual.
template <typename TI, bool EF>
__device__ __forceinline__ void peer_q8_quantize_blocks(const u32x4* __restrict__ win, u32x4* __restrict__ packed, size_t exp_vec,
                                                        size_t b0, size_t b1, size_t count, u32x4* __restrict__ residual) {
  constexpr int L = kPeerLanes<TI>;
  constexpr int G = kQ8Block / L;
  constexpr int R = L / 4;  // residual vectors per window vector
  constexpr int U = 4;
  unsigned char* exps = reinterpret_cast<unsigned char*>(packed + exp_vec);
  const size_t end = b1 * G, stride = (size_t)gridDim.x * gtk::kStreamBlock;
  for (size_t base = b0 * G + (size_t)blockIdx.x * gtk::kStreamBlock + threadIdx.x; base < end; base += stride * U) {
    u32x4 r[U];
    u32x4 q[U][R];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t v = base + (size_t)u * stride;
      r[u] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < R; ++j) q[u][j] = u32x4{0u, 0u, 0u, 0u};
      if (v < end && v * L < count) {  // a vector wholly past the count is not read
        r[u] = __builtin_nontemporal_load(win + v);
        if constexpr (EF) {
#pragma unroll
          for (int j = 0; j < R; ++j) q[u][j] = __builtin_nontemporal_load(residual + v * R + j);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t v = base + (size_t)u * stride;
      if (v < end) q8_quantize_vec<TI, EF>(r[u], q[u], v, count, packed, exps, residual);
    }
  }
}

template <typename TI>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_q8_quantize_kernel(const u32x4* __restrict__ win,
                                                                             u32x4* __restrict__ packed, size_t exp_vec,
                                                                             size_t b0, size_t b1, size_t count) {
  peer_q8_quantize_blocks<TI, false>(win, packed, exp_vec, b0, b1, count, nullptr);
}

// The feedback form: `residual` is the rank's own fp32 buffer, one float per element of the window, read
// and rewritten in blocks [b0, b1) alone.
template <typename TI>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_q8_quantize_ef_kernel(const u32x4* __restrict__ win,
                                                                                u32x4* __restrict__ packed, size_t exp_vec,
                                                                                size_t b0, size_t b1, size_t count,
                                                                                u32x4* __restrict__ residual) {
  peer_q8_quantize_blocks<TI, true>(win, packed, exp_vec, b0, b1, count, residual);
}

// The 16 values of one code vector: float(code) * 2^e, `ebyte` being the block's stored exponent byte.
__device__ __forceinline__ void q8_widen(const u32x4& c, unsigned int ebyte, float (&f)[16]) {
  const float up = __uint_as_float(ebyte << 23);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[j], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[j], true);
    f[4 * j] = lo[0] * up;
    f[4 * j + 1] = lo[1] * up;
    f[4 * j + 2] = hi[0] * up;
    f[4 * j + 3] = hi[1] * up;
  }
}

// The 16 results of code vector v: two vectors of a bf16 out at 2 v, four of an fp32 out at 4 v, of `dst`
// through `sink` (PeerOneDst or PeerPushDst of peer_allreduce.h).
template <typename TO, typename Sink>
__device__ __forceinline__ void q8_store(const float (&acc)[16], const Sink& sink, u32x4* __restrict__ dst, size_t v) {
  constexpr int L = kPeerLanes<TO>;
  u32x4 out[16 / L];
#pragma unroll
  for (int p = 0; p < 16 / L; ++p) {
    float part[L];
#pragma unroll
    for (int j = 0; j < L; ++j) part[j] = acc[p * L + j];
    out[p] = peer_narrow(part);
  }
  sink(out, dst, v * (16 / L));
}

// The reduce's epilogue (PeerStoreEpi of peer_allreduce.h) for the sixteen sums of a code vector: one multiply
// by `scale`, one rounding and the stores of q8_store.
template <typename TO, typename Sink>
struct PeerQ8StoreEpi {
  Sink sink;
  float scale;
  template <int U>
  struct Pre {};
  template <int U>
  __device__ __forceinline__ void load(Pre<U>&, int, size_t) const {}
  template <int U>
  __device__ __forceinline__ void operator()(const Pre<U>&, int, float (&acc)[16], u32x4* __restrict__ dst, size_t v) const {
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = acc[j] * scale;
    q8_store<TO>(acc, sink, dst, v);
  }
};

// peer_reduce_vecs on the packed form: U code vectors per lane, `stride` apart from `i`; the k x U code
// loads and the k x U exponent words (member-major, all in flight before the first add) and the epilogue's
// own, then per position the sum in member order and the epilogue: for the reduce one multiply by `scale`,
// one rounding and the stores.  r[][] and x[][] are indexed by constants only.
template <int KB, int U, typename Epi>
__device__ __forceinline__ void peer_q8_sum_vecs(const SrcSet& srcs, int k, size_t exp_vec, const Epi& epi, u32x4* __restrict__ dst,
                                                 size_t i, size_t stride) {
  u32x4 r[KB][U];
  unsigned int x[KB][U];
  typename Epi::template Pre<U> pre;
#pragma unroll
  for (int m = 0; m < KB; ++m)
    if (m < k) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const size_t v = i + (size_t)u * stride;
        r[m][u] = __builtin_nontemporal_load(srcs.p[m] + v);
        x[m][u] = __builtin_nontemporal_load(reinterpret_cast<const unsigned int*>(srcs.p[m] + exp_vec) + (v >> 3));
      }
    }
#pragma unroll
  for (int u = 0; u < U; ++u) epi.load(pre, u, i + (size_t)u * stride);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const size_t v = i + (size_t)u * stride;
    const unsigned int shift = 8u * (unsigned int)((v >> 1) & 3);  // block v / 2 is byte (v / 2) % 4 of word v / 8
    float acc[16];
    q8_widen(r[0][u], (x[0][u] >> shift) & 0xffu, acc);
#pragma unroll
    for (int m = 1; m < KB; ++m)
      if (m < k) {
        float y[16];
        q8_widen(r[m][u], (x[m][u] >> shift) & 0xffu, y);
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = acc[j] + y[j];
      }
    epi(pre, u, acc, dst, v);
  }
}

// The epilogue of the sum over members m < k of the dequantised blocks [b0, b1) of srcs.p[m], every member's
// packed buffer, code vector by code vector.  With PeerQ8StoreEpi: blocks [b0, b1) of dst, and of what else the
// sink stores to (whole blocks of the output type TO: float, or bf16 as raw u16) = scale * that sum.
// The range is code vectors [2 b0, 2 b1), cut as peer_reduce_kernel cuts its vectors: whole tiles in one
// contiguous run per block, the rest one vector per lane over the whole grid.
template <int KB, int U, typename Epi>
__device__ __forceinline__ void peer_q8_sum_range(const SrcSet& srcs, int k, size_t exp_vec, size_t b0, size_t b1, const Epi& epi,
                                                  u32x4* __restrict__ dst) {
  const size_t v0 = 2 * b0, v1 = 2 * b1;
  const size_t tile = (size_t)gtk::kStreamBlock * U;
  const size_t n_tiles = (v1 - v0) / tile;
  const size_t per = (n_tiles + gridDim.x - 1) / gridDim.x;
  const size_t t0 = (size_t)blockIdx.x * per;
  const size_t t1 = std::min(n_tiles, t0 + per);
  for (size_t t = t0; t < t1; ++t)
    peer_q8_sum_vecs<KB, U>(srcs, k, exp_vec, epi, dst, v0 + t * tile + threadIdx.x, gtk::kStreamBlock);
  for (size_t i = v0 + n_tiles * tile + (size_t)blockIdx.x * gtk::kStreamBlock + threadIdx.x; i < v1;
       i += (size_t)gridDim.x * gtk::kStreamBlock)
    peer_q8_sum_vecs<KB, 1>(srcs, k, exp_vec, epi, dst, i, 0);
}

// The sum into the launching member's own `dst`.
template <typename TO, int KB, int U>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_q8_sum_kernel(SrcSet srcs, int k, size_t exp_vec, size_t b0,
                                                                        size_t b1, u32x4* __restrict__ dst, float scale) {
  peer_q8_sum_range<KB, U>(srcs, k, exp_vec, b0, b1, PeerQ8StoreEpi<TO, PeerOneDst>{PeerOneDst{}, scale}, dst);
}

// The push form of the sum: the same blocks, sum and rounding, every result vector stored to the same
// offset of every dsts.p[d], d < k (every member's `out`), as peer_reduce_push_kernel does.
template <typename TO, int KB, int U>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_q8_sum_push_kernel(SrcSet srcs, DstSet dsts, int k, size_t exp_vec,
                                                                             size_t b0, size_t b1, float scale) {
  peer_q8_sum_range<KB, U>(srcs, k, exp_vec, b0, b1, PeerQ8StoreEpi<TO, PeerPushDst<KB>>{PeerPushDst<KB>{dsts, k}, scale}, dsts.p[0]);
}

// peer_q8_sum_vecs up to the multiply by `scale` (k x U code vectors and exponent words in flight, the sum
// in member order), then the 16 results a lane holds are packed, not stored: a block is the two adjacent
// lanes with code vectors 2 b and 2 b + 1, so its amax is one lane exchange after the canonicalise / fmaxf
// of q8_quantize_vec; every lane stores its 16 codes as one vector, the even lane the exponent byte.
template <int KB, int U>
__device__ __forceinline__ void peer_q8_repack_vecs(const SrcSet& srcs, int k, size_t exp_vec, u32x4* __restrict__ packed,
                                                    unsigned char* __restrict__ exps, size_t i, size_t stride, float scale) {
  u32x4 r[KB][U];
  unsigned int x[KB][U];
#pragma unroll
  for (int m = 0; m < KB; ++m)
    if (m < k) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const size_t v = i + (size_t)u * stride;
        r[m][u] = __builtin_nontemporal_load(srcs.p[m] + v);
        x[m][u] = __builtin_nontemporal_load(reinterpret_cast<const unsigned int*>(srcs.p[m] + exp_vec) + (v >> 3));
      }
    }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const size_t v = i + (size_t)u * stride;
    const unsigned int shift = 8u * (unsigned int)((v >> 1) & 3);
    float acc[16];
    q8_widen(r[0][u], (x[0][u] >> shift) & 0xffu, acc);
#pragma unroll
    for (int m = 1; m < KB; ++m)
      if (m < k) {
        float y[16];
        q8_widen(r[m][u], (x[m][u] >> shift) & 0xffu, y);
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = acc[j] + y[j];
      }
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = acc[j] * scale;
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) amax = fmaxf(amax, fabsf(__builtin_canonicalizef(acc[j])));
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    const int e = q8_block_exp(amax);
    const float down = q8_pow2(-e);
    u32x4 c;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      c[j] = q8_codes2(acc[4 * j] * down, acc[4 * j + 1] * down) | (q8_codes2(acc[4 * j + 2] * down, acc[4 * j + 3] * down) << 16);
    __builtin_nontemporal_store(c, packed + v);
    if ((v & 1) == 0) exps[v >> 1] = (unsigned char)(e + kQ8Bias);
  }
}

// Phase 1 of the fp8x2 two-shot: blocks [b0, b1) of `packed` (the rank's second packed buffer, its
// exponent bytes at `exp_vec` too) = the packed form of scale * the sum over members m < k of the
// dequantised blocks [b0, b1) of srcs.p[m].  The range is cut as peer_q8_sum_kernel cuts it.  The first
// code vector 2 b0, the tile (kStreamBlock x U) and the tail's grid stride are even, so a lane's vector
// has the parity of its threadIdx.x: lanes 2 j and 2 j + 1 of one wave hold the two vectors of one block.
// The tile runs have no per-lane branch, and in the tail an even vector below the even end 2 b1 has its
// odd neighbour below it as well, so the two lanes of a block take every branch together.
template <int KB, int U>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_q8_repack_kernel(SrcSet srcs, int k, size_t exp_vec, size_t b0,
                                                                           size_t b1, u32x4* __restrict__ packed, float scale) {
  unsigned char* exps = reinterpret_cast<unsigned char*>(packed + exp_vec);
  const size_t v0 = 2 * b0, v1 = 2 * b1;
  const size_t tile = (size_t)gtk::kStreamBlock * U;
  const size_t n_tiles = (v1 - v0) / tile;
  const size_t per = (n_tiles + gridDim.x - 1) / gridDim.x;
  const size_t t0 = (size_t)blockIdx.x * per;
  const size_t t1 = std::min(n_tiles, t0 + per);
  for (size_t t = t0; t < t1; ++t)
    peer_q8_repack_vecs<KB, U>(srcs, k, exp_vec, packed, exps, v0 + t * tile + threadIdx.x, gtk::kStreamBlock, scale);
  for (size_t i = v0 + n_tiles * tile + (size_t)blockIdx.x * gtk::kStreamBlock + threadIdx.x; i < v1;
       i += (size_t)gridDim.x * gtk::kStreamBlock)
    peer_q8_repack_vecs<KB, 1>(srcs, k, exp_vec, packed, exps, i, 0, scale);
}

// Phase 2 of the fp8x2 two-shot: slice s is blocks [first, first + count) of sl.p[s], a rank's second
// packed buffer (this rank's own is one of them), widened with the exponent byte read as the sum reads
// it and stored to the same blocks of dst in the output type TO.  Block b of the grid serves slice
// b % nsrc with gridDim / nsrc blocks, as peer_allgather_kernel does; slices may be empty.  U code
// vectors and exponent words per lane are loaded before the first is converted.
template <typename TO>
__global__ __launch_bounds__(gtk::kStreamBlock) void peer_q8_unpack_kernel(SliceSet sl, int nsrc, size_t exp_vec,
                                                                           u32x4* __restrict__ dst) {
  constexpr int U = 4;
  const int s = blockIdx.x % nsrc;
  const size_t blk = blockIdx.x / nsrc, nblk = gridDim.x / nsrc;
  const u32x4* src = sl.p[s];
  const unsigned int* exps = reinterpret_cast<const unsigned int*>(src + exp_vec);
  const size_t v1 = 2 * (sl.first[s] + sl.count[s]), stride = nblk * gtk::kStreamBlock;
  for (size_t base = 2 * sl.first[s] + blk * gtk::kStreamBlock + threadIdx.x; base < v1; base += stride * U) {
    u32x4 r[U];
    unsigned int x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t v = base + (size_t)u * stride;
      r[u] = u32x4{0u, 0u, 0u, 0u};
      x[u] = 0u;
      if (v < v1) {
        r[u] = __builtin_nontemporal_load(src + v);
        x[u] = __builtin_nontemporal_load(exps + (v >> 3));
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t v = base + (size_t)u * stride;
      if (v < v1) {
        float f[16];
        q8_widen(r[u], (x[u] >> (8u * (unsigned int)((v >> 1) & 3))) & 0xffu, f);
        q8_store<TO>(f, PeerOneDst{}, dst, v);
      }
    }
  }
}

}  // namespace
