#pragma once
// Split-KV flash attention (csrc/ops/attention_splitkv.hip): the launch functions the host code of
// attention.hip reaches the kernels through, and the one rule by which a query block's keys are dealt to
// its splits, shared by the kernels, the merge and the host.
#include "bf16.h"

namespace gtk_splitkv {

using gtk::u16;

constexpr int kMaxSplits = 16;

// Query block qb of a window at q_offset sees P key blocks of 128 keys, the last one its diagonal.  Split z
// of n takes key blocks [z pp, min((z + 1) pp, P)) with pp = ceil(P / n): split 0 is never empty, the
// diagonal block lies in the last non-empty split, and the empty ones are those with z pp >= P.
struct SplitRange {
  int P, pp;
  __host__ __device__ SplitRange(int q_offset, int qb, int n) : P(q_offset / 128 + qb + 1), pp((P + n - 1) / n) {}
  __host__ __device__ int begin(int z) const { return z * pp; }
  __host__ __device__ int end(int z) const { return (z + 1) * pp < P ? (z + 1) * pp : P; }
  __host__ __device__ int nonempty() const { return (P + pp - 1) / pp; }
};

// grid (B*H, Sq/128, n): o_part fp32 [n, B, Sq, H, 128] (normalised per split), lse_part fp32 [n, B, H, Sq]
void launch_fwd(dim3 grid, hipStream_t st, const u16* q, const u16* k, const u16* v, float* o_part, float* lse_part, int H,
                int Hkv, int Sq, float c, int Sk, int q_offset);
// o bf16 [B, Sq, H, 128] and lse2 fp32 [B, H, Sq] from the n partials
void launch_combine(hipStream_t st, const float* o_part, const float* lse_part, u16* o, float* lse2, int B, int H, int Sq,
                    int n);
// grid as the forward's: dq_part fp32 [n, B, H, Sq, 128], unscaled; an empty split writes nothing
void launch_dq(dim3 grid, hipStream_t st, const u16* q, const u16* k, const u16* v, const u16* dout, const float* lse2,
               const float* delta, float* dq_part, int H, int Hkv, int Sq, float c, int Sk, int q_offset);
// dq bf16 [B, H, Sq, 128] = scale * the sum of the non-empty splits' partials
void launch_dq_reduce(hipStream_t st, const float* dq_part, u16* dq, int B, int H, int Sq, float scale, int q_offset, int n);

}  // namespace gtk_splitkv
