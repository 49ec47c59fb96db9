// Head-dim-64 flash attention kernels (attention_d64_kernels.h) and their launch functions for the host
// code of attention.hip, which dispatches on q.size(3).  A null document bound selects the causal
// instantiation.  A translation unit of its own, built with packed fp32 VALU off and the MFMA VGPR form
// (see _native/build.py), like attention_doc.hip.
#include "attention_d64_kernels.h"

namespace gtk_attn64 {

void launch_fwd(hipStream_t st, const u16* q, const u16* k, const u16* v, u16* o, float* lse2, int B, int H, int Hkv, int S,
                float c, u16* ot, const int* doc_start) {
  const dim3 grid(B * H, S / BQ);
  if (doc_start)
    hipLaunchKernelGGL(attn64_fwd_kernel<true>, grid, dim3(256), 0, st, q, k, v, o, lse2, H, Hkv, S, c, ot, doc_start);
  else
    hipLaunchKernelGGL(attn64_fwd_kernel<false>, grid, dim3(256), 0, st, q, k, v, o, lse2, H, Hkv, S, c, ot, doc_start);
}

void launch_bwd_pre(hipStream_t st, const u16* dout, const u16* out, const float* lse2, float* delta, float* nls, float* ndl,
                    int B, int H, int S, float inv_c) {
  const int rows = B * S * H;
  hipLaunchKernelGGL(attn64_bwd_pre_kernel, dim3((rows + 31) / 32), dim3(256), 0, st, dout, out, lse2, delta, nls, ndl, B, H, S,
                     inv_c);
}

void launch_dkdv(hipStream_t st, const u16* q, const u16* k, const u16* v, const u16* dout, const float* nls, const float* ndl,
                 u16* dk, u16* dv, int B, int H, int Hkv, int S, float c, float scale, const int* doc_end) {
  const dim3 grid(B * Hkv, S / KB);
  if (doc_end)
    hipLaunchKernelGGL(attn64_bwd_dkdv_kernel<true>, grid, dim3(256), 0, st, q, k, v, dout, nls, ndl, dk, dv, H, Hkv, S, c, scale,
                       doc_end);
  else
    hipLaunchKernelGGL(attn64_bwd_dkdv_kernel<false>, grid, dim3(256), 0, st, q, k, v, dout, nls, ndl, dk, dv, H, Hkv, S, c, scale,
                       doc_end);
}

void launch_dq(hipStream_t st, const u16* q, const u16* k, const u16* v, const u16* dout, const float* lse2, const float* delta,
               u16* dq, int B, int H, int Hkv, int S, float c, float scale, const int* doc_start) {
  const dim3 grid(B * H, S / BQ);
  if (doc_start)
    hipLaunchKernelGGL(attn64_bwd_dq_kernel<true>, grid, dim3(256), 0, st, q, k, v, dout, lse2, delta, dq, H, Hkv, S, c, scale,
                       doc_start);
  else
    hipLaunchKernelGGL(attn64_bwd_dq_kernel<false>, grid, dim3(256), 0, st, q, k, v, dout, lse2, delta, dq, H, Hkv, S, c, scale,
                       doc_start);
}

}  // namespace gtk_attn64
