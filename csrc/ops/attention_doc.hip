// Document-masked flash attention kernels for packed sequences (gfx950): attention_kernels.h compiled
// with kDoc = true, which gives the forward, dK/dV and dQ kernels with the document bounds as one more
// parameter in namespace gtk_docmask, and their launch functions for the host code of attention.hip.
//
// A translation unit of their own, so that this code is built with packed fp32 VALU off
// (-target-feature -packed-fp32-ops, see _native/build.py) while the causal kernels of attention.hip
// keep the flags, and with them the code, they were measured with.
#define GTK_ATTN_DOC_TU 1
#include "attention_kernels.h"

namespace gtk_docmask {

void launch_fwd(dim3 grid, hipStream_t st, const u16* q, const u16* k, const u16* v, u16* o, float* lse2, int H, int Hkv, int S,
                float c, u16* ot, const int* doc_start) {
  hipLaunchKernelGGL(attn_fwd2_kernel, grid, dim3(256), 0, st, q, k, v, o, lse2, H, Hkv, S, c, ot, doc_start);
}
void launch_dkdv(dim3 grid, hipStream_t st, const u16* q, const u16* k, const u16* v, const u16* dout, const float* nls,
                 const float* ndl, u16* dk, u16* dv, int H, int Hkv, int S, float c, float scale, const int* doc_end) {
  hipLaunchKernelGGL(attn_bwd_dkdv_kernel, grid, dim3(256), 0, st, q, k, v, dout, nls, ndl, dk, dv, H, Hkv, S, c, scale, doc_end);
}
void launch_dq(dim3 grid, hipStream_t st, const u16* q, const u16* k, const u16* v, const u16* dout, const float* lse2,
               const float* delta, u16* dq, int H, int Hkv, int S, float c, float scale, const int* doc_start) {
  hipLaunchKernelGGL(attn_bwd_dq2n_kernel, grid, dim3(256), 0, st, q, k, v, dout, lse2, delta, dq, H, Hkv, S, c, scale, doc_start);
}

}  // namespace gtk_docmask
