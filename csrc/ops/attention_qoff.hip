// Causal flash attention kernels for a query chunk at an offset into longer K/V (gfx950): what a rank of a
// context-parallel job runs after the all-gather of K and V, and what chunked prefill against a KV cache
// runs.  attention_kernels.h compiled with kQoff = true, which gives the forward, dK/dV and dQ kernels
// with the key length Sk and the offset as two more parameters in namespace gtk_qoff, and their launch
// functions for the host code of attention.hip.
//
// A translation unit of its own with attention_doc.hip's flags (packed fp32 VALU off, the MFMA VGPR form;
// see _native/build.py), so that the causal and document-masked kernels stay compiled as they were.
#define GTK_ATTN_QOFF_TU 1
#include "attention_kernels.h"

namespace gtk_qoff {

void launch_fwd(dim3 grid, hipStream_t st, const u16* q, const u16* k, const u16* v, u16* o, float* lse2, int H, int Hkv, int S,
                float c, u16* ot, int Sk, int q_offset) {
  hipLaunchKernelGGL(attn_fwd2_kernel, grid, dim3(256), 0, st, q, k, v, o, lse2, H, Hkv, S, c, ot, Sk, q_offset);
}
void launch_dkdv(dim3 grid, hipStream_t st, const u16* q, const u16* k, const u16* v, const u16* dout, const float* nls,
                 const float* ndl, u16* dk, u16* dv, int H, int Hkv, int S, float c, float scale, int Sk, int q_offset) {
  hipLaunchKernelGGL(attn_bwd_dkdv_kernel, grid, dim3(256), 0, st, q, k, v, dout, nls, ndl, dk, dv, H, Hkv, S, c, scale, Sk,
                     q_offset);
}
void launch_dq(dim3 grid, hipStream_t st, const u16* q, const u16* k, const u16* v, const u16* dout, const float* lse2,
               const float* delta, u16* dq, int H, int Hkv, int S, float c, float scale, int Sk, int q_offset) {
  hipLaunchKernelGGL(attn_bwd_dq2n_kernel, grid, dim3(256), 0, st, q, k, v, dout, lse2, delta, dq, H, Hkv, S, c, scale, Sk,
                     q_offset);
}

}  // namespace gtk_qoff
