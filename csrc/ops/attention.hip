// Causal GQA flash attention for gfx950: the causal kernels and the pre-kernel (attention_kernels.h
// compiled with kDoc = false) and the host code of both masks.  The document-masked kernels of packed
// sequences are the same header compiled with kDoc = true in attention_doc.hip; the bindings here reach
// them through gtk_docmask::launch_*.  Head dim 64 goes to the kernels of attention_d64.hip (both masks)
// through gtk_attn64::launch_*; the host checks and the outputs are the same.  A query chunk at an offset
// into longer K/V (attn_*_qoff) goes to the kernels of attention_qoff.hip through gtk_qoff::launch_*, and with
// its keys split over several workgroups (attn_*_qoff_split) to those of attention_splitkv.hip.  A decode step
// over a ragged KV cache (attn_decode) goes to the kernel of attention_decode.hip through gtk_decode::launch, and
// over a paged cache (attn_decode_paged, kv_append_paged) to those of attention_decode_paged.hip, over a paged
// cache of e4m3 codes (attn_decode_paged_fp8, kv_append_paged_fp8) to those of attention_decode_paged_fp8.hip.  Prefill
// over the paged cache (attn_prefill_paged, kv_append_paged_chunk) goes to the kernels of attention_prefill_paged.hip, over
// the fp8 cache (attn_prefill_paged_fp8, kv_append_paged_chunk_fp8) to those of attention_prefill_paged_fp8.hip.
#include "attention_kernels.h"
#include "attention_splitkv.h"

namespace gtk_attn64 {  // csrc/ops/attention_d64.hip; a null document bound: the causal kernels

using gtk::u16;

void launch_fwd(hipStream_t st, const u16* q, const u16* k, const u16* v, u16* o, float* lse2, int B, int H, int Hkv, int S,
                float c, u16* ot, const int* doc_start);
void launch_bwd_pre(hipStream_t st, const u16* dout, const u16* out, const float* lse2, float* delta, float* nls, float* ndl,
                    int B, int H, int S, float inv_c);
void launch_dkdv(hipStream_t st, const u16* q, const u16* k, const u16* v, const u16* dout, const float* nls, const float* ndl,
                 u16* dk, u16* dv, int B, int H, int Hkv, int S, float c, float scale, const int* doc_end);
void launch_dq(hipStream_t st, const u16* q, const u16* k, const u16* v, const u16* dout, const float* lse2, const float* delta,
               u16* dq, int B, int H, int Hkv, int S, float c, float scale, const int* doc_start);

}  // namespace gtk_attn64

namespace gtk_decode {  // csrc/ops/attention_decode.hip

using gtk::u16;

constexpr int kMaxRows = 32;    // Sq * (H / Hkv): the query columns of one 32x32 MFMA tile
constexpr int kMaxSplits = 64;

// grid (B*Hkv, n).  n = 1: o bf16 [B, Sq, H, 128] and lse2 fp32 [B, H, Sq]; n > 1: the partials o_part fp32
// [n, B, Sq, H, 128] and lse_part fp32 [n, B, H, Sq] that gtk_splitkv::launch_combine reads
void launch(hipStream_t st, const u16* q, const u16* kc, const u16* vc, const int* kv_len, u16* o, float* lse2, float* o_part,
            float* lse_part, int B, int H, int Hkv, int Sq, int Smax, float c, int n);

// csrc/ops/attention_decode_paged.hip: the same over pools [num_pages, Hkv, page_size, 128] and an int32 block table
// [B, max_pages], and the append of k_new, v_new [B, Hkv, Sq, 128] at positions kv_len[b] - Sq .. kv_len[b] - 1
constexpr int kMaxAppend = 32;
void launch_paged(hipStream_t st, const u16* q, const u16* kp, const u16* vp, const int* block_table, const int* kv_len, u16* o,
                  float* lse2, float* o_part, float* lse_part, int B, int H, int Hkv, int Sq, int page_size, int max_pages,
                  int num_pages, float c, int n);
void launch_append(hipStream_t st, const u16* k_new, const u16* v_new, u16* kp, u16* vp, const int* block_table, const int* kv_len,
                   int B, int Hkv, int Sq, int page_size, int max_pages, int num_pages);

// csrc/ops/attention_decode_paged_fp8.hip: the same two over a cache of e4m3 codes, kc, vc uint8 [num_pages, Hkv,
// page_size, 128], and one exponent byte per row, kx, vx uint8 [num_pages, Hkv, page_size]; the append quantises
void launch_paged_fp8(hipStream_t st, const u16* q, const uint8_t* kc, const uint8_t* vc, const uint8_t* kx, const uint8_t* vx,
                      const int* block_table, const int* kv_len, u16* o, float* lse2, float* o_part, float* lse_part, int B, int H,
                      int Hkv, int Sq, int page_size, int max_pages, int num_pages, float c, int n);
void launch_append_fp8(hipStream_t st, const u16* k_new, const u16* v_new, uint8_t* kc, uint8_t* vc, uint8_t* kx, uint8_t* vx,
                       const int* block_table, const int* kv_len, int B, int Hkv, int Sq, int page_size, int max_pages, int num_pages);

// csrc/ops/attention_prefill_paged.hip: ragged query chunks over the bf16 pools, grid (B*H, ceil(Sq / 128)), q_len int32
// [B] the real rows of each sequence; and the append of a chunk's rows, any Sq, in one launch
void launch_prefill_paged(hipStream_t st, const u16* q, const u16* kp, const u16* vp, const int* block_table, const int* kv_len,
                          const int* q_len, u16* o, float* lse2, int B, int H, int Hkv, int Sq, int page_size, int max_pages,
                          int num_pages, float c);
void launch_append_chunk(hipStream_t st, const u16* k_new, const u16* v_new, u16* kp, u16* vp, const int* block_table,
                         const int* kv_len, const int* q_len, int B, int Hkv, int Sq, int page_size, int max_pages, int num_pages);

// csrc/ops/attention_prefill_paged_fp8.hip: the same two over the cache of e4m3 codes; the append quantises
void launch_prefill_paged_fp8(hipStream_t st, const u16* q, const uint8_t* kc, const uint8_t* vc, const uint8_t* kx, const uint8_t* vx,
                              const int* block_table, const int* kv_len, const int* q_len, u16* o, float* lse2, int B, int H, int Hkv,
                              int Sq, int page_size, int max_pages, int num_pages, float c);
void launch_append_chunk_fp8(hipStream_t st, const u16* k_new, const u16* v_new, uint8_t* kc, uint8_t* vc, uint8_t* kx, uint8_t* vx,
                             const int* block_table, const int* kv_len, const int* q_len, int B, int Hkv, int Sq, int page_size,
                             int max_pages, int num_pages);

}  // namespace gtk_decode

namespace gtk_attn {

// ==================================================================================== host
void check_qkv(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v) {
  for (const at::Tensor* x : {&q, &k, &v})
    TORCH_CHECK(x->is_cuda() && x->scalar_type() == at::kBFloat16 && x->is_contiguous() && x->dim() == 4,
                "attention: q/k/v must be contiguous bf16 [B, heads, S, D] GPU tensors");
  const int64_t Dh = q.size(3);
  TORCH_CHECK((Dh == 64 || Dh == D) && k.size(3) == Dh && v.size(3) == Dh, "attention: head dim must be 64 or 128");
  TORCH_CHECK(k.sizes() == v.sizes() && q.size(0) == k.size(0) && q.size(2) == k.size(2), "attention: shape mismatch");
  TORCH_CHECK(q.size(1) % k.size(1) == 0, "attention: q heads must be a multiple of kv heads");
  TORCH_CHECK(q.size(2) % BQ == 0, "attention: sequence length must be a multiple of 128");
  TORCH_CHECK(q.size(1) * q.size(2) * Dh * 2 < (int64_t(1) << 31), "attention: per-batch q/dO bytes must fit the 32-bit buffer offsets");
  TORCH_CHECK(k.device() == q.device() && v.device() == q.device(), "attention: q/k/v must be on one device");
}

// the forward takes its running max on raw scores and scales afterwards: only right for c > 0
void check_scale(double scale) {
  TORCH_CHECK(std::isfinite(scale) && scale > 0 && std::isfinite((float)scale) && (float)scale > 0.f,
              "attention: scale must be finite and greater than 0");
}

// the document bounds of fused.doc_bounds: the kernels clamp their content, not their extent
void check_doc(const at::Tensor& q, const at::Tensor& doc_start, const at::Tensor& doc_end) {
  for (const at::Tensor* x : {&doc_start, &doc_end})
    TORCH_CHECK(x->is_cuda() && x->device() == q.device() && x->scalar_type() == at::kInt && x->is_contiguous() &&
                    x->dim() == 2 && x->size(0) == q.size(0) && x->size(1) == q.size(2),
                "attention: doc_start/doc_end must be contiguous int32 [B, S] GPU tensors on q's device");
}

// forward (fwd2); with_t: also O^T [H*D, B*S] (the o-projection's NT-layout x^T) from the epilogue;
// doc_start / doc_end: both or neither, the document-masked kernel
std::vector<at::Tensor> attn_fwd_impl(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, double scale,
                                      bool with_t, const at::Tensor* doc_start = nullptr,
                                      const at::Tensor* doc_end = nullptr) {
  check_qkv(q, k, v);
  check_scale(scale);
  if (doc_start) check_doc(q, *doc_start, *doc_end);
  const int B = q.size(0), H = q.size(1), S = q.size(2), Hkv = k.size(1), Dh = q.size(3);
  auto o = at::empty({B, S, H, Dh}, q.options());
  auto lse = at::empty({B, H, S}, q.options().dtype(at::kFloat));
  const float c = (float)(scale * 1.4426950408889634);
  at::Tensor ot;
  if (with_t) ot = at::empty({(int64_t)H * Dh, (int64_t)B * S}, q.options());
  if (Dh == 64)
    gtk_attn64::launch_fwd(cur_stream(), bp(q), bp(k), bp(v), bpm(o), lse.data_ptr<float>(), B, H, Hkv, S, c,
                           with_t ? bpm(ot) : nullptr, doc_start ? doc_start->data_ptr<int>() : nullptr);
  else if (doc_start)
    gtk_docmask::launch_fwd(dim3(B * H, S / BQ), cur_stream(), bp(q), bp(k), bp(v), bpm(o), lse.data_ptr<float>(), H, Hkv, S, c,
                            with_t ? bpm(ot) : nullptr, doc_start->data_ptr<int>());
  else
    hipLaunchKernelGGL(attn_fwd2_kernel, dim3(B * H, S / BQ), dim3(256), 0, cur_stream(), bp(q), bp(k), bp(v), bpm(o),
                       lse.data_ptr<float>(), H, Hkv, S, c, with_t ? bpm(ot) : nullptr);
  if (with_t) return {o, lse, ot};
  return {o, lse};
}

// the document-masked forward: the same outputs, query i seeing the keys doc_start[b, i] .. i
std::vector<at::Tensor> attn_fwd_doc(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, double scale,
                                     const at::Tensor& doc_start, const at::Tensor& doc_end) {
  return attn_fwd_impl(q, k, v, scale, false, &doc_start, &doc_end);
}

std::vector<at::Tensor> attn_fwd_t_doc(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, double scale,
                                       const at::Tensor& doc_start, const at::Tensor& doc_end) {
  return attn_fwd_impl(q, k, v, scale, true, &doc_start, &doc_end);
}

// {o, lse, ot}
std::vector<at::Tensor> attn_fwd_t(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, double scale) {
  return attn_fwd_impl(q, k, v, scale, true);
}

std::vector<at::Tensor> attn_fwd(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, double scale) {
  return attn_fwd_impl(q, k, v, scale, false);
}

// backward: delta (+ -lse/c, -delta for dK/dV), dK/dV, dQ
std::vector<at::Tensor> attn_bwd_impl(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                                      const at::Tensor& out, const at::Tensor& lse, double scale,
                                      const at::Tensor* doc_start = nullptr, const at::Tensor* doc_end = nullptr) {
  check_qkv(q, k, v);
  check_scale(scale);
  if (doc_start) check_doc(q, *doc_start, *doc_end);
  const int B = q.size(0), H = q.size(1), S = q.size(2), Hkv = k.size(1), Dh = q.size(3);
  for (const at::Tensor* x : {&dout, &out})
    TORCH_CHECK(x->is_cuda() && x->device() == q.device() && x->scalar_type() == at::kBFloat16 && x->is_contiguous() &&
                    x->dim() == 4 && x->size(0) == B && x->size(1) == S && x->size(2) == H && x->size(3) == Dh,
                "attention bwd: dout/out must be contiguous bf16 [B, S, H, D] GPU tensors on q's device");
  TORCH_CHECK(lse.is_cuda() && lse.device() == q.device() && lse.is_contiguous() && lse.scalar_type() == at::kFloat &&
                  lse.dim() == 3 && lse.size(0) == B && lse.size(1) == H && lse.size(2) == S,
              "attention bwd: lse must be a contiguous fp32 [B, H, S] GPU tensor on q's device");
  auto fopt = q.options().dtype(at::kFloat);
  auto delta = at::empty({B, H, S}, fopt), nls = at::empty({B, H, S}, fopt), ndl = at::empty({B, H, S}, fopt);
  auto dq = at::empty_like(q), dk = at::empty_like(k), dv = at::empty_like(v);
  const int rows = B * S * H;
  const float c = (float)(scale * 1.4426950408889634);
  if (Dh == 64) {
    gtk_attn64::launch_bwd_pre(cur_stream(), bp(dout), bp(out), lse.data_ptr<float>(), delta.data_ptr<float>(),
                               nls.data_ptr<float>(), ndl.data_ptr<float>(), B, H, S, 1.f / c);
    gtk_attn64::launch_dkdv(cur_stream(), bp(q), bp(k), bp(v), bp(dout), nls.data_ptr<float>(), ndl.data_ptr<float>(), bpm(dk),
                            bpm(dv), B, H, Hkv, S, c, (float)scale, doc_end ? doc_end->data_ptr<int>() : nullptr);
    gtk_attn64::launch_dq(cur_stream(), bp(q), bp(k), bp(v), bp(dout), lse.data_ptr<float>(), delta.data_ptr<float>(), bpm(dq), B,
                          H, Hkv, S, c, (float)scale, doc_start ? doc_start->data_ptr<int>() : nullptr);
    return {dq, dk, dv};
  }
  hipLaunchKernelGGL(attn_bwd_pre_kernel, dim3((rows + 15) / 16), dim3(256), 0, cur_stream(), bp(dout), bp(out),
                     lse.data_ptr<float>(), delta.data_ptr<float>(), nls.data_ptr<float>(), ndl.data_ptr<float>(), B, H, S,
                     1.f / c);
  if (doc_start) {
    gtk_docmask::launch_dkdv(dim3(B * Hkv, S / KB), cur_stream(), bp(q), bp(k), bp(v), bp(dout), nls.data_ptr<float>(),
                             ndl.data_ptr<float>(), bpm(dk), bpm(dv), H, Hkv, S, c, (float)scale, doc_end->data_ptr<int>());
    gtk_docmask::launch_dq(dim3(B * H, S / BQ), cur_stream(), bp(q), bp(k), bp(v), bp(dout), lse.data_ptr<float>(),
                           delta.data_ptr<float>(), bpm(dq), H, Hkv, S, c, (float)scale, doc_start->data_ptr<int>());
    return {dq, dk, dv};
  }
  hipLaunchKernelGGL(attn_bwd_dkdv_kernel, dim3(B * Hkv, S / KB), dim3(256), 0, cur_stream(), bp(q), bp(k), bp(v), bp(dout),
                     nls.data_ptr<float>(), ndl.data_ptr<float>(), bpm(dk), bpm(dv), H, Hkv, S, c, (float)scale);
  hipLaunchKernelGGL(attn_bwd_dq2n_kernel, dim3(B * H, S / BQ), dim3(256), 0, cur_stream(), bp(q), bp(k), bp(v), bp(dout),
                     lse.data_ptr<float>(), delta.data_ptr<float>(), bpm(dq), H, Hkv, S, c, (float)scale);
  return {dq, dk, dv};
}

std::vector<at::Tensor> attn_bwd(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                                 const at::Tensor& out, const at::Tensor& lse, double scale) {
  return attn_bwd_impl(dout, q, k, v, out, lse, scale);
}

// ---------------------------------------------------------------- a query chunk at an offset into longer K/V
// q [B, H, Sq, 128] stands at positions q_offset .. q_offset + Sq - 1 of the Sk keys of k, v [B, Hkv, Sk, 128];
// query i sees key j iff j <= q_offset + i.  check_qkv's checks with the equal sequence lengths replaced by
// the window's requirements; every refusal names what was wrong.
void check_qkv_qoff(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, int64_t q_offset) {
  for (const at::Tensor* x : {&q, &k, &v})
    TORCH_CHECK(x->is_cuda() && x->scalar_type() == at::kBFloat16 && x->is_contiguous() && x->dim() == 4,
                "attention: q/k/v must be contiguous bf16 [B, heads, S, D] GPU tensors");
  TORCH_CHECK(q.size(3) == D && k.size(3) == D && v.size(3) == D, "attention: q_offset needs head dim 128, got ", q.size(3));
  TORCH_CHECK(k.sizes() == v.sizes() && q.size(0) == k.size(0), "attention: shape mismatch (k and v alike, one batch size)");
  TORCH_CHECK(q.size(1) % k.size(1) == 0, "attention: q heads must be a multiple of kv heads");
  const int64_t Sq = q.size(2), Sk = k.size(2);
  TORCH_CHECK(Sq > 0 && Sq % BQ == 0, "attention: query length must be a positive multiple of 128, got ", Sq);
  TORCH_CHECK(Sk % KB == 0, "attention: key length must be a multiple of 128, got ", Sk);
  TORCH_CHECK(q_offset >= 0 && q_offset % BQ == 0, "attention: q_offset must be a non-negative multiple of 128, got ", q_offset);
  TORCH_CHECK(q_offset + Sq <= Sk, "attention: q_offset + query length (", q_offset, " + ", Sq, ") exceeds the key length ", Sk);
  TORCH_CHECK(q.size(1) * Sq * D * 2 < (int64_t(1) << 31), "attention: per-batch q/dO bytes must fit the 32-bit buffer offsets");
  TORCH_CHECK(k.size(1) * Sk * D * 2 < (int64_t(1) << 31), "attention: per-batch K/V bytes must fit the 32-bit buffer offsets");
  TORCH_CHECK(k.device() == q.device() && v.device() == q.device(), "attention: q/k/v must be on one device");
}

std::vector<at::Tensor> attn_fwd_qoff_impl(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, double scale,
                                           int64_t q_offset, bool with_t) {
  check_qkv_qoff(q, k, v, q_offset);
  check_scale(scale);
  const int B = q.size(0), H = q.size(1), Sq = q.size(2), Hkv = k.size(1), Sk = k.size(2);
  auto o = at::empty({B, Sq, H, D}, q.options());
  auto lse = at::empty({B, H, Sq}, q.options().dtype(at::kFloat));
  at::Tensor ot;
  if (with_t) ot = at::empty({(int64_t)H * D, (int64_t)B * Sq}, q.options());
  gtk_qoff::launch_fwd(dim3(B * H, Sq / BQ), cur_stream(), bp(q), bp(k), bp(v), bpm(o), lse.data_ptr<float>(), H, Hkv, Sq,
                       (float)(scale * 1.4426950408889634), with_t ? bpm(ot) : nullptr, Sk, (int)q_offset);
  if (with_t) return {o, lse, ot};
  return {o, lse};
}

// -> (o [B, Sq, H, 128], lse2 [B, H, Sq])
std::vector<at::Tensor> attn_fwd_qoff(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, double scale,
                                      int64_t q_offset) {
  return attn_fwd_qoff_impl(q, k, v, scale, q_offset, false);
}

// -> (o, lse2, O^T [H*128, B*Sq])
std::vector<at::Tensor> attn_fwd_t_qoff(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, double scale,
                                        int64_t q_offset) {
  return attn_fwd_qoff_impl(q, k, v, scale, q_offset, true);
}

// what the window's backward is given beside q, k, v
void check_bwd_qoff(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& out, const at::Tensor& lse) {
  const int64_t B = q.size(0), H = q.size(1), Sq = q.size(2);
  for (const at::Tensor* x : {&dout, &out})
    TORCH_CHECK(x->is_cuda() && x->device() == q.device() && x->scalar_type() == at::kBFloat16 && x->is_contiguous() &&
                    x->dim() == 4 && x->size(0) == B && x->size(1) == Sq && x->size(2) == H && x->size(3) == D,
                "attention bwd: dout/out must be contiguous bf16 [B, Sq, H, D] GPU tensors on q's device");
  TORCH_CHECK(lse.is_cuda() && lse.device() == q.device() && lse.is_contiguous() && lse.scalar_type() == at::kFloat &&
                  lse.dim() == 3 && lse.size(0) == B && lse.size(1) == H && lse.size(2) == Sq,
              "attention bwd: lse must be a contiguous fp32 [B, H, Sq] GPU tensor on q's device");
}

// -> (dq [B, H, Sq, 128], dk, dv [B, Hkv, Sk, 128]) from the out and lse it is given; keys no query sees
// (at or after q_offset + Sq) get zeros, written by the dK/dV kernel
std::vector<at::Tensor> attn_bwd_qoff(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                                      const at::Tensor& out, const at::Tensor& lse, double scale, int64_t q_offset) {
  check_qkv_qoff(q, k, v, q_offset);
  check_scale(scale);
  const int B = q.size(0), H = q.size(1), Sq = q.size(2), Hkv = k.size(1), Sk = k.size(2);
  check_bwd_qoff(dout, q, out, lse);
  auto fopt = q.options().dtype(at::kFloat);
  auto delta = at::empty({B, H, Sq}, fopt), nls = at::empty({B, H, Sq}, fopt), ndl = at::empty({B, H, Sq}, fopt);
  auto dq = at::empty_like(q), dk = at::empty_like(k), dv = at::empty_like(v);
  const int rows = B * Sq * H;
  const float c = (float)(scale * 1.4426950408889634);
  hipLaunchKernelGGL(attn_bwd_pre_kernel, dim3((rows + 15) / 16), dim3(256), 0, cur_stream(), bp(dout), bp(out),
                     lse.data_ptr<float>(), delta.data_ptr<float>(), nls.data_ptr<float>(), ndl.data_ptr<float>(), B, H, Sq,
                     1.f / c);
  gtk_qoff::launch_dkdv(dim3(B * Hkv, Sk / KB), cur_stream(), bp(q), bp(k), bp(v), bp(dout), nls.data_ptr<float>(),
                        ndl.data_ptr<float>(), bpm(dk), bpm(dv), H, Hkv, Sq, c, (float)scale, Sk, (int)q_offset);
  gtk_qoff::launch_dq(dim3(B * H, Sq / BQ), cur_stream(), bp(q), bp(k), bp(v), bp(dout), lse.data_ptr<float>(),
                      delta.data_ptr<float>(), bpm(dq), H, Hkv, Sq, c, (float)scale, Sk, (int)q_offset);
  return {dq, dk, dv};
}

// ---------------------------------------------------------------- the same window, its keys split over n workgroups
// The kernels of attention_splitkv.hip: every query block's key range dealt to n workgroups, whose fp32
// partials a second kernel merges in split order.  The workspace is the caching allocator's, per call, and
// is not cleared: the merges read no partial that was not written.
void check_splits(const at::Tensor& q, int64_t n) {
  TORCH_CHECK(n >= 1 && n <= gtk_splitkv::kMaxSplits, "attention: kv_splits must be between 1 and ", gtk_splitkv::kMaxSplits,
              ", got ", n);
  TORCH_CHECK(q.size(0) * q.size(1) * q.size(2) < (int64_t(1) << 31), "attention: kv_splits needs B * H * Sq below 2^31");
}

// -> (o [B, Sq, H, 128], lse2 [B, H, Sq]), as attn_fwd_qoff
std::vector<at::Tensor> attn_fwd_qoff_split(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, double scale,
                                            int64_t q_offset, int64_t n) {
  check_qkv_qoff(q, k, v, q_offset);
  check_scale(scale);
  check_splits(q, n);
  const int B = q.size(0), H = q.size(1), Sq = q.size(2), Hkv = k.size(1), Sk = k.size(2);
  auto fopt = q.options().dtype(at::kFloat);
  auto o = at::empty({B, Sq, H, D}, q.options());
  auto lse = at::empty({B, H, Sq}, fopt);
  auto o_part = at::empty({n, B, Sq, H, D}, fopt), lse_part = at::empty({n, B, H, Sq}, fopt);
  gtk_splitkv::launch_fwd(dim3(B * H, Sq / BQ, (unsigned)n), cur_stream(), bp(q), bp(k), bp(v), o_part.data_ptr<float>(),
                          lse_part.data_ptr<float>(), H, Hkv, Sq, (float)(scale * 1.4426950408889634), Sk, (int)q_offset);
  gtk_splitkv::launch_combine(cur_stream(), o_part.data_ptr<float>(), lse_part.data_ptr<float>(), bpm(o), lse.data_ptr<float>(),
                              B, H, Sq, (int)n);
  return {o, lse};
}

// -> (dq, dk, dv) as attn_bwd_qoff: its pre-kernel and its dK/dV kernel, dQ from n splits and their sum
std::vector<at::Tensor> attn_bwd_qoff_split(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k,
                                            const at::Tensor& v, const at::Tensor& out, const at::Tensor& lse, double scale,
                                            int64_t q_offset, int64_t n) {
  check_qkv_qoff(q, k, v, q_offset);
  check_scale(scale);
  check_splits(q, n);
  const int B = q.size(0), H = q.size(1), Sq = q.size(2), Hkv = k.size(1), Sk = k.size(2);
  check_bwd_qoff(dout, q, out, lse);
  auto fopt = q.options().dtype(at::kFloat);
  auto delta = at::empty({B, H, Sq}, fopt), nls = at::empty({B, H, Sq}, fopt), ndl = at::empty({B, H, Sq}, fopt);
  auto dq = at::empty_like(q), dk = at::empty_like(k), dv = at::empty_like(v);
  auto dq_part = at::empty({n, B, H, Sq, D}, fopt);
  const int rows = B * Sq * H;
  const float c = (float)(scale * 1.4426950408889634);
  hipLaunchKernelGGL(attn_bwd_pre_kernel, dim3((rows + 15) / 16), dim3(256), 0, cur_stream(), bp(dout), bp(out),
                     lse.data_ptr<float>(), delta.data_ptr<float>(), nls.data_ptr<float>(), ndl.data_ptr<float>(), B, H, Sq,
                     1.f / c);
  gtk_qoff::launch_dkdv(dim3(B * Hkv, Sk / KB), cur_stream(), bp(q), bp(k), bp(v), bp(dout), nls.data_ptr<float>(),
                        ndl.data_ptr<float>(), bpm(dk), bpm(dv), H, Hkv, Sq, c, (float)scale, Sk, (int)q_offset);
  gtk_splitkv::launch_dq(dim3(B * H, Sq / BQ, (unsigned)n), cur_stream(), bp(q), bp(k), bp(v), bp(dout), lse.data_ptr<float>(),
                         delta.data_ptr<float>(), dq_part.data_ptr<float>(), H, Hkv, Sq, c, Sk, (int)q_offset);
  gtk_splitkv::launch_dq_reduce(cur_stream(), dq_part.data_ptr<float>(), bpm(dq), B, H, Sq, (float)scale, (int)q_offset, (int)n);
  return {dq, dk, dv};
}

// ---------------------------------------------------------------- a decode step over a ragged KV cache
// q [B, H, Sq, 128], Sq * (H / Hkv) <= 32 new tokens' queries; k_cache, v_cache [B, Hkv, Smax, 128]; kv_len int32 [B]
// on the device, the valid keys of each sequence with the Sq new tokens appended.  Query i of sequence b sees
// key j iff j <= kv_len[b] - Sq + i.  The kernel of attention_decode.hip clamps kv_len into [Sq, Smax]; nothing
// here reads it.  n key splits per (sequence, KV head), merged by the split-KV combine when n > 1.
// -> (o [B, Sq, H, 128], lse2 [B, H, Sq])
std::vector<at::Tensor> attn_decode(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                                    const at::Tensor& kv_len, double scale, int64_t n) {
  for (const at::Tensor* x : {&q, &k_cache, &v_cache})
    TORCH_CHECK(x->is_cuda() && x->scalar_type() == at::kBFloat16 && x->is_contiguous() && x->dim() == 4,
                "attention decode: q and the caches must be contiguous bf16 [B, heads, S, D] GPU tensors");
  TORCH_CHECK(q.size(3) == D && k_cache.size(3) == D && v_cache.size(3) == D, "attention decode: head dim must be 128, got ",
              q.size(3));
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes() && q.size(0) == k_cache.size(0),
              "attention decode: shape mismatch (k_cache and v_cache alike, one batch size)");
  TORCH_CHECK(k_cache.device() == q.device() && v_cache.device() == q.device(), "attention decode: q and the caches must be on one device");
  const int64_t B = q.size(0), H = q.size(1), Sq = q.size(2), Hkv = k_cache.size(1), Smax = k_cache.size(2);
  TORCH_CHECK(B > 0 && Hkv > 0 && H % Hkv == 0, "attention decode: q heads must be a multiple of kv heads");
  TORCH_CHECK(Sq >= 1 && Sq * (H / Hkv) <= gtk_decode::kMaxRows, "attention decode: Sq * (H / Hkv) must be between 1 and ",
              gtk_decode::kMaxRows, ", got ", Sq * (H / Hkv));
  TORCH_CHECK(Smax >= Sq, "attention decode: the cache length ", Smax, " is below the query length ", Sq);
  TORCH_CHECK(Smax * D * 2 < (int64_t(1) << 31), "attention decode: one head's cache bytes must fit the 32-bit buffer offsets");
  TORCH_CHECK(B * H * Sq < (int64_t(1) << 31) && B * Hkv < (int64_t(1) << 31), "attention decode: B * H * Sq must be below 2^31");
  TORCH_CHECK(kv_len.is_cuda() && kv_len.device() == q.device() && kv_len.scalar_type() == at::kInt && kv_len.is_contiguous() &&
                  kv_len.dim() == 1 && kv_len.size(0) == B,
              "attention decode: kv_len must be a contiguous int32 [B] GPU tensor on q's device");
  check_scale(scale);
  TORCH_CHECK(n >= 1 && n <= gtk_decode::kMaxSplits, "attention decode: kv_splits must be between 1 and ", gtk_decode::kMaxSplits,
              ", got ", n);
  auto fopt = q.options().dtype(at::kFloat);
  auto o = at::empty({B, Sq, H, D}, q.options());
  auto lse = at::empty({B, H, Sq}, fopt);
  at::Tensor o_part, lse_part;
  if (n > 1) o_part = at::empty({n, B, Sq, H, D}, fopt), lse_part = at::empty({n, B, H, Sq}, fopt);
  gtk_decode::launch(cur_stream(), bp(q), bp(k_cache), bp(v_cache), kv_len.data_ptr<int>(), bpm(o), lse.data_ptr<float>(),
                     n > 1 ? o_part.data_ptr<float>() : nullptr, n > 1 ? lse_part.data_ptr<float>() : nullptr, (int)B, (int)H,
                     (int)Hkv, (int)Sq, (int)Smax, (float)(scale * 1.4426950408889634), (int)n);
  if (n > 1)
    gtk_splitkv::launch_combine(cur_stream(), o_part.data_ptr<float>(), lse_part.data_ptr<float>(), bpm(o), lse.data_ptr<float>(),
                                (int)B, (int)H, (int)Sq, (int)n);
  return {o, lse};
}

// ---------------------------------------------------------------- a decode step over a paged KV cache
// what the two paged calls share: the pools [num_pages, Hkv, page_size, 128], the table [B, max_pages], kv_len [B]
// the pages' geometry, the table and the lengths: k_pool is the bf16 pool or the pool of codes
static void check_pages(const char* who, const at::Tensor& x, const at::Tensor& k_pool, const at::Tensor& block_table,
                        const at::Tensor& kv_len) {
  const int64_t B = x.size(0), P = k_pool.size(2);
  TORCH_CHECK(k_pool.size(0) > 0 && k_pool.size(0) < (int64_t(1) << 31), who, ": the pool must hold between 1 and 2^31 - 1 pages");
  TORCH_CHECK(P >= 64 && P <= 1024 && P % 64 == 0, who, ": page_size must be a multiple of 64 from 64 to 1024, got ", P);
  TORCH_CHECK(block_table.is_cuda() && block_table.device() == x.device() && block_table.scalar_type() == at::kInt &&
                  block_table.is_contiguous() && block_table.dim() == 2 && block_table.size(0) == B && block_table.size(1) > 0,
              who, ": block_table must be a contiguous int32 [B, max_pages] GPU tensor on the pools' device");
  TORCH_CHECK(block_table.size(1) * P < (int64_t(1) << 31), who, ": max_pages * page_size must be below 2^31");
  TORCH_CHECK(kv_len.is_cuda() && kv_len.device() == x.device() && kv_len.scalar_type() == at::kInt && kv_len.is_contiguous() &&
                  kv_len.dim() == 1 && kv_len.size(0) == B,
              who, ": kv_len must be a contiguous int32 [B] GPU tensor on the pools' device");
}

static void check_paged(const char* who, const at::Tensor& x, const at::Tensor& k_pool, const at::Tensor& v_pool,
                        const at::Tensor& block_table, const at::Tensor& kv_len) {
  for (const at::Tensor* y : {&x, &k_pool, &v_pool})
    TORCH_CHECK(y->is_cuda() && y->scalar_type() == at::kBFloat16 && y->is_contiguous() && y->dim() == 4, who,
                ": the new rows and the pools must be contiguous bf16 4-d GPU tensors");
  TORCH_CHECK(x.size(3) == D && k_pool.size(3) == D && v_pool.size(3) == D, who, ": head dim must be 128, got ", x.size(3));
  TORCH_CHECK(k_pool.sizes() == v_pool.sizes(), who, ": shape mismatch (k_pool and v_pool alike)");
  TORCH_CHECK(k_pool.device() == x.device() && v_pool.device() == x.device(), who, ": all tensors must be on one device");
  check_pages(who, x, k_pool, block_table, kv_len);
}

// the fp8 cache: codes uint8 [num_pages, Hkv, page_size, 128] and exponent bytes uint8 [num_pages, Hkv, page_size]
static void check_paged_fp8(const char* who, const at::Tensor& x, const at::Tensor& k_codes, const at::Tensor& v_codes,
                            const at::Tensor& k_exp, const at::Tensor& v_exp, const at::Tensor& block_table,
                            const at::Tensor& kv_len) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous() && x.dim() == 4 && x.size(3) == D, who,
              ": q and the new rows must be contiguous bf16 [.., .., .., 128] GPU tensors");
  for (const at::Tensor* y : {&k_codes, &v_codes, &k_exp, &v_exp})
    TORCH_CHECK(y->is_cuda() && y->scalar_type() == at::kByte && y->is_contiguous() && y->device() == x.device(), who,
                ": the code and exponent pools must be contiguous uint8 GPU tensors on one device");
  TORCH_CHECK(k_codes.dim() == 4 && k_codes.size(3) == D && v_codes.sizes() == k_codes.sizes(), who,
              ": k_codes and v_codes must be [num_pages, Hkv, page_size, 128] alike");
  TORCH_CHECK(k_exp.dim() == 3 && k_exp.sizes() == k_codes.sizes().slice(0, 3) && v_exp.sizes() == k_exp.sizes(), who,
              ": k_exp and v_exp must be [num_pages, Hkv, page_size] of the code pools");
  check_pages(who, x, k_codes, block_table, kv_len);
}

// attn_decode over a cache of pages: q [B, H, Sq, 128]; k_pool, v_pool [num_pages, Hkv, page_size, 128]; block_table
// int32 [B, max_pages], entry [b, p] the pool page of keys p * page_size .. of sequence b; kv_len int32 [B].  The
// kernel clamps kv_len into [Sq, max_pages * page_size] and every page id into [0, num_pages); nothing here reads
// either.  -> (o [B, Sq, H, 128], lse2 [B, H, Sq]), bit for bit attn_decode's on the gathered slab at the same n
std::vector<at::Tensor> attn_decode_paged(const at::Tensor& q, const at::Tensor& k_pool, const at::Tensor& v_pool,
                                          const at::Tensor& block_table, const at::Tensor& kv_len, double scale, int64_t n) {
  check_paged("attention decode paged", q, k_pool, v_pool, block_table, kv_len);
  const int64_t B = q.size(0), H = q.size(1), Sq = q.size(2), Hkv = k_pool.size(1), P = k_pool.size(2), MP = block_table.size(1);
  TORCH_CHECK(B > 0 && Hkv > 0 && H % Hkv == 0, "attention decode paged: q heads must be a multiple of kv heads");
  TORCH_CHECK(Sq >= 1 && Sq * (H / Hkv) <= gtk_decode::kMaxRows, "attention decode paged: Sq * (H / Hkv) must be between 1 and ",
              gtk_decode::kMaxRows, ", got ", Sq * (H / Hkv));
  TORCH_CHECK(B * H * Sq < (int64_t(1) << 31) && B * Hkv < (int64_t(1) << 31), "attention decode paged: B * H * Sq must be below 2^31");
  check_scale(scale);
  TORCH_CHECK(n >= 1 && n <= gtk_decode::kMaxSplits, "attention decode paged: kv_splits must be between 1 and ",
              gtk_decode::kMaxSplits, ", got ", n);
  auto fopt = q.options().dtype(at::kFloat);
  auto o = at::empty({B, Sq, H, D}, q.options());
  auto lse = at::empty({B, H, Sq}, fopt);
  at::Tensor o_part, lse_part;
  if (n > 1) o_part = at::empty({n, B, Sq, H, D}, fopt), lse_part = at::empty({n, B, H, Sq}, fopt);
  gtk_decode::launch_paged(cur_stream(), bp(q), bp(k_pool), bp(v_pool), block_table.data_ptr<int>(), kv_len.data_ptr<int>(), bpm(o),
                           lse.data_ptr<float>(), n > 1 ? o_part.data_ptr<float>() : nullptr,
                           n > 1 ? lse_part.data_ptr<float>() : nullptr, (int)B, (int)H, (int)Hkv, (int)Sq, (int)P, (int)MP,
                           (int)k_pool.size(0), (float)(scale * 1.4426950408889634), (int)n);
  if (n > 1)
    gtk_splitkv::launch_combine(cur_stream(), o_part.data_ptr<float>(), lse_part.data_ptr<float>(), bpm(o), lse.data_ptr<float>(),
                                (int)B, (int)H, (int)Sq, (int)n);
  return {o, lse};
}

// the Sq new tokens' rows k_new, v_new [B, Hkv, Sq, 128] into the pages, in place: row i of sequence b at position
// kv_len[b] - Sq + i, kv_len counting the new tokens.  A sequence with kv_len outside [Sq, max_pages * page_size]
// and a row whose page id is outside [0, num_pages) are skipped by the kernel
void kv_append_paged(const at::Tensor& k_new, const at::Tensor& v_new, at::Tensor& k_pool, at::Tensor& v_pool,
                     const at::Tensor& block_table, const at::Tensor& kv_len) {
  check_paged("kv append paged", k_new, k_pool, v_pool, block_table, kv_len);
  TORCH_CHECK(v_new.is_cuda() && v_new.scalar_type() == at::kBFloat16 && v_new.is_contiguous() && v_new.sizes() == k_new.sizes() &&
                  v_new.device() == k_new.device(),
              "kv append paged: k_new and v_new must be contiguous bf16 GPU tensors of one shape on one device");
  const int64_t B = k_new.size(0), Hkv = k_new.size(1), Sq = k_new.size(2);
  TORCH_CHECK(B > 0 && Hkv == k_pool.size(1), "kv append paged: the new rows and the pools must have the same KV heads");
  TORCH_CHECK(Sq >= 1 && Sq <= gtk_decode::kMaxAppend, "kv append paged: Sq must be between 1 and ", gtk_decode::kMaxAppend,
              ", got ", Sq);
  TORCH_CHECK(B * Hkv * Sq < (int64_t(1) << 31), "kv append paged: B * Hkv * Sq must be below 2^31");
  gtk_decode::launch_append(cur_stream(), bp(k_new), bp(v_new), bpm(k_pool), bpm(v_pool), block_table.data_ptr<int>(),
                            kv_len.data_ptr<int>(), (int)B, (int)Hkv, (int)Sq, (int)k_pool.size(2), (int)block_table.size(1),
                            (int)k_pool.size(0));
}

// ---------------------------------------------------------------- prefill over a paged KV cache
// what the two chunk calls add to check_paged: q_len, and a padded chunk no longer than the table can hold
static void check_chunk(const char* who, const at::Tensor& x, const at::Tensor& k_pool, const at::Tensor& block_table,
                        const at::Tensor& q_len) {
  TORCH_CHECK(q_len.is_cuda() && q_len.device() == x.device() && q_len.scalar_type() == at::kInt && q_len.is_contiguous() &&
                  q_len.dim() == 1 && q_len.size(0) == x.size(0),
              who, ": q_len must be a contiguous int32 [B] GPU tensor on the pools' device");
  TORCH_CHECK(x.size(0) > 0 && x.size(2) >= 1 && x.size(2) <= block_table.size(1) * k_pool.size(2), who,
              ": Sq must be between 1 and max_pages * page_size, got ", x.size(2));
}

// q [B, H, Sq, 128], any Sq, the batch padded to Sq rows of which q_len[b] are real; pools, table and kv_len as in
// attn_decode_paged.  Row i < q_len[b] sits at kv_len[b] - q_len[b] + i; rows past q_len[b] give o = 0, lse2 = -inf.
// The kernel clamps q_len, kv_len and every page id; nothing here reads them.  -> (o [B, Sq, H, 128], lse2 [B, H, Sq])
std::vector<at::Tensor> attn_prefill_paged(const at::Tensor& q, const at::Tensor& k_pool, const at::Tensor& v_pool,
                                           const at::Tensor& block_table, const at::Tensor& kv_len, const at::Tensor& q_len,
                                           double scale) {
  check_paged("attention prefill paged", q, k_pool, v_pool, block_table, kv_len);
  check_chunk("attention prefill paged", q, k_pool, block_table, q_len);
  const int64_t B = q.size(0), H = q.size(1), Sq = q.size(2), Hkv = k_pool.size(1), P = k_pool.size(2), MP = block_table.size(1);
  TORCH_CHECK(Hkv > 0 && H > 0 && H % Hkv == 0, "attention prefill paged: q heads must be a multiple of kv heads");
  TORCH_CHECK(B * H * Sq < (int64_t(1) << 31), "attention prefill paged: B * H * Sq must be below 2^31");
  check_scale(scale);
  auto o = at::empty({B, Sq, H, D}, q.options());
  auto lse = at::empty({B, H, Sq}, q.options().dtype(at::kFloat));
  gtk_decode::launch_prefill_paged(cur_stream(), bp(q), bp(k_pool), bp(v_pool), block_table.data_ptr<int>(), kv_len.data_ptr<int>(),
                                   q_len.data_ptr<int>(), bpm(o), lse.data_ptr<float>(), (int)B, (int)H, (int)Hkv, (int)Sq, (int)P,
                                   (int)MP, (int)k_pool.size(0), (float)(scale * 1.4426950408889634));
  return {o, lse};
}

// the chunk's rows k_new, v_new [B, Hkv, Sq, 128] into the pages, in place: row i < q_len[b] of sequence b at position
// kv_len[b] - q_len[b] + i.  The kernel skips a sequence with kv_len outside [q_len, max_pages * page_size] and a row
// whose page id is outside [0, num_pages)
void kv_append_paged_chunk(const at::Tensor& k_new, const at::Tensor& v_new, at::Tensor& k_pool, at::Tensor& v_pool,
                           const at::Tensor& block_table, const at::Tensor& kv_len, const at::Tensor& q_len) {
  check_paged("kv append paged chunk", k_new, k_pool, v_pool, block_table, kv_len);
  check_chunk("kv append paged chunk", k_new, k_pool, block_table, q_len);
  TORCH_CHECK(v_new.is_cuda() && v_new.scalar_type() == at::kBFloat16 && v_new.is_contiguous() && v_new.sizes() == k_new.sizes() &&
                  v_new.device() == k_new.device(),
              "kv append paged chunk: k_new and v_new must be contiguous bf16 GPU tensors of one shape on one device");
  const int64_t B = k_new.size(0), Hkv = k_new.size(1), Sq = k_new.size(2);
  TORCH_CHECK(Hkv == k_pool.size(1), "kv append paged chunk: the new rows and the pools must have the same KV heads");
  TORCH_CHECK(B * Hkv * Sq < (int64_t(1) << 31), "kv append paged chunk: B * Hkv * Sq must be below 2^31");
  gtk_decode::launch_append_chunk(cur_stream(), bp(k_new), bp(v_new), bpm(k_pool), bpm(v_pool), block_table.data_ptr<int>(),
                                  kv_len.data_ptr<int>(), q_len.data_ptr<int>(), (int)B, (int)Hkv, (int)Sq, (int)k_pool.size(2),
                                  (int)block_table.size(1), (int)k_pool.size(0));
}

// attn_decode_paged over the fp8 cache -> (o, lse2), bit for bit attn_decode_paged's on the dequantised pools at the same n
std::vector<at::Tensor> attn_decode_paged_fp8(const at::Tensor& q, const at::Tensor& k_codes, const at::Tensor& v_codes,
                                              const at::Tensor& k_exp, const at::Tensor& v_exp, const at::Tensor& block_table,
                                              const at::Tensor& kv_len, double scale, int64_t n) {
  check_paged_fp8("attention decode paged fp8", q, k_codes, v_codes, k_exp, v_exp, block_table, kv_len);
  const int64_t B = q.size(0), H = q.size(1), Sq = q.size(2), Hkv = k_codes.size(1), P = k_codes.size(2), MP = block_table.size(1);
  TORCH_CHECK(B > 0 && Hkv > 0 && H % Hkv == 0, "attention decode paged fp8: q heads must be a multiple of kv heads");
  TORCH_CHECK(Sq >= 1 && Sq * (H / Hkv) <= gtk_decode::kMaxRows, "attention decode paged fp8: Sq * (H / Hkv) must be between 1 and ",
              gtk_decode::kMaxRows, ", got ", Sq * (H / Hkv));
  TORCH_CHECK(B * H * Sq < (int64_t(1) << 31) && B * Hkv < (int64_t(1) << 31), "attention decode paged fp8: B * H * Sq must be below 2^31");
  check_scale(scale);
  TORCH_CHECK(n >= 1 && n <= gtk_decode::kMaxSplits, "attention decode paged fp8: kv_splits must be between 1 and ",
              gtk_decode::kMaxSplits, ", got ", n);
  auto fopt = q.options().dtype(at::kFloat);
  auto o = at::empty({B, Sq, H, D}, q.options());
  auto lse = at::empty({B, H, Sq}, fopt);
  at::Tensor o_part, lse_part;
  if (n > 1) o_part = at::empty({n, B, Sq, H, D}, fopt), lse_part = at::empty({n, B, H, Sq}, fopt);
  gtk_decode::launch_paged_fp8(cur_stream(), bp(q), k_codes.data_ptr<uint8_t>(), v_codes.data_ptr<uint8_t>(), k_exp.data_ptr<uint8_t>(),
                               v_exp.data_ptr<uint8_t>(), block_table.data_ptr<int>(), kv_len.data_ptr<int>(), bpm(o),
                               lse.data_ptr<float>(), n > 1 ? o_part.data_ptr<float>() : nullptr,
                               n > 1 ? lse_part.data_ptr<float>() : nullptr, (int)B, (int)H, (int)Hkv, (int)Sq, (int)P, (int)MP,
                               (int)k_codes.size(0), (float)(scale * 1.4426950408889634), (int)n);
  if (n > 1)
    gtk_splitkv::launch_combine(cur_stream(), o_part.data_ptr<float>(), lse_part.data_ptr<float>(), bpm(o), lse.data_ptr<float>(),
                                (int)B, (int)H, (int)Sq, (int)n);
  return {o, lse};
}

// kv_append_paged into the fp8 cache: every new row is quantised by the row rule on its way in
void kv_append_paged_fp8(const at::Tensor& k_new, const at::Tensor& v_new, at::Tensor& k_codes, at::Tensor& v_codes, at::Tensor& k_exp,
                         at::Tensor& v_exp, const at::Tensor& block_table, const at::Tensor& kv_len) {
  check_paged_fp8("kv append paged fp8", k_new, k_codes, v_codes, k_exp, v_exp, block_table, kv_len);
  TORCH_CHECK(v_new.is_cuda() && v_new.scalar_type() == at::kBFloat16 && v_new.is_contiguous() && v_new.sizes() == k_new.sizes() &&
                  v_new.device() == k_new.device(),
              "kv append paged fp8: k_new and v_new must be contiguous bf16 GPU tensors of one shape on one device");
  const int64_t B = k_new.size(0), Hkv = k_new.size(1), Sq = k_new.size(2);
  TORCH_CHECK(B > 0 && Hkv == k_codes.size(1), "kv append paged fp8: the new rows and the pools must have the same KV heads");
  TORCH_CHECK(Sq >= 1 && Sq <= gtk_decode::kMaxAppend, "kv append paged fp8: Sq must be between 1 and ", gtk_decode::kMaxAppend,
              ", got ", Sq);
  TORCH_CHECK(B * Hkv * Sq < (int64_t(1) << 31), "kv append paged fp8: B * Hkv * Sq must be below 2^31");
  gtk_decode::launch_append_fp8(cur_stream(), bp(k_new), bp(v_new), k_codes.data_ptr<uint8_t>(), v_codes.data_ptr<uint8_t>(),
                                k_exp.data_ptr<uint8_t>(), v_exp.data_ptr<uint8_t>(), block_table.data_ptr<int>(),
                                kv_len.data_ptr<int>(), (int)B, (int)Hkv, (int)Sq, (int)k_codes.size(2), (int)block_table.size(1),
                                (int)k_codes.size(0));
}

// attn_prefill_paged over the fp8 cache -> (o, lse2), bit for bit attn_prefill_paged's on the dequantised pools
std::vector<at::Tensor> attn_prefill_paged_fp8(const at::Tensor& q, const at::Tensor& k_codes, const at::Tensor& v_codes,
                                               const at::Tensor& k_exp, const at::Tensor& v_exp, const at::Tensor& block_table,
                                               const at::Tensor& kv_len, const at::Tensor& q_len, double scale) {
  check_paged_fp8("attention prefill paged fp8", q, k_codes, v_codes, k_exp, v_exp, block_table, kv_len);
  check_chunk("attention prefill paged fp8", q, k_codes, block_table, q_len);
  const int64_t B = q.size(0), H = q.size(1), Sq = q.size(2), Hkv = k_codes.size(1), P = k_codes.size(2), MP = block_table.size(1);
  TORCH_CHECK(Hkv > 0 && H > 0 && H % Hkv == 0, "attention prefill paged fp8: q heads must be a multiple of kv heads");
  TORCH_CHECK(B * H * Sq < (int64_t(1) << 31), "attention prefill paged fp8: B * H * Sq must be below 2^31");
  check_scale(scale);
  auto o = at::empty({B, Sq, H, D}, q.options());
  auto lse = at::empty({B, H, Sq}, q.options().dtype(at::kFloat));
  gtk_decode::launch_prefill_paged_fp8(cur_stream(), bp(q), k_codes.data_ptr<uint8_t>(), v_codes.data_ptr<uint8_t>(),
                                       k_exp.data_ptr<uint8_t>(), v_exp.data_ptr<uint8_t>(), block_table.data_ptr<int>(),
                                       kv_len.data_ptr<int>(), q_len.data_ptr<int>(), bpm(o), lse.data_ptr<float>(), (int)B, (int)H,
                                       (int)Hkv, (int)Sq, (int)P, (int)MP, (int)k_codes.size(0), (float)(scale * 1.4426950408889634));
  return {o, lse};
}

// kv_append_paged_chunk into the fp8 cache: every row i < q_len[b] is quantised by the row rule on its way in
void kv_append_paged_chunk_fp8(const at::Tensor& k_new, const at::Tensor& v_new, at::Tensor& k_codes, at::Tensor& v_codes,
                               at::Tensor& k_exp, at::Tensor& v_exp, const at::Tensor& block_table, const at::Tensor& kv_len,
                               const at::Tensor& q_len) {
  check_paged_fp8("kv append paged chunk fp8", k_new, k_codes, v_codes, k_exp, v_exp, block_table, kv_len);
  check_chunk("kv append paged chunk fp8", k_new, k_codes, block_table, q_len);
  TORCH_CHECK(v_new.is_cuda() && v_new.scalar_type() == at::kBFloat16 && v_new.is_contiguous() && v_new.sizes() == k_new.sizes() &&
                  v_new.device() == k_new.device(),
              "kv append paged chunk fp8: k_new and v_new must be contiguous bf16 GPU tensors of one shape on one device");
  const int64_t B = k_new.size(0), Hkv = k_new.size(1), Sq = k_new.size(2);
  TORCH_CHECK(Hkv == k_codes.size(1), "kv append paged chunk fp8: the new rows and the pools must have the same KV heads");
  TORCH_CHECK(B * Hkv * Sq < (int64_t(1) << 31), "kv append paged chunk fp8: B * Hkv * Sq must be below 2^31");
  gtk_decode::launch_append_chunk_fp8(cur_stream(), bp(k_new), bp(v_new), k_codes.data_ptr<uint8_t>(), v_codes.data_ptr<uint8_t>(),
                                      k_exp.data_ptr<uint8_t>(), v_exp.data_ptr<uint8_t>(), block_table.data_ptr<int>(),
                                      kv_len.data_ptr<int>(), q_len.data_ptr<int>(), (int)B, (int)Hkv, (int)Sq, (int)k_codes.size(2),
                                      (int)block_table.size(1), (int)k_codes.size(0));
}

// the document-masked backward, from the outputs of attn_fwd_doc
std::vector<at::Tensor> attn_bwd_doc(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                                     const at::Tensor& out, const at::Tensor& lse, double scale, const at::Tensor& doc_start,
                                     const at::Tensor& doc_end) {
  return attn_bwd_impl(dout, q, k, v, out, lse, scale, &doc_start, &doc_end);
}

}  // namespace gtk_attn
