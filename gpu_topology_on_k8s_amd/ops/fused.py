"""Autograd front-end of the fused HIP kernels (``csrc/ops/fused_ops.hip``) + PyTorch references.

GPU tensors always take the HIP path and fail loudly (``NativeUnavailable``) when the extension is
missing; CPU tensors take the reference path (used by the CPU test-suite and as the fp32 numerics
oracle of ``tests/test_fused_gpu.py``).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from .._native import load

__all__ = [
    "rmsnorm", "rmsnorm_ref", "rope_tables", "rope_split", "rope_split_ref", "swiglu", "swiglu_ref", "cross_entropy",
    "cross_entropy_ref", "hip", "attention", "attention_ref", "flash_attention_supported", "transpose", "swiglu_bwd_ref",
    "swiglu_bwd_t", "swiglu_fwd_t", "attention_t", "offer_t", "take_t", "clear_t", "doc_bounds", "doc_start_from_eos",
    "kv_splits_for", "attention_decode", "attention_decode_ref", "decode_splits_for",
    "attention_decode_paged", "attention_decode_paged_ref", "kv_cache_append", "kv_cache_append_ref",
    "kv_quantize_ref", "kv_dequantize_ref", "attention_decode_paged_fp8", "attention_decode_paged_fp8_ref",
    "kv_cache_append_fp8", "kv_cache_append_fp8_ref",
    "attention_prefill_paged", "attention_prefill_paged_ref", "kv_cache_append_prefill", "kv_cache_append_prefill_ref",
    "attention_prefill_paged_fp8", "attention_prefill_paged_fp8_ref", "kv_cache_append_prefill_fp8",
    "kv_cache_append_prefill_fp8_ref",
]


def hip():
    return load("_fused")


# ------------------------------------------------------------------------------------ transpose
def transpose(x: torch.Tensor) -> torch.Tensor:
    """Contiguous ``x.t()``: the LDS-tiled HIP kernel for bf16 GPU matrices whose dims are multiples of
    64 (every Llama-3 dim), torch's copy otherwise.  Puts backward-GEMM operands into the NT layout."""
    if x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2 and x.size(0) % 64 == 0 and x.size(1) % 64 == 0:
        return hip().transpose_bf16(x.contiguous())
    return x.t().contiguous()


# ----------------------------------------------------------------- transposed gradients, handed on
# A backward kernel that already holds a gradient tile in LDS can write the gradient's transpose too
# (xent_bwd_t: dlogits^T), which the consumer's NT-layout weight-gradient GEMM needs.  Autograd passes
# only the gradient itself between nodes, so the producer offers the transpose here, keyed by the
# gradient's storage, shape and version, and the consuming linear layer takes it (models/llama.py
# _FlatLinear).  The entry holds the gradient alive, so its address cannot be reused while the entry
# exists; a gradient that autograd summed or copied on the way has another address and simply finds
# nothing (the consumer transposes it itself).  Llama.forward clears leftovers.
_PENDING_T: Dict[Tuple[int, Tuple[int, ...]], Tuple[torch.Tensor, torch.Tensor, int]] = {}


def offer_t(g: torch.Tensor, g_t: torch.Tensor) -> None:
    _PENDING_T[(g.data_ptr(), tuple(g.shape))] = (g, g_t, g._version)


def take_t(g: torch.Tensor) -> Optional[torch.Tensor]:
    """The transpose a producer offered for exactly this gradient (same storage, shape, version), or None."""
    if not _PENDING_T:
        return None
    e = _PENDING_T.pop((g.data_ptr(), tuple(g.shape)), None)
    if e is None or e[2] != g._version or e[0].stride() != g.stride():
        return None
    return e[1]


def clear_t() -> None:
    _PENDING_T.clear()


# ------------------------------------------------------------------------------------ RMSNorm
def rmsnorm_ref(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()).to(x.dtype)


class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, eps):
        x = x.contiguous()
        y, rstd = hip().rmsnorm_fwd(x, w, float(eps))
        ctx.save_for_backward(x, w, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, rstd = ctx.saved_tensors
        dx, dw = hip().rmsnorm_bwd(dy.contiguous(), x, w, rstd)
        return dx, dw, None


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    if x.is_cuda:
        return _RMSNorm.apply(x, w, eps)
    return rmsnorm_ref(x, w, eps)


class _AddRMSNorm(torch.autograd.Function):
    """``h = x + r; y = rmsnorm(h) * w`` as one node: the residual add lives in the norm kernel
    (forward) and the residual-stream gradient is accumulated inside the norm's backward kernel."""

    @staticmethod
    def forward(ctx, x, r, w, eps):
        h, y, rstd = hip().add_rmsnorm_fwd(x.contiguous(), r.contiguous(), w, float(eps))
        ctx.save_for_backward(h, w, rstd)
        return h, y

    @staticmethod
    def backward(ctx, dh, dy):
        h, w, rstd = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(h)
        if dh is None:
            dx, dw = hip().rmsnorm_bwd(dy.contiguous(), h, w, rstd)
        else:
            dx, dw = hip().add_rmsnorm_bwd(dy.contiguous(), h, w, rstd, dh.contiguous())
        return dx, dx, dw, None


def add_rmsnorm_ref(x: torch.Tensor, r: torch.Tensor, w: torch.Tensor, eps: float):
    h = x + r
    return h, rmsnorm_ref(h, w, eps)


def add_rmsnorm(x: torch.Tensor, r: torch.Tensor, w: torch.Tensor, eps: float = 1e-5):
    """``(h, y)`` with ``h = x + r`` (the new residual stream) and ``y = rmsnorm(h) * w``."""
    if x.is_cuda:
        return _AddRMSNorm.apply(x, r, w, eps)
    return add_rmsnorm_ref(x, r, w, eps)


# ------------------------------------------------------------------------------------ RoPE
def rope_tables(seq: int, head_dim: int, theta: float = 500000.0, device=None,
                scaling: dict | None = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 cos/sin tables [seq, head_dim/2] (Llama-3 RoPE; optional llama3 frequency scaling)."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if scaling:  # Llama-3.1 style long-context scaling
        factor, lo, hi, orig = scaling["factor"], scaling["low_freq_factor"], scaling["high_freq_factor"], scaling["original_max_position_embeddings"]
        wavelen = 2 * torch.pi / inv
        smooth = ((orig / wavelen) - lo) / (hi - lo)
        scaled = torch.where(wavelen > orig / lo, inv / factor, inv)
        mid = (wavelen <= orig / lo) & (wavelen >= orig / hi)
        inv = torch.where(mid, (1 - smooth) * inv / factor + smooth * inv, scaled)
    t = torch.arange(seq, dtype=torch.float64)
    f = torch.outer(t, inv)
    return f.cos().float().to(device), f.sin().float().to(device)


def rope_split_ref(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, B: int, S: int, H: int, Hkv: int, Dh: int,
                   pos_offset: int = 0):
    x = qkv.view(B, S, H + 2 * Hkv, Dh).float()
    c = cos[pos_offset:pos_offset + S].view(1, S, 1, Dh // 2)
    s = sin[pos_offset:pos_offset + S].view(1, S, 1, Dh // 2)

    def rot(t):
        a, b = t[..., : Dh // 2], t[..., Dh // 2:]
        return torch.cat([a * c - b * s, b * c + a * s], dim=-1)

    q = rot(x[:, :, :H]).to(qkv.dtype).transpose(1, 2).contiguous()
    k = rot(x[:, :, H:H + Hkv]).to(qkv.dtype).transpose(1, 2).contiguous()
    v = x[:, :, H + Hkv:].to(qkv.dtype).transpose(1, 2).contiguous()
    return q, k, v


class _RopeSplit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cos, sin, B, S, H, Hkv, Dh, pos_offset, want_t=False):
        q, k, v = hip().rope_split_fwd(qkv.contiguous(), cos, sin, B, S, H, Hkv, Dh, pos_offset)
        ctx.save_for_backward(cos, sin)
        ctx.meta = (pos_offset, qkv.shape)
        # backward also writes dqkv^T for the QKV weight gradient (rope_split_bwd_t, offered via offer_t)
        ctx.want_t = bool(want_t) and Dh == 128 and S % 64 == 0 and B * S // 64 <= 65535
        return q, k, v

    @staticmethod
    def backward(ctx, dq, dk, dv):
        cos, sin = ctx.saved_tensors
        pos_offset, shape = ctx.meta
        if ctx.want_t:
            dqkv, dqkv_t = hip().rope_split_bwd_t(dq.contiguous(), dk.contiguous(), dv.contiguous(), cos, sin, pos_offset)
            out = dqkv.view(shape)
            offer_t(out, dqkv_t)
            return out, None, None, None, None, None, None, None, None, None
        dqkv = hip().rope_split_bwd(dq.contiguous(), dk.contiguous(), dv.contiguous(), cos, sin, pos_offset)
        return dqkv.view(shape), None, None, None, None, None, None, None, None, None


def rope_split(qkv, cos, sin, B, S, H, Hkv, Dh, pos_offset: int = 0, want_t: bool = False):
    """Fused QKV split + RoPE: [B*S, (H+2Hkv)*Dh] -> q [B,H,S,Dh], k/v [B,Hkv,S,Dh].  ``want_t``: the
    backward offers dqkv^T to the QKV projection's weight gradient (:func:`offer_t`)."""
    if qkv.is_cuda:
        return _RopeSplit.apply(qkv, cos, sin, B, S, H, Hkv, Dh, pos_offset, want_t)
    return rope_split_ref(qkv, cos, sin, B, S, H, Hkv, Dh, pos_offset)


# ------------------------------------------------------------------------------------ SwiGLU
def swiglu_ref(gu: torch.Tensor) -> torch.Tensor:
    g, u = gu.float().chunk(2, dim=-1)
    return (torch.nn.functional.silu(g) * u).to(gu.dtype)


def swiglu_bwd_ref(dh: torch.Tensor, gu: torch.Tensor) -> torch.Tensor:
    """d[gate | up] of ``silu(g) * u`` (fp32 math, ``gu``'s dtype out)."""
    g, u = gu.float().chunk(2, dim=-1)
    d = dh.float()
    sg = torch.sigmoid(g)
    return torch.cat([d * u * sg * (1 + g * (1 - sg)), d * g * sg], dim=-1).to(gu.dtype)


def swiglu_bwd_t(dh: torch.Tensor, gu: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """SwiGLU backward returning ``(dgu [T, 2F], dgu^T [2F, T])``: the HIP kernel writes the transposed
    copy from its LDS tile (T, F multiples of 64; the kernel picks its tile width); elsewhere the
    reference plus a transpose."""
    if gu.is_cuda and gu.dim() == 2 and gu.size(0) % 64 == 0 and (gu.size(1) // 2) % 64 == 0:
        return tuple(hip().swiglu_bwd_t(dh.contiguous(), gu.contiguous()))
    dgu = hip().swiglu_bwd(dh.contiguous(), gu.contiguous()) if gu.is_cuda else swiglu_bwd_ref(dh, gu)
    return dgu, transpose(dgu)


def swiglu_fwd_t(gu: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """SwiGLU forward returning ``(h [T, F], h^T [F, T])`` (no autograd): the HIP kernel writes the
    transposed copy from its LDS tile; elsewhere the reference plus a transpose."""
    if gu.is_cuda and gu.dim() == 2 and gu.size(0) % 64 == 0 and (gu.size(1) // 2) % 64 == 0:
        return tuple(hip().swiglu_fwd_t(gu.contiguous()))
    h = hip().swiglu_fwd(gu.contiguous()) if gu.is_cuda else swiglu_ref(gu)
    return h, transpose(h)


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        gu = gu.contiguous()
        ctx.save_for_backward(gu)
        return hip().swiglu_fwd(gu)

    @staticmethod
    def backward(ctx, dh):
        (gu,) = ctx.saved_tensors
        return hip().swiglu_bwd(dh.contiguous(), gu)


def swiglu(gu: torch.Tensor) -> torch.Tensor:
    if gu.is_cuda:
        return _SwiGLU.apply(gu)
    return swiglu_ref(gu)


# ------------------------------------------------------------------------------------ loss
def cross_entropy_ref(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
    return torch.nn.functional.cross_entropy(logits.float().view(-1, logits.size(-1)), labels.view(-1), ignore_index=ignore_index)


class _CrossEntropy(torch.autograd.Function):
    """Mean token cross-entropy; backward overwrites the (no longer needed) bf16 logits with dlogits.
    ``want_t``: the backward kernel also writes dlogits^T and offers it (:func:`offer_t`) to the lm_head
    weight gradient (xent_bwd_t, T multiple of 64, V of 128)."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index, want_t=False):
        V = logits.size(-1)
        lg = logits.contiguous().view(-1, V)
        lb = labels.contiguous().view(-1)
        loss_rows, lse = hip().xent_fwd(lg, lb, int(ignore_index))
        nvalid = (lb != ignore_index).sum().clamp_min(1).float()
        ctx.lg, ctx.lb, ctx.lse, ctx.nvalid, ctx.ii, ctx.shape = lg, lb, lse, nvalid, int(ignore_index), logits.shape
        ctx.want_t = bool(want_t) and lg.size(0) % 64 == 0 and V % 128 == 0 and lg.size(0) // 64 <= 65535
        return loss_rows.sum() / nvalid

    @staticmethod
    def backward(ctx, g):
        scale = (g.float() / ctx.nvalid).reshape(1).contiguous()
        lg = ctx.lg
        ctx.lg = None
        if ctx.want_t:
            lg_t = hip().xent_bwd_t(lg, ctx.lb, ctx.lse, scale, ctx.ii)
            out = lg.view(ctx.shape)
            offer_t(out, lg_t)
            return out, None, None, None
        hip().xent_bwd_inplace(lg, ctx.lb, ctx.lse, scale, ctx.ii)
        return lg.view(ctx.shape), None, None, None


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100, want_t: bool = False) -> torch.Tensor:
    if logits.is_cuda:
        return _CrossEntropy.apply(logits, labels, ignore_index, want_t)
    return cross_entropy_ref(logits, labels, ignore_index)


# ------------------------------------------------------------------------------------ attention
def doc_start_from_eos(tokens: torch.Tensor, eos_id: int) -> torch.Tensor:
    """int32 ``doc_start`` [B, S] of a packed batch whose documents end with their EOS token: the token
    after an EOS starts a new document, token 0 starts the first."""
    S = tokens.size(-1)
    pos = torch.arange(S, device=tokens.device, dtype=torch.int32).expand_as(tokens)
    first = torch.ones_like(tokens, dtype=torch.bool)
    first[..., 1:] = tokens[..., :-1] == eos_id
    return torch.where(first, pos, torch.zeros_like(pos)).cummax(-1).values.to(torch.int32)


def doc_bounds(doc_start: torch.Tensor, check: bool = True):
    """``(doc_start, doc_end)`` as contiguous int32 [B, S] on ``doc_start``'s device: the document mask
    of a packed batch as the attention kernels read it.  ``doc_start[b, i]`` is the position of the first
    token of token i's document; query i sees key j iff ``doc_start[b, i] <= j <= i``, which from the
    key's side is ``j <= i < doc_end[b, j]``, one past the last token of j's document.  Computed once
    per batch; ``check`` (one sync) raises ``ValueError`` unless ``doc_start[b, i] <= i``, non-decreasing
    along i and constant inside a document (``doc_start[b, doc_start[b, i]] == doc_start[b, i]``)."""
    if doc_start.dim() != 2 or doc_start.dtype.is_floating_point or doc_start.dtype == torch.bool:
        raise ValueError("doc_bounds: doc_start must be an integer [B, S] tensor")
    ds = doc_start.to(torch.int64)
    B, S = ds.shape
    pos = torch.arange(S, device=ds.device).expand(B, S)
    if check:
        ok = (ds >= 0) & (ds <= pos)
        ok[:, 1:] &= ds[:, 1:] >= ds[:, :-1]
        ok &= ds.gather(1, ds.clamp(0, S - 1)) == ds  # a document's first token starts it: constant inside it
        if not bool(ok.all()):
            raise ValueError("doc_bounds: doc_start must satisfy doc_start[b, i] <= i, be non-decreasing and constant "
                             "inside a document")
    # the next document's start, per token: the smallest first-token position after i (S after the last)
    first = ds == pos
    nxt = torch.where(first, pos, torch.full_like(pos, S)).flip(1).cummin(1).values.flip(1)  # first start at or after i
    end = torch.cat([nxt[:, 1:], torch.full_like(pos[:, :1], S)], 1)
    return ds.to(torch.int32).contiguous(), end.to(torch.int32).contiguous()


def _check_q_offset(q: torch.Tensor, k: torch.Tensor, q_offset, doc) -> None:
    """The requirements of a query chunk at ``q_offset`` into longer K/V, refused before any launch."""
    if doc is not None:
        raise ValueError("attention: q_offset cannot be combined with doc")
    if q.size(-1) != 128:
        raise ValueError(f"attention: q_offset needs head dim 128, got {q.size(-1)}")
    Sq, Sk = q.size(2), k.size(2)
    if isinstance(q_offset, bool) or not isinstance(q_offset, int) or q_offset < 0 or q_offset % 128:
        raise ValueError(f"attention: q_offset must be a non-negative multiple of 128, got {q_offset!r}")
    if Sq == 0 or Sq % 128:
        raise ValueError(f"attention: query length must be a positive multiple of 128, got {Sq}")
    if Sk % 128:
        raise ValueError(f"attention: key length must be a multiple of 128, got {Sk}")
    if q_offset + Sq > Sk:
        raise ValueError(f"attention: q_offset + query length ({q_offset} + {Sq}) exceeds the key length {Sk}")


FWD_BLOCK_SLOTS = 512  # 256 CUs x the two workgroups per CU of the forward and dQ kernels
# The fewest 128-key blocks "auto" leaves each split of the call's largest query block.  Measured on an MI355X
# (bench/attn_splitkv_bench.py, B 1, 32 / 8 heads, Sk 8192, the 30 calls of 2, 4, 8 and 16 chunks, each against
# the unsplit call in the same process, two runs; profiles/attn_splitkv/SUMMARY.md): 9 is the smallest value at
# which no call gets an n > 1 that is slower than the unsplit call by more than the run-to-run spread (the
# largest of the 30 calls: forward 4.6 %, backward 3.0 %).  At 8 and below, Sq 1024 at q_offset 1024 gets n = 2
# with 8 key blocks a split and its forward takes 1.11 to 1.12 times the unsplit one; from 9 on every n > 1
# chosen is a gain (forward 0.51 to 0.98, backward 0.75 to 0.98 of the unsplit call).
MIN_KEY_BLOCKS_PER_SPLIT = 9


def kv_splits_for(B: int, H: int, Sq: int, Sk: int, q_offset: int) -> int:
    """The ``kv_splits`` that ``"auto"`` uses: the smallest n of 1, 2, 4, 8 with ``B * H * (Sq / 128) * n`` at
    least the chip's 512 forward block slots, but no larger than leaves every split of the largest query block
    (``(q_offset + Sq) / 128`` key blocks) ``MIN_KEY_BLOCKS_PER_SPLIT`` key blocks.  A function of the shapes
    alone (``Sk`` does not enter: keys past the window are never visited)."""
    blocks, kmax = B * H * (Sq // 128), (q_offset + Sq) // 128
    n = 1
    while n < 8 and blocks * n < FWD_BLOCK_SLOTS and kmax // (2 * n) >= MIN_KEY_BLOCKS_PER_SPLIT:
        n *= 2
    return n


def _check_kv_splits(q: torch.Tensor, k: torch.Tensor, kv_splits, q_offset, doc):
    """-> None (the unsplit kernels) or the int n of the split ones; refusals before any launch."""
    if kv_splits is None:
        return None
    if doc is not None:
        raise ValueError("attention: kv_splits cannot be combined with doc")
    if q_offset is None:
        raise ValueError("attention: kv_splits needs q_offset (the plain causal case is q_offset=0)")
    if q.size(-1) != 128:
        raise ValueError(f"attention: kv_splits needs head dim 128, got {q.size(-1)}")
    if kv_splits == "auto":
        _check_q_offset(q, k, q_offset, doc)
        n = kv_splits_for(q.size(0), q.size(1), q.size(2), k.size(2), q_offset)
        return n if n > 1 else None  # one split is the unsplit kernel, without the workspace round trip
    if isinstance(kv_splits, bool) or not isinstance(kv_splits, int) or not 1 <= kv_splits <= 16:
        raise ValueError(f"attention: kv_splits must be None, 'auto' or an int from 1 to 16, got {kv_splits!r}")
    return kv_splits


def attention_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float | None = None, doc=None,
                  q_offset: int | None = None) -> torch.Tensor:
    """fp32 causal GQA attention: q [B,H,S,D], k/v [B,Hkv,S,D] -> o [B,S,H,D] (same dtype as q).
    ``doc``: the pair of :func:`doc_bounds`; keys before ``doc_start[b, i]`` are masked too.
    ``q_offset``: q is a chunk of Sq queries at that position of the Sk >= Sq keys, k/v [B,Hkv,Sk,D]:
    query i sees key j iff ``j <= q_offset + i``."""
    if q_offset is not None:
        _check_q_offset(q, k, q_offset, doc)
        rep = q.size(1) // k.size(1)
        s = torch.matmul(q.float(), k.float().repeat_interleave(rep, dim=1).transpose(-1, -2))
        s = s * (scale if scale is not None else q.size(-1) ** -0.5)
        mask = torch.ones(q.size(2), k.size(2), dtype=torch.bool, device=q.device).triu(1 + q_offset)  # j > q_offset + i
        p = torch.softmax(s.masked_fill(mask, float("-inf")), dim=-1)
        return torch.matmul(p, v.float().repeat_interleave(rep, dim=1)).transpose(1, 2).to(q.dtype).contiguous()
    B, H, S, Dh = q.shape
    rep = H // k.size(1)
    kf = k.float().repeat_interleave(rep, dim=1)
    vf = v.float().repeat_interleave(rep, dim=1)
    sc = (scale if scale is not None else Dh ** -0.5)
    s = torch.matmul(q.float(), kf.transpose(-1, -2)) * sc
    mask = torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1)
    if doc is not None:
        mask = mask | (torch.arange(S, device=q.device).view(1, 1, 1, S) < doc[0].view(B, 1, S, 1))
    p = torch.softmax(s.masked_fill(mask, float("-inf")), dim=-1)
    return torch.matmul(p, vf).transpose(1, 2).to(q.dtype).contiguous()


class _FlashAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, with_t=False, doc=None, q_offset=None, kv_splits=None):
        ctx.set_materialize_grads(False)  # no zero-filled gradient for O^T (non-differentiable) in backward
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ctx.q_offset, ctx.kv_splits = q_offset, kv_splits
        if kv_splits is not None:  # the window with every query block's keys split over kv_splits workgroups
            o, lse = hip().attn_fwd_qoff_split(q, k, v, float(scale), q_offset, kv_splits)
            o_t = None
        elif q_offset is not None:  # a query chunk at an offset into longer K/V
            res = (hip().attn_fwd_t_qoff if with_t else hip().attn_fwd_qoff)(q, k, v, float(scale), q_offset)
            o, lse, o_t = res if with_t else (*res, None)
            if with_t:
                ctx.mark_non_differentiable(o_t)
        elif doc is not None:  # the document-masked kernels
            res = (hip().attn_fwd_t_doc if with_t else hip().attn_fwd_doc)(q, k, v, float(scale), doc[0], doc[1])
            o, lse, o_t = res if with_t else (*res, None)
            if with_t:
                ctx.mark_non_differentiable(o_t)
        elif with_t:  # the kernel also writes O^T [H*D, B*S] (the o-projection's NT-layout x^T)
            o, lse, o_t = hip().attn_fwd_t(q, k, v, float(scale))
            ctx.mark_non_differentiable(o_t)
        else:
            o, lse = hip().attn_fwd(q, k, v, float(scale))
            o_t = None
        ctx.save_for_backward(q, k, v, o, lse, *(doc or ()))
        ctx.scale = float(scale)
        return o, o_t

    @staticmethod
    def backward(ctx, do, _do_t=None):
        q, k, v, o, lse, *doc = ctx.saved_tensors
        if ctx.kv_splits is not None:
            dq, dk, dv = hip().attn_bwd_qoff_split(do.contiguous(), q, k, v, o, lse, ctx.scale, ctx.q_offset, ctx.kv_splits)
        elif ctx.q_offset is not None:
            dq, dk, dv = hip().attn_bwd_qoff(do.contiguous(), q, k, v, o, lse, ctx.scale, ctx.q_offset)
        elif doc:
            dq, dk, dv = hip().attn_bwd_doc(do.contiguous(), q, k, v, o, lse, ctx.scale, doc[0], doc[1])
        else:
            dq, dk, dv = hip().attn_bwd(do.contiguous(), q, k, v, o, lse, ctx.scale)
        return dq, dk, dv, None, None, None, None, None


def flash_attention_supported(q: torch.Tensor, k: torch.Tensor, d64: bool = False) -> bool:
    """Whether the HIP flash kernels serve q, k: head dim 128, and with ``d64`` head dim 64 as well (the
    kernels of csrc/ops/attention_d64.hip, which the model routes to only when asked: ``Llama(attn_d64=True)``).
    The query length is what is tested: with ``q_offset`` (head dim 128 only) the key length and the offset
    have requirements of their own, which :func:`attention` checks."""
    dims = (64, 128) if d64 else (128,)
    return q.is_cuda and q.dtype == torch.bfloat16 and q.size(-1) in dims and q.size(2) % 128 == 0 and q.size(1) % k.size(1) == 0


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float | None = None, doc=None,
              q_offset: int | None = None, kv_splits=None):
    """Causal GQA attention -> [B, S, H, D]; the HIP flash kernel on GPU (head dim 64 or 128, S % 128 == 0).
    ``doc``: the pair of :func:`doc_bounds` of a packed batch, no token attends across a document start.
    ``q_offset``: q [B, H, Sq, 128] is a chunk of queries at that position of the keys k/v [B, Hkv, Sk, 128]
    (a rank's chunk of a context-parallel sequence after the all-gather of K and V, or a prefill chunk against
    a KV cache); query i sees key j iff ``j <= q_offset + i``.  Sq, Sk and q_offset are multiples of 128 with
    ``0 <= q_offset`` and ``q_offset + Sq <= Sk``; not together with ``doc`` or head dim 64 (``ValueError``).
    The gradients of k and v are [B, Hkv, Sk, 128], zero for the keys no query sees.
    ``kv_splits`` (with ``q_offset`` only; on the CPU accepted and ignored): ``None`` is the kernels above, one
    workgroup per 128 queries walking all of their keys.  An int n from 1 to 16 deals every query block's keys
    to n workgroups and merges their fp32 partials in split order (csrc/ops/attention_splitkv.hip), forward and
    dQ alike; for a short chunk against long K/V, which alone does not fill the GPU.  ``"auto"`` takes
    :func:`kv_splits_for` of the shapes and, where that is 1, the unsplit kernels."""
    sc = scale if scale is not None else q.size(-1) ** -0.5
    n = _check_kv_splits(q, k, kv_splits, q_offset, doc)
    if q_offset is not None:
        _check_q_offset(q, k, q_offset, doc)
    if q.is_cuda:
        if not flash_attention_supported(q, k, d64=True):
            raise ValueError("HIP flash attention needs bf16, head dim 64 or 128 and S % 128 == 0")
        return _FlashAttention.apply(q, k, v, sc, False, doc, q_offset, n)[0]
    return attention_ref(q, k, v, sc, doc, q_offset)


def attention_t(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float | None = None, doc=None,
                q_offset: int | None = None, kv_splits=None):
    """``(o [B, S, H, D], o^T [H*D, B*S])``: on GPU the forward kernel writes the transposed copy from
    its LDS tile (no gradient flows through it); elsewhere the reference plus a transpose.  ``q_offset`` as
    in :func:`attention` (S is then the query length Sq).  The split kernels write no O^T: ``kv_splits`` is
    refused."""
    if kv_splits is not None:
        raise ValueError("attention_t: kv_splits is not supported (the split kernels write no O^T)")
    sc = scale if scale is not None else q.size(-1) ** -0.5
    if q_offset is not None:
        _check_q_offset(q, k, q_offset, doc)
    if q.is_cuda:
        if not flash_attention_supported(q, k, d64=True):
            raise ValueError("HIP flash attention needs bf16, head dim 64 or 128 and S % 128 == 0")
        return _FlashAttention.apply(q, k, v, sc, True, doc, q_offset)
    o = attention_ref(q, k, v, sc, doc, q_offset)
    B, S, H, D = o.shape
    return o, o.detach().reshape(B * S, H * D).t().contiguous()


# ------------------------------------------------------------------------------------ decode attention
DECODE_BLOCK_SLOTS = 256  # 256 CUs x the one workgroup per CU of the decode kernel (128 KiB of LDS)
DECODE_MAX_ROWS = 32  # Sq * (H / Hkv): the query columns of one 32x32 MFMA tile
# The fewest 64-key tiles "auto" leaves each split of a full cache: two tiles for each of a workgroup's four
# waves.  Measured on one MI355X (bench/attn_decode_bench.py, 32 / 8 heads, Sq 1, B 1, 8, 64 at kv_len 2048, 8192,
# 32768 and B 8 mixed, every n interleaved in one process, two runs; profiles/attn_decode/SUMMARY.md): the rule
# that set MIN_KEY_BLOCKS_PER_SPLIT does not tell the candidates 1, 2, 4, .. 64 apart here, since with none of
# them does a shape get an n > 1 slower than n = 1 by more than the spread (0.7 %).  Among them 8 has the
# smallest time summed over the shapes (0.595 of n = 1; 0.603 at 1, 0.612 at 32): at 1, B 1 at kv_len 2048 gets
# n = 32 and 34.9 us where n = 4 takes 16.8 (n = 1: 42.0); at 32, B 1 at 32768 falls from n = 32 to 16.
MIN_TILES_PER_DECODE_SPLIT = 8


def decode_splits_for(B: int, Hkv: int, Smax: int) -> int:
    """The ``kv_splits`` that ``attention_decode(..., kv_splits="auto")`` uses: the smallest power of two n with
    ``B * Hkv * n`` at least the chip's 256 decode workgroup slots, at most 64, and no larger than leaves every
    split of a full cache (``ceil(Smax / 64)`` tiles) ``MIN_TILES_PER_DECODE_SPLIT`` tiles.  A function of the
    shapes alone: ``kv_len`` lives on the device."""
    tiles, n = -(-Smax // 64), 1
    while n < 64 and B * Hkv * n < DECODE_BLOCK_SLOTS and tiles // (2 * n) >= MIN_TILES_PER_DECODE_SPLIT:
        n *= 2
    return n


def _check_decode(q, k_cache, v_cache, kv_len, kv_splits) -> int:
    """The requirements of :func:`attention_decode`, refused before any launch; -> the number of splits."""
    for name, x in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)):
        if x.dim() != 4 or x.dtype != torch.bfloat16:
            raise ValueError(f"attention_decode: {name} must be a bf16 [B, heads, S, 128] tensor, got {x.dtype} {tuple(x.shape)}")
        if x.size(-1) != 128:
            raise ValueError(f"attention_decode: head dim must be 128, got {x.size(-1)}")
    if k_cache.shape != v_cache.shape or k_cache.size(0) != q.size(0):
        raise ValueError("attention_decode: k_cache and v_cache must have one shape and q's batch size")
    if k_cache.device != q.device or v_cache.device != q.device:
        raise ValueError("attention_decode: q and the caches must be on one device")
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("attention_decode: the caches must be contiguous")
    B, H, Sq, _ = q.shape
    Hkv, Smax = k_cache.size(1), k_cache.size(2)
    if Hkv == 0 or H % Hkv:
        raise ValueError(f"attention_decode: q heads ({H}) must be a multiple of kv heads ({Hkv})")
    if not 1 <= Sq * (H // Hkv) <= DECODE_MAX_ROWS:
        raise ValueError(f"attention_decode: Sq * (H / Hkv) must be between 1 and {DECODE_MAX_ROWS}, got {Sq * (H // Hkv)}")
    if Smax < Sq:
        raise ValueError(f"attention_decode: the cache length {Smax} is below the query length {Sq}")
    if not isinstance(kv_len, torch.Tensor) or kv_len.dtype != torch.int32 or kv_len.shape != (B,) or kv_len.device != q.device:
        raise ValueError("attention_decode: kv_len must be an int32 [B] tensor on the caches' device")
    if torch.is_grad_enabled() and any(x.requires_grad for x in (q, k_cache, v_cache)):
        raise ValueError("attention_decode: forward only, an input requires grad")
    if kv_splits == "auto":
        return decode_splits_for(B, Hkv, Smax)
    if isinstance(kv_splits, bool) or not isinstance(kv_splits, int) or not 1 <= kv_splits <= 64:
        raise ValueError(f"attention_decode: kv_splits must be 'auto' or an int from 1 to 64, got {kv_splits!r}")
    return kv_splits


def attention_decode_ref(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, kv_len: torch.Tensor,
                         scale: float | None = None):
    """fp32 decode attention -> (o [B, Sq, H, D] in q's dtype, lse2 [B, H, Sq] fp32, log2 units): query i of
    sequence b sees the keys ``j <= kv_len[b] - Sq + i`` of its cache; rows at or past ``kv_len[b]`` do not
    enter, whatever they hold."""
    B, H, Sq, D = q.shape
    Hkv, Smax = k_cache.size(1), k_cache.size(2)
    n = kv_len.long().clamp(Sq, Smax).view(B, 1, 1, 1, 1)  # the kernel's clamp
    j = torch.arange(Smax, device=q.device).view(1, 1, 1, 1, Smax)
    valid = (j < n).view(B, 1, 1, Smax, 1)
    k = torch.where(valid, k_cache.float().view(B, Hkv, 1, Smax, D), 0.0)
    v = torch.where(valid, v_cache.float().view(B, Hkv, 1, Smax, D), 0.0)
    sc = scale if scale is not None else D ** -0.5
    s = torch.matmul(q.float().view(B, Hkv, H // Hkv, Sq, D), k.transpose(-1, -2)) * sc
    s = s.masked_fill(j > n - Sq + torch.arange(Sq, device=q.device).view(1, 1, 1, Sq, 1), float("-inf"))
    o = torch.matmul(torch.softmax(s, dim=-1), v).reshape(B, H, Sq, D).transpose(1, 2).to(q.dtype).contiguous()
    return o, (torch.logsumexp(s, dim=-1) * 1.4426950408889634).reshape(B, H, Sq)


def attention_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, kv_len: torch.Tensor,
                     scale: float | None = None, kv_splits="auto", return_lse: bool = False, check: bool = False):
    """One decode step of GQA attention over a ragged KV cache -> o [B, Sq, H, 128] bf16 (with ``return_lse``
    also lse2 [B, H, Sq] fp32, log2 units).  Forward only.

    ``q`` [B, H, Sq, 128] bf16 holds the Sq new tokens' queries, ``1 <= Sq`` and ``Sq * (H / Hkv) <= 32``.
    ``k_cache``, ``v_cache`` [B, Hkv, Smax, 128] bf16, contiguous, any Smax >= Sq.  ``kv_len`` int32 [B] on the
    caches' device: the valid keys of each sequence with the new tokens already appended, ``Sq <= kv_len[b] <=
    Smax``.  Query i of sequence b sits at position ``kv_len[b] - Sq + i`` and sees the keys up to it.  The
    kernel (csrc/ops/attention_decode.hip) reads ``kv_len`` on the device and clamps it into [Sq, Smax]: no
    host sync, and no value moves an access outside the cache.  ``check=True`` costs one sync and raises
    ``ValueError`` for a value outside that range.  The result does not depend on cache rows at or past
    ``kv_len[b]``, NaN and Inf included.

    ``kv_splits``: an int n from 1 to 64 deals each sequence's 64-key tiles to n workgroups per KV head, whose
    fp32 partials the split-KV merge combines in split order; ``"auto"`` is :func:`decode_splits_for`.  On CPU
    tensors the call is :func:`attention_decode_ref`, and ``kv_splits`` is accepted and ignored."""
    n = _check_decode(q, k_cache, v_cache, kv_len, kv_splits)
    Sq, Smax = q.size(2), k_cache.size(2)
    if check and not bool(((kv_len >= Sq) & (kv_len <= Smax)).all()):
        raise ValueError(f"attention_decode: kv_len must lie in [{Sq}, {Smax}], got {kv_len.tolist()}")
    sc = scale if scale is not None else q.size(-1) ** -0.5
    if q.is_cuda:
        o, lse2 = hip().attn_decode(q.contiguous(), k_cache, v_cache, kv_len.contiguous(), float(sc), n)
    else:
        o, lse2 = attention_decode_ref(q, k_cache, v_cache, kv_len, sc)
    return (o, lse2) if return_lse else o


# ------------------------------------------------------------------------------------ decode over a paged KV cache
KV_APPEND_MAX_ROWS = 32  # the new tokens one kv_cache_append call takes per sequence


def _check_paged(who, x, k_pool, v_pool, block_table, kv_len):
    """What :func:`attention_decode_paged` and :func:`kv_cache_append` ask of the pools, the table and the lengths;
    ``x`` is q or k_new."""
    for name, t in ((("q" if who.startswith("attention_") else "k_new"), x), ("k_pool", k_pool), ("v_pool", v_pool)):
        if t.dim() != 4 or t.dtype != torch.bfloat16:
            raise ValueError(f"{who}: {name} must be a bf16 4-d tensor with head dim 128, got {t.dtype} {tuple(t.shape)}")
        if t.size(-1) != 128:
            raise ValueError(f"{who}: head dim must be 128, got {t.size(-1)}")
    if k_pool.shape != v_pool.shape:
        raise ValueError(f"{who}: k_pool and v_pool must have one shape")
    if k_pool.device != x.device or v_pool.device != x.device:
        raise ValueError(f"{who}: all tensors must be on one device")
    if not (k_pool.is_contiguous() and v_pool.is_contiguous()):
        raise ValueError(f"{who}: the pools must be contiguous")
    P = k_pool.size(2)
    if k_pool.size(0) == 0 or P % 64 or not 64 <= P <= 1024:
        raise ValueError(f"{who}: page_size must be a multiple of 64 from 64 to 1024 (and the pool not empty), got {P}")
    B = x.size(0)
    if (not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32 or block_table.dim() != 2
            or block_table.size(0) != B or block_table.size(1) == 0 or block_table.device != x.device):
        raise ValueError(f"{who}: block_table must be an int32 [B, max_pages] tensor on the pools' device")
    if not isinstance(kv_len, torch.Tensor) or kv_len.dtype != torch.int32 or kv_len.shape != (B,) or kv_len.device != x.device:
        raise ValueError(f"{who}: kv_len must be an int32 [B] tensor on the pools' device")


def _check_paged_content(who, Sq, k_pool, block_table, kv_len):
    """``check=True``: one sync.  The lengths lie in [Sq, max_pages * page_size] and every table entry a sequence
    needs names a page of the pool."""
    P, Smax = k_pool.size(2), block_table.size(1) * k_pool.size(2)
    if not bool(((kv_len >= Sq) & (kv_len <= Smax)).all()):
        raise ValueError(f"{who}: kv_len must lie in [{Sq}, {Smax}], got {kv_len.tolist()}")
    needed = torch.arange(block_table.size(1), device=kv_len.device).view(1, -1) * P < kv_len.view(-1, 1)
    if bool((needed & ((block_table < 0) | (block_table >= k_pool.size(0)))).any()):
        raise ValueError(f"{who}: a needed block_table entry lies outside [0, {k_pool.size(0)})")


def _gather_pages(pool: torch.Tensor, block_table: torch.Tensor) -> torch.Tensor:
    """The slab [B, Hkv, max_pages * page_size, D] a block table names; ids clamped into the pool as the kernel does."""
    B, MP = block_table.shape
    pages = pool[block_table.long().clamp(0, pool.size(0) - 1)]  # [B, MP, Hkv, P, D]
    return pages.transpose(1, 2).reshape(B, pool.size(1), MP * pool.size(2), pool.size(3))


def attention_decode_paged_ref(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor,
                               kv_len: torch.Tensor, scale: float | None = None):
    """:func:`attention_decode_ref` on the slab gathered from the pages -> (o, lse2)."""
    return attention_decode_ref(q, _gather_pages(k_pool, block_table), _gather_pages(v_pool, block_table), kv_len, scale)


def attention_decode_paged(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor,
                           kv_len: torch.Tensor, scale: float | None = None, kv_splits="auto", return_lse: bool = False,
                           check: bool = False):
    """:func:`attention_decode` over a paged KV cache -> o [B, Sq, H, 128] bf16 (with ``return_lse`` also lse2).
    Forward only.

    ``k_pool``, ``v_pool`` [num_pages, Hkv, page_size, 128] bf16, contiguous, ``page_size`` a multiple of 64 from
    64 to 1024; the pool may exceed 4 GiB.  ``block_table`` int32 [B, max_pages] on the pools' device: entry
    [b, p] is the pool page holding keys ``p * page_size ..`` of sequence b; only the entries below
    ``ceil(kv_len[b] / page_size)`` are read, and sequences may share pages.  ``kv_len`` and ``q`` as in
    :func:`attention_decode` with ``Smax = max_pages * page_size``.  The kernel
    (csrc/ops/attention_decode_paged.hip) follows the table on the device and clamps the lengths and every page
    id, so no content of either moves an access outside the pools; ``check=True`` costs one sync and raises
    ``ValueError`` for a length out of range or a needed entry outside ``[0, num_pages)``.  The result is
    :func:`attention_decode`'s on the gathered slab at the same ``kv_splits``, bit for bit; ``"auto"`` is
    ``decode_splits_for(B, Hkv, max_pages * page_size)``.  On CPU tensors the call is
    :func:`attention_decode_paged_ref`."""
    who = "attention_decode_paged"
    _check_paged(who, q, k_pool, v_pool, block_table, kv_len)
    B, H, Sq, _ = q.shape
    Hkv, Smax = k_pool.size(1), block_table.size(1) * k_pool.size(2)
    if Hkv == 0 or H % Hkv:
        raise ValueError(f"{who}: q heads ({H}) must be a multiple of kv heads ({Hkv})")
    if not 1 <= Sq * (H // Hkv) <= DECODE_MAX_ROWS:
        raise ValueError(f"{who}: Sq * (H / Hkv) must be between 1 and {DECODE_MAX_ROWS}, got {Sq * (H // Hkv)}")
    if torch.is_grad_enabled() and any(x.requires_grad for x in (q, k_pool, v_pool)):
        raise ValueError(f"{who}: forward only, an input requires grad")
    if kv_splits == "auto":
        n = decode_splits_for(B, Hkv, Smax)
    elif isinstance(kv_splits, bool) or not isinstance(kv_splits, int) or not 1 <= kv_splits <= 64:
        raise ValueError(f"{who}: kv_splits must be 'auto' or an int from 1 to 64, got {kv_splits!r}")
    else:
        n = kv_splits
    if check:
        _check_paged_content(who, Sq, k_pool, block_table, kv_len)
    sc = scale if scale is not None else q.size(-1) ** -0.5
    if q.is_cuda:
        o, lse2 = hip().attn_decode_paged(q.contiguous(), k_pool, v_pool, block_table.contiguous(), kv_len.contiguous(), float(sc), n)
    else:
        o, lse2 = attention_decode_paged_ref(q, k_pool, v_pool, block_table, kv_len, sc)
    return (o, lse2) if return_lse else o


def kv_cache_append_ref(k_new: torch.Tensor, v_new: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                        block_table: torch.Tensor, kv_len: torch.Tensor) -> None:
    """The append as an indexed assignment, in place: row i of sequence b to position ``kv_len[b] - Sq + i``.  A
    sequence whose length is outside [Sq, max_pages * page_size] and a row whose page id is outside the pool
    are skipped."""
    B, _, Sq, _ = k_new.shape
    P, MP = k_pool.size(2), block_table.size(1)
    n = kv_len.long().view(B, 1)
    pos = n - Sq + torch.arange(Sq, device=k_new.device).view(1, Sq)
    page = block_table.long().gather(1, (pos // P).clamp(0, MP - 1))
    ok = (n >= Sq) & (n <= MP * P) & (page >= 0) & (page < k_pool.size(0))
    b, i = ok.nonzero(as_tuple=True)
    k_pool[page[b, i], :, pos[b, i] % P] = k_new[b, :, i]
    v_pool[page[b, i], :, pos[b, i] % P] = v_new[b, :, i]


def kv_cache_append(k_new: torch.Tensor, v_new: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                    block_table: torch.Tensor, kv_len: torch.Tensor, check: bool = False) -> None:
    """The other half of a decode step over a paged cache: write the Sq new tokens' rows ``k_new``, ``v_new``
    [B, Hkv, Sq, 128] bf16 (``1 <= Sq <= 32``) into the pages, in place and on the current stream.  ``kv_len``
    counts the new tokens, the same tensor :func:`attention_decode_paged` then takes: row i of sequence b goes to
    position ``kv_len[b] - Sq + i``, page ``block_table[b, pos // page_size]``, row ``pos % page_size``.  The
    kernel (csrc/ops/attention_decode_paged.hip) skips a sequence whose length is outside [Sq, max_pages *
    page_size] and a row whose page id is outside the pool: a wrong table overwrites nobody's keys.
    ``check=True`` costs one sync and raises ``ValueError`` for either.  On CPU tensors the call is
    :func:`kv_cache_append_ref`."""
    who = "kv_cache_append"
    _check_paged(who, k_new, k_pool, v_pool, block_table, kv_len)
    if v_new.shape != k_new.shape or v_new.dtype != torch.bfloat16 or v_new.device != k_new.device:
        raise ValueError(f"{who}: k_new and v_new must be bf16 tensors of one shape on one device")
    if k_new.size(1) != k_pool.size(1):
        raise ValueError(f"{who}: the new rows have {k_new.size(1)} KV heads, the pools {k_pool.size(1)}")
    if not 1 <= k_new.size(2) <= KV_APPEND_MAX_ROWS:
        raise ValueError(f"{who}: Sq must be between 1 and {KV_APPEND_MAX_ROWS}, got {k_new.size(2)}")
    if torch.is_grad_enabled() and any(x.requires_grad for x in (k_new, v_new, k_pool, v_pool)):
        raise ValueError(f"{who}: forward only, an input requires grad")
    if check:
        _check_paged_content(who, k_new.size(2), k_pool, block_table, kv_len)
    if k_new.is_cuda:
        hip().kv_append_paged(k_new.contiguous(), v_new.contiguous(), k_pool, v_pool, block_table.contiguous(), kv_len.contiguous())
    else:
        kv_cache_append_ref(k_new, v_new, k_pool, v_pool, block_table, kv_len)


# ------------------------------------------------------------------------------------ prefill over the paged KV cache
def _chunk_lengths(who, x, k_pool, block_table, kv_len, q_len, check):
    """-> q_len as an int32 [B] tensor (``None``: every sequence has Sq rows); the refusals :func:`attention_prefill_paged`
    and :func:`kv_cache_append_prefill` add to :func:`_check_paged`.  ``check=True``: one sync."""
    B, Sq = x.size(0), x.size(2)
    P, Smax = k_pool.size(2), block_table.size(1) * k_pool.size(2)
    if B == 0 or not 1 <= Sq <= Smax:
        raise ValueError(f"{who}: Sq must be between 1 and max_pages * page_size = {Smax}, got {Sq}")
    if q_len is None:
        q_len = torch.full((B,), Sq, dtype=torch.int32, device=x.device)
    elif not isinstance(q_len, torch.Tensor) or q_len.dtype != torch.int32 or q_len.shape != (B,) or q_len.device != x.device:
        raise ValueError(f"{who}: q_len must be an int32 [B] tensor on the pools' device")
    if check:
        if not bool(((q_len >= 0) & (q_len <= Sq)).all()):
            raise ValueError(f"{who}: q_len must lie in [0, {Sq}], got {q_len.tolist()}")
        if not bool(((kv_len >= q_len) & (kv_len <= Smax)).all()):
            raise ValueError(f"{who}: kv_len must lie in [q_len, {Smax}], got {kv_len.tolist()} for q_len {q_len.tolist()}")
        needed = (torch.arange(block_table.size(1), device=kv_len.device).view(1, -1) * P < kv_len.view(-1, 1)) & (q_len > 0).view(-1, 1)
        if bool((needed & ((block_table < 0) | (block_table >= k_pool.size(0)))).any()):
            raise ValueError(f"{who}: a needed block_table entry lies outside [0, {k_pool.size(0)})")
    return q_len


def attention_prefill_paged_ref(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor,
                                kv_len: torch.Tensor, q_len: Optional[torch.Tensor] = None, scale: float | None = None):
    """fp32 prefill attention over the pages -> (o [B, Sq, H, D] in q's dtype, lse2 [B, H, Sq] fp32, log2 units):
    :func:`attention_decode_ref` of each sequence's ``ql = clamp(q_len[b], 0, Sq)`` real rows on the gathered slab.
    Rows at or past ``ql`` are not read and give ``o = 0``, ``lse2 = -inf``."""
    B, H, Sq, D = q.shape
    k, v = _gather_pages(k_pool, block_table), _gather_pages(v_pool, block_table)
    ql = [Sq] * B if q_len is None else q_len.clamp(0, Sq).tolist()
    o = torch.zeros(B, Sq, H, D, dtype=q.dtype, device=q.device)
    lse2 = torch.full((B, H, Sq), float("-inf"), dtype=torch.float32, device=q.device)
    for b, n in enumerate(ql):
        if n:
            ob, lb = attention_decode_ref(q[b:b + 1, :, :n], k[b:b + 1], v[b:b + 1], kv_len[b:b + 1], scale)
            o[b, :n], lse2[b, :, :n] = ob[0], lb[0]
    return o, lse2


def attention_prefill_paged(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor,
                            kv_len: torch.Tensor, q_len: Optional[torch.Tensor] = None, scale: float | None = None,
                            return_lse: bool = False, check: bool = False):
    """Prefill and chunked prefill of GQA attention straight over a paged KV cache -> o [B, Sq, H, 128] bf16 (with
    ``return_lse`` also lse2 [B, H, Sq] fp32, log2 units).  Forward only.

    ``q`` [B, H, Sq, 128] bf16, any ``1 <= Sq <= max_pages * page_size``: the batch's chunks padded to Sq rows.
    ``q_len`` int32 [B] on the pools' device says how many rows of each sequence are real (``None``: all Sq); 0 is
    an idle batch slot.  The pools, ``block_table`` and ``kv_len`` are :func:`attention_decode_paged`'s, ``kv_len``
    counting the chunk's tokens (append them first with :func:`kv_cache_append_prefill`).  With ``ql = clamp(q_len[b],
    0, Sq)`` and ``len = clamp(kv_len[b], ql, max_pages * page_size)``, row ``i < ql`` sits at position ``len - ql +
    i`` and sees the keys up to it; rows ``i >= ql`` are not read (they may hold NaN) and give ``o = 0``, ``lse2 =
    -inf``.  The kernel (csrc/ops/attention_prefill_paged.hip) reads the lengths and the table on the device and
    clamps them and every page id: no host sync, and no content moves an access outside the pools, the table or
    ``q``.  The result does not depend on pool rows at or past ``kv_len[b]``, on unused pages or on table entries
    past ``ceil(len / page_size)``, NaN and Inf included.  ``check=True`` costs one sync and raises ``ValueError``
    for a ``q_len`` outside [0, Sq], a ``kv_len`` outside [q_len, max_pages * page_size] or a needed table entry
    outside the pool.  On CPU tensors the call is :func:`attention_prefill_paged_ref`.

    Not served: split-KV for a short chunk against a very long prefix (one workgroup walks a query block's whole
    prefix), a backward, head dim 64.  The fp8 pools: :func:`attention_prefill_paged_fp8`."""
    who = "attention_prefill_paged"
    _check_paged(who, q, k_pool, v_pool, block_table, kv_len)
    H, Hkv = q.size(1), k_pool.size(1)
    if Hkv == 0 or H == 0 or H % Hkv:
        raise ValueError(f"{who}: q heads ({H}) must be a multiple of kv heads ({Hkv})")
    if torch.is_grad_enabled() and any(x.requires_grad for x in (q, k_pool, v_pool)):
        raise ValueError(f"{who}: forward only, an input requires grad")
    ql = _chunk_lengths(who, q, k_pool, block_table, kv_len, q_len, check)
    sc = scale if scale is not None else q.size(-1) ** -0.5
    if q.is_cuda:
        o, lse2 = hip().attn_prefill_paged(q.contiguous(), k_pool, v_pool, block_table.contiguous(), kv_len.contiguous(),
                                           ql.contiguous(), float(sc))
    else:
        o, lse2 = attention_prefill_paged_ref(q, k_pool, v_pool, block_table, kv_len, ql, sc)
    return (o, lse2) if return_lse else o


def kv_cache_append_prefill_ref(k_new: torch.Tensor, v_new: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                                block_table: torch.Tensor, kv_len: torch.Tensor, q_len: Optional[torch.Tensor] = None) -> None:
    """:func:`kv_cache_append_ref`'s indexed assignment for a ragged chunk, in place: row ``i < ql`` of sequence b to
    position ``kv_len[b] - ql + i``.  A sequence whose length is outside [ql, max_pages * page_size] and a row whose
    page id is outside the pool are skipped; rows at or past ``ql`` are not read."""
    B, _, Sq, _ = k_new.shape
    P, MP = k_pool.size(2), block_table.size(1)
    n = kv_len.long().view(B, 1)
    ql = torch.full_like(n, Sq) if q_len is None else q_len.long().clamp(0, Sq).view(B, 1)
    i = torch.arange(Sq, device=k_new.device).view(1, Sq)
    pos = n - ql + i
    page = block_table.long().gather(1, (pos // P).clamp(0, MP - 1))
    ok = (i < ql) & (n >= ql) & (n <= MP * P) & (page >= 0) & (page < k_pool.size(0))
    b, i = ok.nonzero(as_tuple=True)
    k_pool[page[b, i], :, pos[b, i] % P] = k_new[b, :, i]
    v_pool[page[b, i], :, pos[b, i] % P] = v_new[b, :, i]


def kv_cache_append_prefill(k_new: torch.Tensor, v_new: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor,
                            block_table: torch.Tensor, kv_len: torch.Tensor, q_len: Optional[torch.Tensor] = None,
                            check: bool = False) -> None:
    """The other half of a prefill step: write a ragged chunk's rows ``k_new``, ``v_new`` [B, Hkv, Sq, 128] bf16, any
    Sq, into the pages in one launch, in place and on the current stream.  ``kv_len`` and ``q_len`` are the tensors
    :func:`attention_prefill_paged` then takes: row ``i < q_len[b]`` goes to position ``kv_len[b] - q_len[b] + i``.
    The kernel (csrc/ops/attention_prefill_paged.hip) skips a sequence whose length is outside [q_len, max_pages *
    page_size] and a row whose page id is outside the pool, as :func:`kv_cache_append` does; ``check=True`` costs one
    sync and raises ``ValueError`` for either.  On CPU tensors the call is :func:`kv_cache_append_prefill_ref`."""
    who = "kv_cache_append_prefill"
    _check_paged(who, k_new, k_pool, v_pool, block_table, kv_len)
    if v_new.shape != k_new.shape or v_new.dtype != torch.bfloat16 or v_new.device != k_new.device:
        raise ValueError(f"{who}: k_new and v_new must be bf16 tensors of one shape on one device")
    if k_new.size(1) != k_pool.size(1):
        raise ValueError(f"{who}: the new rows have {k_new.size(1)} KV heads, the pools {k_pool.size(1)}")
    if torch.is_grad_enabled() and any(x.requires_grad for x in (k_new, v_new, k_pool, v_pool)):
        raise ValueError(f"{who}: forward only, an input requires grad")
    ql = _chunk_lengths(who, k_new, k_pool, block_table, kv_len, q_len, check)
    if k_new.is_cuda:
        hip().kv_append_paged_chunk(k_new.contiguous(), v_new.contiguous(), k_pool, v_pool, block_table.contiguous(),
                                    kv_len.contiguous(), ql.contiguous())
    else:
        kv_cache_append_prefill_ref(k_new, v_new, k_pool, v_pool, block_table, kv_len, ql)


# ------------------------------------------------------------------------------------ the paged KV cache in fp8
# Cache format (csrc/ops/attention_decode_paged_fp8.hip): ``k_codes``, ``v_codes`` uint8 [num_pages, Hkv, page_size,
# 128], one OCP e4m3fn code per element, and ``k_exp``, ``v_exp`` uint8 [num_pages, Hkv, page_size], one byte
# ``e + 127`` per key row and KV head: 129 bytes a row against 256.  A block is one 128-element row and its rule is
# the one of the K7 fp8 wire (csrc/probe/peer_q8.h, ops/peer_ref.q8_quantize_ref); V is row-major like K.
KV_EXP_MIN, KV_EXP_MAX = -100, 120


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """fp32 ``2^e`` from the exponent field: exact on every device; ``e`` an integer tensor in [-127, 128]."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def _e4m3_values() -> torch.Tensor:
    """float32 value of every e4m3fn code; 0x7f and 0xff, the format's only non-finite codes, are NaN."""
    c = torch.arange(256)
    e, m = (c >> 3) & 15, (c & 7).float()
    mag = torch.where(e == 0, m * 2.0 ** -9, (8 + m) * _pow2(e - 10))
    mag[(c & 0x7F) == 0x7F] = float("nan")
    return torch.where((c & 0x80) != 0, -mag, mag)


_E4M3 = _e4m3_values()


def kv_quantize_ref(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rows ``x`` [..., 128] -> ``(codes uint8 [..., 128], exp uint8 [...])``, the cache format's rule, which decides:
    per row ``e`` is the smallest integer with ``amax * 2^-e <= 448``, clamped to [-100, 120] (``amax == 0``: -100),
    the amax taken over the row's elements that are not NaN (an Inf counts: ``e = 120``); a code is ``x * 2^-e``
    rounded to nearest even into e4m3fn, subnormal codes (quantum ``2^-9``) included; a NaN or an Inf gets the code
    0x7f under its sign bit.  The stored byte is ``e + 127``."""
    v = x.float()
    special = ~torch.isfinite(v)
    amax = torch.where(torch.isnan(v), 0.0, v.abs()).amax(-1)
    inf = torch.isinf(amax)
    m, ex = torch.frexp(torch.where(inf, 0.0, amax))  # amax = m * 2^ex, m in [0.5, 1); 448 = 0.875 * 2^9
    e = torch.where(amax == 0, KV_EXP_MIN, (ex - 9 + (m > 0.875)).clamp(KV_EXP_MIN, KV_EXP_MAX))
    e = torch.where(inf, KV_EXP_MAX, e)
    y = torch.where(special, 0.0, v) * _pow2(-e).unsqueeze(-1)  # exact, or too small for any code but 0
    a = y.abs().double()
    _, ea = torch.frexp(a)  # a in [2^(ea - 1), 2^ea): three mantissa bits below the leading one
    quantum = _pow2((ea - 4).clamp(min=-9)).double()
    r = torch.round(a / quantum) * quantum  # torch.round rounds halves to even
    mr, er = torch.frexp(r)
    code = torch.where(r >= 2.0 ** -6, (er + 6) * 8 + torch.round((mr * 2 - 1) * 8), torch.round(r * 512)).long()
    code = torch.where(special, 0x7F, code.clamp(max=0x7E)) | (torch.signbit(v).long() << 7)
    return code.to(torch.uint8), (e + 127).to(torch.uint8)


def kv_dequantize_ref(codes: torch.Tensor, exp: torch.Tensor) -> torch.Tensor:
    """``float(code) * 2^e`` as bf16 [..., 128], exact: a code has at most 4 significant bits.  The codes 0x7f and
    0xff give NaN."""
    return (_E4M3.to(codes.device)[codes.long()] * _pow2(exp.to(torch.int32) - 127).unsqueeze(-1)).to(torch.bfloat16)


def _check_paged_fp8(who, x, k_codes, v_codes, k_exp, v_exp, block_table, kv_len):
    """What the calls over the fp8 cache ask of the four pools, the table and the lengths; ``x`` is q (the attention
    calls) or k_new (the appends)."""
    name = "q" if who.startswith("attention_") else "k_new"
    if x.dim() != 4 or x.dtype != torch.bfloat16 or x.size(-1) != 128:
        raise ValueError(f"{who}: {name} must be a bf16 4-d tensor with head dim 128, got {x.dtype} {tuple(x.shape)}")
    pools = (("k_codes", k_codes), ("v_codes", v_codes), ("k_exp", k_exp), ("v_exp", v_exp))
    for pname, t in pools:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise ValueError(f"{who}: {pname} must be a uint8 tensor, got {getattr(t, 'dtype', type(t))}")
    if k_codes.dim() != 4 or k_codes.size(-1) != 128 or v_codes.shape != k_codes.shape:
        raise ValueError(f"{who}: k_codes and v_codes must be [num_pages, Hkv, page_size, 128] alike, got "
                         f"{tuple(k_codes.shape)} and {tuple(v_codes.shape)}")
    if k_exp.shape != k_codes.shape[:3] or v_exp.shape != k_codes.shape[:3]:
        raise ValueError(f"{who}: k_exp and v_exp must be [num_pages, Hkv, page_size] of the code pools, got "
                         f"{tuple(k_exp.shape)} and {tuple(v_exp.shape)}")
    if any(t.device != x.device for _, t in pools):
        raise ValueError(f"{who}: all tensors must be on one device")
    if not all(t.is_contiguous() for _, t in pools):
        raise ValueError(f"{who}: the pools must be contiguous")
    P = k_codes.size(2)
    if k_codes.size(0) == 0 or P % 64 or not 64 <= P <= 1024:
        raise ValueError(f"{who}: page_size must be a multiple of 64 from 64 to 1024 (and the pool not empty), got {P}")
    B = x.size(0)
    if (not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32 or block_table.dim() != 2
            or block_table.size(0) != B or block_table.size(1) == 0 or block_table.device != x.device):
        raise ValueError(f"{who}: block_table must be an int32 [B, max_pages] tensor on the pools' device")
    if not isinstance(kv_len, torch.Tensor) or kv_len.dtype != torch.int32 or kv_len.shape != (B,) or kv_len.device != x.device:
        raise ValueError(f"{who}: kv_len must be an int32 [B] tensor on the pools' device")


def attention_decode_paged_fp8_ref(q: torch.Tensor, k_codes: torch.Tensor, v_codes: torch.Tensor, k_exp: torch.Tensor,
                                   v_exp: torch.Tensor, block_table: torch.Tensor, kv_len: torch.Tensor,
                                   scale: float | None = None):
    """:func:`attention_decode_paged_ref` on the dequantised pools -> (o, lse2)."""
    return attention_decode_paged_ref(q, kv_dequantize_ref(k_codes, k_exp), kv_dequantize_ref(v_codes, v_exp), block_table, kv_len,
                                      scale)


def attention_decode_paged_fp8(q: torch.Tensor, k_codes: torch.Tensor, v_codes: torch.Tensor, k_exp: torch.Tensor,
                               v_exp: torch.Tensor, block_table: torch.Tensor, kv_len: torch.Tensor,
                               scale: float | None = None, kv_splits="auto", return_lse: bool = False, check: bool = False):
    """:func:`attention_decode_paged` over a KV cache kept in 8 bits -> o [B, Sq, H, 128] bf16 (with ``return_lse``
    also lse2).  Forward only.

    ``k_codes``, ``v_codes`` uint8 [num_pages, Hkv, page_size, 128] and ``k_exp``, ``v_exp`` uint8 [num_pages, Hkv,
    page_size], contiguous: the format :func:`kv_quantize_ref` defines and :func:`kv_cache_append_fp8` writes, half
    the bytes of the bf16 pools and so twice the tokens a pool holds.  ``page_size``, ``block_table``, ``kv_len``,
    ``q``, ``kv_splits`` and ``check`` are :func:`attention_decode_paged`'s.  The kernel
    (csrc/ops/attention_decode_paged_fp8.hip) widens the codes exactly and carries the rows' power-of-two scales
    on the fp32 scores and probabilities, so the result is :func:`attention_decode_paged`'s on the dequantised pools
    (:func:`kv_dequantize_ref`) at the same ``kv_splits``, bit for bit.  It does not depend on the bytes of unused
    pages or of rows at or past ``kv_len[b]``, and no content of the table, the lengths or the exponent bytes moves
    an access outside the pools.  On CPU tensors the call is :func:`attention_decode_paged_fp8_ref`."""
    who = "attention_decode_paged_fp8"
    _check_paged_fp8(who, q, k_codes, v_codes, k_exp, v_exp, block_table, kv_len)
    B, H, Sq, _ = q.shape
    Hkv, Smax = k_codes.size(1), block_table.size(1) * k_codes.size(2)
    if Hkv == 0 or H % Hkv:
        raise ValueError(f"{who}: q heads ({H}) must be a multiple of kv heads ({Hkv})")
    if not 1 <= Sq * (H // Hkv) <= DECODE_MAX_ROWS:
        raise ValueError(f"{who}: Sq * (H / Hkv) must be between 1 and {DECODE_MAX_ROWS}, got {Sq * (H // Hkv)}")
    if torch.is_grad_enabled() and q.requires_grad:
        raise ValueError(f"{who}: forward only, an input requires grad")
    if kv_splits == "auto":
        n = decode_splits_for(B, Hkv, Smax)
    elif isinstance(kv_splits, bool) or not isinstance(kv_splits, int) or not 1 <= kv_splits <= 64:
        raise ValueError(f"{who}: kv_splits must be 'auto' or an int from 1 to 64, got {kv_splits!r}")
    else:
        n = kv_splits
    if check:
        _check_paged_content(who, Sq, k_codes, block_table, kv_len)
    sc = scale if scale is not None else q.size(-1) ** -0.5
    if q.is_cuda:
        o, lse2 = hip().attn_decode_paged_fp8(q.contiguous(), k_codes, v_codes, k_exp, v_exp, block_table.contiguous(),
                                              kv_len.contiguous(), float(sc), n)
    else:
        o, lse2 = attention_decode_paged_fp8_ref(q, k_codes, v_codes, k_exp, v_exp, block_table, kv_len, sc)
    return (o, lse2) if return_lse else o


def kv_cache_append_fp8_ref(k_new: torch.Tensor, v_new: torch.Tensor, k_codes: torch.Tensor, v_codes: torch.Tensor,
                            k_exp: torch.Tensor, v_exp: torch.Tensor, block_table: torch.Tensor, kv_len: torch.Tensor) -> None:
    """:func:`kv_cache_append_ref` of the new rows' quantised form (:func:`kv_quantize_ref`), in place: the same
    positions, the same skips."""
    B, _, Sq, _ = k_new.shape
    P, MP = k_codes.size(2), block_table.size(1)
    n = kv_len.long().view(B, 1)
    pos = n - Sq + torch.arange(Sq, device=k_new.device).view(1, Sq)
    page = block_table.long().gather(1, (pos // P).clamp(0, MP - 1))
    ok = (n >= Sq) & (n <= MP * P) & (page >= 0) & (page < k_codes.size(0))
    b, i = ok.nonzero(as_tuple=True)
    for new, codes, exp in ((k_new, k_codes, k_exp), (v_new, v_codes, v_exp)):
        c, e = kv_quantize_ref(new)
        codes[page[b, i], :, pos[b, i] % P] = c[b, :, i]
        exp[page[b, i], :, pos[b, i] % P] = e[b, :, i]


def kv_cache_append_fp8(k_new: torch.Tensor, v_new: torch.Tensor, k_codes: torch.Tensor, v_codes: torch.Tensor,
                        k_exp: torch.Tensor, v_exp: torch.Tensor, block_table: torch.Tensor, kv_len: torch.Tensor,
                        check: bool = False) -> None:
    """:func:`kv_cache_append` into the fp8 cache: the Sq new tokens' rows ``k_new``, ``v_new`` [B, Hkv, Sq, 128] bf16
    are quantised by the row rule on their way into the pages, 128 code bytes and one exponent byte a row, in place
    and on the current stream, in one launch that reads nothing of the cache.  Positions, skips and ``check`` are
    :func:`kv_cache_append`'s.  On CPU tensors the call is :func:`kv_cache_append_fp8_ref`."""
    who = "kv_cache_append_fp8"
    _check_paged_fp8(who, k_new, k_codes, v_codes, k_exp, v_exp, block_table, kv_len)
    if v_new.shape != k_new.shape or v_new.dtype != torch.bfloat16 or v_new.device != k_new.device:
        raise ValueError(f"{who}: k_new and v_new must be bf16 tensors of one shape on one device")
    if k_new.size(1) != k_codes.size(1):
        raise ValueError(f"{who}: the new rows have {k_new.size(1)} KV heads, the pools {k_codes.size(1)}")
    if not 1 <= k_new.size(2) <= KV_APPEND_MAX_ROWS:
        raise ValueError(f"{who}: Sq must be between 1 and {KV_APPEND_MAX_ROWS}, got {k_new.size(2)}")
    if torch.is_grad_enabled() and (k_new.requires_grad or v_new.requires_grad):
        raise ValueError(f"{who}: forward only, an input requires grad")
    if check:
        _check_paged_content(who, k_new.size(2), k_codes, block_table, kv_len)
    if k_new.is_cuda:
        hip().kv_append_paged_fp8(k_new.contiguous(), v_new.contiguous(), k_codes, v_codes, k_exp, v_exp, block_table.contiguous(),
                                  kv_len.contiguous())
    else:
        kv_cache_append_fp8_ref(k_new, v_new, k_codes, v_codes, k_exp, v_exp, block_table, kv_len)


# ------------------------------------------------------------------------------------ prefill over the fp8 paged KV cache
def attention_prefill_paged_fp8_ref(q: torch.Tensor, k_codes: torch.Tensor, v_codes: torch.Tensor, k_exp: torch.Tensor,
                                    v_exp: torch.Tensor, block_table: torch.Tensor, kv_len: torch.Tensor,
                                    q_len: Optional[torch.Tensor] = None, scale: float | None = None):
    """:func:`attention_prefill_paged_ref` on the dequantised pools -> (o, lse2)."""
    return attention_prefill_paged_ref(q, kv_dequantize_ref(k_codes, k_exp), kv_dequantize_ref(v_codes, v_exp), block_table, kv_len,
                                       q_len, scale)


def attention_prefill_paged_fp8(q: torch.Tensor, k_codes: torch.Tensor, v_codes: torch.Tensor, k_exp: torch.Tensor,
                                v_exp: torch.Tensor, block_table: torch.Tensor, kv_len: torch.Tensor,
                                q_len: Optional[torch.Tensor] = None, scale: float | None = None, return_lse: bool = False,
                                check: bool = False):
    """:func:`attention_prefill_paged` over a KV cache kept in 8 bits -> o [B, Sq, H, 128] bf16 (with ``return_lse``
    also lse2 [B, H, Sq] fp32, log2 units).  Forward only.

    The four pools are :func:`attention_decode_paged_fp8`'s (write them with :func:`kv_cache_append_prefill_fp8`);
    ``q``, ``q_len``, ``kv_len``, ``block_table``, the clamps, the padded rows (``o = 0``, ``lse2 = -inf``) and
    ``check`` are :func:`attention_prefill_paged`'s.  The kernel (csrc/ops/attention_prefill_paged_fp8.hip) stages a
    tile as codes and turns it, once per workgroup, into the bf16 tile the bf16 kernel works on, so the result is
    :func:`attention_prefill_paged`'s on the dequantised pools (:func:`kv_dequantize_ref`) bit for bit.  It does not
    depend on the bytes of unused pages or of rows at or past ``kv_len[b]``, NaN codes and ``0xff`` exponent bytes
    included, and no content of the table, the lengths or the exponent bytes moves an access outside the four pools,
    the table row or ``q``.  On CPU tensors the call is :func:`attention_prefill_paged_fp8_ref`.

    Not served: split-KV for a short chunk against a very long prefix, a backward, head dim 64."""
    who = "attention_prefill_paged_fp8"
    _check_paged_fp8(who, q, k_codes, v_codes, k_exp, v_exp, block_table, kv_len)
    H, Hkv = q.size(1), k_codes.size(1)
    if Hkv == 0 or H == 0 or H % Hkv:
        raise ValueError(f"{who}: q heads ({H}) must be a multiple of kv heads ({Hkv})")
    if torch.is_grad_enabled() and q.requires_grad:
        raise ValueError(f"{who}: forward only, an input requires grad")
    ql = _chunk_lengths(who, q, k_codes, block_table, kv_len, q_len, check)
    sc = scale if scale is not None else q.size(-1) ** -0.5
    if q.is_cuda:
        o, lse2 = hip().attn_prefill_paged_fp8(q.contiguous(), k_codes, v_codes, k_exp, v_exp, block_table.contiguous(),
                                               kv_len.contiguous(), ql.contiguous(), float(sc))
    else:
        o, lse2 = attention_prefill_paged_fp8_ref(q, k_codes, v_codes, k_exp, v_exp, block_table, kv_len, ql, sc)
    return (o, lse2) if return_lse else o


def kv_cache_append_prefill_fp8_ref(k_new: torch.Tensor, v_new: torch.Tensor, k_codes: torch.Tensor, v_codes: torch.Tensor,
                                    k_exp: torch.Tensor, v_exp: torch.Tensor, block_table: torch.Tensor, kv_len: torch.Tensor,
                                    q_len: Optional[torch.Tensor] = None) -> None:
    """:func:`kv_cache_append_prefill_ref`'s positions and skips applied to the new rows' quantised form
    (:func:`kv_quantize_ref`), in place; rows at or past ``ql`` are not read."""
    B, _, Sq, _ = k_new.shape
    P, MP = k_codes.size(2), block_table.size(1)
    n = kv_len.long().view(B, 1)
    ql = torch.full_like(n, Sq) if q_len is None else q_len.long().clamp(0, Sq).view(B, 1)
    i = torch.arange(Sq, device=k_new.device).view(1, Sq)
    pos = n - ql + i
    page = block_table.long().gather(1, (pos // P).clamp(0, MP - 1))
    ok = (i < ql) & (n >= ql) & (n <= MP * P) & (page >= 0) & (page < k_codes.size(0))
    b, i = ok.nonzero(as_tuple=True)
    for new, codes, exp in ((k_new, k_codes, k_exp), (v_new, v_codes, v_exp)):
        c, e = kv_quantize_ref(new[b, :, i])
        codes[page[b, i], :, pos[b, i] % P] = c
        exp[page[b, i], :, pos[b, i] % P] = e


def kv_cache_append_prefill_fp8(k_new: torch.Tensor, v_new: torch.Tensor, k_codes: torch.Tensor, v_codes: torch.Tensor,
                                k_exp: torch.Tensor, v_exp: torch.Tensor, block_table: torch.Tensor, kv_len: torch.Tensor,
                                q_len: Optional[torch.Tensor] = None, check: bool = False) -> None:
    """:func:`kv_cache_append_prefill` into the fp8 cache: a ragged chunk's rows ``k_new``, ``v_new`` [B, Hkv, Sq, 128]
    bf16, any Sq, are quantised by the row rule on their way into the pages, 128 code bytes and one exponent byte a
    row, in place and on the current stream, in one launch that reads nothing of the cache
    (csrc/ops/attention_prefill_paged_fp8.hip).  Positions, skips, ``q_len`` and ``check`` are
    :func:`kv_cache_append_prefill`'s.  On CPU tensors the call is :func:`kv_cache_append_prefill_fp8_ref`."""
    who = "kv_cache_append_prefill_fp8"
    _check_paged_fp8(who, k_new, k_codes, v_codes, k_exp, v_exp, block_table, kv_len)
    if v_new.shape != k_new.shape or v_new.dtype != torch.bfloat16 or v_new.device != k_new.device:
        raise ValueError(f"{who}: k_new and v_new must be bf16 tensors of one shape on one device")
    if k_new.size(1) != k_codes.size(1):
        raise ValueError(f"{who}: the new rows have {k_new.size(1)} KV heads, the pools {k_codes.size(1)}")
    if torch.is_grad_enabled() and (k_new.requires_grad or v_new.requires_grad):
        raise ValueError(f"{who}: forward only, an input requires grad")
    ql = _chunk_lengths(who, k_new, k_codes, block_table, kv_len, q_len, check)
    if k_new.is_cuda:
        hip().kv_append_paged_chunk_fp8(k_new.contiguous(), v_new.contiguous(), k_codes, v_codes, k_exp, v_exp,
                                        block_table.contiguous(), kv_len.contiguous(), ql.contiguous())
    else:
        kv_cache_append_prefill_fp8_ref(k_new, v_new, k_codes, v_codes, k_exp, v_exp, block_table, kv_len, ql)
