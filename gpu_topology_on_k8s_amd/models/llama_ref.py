"""float64 CPU references of the Llama-step HIP kernels (``csrc/ops/fused_ops.hip``).

Plain ``torch.float64`` on the CPU: no GPU, no HIP kernel.  Every function takes the kernel's own
inputs (bf16 or fp32 tensors, in the kernel's layout) and returns the EXACT value of what the kernel
computes from them, before its single output rounding (bf16, nearest even; fp32 for ``rstd``, ``lse``
and the loss).  Where an output is rounded from an expression with cancellation the function also
returns a condition magnitude ``cond`` >= |value|: the sum of the absolute values of the terms the
kernel's fp32 arithmetic adds.  A kernel's fp32 error is a small multiple of 2^-24 * cond, so
``tests/test_gpu_llama_kernels.py`` accepts an element iff

    |got - value| <= ulp_bf16(value) / 2 + slack * cond

with a slack (2^-18 or 2^-16) far below the 2^-9 of the rounding term: a wrong rounding mode or a
single wrong element cannot pass.  Backward references take ``rstd`` / ``lse`` as arguments (the fp32
tensor the kernel is given), so they are exact for whatever forward values a test passes.

:func:`model_ref64` composes the forward definitions into the whole training step (nothing rounded,
gradients from autograd): what ``tests/test_gpu_llama_model.py`` holds every parameter's gradient to,
under the rule of ``tests/test_llama_model_ref.py``.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from .attention_ref import attn_fwd_ref64
from .mnist_ref import bf16_round

__all__ = ["bf16_round", "rmsnorm_ref", "add_rmsnorm_ref", "rmsnorm_bwd_ref", "rope_split_ref64", "rope_split_bwd_ref64",
           "swiglu_ref64", "swiglu_bwd_ref64", "xent_ref64", "xent_bwd_ref64", "embed_bwd_ref64", "model_ref64"]

T = torch.Tensor


def _f64(t: T) -> T:
    return t.cpu().to(torch.float64)  # differentiable: tests/test_llama_ref.py takes autograd of the forwards


def _eps32(eps: float) -> float:
    """The kernels take ``eps`` as an fp32 argument."""
    return float(torch.tensor(float(eps), dtype=torch.float32))


# ------------------------------------------------------------------------------------ RMSNorm
def rmsnorm_ref(x: T, w: T, eps: float) -> Tuple[T, T]:
    """(y [M, D], rstd [M]): rstd = (mean(x^2) + eps)^-1/2, y = x * rstd * w.  x [M, D], w [D]."""
    x, w = _f64(x), _f64(w)
    x = x.reshape(-1, x.shape[-1])
    rstd = ((x * x).mean(-1) + _eps32(eps)).rsqrt()
    return x * rstd[:, None] * w, rstd


def add_rmsnorm_ref(x: T, r: T, w: T, eps: float) -> Tuple[T, T, T]:
    """(h, y, rstd): h = bf16_round(x + r) is the new residual stream (returned in float64, every
    value a bf16 number: the kernel's h must equal it bit for bit) and the norm is taken of that
    ROUNDED h, as the kernel does."""
    h = bf16_round(_f64(x) + _f64(r)).to(torch.float64)
    y, rstd = rmsnorm_ref(h, w, eps)
    return h.reshape(-1, h.shape[-1]), y, rstd


def rmsnorm_bwd_ref(dy: T, x: T, w: T, rstd: T, dres: Optional[T] = None) -> Tuple[T, T, T, T]:
    """(dx, dw, cond_dx, cond_dw) from the fp32 ``rstd`` the kernel is given (r below):

        dx = r dy w - x r^3 sum(dy w x) / D (+ dres)     cond = |r dy w| + |x| r^3 sum|dy w x| / D (+ |dres|)
        dw = sum over rows of dy x r                     cond = sum |dy x r|
    """
    dy, x, w, r = _f64(dy), _f64(x), _f64(w), _f64(rstd).reshape(-1, 1)
    D = x.shape[-1]
    x, dy = x.reshape(-1, D), dy.reshape(-1, D)
    g = dy * w
    gx = g * x
    r3 = r * r * r
    dx = r * g - x * r3 * gx.sum(-1, keepdim=True) / D
    cdx = (r * g).abs() + x.abs() * r3.abs() * gx.abs().sum(-1, keepdim=True) / D
    if dres is not None:
        dres = _f64(dres).reshape(-1, D)
        dx, cdx = dx + dres, cdx + dres.abs()
    t = dy * x * r
    return dx, t.sum(0), cdx, t.abs().sum(0)


# ------------------------------------------------------------------------------------ RoPE + split
def _tables(cos: T, sin: T, S: int, pos_offset: int) -> Tuple[T, T]:
    c, s = _f64(cos)[pos_offset:pos_offset + S], _f64(sin)[pos_offset:pos_offset + S]
    assert c.shape[0] == S, "rope tables shorter than S + pos_offset"
    return c[None, :, None, :], s[None, :, None, :]


def rope_split_ref64(qkv: T, cos: T, sin: T, B: int, S: int, H: int, Hkv: int, Dh: int, pos_offset: int = 0):
    """qkv [B*S, (H + 2 Hkv) Dh] -> (q [B,H,S,Dh], k [B,Hkv,S,Dh], v [B,Hkv,S,Dh], cond_q, cond_k).

    With a = x[i], b = x[i + Dh/2], c / s = cos / sin[s + pos_offset, i] (the fp32 tables):
    out[i] = a c - b s and out[i + Dh/2] = b c + a s, cond = |a c| + |b s| resp. |b c| + |a s|.
    v is a copy: the kernel's v must equal it bit for bit."""
    x = _f64(qkv).view(B, S, H + 2 * Hkv, Dh)
    c, s = _tables(cos, sin, S, pos_offset)

    def rot(t):
        a, b = t[..., : Dh // 2], t[..., Dh // 2:]
        val = torch.cat([a * c - b * s, b * c + a * s], -1)
        cond = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], -1)
        return val.transpose(1, 2).contiguous(), cond.transpose(1, 2).contiguous()

    q, cq = rot(x[:, :, :H])
    k, ck = rot(x[:, :, H:H + Hkv])
    return q, k, x[:, :, H + Hkv:].transpose(1, 2).contiguous(), cq, ck


def rope_split_bwd_ref64(dq: T, dk: T, dv: T, cos: T, sin: T, pos_offset: int = 0) -> Tuple[T, T]:
    """(dqkv [B*S, (H + 2 Hkv) Dh], cond): the transposed rotation (sin -> -sin) of dq and dk at
    position s + pos_offset, dv copied (its cond is |dv|)."""
    dq, dk, dv = _f64(dq), _f64(dk), _f64(dv)
    B, H, S, Dh = dq.shape
    c, s = _tables(cos, sin, S, pos_offset)

    def unrot(t):
        t = t.transpose(1, 2)  # [B, S, heads, Dh]
        a, b = t[..., : Dh // 2], t[..., Dh // 2:]
        val = torch.cat([a * c + b * s, b * c - a * s], -1)
        cond = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], -1)
        return val, cond

    (q, cq), (k, ck), v = unrot(dq), unrot(dk), dv.transpose(1, 2)
    heads = H + 2 * dk.shape[1]
    return torch.cat([q, k, v], 2).reshape(B * S, heads * Dh), torch.cat([cq, ck, v.abs()], 2).reshape(B * S, heads * Dh)


# ------------------------------------------------------------------------------------ SwiGLU
def swiglu_ref64(gu: T) -> Tuple[T, T]:
    """(h [T, F], cond): h = g sigmoid(g) u from gu = [gate | up]; cond = |h| (1 + |g|), because the
    absolute error of the kernel's fast exponential grows with its argument."""
    g, u = _f64(gu).chunk(2, -1)
    h = g * torch.sigmoid(g) * u
    return h, h.abs() * (1 + g.abs())


def swiglu_bwd_ref64(dh: T, gu: T) -> Tuple[T, T]:
    """(dgu [T, 2F] = [d gate | d up], cond): d up = dh g sg, d gate = dh u sg (1 + g (1 - sg)) with
    sg = sigmoid(g); cond = |value| (1 + |g|), and for d gate + |dh u sg| / 8: the factor
    1 + g (1 - sg) crosses zero at g = -1.27846, where the sum of two terms of magnitude 1 cancels and
    keeps their absolute error (a rounding count of the kernel gives 4.2 * 2^-24, an eighth of the
    2^-18 slack covers twice that; ``tests/test_llama_ref.py``)."""
    g, u = _f64(gu).chunk(2, -1)
    d = _f64(dh).reshape(g.shape)
    sg = torch.sigmoid(g)
    # 1 - sigmoid(g) = sigmoid(-g): no cancellation in the reference for large g
    dgu = torch.cat([d * u * sg * (1 + g * torch.sigmoid(-g)), d * g * sg], -1)
    cancel = torch.cat([(d * u * sg).abs() / 8, torch.zeros_like(g)], -1)
    return dgu, dgu.abs() * (1 + torch.cat([g, g], -1).abs()) + cancel


# ------------------------------------------------------------------------------------ cross-entropy
def _valid(labels: T, V: int, ignore_index: int) -> T:
    return (labels != ignore_index) & (labels >= 0) & (labels < V)


def xent_ref64(logits: T, labels: T, ignore_index: int = -100) -> Tuple[T, T]:
    """(loss_rows [T], lse [T]): lse = log sum exp(x), loss = lse - x[label].

    The kernel's contract: a row whose label is ``ignore_index``, negative, or >= V has loss 0 (its
    lse is still computed)."""
    x, labels = _f64(logits), labels.detach().cpu().long().reshape(-1)
    x = x.reshape(-1, x.shape[-1])
    lse = torch.logsumexp(x, -1)
    ok = _valid(labels, x.shape[1], ignore_index)
    picked = x.gather(1, labels.where(ok, torch.zeros_like(labels))[:, None]).squeeze(1)
    return torch.where(ok, lse - picked, torch.zeros_like(lse)), lse


def xent_bwd_ref64(logits: T, labels: T, lse: T, gscale, ignore_index: int = -100) -> Tuple[T, T]:
    """(dlogits [T, V], cond) from the fp32 ``lse`` the kernel is given:

        value = (exp(x - lse) - onehot) gscale,    cond = (p (1 + |x| + |lse|) + onehot) |gscale|

    (p = exp(x - lse); the exponential's argument carries the rounding of x - lse).  Rows with an
    ignored label (see :func:`xent_ref64`) are exactly 0; x = -inf gives value 0 and cond 0."""
    x, labels, l = _f64(logits), labels.detach().cpu().long().reshape(-1), _f64(lse).reshape(-1, 1)
    x = x.reshape(-1, x.shape[-1])
    g = float(_f64(gscale).reshape(-1)[0]) if isinstance(gscale, torch.Tensor) else float(gscale)
    ok = _valid(labels, x.shape[1], ignore_index)
    p = (x - l).exp()
    onehot = torch.zeros_like(x)
    rows = ok.nonzero().squeeze(1)
    onehot[rows, labels[rows]] = 1.0
    mag = torch.where(p > 0, p * (1 + x.abs() + l.abs()), torch.zeros_like(p))  # NaN-safe: 0 * inf
    val, cond = (p - onehot) * g, (mag + onehot) * abs(g)
    zero = torch.zeros_like(val)
    return torch.where(ok[:, None], val, zero), torch.where(ok[:, None], cond, zero)


# ------------------------------------------------------------------------------------ embedding backward
def embed_bwd_ref64(tok: T, dx: T, V: int) -> Tuple[T, T, T]:
    """(rows [V, D], cond [V, D], owned [V] bool): rows[t] = sum of dx[i] over the positions i with
    tok[i] == t, cond = the same sum of |dx|.  Ids outside [0, V) are skipped; ``owned`` marks the
    rows some position holds (the kernel writes only those)."""
    tok, dx = tok.detach().cpu().long().reshape(-1), _f64(dx)
    dx = dx.reshape(tok.numel(), -1)
    ok = (tok >= 0) & (tok < V)
    rows = torch.zeros(V, dx.shape[1], dtype=torch.float64).index_add_(0, tok[ok], dx[ok])
    cond = torch.zeros(V, dx.shape[1], dtype=torch.float64).index_add_(0, tok[ok], dx[ok].abs())
    owned = torch.zeros(V, dtype=torch.bool)
    owned[tok[ok]] = True
    return rows, cond, owned


# ------------------------------------------------------------------------------------ the whole model
def _embed64(w: T, tokens: T) -> T:
    """[B*S, D]: row tokens[i] of w.  Autograd sums the gradient of a repeated id over its positions."""
    return w[tokens.reshape(-1)]


def _add_norm64(x: T, r: Optional[T], w: T, eps: float) -> Tuple[T, T]:
    """(h, y): h = x + r (h = x for r None) is the residual stream and y = rmsnorm(h) * w the branch input.
    Nothing is rounded here (:func:`add_rmsnorm_ref` rounds h, as the kernel does)."""
    h = x if r is None else x + r
    return h, rmsnorm_ref(h, w, eps)[0]


def model_ref64(cfg, weights: Dict[str, T], tokens: T, labels: T, cos: T, sin: T,
                ignore_index: int = -100) -> Tuple[float, Dict[str, T]]:
    """(loss, {name: gradient}) of the Llama training step (``models/llama.py``) in float64.

    ``weights``: name -> tensor for every name of ``cfg.param_shapes()`` (the model's bf16 weights; their
    float64 copies are the leaves), ``tokens`` / ``labels`` [B, S], ``cos`` / ``sin`` the fp32 RoPE tables.
    Embedding, RMSNorm, the QKV projection, RoPE and split, causal GQA softmax attention, the residuals,
    SwiGLU, the final norm and head, and the mean cross-entropy over the labels that are not
    ``ignore_index``, composed of the float64 definitions of this file and of ``attention_ref.py``.
    No intermediate is rounded and the gradients are autograd's: no GPU, no project kernel."""
    w = {n: _f64(weights[n].detach()).clone().requires_grad_(True) for n, _ in cfg.param_shapes()}
    tokens, labels = tokens.detach().cpu().long(), labels.detach().cpu().long()
    B, S = tokens.shape
    H, Hkv, Dh = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
    x, r = _embed64(w["tok_emb"], tokens), None
    for i in range(cfg.n_layers):
        x, h = _add_norm64(x, r, w[f"l{i}.attn_norm"], cfg.norm_eps)
        q, k, v, _, _ = rope_split_ref64(h @ w[f"l{i}.wqkv"].t(), cos, sin, B, S, H, Hkv, Dh)
        o = attn_fwd_ref64(q, k, v, Dh ** -0.5)[0].reshape(B * S, H * Dh)
        x, h = _add_norm64(x, o @ w[f"l{i}.wo"].t(), w[f"l{i}.ffn_norm"], cfg.norm_eps)
        r = swiglu_ref64(h @ w[f"l{i}.w13"].t())[0] @ w[f"l{i}.w2"].t()
    _, h = _add_norm64(x, r, w["norm"], cfg.norm_eps)
    rows, _ = xent_ref64(h @ w["lm_head"].t(), labels, ignore_index)
    loss = rows.sum() / (labels != ignore_index).sum().clamp_min(1)
    names = list(w)
    grads = torch.autograd.grad(loss, [w[n] for n in names])
    return float(loss.detach()), dict(zip(names, grads))
