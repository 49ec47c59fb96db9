"""float64 CPU references of the causal GQA flash attention kernels (``csrc/ops/attention.hip``).

Plain ``torch.float64`` on the CPU: no GPU, no HIP kernel.  Each function takes the kernel's own inputs
(bf16 q [B, H, S, D], k / v [B, Hkv, S, D], dout / out [B, S, H, D], fp32 lse2 [B, H, S]) and returns
the EXACT value of what the kernel computes from them, before its single output rounding, plus
condition magnitudes: the sums of the absolute values of the terms the kernel adds.

The constants are the fp32 numbers the kernels receive (:func:`kernel_constants`): the exponent factor
``c = fp32(scale * log2(e))`` (scores enter the exponential in log2 units) and ``fp32(scale)`` (the
final factor of dQ and dK).  So the forward is softmax with the factor c ln 2, not ``scale``; the two
differ by one fp32 rounding, which is the kernel's definition and therefore the reference's.

The acceptance rule (``tests/test_attention_ref.py`` implements it, ``tests/test_gpu_attention_exact.py``
applies it to the kernels).  Every output element is one fp32 chain of N products, each product having
one factor that the kernel rounds to bf16 before the MFMA (the "pack" of P or dS, unit roundoff
u = 2^-8), rounded once to bf16 at the end:

    |got - value| <= ulp_bf16(value) / 2 + (u + 2^-24 (N + 64)) * cond  [+ 2^-16 * cond2 for dq, dk]

  * ``ulp_bf16(value) / 2``: the output rounding, to nearest.
  * ``u * cond``: every term P_qk V_kd (O), P_qk dO_qd (dV), dS_qk K_kd (dQ), dS_qk Q_qd (dK) carries the
    relative error u of its packed factor; their magnitudes sum to cond.  In the forward the pack holds
    p = 2^(s - m) with the slack-8 running max m, not P, but rounding to bf16 is scale-free up to the
    exponent, and l sums the UNROUNDED p, so the error of O = sum(pack(p) V) / l is u * sum(p |V|) / l.
  * ``2^-24 (N + 64) * cond``: the fp32 chain.  N additions of the accumulator (N = the visible keys of
    the row for O and dQ; G times the visible queries of the key for dV and dK, G = H / Hkv), and 64 for
    everything that happens once per term or per row: the score's own 128-term fp32 chain seen through
    the exponential (2^-24 * 128 * |s c| ln 2 relative, |s c| <= 64), the fma and v_exp_f32 (1 ulp), the
    O / l rescales (one multiply per moved max, at most S / 64), 1 / l, the row sum l, the final
    multiply by 1 / l or scale.
  * ``2^-16 * cond2`` (dq, dk only): dS = P (dP - delta) cancels.  dP is a 128-term fp32 chain over
    |dO||V|, delta a 128-term chain over |dO * O|; both errors are at most 2^-24 * 128 = 2^-17 of
    those magnitudes, doubled.  condS = P (|dO||V|^T + rowsum|dO * O|) is that magnitude per score and
    cond2 its product sum with |K| (dq) or |Q| (dk).  The exponent's fp32 argument c S - lse2 is
    rounded at magnitude <= 64 (every case asserts |lse2| <= 64): 2^-24 * 64 * ln 2 < 2^-18 relative
    in P, inside this term because condS >= |dS|.

``lse2`` (fp32) passes iff |got - value| <= 2^-15 + 2^-22 |value|: the absolute slack
``models/llama_ref.py`` gives the cross-entropy lse (the relative error of the row sum l is the
absolute error of its logarithm), plus four fp32 roundings of the stored value (m, log2 l, their sum,
the running max's own product with c).

Backward references take ``out`` and ``lse2`` as arguments, as the kernel does: they are exact for
whatever forward values a test passes, and a forward fault cannot reach a backward comparison.
"""
from __future__ import annotations

from typing import Tuple

import torch

from .mnist_ref import bf16_round

__all__ = ["bf16_round", "kernel_constants", "attn_fwd_ref64", "attn_bwd_ref64"]

T = torch.Tensor
LOG2E = 1.4426950408889634


def kernel_constants(scale: float) -> Tuple[float, float]:
    """(c, scale32): ``(float)(scale * 1.4426950408889634)`` and ``(float)scale``, as the host code computes them."""
    c = float(torch.tensor(float(scale) * LOG2E, dtype=torch.float64).to(torch.float32))
    return c, float(torch.tensor(float(scale), dtype=torch.float64).to(torch.float32))


def _f64(t: T) -> T:
    return t.cpu().to(torch.float64)  # differentiable: tests/test_attention_ref.py takes autograd through it


def _grouped(q: T, k: T, v: T):
    """q -> [B, Hkv, G, S, D], k / v -> [B, Hkv, 1, S, D] (q-head h reads kv-head h // G)."""
    q, k, v = _f64(q), _f64(k), _f64(v)
    B, H, S, D = q.shape
    Hkv = k.shape[1]
    assert H % Hkv == 0 and k.shape == v.shape == (B, Hkv, S, D)
    return q.view(B, Hkv, H // Hkv, S, D), k.view(B, Hkv, 1, S, D), v.view(B, Hkv, 1, S, D)


def _scores2(q: T, k: T, c: float) -> T:
    """c QK^T in log2 units, [B, Hkv, G, S, S], -inf above the diagonal."""
    S = q.shape[-2]
    s2 = c * (q @ k.transpose(-1, -2))
    return s2.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))


def _token_major(t: T) -> T:
    """[B, Hkv, G, S, D] -> [B, S, H, D]."""
    B, Hkv, G, S, D = t.shape
    return t.reshape(B, Hkv * G, S, D).transpose(1, 2).contiguous()


def _head_major(t: T, Hkv: int) -> T:
    """[B, S, H, D] -> [B, Hkv, G, S, D]."""
    B, S, H, D = t.shape
    return t.transpose(1, 2).reshape(B, Hkv, H // Hkv, S, D)


def attn_fwd_ref64(q: T, k: T, v: T, scale: float) -> Tuple[T, T, T]:
    """(o [B, S, H, D], lse2 [B, H, S], cond_o [B, S, H, D]).

    P = softmax over the visible keys of c QK^T (base 2), o = P V, lse2 = log2 sum_k 2^(c q.k),
    cond_o[q, d] = sum_k P_qk |V_kd|."""
    c, _ = kernel_constants(scale)
    qg, kg, vg = _grouped(q, k, v)
    B, Hkv, G, S, D = qg.shape
    s2 = _scores2(qg, kg, c)
    m = s2.amax(-1, keepdim=True)
    p = torch.exp2(s2 - m)
    l = p.sum(-1, keepdim=True)
    lse2 = (m + torch.log2(l)).squeeze(-1).reshape(B, Hkv * G, S)
    p = p / l
    return _token_major(p @ vg), lse2, _token_major(p @ vg.abs())


def attn_bwd_ref64(dout: T, q: T, k: T, v: T, out: T, lse2: T, scale: float):
    """(dq, dk, dv, cond_dq, cond_dk, cond_dv, cond2_dq, cond2_dk), dq [B, H, S, D], dk / dv [B, Hkv, S, D].

    A function of the ``out`` and ``lse2`` it is given.  With P = 2^(c QK^T - lse2) on the visible keys,
    delta = rowsum(dout * out), dP = dout V^T, dS = P (dP - delta) and sums over the GQA group g:

        dv = sum_g P^T dout             cond_dv = sum_g P^T |dout|
        dk = scale sum_g dS^T Q         cond_dk = scale sum_g |dS|^T |Q|     cond2_dk = scale sum_g condS^T |Q|
        dq = scale dS K                 cond_dq = scale |dS| |K|             cond2_dq = scale condS |K|

    condS = P (|dout| |V|^T + rowsum|dout * out|): the cancellation in dP - delta."""
    c, sc = kernel_constants(scale)
    qg, kg, vg = _grouped(q, k, v)
    B, Hkv, G, S, D = qg.shape
    do, o = _head_major(_f64(dout), Hkv), _head_major(_f64(out), Hkv)
    l2 = _f64(lse2).view(B, Hkv, G, S, 1)
    p = torch.exp2(_scores2(qg, kg, c) - l2)  # exactly 0 above the diagonal
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (do @ vg.transpose(-1, -2) - delta)
    conds = p * (do.abs() @ vg.abs().transpose(-1, -2) + (do * o).abs().sum(-1, keepdim=True))
    pt, dst, cst = p.transpose(-1, -2), ds.transpose(-1, -2), conds.transpose(-1, -2)
    H = Hkv * G
    dv, cond_dv = (pt @ do).sum(2), (pt @ do.abs()).sum(2)
    dk, cond_dk, cond2_dk = sc * (dst @ qg).sum(2), sc * (dst.abs() @ qg.abs()).sum(2), sc * (cst @ qg.abs()).sum(2)
    dq, cond_dq, cond2_dq = sc * (ds @ kg), sc * (ds.abs() @ kg.abs()), sc * (conds @ kg.abs())
    hm = lambda t: t.reshape(B, H, S, D)  # noqa: E731
    return hm(dq), dk, dv, hm(cond_dq), cond_dk, cond_dv, hm(cond2_dq), cond2_dk
