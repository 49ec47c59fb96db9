"""float64 CPU reference of the AdamW update body (``adam8_update``, ``csrc/common/adamw_update.h``).

Plain ``torch.float64`` on the CPU: no GPU, no HIP kernel.  :func:`adamw_step_ref` takes the kernel's own
inputs (fp32 master, m and v, the bf16 or fp32 gradient, the eight hyper-parameters) and returns the EXACT
value of what the kernel's expressions give from them, before any fp32 rounding::

    gr      = g * grad_scale
    m'      = beta1 * m + (1 - beta1) * gr
    v'      = beta2 * v + (1 - beta2) * gr * gr
    master' = master - lr * ((m' / bias_c1) / (sqrt(v' / bias_c2) + eps) + weight_decay * master)

``1 - beta`` is taken from the fp32 ``beta`` in float64; the kernel's own rounding of it belongs to the slack
of the comparison.  With each value comes a condition magnitude ``cond``: the sum of the magnitudes of the
terms the fp32 arithmetic adds.  A kernel's fp32 error is a small multiple of 2^-24 * cond, and for the master
``cond`` is the magnitude of the STEP, not of the master: ``tests/test_optim_ref.py`` accepts a new master iff

    |got - master'| <= ulp_fp32(master') / 2 + slack * cond

so a step that is wrong by a few parts in a million of itself cannot pass, however large the master it is
subtracted from.  :func:`dev_hyper_ref` derives what the graph-capturable form (``hyper<true>`` of
``csrc/ops/adamw.hip``) derives on the device: the bias corrections from the step count, and the clipping
factor from the exact sum of squares of the gradient.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Union

import torch

from .mnist_ref import bf16_round

__all__ = ["bf16_round", "AdamWRef", "adamw_step_ref", "dev_hyper_ref", "sum_of_squares_ref"]

T = torch.Tensor


class AdamWRef(NamedTuple):
    """Exact new m, v and master (float64) and the condition magnitude of each."""
    m: T
    v: T
    master: T
    cond_m: T
    cond_v: T
    cond_master: T


def _f64(t: T) -> T:
    return t.detach().cpu().to(torch.float64)


def _hyper64(hp8: Union[T, Sequence[float]]) -> Sequence[float]:
    """The eight values as Python floats without a rounding of their own: an fp32 tensor gives the stored
    values exactly, a sequence of floats (:func:`dev_hyper_ref`) is taken as it is."""
    vals = _f64(hp8).tolist() if isinstance(hp8, torch.Tensor) else [float(x) for x in hp8]
    assert len(vals) >= 8, "hp8 = [lr, beta1, beta2, eps, weight_decay, grad_scale, bias_c1, bias_c2]"
    return vals[:8]


def adamw_step_ref(master: T, m: T, v: T, g: T, hp8: Union[T, Sequence[float]]) -> AdamWRef:
    """One AdamW step (decoupled weight decay) of every element, exact in float64.

        cond_m      = |beta1 m| + |(1 - beta1) g grad_scale|
        cond_v      = |beta2 v| + (1 - beta2) (g grad_scale)^2          (= v' for v >= 0)
        cond_master = lr (cond_m / bias_c1 / (sqrt(v' / bias_c2) + eps) + weight_decay |master|)
    """
    lr, b1, b2, eps, wd, gs, bc1, bc2 = _hyper64(hp8)
    p, m, v, gr = _f64(master), _f64(m), _f64(v), _f64(g) * gs
    t1, t2 = b1 * m, (1.0 - b1) * gr
    m2, cm = t1 + t2, t1.abs() + t2.abs()
    u1, u2 = b2 * v, (1.0 - b2) * gr * gr
    v2, cv = u1 + u2, u1.abs() + u2.abs()
    den = (v2 / bc2).sqrt() + eps
    p2 = p - lr * ((m2 / bc1) / den + wd * p)
    cp = abs(lr) * ((cm / abs(bc1)) / den + abs(wd) * p.abs())
    return AdamWRef(m2, v2, p2, cm, cv, cp)


def sum_of_squares_ref(g: T) -> float:
    """The sum of squares of the gradient's values in float64: every square of a bf16 or fp32 value is exact
    there, and the pairwise sum of n of them is good to about log2(n) 2^-53 relative, 2^28 times finer than an
    fp32 rounding."""
    x = _f64(g).reshape(-1)
    return float((x * x).sum())


def dev_hyper_ref(hp_dev: Union[T, Sequence[float]], t: float, sumsq: Optional[float]) -> Sequence[float]:
    """The host form's eight values, in float64, that ``hyper<true>`` derives from the device form
    ``[lr, beta1, beta2, eps, weight_decay, grad_scale, clip_norm (<= 0: off), -]``, the step count ``t`` (after
    this step) and the exact sum of squares of the gradient (``None``: no partials were given, so no clipping):

        norm = sqrt(sumsq) grad_scale;  grad_scale' = grad_scale min(1, clip / (norm + 1e-6))
        bias_c1 = 1 - beta1^t;  bias_c2 = 1 - beta2^t

    ``1e-6`` is the kernel's fp32 constant ``1e-6f``."""
    vals = _f64(hp_dev).tolist() if isinstance(hp_dev, torch.Tensor) else [float(x) for x in hp_dev]
    lr, b1, b2, eps, wd, gs, clip = vals[:7]
    if sumsq is not None and clip > 0.0:
        norm = math.sqrt(sumsq) * gs
        f = clip / (norm + float(torch.tensor(1e-6, dtype=torch.float32)))
        gs = gs * (1.0 if f > 1.0 else f)  # not min(): a NaN norm passes, as in hyper<true>
    return [lr, b1, b2, eps, wd, gs, 1.0 - b1 ** float(t), 1.0 - b2 ** float(t)]
