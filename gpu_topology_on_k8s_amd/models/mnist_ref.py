"""float64 CPU references of the MNIST HIP kernels (``csrc/ops/mnist_conv.hip``).

Plain torch/numpy, no HIP kernel and no library convolution: the convolutions are nine shifted
matrix products, the pooling an explicit four-way stack, the dropout mask the kernels' counter-based
hash recomputed with numpy.  Tensors use the kernels' layouts, so a test compares them directly:
x [B,28,28]; h1 [B,26,26,32] (NHWC); pooled / code / dp [B,12,12,64]; conv1.w [32,3,3];
conv2.w [64,3,3,32] (co, ky, kx, ci).

The kernels multiply bf16 operands and accumulate in fp32, and round an output once (bf16, round to
nearest even).  With small-integer inputs and a power-of-two dropout scale every intermediate is an
integer below 2^24, so the kernels' result does not depend on their summation order and must equal
``bf16_round`` of these references bit for bit (``tests/test_gpu_mnist_kernels.py``);
``conv_exactness_bound`` is the condition.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from .mnist import _mix32

__all__ = ["dropout_keep", "bf16_round", "conv_stack_ref", "conv_stack_grads_ref", "conv_exactness_bound",
           "relu_dropout_ref", "relu_dropout_bwd_ref", "xent10_ref", "xent10_bwd_ref", "HEAD_SEED_XOR"]

HEAD_SEED_XOR = 0x5BD1E995  # the head's dropout hashes with ``drop_seed ^ HEAD_SEED_XOR``
_TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]


def dropout_keep(seed: int, step: float, n: int, p: float) -> torch.Tensor:
    """keep[i] = (hash3(seed, step, i) >> 8) >= round(p * 2^24) for i in [0, n): bool [n].
    hash3(a, b, c) = mix32(a ^ mix32(b ^ mix32(c))); ``seed`` mod 2^32, ``step`` as uint32(float).
    Conv stack: i = win * 64 + co with win in [B,12,12] order (seed = ``drop_seed``); head: i is the
    flat index of [B,128] (seed = ``drop_seed ^ HEAD_SEED_XOR``)."""
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout probability must be in [0, 1)")
    thresh = np.uint32(int(p * 16777216.0 + 0.5))
    a = np.array([int(seed) & 0xFFFFFFFF], dtype=np.uint32)
    b = np.array([int(float(step)) & 0xFFFFFFFF], dtype=np.uint32)
    with np.errstate(over="ignore"):
        h = _mix32(a ^ _mix32(b ^ _mix32(np.arange(n, dtype=np.uint32))))
    return torch.from_numpy((h >> np.uint32(8)) >= thresh)


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16, round to nearest even (what the kernels' ``(__bf16)f`` does).  The value passes
    through fp32 first, as in the kernels; for integers below 2^24 that step is exact."""
    return t.to(torch.float32).to(torch.bfloat16)


def _conv1(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor) -> torch.Tensor:
    z = b1.view(1, 1, 1, -1).expand(x.shape[0], 26, 26, -1).clone()
    for ky, kx in _TAPS:
        z += x[:, ky:ky + 26, kx:kx + 26, None] * w1[:, ky, kx]
    return z


def _conv2(h1: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    """conv2 without bias: [B,24,24,64]."""
    B = h1.shape[0]
    z = torch.zeros(B * 576, w2.shape[0], dtype=h1.dtype)
    for ky, kx in _TAPS:
        z += h1[:, ky:ky + 24, kx:kx + 24, :].reshape(B * 576, -1) @ w2[:, ky, kx, :].t()
    return z.view(B, 24, 24, -1)


def _windows(z: torch.Tensor) -> torch.Tensor:
    """[B,24,24,C] -> [4,B,12,12,C], the 2x2 window's pixels in the kernels' order q = 2*(y&1) + (x&1)."""
    return torch.stack([z[:, 0::2, 0::2], z[:, 0::2, 1::2], z[:, 1::2, 0::2], z[:, 1::2, 1::2]])


def conv_stack_ref(x, w1, b1, w2, b2, keep, p: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """conv1 + ReLU -> conv2 -> 2x2 max-pool -> + bias -> ReLU -> dropout, in float64.

    Returns (h1 [B,26,26,32], pooled [B,12,12,64], code uint8 [B,12,12,64]) with
    code = argmax | pos << 2 | keep << 3: argmax is the FIRST maximum of the window in the order
    q = 2*(y&1) + (x&1) (the kernels compare with a strict ``>``), pos = max + bias > 0, and
    pooled = (max + bias) / (1 - p) where pos and keep, else 0.  ``keep``: bool, B*9216 elements."""
    x, w1, b1, w2, b2 = (t.detach().to(torch.float64).cpu() for t in (x, w1, b1, w2, b2))
    B = x.shape[0]
    x = x.reshape(B, 28, 28)
    h1 = _conv1(x, w1.reshape(32, 3, 3), b1).clamp_min(0.0)
    win = _windows(_conv2(h1, w2.reshape(64, 3, 3, 32)))
    m, am = win[0].clone(), torch.zeros(win[0].shape, dtype=torch.uint8)
    for q in range(1, 4):
        better = win[q] > m
        m = torch.where(better, win[q], m)
        am = torch.where(better, torch.full_like(am, q), am)
    m = m + b2
    pos = m > 0
    keep = keep.reshape(m.shape).cpu().bool()
    pooled = torch.where(pos & keep, m / (1.0 - p), torch.zeros_like(m))
    code = am | (pos.to(torch.uint8) << 2) | (keep.to(torch.uint8) << 3)
    return h1, pooled, code


def conv_stack_grads_ref(x, h1, w2, code, dp, p: float, with_intermediates: bool = False):
    """Backward of ``conv_stack_ref`` from the pooled gradient ``dp`` [B,12,12,64], in float64.

    dy2 is dp / (1 - p) at the window's argmax pixel where pos and keep (code & 12 == 12), else 0;
    conv1's ReLU mask is h1 > 0.  Returns (conv1.w grad [32,3,3], conv1.b grad [32], conv2.w grad
    [64,3,3,32], conv2.b grad [64]); with ``with_intermediates`` also {"dy2": [B,24,24,64],
    "dz1": [B,26,26,32]}."""
    x, h1, w2, dp = (t.detach().to(torch.float64).cpu() for t in (x, h1, w2, dp))
    B = h1.shape[0]
    x, w2, code = x.reshape(B, 28, 28), w2.reshape(64, 3, 3, 32), code.cpu().reshape(B, 12, 12, 64)
    live = (code & 12) == 12
    d = torch.where(live, dp.reshape(B, 12, 12, 64) / (1.0 - p), torch.zeros((), dtype=torch.float64))
    dy2 = torch.zeros(B, 24, 24, 64, dtype=torch.float64)
    for q in range(4):
        dy2[:, (q >> 1)::2, (q & 1)::2] = torch.where((code & 3) == q, d, torch.zeros((), dtype=torch.float64))
    dyf = dy2.reshape(B * 576, 64)
    gw2 = torch.empty(64, 3, 3, 32, dtype=torch.float64)
    dh1 = torch.zeros(B, 26, 26, 32, dtype=torch.float64)
    for ky, kx in _TAPS:
        gw2[:, ky, kx, :] = dyf.t() @ h1[:, ky:ky + 24, kx:kx + 24, :].reshape(B * 576, 32)
        dh1[:, ky:ky + 24, kx:kx + 24, :] += (dyf @ w2[:, ky, kx, :]).view(B, 24, 24, 32)
    gb2 = dyf.sum(0)
    dz1 = torch.where(h1 > 0, dh1, torch.zeros((), dtype=torch.float64))
    gw1 = torch.empty(32, 3, 3, dtype=torch.float64)
    for ky, kx in _TAPS:
        gw1[:, ky, kx] = (dz1 * x[:, ky:ky + 26, kx:kx + 26, None]).sum((0, 1, 2))
    gb1 = dz1.sum((0, 1, 2))
    if with_intermediates:
        return gw1, gb1, gw2, gb2, {"dy2": dy2, "dz1": dz1}
    return gw1, gb1, gw2, gb2


def conv_exactness_bound(x, w1, b1, w2, b2, h1, dy2, dz1, p: float, preload: float = 0.0) -> Dict[str, float]:
    """Upper bounds on the magnitude of every partial sum the conv kernels can form, whatever their
    summation order (a sum's partial sums are bounded by the sum of its terms' magnitudes).  All below
    2^24 with integer inputs and an integer 1/(1-p) = every fp32 intermediate is an exact integer."""
    mx = lambda t: float(t.detach().to(torch.float64).abs().max())  # noqa: E731
    scale = 1.0 / (1.0 - p)
    pre = 288 * mx(h1) * mx(w2)
    return {
        "h1": mx(b1) + 9 * mx(w1) * mx(x),
        "pooled": (pre + mx(b2)) * scale,
        "dz1": 576 * mx(dy2) * mx(w2),
        "conv2.w/b grad": float(dy2.abs().sum((0, 1, 2)).max()) * max(1.0, mx(h1)) + preload,
        "conv1.w/b grad": float(dz1.abs().sum((0, 1, 2)).max()) * max(1.0, mx(x)) + preload,
    }


# ------------------------------------------------------------------------------ classifier head
def relu_dropout_ref(h, keep, p: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y, mask): mask = keep and h > 0 (uint8), y = h / (1 - p) where mask else 0.  h [B,128]."""
    h = h.detach().to(torch.float64).cpu()
    m = (h > 0) & keep.reshape(h.shape).cpu().bool()
    return torch.where(m, h / (1.0 - p), torch.zeros_like(h)), m.to(torch.uint8)


def relu_dropout_bwd_ref(dy, mask, p: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dh, fc1 bias gradient): dh = dy / (1 - p) where mask else 0; the bias gradient is the column
    sums of the bf16-rounded dh (the dh the weight-gradient GEMM sees), as in the kernel."""
    dy = dy.detach().to(torch.float64).cpu()
    dh = torch.where(mask.cpu().bool(), dy / (1.0 - p), torch.zeros_like(dy))
    return dh, bf16_round(dh).to(torch.float64).sum(0)


def xent10_ref(logits, labels) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean softmax cross-entropy, dlog = (softmax - onehot) / B) in float64.  logits [B,10]."""
    z = logits.detach().to(torch.float64).cpu()
    labels = labels.cpu()
    z = z - z.max(1, keepdim=True).values
    e = z.exp()
    s = e.sum(1, keepdim=True)
    rows = torch.arange(z.shape[0])
    loss = (s.log().squeeze(1) - z[rows, labels]).mean()
    d = e / s
    d[rows, labels] -= 1.0
    return loss, d / z.shape[0]


def xent10_bwd_ref(dlog, g: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dlogits = g * dlog, fc2 bias gradient = column sums of the bf16-rounded dlogits)."""
    d = dlog.detach().to(torch.float64).cpu() * float(g)
    return d, bf16_round(d).to(torch.float64).sum(0)
