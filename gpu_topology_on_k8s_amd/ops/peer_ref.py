"""CPU reference of the K7 peer all-reduce (kernels ``csrc/probe/peer_allreduce.h``, driver
``csrc/probe/peer_driver.h``), pure numpy.

The kernels sum every element in fp32 in member order, ``((x0 + x1) + x2) + ...``, multiply once by
the call's scale and round once, so a sequential numpy sum reproduces their result bit for bit; :func:`peer_slices` is the driver's
slice plan of the two-shot algorithm.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

__all__ = ["ELEM", "peer_slices", "bf16_round", "bf16_to_f32", "bits", "out_dtype_of", "allreduce_ref", "reduce_scatter_ref"]

ELEM = {"bf16": 2, "fp32": 4}  # bytes per element


def peer_slices(n_vec: int, k: int) -> List[Tuple[int, int]]:
    """``[first, end)`` in 16-byte vectors of each of ``k`` members' slice of ``n_vec`` vectors:
    ``per = ceil(n_vec / k)`` vectors each, the last one ragged, trailing ones possibly empty."""
    if k < 1 or n_vec < 0:
        raise ValueError("k >= 1 and n_vec >= 0")
    per = -(-n_vec // k)
    return [(min(n_vec, s * per), min(n_vec, (s + 1) * per)) for s in range(k)]


def bf16_round(x: np.ndarray) -> np.ndarray:
    """bf16 bit patterns (uint16) of finite float32 ``x``, round to nearest even on the bit pattern."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((b + (np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)).astype(np.uint16)


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    """float32 values of bf16 bit patterns (uint16)."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bits(a: np.ndarray) -> np.ndarray:
    """The one bit-pattern view of a result: bf16 patterns (uint16) as they are, float32 as uint32."""
    return a.view(np.uint16 if a.dtype == np.uint16 else np.uint32)


def out_dtype_of(dtype: str, out_dtype: Optional[str]) -> str:
    """The output dtype of a reduce of ``dtype`` inputs (none: ``dtype``), or ``ValueError``."""
    if dtype not in ELEM:
        raise ValueError(f"dtype must be bf16|fp32, got {dtype!r}")
    out = dtype if out_dtype is None else out_dtype
    if out not in ELEM:
        raise ValueError(f"out_dtype must be bf16|fp32, got {out!r}")
    if dtype == "fp32" and out == "bf16":
        raise ValueError("fp32 inputs reduce to fp32 only")
    return out


def allreduce_ref(inputs: Sequence[np.ndarray], dtype: str, out_dtype: Optional[str] = None, scale: float = 1.0) -> np.ndarray:
    """What every member holds after the all-reduce of ``inputs`` (finite values; uint16 bit patterns
    for ``bf16``, float32 for ``fp32``): a sequential fp32 sum in member order, one fp32 multiply by
    ``scale`` (rounded to fp32 first, as the kernel's argument is), then one rounding to ``out_dtype``
    (none: ``dtype``; ``fp32`` of ``bf16`` inputs keeps the fp32 sum)."""
    out = out_dtype_of(dtype, out_dtype)
    if not inputs:
        raise ValueError("no inputs")
    wide = [bf16_to_f32(a) if dtype == "bf16" else np.ascontiguousarray(a, dtype=np.float32) for a in inputs]
    acc = wide[0].copy()
    for x in wide[1:]:
        acc = (acc + x).astype(np.float32)
    acc = (acc * np.float32(scale)).astype(np.float32)
    return bf16_round(acc) if out == "bf16" else acc


def reduce_scatter_ref(inputs: Sequence[np.ndarray], dtype: str, out_dtype: Optional[str] = None,
                       scale: float = 1.0) -> List[np.ndarray]:
    """Rank r's piece of the reduce-scatter of ``inputs``: the elements of slice r of :func:`peer_slices`
    over the input's vectors (the last piece ends at the count, trailing pieces may be empty).  The
    pieces concatenate to :func:`allreduce_ref`."""
    full = allreduce_ref(inputs, dtype, out_dtype, scale)
    per = 16 // ELEM[dtype]
    count = int(full.shape[0])
    return [full[min(count, a * per):min(count, b * per)] for a, b in peer_slices(-(-count // per), len(inputs))]
