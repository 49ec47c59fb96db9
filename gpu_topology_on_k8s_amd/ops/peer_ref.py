"""CPU reference of the K7 peer all-reduce (kernels ``csrc/probe/peer_allreduce.h``, driver
``csrc/probe/peer_driver.h``), pure numpy.

The kernels sum every element in fp32 in member order, ``((x0 + x1) + x2) + ...``, multiply once by
the call's scale and round once, so a sequential numpy sum reproduces their result bit for bit; :func:`peer_slices` is the driver's
slice plan of the two-shot algorithm.

The references cover all of IEEE 754, not finite normal values alone.  numpy's fp32 add and multiply are
IEEE: subnormals are kept, ``Inf + -Inf`` and anything with a NaN give NaN, ``-0 + -0 = -0``.  A result
is compared with its reference by :func:`mismatches`: where the reference is NaN the result must be a
NaN (of any sign and payload: which payload an add or a rounding keeps is the hardware's choice), and
every other element, infinities, subnormals and signed zeros included, must have the reference's bits.

The fp8 wire (``csrc/probe/peer_q8.h``) has its reference here too: :func:`q8_quantize_ref` packs one
rank's input into OCP e4m3fn codes with one power-of-two scale per 32 elements, and
:func:`allreduce_q8_ref` sums the dequantised values exactly as :func:`allreduce_ref` sums the inputs.
:func:`allreduce_q8x2_ref` is the two-shot whose gather phase is packed too (``wire="fp8x2"``): the scaled fp32 sum
goes through the same block rule once more, and every member takes its result from that packed form.

Error feedback (:func:`q8_quantize_ef_ref`, :func:`allreduce_q8_ef_ref`, :func:`reduce_scatter_q8_ef_ref`): a
sender adds what its last packing dropped, a float32 *residual* per element, to what it packs next, so over
any number of calls the sum of what it sent differs from the sum of what it was given by the last residual
alone.

The ZeRO-1 step (``csrc/probe/peer_zero1.h``): :func:`adamw_ref` is the AdamW update body of
``csrc/common/adamw_update.h`` in numpy, and :func:`zero1_step_ref` is a whole step, the reduce-scatter's fp32
mean of every rank's slice fed to that update and the new bf16 weights of all slices side by side.  With
``clip_norm`` the step clips by the global norm of that mean: :func:`zero1_sqnorm_ref` is its sum of squares in
float64 and :func:`clip_grad_scale` the one formula that turns it into the norm and the update's ``grad_scale``,
for the reference and for both backends of the communicator.  :func:`zero1_accumulate_ref` is the fp32 gradient
accumulator of a batch split into micro-batches, and ``accumulated=`` of :func:`zero1_step_ref` the step that ends it.

How a launch walks its range: :func:`launch_walk` mirrors ``peer_reduce_range`` (the walk of every K7 kernel that takes
member buckets) and :data:`LAUNCH_U` lists the positions per lane of each of those kernels per bucket, so a test can
say on the CPU which loops a count and a grid reach.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

__all__ = ["ELEM", "peer_slices", "bf16_round", "bf16_to_f32", "bits", "out_dtype_of", "allreduce_ref", "reduce_scatter_ref",
           "is_nan_bits", "mismatches", "Q8_BLOCK", "Q8_EXP_MIN", "Q8_EXP_MAX", "q8_blocks", "q8_slices", "q8_quantize_ref", "q8_dequantize_ref",
           "allreduce_q8_ref", "reduce_scatter_q8_ref", "allreduce_q8x2_ref", "q8_quantize_ef_ref", "allreduce_q8_ef_ref",
           "reduce_scatter_q8_ef_ref", "adamw_ref", "zero1_slices", "zero1_step_ref", "zero1_accumulate_ref", "clip_grad_scale", "zero1_sqnorm_ref",
           "LAUNCH_BLOCK", "LAUNCH_BUCKETS", "LAUNCH_U", "launch_u", "launch_walk"]

ELEM = {"bf16": 2, "fp32": 4}  # bytes per element


def peer_slices(n_vec: int, k: int) -> List[Tuple[int, int]]:
    """``[first, end)`` in 16-byte vectors of each of ``k`` members' slice of ``n_vec`` vectors:
    ``per = ceil(n_vec / k)`` vectors each, the last one ragged, trailing ones possibly empty."""
    if k < 1 or n_vec < 0:
        raise ValueError("k >= 1 and n_vec >= 0")
    per = -(-n_vec // k)
    return [(min(n_vec, s * per), min(n_vec, (s + 1) * per)) for s in range(k)]


def bf16_round(x: np.ndarray) -> np.ndarray:
    """bf16 bit patterns (uint16) of float32 ``x``.  Finite values and the infinities round to nearest
    even on the bit pattern, so a finite value at or above ``0x7F7F8000`` (bf16's maximum and half a unit
    in its last place) becomes Inf and an fp32 subnormal rounds into bf16's subnormals.  A NaN becomes
    the upper half of its own pattern with the quiet bit ``0x0040`` set: its sign and the top six payload
    bits are kept and the mantissa is never zero, so ``0x7F800001`` gives ``0x7FC0`` and ``0xFFFFFFFF``
    gives ``0xFFFF``; rounding the pattern would carry them into +Inf and -0."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((b + (np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)).astype(np.uint16)
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, ((b >> np.uint32(16)) | np.uint32(0x0040)).astype(np.uint16), r)


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    """float32 values of bf16 bit patterns (uint16)."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bits(a: np.ndarray) -> np.ndarray:
    """The one bit-pattern view of a result: bf16 patterns (uint16) as they are, float32 as uint32."""
    return a.view(np.uint16 if a.dtype == np.uint16 else np.uint32)


def is_nan_bits(a: np.ndarray) -> np.ndarray:
    """Which elements of a result (bf16 patterns as uint16, or float32) are NaN: the exponent all ones
    and a non-zero mantissa."""
    b = bits(a)
    if b.dtype == np.uint16:
        return (b & np.uint16(0x7FFF)) > np.uint16(0x7F80)
    return (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def mismatches(got: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """The indices at which ``got`` is not what ``ref`` demands, no element left out: where the reference
    is NaN ``got`` must be a NaN, everywhere else its bits must be the reference's.  Type and shape must
    be the reference's too (``ValueError``)."""
    if got.dtype != ref.dtype or got.shape != ref.shape:
        raise ValueError(f"result is {got.dtype}{got.shape}, reference {ref.dtype}{ref.shape}")
    want_nan = is_nan_bits(ref)
    return np.flatnonzero(np.where(want_nan, ~is_nan_bits(got), bits(got) != bits(ref)))


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
    """What every member holds after the all-reduce of ``inputs`` (any values, non-finite and
    subnormal ones included; uint16 bit patterns for ``bf16``, float32 for ``fp32``): a sequential fp32 sum
    in member order, one fp32 multiply by ``scale`` (rounded to fp32 first, as the kernel's argument is), then one rounding to ``out_dtype``
    (none: ``dtype``; ``fp32`` of ``bf16`` inputs keeps the fp32 sum)."""
    out = out_dtype_of(dtype, out_dtype)
    if not inputs:
        raise ValueError("no inputs")
    wide = [bf16_to_f32(a) if dtype == "bf16" else np.ascontiguousarray(a, dtype=np.float32) for a in inputs]
    acc = wide[0].copy()
    with np.errstate(over="ignore", invalid="ignore"):  # a sum that overflows is Inf and Inf - Inf is NaN: results, not faults
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


# -- the fp8 wire -------------------------------------------------------------------------------
Q8_BLOCK = 32                      # elements that share one scale
Q8_EXP_MIN, Q8_EXP_MAX = -100, 120  # the block exponent's clamp: 2^e, 2^-e and every dequantised value stay normal in fp32


def q8_blocks(count: int) -> int:
    """Blocks of 32 elements that hold ``count`` elements."""
    return -(-int(count) // Q8_BLOCK)


def q8_slices(n_blocks: int, k: int) -> List[Tuple[int, int]]:
    """:func:`peer_slices` applied to blocks: ``[first, end)`` in blocks of each of ``k`` members' slice."""
    return peer_slices(n_blocks, k)


def _e4m3_values() -> np.ndarray:
    """float32 value of every OCP e4m3fn code; 0x7f and 0xff, the format's only non-finite codes, are NaN."""
    c = np.arange(256)
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e.astype(np.float64) - 10))
    mag[(c & 0x7F) == 0x7F] = np.nan
    return (np.where(c & 0x80, -mag, mag)).astype(np.float32)


_E4M3 = _e4m3_values()


def q8_quantize_ref(x: np.ndarray, dtype: str, count: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The packed form of one rank's input ``x`` (uint16 bit patterns for ``bf16``, float32 for
    ``fp32``), of which the first ``count`` elements (none: all) are data and everything after them is
    zero: ``(codes uint8 [n_blocks * 32], exps int32 [n_blocks])``.

    Per block of 32 elements, ``e`` is the smallest integer with ``amax * 2^-e <= 448``, clamped to
    ``[-100, 120]`` (``amax == 0``: -100), and an element's code is ``x * 2^-e`` rounded to nearest even
    into e4m3fn, subnormal codes (quantum ``2^-9``) included.  A code carries its element's sign bit.

    Non-finite elements: the amax is taken over the block's elements that are not NaN, after the count's
    mask.  An Inf counts, so its block has ``e = 120``; a block whose data is all NaN has amax 0 and
    ``e = -100``.  A NaN or an Inf gets a code with ``code & 0x7F == 0x7F``, the format's NaN, since e4m3fn
    has no infinity; here it carries the element's sign bit, but that bit is unspecified and a comparison
    masks it.  The block's finite elements are coded by the ordinary rule with that ``e``, so a NaN
    costs its neighbours nothing and an Inf leaves them what ``2^120`` leaves."""
    if dtype not in ELEM:
        raise ValueError(f"dtype must be bf16|fp32, got {dtype!r}")
    v = bf16_to_f32(x) if dtype == "bf16" else np.ascontiguousarray(x, dtype=np.float32)
    count = int(v.shape[0]) if count is None else int(count)
    if not 0 <= count <= v.shape[0]:
        raise ValueError("count past the end of x")
    nb = q8_blocks(count)
    full = np.zeros(nb * Q8_BLOCK, np.float32)
    full[:count] = v[:count]
    special = ~np.isfinite(full)
    mag = np.where(np.isnan(full), np.float32(0), np.abs(full))  # a NaN takes no part in the amax
    amax = mag.reshape(nb, Q8_BLOCK).max(axis=1) if nb else np.zeros(0, np.float32)
    m, ex = np.frexp(np.where(np.isinf(amax), np.float32(0), amax))  # amax = m * 2^ex, m in [0.5, 1); 448 = 0.875 * 2^9
    e = np.where(amax == 0, Q8_EXP_MIN, np.clip(ex - 9 + (m > 0.875), Q8_EXP_MIN, Q8_EXP_MAX))
    e = np.where(np.isinf(amax), Q8_EXP_MAX, e).astype(np.int32)
    y = np.ldexp(np.where(special, np.float32(0), full), -np.repeat(e, Q8_BLOCK)).astype(np.float32)  # exact, or too small for any code but 0
    a = np.abs(y).astype(np.float64)
    _, ea = np.frexp(a)  # a in [2^(ea - 1), 2^ea): three mantissa bits below the leading one
    quantum = np.ldexp(1.0, np.maximum(ea - 4, -9))
    r = np.rint(a / quantum) * quantum  # numpy's rint rounds halves to even
    mr, er = np.frexp(r)
    normal = r >= 2.0 ** -6
    code = np.where(normal, (er - 1 + 7) * 8 + np.rint((mr * 2 - 1) * 8), np.rint(r * 512)).astype(np.int64)
    code = np.where(special, 0x7F, np.minimum(code, 0x7E))  # no finite element reaches the minimum
    return (code | (np.signbit(full).astype(np.int64) << 7)).astype(np.uint8), e


def q8_dequantize_ref(codes: np.ndarray, exps: np.ndarray) -> np.ndarray:
    """float32 ``float(code) * 2^e`` of every element, exact: the values a member contributes to a sum.
    The codes ``0x7F`` and ``0xFF`` give NaN, so a NaN or an Inf that went in comes out as a NaN.  The one
    finite input that does not come out finite: under ``e = 120`` a magnitude of at least ``248 * 2^120``
    (fp32 ``0x7F780000``, bf16 ``0x7F78``) rounds to the code of 256, and ``256 * 2^120 = 2^128`` is Inf in
    fp32, in numpy's ``ldexp`` as in the kernel's multiply."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    exps = np.ascontiguousarray(exps).astype(np.int32)
    if codes.shape[0] != exps.shape[0] * Q8_BLOCK:
        raise ValueError("32 codes per exponent")
    with np.errstate(over="ignore"):  # 256 * 2^120 is Inf, see above
        return np.ldexp(_E4M3[codes], np.repeat(exps, Q8_BLOCK)).astype(np.float32)


def allreduce_q8_ref(inputs: Sequence[np.ndarray], dtype: str, out_dtype: Optional[str] = None, scale: float = 1.0) -> np.ndarray:
    """:func:`allreduce_ref` on the fp8 wire: every member's input, its own included, goes through
    :func:`q8_quantize_ref` and :func:`q8_dequantize_ref` first; then the same sequential fp32 sum in
    member order, the one multiply by ``scale`` and the one rounding to ``out_dtype``."""
    out = out_dtype_of(dtype, out_dtype)
    if not inputs:
        raise ValueError("no inputs")
    count = int(np.asarray(inputs[0]).shape[0])
    wide = [q8_dequantize_ref(*q8_quantize_ref(a, dtype))[:count] for a in inputs]
    acc = allreduce_ref(wide, "fp32", "fp32", scale)
    return bf16_round(acc) if out == "bf16" else acc


def reduce_scatter_q8_ref(inputs: Sequence[np.ndarray], dtype: str, out_dtype: Optional[str] = None,
                          scale: float = 1.0) -> List[np.ndarray]:
    """Rank r's piece of the reduce-scatter on the fp8 wire: the elements of slice r of :func:`q8_slices`
    over the input's blocks, clipped to the count.  The pieces concatenate to :func:`allreduce_q8_ref`."""
    full = allreduce_q8_ref(inputs, dtype, out_dtype, scale)
    count = int(full.shape[0])
    return [full[min(count, a * Q8_BLOCK):min(count, b * Q8_BLOCK)] for a, b in q8_slices(q8_blocks(count), len(inputs))]


def allreduce_q8x2_ref(inputs: Sequence[np.ndarray], dtype: str, out_dtype: Optional[str] = None, scale: float = 1.0) -> np.ndarray:
    """The two-shot all-reduce with both phases on the fp8 wire (``wire="fp8x2"``).  The fp32 result of
    :func:`allreduce_q8_ref` (the sum in member order of the members' dequantised packed forms, multiplied
    once by ``scale``, not rounded to bf16) is packed by :func:`q8_quantize_ref` unchanged: blocks counted
    from element 0 of the call, the same ``e``, clamp and NaN/Inf coding, elements at or past the count
    zero.  What every member holds, the slice's owner included, is the dequantised form of that, cast to
    ``out_dtype``.  The cast is exact: a dequantised value has at most 4 significant bits and ``e`` lies in
    ``[-100, 120]``, so bf16 holds it.

    An Inf in the sum comes out as NaN, since e4m3fn has no infinity, and a magnitude of at least
    ``248 * 2^120`` comes out Inf.  Per element the result is off from ``allreduce_q8_ref(..., "fp32")`` by at
    most ``amax / 14`` of its block of the scaled sum."""
    out = out_dtype_of(dtype, out_dtype)
    s = allreduce_q8_ref(inputs, dtype, "fp32", scale)
    back = q8_dequantize_ref(*q8_quantize_ref(s, "fp32"))[:s.shape[0]]
    return bf16_round(back) if out == "bf16" else back


# -- error feedback -----------------------------------------------------------------------------
def q8_quantize_ef_ref(x: np.ndarray, dtype: str, residual: np.ndarray,
                       count: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """:func:`q8_quantize_ref` with error feedback: ``(codes, exps, new_residual)``.  ``residual`` is float32,
    one value per element of the whole blocks the ``count`` (none: all of ``x``) covers, and so is ``new_residual``.

    1. ``v`` is ``x`` widened to fp32, elements at or past ``count`` zero, as in :func:`q8_quantize_ref`.
    2. ``y = fp32(v + residual)``, one IEEE add with subnormals kept; at or past ``count`` ``y = 0`` whatever
       ``residual`` holds there.  Where ``residual`` is zero ``y`` is ``v`` itself: the add would turn an input of
       ``-0`` into ``+0`` and its code ``0x80`` into ``0x00``, the one difference from the plain rule that a zero
       residual could make.
    3. ``codes, exps = q8_quantize_ref(y, "fp32")`` and ``dq = q8_dequantize_ref(codes, exps)``: the block
       exponent, its clamp and the NaN/Inf coding are the unchanged rule's, applied to ``y``.
    4. ``new_residual = fp32(y - dq)`` where that difference is finite (the subtraction is then exact), and
       ``+0`` elsewhere: where ``y`` is NaN or Inf, where ``dq`` came out Inf (a magnitude of at least
       ``248 * 2^120`` packed under ``e = 120``) and at or past ``count``.  One overflowing step must not poison
       every later one.

    With ``residual`` all zero the codes and exponents are :func:`q8_quantize_ref`'s.  Where the block
    exponent is not clamped, ``|new_residual| <= amax(y) / 14`` of its block."""
    if dtype not in ELEM:
        raise ValueError(f"dtype must be bf16|fp32, got {dtype!r}")
    v = bf16_to_f32(x) if dtype == "bf16" else np.ascontiguousarray(x, dtype=np.float32)
    count = int(v.shape[0]) if count is None else int(count)
    if not 0 <= count <= v.shape[0]:
        raise ValueError("count past the end of x")
    n = q8_blocks(count) * Q8_BLOCK
    res = np.ascontiguousarray(residual)
    if res.dtype != np.float32 or res.shape != (n,):
        raise ValueError(f"residual: float32, one value per element of the {n // Q8_BLOCK} blocks covered")
    y = np.zeros(n, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):  # Inf and NaN are results here, not faults
        y[:count] = np.where(res[:count] == 0, v[:count], (v[:count] + res[:count]).astype(np.float32))
        codes, exps = q8_quantize_ref(y, "fp32")
        diff = (y - q8_dequantize_ref(codes, exps)).astype(np.float32)
    return codes, exps, np.where(np.isfinite(diff), diff, np.float32(0)).astype(np.float32)


def _q8_ef_contributions(inputs: Sequence[np.ndarray], residuals: Sequence[np.ndarray], dtype: str):
    """Every member's dequantised packing with feedback, cut to the count, and its new residual."""
    if not inputs:
        raise ValueError("no inputs")
    if len(residuals) != len(inputs):
        raise ValueError("one residual per member")
    count = int(np.asarray(inputs[0]).shape[0])
    wide, new = [], []
    for a, r in zip(inputs, residuals):
        codes, exps, nr = q8_quantize_ef_ref(a, dtype, r)
        wide.append(q8_dequantize_ref(codes, exps)[:count])
        new.append(nr)
    return wide, new


def allreduce_q8_ef_ref(inputs: Sequence[np.ndarray], residuals: Sequence[np.ndarray], dtype: str, out_dtype: Optional[str] = None,
                        scale: float = 1.0, wire: str = "fp8") -> Tuple[np.ndarray, List[np.ndarray]]:
    """:func:`allreduce_q8_ref` (``wire="fp8"``) or :func:`allreduce_q8x2_ref` (``wire="fp8x2"``) with error
    feedback: ``(result, new_residuals)``.  Member m's contribution is the dequantised packing of
    :func:`q8_quantize_ef_ref` on ``inputs[m]`` and ``residuals[m]``; the sum, the scale, the rounding and,
    for ``fp8x2``, the second packing are exactly those functions'.

    Feedback covers the sender's packing only.  The second rounding of ``fp8x2``, phase 1 packing the sum
    again, is not fed back: it is the slice owner's, and its error stays in the result."""
    out = out_dtype_of(dtype, out_dtype)
    if wire not in ("fp8", "fp8x2"):
        raise ValueError(f'wire must be "fp8" or "fp8x2", got {wire!r}')
    wide, new = _q8_ef_contributions(inputs, residuals, dtype)
    acc = allreduce_ref(wide, "fp32", "fp32", scale)
    if wire == "fp8x2":
        acc = q8_dequantize_ref(*q8_quantize_ref(acc, "fp32"))[:acc.shape[0]]
    return (bf16_round(acc) if out == "bf16" else acc), new


def reduce_scatter_q8_ef_ref(inputs: Sequence[np.ndarray], residuals: Sequence[np.ndarray], dtype: str,
                             out_dtype: Optional[str] = None, scale: float = 1.0) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """:func:`reduce_scatter_q8_ref` with error feedback: ``(pieces, new_residuals)``.  The pieces concatenate
    to :func:`allreduce_q8_ef_ref`'s result on the fp8 wire; every member packs its whole input, so the
    residuals are that function's too.  Feedback covers the sender's packing only."""
    full, new = allreduce_q8_ef_ref(inputs, residuals, dtype, out_dtype, scale)
    count = int(full.shape[0])
    return [full[min(count, a * Q8_BLOCK):min(count, b * Q8_BLOCK)] for a, b in q8_slices(q8_blocks(count), len(inputs))], new


# -- the ZeRO-1 step ------------------------------------------------------------------------------
def adamw_ref(p: np.ndarray, m: np.ndarray, v: np.ndarray, g: np.ndarray, hyper: Sequence[float]):
    """One AdamW update (decoupled weight decay) of float32 master ``p``, ``m`` and ``v`` with the float32
    gradient ``g``: ``(p, m, v, w)``, new arrays, ``w`` the bf16 bit patterns of the new master.

    ``hyper`` is the kernels' host form, eight values taken as float32: ``lr, beta1, beta2, eps, weight_decay,
    grad_scale, bias_c1, bias_c2`` with ``bias_c = 1 - beta^t``.  Every operation is one float32 operation, in
    the order of ``adam8_update`` (``csrc/common/adamw_update.h``)::

        gr = g * grad_scale
        m  = beta1 * m + (1 - beta1) * gr
        v  = beta2 * v + ((1 - beta2) * gr) * gr
        p  = p - lr * ((m / bias_c1) / (sqrt(v / bias_c2) + eps) + weight_decay * p)

    The kernel may fuse a multiply into the add that follows it, so it matches this to a few units in the last
    place, not bit for bit; with ``beta1 = beta2 = 0`` the new ``m`` is ``gr`` and the new ``v`` is ``gr * gr``
    rounded once, fused or not.  A NaN or an Inf in ``g`` reaches its own element alone."""
    lr, b1, b2, eps, wd, gs, bc1, bc2 = (np.float32(x) for x in hyper)
    one = np.float32(1)
    p, m, v, g = (np.ascontiguousarray(a, dtype=np.float32) for a in (p, m, v, g))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):  # Inf and NaN are results here
        gr = g * gs
        m = b1 * m + (one - b1) * gr
        v = b2 * v + (one - b2) * gr * gr
        upd = (m / bc1) / (np.sqrt(v / bc2) + eps)
        p = p - lr * (upd + wd * p)
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v, bf16_round(p)


def zero1_slices(count: int, k: int, wire: Optional[str] = None) -> List[Tuple[int, int]]:
    """``[first, end)`` in elements of each of ``k`` ranks' slice of ``count`` parameters, in whole units of the
    wire, not clipped to the count: vectors of 8 bf16 cut by :func:`peer_slices` on the native wire, blocks of 32
    cut by :func:`q8_slices` on ``"fp8"``.  A rank's optimizer state has ``end - first`` elements."""
    if wire == "fp8":
        return [(a * Q8_BLOCK, b * Q8_BLOCK) for a, b in q8_slices(q8_blocks(count), k)]
    if wire not in (None, "native"):
        raise ValueError(f'wire must be None, "native" or "fp8", got {wire!r}')
    return [(8 * a, 8 * b) for a, b in peer_slices(-(-int(count) // 8), k)]


def clip_grad_scale(total: float, grad_scale: float, clip_norm: float) -> Tuple[float, float]:
    """``(norm, grad_scale')`` of global-norm clipping, in float64::

        norm        = sqrt(total) * grad_scale
        grad_scale' = grad_scale * min(1, clip_norm / (norm + float32(1e-6)))

    ``total`` is the sum of squares of the gradient before ``grad_scale``.  It is the formula of
    ``models/optim_ref.dev_hyper_ref`` and of ``hyper<true>`` (``csrc/ops/adamw.hip``).  The minimum is a comparison,
    not an ``fmin``: a NaN norm gives a NaN factor, and with it a NaN in every element, where an ``fmin`` would
    switch the clipping off quietly.  An infinite norm gives the factor 0; ``clip_norm = inf`` never clips a finite
    norm.  Every rank evaluates this on the same values in the same order and so holds the same bits."""
    with np.errstate(all="ignore"):  # Inf and NaN are results here, not faults
        gs = np.float64(grad_scale)
        norm = np.sqrt(np.float64(total)) * gs
        f = np.float64(clip_norm) / (norm + np.float64(np.float32(1e-6)))
        return float(norm), float(gs * (np.float64(1.0) if f > 1.0 else f))


def zero1_sqnorm_ref(pieces: Sequence[np.ndarray]) -> float:
    """The sum of squares, in float64, of the ranks' float32 gradient pieces (what :func:`reduce_scatter_ref` with an
    fp32 output returns).  Every element is widened first, so each square is exact; a piece's squares are added by
    ``math.fsum``, which rounds their exact sum once, so neither the order inside a piece nor zeros appended to it change
    a bit; the pieces' sums are then added one by one in rank order, as the ranks' published values are."""
    total = 0.0
    for p in pieces:
        total += math.fsum(np.square(np.asarray(p, dtype=np.float32).astype(np.float64)).tolist())
    return total


def _zero1_pieces(inputs: Sequence[np.ndarray], dtype: str, scale: float, wire: Optional[str],
                  residuals: Optional[List[np.ndarray]]) -> List[np.ndarray]:
    """Every rank's fp32 piece of the reduce-scatter of ``inputs`` on ``wire``, clipped to the count; with ``residuals``
    (``wire="fp8"``) the packing feeds back, and the list is given the residuals after it."""
    if residuals is not None:
        if wire != "fp8":
            raise ValueError('residuals belong to wire="fp8"')
        pieces, after = reduce_scatter_q8_ef_ref(inputs, residuals, dtype, "fp32", scale)
        residuals[:] = after
        return pieces
    if wire == "fp8":
        return reduce_scatter_q8_ref(inputs, dtype, "fp32", scale)
    return reduce_scatter_ref(inputs, dtype, "fp32", scale)


def zero1_accumulate_ref(acc: Optional[Sequence[np.ndarray]], inputs: Sequence[np.ndarray], dtype: str, scale: float,
                         wire: Optional[str] = None, residuals: Optional[List[np.ndarray]] = None) -> List[np.ndarray]:
    """The ranks' float32 gradient accumulators after one more micro-batch: new arrays, rank r's of the size of its slice
    of :func:`zero1_slices`, zero in the padding.

    ``inputs`` are the ranks' bf16 gradients of the micro-batch.  Rank r's piece is the step's: its piece of
    :func:`reduce_scatter_ref` with an fp32 output (``wire="fp8"``: of :func:`reduce_scatter_q8_ref`; with
    ``residuals``: of :func:`reduce_scatter_q8_ef_ref`, and the list is given the residuals after the call), the sum in
    member order multiplied once by ``scale``.  ``acc`` is ``None`` for the first micro-batch, which stores the piece;
    otherwise the accumulators so far, and the new one is ``float32(acc + piece)``: one fp32 add per element, the
    product rounded before it (no fused multiply-add)."""
    if dtype != "bf16":
        raise ValueError("the ZeRO-1 step takes bf16 gradients: fp32 windows are refused")
    k = len(inputs)
    count = int(np.asarray(inputs[0]).shape[0])
    plan = zero1_slices(count, k, wire)
    if acc is not None and (len(acc) != k or any(np.asarray(x).dtype != np.float32 or np.asarray(x).shape != (b - a,)
                                                 for x, (a, b) in zip(acc, plan))):
        raise ValueError("one float32 accumulator per rank, of the size of its slice")
    out = []
    for r, ((a, b), piece) in enumerate(zip(plan, _zero1_pieces(inputs, dtype, scale, wire, residuals))):
        g = np.zeros(b - a, np.float32)
        g[:piece.shape[0]] = piece
        if acc is not None:
            with np.errstate(over="ignore", invalid="ignore"):  # Inf and NaN are results here, not faults
                g = (np.asarray(acc[r]) + g).astype(np.float32)
        out.append(g)
    return out


def zero1_step_ref(inputs: Sequence[np.ndarray], states: Sequence[Tuple[np.ndarray, np.ndarray, np.ndarray]], dtype: str, scale: float,
                   hyper: Sequence[float], wire: Optional[str] = None, residuals: Optional[List[np.ndarray]] = None,
                   clip_norm: Optional[float] = None, accumulated: Optional[Sequence[np.ndarray]] = None):
    """One ZeRO-1 step: ``(new_states, weights)``; with ``clip_norm``, ``(new_states, weights, norm)``.

    ``inputs`` are the ranks' gradients (``dtype`` must be ``"bf16"``: bit patterns, ``count`` each), ``states[r]``
    rank r's float32 ``(master, m, v)`` of its slice of :func:`zero1_slices`, padding included.  Rank r's gradient is
    its piece of :func:`reduce_scatter_ref` with an fp32 output (``wire="fp8"``: of :func:`reduce_scatter_q8_ref`;
    with ``residuals``, every rank's error-feedback residual, of :func:`reduce_scatter_q8_ef_ref`, and the list is
    given the residuals after the step), zero in the padding; :func:`adamw_ref` with ``hyper`` updates the
    slice.  ``weights`` are the ``count`` new bf16 weights every rank's out then holds.

    ``clip_norm`` clips by the global norm: :func:`clip_grad_scale` of :func:`zero1_sqnorm_ref` of the pieces, which
    are scaled already, with ``hyper``'s ``grad_scale`` gives ``norm`` and the ``grad_scale`` of the update, rounded to
    float32 as every hyper-parameter is.  Clipping comes after the sum, so the residuals are those of an unclipped step.

    ``accumulated`` are the ranks' float32 accumulators of the micro-batches before this one, as
    :func:`zero1_accumulate_ref` returned them; ``inputs`` is then the last micro-batch, and every rank's gradient piece
    becomes ``float32(accumulator + piece)``, one add, before the norm and the update.  The residuals are those of an
    unaccumulated step."""
    if dtype != "bf16":
        raise ValueError("the ZeRO-1 step takes bf16 gradients: fp32 windows are refused")
    k = len(inputs)
    if len(states) != k:
        raise ValueError("one state per rank")
    count = int(np.asarray(inputs[0]).shape[0])
    plan = zero1_slices(count, k, wire)
    if accumulated is not None:
        pieces = zero1_accumulate_ref(accumulated, inputs, dtype, scale, wire, residuals)
    else:
        pieces = _zero1_pieces(inputs, dtype, scale, wire, residuals)
    norm = None
    if clip_norm is not None:
        norm, gs = clip_grad_scale(zero1_sqnorm_ref(pieces), float(hyper[5]), clip_norm)
        hyper = list(hyper[:5]) + [float(np.float32(gs))] + list(hyper[6:])
    new, w = [], []
    for (a, b), piece, (p, m, v) in zip(plan, pieces, states):
        g = np.zeros(b - a, np.float32)
        g[:piece.shape[0]] = piece
        p, m, v, bits16 = adamw_ref(p, m, v, g, hyper)
        new.append((p, m, v))
        w.append(bits16)
    if clip_norm is not None:
        return new, np.concatenate(w)[:count], norm
    return new, np.concatenate(w)[:count]


# -- how a launch walks its range -----------------------------------------------------------------
LAUNCH_BLOCK = 256               # gtk::kStreamBlock: lanes of a block, one unit (a 16-byte vector) per lane and position
LAUNCH_BUCKETS = (2, 4, 8, 16)   # the member buckets KB: a launch of k members takes the first bucket with k <= KB

#: Positions per lane, U, of each bucketed kernel (``name_kernel<.., KB, U>`` on the launch lines of
#: ``csrc/probe/peer_driver.h`` and ``csrc/probe/peer_zero1.h``), in the order of :data:`LAUNCH_BUCKETS`.
LAUNCH_U = {
    "peer_reduce": (4, 4, 2, 1),
    "peer_reduce_push": (4, 4, 2, 1),
    "peer_q8_sum": (4, 4, 2, 1),
    "peer_q8_sum_push": (4, 4, 2, 1),
    "peer_q8_repack": (4, 4, 2, 1),
    "peer_reduce_adamw_push": (4, 2, 2, 1),
    "peer_q8_sum_adamw_push": (2, 2, 1, 1),
    "peer_reduce_sqnorm_stash": (4, 4, 2, 1),
    "peer_q8_sum_sqnorm_stash": (4, 4, 2, 1),
    "peer_reduce_sqnorm_accum": (4, 4, 2, 1),
    "peer_q8_sum_sqnorm_accum": (4, 4, 2, 1),
    "peer_adamw_push": (2, 2, 2, 2),
}


def launch_u(kernel: str, k: int) -> int:
    """U of ``kernel`` (a key of :data:`LAUNCH_U`) in a launch of ``k`` members."""
    if not 1 <= k <= LAUNCH_BUCKETS[-1]:
        raise ValueError(f"1..{LAUNCH_BUCKETS[-1]} members")
    return LAUNCH_U[kernel][next(i for i, kb in enumerate(LAUNCH_BUCKETS) if k <= kb)]


def launch_walk(n_units: int, grid: int, U: int) -> Tuple[List[int], List[List[int]]]:
    """``peer_reduce_range`` (``csrc/probe/peer_allreduce.h``; ``peer_q8_sum_range``, the repack and
    ``peer_adamw_push_kernel`` walk alike) over ``n_units`` units on ``grid`` blocks, transcribed: ``(tiles, trips)``.

    ``tiles[b]`` is the number of whole tiles of ``256 * U`` units that block b takes: ``per = ceil(n_tiles / grid)``
    consecutive ones from tile ``b * per``, as far as there are tiles.  ``trips[t][b]`` is the number of live lanes of
    block b in trip t of the remainder loop, which walks what is left, under one tile, one unit per lane and ``grid *
    256`` units per trip; a trip with no live lane is not listed, so an empty remainder gives ``[]``."""
    if n_units < 0 or grid < 1 or U < 1:
        raise ValueError("n_units >= 0, grid >= 1, U >= 1")
    tile = LAUNCH_BLOCK * U
    n_tiles = n_units // tile
    per = -(-n_tiles // grid)
    tiles = []
    for b in range(grid):
        t0 = b * per
        t1 = min(n_tiles, t0 + per)
        tiles.append(max(0, t1 - t0))
    trips = []
    first = n_tiles * tile
    while first < n_units:
        trips.append([max(0, min(LAUNCH_BLOCK, n_units - (first + b * LAUNCH_BLOCK))) for b in range(grid)])
        first += grid * LAUNCH_BLOCK
    return tiles, trips
