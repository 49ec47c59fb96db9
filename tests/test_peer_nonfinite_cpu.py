"""CPU tests of the K7 references (ops/peer_ref.py) on the values the other peer tests leave out: NaN of
every kind, the infinities, fp32 and bf16 subnormals, signed zeros and sums that overflow on the final
rounding.  ``bf16_round`` and the fp8 wire's quantize are checked against their stated rules and against
torch's casts, the sums against IEEE arithmetic worked out by hand, and the peer communicator's host
backend runs the inputs that tests/test_gpu_peer_nonfinite.py gives the kernels.

This module also makes those inputs (the specials, the table of their ordered pairs, where the table
lies in a call, the fp8 wire's crafted blocks), so that both files test the same thing."""
import functools
import math
import warnings

import numpy as np
import pytest

import test_peer_q8_cpu as Q
from gpu_topology_on_k8s_amd.ops.peer_ref import (ELEM, Q8_BLOCK, allreduce_q8_ref, allreduce_ref, bf16_round, bf16_to_f32, bits, is_nan_bits,
                                                  mismatches, peer_slices, q8_blocks, q8_dequantize_ref, q8_quantize_ref,
                                                  reduce_scatter_q8_ref, reduce_scatter_ref)
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

PAIRS = (("bf16", "bf16"), ("fp32", "fp32"), ("bf16", "fp32"))

# -- the specials -----------------------------------------------------------------------------
#: fp32 bit patterns: 0, the smallest and the largest subnormal, the smallest normal, 1, 2^24, the largest
#: finite value and Inf, each of both signs, and three NaNs (quiet, signalling, all ones)
_F32_MAGS = (0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x4B800000, 0x7F7FFFFF, 0x7F800000)
F32_NANS = (0x7FC00000, 0x7F800001, 0xFFFFFFFF)
F32_SPECIALS = np.array([s | m for m in _F32_MAGS for s in (0, 0x80000000)] + list(F32_NANS), np.uint32)
#: bf16 bit patterns: the same classes, and values whose fp32 sums land on bf16's rounding edges:
#:   0x7F7F + 0x7B00 = max + 2^119 = 0x7F7F8000, a tie under an odd upper half: Inf
#:   0x7F7F + 0x7A80 = max + 2^118 = 0x7F7F4000: stays the maximum
#:   0x3F80 + 0x3B80 = 1 + 2^-8 = 0x3F808000, a tie under an even upper half: 0x3F80
#:   0x3F81 + 0x3B80 = 0x3F818000, a tie under an odd upper half: 0x3F82
#:   (0x0001 + 0x0002) / 2 = 0x00018000, a subnormal tie under an odd upper half: 0x0002
#:   (0x0002 + 0x0003) / 2 = 0x00028000, a subnormal tie under an even upper half: 0x0002
#: (the halved ones are met where the scale is 1/2: sums of bf16 subnormals have a zero low half)
_BF16_MAGS = (0x0000, 0x0001, 0x007F, 0x0080, 0x3F80, 0x4B80, 0x7F7F, 0x7F80)
BF16_NANS = (0x7FC0, 0x7F81, 0xFFFF)
BF16_EDGES = (0x7B00, 0x7A80, 0x3B80, 0x3F81, 0x0002, 0x0003)
BF16_SPECIALS = np.array([s | m for m in _BF16_MAGS for s in (0, 0x8000)] + list(BF16_NANS) + list(BF16_EDGES), np.uint16)


def specials(dtype):
    """The specials as a wire input: uint16 patterns for bf16, float32 for fp32."""
    return BF16_SPECIALS.copy() if dtype == "bf16" else F32_SPECIALS.view(np.float32).copy()


@functools.lru_cache(maxsize=None)
def pair_table(dtype):
    """Every ordered pair (a, b) of the specials: two input arrays of len(specials)^2 elements."""
    s = specials(dtype)
    a, b = np.repeat(s, s.size), np.tile(s, s.size)
    assert a.size == s.size ** 2 < 1000
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def reduce_unroll(k):
    """Vectors a lane of peer_reduce_kernel holds per member in k's bucket (peer_driver.h): a tile is 256 of them."""
    return 4 if k <= 4 else 2 if k <= 8 else 1


def runs(k, algo, n_vec):
    """``(first, end of the whole tiles, end)`` in vectors of every range one reduce launch covers: the
    call for one-shot, a member's slice for two-shot."""
    tile = 256 * reduce_unroll(k)
    ranges = [(0, n_vec)] if algo == "oneshot" else peer_slices(n_vec, k)
    return [(a, a + (b - a) // tile * tile, b) for a, b in ranges]


TAIL_VECS = 208  # vectors of a tail that holds the pair table twice: 1664 bf16 or 832 fp32 elements


def native_counts(k, algo, dtype):
    """``8 * 1024 * k + 11``, the smallest count at which every two-shot slice has a tile and the call ends
    in a tail and padding; its tails are one to three vectors and hold the first pairs only.  So a second
    count: every launch's range is whole tiles and a tail of 208 vectors, five elements short of a vector."""
    per = 16 // ELEM[dtype]
    tile = 256 * reduce_unroll(k)
    n_vec = k * tile + TAIL_VECS if algo == "oneshot" else k * (tile + TAIL_VECS)
    return [8 * 1024 * k + 11, n_vec * per - 5]


def _normal(rng, count, dtype):
    x = rng.standard_normal(count, dtype=np.float32)
    return bf16_round(x) if dtype == "bf16" else x


@functools.lru_cache(maxsize=None)
def native_case(k, algo, dtype, count):
    """k members' inputs of ``count`` elements, N(0, 1) but for the pair table, which lies four times in
    them: as (member 0, member 1), the accumulator's first value and the first add, and as (member k - 2,
    member k - 1) after the others' finite values; each inside the whole tiles and inside the tail of a
    launch's range (two-shot: member 0's slice for the first pair of members, the last slice for the
    second).  What does not fit before the count is cut off.  Returns ``(inputs, places)``, a place being
    ``(first element, elements, member of a, member of b, "tiles" | "tail")``."""
    per = 16 // ELEM[dtype]
    rng = np.random.default_rng([k, count, algo == "oneshot", dtype == "bf16"])
    xs = [_normal(rng, count, dtype) for _ in range(k)]
    ta, tb = pair_table(dtype)
    rs = runs(k, algo, -(-count // per))
    places = []

    def put(first, end, ma, mb, where):
        n = max(0, min(ta.size, min(end, count) - first))
        xs[ma][first:first + n], xs[mb][first:first + n] = ta[:n], tb[:n]
        places.append((first, n, ma, mb, where))
        return first + n

    for where, lo, hi in (("tiles", 0, 1), ("tail", 1, 2)):
        a_run, b_run = rs[0], rs[-1]
        nxt = put(a_run[lo] * per, a_run[hi] * per, 0, 1, where)
        start = nxt if b_run is a_run else b_run[lo] * per
        put(-(-start // per) * per, b_run[hi] * per, k - 2, k - 1, where)
    for x in xs:
        x.setflags(write=False)
    return tuple(xs), tuple(places)


@functools.lru_cache(maxsize=None)
def native_reference(k, algo, dtype, count, out, scale):
    ref = allreduce_ref(native_case(k, algo, dtype, count)[0], dtype, out, scale)
    ref.setflags(write=False)
    return ref


# -- the fp8 wire's crafted blocks ------------------------------------------------------------
def _poke(x, dtype, where, pattern32):
    """Bit pattern ``pattern32`` (bf16: its upper half) at element ``where`` of the input array ``x``."""
    if dtype == "bf16":
        x[where] = np.uint16(pattern32 >> 16)
    else:
        x.view(np.uint32)[where] = np.uint32(pattern32)


_NAN32 = (0x7FC00000, 0x7F810000, 0xFFFF0000, 0x7FFF0000, 0xFFC00000)  # every one a NaN in its upper half too
_PINF, _NINF = 0x7F800000, 0xFF800000


@functools.lru_cache(maxsize=None)
def special_blocks(dtype):
    """Whole blocks of 32, as a wire input, and the elements that are NaN or Inf.  In order: one NaN among
    finite values at element 0, 7, 8, 15, 16 and 31 (the first and last element of a lane and of a lane
    group, for 8 and 4 elements per lane); a NaN whose pattern is larger than every finite value's, among
    tiny values; +Inf, then -Inf, among finite values; NaN and both infinities together; an Inf among
    values near 1e38, which keep non-zero codes under e = 120; an all-NaN block; a block of subnormals
    only; a block at the largest finite value, both signs; and the block's amax right before, then two
    elements before, a signalling NaN in its own lane: a max instruction answers a signalling NaN with a
    NaN, and the next one then forgets what came before."""
    base = ((np.arange(Q8_BLOCK) - 15.5) * 0.173).astype(np.float32)
    blocks = []

    def block(vals, pokes):
        b = Q.as_input(np.asarray(vals, np.float32), dtype).copy()
        for where, pat in pokes:
            _poke(b, dtype, where, pat)
        blocks.append(b)

    for n, where in enumerate((0, 7, 8, 15, 16, 31)):
        block(base * np.float32(2.0 ** n), [(where, _NAN32[n % len(_NAN32)])])
    block(base * np.float32(2.0 ** -20), [(5, 0x7FFF0000)])
    block(base, [(3, _PINF)])
    block(base * np.float32(37.0), [(20, _NINF)])
    block(base, [(2, _NAN32[1]), (9, _NINF), (30, _PINF), (31, _NAN32[2])])
    block(base * np.float32(1.0e38), [(12, _PINF)])
    block(base, [(i, _NAN32[i % len(_NAN32)]) for i in range(Q8_BLOCK)])
    if dtype == "bf16":  # 0x0001 .. 0x007F, both signs
        block(base, [(i, ((1 + 4 * i) | (0x8000 * (i & 1))) << 16) for i in range(Q8_BLOCK)])
    else:                # 0x00000001 .. 0x007FFFFF, both signs
        block(base, [(i, (0x007FFFFF >> (22 - min(i, 22))) | (0x80000000 * (i & 1))) for i in range(Q8_BLOCK)])
    block(base, [(i, 0x7F7FFFFF | (0x80000000 * (i % 3 == 0))) for i in range(Q8_BLOCK)])
    if dtype == "bf16":  # the largest finite bf16, not the rounding of fp32's
        blocks[-1] = (blocks[-1] & np.uint16(0x8000)) | np.uint16(0x7F7F)
    for big, nan in ((6, 7), (4, 5)):
        vals = base * np.float32(0.01)
        vals[big] = 100.0
        block(vals, [(nan, 0x7F810000)])
    x = np.concatenate(blocks)
    x.setflags(write=False)
    return x


def wide(x, dtype):
    """float32 values of a wire input."""
    return bf16_to_f32(x) if dtype == "bf16" else np.ascontiguousarray(x, np.float32)


def masked_tail_case(dtype):
    """(input of 64 elements, count 40): finite data, and NaN patterns in the window after the count."""
    x = Q.as_input(((np.arange(64) - 20.25) * 0.31).astype(np.float32), dtype).copy()
    for i in range(40, 64):
        _poke(x, dtype, i, _NAN32[i % len(_NAN32)])
    return x, 40


Q8_HOLDERS = ("first", "last", "both")


def q8_counts(k):
    return [33, 512 * k + 37]


@functools.lru_cache(maxsize=None)
def q8_case(k, dtype, count, holders):
    """k members' inputs on the fp8 wire: values over 2^-73 .. 2^13, and the special blocks from element
    0 on (count 33: the block of NaN and infinities together, and a NaN as the only element of block 1),
    held by member 0, by the last member or by both, the last member holding the blocks in reverse order.
    A holder of the larger count also ends in an Inf and a NaN inside the ragged last block."""
    xs = [Q.as_input(Q.wide_random(count, dtype, seed=200 + m) * np.float32(2.0 ** -30), dtype).copy() for m in range(k)]
    sp = special_blocks(dtype).reshape(-1, Q8_BLOCK)
    for m in {"first": [0], "last": [k - 1], "both": [0, k - 1]}[holders]:
        order = sp if m == 0 else sp[::-1]
        if count == 33:
            xs[m][:32] = sp[9]
            _poke(xs[m], dtype, 32, _NAN32[m % 2])
        else:
            xs[m][:order.size] = order.reshape(-1)
            _poke(xs[m], dtype, count - 2, _NINF if m else _PINF)
            _poke(xs[m], dtype, count - 1, _NAN32[3])
    for x in xs:
        x.setflags(write=False)
    return tuple(xs)


def q8_scale(k, dtype, out):
    return 1.0 / k if dtype != out else 1.0


@functools.lru_cache(maxsize=None)
def q8_reference(k, dtype, count, holders, out):
    ref = allreduce_q8_ref(q8_case(k, dtype, count, holders), dtype, out, q8_scale(k, dtype, out))
    ref.setflags(write=False)
    return ref


# -- 1. bf16_round ----------------------------------------------------------------------------
def _f32(*patterns):
    return np.array(patterns, np.uint32).view(np.float32)


def test_bf16_round_spot_values():
    got = bf16_round(_f32(0x7F800001, 0x7FFFFFFF, 0xFFFFFFFF, 0xFF800001, 0x7FC00000, 0x7F808000, 0x7F80FFFF))
    assert got.tolist() == [0x7FC0, 0x7FFF, 0xFFFF, 0xFFC0, 0x7FC0, 0x7FC0, 0x7FC0]  # the upper half with 0x0040 set
    got = bf16_round(_f32(0x7F800000, 0xFF800000, 0x7F7F8000, 0x7F7F7FFF, 0xFF7FFFFF, 0x7F7F0000))
    assert got.tolist() == [0x7F80, 0xFF80, 0x7F80, 0x7F7F, 0xFF80, 0x7F7F]
    got = bf16_round(_f32(0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00008001, 0x00018000, 0x00028000, 0x807F8000, 0x007FFFFF))
    assert got.tolist() == [0x0000, 0x8000, 0x0000, 0x0000, 0x0001, 0x0002, 0x0002, 0x8080, 0x0080]


def test_bf16_round_keeps_every_finite_bit_and_matches_torch():
    """All 65536 upper halves under six lower halves.  Non-NaN inputs: the earlier one-line rule and torch's
    cast, bit for bit.  NaN inputs: a NaN of the same sign, and torch gives a NaN too."""
    torch = pytest.importorskip("torch")
    hi = np.arange(1 << 16, dtype=np.uint32) << np.uint32(16)
    b = np.concatenate([hi | np.uint32(lo) for lo in (0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF)] + [F32_SPECIALS])
    x = b.view(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = bf16_round(x)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    assert nan.sum() > 700 and np.array_equal(nan, np.isnan(x))
    old = ((b + (np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)).astype(np.uint16)
    np.testing.assert_array_equal(got[~nan], old[~nan])
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(got[~nan], want[~nan])
    assert np.array_equal(is_nan_bits(got), nan) and np.array_equal(is_nan_bits(want), nan)
    assert np.array_equal(got[nan] >> 15, (b[nan] >> 31).astype(np.uint16))
    np.testing.assert_array_equal(np.isnan(bf16_to_f32(got)), nan)


# -- 2. the comparison ------------------------------------------------------------------------
def test_mismatches_demands_a_nan_for_a_nan_and_the_bits_for_everything_else():
    ref = _f32(0x7FC00000, 0xFFFFFFFF, 0x7F800000, 0x80000000, 0x00000001, 0x3F800000)
    assert mismatches(ref.copy(), ref).size == 0
    assert mismatches(_f32(0xFFC12345, 0x7F800001, 0x7F800000, 0x80000000, 0x00000001, 0x3F800000), ref).size == 0  # any NaN will do
    got = _f32(0x7F800000, 0x00000000, 0x7FC00000, 0x00000000, 0x00000000, 0x3F800001)
    assert mismatches(got, ref).tolist() == [0, 1, 2, 3, 4, 5]  # Inf or 0 for a NaN, NaN for Inf, +0 for -0, a flushed subnormal, one ulp
    r16 = np.array([0x7FC0, 0xFF81, 0x7F80, 0x8000, 0x0001], np.uint16)
    assert mismatches(np.array([0xFFFF, 0x7FC0, 0x7F80, 0x8000, 0x0001], np.uint16), r16).size == 0
    assert mismatches(np.array([0x7F80, 0xFF80, 0x7F81, 0x0000, 0x0000], np.uint16), r16).tolist() == [0, 1, 2, 3, 4]
    assert is_nan_bits(r16).tolist() == [True, True, False, False, False]
    for bad in (lambda: mismatches(ref.view(np.uint32), ref), lambda: mismatches(ref[:3], ref), lambda: mismatches(r16, ref)):
        with pytest.raises(ValueError):
            bad()


# -- 3. the sums ------------------------------------------------------------------------------
def test_sums_of_the_pair_table_are_ieee():
    """The reference on every ordered pair of the specials, against the rules worked out by hand."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a, b = pair_table("fp32")
        s = allreduce_ref([a, b], "fp32")
        ab, bb, sb = bits(a).astype(np.int64), bits(b).astype(np.int64), bits(s).astype(np.int64)
        nan_in = is_nan_bits(a) | is_nan_bits(b)
        inf_a, inf_b = np.isinf(a), np.isinf(b)
        opposite = inf_a & inf_b & (np.signbit(a) != np.signbit(b))
        np.testing.assert_array_equal(is_nan_bits(s), nan_in | opposite)
        one_inf = (inf_a | inf_b) & ~nan_in & ~opposite
        np.testing.assert_array_equal(sb[one_inf], np.where(inf_a, ab, bb)[one_inf])
        # two values under 2^-125 of one sign: the bit patterns add as integers, nothing is flushed
        small = (ab & 0x7FFFFFFF < 0x00800001) & (bb & 0x7FFFFFFF < 0x00800001) & ((ab >> 31) == (bb >> 31))
        assert small.sum() == 32
        np.testing.assert_array_equal(sb[small], (ab + (bb & 0x7FFFFFFF))[small])
        zeros = (ab & 0x7FFFFFFF == 0) & (bb & 0x7FFFFFFF == 0)
        assert sb[zeros].tolist() == [0, 0, 0, 0x80000000]  # only -0 + -0 is -0
        big = (ab == 0x7F7FFFFF) & (bb == 0x7F7FFFFF)
        assert sb[big].tolist() == [0x7F800000]  # the sum overflows
        # adding -0 changes no bit of anything that is not a NaN
        keep = (bb == 0x80000000) & ~nan_in
        np.testing.assert_array_equal(sb[keep], ab[keep])

        def at(x, y, dtype, out=None, scale=1.0):
            r = allreduce_ref([np.array([x], np.uint16), np.array([y], np.uint16)], dtype, out, scale)
            return int(bits(r)[0])

        assert at(0x7F7F, 0x7B00, "bf16") == 0x7F80 and at(0xFF7F, 0xFB00, "bf16") == 0xFF80  # max + 2^119: a tie, up to Inf
        assert at(0x7F7F, 0x7A80, "bf16") == 0x7F7F and at(0x7F7F, 0x7B00, "bf16", "fp32") == 0x7F7F8000
        assert at(0x7F7F, 0x7F7F, "bf16") == 0x7F80 and at(0x7F7F, 0x7F7F, "bf16", "fp32") == 0x7F800000
        assert at(0x7F7F, 0x7F7F, "bf16", None, 0.5) == 0x7F80  # the sum overflowed before the scale
        assert at(0x3F80, 0x3B80, "bf16") == 0x3F80 and at(0x3F81, 0x3B80, "bf16") == 0x3F82
        assert at(0x0001, 0x0002, "bf16", None, 0.5) == 0x0002 and at(0x0002, 0x0003, "bf16", None, 0.5) == 0x0002
        assert at(0x0001, 0x0002, "bf16", "fp32", 0.5) == 0x00018000
        assert at(0x0001, 0x0001, "bf16") == 0x0002 and at(0x007F, 0x0001, "bf16") == 0x0080 and at(0x0080, 0x8001, "bf16") == 0x007F
        assert at(0x7F80, 0xFF80, "bf16") & 0x7FFF > 0x7F80 and at(0x7F81, 0x3F80, "bf16") & 0x7FFF > 0x7F80


def test_native_cases_hold_the_table_where_they_say():
    for k in (2, 3, 8, 16):
        for algo in pc.ALGOS:
            for dtype in ("bf16", "fp32"):
                per = 16 // ELEM[dtype]
                ta, tb = pair_table(dtype)
                issue, tail = native_counts(k, algo, dtype)
                assert issue == 8 * 1024 * k + 11 and issue % per and tail % per
                for count in (issue, tail):
                    xs, places = native_case(k, algo, dtype, count)
                    assert len(xs) == k and all(x.shape == (count,) for x in xs)
                    assert [(p[2], p[3], p[4]) for p in places] == [(0, 1, "tiles"), (k - 2, k - 1, "tiles"), (0, 1, "tail"), (k - 2, k - 1, "tail")]
                    rs = runs(k, algo, -(-count // per))
                    for (first, n, ma, mb, where), run in zip(places, (rs[0], rs[-1], rs[0], rs[-1])):
                        lo, hi = (run[0], run[1]) if where == "tiles" else (run[1], run[2])
                        assert n == 0 or (lo * per <= first and first + n <= min(hi * per, count))
                        assert n == ta.size or (where == "tail" and count == issue)
                        np.testing.assert_array_equal(bits(xs[ma][first:first + n]), bits(ta[:n]))
                        np.testing.assert_array_equal(bits(xs[mb][first:first + n]), bits(tb[:n]))
                        for m in set(range(k)) - {ma, mb}:
                            assert np.all(np.isfinite(wide(xs[m][first:first + n], dtype)))
                    if count == tail:
                        assert all(p[1] == ta.size for p in places)
                    else:
                        assert sum(p[1] for p in places if p[4] == "tail") > 0


# -- 4. the fp8 wire's format -----------------------------------------------------------------
def _block_exp(v):
    """The block exponent of float32 values by the stated rule, in Python floats."""
    fin = [abs(float(t)) for t in v if not math.isnan(t)]
    amax = max(fin) if fin else 0.0
    if amax == 0:
        return -100
    if math.isinf(amax):
        return 120
    e = math.frexp(amax)[1] - 9
    while amax * 2.0 ** -e > 448:
        e += 1
    while amax * 2.0 ** -(e - 1) <= 448:
        e -= 1
    return min(max(e, -100), 120)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_quantize_ref_rules_on_the_crafted_blocks(dtype):
    torch = pytest.importorskip("torch")
    x = special_blocks(dtype)
    v = wide(x, dtype)
    special = ~np.isfinite(v)
    assert special.sum() == 6 + 1 + 2 + 4 + 1 + 32 + 2 and x.size == 16 * Q8_BLOCK
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # rule 5
        codes, exps = q8_quantize_ref(x, dtype)
        back = q8_dequantize_ref(codes, exps)
    assert exps.tolist() == [_block_exp(b) for b in v.reshape(-1, Q8_BLOCK)]                       # rule 1
    assert exps[7] == exps[8] == exps[9] == exps[10] == 120 and exps[11] == -100 and exps[12] == -100 and exps[13] == 120 and exps[14] == exps[15] == -2
    assert np.all((codes[special] & 0x7F) == 0x7F) and not np.any((codes[~special] & 0x7F) == 0x7F)  # rule 2
    np.testing.assert_array_equal(np.isnan(back), special)                                         # rule 4
    # rule 3: the finite elements are coded as if the block's specials were not there but its exponent were;
    # torch's cast of the exactly scaled values is the independent rounding
    e = np.repeat(exps, Q8_BLOCK)
    y = np.ldexp(np.where(special, np.float32(0), v), -e).astype(np.float32)
    f8 = torch.from_numpy(y).to(torch.float8_e4m3fn)
    np.testing.assert_array_equal((codes & 0x7F)[~special], (f8.view(torch.uint8).numpy() & 0x7F)[~special])
    np.testing.assert_array_equal((codes >> 7)[~special], np.signbit(v)[~special])
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(back[~special], np.ldexp(f8.to(torch.float32).numpy(), e).astype(np.float32)[~special])
    # the largest finite value packs to the code of 256 under e = 120, and 256 * 2^120 is Inf of its sign
    top = slice(13 * Q8_BLOCK, 14 * Q8_BLOCK)
    assert np.all(codes[top] & 0x7F == 0x78) and np.array_equal(back[top], np.where(np.signbit(v[top]), -np.inf, np.inf))
    assert np.isinf(back).sum() == Q8_BLOCK
    nz = ~special & (np.abs(np.where(special, np.float32(0), v)) >= np.exp2(e - 9.0).astype(np.float32))
    assert np.all(back[nz] != 0) and nz.reshape(-1, Q8_BLOCK)[10].sum() >= 20  # next to the Inf of block 10 too
    # a NaN costs its neighbours nothing: the block without it packs to the same codes and exponent
    for b in range(7):
        blk = x[b * Q8_BLOCK:(b + 1) * Q8_BLOCK].copy()
        where = np.flatnonzero(special[b * Q8_BLOCK:(b + 1) * Q8_BLOCK])
        assert where.size == 1
        blk[where] = 0
        c0, e0 = q8_quantize_ref(blk, dtype)
        keep = np.arange(Q8_BLOCK) != where[0]
        assert e0[0] == exps[b] and np.array_equal(c0[keep], codes[b * Q8_BLOCK:(b + 1) * Q8_BLOCK][keep])


def test_quantize_ref_spot_values_with_a_nan_and_an_inf():
    x = np.zeros(Q8_BLOCK, np.float32)
    x[4], x[9] = 1.0, np.nan
    codes, exps = q8_quantize_ref(x, "fp32")
    assert exps.tolist() == [-8] and codes[4] == 0x78 and codes[9] & 0x7F == 0x7F
    back = q8_dequantize_ref(codes, exps)
    assert back[4] == 1.0 and np.isnan(back[9]) and not back[np.arange(Q8_BLOCK) % 5 != 4].any()
    x[4], x[9] = 2.0, -np.inf
    codes, exps = q8_quantize_ref(x, "fp32")
    assert exps.tolist() == [120] and codes[4] == 0 and codes[9] & 0x7F == 0x7F
    x[4] = 3.0e38
    codes, exps = q8_quantize_ref(x, "fp32")
    back = q8_dequantize_ref(codes, exps)
    assert exps.tolist() == [120] and abs(back[4] - 3.0e38) <= 2.0 ** 124 and np.isnan(back[9])
    assert np.isnan(q8_dequantize_ref(np.array([0x7F, 0xFF] * 16, np.uint8), np.array([3], np.int32))).all()
    codes, exps = q8_quantize_ref(np.full(Q8_BLOCK, np.nan, np.float32), "fp32")
    assert exps.tolist() == [-100] and np.all(codes & 0x7F == 0x7F)
    Q.test_spot_values()  # and every earlier spot value stands
    Q.test_ties_round_to_even_and_subnormal_codes_exist()
    Q.test_integer_patterns_and_count()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_quantize_ref_matches_torch_on_specials_too(dtype):
    """torch casts NaN and +Inf to 0x7F and -Inf to 0xFF: below the sign bit the codes agree everywhere."""
    torch = pytest.importorskip("torch")
    x = np.concatenate([special_blocks(dtype), Q.as_input(Q.crafted(dtype), dtype), Q.as_input(Q.wide_random(4096, dtype), dtype)])
    v = wide(x, dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        codes, exps = q8_quantize_ref(x, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.ldexp(v, -np.repeat(exps, Q8_BLOCK)).astype(np.float32)
    want = torch.from_numpy(y).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    np.testing.assert_array_equal(codes & 0x7F, want & 0x7F)
    fin = np.isfinite(v)
    np.testing.assert_array_equal(codes[fin & (v != 0)], want[fin & (v != 0)])


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_nan_patterns_after_the_count_are_masked(dtype):
    x, count = masked_tail_case(dtype)
    assert np.isnan(wide(x, dtype)[count:]).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        codes, exps = q8_quantize_ref(x, dtype, count=count)
    clean = x.copy()
    clean[count:] = 0
    c0, e0 = q8_quantize_ref(clean, dtype)
    assert not codes[count:].any() and np.array_equal(codes, c0) and np.array_equal(exps, e0)
    assert exps.tolist() == [_block_exp(wide(x, dtype)[:32]), _block_exp(wide(x, dtype)[32:count])]


def test_q8_references_carry_a_nan_to_every_rank_and_keep_the_rest():
    for dtype, out in PAIRS:
        for k in (2, 3):
            for holders in Q8_HOLDERS:
                count = q8_counts(k)[1]
                xs = q8_case(k, dtype, count, holders)
                ref = q8_reference(k, dtype, count, holders, out)
                sp = np.zeros(count, bool)
                for x in xs:
                    sp |= ~np.isfinite(wide(x, dtype))
                np.testing.assert_array_equal(is_nan_bits(ref), sp)  # NaN and Inf alike leave the wire as NaN, nothing else does
                pieces = reduce_scatter_q8_ref(xs, dtype, out, q8_scale(k, dtype, out))
                assert mismatches(np.concatenate(pieces), ref).size == 0
                # the finite elements are those of the same call with the specials zeroed, bit for bit, unless an Inf moved their block's exponent
                clean = [np.where(np.isfinite(wide(x, dtype)), x, np.zeros_like(x)) for x in xs]
                same_e = np.ones(count, bool)
                for x, c in zip(xs, clean):
                    same_e &= np.repeat(q8_quantize_ref(x, dtype)[1] == q8_quantize_ref(c, dtype)[1], Q8_BLOCK)[:count]
                ref0 = allreduce_q8_ref(clean, dtype, out, q8_scale(k, dtype, out))
                keep = ~sp & same_e
                assert keep.sum() > count // 2
                if holders == "first":  # the neighbours of the seven single NaNs among them
                    assert (keep & (np.arange(count) < 7 * Q8_BLOCK)).sum() == 7 * 31
                np.testing.assert_array_equal(bits(ref)[keep], bits(ref0)[keep])


# -- 5. the host backend ----------------------------------------------------------------------
def comm_plan(k):
    """(case, inputs) of every collective both backends run on the special inputs: the native wire on the
    pair table (all_reduce under both algorithms, reduce_scatter on the two-shot placement; scale 1, the
    wide pair 1/k), the fp8 wire on the crafted blocks held by the first and the last member."""
    plan = []
    for dtype, out in PAIRS:
        scale = 1.0 / k if dtype != out else 1.0
        for algo in pc.ALGOS:
            count = native_counts(k, algo, dtype)[0]
            xs = native_case(k, algo, dtype, count)[0]
            plan.append(({"op": "all_reduce", "count": count, "dtype": dtype, "out_dtype": out, "algo": algo, "scale": scale}, xs))
        plan.append(({"op": "reduce_scatter", "count": count, "dtype": dtype, "out_dtype": out, "algo": "oneshot", "scale": scale}, xs))
        for count in q8_counts(k):
            xs = q8_case(k, dtype, count, "both")
            for algo in pc.ALGOS:
                plan.append(({"op": "all_reduce", "count": count, "dtype": dtype, "out_dtype": out, "algo": algo, "scale": scale, "wire": "fp8"}, xs))
            plan.append(({"op": "reduce_scatter", "count": count, "dtype": dtype, "out_dtype": out, "algo": "oneshot", "scale": scale,
                          "wire": "fp8"}, xs))
    return plan


def plan_capacity(k):
    return pc._case_capacity(k, [c for c, _ in comm_plan(k)])


def plan_body(k):
    """A rank's body: issues the plan; returns (barriers of each collective, each result, each reference)."""
    plan = comm_plan(k)

    def body(comm):
        out = []
        for case, xs in plan:
            before = comm.barriers
            got, ref = pc.run_case(comm, case, list(xs))
            out.append((comm.barriers - before, got, ref))
        return out

    return body


@functools.lru_cache(maxsize=None)
def host_results(k):
    """The plan on the host backend: (fabric, per-rank results)."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fabric, results, errors = Q._run_threads(k, plan_body(k), cap=plan_capacity(k))
    assert not errors, errors
    return fabric, [results[r] for r in range(k)]


@pytest.mark.parametrize("k", [2, 3])
def test_host_backend_runs_the_special_inputs(k):
    fabric, results = host_results(k)
    plan = comm_plan(k)
    assert len(plan) == 3 * (3 + 2 * 3)
    for r in range(k):
        assert len(results[r]) == len(plan)
        for (case, xs), (barriers, got, ref) in zip(plan, results[r]):
            assert barriers == 2, case
            bad = mismatches(got, ref)
            assert bad.size == 0, (case, r, bad[:8].tolist())
            if case["op"] == "all_reduce":  # the reference run_case made is the shared one, and it does hold NaN
                shared = (q8_reference(k, case["dtype"], case["count"], "both", case["out_dtype"]) if case.get("wire") else
                          native_reference(k, case["algo"], case["dtype"], case["count"], case["out_dtype"], case["scale"]))
                assert mismatches(ref, shared).size == 0 and is_nan_bits(ref).sum() > 0
                np.testing.assert_array_equal(bits(got), bits(results[0][plan.index((case, xs))][1]))  # every rank the same bits
    assert fabric.conflicts() == []
