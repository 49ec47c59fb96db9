"""GPU tests of the K7 kernels on the values the other peer tests leave out (NaN of every kind, the
infinities, fp32 and bf16 subnormals, signed zeros, sums on bf16's rounding edges): the native wire
(csrc/probe/peer_allreduce.h) on the table of all ordered pairs of the specials, the fp8 wire's quantize
and sum (csrc/probe/peer_q8.h) on crafted blocks, and both through the peer communicator's device
backend against its host backend.

Members repeat device 0.  The inputs, their placement and the references come from
tests/test_peer_nonfinite_cpu.py, are made once and are read-only; a result is compared with
``ops.peer_ref.mismatches``: a NaN where the reference has one, the reference's bits everywhere else."""
import numpy as np
import pytest

import test_peer_nonfinite_cpu as N
from gpu_topology_on_k8s_amd.ops import probe
from gpu_topology_on_k8s_amd.ops.peer_ref import Q8_BLOCK, bits, is_nan_bits, mismatches, q8_quantize_ref
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

pytestmark = pytest.mark.gpu

KS = [2, 3, 8, 16]


def _assert_members(outs, ref, k, what):
    assert len(outs) == k
    for m, o in enumerate(outs):
        bad = mismatches(o, ref)
        assert bad.size == 0, (what, m, bad.size, [(int(i), hex(bits(o)[i]), hex(bits(ref)[i])) for i in bad[:8]])
        # every member ran the same instructions on the same inputs: NaN payloads included
        assert np.array_equal(bits(o), bits(outs[0])), (what, m)


# -- 1. the native wire -----------------------------------------------------------------------
@pytest.mark.parametrize("algo", pc.ALGOS)
@pytest.mark.parametrize("k", KS)
def test_native_wire_sums_the_pair_table_as_ieee(k, algo):
    for dtype, out in N.PAIRS:
        ta, tb = N.pair_table(dtype)
        for count in N.native_counts(k, algo, dtype):
            xs, places = N.native_case(k, algo, dtype, count)
            for scale in (1.0, 1.0 / k):
                ref = N.native_reference(k, algo, dtype, count, out, scale)
                outs = probe.peer_allreduce_arrays([0] * k, list(xs), dtype, algo, 1, out, scale)
                _assert_members(outs, ref, k, (dtype, out, algo, k, count, scale))
                if k == 2 and scale == 1.0:
                    # x + -0 = x: no subnormal is flushed, no signed zero loses its sign, nothing that is
                    # not a NaN changes a bit, through the add, the multiply by 1 and the rounding
                    keep = (bits(tb) == (0x8000 if dtype == "bf16" else 0x80000000)) & ~is_nan_bits(ta)
                    assert keep.sum() == np.sum(~is_nan_bits(N.specials(dtype)))
                    for first, n, ma, mb, where in places:
                        at = first + np.flatnonzero(keep[:n])
                        want = N.wide(xs[ma][at], dtype) if out != dtype else xs[ma][at]
                        assert np.array_equal(bits(outs[0][at]), bits(want)), (dtype, out, algo, where)


# -- 2. the fp8 wire's quantize kernel ---------------------------------------------------------
def _assert_codes(got, want, x, dtype, what):
    (got_c, got_e), (want_c, want_e) = got, want
    assert got_c.dtype == np.uint8 and got_c.shape == want_c.shape and got_e.shape == want_e.shape
    assert got_e.tolist() == want_e.tolist(), what
    v = N.wide(x, dtype)
    special = np.zeros(want_c.size, bool)
    special[:v.size] = ~np.isfinite(v)
    special &= (want_c & 0x7F) == 0x7F  # past a count nothing is special: masked elements are zero
    bad = np.flatnonzero(np.where(special, (got_c & 0x7F) != 0x7F, got_c != want_c))
    assert bad.size == 0, (what, bad.size, [(int(i), hex(got_c[i]), hex(want_c[i])) for i in bad[:12]])


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_quantize_kernel_follows_the_rule_on_non_finite_blocks(dtype):
    x = N.special_blocks(dtype)
    want = q8_quantize_ref(x, dtype)
    assert np.sum((want[0] & 0x7F) == 0x7F) == 48
    _assert_codes(probe.peer_q8_quantize(0, x, dtype), want, x, dtype, "special blocks")
    # a count that ends mid-block, NaN patterns in the window after it: code 0 there, the exponent untouched
    x, count = N.masked_tail_case(dtype)
    want = q8_quantize_ref(x, dtype, count=count)
    assert not want[0][count:].any()
    got = probe.peer_q8_quantize(0, x, dtype, count)
    _assert_codes(got, want, x, dtype, "masked tail")
    assert not got[0][count:].any()
    # and the special blocks cut inside the all-NaN block: its data is all NaN, the rest masked
    x = N.special_blocks(dtype)
    count = 11 * Q8_BLOCK + 9
    want = q8_quantize_ref(x, dtype, count=count)
    assert want[1][-1] == -100 and want[0].size == 12 * Q8_BLOCK
    _assert_codes(probe.peer_q8_quantize(0, x, dtype, count), want, x[:12 * Q8_BLOCK], dtype, "cut in the all-NaN block")


# -- 3. the fp8 wire's all-reduce --------------------------------------------------------------
@pytest.mark.parametrize("algo", pc.ALGOS)
@pytest.mark.parametrize("k", KS)
def test_fp8_wire_carries_non_finite_blocks_on_every_member(k, algo):
    for dtype, out in N.PAIRS:
        for count in N.q8_counts(k):
            for holders in N.Q8_HOLDERS:
                xs = N.q8_case(k, dtype, count, holders)
                ref = N.q8_reference(k, dtype, count, holders, out)
                assert is_nan_bits(ref).sum() > 0
                outs = probe.peer_allreduce_arrays([0] * k, list(xs), dtype, algo, 1, out, N.q8_scale(k, dtype, out), wire="fp8")
                _assert_members(outs, ref, k, (dtype, out, algo, k, count, holders))


# -- 4. thread ranks on the device backend against the host backend ---------------------------
def test_thread_ranks_equal_the_host_backend_on_both_wires():
    k = 3
    _, host = N.host_results(k)
    plan = N.comm_plan(k)
    res = pc.run_thread_ranks([0] * k, N.plan_body(k), N.plan_capacity(k), timeout_s=30.0)
    assert len(res) == k and {c.get("wire", "native") for c, _ in plan} == {"native", "fp8"}
    for r in range(k):
        assert len(res[r]) == len(plan)
        for (case, _), (barriers, got, ref), (_, want, _) in zip(plan, res[r], host[r]):
            assert barriers == 2, case
            bad = mismatches(got, want)
            assert bad.size == 0, (case, r, bad.size, bad[:8].tolist())
            assert mismatches(got, ref).size == 0, (case, r)
