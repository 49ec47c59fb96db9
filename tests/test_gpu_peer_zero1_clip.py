"""GPU tests of the clipped ZeRO-1 step (peer_reduce_sqnorm_stash_kernel, peer_q8_sum_sqnorm_stash_kernel and
peer_adamw_push_kernel of csrc/probe/peer_zero1.h) through the peer communicator's device backend on thread ranks:
launch 1 sums the rank's slice of every window into its own fp32 stash and leaves one sum-of-squares partial per block,
the ranks exchange their float64 totals at a third barrier, launch 2 applies AdamW from the stash with the clipped
grad_scale and pushes the new weights.

Members repeat device 0; one test runs on two devices where two are visible.  The norm and the stash are compared bit
for bit on gradients from {-1, 0, 1} (tests 1 and 2), where every fp32 summation order gives the same sum of squares;
the update is held to ops/peer_ref.zero1_step_ref(clip_norm=...) at the tolerances of tests/test_gpu_peer_zero1.py
(rtol 1e-5; atol 1e-6 for master and m, 1e-7 for v).  Inputs and references are made once
(tests/test_peer_zero1_cpu.py, tests/test_peer_zero1_clip_cpu.py) and are read-only."""
import functools
import math

import numpy as np
import pytest

import test_peer_zero1_clip_cpu as C
import test_peer_zero1_cpu as Z
from gpu_topology_on_k8s_amd.ops.peer_ref import (bf16_round, bf16_to_f32, bits, clip_grad_scale, is_nan_bits, reduce_scatter_q8_ref,
                                                   reduce_scatter_ref, zero1_slices, zero1_step_ref)
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

pytestmark = pytest.mark.gpu

KS = [2, 3, 8, 16]
WIRES = ["native", "fp8"]
HP = Z.HP
TOL = ((1e-5, 1e-6), (1e-5, 1e-6), (1e-5, 1e-7))  # (rtol, atol) of master, m, v
EXACT = dict(lr=0.0, beta1=0.0, beta2=0.0, eps=1e-8, weight_decay=0.0)  # m is the scaled gradient, v its square, master untouched


def _ranks(devices, body, cap):
    return pc.run_thread_ranks(devices, body, cap, timeout_s=30.0)


def _close(got, ref, what):
    for name, (rtol, atol), a, b in zip(("master", "m", "v"), TOL, got, ref):
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape, (what, name)
        np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=f"{what} {name}")


@functools.lru_cache(maxsize=None)
def signs(k, count):
    """Every rank's gradient from {-1, 0, 1} as bf16 bit patterns, and the exact integer sum over the ranks.  Both
    wires carry these values exactly, so on either the reduce-scatter's pieces are the integer sums (test 2 asserts it),
    and a slice's sum of squares stays below 2^24 (exact_total asserts it), where fp32 adds integers exactly."""
    ints = np.random.default_rng([41, k, count]).integers(-1, 2, size=(k, count))
    xs = tuple(bf16_round(row.astype(np.float32)) for row in ints)
    for a in xs:
        a.setflags(write=False)
    total = ints.sum(axis=0)
    total.setflags(write=False)
    return xs, total


def exact_total(k, count, wire):
    _, total = signs(k, count)
    plan = zero1_slices(count, k, wire)
    assert max(int((total[a:min(b, count)] ** 2).sum()) for a, b in plan) < 2 ** 24  # every summation order is exact
    return int((total ** 2).sum())


# -- 1. the norm is exact -----------------------------------------------------------------------------
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_the_norm_is_exact(k, wire):
    """scale = 1 and clip_norm = inf on gradients from {-1, 0, 1}: the returned norm is sqrt(the exact integer total),
    bit for bit, on every rank; a rank whose slice is empty has published 0.0 without a launch."""

    inputs = {count: signs(k, count)[0] for count in Z.counts(k)}  # made once, before the ranks ask for them

    def body(comm):
        got = []
        for count in Z.counts(k):
            comm.zero1_init(count, Z.weights0(count), wire)
            comm.write(inputs[count][comm.rank])
            launches = comm.launches
            got.append((comm.zero1_step(step=1, scale=1.0, clip_norm=float("inf"), **HP), comm.launches - launches))
        return got

    res = _ranks([0] * k, body, Z.capacity(max(Z.counts(k))))
    for ci, count in enumerate(Z.counts(k)):
        want = math.sqrt(exact_total(k, count, wire))
        plan = zero1_slices(count, k, wire)
        for r in range(k):
            norm, launches = res[r][ci]
            print(f"norm k={k} {wire} count={count} rank {r}: {norm!r} (exact {want!r})")
            assert isinstance(norm, float) and norm == want, (k, wire, count, r, norm, want)
            assert launches == (wire == "fp8") + 2 * (plan[r][1] > plan[r][0])


# -- 2. the stash and the factor are exact ------------------------------------------------------------
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_the_stash_and_the_factor_are_exact(k, wire):
    """The same inputs with beta1 = beta2 = lr = weight_decay = 0 and clip_norm at half the exact norm: the stash is
    the reduce-scatter's piece, zero in the padding; m is float32(g x gs') with gs' from clip_grad_scale(exact total),
    v its square rounded once, and master keeps its bits."""

    inputs = {count: signs(k, count)[0] for count in Z.counts(k)}
    clips = {count: 0.5 * math.sqrt(exact_total(k, count, wire)) for count in Z.counts(k)}

    def body(comm):
        got = []
        for count in Z.counts(k):
            comm.zero1_init(count, Z.weights0(count), wire)
            comm.write(inputs[count][comm.rank])
            norm = comm.zero1_step(step=1, scale=1.0, clip_norm=clips[count], **EXACT)
            a, b = zero1_slices(count, k, wire)[comm.rank]
            got.append((norm, comm._b.zero1_read_state(3, 0, b - a), comm.zero1_state()))
        return got

    res = _ranks([0] * k, body, Z.capacity(max(Z.counts(k))))
    for ci, count in enumerate(Z.counts(k)):
        xs = list(signs(k, count)[0])
        total = exact_total(k, count, wire)
        pieces = (reduce_scatter_q8_ref if wire == "fp8" else reduce_scatter_ref)(xs, "bf16", "fp32", 1.0)
        norm, gs = clip_grad_scale(total, 1.0, 0.5 * math.sqrt(total))
        assert 0.49 < gs < 0.51
        gs32 = np.float32(gs)
        start = Z.states0(k, count, wire)
        for r, (a, b) in enumerate(zero1_slices(count, k, wire)):
            what = f"k={k} {wire} count={count} rank {r}"
            g = np.zeros(b - a, np.float32)
            g[:pieces[r].size] = pieces[r]
            np.testing.assert_array_equal(g[:pieces[r].size], signs(k, count)[1][a:a + pieces[r].size].astype(np.float32))
            got_norm, stash, (master, m, v) = res[r][ci]
            assert got_norm == norm, what
            np.testing.assert_array_equal(bits(stash), bits(g), err_msg="stash " + what)
            gr = (g * gs32).astype(np.float32)
            np.testing.assert_array_equal(bits(m), bits(gr), err_msg="m " + what)
            np.testing.assert_array_equal(bits(v), bits((gr * gr).astype(np.float32)), err_msg="v " + what)
            np.testing.assert_array_equal(bits(master), bits(start[r][0]), err_msg="master " + what)


# -- 3. the update ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", C.CLIPS)
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_three_clipped_steps_follow_the_reference(k, wire, which):
    """Random gradients, clip_norm at half the reference norm of step 1 (every step clips) and at four times it (the
    factor is 1).  The norm is held to (slice_elems / 256 + 32) x 2^-25 relative, slice_elems the largest rank's slice:
    the adds on the longest chain of one block (elements per lane plus at most 16), eight tree adds and the square, 2^-24
    each, halved by the square root."""

    clips = {count: C.clip_of(k, count, wire, which) for count in Z.counts(k)}  # made once, before the ranks ask for them

    def body(comm):
        return [C.three_clipped_steps(comm, count, wire, clips[count]) for count in Z.counts(k)]

    res = _ranks([0] * k, body, Z.capacity(max(Z.counts(k))))
    for ci, count in enumerate(Z.counts(k)):
        ref = C.clip_trajectory(k, count, wire, which)
        plan = zero1_slices(count, k, wire)
        bound = (max(b - a for a, b in plan) / 256 + 32) * 2.0 ** -25
        for r in range(k):
            (first, n), got = res[r][ci]
            for t, (state, out, barriers, launches, norm) in enumerate(got):
                what = f"k={k} {wire} {which} count={count} rank {r} step {t + 1}"
                rel = abs(norm - ref[t][2]) / ref[t][2]
                if r == 0:
                    print(f"norm {what}: {norm!r} reference {ref[t][2]!r} relative {rel:.3e} bound {bound:.3e}")
                assert barriers == 3 and launches == (wire == "fp8") + 2 * (plan[r][1] > plan[r][0]), what
                assert rel <= bound, (what, norm, ref[t][2], rel, bound)
                assert norm == res[0][ci][1][t][4], what  # the same float on every rank
                _close(state, ref[t][0][r], what)
                assert np.isfinite(state[0]).all()
                np.testing.assert_array_equal(out[first:first + n], bf16_round(state[0])[:n], err_msg=what)  # the owner's own master, rounded once
                np.testing.assert_array_equal(out, res[0][ci][1][t][1], err_msg=what + " vs rank 0's out")
                np.testing.assert_allclose(bf16_to_f32(out), bf16_to_f32(ref[t][1]), rtol=2.0 ** -7, atol=1e-6, err_msg=what)


# -- 4. untouched memory ------------------------------------------------------------------------------
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", [3, 16])
def test_the_padding_is_zero_and_nothing_past_it_is_written(k, wire):
    """The poison test of tests/test_gpu_peer_zero1.py on the clipped path: every byte of out[0, end + 4096 elements)
    is 0xFF before the step; after it the count's weights are there, the rest of the last vector (fp8: block) is zero
    and everything after is 0xFF."""
    unit = 32 if wire == "fp8" else 8
    cases = [(count, unit * (-(-count // unit))) for count in Z.counts(k)]
    per = 8 * (-(-(max(end for _, end in cases) + 4096) // (8 * k)))  # elements every rank contributes to the poison
    cap = max(Z.capacity(max(Z.counts(k))), 2 * k * per)
    clips = {count: C.clip_of(k, count, wire, "half") for count, _ in cases}

    def body(comm):
        got = []
        for count, end in cases:
            comm.zero1_init(count, Z.weights0(count), wire)
            comm.write(np.full(per, 0xFFFF, np.uint16), comm.gather_slot(per, "bf16"))
            comm.all_gather(per, "bf16")
            poisoned = comm.read(0, k * per, "bf16")
            comm.write(Z.grads(k, count, 0)[comm.rank])
            comm.zero1_step(step=1, clip_norm=clips[count], **HP)
            got.append((poisoned, comm.read(0, k * per, "bf16")))
        return got

    res = _ranks([0] * k, body, cap)
    for ci, (count, end) in enumerate(cases):
        for r in range(k):
            poisoned, out = res[r][ci]
            assert (poisoned == 0xFFFF).all()
            assert not is_nan_bits(out[:count]).any() and (out[:count] != 0xFFFF).all()
            assert not out[count:end].any(), (k, wire, count, r)
            assert (out[end:] == 0xFFFF).all() and out[end:].size >= 4096, (k, wire, count, r)
            np.testing.assert_array_equal(out, res[0][ci][1])


# -- 5. non-finite gradients --------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["nan", "inf"])
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", [3, 8])
def test_a_nan_poisons_everything_and_an_inf_zeroes_the_factor(k, wire, bad):
    """A NaN in member 1's gradient makes the norm NaN and, through the factor, every value of every rank NaN, as in
    the reference.  An Inf alone makes the norm Inf and the factor 0: the pattern of NaN and finite values is the
    reference's (on the fp8 wire an Inf travels as the format's NaN, so there it is the first case again) and the finite
    values are within tolerance."""
    count = 8 * 1024 * k + 11
    xs = [x.copy() for x in Z.grads(k, count, 0)]
    xs[1][8 * 517 + 3] = 0x7FC0 if bad == "nan" else 0xFF80  # a quiet NaN, -Inf
    clip = C.clip_of(k, count, wire, "half")

    def body(comm):
        comm.zero1_init(count, Z.weights0(count), wire)
        comm.write(xs[comm.rank])
        norm = comm.zero1_step(step=1, clip_norm=clip, **HP)
        return norm, comm.zero1_state(), comm.read(0, count, "bf16")

    res = _ranks([0] * k, body, Z.capacity(count))
    ref_state, ref_w, ref_norm = zero1_step_ref(xs, Z.states0(k, count, wire), "bf16", C.mean(k), Z.hyper(1), wire, clip_norm=clip)
    all_nan = bad == "nan" or wire == "fp8"
    assert math.isnan(ref_norm) if all_nan else ref_norm == float("inf")
    for r in range(k):
        norm, state, out = res[r]
        what = f"k={k} {wire} {bad} rank {r}"
        assert math.isnan(norm) if all_nan else norm == float("inf"), what
        for name, (rtol, atol), a, b in zip(("master", "m", "v"), TOL, state, ref_state[r]):
            np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=f"{what} {name}: which values are NaN")
            fin = ~np.isnan(b)
            assert np.isfinite(b[fin]).all()
            np.testing.assert_allclose(a[fin], b[fin], rtol=rtol, atol=atol, err_msg=f"{what} {name}")
            if all_nan:
                assert np.isnan(a).all(), (what, name)
        np.testing.assert_array_equal(is_nan_bits(out), is_nan_bits(ref_w), err_msg=what)
        assert is_nan_bits(out).all() if all_nan else int(is_nan_bits(out).sum()) == 1, what
        np.testing.assert_array_equal(out, res[0][2], err_msg=what)


# -- 6. mixing clipped and unclipped steps ------------------------------------------------------------
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", [3, 16])
def test_an_unclipped_step_after_a_clipped_one_has_the_bits_of_a_run_that_never_clipped(k, wire):
    count = 8 * 1024 * k + 11
    clip = C.clip_of(k, count, wire, "half")

    def body(comm):
        comm.zero1_init(count, Z.weights0(count), wire)
        comm.write(Z.grads(k, count, 0)[comm.rank])
        comm.zero1_step(step=1, clip_norm=clip, **HP)
        saved = comm.zero1_state()
        comm.write(Z.grads(k, count, 1)[comm.rank])
        ret = comm.zero1_step(step=2, **HP)
        mixed = (comm.zero1_state(), comm.read(0, count, "bf16"))
        comm.zero1_init(count, Z.weights0(count), wire, state=saved)  # the same state in a run that never clipped: no stash
        assert comm._b.zero1_bytes == 12 * saved[0].size
        comm.write(Z.grads(k, count, 1)[comm.rank])
        comm.zero1_step(step=2, **HP)
        return ret, mixed, (comm.zero1_state(), comm.read(0, count, "bf16"))

    for r, (ret, mixed, plain) in enumerate(_ranks([0] * k, body, Z.capacity(count))):
        assert ret is None
        for a, b in zip(mixed[0], plain[0]):
            np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"k={k} {wire} rank {r}")
        np.testing.assert_array_equal(mixed[1], plain[1], err_msg=f"k={k} {wire} rank {r}")


# -- 7. counters and refusals -------------------------------------------------------------------------
@pytest.mark.parametrize("wire", WIRES)
def test_the_stash_is_counted_once_and_refusals_come_before_any_barrier(wire):
    k, count = 3, 8 * 1024 * 3 + 11
    plan = zero1_slices(count, k, wire)

    def body(comm):
        n = plan[comm.rank][1] - plan[comm.rank][0]
        comm.zero1_init(count, Z.weights0(count), wire)
        comm.write(Z.grads(k, count, 0)[comm.rank])
        seen = [comm._b.zero1_bytes]
        barriers = comm.barriers
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="clip_norm"):
                comm.zero1_step(step=1, clip_norm=bad, **HP)
        with pytest.raises(ValueError):
            comm._b.zero1_read_state(3, 0, 8)  # no stash before the first clipped step
        assert comm.barriers == barriers and comm._b.zero1_bytes == seen[0]
        comm.zero1_step(step=1, **HP)
        seen.append(comm._b.zero1_bytes)
        for t in (2, 3):
            comm.zero1_step(step=t, clip_norm=1.0, **HP)
            seen.append(comm._b.zero1_bytes)
        assert len(comm.zero1_state()) == 3
        with pytest.raises(ValueError):
            comm._b.r.adamw_push(0, n // 8 + 1, Z.hyper(1))  # more vectors than the stash holds
        with pytest.raises(ValueError):
            comm._b.r.reduce_sqnorm_stash(0, 1 << 40, 1.0)
        comm.zero1_init(count, Z.weights0(count), wire)
        seen.append(comm._b.zero1_bytes)
        return n, seen

    for n, seen in _ranks([0] * k, body, Z.capacity(count)):
        assert seen == [12 * n, 12 * n, 16 * n, 16 * n, 12 * n]  # 4 n more on the first clipped step only; a new init frees it


# -- 8. two distinct devices --------------------------------------------------------------------------
def _ndev() -> int:
    import torch

    return int(torch.cuda.device_count())  # counts without initialising HIP on this image


@pytest.mark.skipif(_ndev() < 2, reason="needs >= 2 visible GPUs (single-GPU box): no load or store of the step crosses a link")
def test_two_distinct_devices():
    count = 8 * 1024 * 2 + 11
    for wire in WIRES:
        clip = C.clip_of(2, count, wire, "half")
        res = _ranks([0, 1], lambda comm: C.three_clipped_steps(comm, count, wire, clip), Z.capacity(count))
        ref = C.clip_trajectory(2, count, wire, "half")
        bound = (max(b - a for a, b in zero1_slices(count, 2, wire)) / 256 + 32) * 2.0 ** -25
        for r in range(2):
            for t, (state, out, _, _, norm) in enumerate(res[r][1]):
                _close(state, ref[t][0][r], f"devices 0,1 {wire} rank {r} step {t + 1}")
                assert abs(norm - ref[t][2]) / ref[t][2] <= bound and norm == res[0][1][t][4]
                np.testing.assert_array_equal(out, res[0][1][t][1])
