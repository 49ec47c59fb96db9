"""CPU tests of the clipped ZeRO-1 step through the peer communicator's host backend: barrier A, launch 1 (the
rank's slice summed into its own stash, the sum of squares returned), barrier N carrying every rank's sum of squares
through the store, launch 2 (AdamW from the stash with the clipped grad_scale, pushed), barrier B.  Bits against
ops/peer_ref.zero1_step_ref(clip_norm=...), the race detector on the three-barrier protocol, the descriptor's clip,
the store encoding of the published value, the one formula against models/optim_ref.dev_hyper_ref, and the residuals of
error feedback, which clipping must leave alone.  Inputs and helpers are those of tests/test_peer_zero1_cpu.py; the GPU
tests (tests/test_gpu_peer_zero1_clip.py) take their references from here."""
import functools
import math

import numpy as np
import pytest

import test_peer_zero1_cpu as Z
from gpu_topology_on_k8s_amd.models.optim_ref import dev_hyper_ref
from gpu_topology_on_k8s_amd.ops.peer_ref import (clip_grad_scale, reduce_scatter_q8_ref, reduce_scatter_ref, zero1_slices, zero1_sqnorm_ref,
                                                   zero1_step_ref)
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

KS = Z.KS
WIRES = Z.WIRES
HP = Z.HP
CLIPS = ("half", "loose")  # half the reference norm of step 1: every step clips; four times it: the factor is 1


def mean(k):
    return float(np.float32(1.0 / k))


@functools.lru_cache(maxsize=None)
def norm1(k, count, wire):
    """The reference's global norm of step 1's mean gradient."""
    pieces = (reduce_scatter_q8_ref if wire == "fp8" else reduce_scatter_ref)(list(Z.grads(k, count, 0)), "bf16", "fp32", mean(k))
    return clip_grad_scale(zero1_sqnorm_ref(pieces), 1.0, float("inf"))[0]


def clip_of(k, count, wire, which):
    return {"half": 0.5, "loose": 4.0}[which] * norm1(k, count, wire)


@functools.lru_cache(maxsize=None)
def clip_trajectory(k, count, wire, which, steps=3, ef=False):
    """The reference's states, weights, norm (and residuals) after each of ``steps`` clipped steps from weights0."""
    st = Z.states0(k, count, wire)
    res = [np.zeros(32 * (-(-count // 32)), np.float32) for _ in range(k)] if ef else None
    clip, out = clip_of(k, count, wire, which), []
    for t in range(1, steps + 1):
        st, w, norm = zero1_step_ref(list(Z.grads(k, count, t - 1)), st, "bf16", mean(k), Z.hyper(t), wire, res, clip_norm=clip)
        out.append((st, w, norm, None if res is None else [r.copy() for r in res]))
    return out


def three_clipped_steps(comm, count, wire, clip, ef=False):
    """zero1_init from weights0 and three clipped steps of grads: per step this rank's state, its out[0, count), the
    barriers and launches the step took and the norm it returned."""
    k = comm.world
    first, n = comm.zero1_init(count, Z.weights0(count), wire)
    got = []
    for t in range(1, 4):
        comm.write(Z.grads(k, count, t - 1)[comm.rank])
        before, launches = comm.barriers, comm.launches
        norm = comm.zero1_step(step=t, error_feedback=ef, clip_norm=clip, **HP)
        got.append((comm.zero1_state(), comm.read(0, count, "bf16"), comm.barriers - before, comm.launches - launches, norm))
    return (first, n), got


# -- 1. the formula -----------------------------------------------------------------------------------
def test_clip_grad_scale_is_dev_hyper_refs_formula_nan_and_inf_included():
    totals = [0.0, 5e-324, 1e-30, 1e-12, 0.25, 1.0, 2.0, 88952.0, 1e12, 3.4e38 ** 2, float("inf"), float("nan")]
    for total in totals:
        for gs in (1.0, 0.5, 1.0 / 1024):
            for clip in (1e-3, 1.0, 7.5, 1e6):
                norm, got = clip_grad_scale(total, gs, clip)
                want = dev_hyper_ref([1e-3, 0.9, 0.95, 1e-8, 0.1, gs, clip, 0.0], 3.0, total)[5]
                assert (math.isnan(got) and math.isnan(want)) or got == want, (total, gs, clip, got, want)
                assert (math.isnan(norm) and math.isnan(total)) or norm == math.sqrt(total) * gs
    assert math.isnan(clip_grad_scale(float("nan"), 1.0, 1.0)[1])   # a NaN norm passes: no fmin
    assert math.isnan(clip_grad_scale(float("nan"), 1.0, float("inf"))[1])
    assert clip_grad_scale(float("inf"), 0.5, 1.0) == (float("inf"), 0.0)  # an infinite norm: the factor 0
    assert clip_grad_scale(4.0, 0.5, float("inf")) == (1.0, 0.5)           # inf measures and never clips
    assert clip_grad_scale(4.0, 1.0, 4.0) == (2.0, 1.0)                    # under the bound: the factor is exactly 1
    norm, gs = clip_grad_scale(4.0, 1.0, 1.0)
    assert norm == 2.0 and gs == 1.0 / (2.0 + float(np.float32(1e-6)))


def test_zero1_sqnorm_ref_is_exact_and_ignores_zero_padding():
    rng = np.random.default_rng(11)
    a, b = rng.standard_normal(1000, dtype=np.float32), rng.standard_normal(37, dtype=np.float32)
    want = math.fsum(float(x) * float(x) for x in a) + math.fsum(float(x) * float(x) for x in b)
    assert zero1_sqnorm_ref([a, b]) == want
    assert zero1_sqnorm_ref([np.concatenate([a, np.zeros(24, np.float32)]), b[::-1].copy()]) == want
    assert zero1_sqnorm_ref([a[:0], b[:0]]) == 0.0
    assert zero1_sqnorm_ref([np.array([3e38], np.float32)]) == float(np.float32(3e38)) ** 2  # about 9e76: no overflow in float64
    assert math.isinf(zero1_sqnorm_ref([np.array([1.0, -np.inf], np.float32)])) and math.isnan(zero1_sqnorm_ref([np.array([np.inf, np.nan], np.float32)]))


# -- 2. three clipped steps, bit for bit, and the three-barrier protocol ------------------------------
@pytest.mark.parametrize("which", CLIPS)
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_three_clipped_steps_equal_the_reference_bit_for_bit(k, wire, which):
    for count in Z.counts(k):
        clip = clip_of(k, count, wire, which)
        fabric, results, errors = Z._run_threads(k, lambda comm: three_clipped_steps(comm, count, wire, clip), Z.capacity(count))
        assert not errors, errors
        ref = clip_trajectory(k, count, wire, which)
        plan = zero1_slices(count, k, wire)
        for r in range(k):
            _, got = results[r]
            for t, (state, out, barriers, _, norm) in enumerate(got):
                assert barriers == 3
                assert len(state) == 3  # the stash is scratch, no part of the state
                assert all(Z._same(a, b) for a, b in zip(state, ref[t][0][r])), (k, count, wire, r, t)
                assert Z._same(out, ref[t][1]), (k, count, wire, r, t)
                assert isinstance(norm, float) and norm == ref[t][2], (k, count, wire, r, t)
        if which == "half":
            assert not Z._same(ref[2][1], Z.trajectory(k, count, wire)[2][1])  # clipping does change the trajectory
        else:
            assert Z._same(ref[2][1], Z.trajectory(k, count, wire)[2][1])      # a factor of 1 changes nothing
        # the race detector: launch 1 reads the peers and writes the rank's own stash, launch 2 writes every out
        assert fabric.conflicts() == []
        log = fabric.log
        assert all(a[0] == a[1] for a in log if a[2] in ("zero1", "residual"))
        assert not any(a[2] == "out" and a[5] == "r" and a[0] != a[1] for a in log)
        src = "packed" if wire == "fp8" else "window"
        busy = [r for r in range(k) if plan[r][1] > plan[r][0]]
        for r in busy:
            assert {a[1] for a in log if a[0] == r and a[2] == "out" and a[5] == "w"} == set(range(k))
            assert {a[1] for a in log if a[0] == r and a[2] == src and a[5] == "r"} == set(range(k))
            reads = {a[6] for a in log if a[0] == r and a[2] == src and a[5] == "r"}
            writes = {a[6] for a in log if a[0] == r and a[2] == "out" and a[5] == "w"}
            assert {e + 1 for e in reads} == writes  # every peer read lies one barrier, N, before the stores into out
        for r in set(range(k)) - set(busy):
            assert not any(a[0] == r and a[2] == "out" and a[5] == "w" for a in log)
        assert fabric.launches == 3 * (2 * len(busy) + (k if wire == "fp8" else 0))


def test_none_is_the_unclipped_path_and_returns_none():
    k, count = 3, 8 * 100 * 3 + 5

    def body(comm):
        comm.zero1_init(count, Z.weights0(count))
        comm.write(Z.grads(k, count, 0)[comm.rank])
        before = comm.barriers
        ret = comm.zero1_step(step=1, clip_norm=None, **HP)
        return ret, comm.barriers - before, comm._b.zero1_bytes, comm.zero1_state(), comm.read(0, count, "bf16")

    fabric, results, errors = Z._run_threads(k, body, Z.capacity(count))
    assert not errors, errors
    ref = Z.trajectory(k, count, "native")
    plan = zero1_slices(count, k)
    for r in range(k):
        ret, barriers, nbytes, state, out = results[r]
        assert ret is None and barriers == 2 and nbytes == 12 * (plan[r][1] - plan[r][0])  # no stash was made
        assert all(Z._same(a, b) for a, b in zip(state, ref[0][0][r])) and Z._same(out, ref[0][1])


# -- 3. the descriptor and the refusals ---------------------------------------------------------------
@pytest.mark.parametrize("other", (2.0, None, float("inf")))
def test_ranks_that_disagree_on_clip_norm_get_a_mismatch_before_any_launch(other):
    k, count = 3, 8 * 64 * 3

    def body(comm):
        comm.zero1_init(count, Z.weights0(count))
        comm.write(Z.grads(k, count, 0)[comm.rank])
        comm.zero1_step(step=1, clip_norm=other if comm.rank == 1 else 1.0, **HP)

    fabric, _, errors = Z._run_threads(k, body, Z.capacity(count))
    assert sorted(errors) == list(range(k)) and all(isinstance(e, pc.PeerCommMismatch) for e in errors.values()), errors
    assert '"clip"' in str(errors[0])
    assert fabric.launches == 0 and not any(a[2] in ("out", "window") and a[5] == "r" and a[0] != a[1] for a in fabric.log)


def test_refusals_and_the_stash_bytes():
    store, fabric = pc.MemoryStore(), pc.HostFabric(2, 4096)
    comm = pc.PeerComm(0, 2, 0, store, 4096, backend="host", fabric=fabric)
    with pytest.raises(ValueError, match="zero1_init"):
        comm.zero1_step(step=1, clip_norm=1.0, **HP)
    assert comm.zero1_init(256, Z.weights0(256)) == (0, 128)
    for bad in (0.0, -1.0, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="clip_norm"):
            comm.zero1_step(step=1, clip_norm=bad, **HP)
    with pytest.raises(ValueError, match="error_feedback"):
        comm.zero1_step(step=1, clip_norm=1.0, error_feedback=True, **HP)
    assert comm.barriers == 0 and fabric.launches == 0 and comm._b.zero1_bytes == 3 * 128 * 4  # and no stash was made
    with pytest.raises(ValueError):
        comm._b.zero1_read_state(3, 0, 1)  # no stash yet
    with pytest.raises(ValueError):
        comm._b.reduce_sqnorm_stash(0, 1, 1.0)
    comm._b.zero1_stash_alloc()
    assert comm._b.zero1_bytes == 4 * 128 * 4 and not comm._b.zero1_read_state(3, 0, 128).any()
    comm._b.zero1_stash_alloc()
    assert comm._b.zero1_bytes == 4 * 128 * 4
    for bad in (lambda: comm._b.reduce_sqnorm_stash(0, 17, 1.0), lambda: comm._b.reduce_q8_sqnorm_stash(0, 5, 1.0),
                lambda: comm._b.adamw_push(0, 17, Z.hyper(1)), lambda: comm._b.zero1_read_state(3, 120, 16),
                lambda: comm._b.zero1_read_state(4, 0, 1)):
        with pytest.raises(ValueError):
            bad()
    assert comm._b.reduce_sqnorm_stash(5, 5, 1.0) == 0.0 and fabric.launches == 0  # an empty slice: no launch, 0.0
    comm.zero1_init(256, Z.weights0(256))  # a new init frees the stash
    assert comm._b.zero1_bytes == 3 * 128 * 4


# -- 4. what barrier N carries -------------------------------------------------------------------------
def test_nan_inf_and_a_subnormal_total_survive_the_store_exactly():
    k = 3
    values = [[float("nan"), 1.5, 0.0], [float("inf"), 5e-324, 2.0 ** -1074 * 3], [0.1, 1.7976931348623157e308, 88952.0],
              [2.2250738585072014e-308, 1 / 3, float("inf")]]

    def body(comm):
        return [comm._exchange_sqnorm(i, vals[comm.rank]) for i, vals in enumerate(values)], comm.barriers

    fabric, results, errors = Z._run_threads(k, body, 4096)
    assert not errors, errors
    for r in range(k):
        got, barriers = results[r]
        assert barriers == len(values)
        for g, want in zip(got, values):
            for x, y in zip(g, want):  # a NaN comes back a NaN; every other value, the subnormals too, with its bits
                assert math.isnan(x) if math.isnan(y) else x.hex() == y.hex(), (r, x, y)


def test_the_sqnorm_keys_leave_the_store():
    k, count, steps = 2, 8 * 64 * 2, 8
    per_step = 2 * k + 6  # k descriptors, k sums of squares, three barriers of two keys

    def body(comm):
        comm.zero1_init(count, Z.weights0(count))
        for t in range(1, steps + 1):
            comm.write(Z.grads(k, count, (t - 1) % 3)[comm.rank])
            comm.zero1_step(step=t, clip_norm=1.0, **HP)
        return comm._store.num_keys()

    _, results, errors = Z._run_threads(k, body, Z.capacity(count))
    assert not errors, errors
    assert max(results.values()) <= 2 * per_step < steps * per_step  # keys are deleted two barriers later, the published sums too


# -- 5. error feedback ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (2, 3))
def test_clipping_leaves_the_error_feedback_residuals_alone(k):
    count = 512 * k + 37
    n = 32 * (-(-count // 32))
    clip = clip_of(k, count, "fp8", "half")

    def body(comm):
        _, got = three_clipped_steps(comm, count, "fp8", clip, ef=True)
        return got, comm.residual(0, n)

    fabric, results, errors = Z._run_threads(k, body, Z.capacity(count))
    assert not errors, errors
    ref = clip_trajectory(k, count, "fp8", "half", 3, True)
    unclipped = Z.trajectory(k, count, "fp8", 3, True)
    for r in range(k):
        got, residual = results[r]
        for t in range(3):
            assert all(Z._same(a, b) for a, b in zip(got[t][0], ref[t][0][r])) and Z._same(got[t][1], ref[t][1]) and got[t][4] == ref[t][2]
        assert Z._same(residual, ref[2][3][r])
        assert Z._same(residual, unclipped[2][2][r])  # clipping happens after the sum
    assert not Z._same(ref[2][1], unclipped[2][1])
    assert fabric.conflicts() == []
