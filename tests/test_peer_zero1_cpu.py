"""CPU tests of the ZeRO-1 step through the peer communicator's host backend: rank r sums slice r of every window,
applies AdamW to its own master/m/v and stores the new bf16 weights into slice r of every rank's out, in one
launch between the two barriers.  Bits against ops/peer_ref.zero1_step_ref, every rank's out alike, the race
detector on the peer writes (clean on the protocol, non-empty on a step that skips barrier A), the descriptor's
hyper-parameters, the refusals and a restored state."""
import functools
import threading

import numpy as np
import pytest

from gpu_topology_on_k8s_amd.ops.peer_ref import (adamw_ref, allreduce_ref, bf16_round, bf16_to_f32, reduce_scatter_ref, zero1_slices,
                                                   zero1_step_ref)
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

KS = (2, 3, 8, 16)
WIRES = ("native", "fp8")
HP = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1)
CI = 40  # the case index of these tests' inputs: case_input(CI, issue, rank, count, "bf16")


def counts(k):
    return (8 * (k - 1), 8 * 1024 * k + 11)  # some slices empty; tiles, a tail and padding


def capacity(count):
    return 64 * (-(-count // 32))  # whole blocks of bf16: enough for both wires


def hyper(step, grad_scale=1.0, **over):
    h = {**HP, **over}
    return [float(x) for x in np.array([h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"], grad_scale,
                                        1 - h["beta1"] ** step, 1 - h["beta2"] ** step], np.float32)]


@functools.lru_cache(maxsize=None)
def weights0(count):
    w = bf16_round(np.random.default_rng([CI, count]).standard_normal(count, dtype=np.float32))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def grads(k, count, issue):
    xs = tuple(pc.case_input(CI, issue, p, count, "bf16") for p in range(k))
    for a in xs:
        a.setflags(write=False)
    return xs


def states0(k, count, wire):
    out = []
    for a, b in zero1_slices(count, k, wire):
        master = np.zeros(b - a, np.float32)
        mine = bf16_to_f32(weights0(count)[a:min(b, count)])
        master[:mine.size] = mine
        out.append((master, np.zeros(b - a, np.float32), np.zeros(b - a, np.float32)))
    return out


@functools.lru_cache(maxsize=None)
def trajectory(k, count, wire, steps=3, ef=False):
    """The reference's states, weights (and residuals) after each of ``steps`` steps from weights0."""
    st = states0(k, count, wire)
    res = [np.zeros(32 * (-(-count // 32)), np.float32) for _ in range(k)] if ef else None
    out = []
    for t in range(1, steps + 1):
        st, w = zero1_step_ref(list(grads(k, count, t - 1)), st, "bf16", float(np.float32(1.0 / k)), hyper(t), wire, res)
        out.append((st, w, None if res is None else [r.copy() for r in res]))
    return out


def _run_threads(k, body, cap, comm_cls=pc.PeerComm, timeout_s=30.0):
    store, fabric = pc.MemoryStore(timeout_s=timeout_s), pc.HostFabric(k, cap)
    results, errors = {}, {}

    def run(r):
        try:
            results[r] = body(comm_cls(r, k, 0, store, cap, timeout_s=timeout_s, backend="host", fabric=fabric))
        except BaseException as e:  # handed to the test's thread
            errors[r] = e

    threads = [threading.Thread(target=run, args=(r,)) for r in range(k)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not any(t.is_alive() for t in threads)
    return fabric, results, errors


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(pc._bits(got), pc._bits(want))


# -- 1. the reference ---------------------------------------------------------------------------------
def test_adamw_ref_is_adam8_in_float32():
    rng = np.random.default_rng(3)
    p, g = rng.standard_normal(64, dtype=np.float32), rng.standard_normal(64, dtype=np.float32)
    m, v = np.abs(rng.standard_normal(64, dtype=np.float32)) * 0.01, np.abs(rng.standard_normal(64, dtype=np.float32)) * 0.001
    h = hyper(3, grad_scale=0.5)
    np1, nm1, nv1, w = adamw_ref(p, m, v, g, h)
    f = np.float32
    lr, b1, b2, eps, wd, gs, bc1, bc2 = (f(x) for x in h)
    for i in (0, 17, 63):  # the same expressions, one scalar float32 operation at a time
        gr = f(g[i] * gs)
        mi = f(f(b1 * m[i]) + f(f(f(1) - b1) * gr))
        vi = f(f(b2 * v[i]) + f(f(f(f(1) - b2) * gr) * gr))
        upd = f(f(mi / bc1) / f(f(np.sqrt(f(vi / bc2))) + eps))
        pi = f(p[i] - f(lr * f(upd + f(wd * p[i]))))
        assert (nm1[i], nv1[i], np1[i]) == (mi, vi, pi)
    assert all(a.dtype == np.float32 for a in (np1, nm1, nv1)) and np.array_equal(w, bf16_round(np1))
    # beta1 = beta2 = lr = wd = 0: m is the scaled gradient, v its square, master untouched
    zp, zm, zv, zw = adamw_ref(p, m, v, g, hyper(1, beta1=0.0, beta2=0.0, lr=0.0, weight_decay=0.0))
    assert np.array_equal(zm, g) and np.array_equal(zv, g * g) and np.array_equal(pc._bits(zp), pc._bits(p))
    # a NaN and an Inf reach their own elements alone
    g2 = g.copy()
    g2[5], g2[9] = np.nan, np.inf
    out = adamw_ref(p, m, v, g2, h)
    hit = np.zeros(64, bool)
    hit[[5, 9]] = True
    for a, b in zip(out, (np1, nm1, nv1, w)):
        assert np.array_equal(pc._bits(a)[~hit], pc._bits(b)[~hit])
    assert all(not np.isfinite(a[i]) for a in out[:3] for i in (5, 9))


def test_zero1_slices_and_step_ref_are_built_on_the_reduce_scatter():
    for k in KS:
        for count in counts(k):
            for wire in WIRES:
                sl = zero1_slices(count, k, wire)
                unit = 32 if wire == "fp8" else 8
                assert sl[0][0] == 0 and all(a % unit == 0 and b % unit == 0 and a <= b for a, b in sl)
                assert all(sl[i][1] == sl[i + 1][0] for i in range(k - 1)) and count <= sl[-1][1] < count + unit
    k, count = 3, 8 * 100 * 3 + 5
    xs, st = list(grads(k, count, 0)), states0(k, count, "native")
    new, w = zero1_step_ref(xs, st, "bf16", 1.0 / k, hyper(1))
    pieces = reduce_scatter_ref(xs, "bf16", "fp32", 1.0 / k)
    assert w.dtype == np.uint16 and w.shape == (count,)
    for r, (a, b) in enumerate(zero1_slices(count, k)):
        g = np.zeros(b - a, np.float32)
        g[:pieces[r].size] = pieces[r]
        want = adamw_ref(*st[r], g, hyper(1))
        assert all(_same(x, y) for x, y in zip(new[r], want[:3]))
        assert np.array_equal(w[a:min(b, count)], want[3][:min(b, count) - a])
        assert not want[3][min(b, count) - a:].any()  # the padding's weights are zero
    with pytest.raises(ValueError, match="bf16"):
        zero1_step_ref([x.astype(np.float32) for x in xs], st, "fp32", 1.0, hyper(1))
    with pytest.raises(ValueError, match="fp8"):
        zero1_step_ref(xs, st, "bf16", 1.0, hyper(1), None, residuals=[np.zeros(32, np.float32)] * k)
    with pytest.raises(ValueError):
        zero1_slices(64, 2, "fp8x2")


# -- 2. three steps, bit for bit, every rank's out alike ----------------------------------------------
def three_steps(comm, count, wire, ef=False):
    """zero1_init from weights0 and three steps of grads: per step this rank's state and its out[0, count)."""
    k = comm.world
    first, n = comm.zero1_init(count, weights0(count), wire)
    got = []
    for t in range(1, 4):
        comm.write(grads(k, count, t - 1)[comm.rank])
        before, launches = comm.barriers, comm.launches
        comm.zero1_step(step=t, error_feedback=ef, **HP)
        got.append((comm.zero1_state(), comm.read(0, count, "bf16"), comm.barriers - before, comm.launches - launches))
    return (first, n), got


@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_three_steps_equal_the_reference_bit_for_bit(k, wire):
    for count in counts(k):
        fabric, results, errors = _run_threads(k, lambda comm: three_steps(comm, count, wire), capacity(count))
        assert not errors, errors
        ref = trajectory(k, count, wire)
        plan = zero1_slices(count, k, wire)
        for r in range(k):
            (first, n), got = results[r]
            assert (first, n) == (min(count, plan[r][0]), min(count, plan[r][1]) - min(count, plan[r][0]))
            for t, (state, out, barriers, _) in enumerate(got):
                assert barriers == 2
                assert all(_same(a, b) for a, b in zip(state, ref[t][0][r])), (k, count, wire, r, t)
                assert _same(out, ref[t][1]), (k, count, wire, r, t)
                assert np.array_equal(out, results[0][1][t][1])  # every rank's out is rank 0's
        assert fabric.conflicts() == []
        log = fabric.log
        assert any(a[2] == "out" and a[5] == "w" and a[0] != a[1] for a in log)      # peers do write a rank's out
        assert not any(a[2] == "out" and a[5] == "r" and a[0] != a[1] for a in log)  # and nobody reads a peer's
        assert all(a[0] == a[1] for a in log if a[2] in ("zero1", "residual"))        # the state is its owner's alone
        busy = [r for r in range(k) if plan[r][1] > plan[r][0]]
        for r in busy:  # a rank with a slice wrote every owner's out and read every rank's window or packed buffer
            assert {a[1] for a in log if a[0] == r and a[2] == "out" and a[5] == "w"} == set(range(k))
            assert {a[1] for a in log if a[0] == r and a[2] == ("packed" if wire == "fp8" else "window") and a[5] == "r"} == set(range(k))
        for r in set(range(k)) - set(busy):  # an empty slice: nothing written anywhere, both barriers taken all the same
            assert not any(a[0] == r and a[2] == "out" and a[5] == "w" for a in log)
        # one launch per rank with a slice and step, and on the fp8 wire every rank's quantize
        assert fabric.launches == 3 * (len(busy) + (k if wire == "fp8" else 0))


@pytest.mark.parametrize("k", (2, 3))
def test_error_feedback_steps_keep_the_chained_reference(k):
    count = 512 * k + 37
    n = 32 * (-(-count // 32))

    def body(comm):
        _, got = three_steps(comm, count, "fp8", ef=True)
        return got, comm.residual(0, n)

    fabric, results, errors = _run_threads(k, body, capacity(count))
    assert not errors, errors
    ref = trajectory(k, count, "fp8", 3, True)
    for r in range(k):
        got, residual = results[r]
        for t in range(3):
            assert all(_same(a, b) for a, b in zip(got[t][0], ref[t][0][r])) and _same(got[t][1], ref[t][1])
        assert _same(residual, ref[2][2][r])
    assert not _same(ref[2][1], trajectory(k, count, "fp8")[2][1])  # feedback does change the trajectory
    assert fabric.conflicts() == []


# -- 3. among the other collectives -------------------------------------------------------------------
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", (2, 3, 8))
def test_interleaved_with_the_other_collectives_there_is_no_conflict(k, wire):
    count = 8 * 64 * k + 11
    other = 8 * 24 * k - 5  # its slices overlap the step's
    trajectory(k, count, wire)  # made once, before the ranks ask for it

    def body(comm):
        r, bad = comm.rank, 0
        comm.zero1_init(count, weights0(count), wire)
        ref = trajectory(k, count, wire)
        for t in range(1, 4):
            xs = [pc.case_input(60 + t, 0, p, other, "bf16") for p in range(k)]
            comm.write(xs[r])
            comm.all_reduce(other, "bf16", "twoshot" if t != 2 else "push")
            bad += not _same(comm.read(0, other, "bf16"), allreduce_ref(xs, "bf16"))
            comm.write(grads(k, count, t - 1)[r])
            comm.zero1_step(step=t, **HP)
            bad += not _same(comm.read(0, count, "bf16"), ref[t - 1][1])
            per = 8 * 5
            comm.write(xs[r][:per], comm.gather_slot(per, "bf16"))
            nv = comm.all_gather(per, "bf16")
            bad += not _same(comm.read(0, k * nv * 8, "bf16"), np.concatenate([x[:per] for x in xs]))
        return bad

    fabric, results, errors = _run_threads(k, body, capacity(count))
    assert not errors, errors
    assert [results[r] for r in range(k)] == [0] * k
    assert fabric.conflicts() == []
    assert any(a[2] == "out" and a[5] == "r" and a[0] != a[1] for a in fabric.log)  # the two-shots' gathers do read a peer's out


class _NoBarrierA(pc.PeerComm):
    """A collective that launches without meeting the other ranks first (test-only): a step's stores into a peer's
    out are then not ordered after that peer's last read of it."""

    def _enter(self, desc):
        self._seq += 1
        self._b.synchronize()


@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", (2, 3))
def test_a_step_that_writes_out_before_barrier_a_is_reported(k, wire):
    count = 8 * 64 * k

    def body(comm):
        comm.zero1_init(count, weights0(count), wire)
        for t in (1, 2):
            comm.write(grads(k, count, t - 1)[comm.rank])
            comm.zero1_step(step=t, **HP)
            comm.read(0, count, "bf16")  # in the epoch in which the peers' next step, unordered, overwrites it

    fabric, _, errors = _run_threads(k, body, capacity(count), comm_cls=_NoBarrierA)
    assert not errors, errors
    found = fabric.conflicts()
    assert found
    assert any(w[2] == "out" and w[0] != w[1] and a[0] == w[1] and a[5] == "r" for w, a in found)  # a peer's write, the owner's read
    fabric, _, errors = _run_threads(k, body, capacity(count))
    assert not errors and fabric.conflicts() == []


# -- 4. the descriptor and the refusals ---------------------------------------------------------------
@pytest.mark.parametrize("k", (2, 3))
def test_a_mismatched_lr_is_a_mismatch_on_every_rank_before_any_launch(k):
    count = 8 * 64 * k

    def body(comm):
        comm.zero1_init(count, weights0(count))
        comm.write(grads(k, count, 0)[comm.rank])
        comm.zero1_step(step=1, **{**HP, "lr": 2e-3 if comm.rank == 1 else 1e-3})

    fabric, _, errors = _run_threads(k, body, capacity(count))
    assert sorted(errors) == list(range(k)) and all(isinstance(e, pc.PeerCommMismatch) for e in errors.values()), errors
    assert '"op": "zero1_step"' in str(errors[0]) and '"hyper"' in str(errors[0])
    assert fabric.launches == 0 and not any(a[2] == "out" for a in fabric.log)


def test_refusals_come_before_any_barrier_or_launch():
    store, fabric = pc.MemoryStore(), pc.HostFabric(2, 4096)
    comm = pc.PeerComm(0, 2, 0, store, 4096, backend="host", fabric=fabric)
    w = weights0(256)
    with pytest.raises(ValueError, match="zero1_init"):
        comm.zero1_step(step=1, **HP)
    with pytest.raises(ValueError, match="zero1_init"):
        comm.zero1_state()
    with pytest.raises(ValueError, match="fp8x2"):
        comm.zero1_init(256, w, wire="fp8x2")
    with pytest.raises(ValueError, match="zero1_init"):  # the refused init recorded nothing
        comm.zero1_step(step=1, **HP)
    with pytest.raises(ValueError, match="window"):
        comm.zero1_init(4096, weights0(4096))
    with pytest.raises(ValueError, match="weights"):
        comm.zero1_init(256, w[:255])
    with pytest.raises(ValueError, match="weights"):
        comm.zero1_init(256, bf16_to_f32(w))  # fp32 weights, like fp32 windows, are refused
    assert comm.zero1_init(256, w, wire="native") == (0, 128)
    with pytest.raises(ValueError, match="error_feedback"):
        comm.zero1_step(step=1, error_feedback=True, **HP)
    with pytest.raises(ValueError, match="step"):
        comm.zero1_step(step=0, **HP)
    with pytest.raises(ValueError, match="state"):
        comm.zero1_init(256, w, state=(np.zeros(64, np.float32),) * 3)
    with pytest.raises(ValueError):
        comm._b.reduce_adamw_push(0, 17, 1.0, hyper(1))  # more vectors than the state holds
    with pytest.raises(ValueError):
        comm._b.reduce_q8_adamw_push(0, 65, 1.0, hyper(1))
    assert fabric.launches == 0 and comm.barriers == 0 and not any(a[2] != "zero1" for a in fabric.log)
    fresh = pc.PeerComm(1, 2, 0, pc.MemoryStore(), 4096, backend="host", fabric=pc.HostFabric(2, 4096))
    assert fresh._b.zero1_bytes == 0 and comm._b.zero1_bytes == 3 * 128 * 4  # a communicator that never asks holds none


# -- 5. a restored state ------------------------------------------------------------------------------
@pytest.mark.parametrize("wire", WIRES)
def test_a_restored_state_continues_the_trajectory_bit_for_bit(wire):
    k, count = 3, 8 * 100 * 3 + 5
    ref = trajectory(k, count, wire)

    def first_two(comm):
        comm.zero1_init(count, weights0(count), wire)
        for t in (1, 2):
            comm.write(grads(k, count, t - 1)[comm.rank])
            comm.zero1_step(step=t, **HP)
        return comm.zero1_state()

    _, saved, errors = _run_threads(k, first_two, capacity(count))
    assert not errors, errors

    def third(comm):
        comm.zero1_init(count, np.zeros(count, np.uint16), wire, state=saved[comm.rank])  # the weights play no part
        comm.write(grads(k, count, 2)[comm.rank])
        comm.zero1_step(step=3, **HP)
        return comm.zero1_state(), comm.read(0, count, "bf16")

    fabric, results, errors = _run_threads(k, third, capacity(count))
    assert not errors, errors
    for r in range(k):
        assert all(_same(a, b) for a, b in zip(results[r][0], ref[2][0][r])) and _same(results[r][1], ref[2][1])
    assert fabric.conflicts() == []
