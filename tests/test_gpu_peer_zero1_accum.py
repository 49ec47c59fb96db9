"""GPU tests of fp32 gradient accumulation in the ZeRO-1 step (peer_reduce_sqnorm_accum_kernel and
peer_q8_sum_sqnorm_accum_kernel of csrc/probe/peer_zero1.h) through the peer communicator's device backend on thread
ranks: ``zero1_accumulate`` stores the first micro-batch's scaled sum into the rank's fp32 stash and adds every later
one to it, and ``zero1_step(accumulated=True)`` adds the last, stores the total back, squares it and applies AdamW from
the stash.

Members repeat device 0; one test runs on two devices where two are visible.  The accumulator is compared bit for bit
with ops/peer_ref.zero1_accumulate_ref (the kernel multiplies and adds in two roundings, as the reference does); the
norm is compared bit for bit on gradients from {-1, 0, 1}, where every fp32 order of summation is exact; the update is
held to ops/peer_ref.zero1_step_ref(accumulated=...) at the tolerances of tests/test_gpu_peer_zero1.py (rtol 1e-5; atol
1e-6 for master and m, 1e-7 for v).  Inputs and references are made once (tests/test_peer_zero1_accum_cpu.py,
tests/test_peer_zero1_cpu.py, tests/test_peer_zero1_loops_cpu.py) and are read-only."""
import functools
import math

import numpy as np
import pytest

import test_gpu_peer_zero1_clip as G
import test_peer_zero1_accum_cpu as A
import test_peer_zero1_clip_cpu as C
import test_peer_zero1_cpu as Z
import test_peer_zero1_loops_cpu as L
from gpu_topology_on_k8s_amd.ops.peer_ref import (bf16_round, bits, clip_grad_scale, is_nan_bits, launch_u, launch_walk, mismatches,
                                                   zero1_accumulate_ref, zero1_slices, zero1_sqnorm_ref, zero1_step_ref)
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

pytestmark = pytest.mark.gpu

KS = [2, 3, 8, 16]
WIRES = ["native", "fp8"]
HP = Z.HP
M = A.M
_close = G._close


def _ranks(devices, body, cap, **kw):
    return pc.run_thread_ranks(devices, body, cap, timeout_s=30.0, **kw)


def _norm_bound(plan):
    """The relative bound tests/test_gpu_peer_zero1_clip.py derives for launch 1's norm; the adding launch sums its
    squares in the same order."""
    return (max(b - a for a, b in plan) / 256 + 32) * 2.0 ** -25


# -- 1. the accumulator, bit for bit --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def accs_ref(k, count, wire):
    """The ranks' accumulators after each of M accumulates of Z.grads(k, count, 0..M-1)."""
    out, acc = [], None
    for j in range(M):
        acc = zero1_accumulate_ref(acc, list(Z.grads(k, count, j)), "bf16", C.mean(k), wire)
        out.append(acc)
    return out


def accumulate_m(comm, count, wire):
    """zero1_init and M accumulates of Z.grads: after each the rank's stash and the launches the call made."""
    k = comm.world
    comm.zero1_init(count, Z.weights0(count), wire)
    a, b = zero1_slices(count, k, wire)[comm.rank]
    got = []
    for j in range(M):
        comm.write(Z.grads(k, count, j)[comm.rank])
        launches, barriers = comm.launches, comm.barriers
        comm.zero1_accumulate()
        got.append((comm._b.zero1_read_state(3, 0, b - a), comm.launches - launches, comm.barriers - barriers, comm.zero1_accumulated))
    comm.zero1_reset_accumulated()
    return got


def _assert_accumulators(res_of_rank, k, count, wire, what):
    ref = accs_ref(k, count, wire)
    plan = zero1_slices(count, k, wire)
    for r, (a, b) in enumerate(plan):
        for j, (stash, launches, barriers, n_acc) in enumerate(res_of_rank(r)):
            where = f"{what} k={k} {wire} count={count} rank {r} after micro-batch {j}"
            assert launches == (wire == "fp8") + (b > a) and barriers == 2 and n_acc == j + 1, where
            assert stash.dtype == np.float32 and stash.shape == (b - a,), where
            np.testing.assert_array_equal(bits(stash), bits(ref[j][r]), err_msg=where)
            assert not stash[max(0, min(count, b) - a):].any(), where  # the padding is zero


@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_the_accumulator_has_the_reference_bits_after_every_call(k, wire):
    for count in Z.counts(k):
        accs_ref(k, count, wire)  # made once, before the ranks run

    res = _ranks([0] * k, lambda comm: [accumulate_m(comm, count, wire) for count in Z.counts(k)], Z.capacity(max(Z.counts(k))))
    for ci, count in enumerate(Z.counts(k)):
        _assert_accumulators(lambda r: res[r][ci], k, count, wire, "accumulator")


# -- 2. the norm of the accumulated total is exact ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def signs(k, count):
    """Per micro-batch every rank's gradient from {-1, 0, 1} as bf16 bit patterns, and the exact integer total over
    micro-batches and ranks.  Both wires carry these values exactly and every partial sum is a small integer."""
    ints = [np.random.default_rng([43, k, count, j]).integers(-1, 2, size=(k, count)) for j in range(M)]
    xs = tuple(tuple(bf16_round(row.astype(np.float32)) for row in batch) for batch in ints)
    for batch in xs:
        for a in batch:
            a.setflags(write=False)
    total = sum(batch.sum(axis=0) for batch in ints)
    total.setflags(write=False)
    return xs, total


def exact_total(k, count, wire):
    _, total = signs(k, count)
    worst = max(int((total[a:min(b, count)] ** 2).sum()) for a, b in zero1_slices(count, k, wire))
    assert worst < 2 ** 24, worst  # a condition: below it fp32 adds these integers exactly in every order
    return int((total ** 2).sum())


@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_the_norm_of_the_accumulated_total_is_exact(k, wire):
    """scale = 1 and clip_norm = inf on gradients from {-1, 0, 1}: the accumulator holds small integers, and the norm
    the accumulated step returns is sqrt of the exact integer total of their squares, the same float on every rank."""
    inputs = {count: signs(k, count)[0] for count in Z.counts(k)}

    def body(comm):
        got = []
        for count in Z.counts(k):
            comm.zero1_init(count, Z.weights0(count), wire)
            for j in range(M - 1):
                comm.write(inputs[count][j][comm.rank])
                comm.zero1_accumulate(scale=1.0)
            comm.write(inputs[count][M - 1][comm.rank])
            launches, barriers = comm.launches, comm.barriers
            norm = comm.zero1_step(step=1, scale=1.0, clip_norm=float("inf"), accumulated=True, **HP)
            a, b = zero1_slices(count, k, wire)[comm.rank]
            got.append((norm, comm.launches - launches, comm.barriers - barriers, comm._b.zero1_read_state(3, 0, b - a)))
        return got

    res = _ranks([0] * k, body, Z.capacity(max(Z.counts(k))))
    for ci, count in enumerate(Z.counts(k)):
        want = math.sqrt(exact_total(k, count, wire))
        total = signs(k, count)[1]
        for r, (a, b) in enumerate(zero1_slices(count, k, wire)):
            norm, launches, barriers, stash = res[r][ci]
            print(f"norm k={k} {wire} count={count} rank {r}: {norm!r} (exact {want!r})")
            assert isinstance(norm, float) and norm == want, (k, wire, count, r, norm, want)
            assert launches == (wire == "fp8") + 2 * (b > a) and barriers == 3
            mine = total[a:min(b, count)].astype(np.float32)
            np.testing.assert_array_equal(stash[:mine.size], mine)  # the total, stored back
            assert not stash[mine.size:].any()


# -- 3. the update --------------------------------------------------------------------------------------
def _assert_steps(res_of_rank, k, count, wire, which, ref, what):
    plan = zero1_slices(count, k, wire)
    bound = _norm_bound(plan)
    first_rank = res_of_rank(0)
    for r, (a, b) in enumerate(plan):
        (first, n), got = res_of_rank(r)
        for t, (accs, stash, state, out, (barriers, launches), norm, left) in enumerate(got):
            where = f"{what} k={k} {wire} clip={which} count={count} rank {r} step {t + 1}"
            for j, (acc, ab, al, n_acc) in enumerate(accs):
                assert ab == 2 and al == (wire == "fp8") + (b > a) and n_acc == j + 1, where
                np.testing.assert_array_equal(bits(acc), bits(ref[t][0][j][r]), err_msg=f"{where} accumulator {j}")
            np.testing.assert_array_equal(bits(stash), bits(ref[t][1][r]), err_msg=where + " total")
            assert barriers == (2 if which is None else 3) and launches == (wire == "fp8") + 2 * (b > a) and left == 0, where
            if which is None:
                assert norm is None, where
            else:
                rel = abs(norm - ref[t][5]) / ref[t][5]
                if r == 0:
                    print(f"norm {where}: {norm!r} reference {ref[t][5]!r} relative {rel:.3e} bound {bound:.3e}")
                assert rel <= bound, (where, norm, ref[t][5], rel, bound)
                assert norm == first_rank[1][t][5], where  # the same float on every rank
            _close(state, ref[t][3][r], where)
            assert np.isfinite(state[0]).all()
            np.testing.assert_array_equal(out[first:first + n], bf16_round(state[0])[:n], err_msg=where)  # the owner's own master, rounded once
            np.testing.assert_array_equal(out, first_rank[1][t][3], err_msg=where + " vs rank 0's out")


@pytest.mark.parametrize("which", A.CLIPS)
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_two_accumulated_steps_follow_the_reference(k, wire, which):
    """Two optimizer steps of M = 3 micro-batches, unclipped, with clip_norm at half the norm of one micro-batch's mean
    (every step clips) and at four times it (the factor is 1).  Every rank's out is the owning rank's master rounded
    once: each rank's own slice against its own master, and every rank's out against rank 0's."""
    clips = {count: A.clip_of(k, count, wire, which) for count in Z.counts(k)}
    for count in Z.counts(k):
        A.trajectory(k, count, wire, which)  # made once, before the ranks run

    res = _ranks([0] * k, lambda comm: [A.accumulated_steps(comm, count, wire, clips[count]) for count in Z.counts(k)],
                 Z.capacity(max(Z.counts(k))))
    for ci, count in enumerate(Z.counts(k)):
        _assert_steps(lambda r: res[r][ci], k, count, wire, which, A.trajectory(k, count, wire, which), "update")


# -- 4. many tiles per block ----------------------------------------------------------------------------
class Comm(L.Capped, pc.PeerComm):
    pass


@functools.lru_cache(maxsize=None)
def loops_ref(k, wire):
    """One optimizer step of two micro-batches at the count of tests/test_peer_zero1_loops_cpu.py, clipped at half the
    norm of the accumulated total, in the layout of A.trajectory.  The first accumulate stores the piece of
    Z.grads(k, count, 0), which L.pieces holds already; the step's launch 1 is the adding launch."""
    count = L.count_of(k, wire)
    acc = list(L.pieces(k, wire))
    last = list(Z.grads(k, count, 1))
    total = zero1_accumulate_ref(acc, last, "bf16", C.mean(k), wire)
    clip = 0.5 * clip_grad_scale(zero1_sqnorm_ref(total), 1.0, float("inf"))[0]
    st, w, norm = zero1_step_ref(last, Z.states0(k, count, wire), "bf16", C.mean(k), Z.hyper(1), wire, clip_norm=clip, accumulated=acc)
    return clip, [([acc], total, None, st, w, norm)]


@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_a_block_that_walks_many_tiles_accumulates_and_steps_alike(k, wire):
    """Under a grid cap of two blocks, at the counts of tests/test_peer_zero1_loops_cpu.py: block 0 of the adding launch
    takes at least two tiles, block 1 fewer, and the remainder loop runs.  One accumulate stores and the accumulated step
    adds: the stash after it is the adding launch's accumulator, held to the bits of test 1, and the update to test 3's
    tolerances."""
    count = L.count_of(k, wire)
    name = "peer_q8_sum_sqnorm_accum" if wire == "fp8" else "peer_reduce_sqnorm_accum"
    U = launch_u(name, k)
    units = L.slice_elems(k, wire) // (16 if wire == "fp8" else 8)
    tiles, trips = launch_walk(units, L.GRID, U)
    L.assert_many_tiles(tiles, trips, U, (name, k, wire))
    clip, ref = loops_ref(k, wire)
    plan = zero1_slices(count, k, wire)

    def body(comm):
        first, n = comm.zero1_init(count, Z.weights0(count), wire)
        a, b = plan[comm.rank]
        comm.write(Z.grads(k, count, 0)[comm.rank])
        barriers, launches = comm.barriers, comm.launches
        comm.zero1_accumulate()
        accs = [(comm._b.zero1_read_state(3, 0, b - a), comm.barriers - barriers, comm.launches - launches, comm.zero1_accumulated)]
        grid0 = comm._b.r.last_grid
        comm.write(Z.grads(k, count, 1)[comm.rank])
        barriers, launches = comm.barriers, comm.launches
        norm = comm.zero1_step(step=1, clip_norm=clip, accumulated=True, **HP)
        step = (comm.barriers - barriers, comm.launches - launches)
        got = (accs, comm._b.zero1_read_state(3, 0, b - a), comm.zero1_state(), comm.read(0, count, "bf16"), step, norm, comm.zero1_accumulated)
        return ((first, n), [got]), (grid0, comm.grid1, comm._b.r.last_grid)

    res = _ranks([0] * k, body, Z.capacity(count), comm_cls=functools.partial(Comm, max_ctas=L.GRID))
    assert all(grids == (L.GRID,) * 3 for _, grids in res), [grids for _, grids in res]  # the store, the adding launch and launch 2
    _assert_steps(lambda r: res[r][0], k, count, wire, "half", ref, "many tiles")


# -- 5. non-finite gradients ----------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["nan", "inf"])
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", [3, 8])
def test_a_nan_and_an_inf_stay_in_their_own_accumulator_element(k, wire, bad):
    """Micro-batch 0 of member 1 holds a -Inf and, in the "nan" case, a NaN as well, in two different blocks.  After
    each accumulate the stash is the reference's: exactly those elements are not finite, every other keeps its bits (on
    the fp8 wire an Inf travels as the format's NaN and its block's finite values are packed under e = 120, as the
    reference has it).  The accumulated clipped step then does what the clipped step documents: a NaN anywhere makes
    every value of every rank NaN; an Inf alone makes the norm Inf and the factor 0."""
    count = 8 * 1024 * k + 11
    at_inf, at_nan = 8 * 517 + 3, 8 * 901 + 6
    xs = [[x.copy() for x in Z.grads(k, count, j)] for j in range(M)]
    xs[0][1][at_inf] = 0xFF80
    if bad == "nan":
        xs[0][1][at_nan] = 0x7FC0
    hit = sorted([at_inf] + ([at_nan] if bad == "nan" else []))
    clip = C.clip_of(k, count, wire, "half")
    plan = zero1_slices(count, k, wire)
    acc, accs = None, []
    for j in range(M - 1):
        acc = zero1_accumulate_ref(acc, xs[j], "bf16", C.mean(k), wire)
        accs.append(acc)
    ref_state, ref_w, ref_norm = zero1_step_ref(xs[M - 1], Z.states0(k, count, wire), "bf16", C.mean(k), Z.hyper(1), wire, clip_norm=clip,
                                                accumulated=acc)
    for a in accs:  # the reference itself: the bad values reach their own elements alone
        assert sorted(np.flatnonzero(~np.isfinite(np.concatenate(a)[:count])).tolist()) == hit

    def body(comm):
        comm.zero1_init(count, Z.weights0(count), wire)
        a, b = plan[comm.rank]
        got = []
        for j in range(M - 1):
            comm.write(xs[j][comm.rank])
            comm.zero1_accumulate()
            got.append(comm._b.zero1_read_state(3, 0, b - a))
        comm.write(xs[M - 1][comm.rank])
        norm = comm.zero1_step(step=1, clip_norm=clip, accumulated=True, **HP)
        return got, norm, comm.zero1_state(), comm.read(0, count, "bf16")

    res = _ranks([0] * k, body, Z.capacity(count))
    all_nan = bad == "nan" or wire == "fp8"
    assert math.isnan(ref_norm) if all_nan else ref_norm == float("inf")
    for r in range(k):
        got, norm, state, out = res[r]
        what = f"k={k} {wire} {bad} rank {r}"
        for j in range(M - 1):
            assert mismatches(got[j], accs[j][r]).size == 0, (what, j)  # NaN where the reference is NaN, its bits elsewhere
            np.testing.assert_array_equal(np.isfinite(got[j]), np.isfinite(accs[j][r]), err_msg=what)
        assert math.isnan(norm) if all_nan else norm == float("inf"), what
        for name, (rtol, atol), a, b in zip(("master", "m", "v"), G.TOL, state, ref_state[r]):
            np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=f"{what} {name}: which values are NaN")
            fin = ~np.isnan(b)
            assert np.isfinite(b[fin]).all()
            np.testing.assert_allclose(a[fin], b[fin], rtol=rtol, atol=atol, err_msg=f"{what} {name}")
            if all_nan:
                assert np.isnan(a).all(), (what, name)
        np.testing.assert_array_equal(is_nan_bits(out), is_nan_bits(ref_w), err_msg=what)
        assert is_nan_bits(out).all() if all_nan else int(is_nan_bits(out).sum()) == 1, what
        np.testing.assert_array_equal(out, res[0][3], err_msg=what)


# -- 6. two distinct devices ----------------------------------------------------------------------------
@pytest.mark.skipif(G._ndev() < 2, reason="needs >= 2 visible GPUs (single-GPU box): no load or store of the step crosses a link")
def test_two_distinct_devices():
    count = 8 * 1024 * 2 + 11
    for wire in WIRES:
        clip = A.clip_of(2, count, wire, "half")
        ref = A.trajectory(2, count, wire, "half")
        res = _ranks([0, 1], lambda comm: A.accumulated_steps(comm, count, wire, clip), Z.capacity(count))
        _assert_steps(lambda r: res[r], 2, count, wire, "half", ref, "devices 0,1")
