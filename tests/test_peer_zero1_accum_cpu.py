"""CPU tests of fp32 gradient accumulation in the ZeRO-1 step, through the peer communicator's host backend: every
micro-batch but the last goes through ``zero1_accumulate`` (barrier A, one launch that stores to or adds to the rank's
own stash, barrier B), the last one through ``zero1_step(accumulated=True)``, whose launch 1 adds once more, stores the
total back and squares it, and whose launch 2 is the clipped step's.  Bits against ops/peer_ref.zero1_accumulate_ref and
zero1_step_ref(accumulated=...), the race detector on the protocol, the descriptors, the refusals and the count.  Inputs
and helpers are those of tests/test_peer_zero1_cpu.py and tests/test_peer_zero1_clip_cpu.py; the GPU tests
(tests/test_gpu_peer_zero1_accum.py) take their references from here."""
import functools

import numpy as np
import pytest

import test_peer_zero1_clip_cpu as C
import test_peer_zero1_cpu as Z
from gpu_topology_on_k8s_amd.ops.peer_ref import (adamw_ref, allreduce_ref, clip_grad_scale, reduce_scatter_q8_ef_ref, reduce_scatter_q8_ref,
                                                   reduce_scatter_ref, zero1_accumulate_ref, zero1_slices, zero1_sqnorm_ref, zero1_step_ref)
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

KS = Z.KS
WIRES = Z.WIRES
HP = Z.HP
M = 3                              # micro-batches of an optimizer step: M - 1 accumulates, then the accumulated step
STEPS = 2
CLIPS = (None,) + tuple(C.CLIPS)   # unclipped; half the norm of one micro-batch's mean (every step clips); four times it


def micro(k, count, step, j):
    """Every rank's gradient of micro-batch j of optimizer step ``step`` (from 1): Z.grads, read-only."""
    return Z.grads(k, count, M * (step - 1) + j)


def clip_of(k, count, wire, which):
    return None if which is None else C.clip_of(k, count, wire, which)


def _copies(res):
    return None if res is None else [r.copy() for r in res]


@functools.lru_cache(maxsize=None)
def trajectory(k, count, wire, which=None, ef=False, steps=STEPS):
    """The reference's run of ``steps`` optimizer steps of M micro-batches from weights0.  Per step: the ranks'
    accumulators after each of the M - 1 accumulates, the total the step stores back, the residuals after each of the M
    calls (None without feedback), the states, the weights and the norm (None unclipped)."""
    st = Z.states0(k, count, wire)
    res = [np.zeros(32 * (-(-count // 32)), np.float32) for _ in range(k)] if ef else None
    clip, out = clip_of(k, count, wire, which), []
    for t in range(1, steps + 1):
        acc, accs, after = None, [], []
        for j in range(M - 1):
            acc = zero1_accumulate_ref(acc, list(micro(k, count, t, j)), "bf16", C.mean(k), wire, res)
            accs.append(acc)
            after.append(_copies(res))
        last = list(micro(k, count, t, M - 1))
        total = zero1_accumulate_ref(acc, last, "bf16", C.mean(k), wire, _copies(res))
        ret = zero1_step_ref(last, st, "bf16", C.mean(k), Z.hyper(t), wire, res, clip_norm=clip, accumulated=acc)
        st = ret[0]
        after.append(_copies(res))
        out.append((accs, total, after, st, ret[1], ret[2] if clip is not None else None))
    return out


def accumulated_steps(comm, count, wire, clip, ef=False, steps=STEPS):
    """zero1_init from weights0 and ``steps`` optimizer steps of M micro-batches.  Per step: after each accumulate the
    rank's stash, the barriers and launches the call took and the count; then the stash after the step, the state, out,
    the step's barriers and launches, the norm, and the count after it."""
    k = comm.world
    first, n = comm.zero1_init(count, Z.weights0(count), wire)
    a, b = zero1_slices(count, k, wire)[comm.rank]
    got = []
    for t in range(1, steps + 1):
        accs = []
        for j in range(M - 1):
            comm.write(micro(k, count, t, j)[comm.rank])
            barriers, launches = comm.barriers, comm.launches
            comm.zero1_accumulate(error_feedback=ef)
            accs.append((comm._b.zero1_read_state(3, 0, b - a), comm.barriers - barriers, comm.launches - launches, comm.zero1_accumulated))
        comm.write(micro(k, count, t, M - 1)[comm.rank])
        barriers, launches = comm.barriers, comm.launches
        norm = comm.zero1_step(step=t, error_feedback=ef, clip_norm=clip, accumulated=True, **HP)
        step = (comm.barriers - barriers, comm.launches - launches)
        got.append((accs, comm._b.zero1_read_state(3, 0, b - a), comm.zero1_state(), comm.read(0, count, "bf16"), step, norm,
                    comm.zero1_accumulated))
    return (first, n), got


# -- 1. the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_accumulate_ref_is_the_reduce_scatter_piece_by_piece_then_one_add(k, wire):
    f = np.float32
    for count in Z.counts(k):
        plan = zero1_slices(count, k, wire)
        rs = reduce_scatter_q8_ref if wire == "fp8" else reduce_scatter_ref
        pieces = [rs(list(Z.grads(k, count, j)), "bf16", "fp32", C.mean(k)) for j in range(3)]
        acc = None
        for j in range(3):
            new = zero1_accumulate_ref(acc, list(Z.grads(k, count, j)), "bf16", C.mean(k), wire)
            assert len(new) == k
            for r, (a, b) in enumerate(plan):
                p = pieces[j][r]
                assert new[r].dtype == np.float32 and new[r].shape == (b - a,)
                assert not new[r][p.size:].any()  # the padding is zero
                want = p if acc is None else (acc[r][:p.size] + p).astype(f)  # the first call stores, a later one adds once
                assert Z._same(new[r][:p.size], want), (k, wire, count, j, r)
                if acc is not None and p.size:
                    i = p.size // 2  # the same, one scalar float32 add
                    assert new[r][i] == f(f(acc[r][i]) + f(p[i]))
                    assert acc[r] is not new[r]  # new arrays: the caller's accumulators are left alone
            acc = new
    with pytest.raises(ValueError, match="bf16"):
        zero1_accumulate_ref(None, [x.astype(np.float32) for x in Z.grads(2, 8, 0)], "fp32", 1.0)
    with pytest.raises(ValueError, match="accumulator"):
        zero1_accumulate_ref([np.zeros(8, np.float32)], list(Z.grads(2, 8, 0)), "bf16", 1.0)
    with pytest.raises(ValueError, match="fp8"):
        zero1_accumulate_ref(None, list(Z.grads(2, 8, 0)), "bf16", 1.0, None, residuals=[np.zeros(32, np.float32)] * 2)


@pytest.mark.parametrize("wire", WIRES)
def test_these_inputs_tell_a_fused_multiply_add_from_two_roundings(wire):
    """The kernels must round the product by ``scale`` before the add, as the reference does.  Here the sum is added
    with the exact product instead (float64 holds it), as a fused multiply-add would: on these inputs that changes bits,
    so an accumulator with the reference's bits was not computed that way.  k = 3: 1 / k is no power of two."""
    k = 3
    count = Z.counts(k)[-1]
    xs = [list(Z.grads(k, count, j)) for j in range(2)]
    first = zero1_accumulate_ref(None, xs[0], "bf16", C.mean(k), wire)
    want = zero1_accumulate_ref(first, xs[1], "bf16", C.mean(k), wire)
    unscaled = zero1_accumulate_ref(None, xs[1], "bf16", 1.0, wire)
    differ = 0
    for a, b, w in zip(first, unscaled, want):
        fused = (a.astype(np.float64) + b.astype(np.float64) * np.float64(np.float32(C.mean(k)))).astype(np.float32)
        differ += int((pc._bits(fused) != pc._bits(w)).sum())
    assert differ > count // 100, differ


def test_accumulate_ref_with_feedback_is_the_feedback_reduce_scatter_and_chains_the_residuals():
    k, count = 3, 512 * 3 + 37
    n = 32 * (-(-count // 32))
    res = [np.zeros(n, np.float32) for _ in range(k)]
    mine = [r.copy() for r in res]
    acc = None
    for j in range(3):
        pieces, after = reduce_scatter_q8_ef_ref(list(Z.grads(k, count, j)), mine, "bf16", "fp32", C.mean(k))
        new = zero1_accumulate_ref(acc, list(Z.grads(k, count, j)), "bf16", C.mean(k), "fp8", res)
        for r in range(k):
            p = pieces[r]
            assert Z._same(new[r][:p.size], p if acc is None else (acc[r][:p.size] + p).astype(np.float32))
            assert Z._same(res[r], after[r])
        acc, mine = new, after
    assert any(r.any() for r in res)


def test_step_ref_accumulated_adds_once_before_the_norm_and_the_update():
    k, count = 3, 8 * 100 * 3 + 5
    for wire in WIRES:
        xs = [list(Z.grads(k, count, j)) for j in range(3)]
        acc = zero1_accumulate_ref(zero1_accumulate_ref(None, xs[0], "bf16", C.mean(k), wire), xs[1], "bf16", C.mean(k), wire)
        total = zero1_accumulate_ref(acc, xs[2], "bf16", C.mean(k), wire)
        st = Z.states0(k, count, wire)
        new, w, norm = zero1_step_ref(xs[2], st, "bf16", C.mean(k), Z.hyper(1), wire, clip_norm=1.0, accumulated=acc)
        # the same from its parts: the norm of the total, and AdamW with the total as every rank's gradient
        want_norm, gs = clip_grad_scale(zero1_sqnorm_ref(total), 1.0, 1.0)
        assert norm == want_norm
        h = Z.hyper(1)
        h = h[:5] + [float(np.float32(gs))] + h[6:]
        for r in range(k):
            want = adamw_ref(*st[r], total[r], h)
            assert all(Z._same(x, y) for x, y in zip(new[r], want[:3]))
        plain = zero1_step_ref(xs[2], st, "bf16", C.mean(k), Z.hyper(1), wire, clip_norm=1.0)
        assert not Z._same(plain[1], w)  # the accumulator does take part


# -- 2. two optimizer steps of M micro-batches, bit for bit ----------------------------------------------
@pytest.mark.parametrize("which", CLIPS)
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_two_accumulated_steps_equal_the_reference_bit_for_bit(k, wire, which):
    for count in Z.counts(k):
        clip = clip_of(k, count, wire, which)
        fabric, results, errors = Z._run_threads(k, lambda comm: accumulated_steps(comm, count, wire, clip), Z.capacity(count))
        assert not errors, errors
        ref = trajectory(k, count, wire, which)
        plan = zero1_slices(count, k, wire)
        busy = [r for r in range(k) if plan[r][1] > plan[r][0]]
        for r in range(k):
            _, got = results[r]
            for t, (accs, stash, state, out, (barriers, _), norm, left) in enumerate(got):
                what = (k, count, wire, which, r, t)
                for j, (acc, b, _, n_acc) in enumerate(accs):
                    assert b == 2 and n_acc == j + 1, what
                    assert Z._same(acc, ref[t][0][j][r]), what + (j,)
                assert Z._same(stash, ref[t][1][r]), what  # launch 1 of the step stores the total back
                assert barriers == (2 if which is None else 3) and left == 0, what  # the step ends the accumulation
                assert len(state) == 3 and all(Z._same(a, b) for a, b in zip(state, ref[t][3][r])), what
                assert Z._same(out, ref[t][4]), what
                assert norm is None if which is None else (isinstance(norm, float) and norm == ref[t][5]), what
        if which != "loose":
            assert ref[0][5] is None or ref[0][5] > clip  # "half" does clip the accumulated total
        # the race detector: the accumulates and launch 1 read the peers and write the rank's own stash, launch 2 every out
        assert fabric.conflicts() == []
        log = fabric.log
        assert all(a[0] == a[1] for a in log if a[2] in ("zero1", "residual"))
        assert not any(a[2] == "out" and a[5] == "r" and a[0] != a[1] for a in log)
        src = "packed" if wire == "fp8" else "window"
        for r in busy:
            assert {a[1] for a in log if a[0] == r and a[2] == src and a[5] == "r"} == set(range(k))
            assert {a[1] for a in log if a[0] == r and a[2] == "out" and a[5] == "w"} == set(range(k))
            lo = 3 * (plan[r][1] - plan[r][0]) * 4 // 16  # the stash is row 3 of the rank's state
            assert any(a[0] == r and a[2] == "zero1" and a[5] == "r" and a[3] >= lo for a in log)  # the adding launch reads it
            assert any(a[0] == r and a[2] == "zero1" and a[5] == "w" and a[3] >= lo for a in log)  # and writes it back
        for r in set(range(k)) - set(busy):  # an empty slice: no launch, nothing written, every barrier taken all the same
            assert not any(a[0] == r and a[2] == "out" and a[5] == "w" for a in log)
        # per optimizer step M - 1 accumulates of one launch and a step of two, per rank with a slice; on the fp8 wire
        # every rank's quantize in each of the M calls
        assert fabric.launches == STEPS * ((M + 1) * len(busy) + (M * k if wire == "fp8" else 0))


@pytest.mark.parametrize("which", (None, "half"))
@pytest.mark.parametrize("k", (2, 3))
def test_error_feedback_chains_through_accumulates_and_steps(k, which):
    count = 512 * k + 37
    n = 32 * (-(-count // 32))
    clip = clip_of(k, count, "fp8", which)

    def body(comm):
        comm.zero1_init(count, Z.weights0(count), "fp8")
        a, b = zero1_slices(count, k, "fp8")[comm.rank]
        got = []
        for t in range(1, STEPS + 1):
            for j in range(M):
                comm.write(micro(k, count, t, j)[comm.rank])
                if j < M - 1:
                    comm.zero1_accumulate(error_feedback=True)
                    got.append((comm._b.zero1_read_state(3, 0, b - a), comm.residual(0, n)))
                else:
                    norm = comm.zero1_step(step=t, error_feedback=True, clip_norm=clip, accumulated=True, **HP)
                    got.append((comm.zero1_state(), comm.read(0, count, "bf16"), norm, comm.residual(0, n)))
        return got

    fabric, results, errors = Z._run_threads(k, body, Z.capacity(count))
    assert not errors, errors
    ref = trajectory(k, count, "fp8", which, True)
    for r in range(k):
        calls = iter(results[r])
        for t in range(STEPS):
            for j in range(M - 1):
                acc, residual = next(calls)
                assert Z._same(acc, ref[t][0][j][r]) and Z._same(residual, ref[t][2][j][r]), (k, which, r, t, j)
            state, out, norm, residual = next(calls)
            assert all(Z._same(a, b) for a, b in zip(state, ref[t][3][r])) and Z._same(out, ref[t][4]), (k, which, r, t)
            assert norm == ref[t][5] and Z._same(residual, ref[t][2][M - 1][r]), (k, which, r, t)
    assert not Z._same(ref[-1][4], trajectory(k, count, "fp8", which)[-1][4])  # feedback does change the trajectory
    assert fabric.conflicts() == []


# -- 3. among the other collectives -------------------------------------------------------------------
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", (2, 3, 8))
def test_interleaved_with_the_other_collectives_there_is_no_conflict(k, wire):
    count = 8 * 64 * k + 11
    other = 8 * 24 * k - 5  # its slices overlap the step's
    g = [list(Z.grads(k, count, j)) for j in range(4)]
    acc = zero1_accumulate_ref(zero1_accumulate_ref(None, g[0], "bf16", C.mean(k), wire), g[1], "bf16", C.mean(k), wire)
    st1, w1 = zero1_step_ref(g[2], Z.states0(k, count, wire), "bf16", C.mean(k), Z.hyper(1), wire, accumulated=acc)
    st2, w2 = zero1_step_ref(g[3], st1, "bf16", C.mean(k), Z.hyper(2), wire)  # a plain step after the accumulated one

    def body(comm):
        r, bad = comm.rank, 0
        comm.zero1_init(count, Z.weights0(count), wire)
        xs = [pc.case_input(70, 0, p, other, "bf16") for p in range(k)]
        comm.write(xs[r])
        comm.all_reduce(other, "bf16", "twoshot")
        bad += not Z._same(comm.read(0, other, "bf16"), allreduce_ref(xs, "bf16"))
        comm.write(g[0][r])
        comm.zero1_accumulate()
        comm.write(xs[r])
        first, n = comm.reduce_scatter(other, "bf16", "fp32", 0.5)  # it writes this rank's out, not its stash
        bad += not Z._same(comm.read(first, n, "fp32"), reduce_scatter_ref(xs, "bf16", "fp32", 0.5)[r])
        comm.write(g[1][r])
        comm.zero1_accumulate()
        comm.write(xs[r])
        comm.all_reduce(other, "bf16", "push")
        bad += not Z._same(comm.read(0, other, "bf16"), allreduce_ref(xs, "bf16"))
        comm.write(g[2][r])
        comm.zero1_step(step=1, accumulated=True, **HP)
        bad += not Z._same(comm.read(0, count, "bf16"), w1)
        comm.write(g[3][r])
        comm.zero1_step(step=2, **HP)
        bad += not Z._same(comm.read(0, count, "bf16"), w2)
        bad += not all(Z._same(a, b) for a, b in zip(comm.zero1_state(), st2[r]))
        return bad

    fabric, results, errors = Z._run_threads(k, body, Z.capacity(count))
    assert not errors, errors
    assert [results[r] for r in range(k)] == [0] * k
    assert fabric.conflicts() == []


class _WritesItsWindowEarly(pc.PeerComm):
    """A rank that refills its window with the next micro-batch between barriers A and B of an accumulate (test-only):
    on the native wire its peers are reading that window then."""

    def _enter(self, desc):
        super()._enter(desc)
        if desc["op"] == "zero1_accumulate":
            self._b.write_host(np.zeros(desc["count"], np.uint16))


@pytest.mark.parametrize("k", (2, 3))
def test_a_window_written_between_the_barriers_of_an_accumulate_is_reported(k):
    count = 8 * 64 * k

    def body(comm, wire):
        comm.zero1_init(count, Z.weights0(count), wire)
        for j in range(2):
            comm.write(Z.grads(k, count, j)[comm.rank])
            comm.zero1_accumulate()

    fabric, _, errors = Z._run_threads(k, lambda comm: body(comm, "native"), Z.capacity(count), comm_cls=_WritesItsWindowEarly)
    assert not errors, errors
    found = fabric.conflicts()
    assert found
    assert any(w[2] == "window" and w[0] == w[1] and w[5] == "w" and a[5] == "r" and a[0] != w[0] for w, a in found)  # the owner's write, a peer's read
    fabric, _, errors = Z._run_threads(k, lambda comm: body(comm, "native"), Z.capacity(count))
    assert not errors and fabric.conflicts() == []
    # on the fp8 wire the peers read the packed buffer, and the window is its owner's again once the quantize is done
    fabric, _, errors = Z._run_threads(k, lambda comm: body(comm, "fp8"), Z.capacity(count), comm_cls=_WritesItsWindowEarly)
    assert not errors and fabric.conflicts() == []


# -- 4. the descriptors -------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ("scale", "count", "accumulated"))
@pytest.mark.parametrize("k", (2, 3))
def test_ranks_that_disagree_get_a_mismatch_before_any_launch(k, what):
    count = 8 * 64 * k
    seen = {}

    def body(comm):
        odd = comm.rank == 1
        comm.zero1_init(count, Z.weights0(count))
        comm.write(Z.grads(k, count, 0)[comm.rank])
        if what == "scale":
            seen[comm.rank] = comm.launches
            comm.zero1_accumulate(scale=0.5 if odd else 0.25)
            return
        comm.zero1_accumulate()
        comm.barrier()  # every rank's first accumulate is counted before any rank looks
        seen[comm.rank] = comm.launches
        if odd:
            comm.zero1_reset_accumulated()  # local: this rank's count is 0, the others' 1
        if what == "count":
            comm.zero1_accumulate()
        else:
            comm.zero1_step(step=1, accumulated=not odd, **HP)

    fabric, _, errors = Z._run_threads(k, body, Z.capacity(count))
    assert sorted(errors) == list(range(k)) and all(isinstance(e, pc.PeerCommMismatch) for e in errors.values()), errors
    assert '"accumulated"' in str(errors[0]) and ('"op": "zero1_step"' if what == "accumulated" else '"op": "zero1_accumulate"') in str(errors[0])
    assert fabric.launches == seen[0] == (0 if what == "scale" else k)  # nothing was launched after the descriptors met
    assert not any(a[2] == "out" and a[5] == "w" for a in fabric.log)


# -- 5. the refusals, the count and the bytes ---------------------------------------------------------
def test_refusals_come_before_any_barrier_or_launch():
    store, fabric = pc.MemoryStore(), pc.HostFabric(2, 4096)
    comm = pc.PeerComm(0, 2, 0, store, 4096, backend="host", fabric=fabric)
    with pytest.raises(ValueError, match="zero1_init"):
        comm.zero1_accumulate()
    with pytest.raises(ValueError, match="zero1_init"):
        comm.zero1_step(step=1, accumulated=True, **HP)
    assert comm.zero1_accumulated == 0
    assert comm.zero1_init(256, Z.weights0(256)) == (0, 128)
    with pytest.raises(ValueError, match="error_feedback"):
        comm.zero1_accumulate(error_feedback=True)
    with pytest.raises(ValueError, match="error_feedback"):
        comm.zero1_step(step=1, accumulated=True, error_feedback=True, **HP)
    with pytest.raises(ValueError, match="nothing is accumulated"):
        comm.zero1_step(step=1, accumulated=True, **HP)
    with pytest.raises(ValueError, match="nothing is accumulated"):
        comm.zero1_step(step=1, accumulated=True, clip_norm=1.0, **HP)
    assert comm.barriers == 0 and fabric.launches == 0 and comm.zero1_accumulated == 0
    assert comm._b.zero1_bytes == 3 * 128 * 4  # and no stash was made
    comm._b.zero1_stash_alloc()
    for bad in (lambda: comm._b.reduce_sqnorm_accum(0, 17, 1.0), lambda: comm._b.reduce_q8_sqnorm_accum(0, 5, 1.0)):
        with pytest.raises(ValueError):
            bad()  # more than the stash holds
    assert comm._b.reduce_sqnorm_accum(5, 5, 1.0) == 0.0 and comm._b.reduce_q8_sqnorm_accum(2, 2, 1.0) == 0.0 and fabric.launches == 0


@pytest.mark.parametrize("wire", WIRES)
def test_the_count_the_refused_plain_step_and_the_stash_bytes(wire):
    k, count = 3, 8 * 100 * 3 + 5
    plan = zero1_slices(count, k, wire)
    ref0 = zero1_accumulate_ref(None, list(Z.grads(k, count, 0)), "bf16", C.mean(k), wire)
    ref2 = zero1_accumulate_ref(None, list(Z.grads(k, count, 2)), "bf16", C.mean(k), wire)
    ref23 = zero1_accumulate_ref(ref2, list(Z.grads(k, count, 3)), "bf16", C.mean(k), wire)

    def body(comm):
        n = plan[comm.rank][1] - plan[comm.rank][0]
        comm.zero1_init(count, Z.weights0(count), wire)
        seen, counts, stashes = [comm._b.zero1_bytes], [comm.zero1_accumulated], []
        for j in (0, 1):
            comm.write(Z.grads(k, count, j)[comm.rank])
            comm.zero1_accumulate()
            seen.append(comm._b.zero1_bytes)
            counts.append(comm.zero1_accumulated)
            if j == 0:
                stashes.append(comm._b.zero1_read_state(3, 0, n))
        barriers, launches = comm.barriers, comm.launches
        with pytest.raises(ValueError, match="would drop"):
            comm.zero1_step(step=1, **HP)  # accumulated=False while two micro-batches are accumulated
        with pytest.raises(ValueError, match="would drop"):
            comm.zero1_step(step=1, clip_norm=1.0, **HP)
        assert (comm.barriers, comm.zero1_accumulated) == (barriers, 2)
        refused = comm.launches - launches
        comm.zero1_reset_accumulated()  # a skipped step: local, no barrier
        assert comm.barriers == barriers
        counts.append(comm.zero1_accumulated)
        for j in (2, 3):  # the first accumulate after a reset stores again
            comm.write(Z.grads(k, count, j)[comm.rank])
            comm.zero1_accumulate()
            counts.append(comm.zero1_accumulated)
            stashes.append(comm._b.zero1_read_state(3, 0, n))
        comm.zero1_init(count, Z.weights0(count), wire)
        counts.append(comm.zero1_accumulated)
        seen.append(comm._b.zero1_bytes)
        return n, seen, counts, stashes, refused

    fabric, results, errors = Z._run_threads(k, body, Z.capacity(count))
    assert not errors, errors
    for r in range(k):
        n, seen, counts, stashes, refused = results[r]
        assert seen == [12 * n, 16 * n, 16 * n, 12 * n]  # the stash is counted from the first accumulate on; a new init frees it
        assert counts == [0, 1, 2, 0, 1, 2, 0] and refused == 0
        assert Z._same(stashes[0], ref0[r]) and Z._same(stashes[1], ref2[r]) and Z._same(stashes[2], ref23[r])
    assert fabric.conflicts() == []
