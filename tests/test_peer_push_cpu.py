"""CPU tests of the K7 push all-reduce through the peer communicator's host backend: rank r sums slice r of
every window and stores the result into slice r of every rank's out, in one launch between the two barriers.
Bits against ops/peer_ref.py, barriers and launches per call, the race detector on peer writes of out (clean
on the protocol, non-empty on overlapping pushes and on a push beside an unordered gather), and the arguments."""
import threading

import numpy as np
import pytest

from gpu_topology_on_k8s_amd.ops.peer_ref import allreduce_q8_ref, allreduce_ref, peer_slices, reduce_scatter_ref
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

KS = (2, 3, 4, 8)


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


def _reference(case, xs):
    ref = allreduce_q8_ref if case.get("wire") == "fp8" else allreduce_ref
    return ref(xs, case["dtype"], case["out_dtype"], case["scale"])


# -- 1. the case list ---------------------------------------------------------------------------
def test_push_case_list_and_the_lists_that_stay():
    for k in KS:
        cases = pc.selftest_cases_push(k)
        native, fp8 = [c for c in cases if "wire" not in c], [c for c in cases if c.get("wire") == "fp8"]
        assert len(native) + len(fp8) == len(cases) == 5 * 3 + 7 * 2
        assert {(c["op"], c["algo"]) for c in cases} == {("all_reduce", "push")}
        assert [c["count"] for c in native[::3]] == pc.selftest_counts(k)
        assert [c["count"] for c in fp8[::2]] == pc.selftest_counts_q8(k)
        assert {(c["dtype"], c["out_dtype"], c["scale"]) for c in native} == {("bf16", "bf16", 1.0), ("fp32", "fp32", 1.0),
                                                                              ("bf16", "fp32", 1.0 / k)}
        assert {(c["dtype"], c["out_dtype"], c["scale"]) for c in fp8} == {("bf16", "bf16", 1.0), ("bf16", "fp32", 1.0 / k)}
        assert not any(c["algo"] == "push" for c in pc.selftest_cases(k) + pc.selftest_cases_q8(k) + pc.selftest_cases_q8x2(k))
    assert pc.ALGOS == ("oneshot", "twoshot") and pc.PUSH == "push"
    assert pc.selftest_cases_push(3, [5]) == [
        {"op": "all_reduce", "count": 5, "dtype": d, "out_dtype": o, "algo": "push", "scale": s}
        for d, o, s in (("bf16", "bf16", 1.0), ("fp32", "fp32", 1.0), ("bf16", "fp32", 1.0 / 3))] + [
        {"op": "all_reduce", "count": 5, "dtype": "bf16", "out_dtype": o, "algo": "push", "scale": s, "wire": "fp8"}
        for o, s in (("bf16", 1.0), ("fp32", 1.0 / 3))]


# -- 2. every case, twice, on the host backend ----------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_push_protocol_is_exact_with_two_barriers_one_launch_and_no_conflict(k):
    cases = pc.selftest_cases_push(k)
    once = pc._Once()  # the inputs and the reference of (case, issue), made by the first rank that asks

    def body(comm):
        bad = []
        for ci, case in enumerate(cases):
            for issue in range(2):
                xs = once.get(("in", ci, issue), lambda: [pc.case_input(ci, issue, p, case["count"], case["dtype"]) for p in range(k)],
                              lambda o: o[1] >= ci - 1)
                want = once.get(("ref", ci, issue), lambda: _reference(case, xs), lambda o: o[1] >= ci - 1)
                comm.write(xs[comm.rank])
                comm.barrier()  # a barrier on each side of a reading of the fabric's launch counter, which counts every rank's
                first = comm.launches
                comm.barrier()
                before = comm.barriers
                comm.all_reduce(case["count"], case["dtype"], "push", case["out_dtype"], case["scale"], wire=case.get("wire"))
                if comm.barriers - before != 2:
                    bad.append(("barriers", case, comm.barriers - before))
                got = comm.read(0, case["count"], case["out_dtype"])
                comm.barrier()
                if comm.launches - first != (2 * k if case.get("wire") == "fp8" else k):
                    bad.append(("launches", case, comm.launches - first))
                if not _same(got, want):
                    bad.append(("bits", case, issue))
        return bad

    fabric, results, errors = _run_threads(k, body, pc._case_capacity(k, cases))
    assert not errors, errors
    for r in range(k):
        assert results[r] == [], results[r][:3]
    assert fabric.conflicts() == []
    log = fabric.log
    assert any(a[2] == "out" and a[5] == "w" and a[0] != a[1] for a in log)   # peers do write a rank's out
    assert not any(a[2] == "out" and a[5] == "r" and a[0] != a[1] for a in log)  # and nobody reads a peer's
    for r in range(k):  # every rank wrote every owner's out
        assert {a[1] for a in log if a[0] == r and a[2] == "out" and a[5] == "w"} == set(range(k))


@pytest.mark.parametrize("k", KS)
def test_error_feedback_push_keeps_the_chained_reference(k):
    """wire="fp8" with error feedback: the quantize before barrier A is the one the other algorithms use, so the
    chained reference of the two-shot holds for the push, result and residual."""
    count = 512 * k + 37
    case = {"op": "all_reduce", "count": count, "dtype": "bf16", "out_dtype": "bf16", "algo": "push", "scale": 1.0, "wire": "fp8",
            "ef": True}

    def body(comm):
        residuals, bad = [], []
        for issue in range(3):
            xs = [pc.case_input(7, issue, p, count, "bf16") for p in range(k)]
            before = comm.barriers
            got, ref = pc.run_case(comm, case, xs, residuals)
            if comm.barriers - before != 2 or not _same(got, ref):
                bad.append(issue)
            if not np.array_equal(pc._bits(comm.residual(0, residuals[comm.rank].size)), pc._bits(residuals[comm.rank])):
                bad.append(("residual", issue))
        return bad

    fabric, results, errors = _run_threads(k, body, pc._case_capacity(k, [case]))
    assert not errors, errors
    assert all(results[r] == [] for r in range(k)), results
    assert fabric.conflicts() == []


# -- 3. mixed with the other collectives, slices of consecutive calls overlapping -----------------
def mixed_sequence(comm, counts, dtype="bf16"):
    """twoshot(A) -> push(B) -> twoshot(C) -> push(A) -> reduce_scatter -> push: the number of wrong results."""
    k, r = comm.world, comm.rank
    a, b, c = counts
    bad = 0
    steps = (("twoshot", a), ("push", b), ("twoshot", c), ("push", a), ("reduce_scatter", b), ("push", c))
    for i, (what, count) in enumerate(steps):
        xs = [pc.case_input(100 + i, 0, p, count, dtype) for p in range(k)]
        comm.write(xs[r])
        if what == "reduce_scatter":
            first, n = comm.reduce_scatter(count, dtype)
            bad += not _same(comm.read(first, n, dtype), reduce_scatter_ref(xs, dtype, dtype, 1.0)[r])
        else:
            comm.all_reduce(count, dtype, what)
            bad += not _same(comm.read(0, count, dtype), allreduce_ref(xs, dtype, dtype, 1.0))
    return bad


@pytest.mark.parametrize("k", KS)
def test_mixed_sequence_is_exact_and_free_of_conflicts(k):
    counts = (8 * 64 * k + 11, 8 * 24 * k - 5, 8 * 100 * k + 3)
    # the slices of consecutive calls do overlap: rank 1's slice of one count reaches into rank 0's of the next
    sl = [peer_slices(-(-c * 2 // 16), k) for c in counts]
    assert sl[1][1][0] < sl[0][0][1] and sl[0][1][0] < sl[2][0][1]
    fabric, results, errors = _run_threads(k, lambda comm: mixed_sequence(comm, counts), 16 * (-(-max(counts) * 2 // 16)))
    assert not errors, errors
    assert [results[r] for r in range(k)] == [0] * k
    assert fabric.conflicts() == []
    assert any(a[2] == "out" and a[5] == "w" and a[0] != a[1] for a in fabric.log)
    assert any(a[2] == "out" and a[5] == "r" and a[0] != a[1] for a in fabric.log)  # the two-shots' gathers


# -- 4. the race detector sees peer writes --------------------------------------------------------
def _two_backends(cap=4096):
    fabric = pc.HostFabric(2, cap)
    b0, b1 = pc._HostBackend(0, 2, fabric), pc._HostBackend(1, 2, fabric)
    for b in (b0, b1):
        b.write_host(pc.case_input(0, 0, b.rank, 256, "bf16"))
        b.epoch = 1  # past a barrier: the windows are written
    return fabric, b0, b1


def test_overlapping_pushes_in_one_epoch_are_a_conflict():
    fabric, b0, b1 = _two_backends()
    b0.reduce_push(0, 8, "bf16", "bf16", 1.0)
    b1.reduce_push(4, 12, "bf16", "bf16", 1.0)
    found = fabric.conflicts()
    assert found and all(w[2] == "out" and w[5] == "w" for w, _ in found)
    assert {w[1] for w, _ in found} == {0, 1}  # on both owners' out
    # the protocol's disjoint slices, and the same overlap a barrier apart, are none
    fabric, b0, b1 = _two_backends()
    b0.reduce_push(0, 8, "bf16", "bf16", 1.0)
    b1.reduce_push(8, 16, "bf16", "bf16", 1.0)
    assert fabric.conflicts() == []
    fabric, b0, b1 = _two_backends()
    b0.reduce_push(0, 8, "bf16", "bf16", 1.0)
    b1.epoch = 2
    b1.reduce_push(4, 12, "bf16", "bf16", 1.0)
    assert fabric.conflicts() == []


def test_a_push_beside_an_unordered_gather_of_the_same_out_is_a_conflict():
    """Rank 1 is still in phase 2 of a two-shot, reading slice 0 of rank 0's out and writing its own, when rank 0
    pushes: the barrier that orders them (the push's barrier A) left out."""
    for fp8 in (False, True):
        fabric, b0, b1 = _two_backends()
        if fp8:
            for b in (b0, b1):
                b.quantize(0, 8, 256, "bf16")
            b0.epoch = b1.epoch = 2
            b0.reduce_q8_push(0, 4, "bf16", 1.0)  # blocks [0, 4) are vectors [0, 16) of a bf16 out
        else:
            b0.reduce_push(0, 16, "bf16", "bf16", 1.0)
        b1.gather([(0, 16), (16, 32)])
        found = fabric.conflicts()
        assert found
        assert any(w[0] == 0 and w[1] == 0 and a[0] == 1 and a[5] == "r" for w, a in found)  # the peer's read of what rank 0 rewrites
        assert any(w[1] == 1 and {w[0], a[0]} == {0, 1} and a[5] == "w" for w, a in found)   # and both write rank 1's out
    fabric, b0, b1 = _two_backends()
    b1.gather([(0, 16), (16, 32)])
    b0.epoch = 2  # the barrier between them
    b0.reduce_push(0, 16, "bf16", "bf16", 1.0)
    assert fabric.conflicts() == []


class _NoBarrierB(pc.PeerComm):
    """A push that returns after its stream synchronise, without barrier B: a rank then reads an out its peers
    may still be writing."""

    def _leave(self):
        self._b.synchronize()


@pytest.mark.parametrize("k", (2, 3))
def test_a_push_without_barrier_b_is_a_conflict(k):
    def body(comm):
        comm.write(pc.case_input(0, 0, comm.rank, 2048, "bf16"))
        comm.all_reduce(2048, "bf16", "push")
        comm.read(0, 2048, "bf16")

    fabric, _, errors = _run_threads(k, body, 4096, comm_cls=_NoBarrierB)
    assert not errors, errors
    found = fabric.conflicts()
    assert found and any(w[0] != w[1] and a[0] == w[1] and a[5] == "r" for w, a in found)  # the owner's read, a peer's write
    fabric, _, errors = _run_threads(k, body, 4096)
    assert not errors and fabric.conflicts() == []


# -- 5. arguments ---------------------------------------------------------------------------------
def test_arguments_are_refused_before_any_barrier_or_launch():
    store, fabric = pc.MemoryStore(), pc.HostFabric(2, 4096)
    comm = pc.PeerComm(0, 2, 0, store, 4096, backend="host", fabric=fabric)
    with pytest.raises(ValueError, match="fp8x2"):
        comm.all_reduce(64, "bf16", "push", wire="fp8x2")
    with pytest.raises(ValueError, match="fp8x2"):
        comm.all_reduce(64, "bf16", "push", wire="fp8x2", error_feedback=True)
    with pytest.raises(ValueError, match="error_feedback"):
        comm.all_reduce(64, "bf16", "push", error_feedback=True)
    with pytest.raises(ValueError, match="error_feedback"):
        comm.all_reduce(64, "bf16", "push", wire="native", error_feedback=True)
    with pytest.raises(ValueError, match="push"):
        comm.all_reduce(64, "bf16", "ring")
    with pytest.raises(ValueError, match="push"):
        pc.thread_sweep([0, 0], [4096], "bf16", "ring")
    with pytest.raises(ValueError, match="fp8x2"):
        pc.thread_sweep([0, 0], [4096], "bf16", "push", wire="fp8x2")
    with pytest.raises(ValueError):
        comm.all_reduce(4096, "bf16", "push")  # past the window
    with pytest.raises(ValueError):
        comm._b.reduce_q8_push(0, 65, "bf16", 1.0)
    assert fabric.launches == 0 and comm.barriers == 0 and fabric.log == []


@pytest.mark.parametrize("k", (2, 3, 5))
def test_push_against_twoshot_is_a_mismatch_on_every_rank_before_any_launch(k):
    def body(comm):
        comm.write(pc.case_input(0, 0, comm.rank, 100, "bf16"))
        comm.all_reduce(100, "bf16", "push" if comm.rank == 0 else "twoshot")

    fabric, _, errors = _run_threads(k, body, 4096)
    assert sorted(errors) == list(range(k)) and all(isinstance(e, pc.PeerCommMismatch) for e in errors.values()), errors
    assert '"algo": "push"' in str(errors[k - 1]) and '"algo": "twoshot"' in str(errors[0])
    assert fabric.launches == 0
    assert not any(a[2] == "out" for a in fabric.log)


def test_front_end_names():
    from gpu_topology_on_k8s_amd.ops import probe

    assert probe.PEER_ALGOS == ("oneshot", "twoshot") and probe.PEER_PUSH == "push"
    with pytest.raises(ValueError, match="push"):
        probe.peer_sweep([0, 0], [4096], "bf16", "ring")
    with pytest.raises(ValueError, match="dtype"):
        probe.peer_sweep([0, 0], [4096], "fp16", "push")
    with pytest.raises(ValueError, match="dtype"):
        probe.peer_sweep([0, 0], [4096], "fp16", "all")


def test_validate_algo_option():
    import test_peer_q8_cpu as Q

    common = ("--devices", "0,0", "--resolve-only", "--cpu-bind", "off")
    for algo in ("push", "all"):
        assert Q._gtk("validate", "--backend", "peer", "--algo", algo, *common).returncode == 0
        assert Q._gtk("validate", "--backend", "peer", "--algo", algo, "--ranks", "thread", "--max-bytes", "1048576", *common).returncode == 0
        assert Q._gtk("validate", "--backend", "peer", "--algo", algo, "--wire", "fp8", *common).returncode == 0
    p = Q._gtk("validate", "--backend", "peer", "--algo", "push", "--wire", "fp8x2", *common)
    assert p.returncode == 2 and "fp8x2" in p.stderr
    assert Q._gtk("validate", "--backend", "peer", "--algo", "ring", *common).returncode == 2
