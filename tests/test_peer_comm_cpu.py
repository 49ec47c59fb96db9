"""CPU tests of the peer communicator (parallel/peer_comm.py): the references of the scaled and wide
reduce, the two-barrier protocol on the host backend with threads as ranks and its race detector,
timeouts, store failures, mismatched calls, the keys it leaves in the store, and the register budget
of the new reduce instantiations."""
import os
import random
import sys
import threading
import time

import numpy as np
import pytest

from gpu_topology_on_k8s_amd.ops.peer_ref import allreduce_ref, bf16_round, bf16_to_f32, peer_slices, reduce_scatter_ref
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


def _inputs(k, count, dtype, seed=0):
    rng = np.random.default_rng([seed, k, count])
    xs = [rng.standard_normal(count).astype(np.float32) for _ in range(k)]
    return [bf16_round(x) for x in xs] if dtype == "bf16" else xs


# -- 1. references ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_reference_defaults_are_the_old_reference(dtype):
    xs = _inputs(5, 1003, dtype)
    acc = (bf16_to_f32(xs[0]) if dtype == "bf16" else xs[0]).copy()
    for x in xs[1:]:
        acc = (acc + (bf16_to_f32(x) if dtype == "bf16" else x)).astype(np.float32)
    old = bf16_round(acc) if dtype == "bf16" else acc
    np.testing.assert_array_equal(allreduce_ref(xs, dtype), old)
    np.testing.assert_array_equal(allreduce_ref(xs, dtype, None, 1.0), allreduce_ref(xs, dtype))
    np.testing.assert_array_equal(allreduce_ref(xs, dtype, dtype, 1.0), allreduce_ref(xs, dtype))


def order_case():
    """fp32, k = 3, scale = 1/3 on a fixed seed: the case in which the order of sum and scale shows."""
    rng = np.random.default_rng(20240607)
    return [rng.standard_normal(4096).astype(np.float32) for _ in range(3)]


def test_sum_then_scale_differs_from_scale_then_sum():
    xs = order_case()
    s = np.float32(1.0 / 3.0)
    ref = allreduce_ref(xs, "fp32", None, 1.0 / 3.0)
    np.testing.assert_array_equal(ref, ((xs[0] + xs[1]) + xs[2]) * s)
    other = allreduce_ref([(x * s).astype(np.float32) for x in xs], "fp32")
    assert np.count_nonzero(ref.view(np.uint32) != other.view(np.uint32)) >= 1


def test_wide_output_keeps_what_bf16_rounds_away():
    xs = _inputs(3, 4099, "bf16")
    wide = allreduce_ref(xs, "bf16", "fp32")
    narrow = allreduce_ref(xs, "bf16")
    assert wide.dtype == np.float32 and narrow.dtype == np.uint16
    np.testing.assert_array_equal(bf16_round(wide), narrow)
    assert np.count_nonzero(wide.view(np.uint32) & np.uint32(0xFFFF)) >= 1  # bits below bf16's mantissa
    assert np.count_nonzero(bf16_to_f32(narrow) != wide) >= 1
    with pytest.raises(ValueError):
        allreduce_ref([x.astype(np.float32) for x in xs], "fp32", "bf16")


@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("pair", [("bf16", None), ("fp32", None), ("bf16", "fp32")])
def test_reduce_scatter_pieces_concatenate_to_the_allreduce(pair, k):
    dtype, out = pair
    for count in (1, 7, 8 * (k - 1), 8 * 64 * k + 11):
        xs = _inputs(k, count, dtype)
        pieces = reduce_scatter_ref(xs, dtype, out, 1.0 / k)
        assert len(pieces) == k
        np.testing.assert_array_equal(np.concatenate(pieces), allreduce_ref(xs, dtype, out, 1.0 / k))
        per = 8 if dtype == "bf16" else 4
        assert [len(p) for p in pieces] == [min(count, b * per) - min(count, a * per) for a, b in peer_slices(-(-count // per), k)]


# -- 2-6. the protocol on the host backend ----------------------------------------------------
CAP = 1 << 17


def _counts(k):
    return [1, 7, 8 * (k - 1), 8 * 64 * k + 11]


def _run_threads(k, body, timeout_s=20.0, skip_second_barrier=False, ranks=None):
    """One thread per rank in ``ranks`` (all by default) runs ``body(comm)``; returns (fabric, store, results, errors)."""
    store, fabric = pc.MemoryStore(timeout_s=timeout_s), pc.HostFabric(k, CAP)
    results, errors = {}, {}

    def run(r):
        rnd = random.Random(r)
        try:
            comm = pc.PeerComm(r, k, 0, store, CAP, timeout_s=timeout_s, backend="host", fabric=fabric)
            real, calls = comm._barrier, [0]

            def barrier():
                time.sleep(rnd.random() * 0.002)  # ranks arrive in a different order every time
                calls[0] += 1
                if skip_second_barrier and calls[0] % 2 == 0:
                    return
                real()

            comm._barrier = barrier
            results[r] = body(comm)
        except BaseException as e:  # handed to the test's thread
            errors[r] = e

    threads = [threading.Thread(target=run, args=(r,)) for r in (range(k) if ranks is None else ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads)
    return fabric, store, results, errors


def _sequence(comm):
    """Every op, both algorithms, every dtype pair, each issued twice in a row with different inputs."""
    bad, n = [], 0
    for ci, case in enumerate(pc.selftest_cases(comm.world, _counts(comm.world))):
        for issue in range(2):
            xs = [pc.case_input(ci, issue, p, case["count"], case["dtype"]) for p in range(comm.world)]
            before = comm.barriers
            got, ref = pc.run_case(comm, case, xs)
            n += 1
            if comm.barriers - before != 2:
                bad.append(("barriers", case, comm.barriers - before))
            if got.dtype != ref.dtype or got.shape != ref.shape or not np.array_equal(pc._bits(got), pc._bits(ref)):
                bad.append(("bits", case, issue))
    return n, bad


@pytest.mark.parametrize("k", [2, 3, 5])
def test_protocol_is_exact_with_two_barriers_and_no_conflict(k):
    cases = pc.selftest_cases(k, _counts(k))
    assert {c["op"] for c in cases} == {"all_reduce", "reduce_scatter", "all_gather"}
    assert {(c["dtype"], c["out_dtype"]) for c in cases} == {("bf16", "bf16"), ("fp32", "fp32"), ("bf16", "fp32")}
    assert {c["algo"] for c in cases if c["op"] == "all_reduce"} == {"oneshot", "twoshot"}
    fabric, _, results, errors = _run_threads(k, _sequence)
    assert not errors, errors
    for r in range(k):
        n, bad = results[r]
        assert n == 2 * len(cases) and not bad, (r, bad[:3])
    assert fabric.log and {a[5] for a in fabric.log} == {"r", "w"}
    assert fabric.conflicts() == []


@pytest.mark.parametrize("k", [2, 3, 5])
def test_the_detector_reports_a_skipped_barrier(k):
    fabric, _, _, errors = _run_threads(k, _sequence, skip_second_barrier=True)
    assert not errors, errors
    assert len(fabric.conflicts()) >= 1


def test_dead_rank_times_out_and_breaks_the_comm():
    k, took = 3, {}

    def body(comm):
        comm.write(np.ones(64, np.float32))
        t0 = time.monotonic()
        with pytest.raises(pc.PeerCommTimeout):
            comm.all_reduce(64, "fp32", "oneshot")
        took[comm.rank] = time.monotonic() - t0
        assert comm.broken
        t0 = time.monotonic()
        with pytest.raises(pc.PeerCommTimeout):
            comm.all_reduce(64, "fp32", "oneshot")
        assert time.monotonic() - t0 < 0.5  # at once: no barrier is tried
        t0 = time.monotonic()
        comm.close()
        assert time.monotonic() - t0 < 0.5  # and close() skips its barriers
        return True

    fabric, _, results, errors = _run_threads(k, body, timeout_s=2.0, ranks=[0, 2])  # rank 1 never calls
    assert not errors, errors
    assert results == {0: True, 2: True}
    assert all(1.5 < t < 4.0 for t in took.values()), took
    assert fabric.launches == 0


def test_mismatched_calls_raise_on_every_rank_before_any_launch():
    k = 3

    def body(comm):
        comm.write(np.ones(64, np.float32))
        with pytest.raises(pc.PeerCommMismatch):
            comm.all_reduce(64 if comm.rank != 1 else 60, "fp32", "twoshot")
        return comm.barriers

    fabric, _, results, errors = _run_threads(k, body)
    assert not errors, errors
    assert results == {0: 1, 1: 1, 2: 1}
    assert fabric.launches == 0


def test_over_capacity_raises_before_any_barrier():
    store, fabric = pc.MemoryStore(), pc.HostFabric(2, 256)
    comm = pc.PeerComm(0, 2, 0, store, 256, backend="host", fabric=fabric)
    before = dict(store.ops)
    for call in (lambda: comm.all_reduce(129, "bf16", "oneshot"), lambda: comm.all_reduce(65, "fp32", "twoshot"),
                 lambda: comm.reduce_scatter(129, "bf16"), lambda: comm.all_gather(65, "bf16"),
                 lambda: comm.all_reduce(8, "fp32", "oneshot", "bf16"), lambda: comm.all_reduce(8, "fp16", "oneshot"),
                 lambda: comm.all_reduce(8, "bf16", "ring"), lambda: comm.write(np.zeros(65, np.float32))):
        with pytest.raises(ValueError):
            call()
    assert store.ops == before and comm.barriers == 0 and fabric.launches == 0 and fabric.log == []


def test_store_keys_do_not_grow_with_the_number_of_collectives():
    """Barrier and descriptor keys are deleted two barriers later: the store holds a bounded number
    of keys however many collectives ran (each leaves 2 barrier counters, 2 flags and k descriptors)."""
    k, seen = 3, {}

    def body(comm):
        for i in range(40):
            comm.write(np.full(64, comm.rank + i, np.float32))
            comm.all_reduce(64, "fp32", "twoshot" if i % 2 else "oneshot")
            if comm.rank == 0 and i in (9, 39):
                seen[i] = comm._store.num_keys()
            np.testing.assert_array_equal(comm.read(0, 64, "fp32"), np.full(64, 3 * i + 3, np.float32))
        comm.close()
        return comm.barriers

    fabric, store, results, errors = _run_threads(k, body)
    assert not errors, errors
    assert results == {0: 82, 1: 82, 2: 82}
    assert seen[9] <= 4 * (2 + k) and seen[39] <= 4 * (2 + k), seen  # what four barriers may still need
    assert store.num_keys() <= 4 * (2 + k) and store.ops["delete_key"] > 40 * (4 + k) - 4 * (2 + k)
    assert fabric.conflicts() == []


class _FailingStore(pc.MemoryStore):
    """Fails the n-th ``set`` or ``get`` from now on, as a store whose server went away does."""

    fail = None

    def set(self, key, value):
        if self.fail == "set" and "/desc/" in key:
            raise ConnectionError("store is gone")
        super().set(key, value)

    def get(self, key):
        if self.fail == "get":
            raise ConnectionError("store is gone")
        return super().get(key)


@pytest.mark.parametrize("op", ["set", "get"])
def test_a_store_error_in_the_descriptor_exchange_breaks_the_comm(op):
    k = 2
    store, fabric = _FailingStore(timeout_s=2.0), pc.HostFabric(k, CAP)
    comms = [pc.PeerComm(r, k, 0, store, CAP, timeout_s=2.0, backend="host", fabric=fabric) for r in range(k)]
    store.fail = op
    out = {}

    def run(c):
        try:
            c.all_reduce(8, "fp32", "oneshot")
        except BaseException as e:
            out[c.rank] = e

    threads = [threading.Thread(target=run, args=(c,)) for c in comms]
    for t in threads:
        t.start()
    for t in threads:
        t.join(30)
    for c in comms:
        assert isinstance(out[c.rank], pc.PeerCommTimeout) and "store is gone" in str(out[c.rank]), out
        assert c.broken and fabric.launches == 0
        with pytest.raises(pc.PeerCommTimeout):
            c.all_reduce(8, "fp32", "oneshot")
        c.close()


def test_only_the_host_backend_exists():
    with pytest.raises(ValueError, match="host"):
        pc.PeerComm(0, 2, 0, pc.MemoryStore(), 256, backend="native")


# -- 7. register budget -----------------------------------------------------------------------
def test_every_reduce_instantiation_uses_no_scratch(tmp_path):
    """Register budget only: the reduce kernel in its three type pairs, four member buckets each."""
    import isa

    st = isa.kernel_stats(os.path.join(REPO, "csrc", "probe", "probe.hip"), target="_probe", out=str(tmp_path / "probe.s"))
    reduce_k = {k: v for k, v in st.items() if "peer_reduce_kernel" in k}
    assert len(reduce_k) == 12, sorted(reduce_k)  # (bf16, bf16), (fp32, fp32), (bf16, fp32) x buckets 2 / 4 / 8 / 16
    for name, v in reduce_k.items():
        assert v["ScratchSize"] == 0 and v["scratch"] == 0, (name, v)
