"""GPU tests of the peer communicator's device backend (parallel/peer_comm.py, ``backend="device"``, over
``_probe.PeerRank`` of csrc/probe/peer_rank.h): ranks are threads of this process, each with its own
stream and device buffers, and the K7 kernels are ordered by the host protocol alone.

Every rank is device 0 unless a test says otherwise, so a one-GPU box runs every member bucket.  Inputs
and references are made once in the test's thread (ops/peer_ref.py) and are read-only; the rank threads
only issue and compare, bit for bit."""
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from gpu_topology_on_k8s_amd.ops.peer_ref import (Q8_BLOCK, allreduce_ref, bf16_round, launch_u, launch_walk, peer_slices, q8_blocks,
                                                   q8_dequantize_ref, q8_quantize_ef_ref, q8_quantize_ref, q8_slices, reduce_scatter_ref)
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts(k):
    # one element; under one vector; k - 1 bf16 vectors (the last two-shot slice is empty); k whole
    # 256 x U tiles, a tail and padding
    return [1, 7, 8 * (k - 1), 8 * 1024 * k + 11]


@functools.lru_cache(maxsize=None)
def _inputs(k, count, dtype, issue):
    rng = np.random.default_rng([k, count, issue, 0 if dtype == "bf16" else 1])
    xs = [rng.standard_normal(count, dtype=np.float32) for _ in range(k)]
    xs = tuple(bf16_round(x) if dtype == "bf16" else x for x in xs)
    for x in xs:
        x.setflags(write=False)
    return xs


@functools.lru_cache(maxsize=None)
def _packed_inputs(k, count, dtype, issue, ef):
    """What every member contributes on a packed wire: its input through q8_quantize_ref and q8_dequantize_ref, cut to
    the count; ``ef``: through q8_quantize_ef_ref from a zero residual, with the residual that leaves.  Made once per
    input set, since the packing is what a packed reference costs."""
    wide, residuals = [], []
    for x in _inputs(k, count, dtype, issue):
        if ef:
            codes, exps, res = q8_quantize_ef_ref(x, dtype, np.zeros(q8_blocks(count) * Q8_BLOCK, np.float32))
            residuals.append(res)
        else:
            codes, exps = q8_quantize_ref(x, dtype)
        wide.append(q8_dequantize_ref(codes, exps)[:count])
    for a in wide + residuals:
        a.setflags(write=False)
    return tuple(wide), tuple(residuals)


@functools.lru_cache(maxsize=None)
def _reference(k, count, op, dtype, out, scale, issue, wire=None, ef=False):
    """What every rank must hold: one array (all_reduce, all_gather) or rank r's piece (reduce_scatter).  On a packed
    wire it is ops/peer_ref's allreduce_q8_ref, allreduce_q8x2_ref, reduce_scatter_q8_ref and their feedback forms from
    a zero residual, composed as those compose them from the members' packed inputs (tests/test_peer_zero1_loops_cpu.py
    holds the composition to them)."""
    if wire in ("fp8", "fp8x2"):
        wide, _ = _packed_inputs(k, count, dtype, issue, ef)
        acc = allreduce_ref(list(wide), "fp32", "fp32", scale)
        if wire == "fp8x2":
            acc = q8_dequantize_ref(*q8_quantize_ref(acc, "fp32"))[:count]
        full = bf16_round(acc) if out == "bf16" else acc
        if op == "all_reduce":
            ref = [full] * k
        else:
            ref = [full[min(count, a * Q8_BLOCK):min(count, b * Q8_BLOCK)] for a, b in q8_slices(q8_blocks(count), k)]
        for a in ref:
            a.setflags(write=False)
        return tuple(ref)
    xs = list(_inputs(k, count, dtype, issue))
    if op == "all_gather":
        ref = [np.concatenate(xs)] * k
    elif op == "all_reduce":
        ref = [allreduce_ref(xs, dtype, out, scale)] * k
    else:
        ref = reduce_scatter_ref(xs, dtype, out, scale)
    for a in ref:
        a.setflags(write=False)
    return tuple(ref)


def _plan(k, counts, cases=None, issues=2):
    """(case, issue, inputs, per-rank reference) of every case of ``selftest_cases`` (or of ``cases``), each issued
    ``issues`` times in a row."""
    plan = []
    for case in (pc.selftest_cases(k, counts) if cases is None else cases):
        for issue in range(issues):
            key = (k, case["count"], case["op"], case["dtype"], case["out_dtype"], case["scale"], issue, case.get("wire"), bool(case.get("ef")))
            plan.append((case, issue, list(_inputs(k, case["count"], case["dtype"], issue)), _reference(*key)))
    return plan


def _capacity(k, counts, cases=None):
    return pc._case_capacity(k, pc.selftest_cases(k, counts) if cases is None else cases)


def _issue(comm, case, x):
    """A case as ``run_case`` issues it, without the reference that ``run_case`` computes in every rank's thread: the
    packed wires' references cost too much for that.  A feedback case starts from a reset residual, which is what its
    reference assumes."""
    count, dtype, out, ef = int(case["count"]), case["dtype"], case["out_dtype"], bool(case.get("ef"))
    if case["op"] == "all_gather":
        comm.write(x, comm.gather_slot(count, dtype))
        n = comm.all_gather(count, dtype)
        return np.concatenate([comm.read(p * n * (16 // pc._ELEM[dtype]), count, dtype) for p in range(comm.world)])
    if ef:
        comm.reset_error_feedback()
    comm.write(x)
    if case["op"] == "all_reduce":
        comm.all_reduce(count, dtype, case["algo"], out, case["scale"], wire=case.get("wire"), error_feedback=ef)
        return comm.read(0, count, out)
    first, n = comm.reduce_scatter(count, dtype, out, case["scale"], wire=case.get("wire"), error_feedback=ef)
    return comm.read(first, n, out)


def _issue_all(plan, run_case=True):
    """A rank's body: issues the plan through ``run_case`` (or, for a plan with packed wires or large counts, through
    ``_issue``, which makes the same calls); returns what differed."""

    def body(comm):
        bad = []
        for case, issue, xs, refs in plan:
            before = comm.barriers
            got = pc.run_case(comm, case, xs)[0] if run_case else _issue(comm, case, xs[comm.rank])
            ref = refs[comm.rank]
            what = (case["op"], case["count"], case["dtype"], case["out_dtype"], case["algo"], issue, case.get("wire"), bool(case.get("ef")))
            if comm.barriers - before != 2:
                bad.append(("barriers", comm.barriers - before) + what)
            if got.dtype != ref.dtype or got.shape != ref.shape:
                bad.append(("type", str(got.dtype), got.shape) + what)
            elif not np.array_equal(pc._bits(got), pc._bits(ref)):
                bad.append(("bits", int(np.count_nonzero(pc._bits(got) != pc._bits(ref)))) + what)
            if case.get("ef"):  # what the packing dropped, of the rank's whole window
                want = _packed_inputs(comm.world, case["count"], case["dtype"], issue, True)[1][comm.rank]
                res = comm.residual(0, want.size)
                if not np.array_equal(pc._bits(res), pc._bits(want)):
                    bad.append(("residual", int(np.count_nonzero(pc._bits(res) != pc._bits(want)))) + what)
        return bad, comm.launches

    return body


def _assert_exact(devices, counts, cases=None, issues=2, comm_cls=pc.PeerComm, run_case=True):
    k = len(devices)
    plan = _plan(k, counts, cases, issues)
    res = pc.run_thread_ranks(devices, _issue_all(plan, run_case), _capacity(k, counts, cases), timeout_s=30.0, comm_cls=comm_cls)
    assert len(res) == k
    for r, (bad, launches) in enumerate(res):
        assert not bad, (r, bad[:4])
        assert launches >= len(plan) // 2  # the kernels ran: only empty slices launch nothing
    return plan


# -- 1. exact bits, every op ------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 8, 16])
def test_every_op_is_exact_on_thread_ranks(k):
    plan = _assert_exact([0] * k, _counts(k))
    cases = [c for c, issue, _, _ in plan if issue == 0]
    assert {c["op"] for c in cases} == {"all_reduce", "reduce_scatter", "all_gather"}
    assert {(c["dtype"], c["out_dtype"]) for c in cases} == {("bf16", "bf16"), ("fp32", "fp32"), ("bf16", "fp32")}
    assert {c["algo"] for c in cases if c["op"] == "all_reduce"} == {"oneshot", "twoshot"}
    assert all(c["scale"] == 1.0 / k for c in cases if (c["dtype"], c["out_dtype"]) == ("bf16", "fp32"))


# -- 2. more than one tile per block ----------------------------------------------------------
class _Phase1Grids(pc.PeerComm):
    """Records the grid of every phase 1: ``_leave`` is the first thing a rank does after that launch."""

    def _leave(self):
        self.grids = getattr(self, "grids", []) + [self._b.r.last_grid]
        super()._leave()


WIDE_CTAS = 16  # the cap of the test below


def test_wide_mean_with_more_than_one_tile_per_block():
    """131587 vectors are 128 tiles of 256 x 4: on the default grid (CUs x 8 / 4 members, 512 blocks on 256 CUs) every
    block takes one tile at most, in the one-shot as in the two-shot's slice of 32 tiles.  The communicator is therefore
    capped at WIDE_CTAS blocks, and the test asserts what its name says from the grids the launches had."""
    k, count = 4, (1 << 20) + 4113
    plan = []
    for algo in pc.ALGOS:
        case = {"op": "all_reduce", "count": count, "dtype": "bf16", "out_dtype": "fp32", "algo": algo, "scale": 1.0 / k}
        plan.append((case, 0, list(_inputs(k, count, "bf16", 0)), _reference(k, count, "all_reduce", "bf16", "fp32", 1.0 / k, 0)))
    issue = _issue_all(plan)
    res = pc.run_thread_ranks([0] * k, lambda comm: issue(comm) + (comm.grids,), -(-count * 2 // 16) * 16, timeout_s=30.0,
                              comm_cls=functools.partial(_Phase1Grids, max_ctas=WIDE_CTAS))
    n_vec = -(-count // 8)
    units = {"oneshot": [n_vec] * k, "twoshot": [b - a for a, b in peer_slices(n_vec, k)]}
    for r, (bad, launches, grids) in enumerate(res):
        assert not bad, (r, bad)
        assert launches == 3  # one-shot: a reduce; two-shot: a reduce and a gather
        assert len(grids) == len(pc.ALGOS)
        for algo, grid in zip(pc.ALGOS, grids):
            tiles, _ = launch_walk(units[algo][r], grid, launch_u("peer_reduce", k))
            print(f"wide mean rank {r} {algo}: grid {grid}, tiles per block {tiles}")
            assert 1 <= grid <= WIDE_CTAS and min(tiles) >= 2, (r, algo, grid, tiles)


# -- 3. mismatch ------------------------------------------------------------------------------
def test_mismatched_calls_raise_on_every_rank_before_any_launch():
    def body(comm):
        comm.write(np.ones(64, np.float32))
        with pytest.raises(pc.PeerCommMismatch):
            comm.all_reduce(64 if comm.rank != 1 else 60, "fp32", "twoshot")
        return comm.barriers, comm.launches

    assert pc.run_thread_ranks([0, 0, 0], body, 1 << 12, timeout_s=20.0) == [(1, 0)] * 3


# -- 4. a late rank cannot hang the GPU -------------------------------------------------------
def test_late_rank_times_the_others_out_on_the_host():
    cap, parked = 1 << 12, pc.parked_bytes()

    def body(comm):
        if comm.rank == 1:
            return "late"  # constructed, never calls the collective
        comm.write(np.ones(64, np.float32))
        t0 = time.monotonic()
        with pytest.raises(pc.PeerCommTimeout):
            comm.all_reduce(64, "fp32", "oneshot")
        took = time.monotonic() - t0
        assert comm.broken and comm.launches == 0
        t0 = time.monotonic()
        with pytest.raises(pc.PeerCommTimeout):
            comm.all_reduce(64, "fp32", "oneshot")
        assert time.monotonic() - t0 < 0.5  # at once: no barrier is tried
        t0 = time.monotonic()
        comm.close()
        assert time.monotonic() - t0 < 0.5  # close() skips its barriers, and frees nothing
        return took

    res = pc.run_thread_ranks([0, 0, 0], body, cap, timeout_s=2.0)
    assert res[1] == "late"
    assert all(1.5 < res[r] < 4.0 for r in (0, 2)), res
    assert pc.parked_bytes() >= parked + 2 * 3 * cap  # ranks 0 and 2 kept their window and out
    _assert_exact([0, 0, 0], [7])  # the device is as usable as before


# -- 5. missing rank at construction ----------------------------------------------------------
def test_missing_rank_times_out_in_the_constructor():
    from gpu_topology_on_k8s_amd._native import load

    load("_probe").PeerRank(0, 0, 2, 1 << 12).release()  # the runtime and the device are up before the clock starts
    parked = pc.parked_bytes()
    t0 = time.monotonic()
    with pytest.raises(pc.PeerCommTimeout):
        pc.PeerComm(0, 2, 0, pc.MemoryStore(timeout_s=1.0), 1 << 12, timeout_s=1.0, backend="device")
    assert 0.5 < time.monotonic() - t0 < 3.0
    assert pc.parked_bytes() == parked  # released: no peer ever had the addresses


# -- 6. foreign pointer -----------------------------------------------------------------------
def test_an_address_of_another_process_is_refused(monkeypatch):
    made = []

    class Spy(pc._DeviceBackend):
        def __init__(self, *a):
            super().__init__(*a)
            made.append(self.r)

    monkeypatch.setattr(pc, "_DeviceBackend", Spy)
    store = pc.MemoryStore(timeout_s=5.0)
    store.set("peer_comm/ptr/1", json.dumps({"pid": os.getpid() + 1, "device": 0, "window": 1 << 40, "out": 1 << 41}))
    with pytest.raises(pc.PeerCommError, match="threads of one process"):
        pc.PeerComm(0, 2, 0, store, 1 << 12, timeout_s=5.0, backend="device")
    assert len(made) == 1 and made[0].launches == 0 and made[0].released


# -- 7. two distinct devices ------------------------------------------------------------------
def test_two_distinct_devices():
    from gpu_topology_on_k8s_amd.ops.probe import device_count

    if device_count() < 2:
        pytest.skip("needs two GPUs: the only test here that crosses a link")
    _assert_exact([0, 1], [8 * 1024 * 2 + 11])


# -- 8. CLI -----------------------------------------------------------------------------------
def _validate(*extra):
    p = subprocess.run([sys.executable, "-m", "gpu_topology_on_k8s_amd", "validate", "--backend", "peer", *extra, "--devices", "0,0,0",
                        "--dtype", "bf16", "--min-bytes", "4096", "--max-bytes", "1048576"],
                       capture_output=True, text=True, timeout=240, cwd=REPO)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    return [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]


def test_validate_cli_thread_ranks():
    lines = _validate("--ranks", "thread")
    first, summary, points = lines[0], lines[-1], lines[1:-1]
    assert first["selftest"] is True and first["wrong"] == 0 and first["barriers_per_collective"] == [2]
    assert first["collectives"] == 2 * first["cases"] == 2 * len(pc.selftest_cases(3)) and first["launches"] > 0
    assert [p["bytes"] for p in points] == [b for b in (4096, 16384, 65536, 262144, 1048576) for _ in range(2)]
    for p in points:
        assert p["ranks"] == "thread" and p["wrong"] == 0 and p["backend"] == "peer" and p["k"] == 3
        assert p["count"] * 2 == p["bytes"] and p["time_us"] > 0 and 0 < p["barrier_us"] <= p["time_us"]
    assert [p["algo"] for p in points[:2]] == ["oneshot", "twoshot"]
    assert summary["summary"] is True and summary["wrong"] == 0 and summary["ranks"] == "thread"


def test_validate_cli_driver_ranks_print_what_they_printed():
    lines = _validate()
    keys = {"k", "devices", "bytes", "count", "time_us", "algbw_gbps", "busbw_gbps", "wrong", "backend", "algo"}
    assert len(lines) == 11 and all(set(p) == keys for p in lines[:-1])
    assert "ranks" not in lines[-1] and "selftest" not in lines[0] and lines[-1]["wrong"] == 0
