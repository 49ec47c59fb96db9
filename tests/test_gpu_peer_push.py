"""GPU tests of the K7 push all-reduce (peer_reduce_push_kernel, peer_q8_sum_push_kernel): member m sums slice m
of every input and stores the result into slice m of every member's out, in one launch with no second phase.

Members repeat device 0, so every remote store lands in the device's own memory; one test runs on two
devices where two are visible.  Every comparison is bit for bit against ops/peer_ref.py (where a NaN comes
out, which NaN is free, as in tests/test_gpu_peer_nonfinite.py).  Inputs and references are made once and are
read-only."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_peer_nonfinite_cpu as N
import test_peer_push_cpu as P
from gpu_topology_on_k8s_amd.ops import probe
from gpu_topology_on_k8s_amd.ops.peer_ref import allreduce_q8_ref, allreduce_ref, bits, is_nan_bits, mismatches
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [2, 3, 8, 16]
PAIRS = (("bf16", "bf16"), ("fp32", "fp32"), ("bf16", "fp32"))
PUSH = probe.PEER_PUSH


def _scale(dtype, out, k):
    return 1.0 / k if dtype != out else 1.0


@functools.lru_cache(maxsize=None)
def _inputs(dtype, k, count):
    xs = tuple(pc.case_input(0, 0, m, count, dtype) for m in range(k))
    for a in xs:
        a.setflags(write=False)
    return xs


@functools.lru_cache(maxsize=None)
def _reference(dtype, out, k, count, wire):
    ref = (allreduce_q8_ref if wire == "fp8" else allreduce_ref)(list(_inputs(dtype, k, count)), dtype, out, _scale(dtype, out, k))
    ref.setflags(write=False)
    return ref


def _assert_all_members(outs, ref, k, what):
    assert len(outs) == k > 1
    for m, o in enumerate(outs):
        assert o.dtype == ref.dtype and o.shape == ref.shape, (what, m)
        np.testing.assert_array_equal(bits(o), bits(ref), err_msg=f"{what} member {m}")
        np.testing.assert_array_equal(bits(o), bits(outs[0]), err_msg=f"{what} member {m} vs member 0")


# -- 1. the driver on the caller's arrays -----------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("pair", PAIRS)
def test_every_member_holds_the_exact_sum(pair, k):
    dtype, out = pair
    for count in pc.selftest_counts(k):
        outs = probe.peer_allreduce_arrays([0] * k, list(_inputs(dtype, k, count)), dtype, PUSH, 1, out, _scale(dtype, out, k))
        _assert_all_members(outs, _reference(dtype, out, k, count, "native"), k, f"{dtype}->{out} push k={k} count={count}")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("pair", PAIRS)
def test_every_member_holds_the_exact_sum_on_the_fp8_wire(pair, k):
    dtype, out = pair
    for count in pc.selftest_counts_q8(k):
        outs = probe.peer_allreduce_arrays([0] * k, list(_inputs(dtype, k, count)), dtype, PUSH, 1, out, _scale(dtype, out, k),
                                           wire="fp8")
        _assert_all_members(outs, _reference(dtype, out, k, count, "fp8"), k, f"{dtype}->{out} push fp8 k={k} count={count}")


@pytest.mark.parametrize("wire", ["native", "fp8"])
@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("pair", PAIRS)
def test_rounds_repeat_the_result(pair, k, wire):
    """Three pushes of the same inputs back to back, with no event between the members on the native wire,
    leave what one leaves."""
    dtype, out = pair
    count = 8 * 1024 * k + 11
    xs, scale = list(_inputs(dtype, k, count)), _scale(dtype, out, k)
    once = probe.peer_allreduce_arrays([0] * k, xs, dtype, PUSH, 1, out, scale, wire=wire)
    thrice = probe.peer_allreduce_arrays([0] * k, xs, dtype, PUSH, 3, out, scale, wire=wire)
    _assert_all_members(thrice, _reference(dtype, out, k, count, wire), k, f"{dtype}->{out} {wire} rounds=3")
    for a, b in zip(once, thrice):
        np.testing.assert_array_equal(bits(a), bits(b))


@pytest.mark.parametrize("wire", ["native", "fp8"])
@pytest.mark.parametrize("k", KS)
def test_push_equals_twoshot_array_for_array(k, wire):
    for dtype, out in PAIRS:
        for count in (8 * (k - 1), 8 * 1024 * k + 11):
            xs, scale = list(_inputs(dtype, k, count)), _scale(dtype, out, k)
            push = probe.peer_allreduce_arrays([0] * k, xs, dtype, PUSH, 1, out, scale, wire=wire)
            two = probe.peer_allreduce_arrays([0] * k, xs, dtype, "twoshot", 1, out, scale, wire=wire)
            assert len(push) == len(two) == k
            for m in range(k):
                np.testing.assert_array_equal(bits(push[m]), bits(two[m]), err_msg=f"{dtype}->{out} {wire} k={k} count={count} member {m}")


def test_sum_is_taken_in_member_order():
    """fp32 (2^24, 1, -2^24): member order gives (2^24 + 1) - 2^24 = 0, any other order or a tree gives 1."""
    xs = [np.full(4096, v, dtype=np.float32) for v in (2.0 ** 24, 1.0, -(2.0 ** 24))]
    np.testing.assert_array_equal(allreduce_ref(xs, "fp32"), np.zeros(4096, np.float32))
    outs = probe.peer_allreduce_arrays([0, 0, 0], xs, "fp32", PUSH)
    assert len(outs) == 3
    for o in outs:
        np.testing.assert_array_equal(bits(o), np.zeros(4096, np.uint32))


# -- 2. the values the other tests leave out --------------------------------------------------------
def _assert_members_nan_free(outs, ref, k, what):
    assert len(outs) == k
    for m, o in enumerate(outs):
        bad = mismatches(o, ref)
        assert bad.size == 0, (what, m, bad.size, [(int(i), hex(bits(o)[i]), hex(bits(ref)[i])) for i in bad[:8]])
        assert np.array_equal(bits(o), bits(outs[0])), (what, m)  # one member computed the slice: NaN payloads included


@pytest.mark.parametrize("k", KS)
def test_native_wire_sums_the_pair_table_as_ieee(k):
    """All ordered pairs of the specials (signed zeros, fp32 and bf16 subnormals, the infinities, NaNs, sums on
    bf16's rounding edges) at the two-shot's placement, which is the push's: every slice's tiles and tail."""
    for dtype, out in N.PAIRS:
        for count in N.native_counts(k, "twoshot", dtype):
            xs, _ = N.native_case(k, "twoshot", dtype, count)
            for scale in (1.0, 1.0 / k):
                ref = N.native_reference(k, "twoshot", dtype, count, out, scale)
                assert is_nan_bits(ref).sum() > 0
                outs = probe.peer_allreduce_arrays([0] * k, list(xs), dtype, PUSH, 1, out, scale)
                _assert_members_nan_free(outs, ref, k, (dtype, out, k, count, scale))


@pytest.mark.parametrize("k", KS)
def test_fp8_wire_carries_non_finite_blocks_on_every_member(k):
    for dtype, out in N.PAIRS:
        for count in N.q8_counts(k):
            for holders in N.Q8_HOLDERS:
                xs = N.q8_case(k, dtype, count, holders)
                ref = N.q8_reference(k, dtype, count, holders, out)
                assert is_nan_bits(ref).sum() > 0
                outs = probe.peer_allreduce_arrays([0] * k, list(xs), dtype, PUSH, 1, out, N.q8_scale(k, dtype, out), wire="fp8")
                _assert_members_nan_free(outs, ref, k, (dtype, out, k, count, holders))


# -- 3. the timed entry point checks itself ---------------------------------------------------------
@pytest.mark.parametrize("wire", ["native", "fp8"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_timed_allreduce_checks_itself(dtype, wire):
    elem = 2 if dtype == "bf16" else 4
    count = ((2 << 20) + 4112) // elem
    r = probe.peer_allreduce([0] * 4, count, dtype, PUSH, iters=3, warmup_iters=1, wire=wire)
    print(json.dumps({"dtype": dtype, "wire": wire, "algo": r["algo"], "algbw_gbps": round(r["algbw_gbps"], 1),
                      "time_us": round(r["time_us"], 1)}))
    assert r["ok"] is True and r["wrong"] == 0 and r["algo"] == PUSH and r["dry_run"] is False, r
    assert len(r["ms_member"]) == 4 and r["time_us"] == pytest.approx(max(r["ms_member"]) * 1e3 / 3)
    if wire == "fp8":
        assert r["quantize_us"] > 0 and r["sum_us"] > 0 and "gather_us" not in r


@pytest.mark.parametrize("wire", ["native", "fp8"])
@pytest.mark.parametrize("k,vectors", [(3, None), (16, 15)])
@pytest.mark.parametrize("iters", [1, 2])
def test_timed_allreduce_without_warmup(iters, k, vectors, wire):
    """One round on one input set, two rounds on two; k=16 with 15 vectors (fp8: 15 blocks) leaves the last member's slice empty."""
    for dtype in ("bf16", "fp32"):
        elem = 2 if dtype == "bf16" else 4
        count = 8 * 1024 * 3 + 11 if vectors is None else (32 if wire == "fp8" else 16 // elem) * vectors
        r = probe.peer_allreduce([0] * k, count, dtype, PUSH, iters=iters, warmup_iters=0, wire=wire)
        assert r["ok"] is True and r["wrong"] == 0 and len(r["ms_member"]) == k, r


@pytest.mark.parametrize("wire", ["native", "fp8"])
def test_a_dry_run_fails_the_check(wire):
    """Everything but the kernels of the rounds: every out keeps its poison, so the check must say so."""
    for dtype in ("bf16", "fp32"):
        for warm in (0, 1):
            r = probe.peer_allreduce([0] * 3, 8 * 1024 * 3 + 11, dtype, PUSH, iters=2, warmup_iters=warm, wire=wire, dry_run=True)
            assert r["ok"] is False and r["wrong"] > 0 and r["dry_run"] is True, r


def test_argument_checks():
    x = np.zeros(64, np.float32)
    with pytest.raises(ValueError, match="fp8x2"):
        probe.peer_allreduce([0, 0], 64, "bf16", PUSH, wire="fp8x2")
    with pytest.raises(ValueError, match="fp8x2"):
        probe.peer_allreduce_arrays([0, 0], [x, x], "fp32", PUSH, wire="fp8x2")
    with pytest.raises(ValueError, match="push"):
        probe.peer_allreduce([0, 0], 64, "bf16", "ring")
    with pytest.raises(ValueError):
        probe.peer_allreduce([0], 64, "bf16", PUSH)
    pts = probe.peer_sweep([0, 0, 0], [4096, 65536], "bf16", "all", iters=1, warmup_iters=0)
    assert [(p["bytes"], p["algo"]) for p in pts] == [(b, a) for b in (4096, 65536) for a in ("oneshot", "twoshot", PUSH)]
    assert all(p["ok"] for p in pts) and [sum(p["fastest"] for p in pts[i:i + 3]) for i in (0, 3)] == [1, 1]
    assert [p["algo"] for p in probe.peer_sweep([0, 0], [4096], "bf16", PUSH, iters=1, warmup_iters=0)] == [PUSH]


# -- 4. the communicator's device backend on thread ranks -------------------------------------------
@pytest.mark.parametrize("devices", [[0, 0, 0], [0] * 4])
def test_selftest_reports_the_push_cases(devices):
    k = len(devices)
    counts = [1, 33, 8 * (k - 1), 8 * 1024 * k + 11]
    st = pc.selftest(devices, counts=counts, timeout_s=30.0, push=True)
    n = len(pc.selftest_cases_push(k, counts))
    assert st["push_cases"] == n == 5 * len(counts) and st["push_collectives"] == 2 * n
    assert st["push_wrong"] == 0 and st["wrong"] == 0 and st["q8_wrong"] == 0
    assert st["barriers_per_collective"] == [2]
    # per count, issue and rank: three native pushes of at most one launch, two fp8 ones of at most two (a rank
    # whose slice is empty launches no sum); at least the k quantizes of every fp8 issue
    assert 2 * 2 * k * len(counts) <= st["push_launches"] <= 2 * k * len(counts) * (3 + 2 * 2)
    assert st["cases"] == len(pc.selftest_cases(k, counts)) and "push_cases" not in pc.selftest(devices[:2], counts=[33])


@pytest.mark.parametrize("devices", [[0, 0, 0], [0] * 4])
def test_mixed_sequence_and_launches_on_thread_ranks(devices):
    k = len(devices)
    counts = (8 * 64 * k + 11, 8 * 24 * k - 5, 8 * 100 * k + 3)

    def body(comm):
        bad = P.mixed_sequence(comm, counts)
        grew = []
        for issue in range(3):  # every rank's slice holds vectors: one launch per rank and push
            xs = [pc.case_input(9, issue, p, counts[0], "bf16") for p in range(k)]
            comm.write(xs[comm.rank])
            before = comm.launches
            comm.all_reduce(counts[0], "bf16", "push")
            grew.append(comm.launches - before)
            bad += not P._same(comm.read(0, counts[0], "bf16"), allreduce_ref(xs, "bf16"))
        before = comm.launches
        comm.all_reduce(counts[0], "bf16", "push", wire="fp8")  # the quantize and the sum
        return bad, grew, comm.launches - before

    res = pc.run_thread_ranks(devices, body, 16 * (-(-max(counts) * 2 // 16) + 4), timeout_s=30.0)
    assert res == [(0, [1, 1, 1], 2)] * k, res


def _validate(*extra):
    p = subprocess.run([sys.executable, "-m", "gpu_topology_on_k8s_amd", "validate", "--backend", "peer", "--devices", "0,0,0", "--algo",
                        "push", "--max-bytes", "1048576", "--cpu-bind", "off", *extra], capture_output=True, text=True, timeout=240, cwd=REPO)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    return [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]


def test_validate_cli_push():
    lines = _validate()
    summary, points = lines[-1], lines[:-1]
    assert summary["summary"] is True and summary["wrong"] == 0 and summary["algo"] == "push" and summary["k"] == 3
    assert points and all(q["wrong"] == 0 and q["algo"] == "push" and q["backend"] == "peer" for q in points)
    assert points[-1]["bytes"] == 1048576


def test_validate_cli_push_thread_ranks():
    lines = _validate("--ranks", "thread")
    first, summary, points = lines[0], lines[-1], lines[1:-1]
    assert first["selftest"] is True and first["wrong"] == 0 and first["push_wrong"] == 0
    assert first["push_collectives"] == 2 * first["push_cases"] == 2 * len(pc.selftest_cases_push(3)) and first["push_launches"] > 0
    assert points and all(q["wrong"] == 0 and q["algo"] == "push" and q["ranks"] == "thread" for q in points)
    assert summary["summary"] is True and summary["wrong"] == 0 and summary["selftest_wrong"] == 0 and summary["ranks"] == "thread"


# -- 5. two distinct devices ------------------------------------------------------------------------
def _ndev() -> int:
    import torch

    return int(torch.cuda.device_count())  # counts without initialising HIP on this image


@pytest.mark.skipif(_ndev() < 2, reason="needs >= 2 visible GPUs (single-GPU box): no store of the push crosses a link")
def test_two_distinct_devices():
    count = (1 << 20) + 4113
    for wire in ("native", "fp8"):
        for dtype, out in PAIRS:
            outs = probe.peer_allreduce_arrays([0, 1], list(_inputs(dtype, 2, count)), dtype, PUSH, 1, out, _scale(dtype, out, 2), wire=wire)
            _assert_all_members(outs, _reference(dtype, out, 2, count, wire), 2, f"{dtype}->{out} {wire} devices 0,1")
    st = pc.selftest([0, 1], counts=[8 * 1024 * 2 + 11], timeout_s=30.0, push=True)
    assert st["push_wrong"] == 0 and st["wrong"] == 0
