"""GPU tests of the K7 peer all-reduce (csrc/probe/peer_allreduce.h and its driver, peer_driver.h).

Members repeat device 0, which runs the k-member indexing, the slice plan and the event ordering on
one GPU.  The exact tests compare every element of every member's output with the numpy reference
(ops/peer_ref.py: fp32 sum in member order, one rounding) at tolerance zero."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_topology_on_k8s_amd.ops.peer_ref import allreduce_ref, bf16_round

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["bf16", "fp32"]
ALGOS = ["oneshot", "twoshot"]


def _ndev() -> int:
    import torch

    return int(torch.cuda.device_count())  # counts without initialising HIP on this image


def _counts(k):
    # one element; under one vector; k - 1 bf16 vectors for k members (the last slice is empty); whole
    # tiles, then a vector tail, then zero padding; and more than one tile for every block's member
    return [1, 7, 8 * (k - 1), 8 * 1024 * k + 11, (1 << 20) + 4113]


@functools.lru_cache(maxsize=None)
def _case(dtype, k, count):
    """k members' N(0,1) inputs (rounded to bf16 for bf16) and the reference result; made once, read-only."""
    rng = np.random.default_rng(1000 * k + count % 997 + (dtype == "bf16"))
    xs = [rng.standard_normal(count).astype(np.float32) for _ in range(k)]
    if dtype == "bf16":
        xs = [bf16_round(x) for x in xs]
    ref = allreduce_ref(xs, dtype)
    for a in xs + [ref]:
        a.setflags(write=False)
    return xs, ref


def _assert_all_members(outs, ref, what):
    assert len(outs) > 1
    for m, o in enumerate(outs):
        assert o.dtype == ref.dtype and o.shape == ref.shape, (what, m)
        # bit patterns, so that -0.0 / 0.0 and every fp32 bit count
        np.testing.assert_array_equal(o.view(np.uint16 if o.dtype == np.uint16 else np.uint32),
                                      ref.view(np.uint16 if ref.dtype == np.uint16 else np.uint32), err_msg=f"{what} member {m}")
        np.testing.assert_array_equal(o, outs[0], err_msg=f"{what} member {m} vs member 0")


@pytest.mark.parametrize("k", [2, 3, 8, 16])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_member_holds_the_exact_sum(dtype, algo, k):
    from gpu_topology_on_k8s_amd.ops.probe import peer_allreduce_arrays

    for count in _counts(k):
        xs, ref = _case(dtype, k, count)
        outs = peer_allreduce_arrays([0] * k, xs, dtype, algo)
        assert len(outs) == k
        _assert_all_members(outs, ref, f"{dtype} {algo} k={k} count={count}")


@pytest.mark.parametrize("algo", ALGOS)
def test_sum_is_taken_in_member_order(algo):
    """fp32 (2^24, 1, -2^24): member order gives (2^24 + 1) - 2^24 = 0, any other order or a tree gives 1."""
    from gpu_topology_on_k8s_amd.ops.probe import peer_allreduce_arrays

    xs = [np.full(4096, v, dtype=np.float32) for v in (2.0 ** 24, 1.0, -(2.0 ** 24))]
    np.testing.assert_array_equal(allreduce_ref(xs, "fp32"), np.zeros(4096, np.float32))
    outs = peer_allreduce_arrays([0, 0, 0], xs, "fp32", algo)
    assert len(outs) == 3
    for o in outs:
        np.testing.assert_array_equal(o, np.zeros(4096, np.float32))


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rounds_repeat_the_result(dtype, algo):
    """Three all-reduces of the same inputs back to back (twoshot: each phase 1 overwrites the slice
    the other members' phase 2 has just read) leave what one leaves."""
    from gpu_topology_on_k8s_amd.ops.probe import peer_allreduce_arrays

    k, count = 3, 8 * 1024 * 3 + 11
    xs, ref = _case(dtype, k, count)
    once = peer_allreduce_arrays([0] * k, xs, dtype, algo, rounds=1)
    thrice = peer_allreduce_arrays([0] * k, xs, dtype, algo, rounds=3)
    _assert_all_members(thrice, ref, f"{dtype} {algo} rounds=3")
    for a, b in zip(once, thrice):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_timed_allreduce_checks_itself(dtype, algo):
    """The timed entry point: device-made inputs, rounds alternating between two input sets, every
    member's output checked on the device against the last round's set."""
    from gpu_topology_on_k8s_amd.ops.probe import peer_allreduce

    nbytes = (8 << 20) + 4112
    elem = 2 if dtype == "bf16" else 4
    r = peer_allreduce([0] * 4, nbytes // elem, dtype, algo, iters=3, warmup_iters=1)
    print(json.dumps({"dtype": dtype, "algo": algo, "algbw_gbps": round(r["algbw_gbps"], 1), "time_us": round(r["time_us"], 1)}))
    assert r["ok"] is True and r["wrong"] == 0, r
    assert r["bytes"] == nbytes and r["count"] == nbytes // elem
    assert len(r["ms_member"]) == 4 and r["time_us"] == pytest.approx(max(r["ms_member"]) * 1e3 / 3)
    assert r["algbw_gbps"] > 0 and r["wall_ms"] > 0
    assert r["busbw_gbps"] == pytest.approx(r["algbw_gbps"] * 1.5)


@pytest.mark.parametrize("k,vectors", [(3, None), (16, 15)])
@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_timed_allreduce_without_warmup(dtype, algo, iters, k, vectors):
    """The timed entry point with no round before the timed ones: one round on one input set
    (iters=1), two rounds on two sets (iters=2).  k=3 with tiles, a tail and padding; k=16 with 15
    vectors, so the last member's slice is empty and its two-shot reduce launches nothing."""
    from gpu_topology_on_k8s_amd.ops.probe import peer_allreduce

    elem = 2 if dtype == "bf16" else 4
    count = 8 * 1024 * 3 + 11 if vectors is None else (16 // elem) * vectors
    r = peer_allreduce([0] * k, count, dtype, algo, iters=iters, warmup_iters=0)
    assert r["ok"] is True and r["wrong"] == 0, r
    assert len(r["ms_member"]) == k
    assert r["bytes"] == count * elem and r["count"] == count


def test_argument_checks():
    from gpu_topology_on_k8s_amd.ops.probe import peer_allreduce, peer_allreduce_arrays

    x = np.zeros(8, np.float32)
    for bad in (lambda: peer_allreduce([0], 8), lambda: peer_allreduce([0] * 17, 8), lambda: peer_allreduce([0, 99], 8),
                lambda: peer_allreduce([0, 0], 0), lambda: peer_allreduce([0, 0], 8, "fp16"),
                lambda: peer_allreduce([0, 0], 8, "bf16", "ring"), lambda: peer_allreduce_arrays([0, 0], [x], "fp32"),
                lambda: peer_allreduce_arrays([0, 0], [x, x], "bf16"), lambda: peer_allreduce_arrays([0, 0], [x, x[:4]], "fp32")):
        with pytest.raises(ValueError):
            bad()


def test_validate_cli_peer_backend():
    """``gtk validate --backend peer`` in a child process: both algorithms at every size, exact."""
    p = subprocess.run([sys.executable, "-m", "gpu_topology_on_k8s_amd", "validate", "--backend", "peer", "--devices", "0,0,0",
                        "--min-bytes", "1024", "--max-bytes", "1048576", "--algo", "both", "--cpu-bind", "off"],
                       capture_output=True, text=True, timeout=240, cwd=REPO)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    summary = lines[-1]
    assert summary["summary"] is True and summary["wrong"] == 0 and summary["backend"] == "peer" and summary["k"] == 3
    points = lines[:-1]
    assert [(q["bytes"], q["algo"]) for q in points] == [(b, a) for b in (1024, 4096, 16384, 65536, 262144, 1048576) for a in ALGOS]
    assert all(q["wrong"] == 0 and q["backend"] == "peer" for q in points)


@pytest.mark.skipif(_ndev() < 2, reason="needs >= 2 visible GPUs (single-GPU box): the xGMI path of K7 is not run")
def test_two_distinct_devices():
    from gpu_topology_on_k8s_amd.ops.probe import peer_allreduce_arrays

    for algo in ALGOS:
        for dtype in DTYPES:
            xs, ref = _case(dtype, 2, (1 << 20) + 4113)
            _assert_all_members(peer_allreduce_arrays([0, 1], xs, dtype, algo), ref, f"{dtype} {algo} devices 0,1")
