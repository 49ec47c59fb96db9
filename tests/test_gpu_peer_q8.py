"""GPU tests of the K7 fp8 wire (csrc/probe/peer_q8.h): the quantize kernel against the numpy rule, code for
code, which is what decides between the hardware conversions and integer arithmetic; the all-reduce on
the packed form against ``allreduce_q8_ref``, bit for bit on every member; the ordering of the packed
buffers' reuse; and the wire through the peer communicator's device backend and the CLI.

Members repeat device 0, so a one-GPU box runs every member bucket.  Every member's packed form is made
once on the host (ops/peer_ref.py), shared by the cases that sum it and left unchanged."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_peer_q8_cpu as Q
from gpu_topology_on_k8s_amd.ops import probe
from gpu_topology_on_k8s_amd.ops.peer_ref import (allreduce_q8_ref, allreduce_ref, bf16_round, q8_dequantize_ref, q8_quantize_ref,
                                                  reduce_scatter_q8_ref)
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = (("bf16", "bf16"), ("fp32", "fp32"), ("bf16", "fp32"))
BIG = (1 << 20) + 4113


# -- 1. the quantize kernel -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_quantize_kernel_matches_the_rule_code_for_code(dtype):
    """Crafted blocks (spot values, ties of both signs, subnormal codes, zeros, one large among tiny) and
    1 Mi random values over 2^-43 .. 2^43; the count is no multiple of 32 and the window holds non-zero
    bytes after it."""
    x = np.concatenate([Q.crafted(dtype), Q.wide_random(1 << 20, dtype)])[:-5]
    want_c, want_e = q8_quantize_ref(Q.as_input(x, dtype), dtype)
    got_c, got_e = probe.peer_q8_quantize(0, Q.as_input(x, dtype), dtype)
    assert got_c.dtype == np.uint8 and got_c.shape == want_c.shape and got_e.shape == want_e.shape
    bad_e = np.flatnonzero(got_e != want_e)
    assert bad_e.size == 0, [(int(b), int(got_e[b]), int(want_e[b])) for b in bad_e[:8]]
    bad = np.flatnonzero(got_c != want_c)
    assert bad.size == 0, (bad.size, [(int(i), float(x[i]) if i < x.size else None, int(want_e[i // 32]), hex(got_c[i]), hex(want_c[i]))
                                      for i in bad[:12]])


# -- 2. the all-reduce on the caller's arrays -------------------------------------------------
def _counts(k):
    return [1, 31, 32, 33, 32 * (k - 1), 512 * k + 37, BIG]


@functools.lru_cache(maxsize=None)
def _member(dtype, m, count):
    """Member m's input and what it contributes to a sum, its dequantised packed form."""
    x = Q.as_input(Q.wide_random(count, dtype, seed=100 + m) * np.float32(2.0 ** -30), dtype)
    back = q8_dequantize_ref(*q8_quantize_ref(x, dtype))[:count]
    x.setflags(write=False)
    back.setflags(write=False)
    return x, back


@functools.lru_cache(maxsize=None)
def _reference(k, count, dtype, out):
    acc = allreduce_ref([_member(dtype, m, count)[1] for m in range(k)], "fp32", "fp32", 1.0 / k if dtype != out else 1.0)
    ref = bf16_round(acc) if out == "bf16" else acc
    ref.setflags(write=False)
    return ref


def test_shared_reference_is_allreduce_q8_ref():
    for dtype, out in PAIRS:
        xs = [_member(dtype, m, 512 * 3 + 37)[0] for m in range(3)]
        np.testing.assert_array_equal(_reference(3, 512 * 3 + 37, dtype, out), allreduce_q8_ref(xs, dtype, out, 1.0 / 3 if dtype != out else 1.0))


@pytest.mark.parametrize("algo", ["oneshot", "twoshot"])
@pytest.mark.parametrize("k", [2, 3, 5, 8, 16])
def test_arrays_are_bit_equal_on_every_member(k, algo):
    for dtype, out in PAIRS:
        for count in _counts(k):
            xs = [_member(dtype, m, count)[0] for m in range(k)]
            ref = _reference(k, count, dtype, out)
            rounds = 3 if count == 512 * k + 37 else 1
            got = probe.peer_allreduce_arrays([0] * k, xs, dtype, algo, rounds, out, 1.0 / k if dtype != out else 1.0, wire="fp8")
            assert len(got) == k
            for m, g in enumerate(got):
                assert g.dtype == ref.dtype and g.shape == ref.shape
                bad = np.flatnonzero(pc._bits(g) != pc._bits(ref))
                assert bad.size == 0, (dtype, out, count, m, bad.size, bad[:8].tolist())


def test_native_wire_is_the_default_and_unchanged():
    xs = [_member("bf16", m, 4099)[0] for m in range(3)]
    ref = allreduce_ref(xs, "bf16")
    for got in (probe.peer_allreduce_arrays([0] * 3, xs, "bf16", "twoshot"), probe.peer_allreduce_arrays([0] * 3, xs, "bf16", "twoshot", wire="native")):
        for g in got:
            np.testing.assert_array_equal(g, ref)
    with pytest.raises(ValueError):
        probe.peer_allreduce_arrays([0] * 3, xs, "bf16", "twoshot", wire="fp4")


# -- 3. packed buffers are reused in order ----------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("algo", ["oneshot", "twoshot"])
def test_alternating_rounds_leave_the_last_rounds_sum(algo, dtype):
    """Rounds alternate between two input sets; the integer patterns survive packing unchanged, so a round
    that read a packed buffer before or after its turn leaves elements of the other set's sum."""
    r = probe.peer_allreduce([0] * 4, BIG, dtype, algo, iters=3, warmup_iters=1, wire="fp8")
    assert r["wire"] == "fp8" and r["wrong"] == 0 and r["ok"] and r["quantize_us"] > 0 and r["sum_us"] > 0


# -- 4. thread ranks on the device backend ----------------------------------------------------
def _small(k):
    return [1, 33, 32 * (k - 1), 512 * k + 37]


def test_thread_ranks_are_bit_equal_twice_in_a_row():
    k = 3
    cases = pc.selftest_cases_q8(k, _small(k))
    plan = []
    for ci, case in enumerate(cases):
        for issue in range(2):
            xs = [pc.case_input(ci, issue, p, case["count"], case["dtype"]) for p in range(k)]
            args = (xs, case["dtype"], case["out_dtype"], case["scale"])
            ref = [allreduce_q8_ref(*args)] * k if case["op"] == "all_reduce" else reduce_scatter_q8_ref(*args)
            plan.append((case, xs, ref))

    def body(comm):
        bad = []
        for case, xs, ref in plan:
            before = comm.barriers
            got, _ = pc.run_case(comm, case, xs)
            if comm.barriers - before != 2 or got.dtype != ref[comm.rank].dtype or not np.array_equal(pc._bits(got), pc._bits(ref[comm.rank])):
                bad.append((case, comm.barriers - before))
        return bad

    res = pc.run_thread_ranks([0] * k, body, pc._case_capacity(k, cases), timeout_s=30.0)
    assert res == [[]] * k, [r[:2] for r in res]


def test_thread_ranks_mask_the_stale_window_and_count_launches():
    k = 3
    big, small = Q.stale_window_case(k)
    ref = allreduce_q8_ref(small, "bf16")
    stale = Q.stale_window_body(big, small)

    def body(comm):
        outs = stale(comm)
        counts = []
        for algo in pc.ALGOS:  # 128 blocks: no rank's slice is empty, and an empty slice is no launch
            before = comm.launches
            comm.all_reduce(4096, "bf16", algo, wire="fp8")
            counts.append(comm.launches - before)
        before = comm.launches
        comm.all_reduce(4096, "bf16", "oneshot")
        return outs, counts + [comm.launches - before]

    for outs, counts in pc.run_thread_ranks([0] * k, body, 4096 * 2, timeout_s=30.0):
        assert counts == [2, 3, 1]  # quantize and sum; quantize, sum and gather; the native reduce alone
        for got in outs:
            np.testing.assert_array_equal(got, ref)


def test_rank_checks_bounds_before_any_launch():
    from gpu_topology_on_k8s_amd._native import load

    cap = 64 * 4 + 16  # four blocks of bf16 and one vector more
    ranks = [load("_probe").PeerRank(0, r, 2, cap) for r in range(2)]
    try:
        devs, wins, outs = [0, 0], [r.window_ptr() for r in ranks], [r.out_ptr() for r in ranks]
        packs = [r.packed_ptr() for r in ranks]
        ranks[0].open_peers(devs, wins, outs)
        for call in (lambda: ranks[0].quantize(0, 1, 32, "bf16"), lambda: ranks[0].reduce_q8(0, 1, "bf16", 1.0)):
            with pytest.raises(RuntimeError):
                call()
        with pytest.raises(ValueError):
            ranks[0].open_peers(devs, wins, outs, [packs[1], packs[0]])
        with pytest.raises(ValueError):
            ranks[0].open_peers(devs, wins, outs, [packs[0], wins[1] + 16])
        for r in ranks:
            r.open_peers(devs, wins, outs, packs)
        for call in (lambda: ranks[0].quantize(0, 5, 160, "bf16"), lambda: ranks[0].quantize(0, 3, 96, "fp32"), lambda: ranks[0].quantize(2, 1, 32, "bf16"),
                     lambda: ranks[0].reduce_q8(0, 5, "bf16", 1.0), lambda: ranks[0].reduce_q8(0, 5, "fp32", 1.0), lambda: ranks[0].reduce_q8(3, 2, "fp32", 1.0),
                     lambda: ranks[0].quantize(0, 1, 32, "fp16"), lambda: ranks[0].reduce_q8(0, 1, "fp16", 1.0)):
            with pytest.raises(ValueError):
                call()
        assert ranks[0].launches == 0
        # the whole capacity in blocks: the last whole block of an fp32 out ends where out ends
        x = bf16_round(np.linspace(-3, 3, 128).astype(np.float32))
        for r in ranks:
            r.write_host(x, 0)
            r.quantize(0, 4, 128, "bf16")
            r.synchronize()
        ranks[0].reduce_q8(0, 4, "fp32", 0.5)
        got = ranks[0].read_host(0, 128 * 4).view(np.float32)
        np.testing.assert_array_equal(got, allreduce_q8_ref([x, x], "bf16", "fp32", 0.5))
        assert ranks[0].launches == 2
    finally:
        for r in ranks:
            r.release()


# -- 5. CLI -----------------------------------------------------------------------------------
def test_validate_cli_fp8_thread_ranks():
    p = subprocess.run([sys.executable, "-m", "gpu_topology_on_k8s_amd", "validate", "--backend", "peer", "--wire", "fp8", "--ranks", "thread",
                        "--devices", "0,0,0", "--dtype", "bf16", "--min-bytes", "4096", "--max-bytes", "262144"],
                       capture_output=True, text=True, timeout=240, cwd=REPO)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    first, summary, points = lines[0], lines[-1], lines[1:-1]
    assert first["selftest"] is True and first["wrong"] == 0 and first["q8_wrong"] == 0 and first["barriers_per_collective"] == [2]
    assert first["q8_collectives"] == 2 * len(pc.selftest_cases_q8(3)) and first["q8_launches"] > 0
    assert points and all(p["wire"] == "fp8" and p["wrong"] == 0 for p in points)
    assert summary["wire"] == "fp8" and summary["wrong"] == 0 and summary["selftest_wrong"] == 0
