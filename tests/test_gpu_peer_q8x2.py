"""GPU tests of the K7 fp8x2 wire (csrc/probe/peer_q8.h: peer_q8_repack_kernel, peer_q8_unpack_kernel): the two-shot
all-reduce whose gather phase is packed too, against ``allreduce_q8x2_ref`` bit for bit on every member; sums
on ties between codes; non-finite and subnormal values; the ordering of the second packed buffers' reuse;
the wire through the peer communicator's device backend, ``PeerRank``'s bounds and the CLI.

Members repeat device 0, so a one-GPU box runs every member bucket.  The members' inputs and packed forms are
those of tests/test_gpu_peer_q8.py, made once on the host and left unchanged."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_peer_q8 as T
import test_peer_q8_cpu as Q
import test_peer_q8x2_cpu as X
from gpu_topology_on_k8s_amd.ops import probe
from gpu_topology_on_k8s_amd.ops.peer_ref import (allreduce_q8_ref, allreduce_q8x2_ref, allreduce_ref, bf16_round, bf16_to_f32, is_nan_bits,
                                                  mismatches, q8_dequantize_ref, q8_quantize_ref)
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = T.PAIRS
BIG = T.BIG  # the smallest of the counts here at which every slice of k = 3 and of k = 16 spans more than one tile
WIRE = "fp8x2"


# -- 1. the all-reduce on the caller's arrays -------------------------------------------------
def _counts(k):
    return [1, 31, 32, 33, 32 * (k - 1), 512 * k + 37, 8 * 1024 * k + 11] + ([BIG] if k in (3, 16) else [])


@functools.lru_cache(maxsize=None)
def _reference(k, count, dtype, out):
    """The rule from the members' shared packed forms: their fp32 sum in member order, scaled, packed again."""
    s = allreduce_ref([T._member(dtype, m, count)[1] for m in range(k)], "fp32", "fp32", X._scale(dtype, out, k))
    back = q8_dequantize_ref(*q8_quantize_ref(s, "fp32"))[:count]
    ref = bf16_round(back) if out == "bf16" else back
    ref.setflags(write=False)
    return ref


def test_shared_reference_is_allreduce_q8x2_ref():
    for dtype, out in PAIRS:
        xs = [T._member(dtype, m, 512 * 3 + 37)[0] for m in range(3)]
        ref = _reference(3, 512 * 3 + 37, dtype, out)
        np.testing.assert_array_equal(ref, allreduce_q8x2_ref(xs, dtype, out, X._scale(dtype, out, 3)))
    # the inputs' range reaches subnormal codes and zeros in the second packing
    codes, _ = q8_quantize_ref(allreduce_q8_ref(xs, "bf16", "fp32", 1.0 / 3), "fp32")
    assert np.any((codes & 0x7F) == 0) and np.any(((codes & 0x7F) > 0) & ((codes & 0x7F) < 8))


@pytest.mark.parametrize("k", [2, 3, 5, 8, 16])
def test_arrays_are_bit_equal_on_every_member(k):
    for dtype, out in PAIRS:
        for count in _counts(k):
            xs = [T._member(dtype, m, count)[0] for m in range(k)]
            ref = _reference(k, count, dtype, out)
            rounds = 3 if count == 512 * k + 37 else 1
            got = probe.peer_allreduce_arrays([0] * k, xs, dtype, "twoshot", rounds, out, X._scale(dtype, out, k), wire=WIRE)
            assert len(got) == k
            for m, g in enumerate(got):
                assert g.dtype == ref.dtype and g.shape == ref.shape
                bad = np.flatnonzero(pc._bits(g) != pc._bits(ref))
                assert bad.size == 0, (dtype, out, count, m, bad.size, bad[:8].tolist())


def test_oneshot_has_no_gather_phase_to_pack():
    xs = [T._member("bf16", m, 4099)[0] for m in range(3)]
    with pytest.raises(ValueError):
        probe.peer_allreduce_arrays([0] * 3, xs, "bf16", "oneshot", wire=WIRE)
    with pytest.raises(ValueError):
        probe.peer_allreduce([0] * 4, 4099, "bf16", "oneshot", iters=1, warmup_iters=0, wire=WIRE)


@pytest.mark.parametrize("pair", PAIRS)
def test_sums_on_ties_between_codes(pair):
    dtype, out = pair
    k, count = 16, 512 * 16 + 37
    xs = X.integer_inputs(k, count, dtype)
    ref = allreduce_q8x2_ref(xs, dtype, out, 1.0)
    assert np.count_nonzero(pc._bits(ref) != pc._bits(allreduce_q8_ref(xs, dtype, out, 1.0))) > 0
    for g in probe.peer_allreduce_arrays([0] * k, xs, dtype, "twoshot", 1, out, 1.0, wire=WIRE):
        np.testing.assert_array_equal(g, ref)


# -- 2. non-finite and subnormal values -------------------------------------------------------
def crafted_members(dtype):
    """Three members' inputs (float32 values, bf16-representable), one block of 32 elements per case, each
    among ordinary values, and the element of every block the case is about."""
    rng = np.random.default_rng(5)
    blocks, spots = [], []

    def block(e0, e1, e2, at=5, rest=1.0):
        b = [(rng.standard_normal(32) * rest).astype(np.float32) for _ in range(3)]
        for m, v in enumerate((e0, e1, e2)):
            b[m][at] = v
        blocks.append(b)
        spots.append(32 * (len(blocks) - 1) + at)

    block(np.nan, 1.0, 2.0)                                        # a NaN in one member
    block(np.inf, -np.inf, 1.0)                                    # +Inf and -Inf in different members of one element
    block(2.0 ** 127, 2.0 ** 127, 0.0, rest=2.0 ** 100)            # a finite sum that reaches Inf: the second packing codes it as NaN
    block(2.0 ** 126, 2.0 ** 126, 1.875 * 2.0 ** 126, rest=2.0 ** 100)  # a sum of exactly 248 * 2^120: it comes out Inf
    blocks.append([np.zeros(32, np.float32) for _ in range(3)])     # an all-zero block
    spots.append(32 * (len(blocks) - 1))
    blocks.append([np.full(32, -0.0, np.float32) for _ in range(3)])  # -0 + -0 + -0
    spots.append(32 * (len(blocks) - 1))
    sub = np.float32(2.0 ** -133)                                  # subnormal in fp32 and in bf16
    blocks.append([(np.arange(32) - 16).astype(np.float32) * sub * np.float32(m + 1) for m in range(3)])
    spots.append(32 * (len(blocks) - 1) + 3)
    block(3 * sub, -sub, 1.0, rest=1.0)                            # subnormals beside ordinary values
    xs = [np.concatenate([b[m] for b in blocks])[:-3] for m in range(3)]  # the count ends inside the last block
    return [Q.as_input(bf16_to_f32(bf16_round(x)) if dtype == "bf16" else x, dtype) for x in xs], spots


@pytest.mark.parametrize("pair", PAIRS)
def test_non_finite_and_subnormal_values(pair):
    dtype, out = pair
    xs, spots = crafted_members(dtype)
    ref = allreduce_q8x2_ref(xs, dtype, out, 1.0)
    val = bf16_to_f32(ref) if out == "bf16" else ref
    nan = is_nan_bits(ref)
    assert nan[spots[0]] and nan[spots[1]] and nan[spots[2]]       # the reference says what the cases are about
    assert np.isposinf(val[spots[3]])
    assert not pc._bits(ref)[spots[4]:spots[4] + 32].any()
    assert np.all(pc._bits(ref)[spots[5]:spots[5] + 32] == (0x8000 if out == "bf16" else 0x80000000))
    assert not np.any(val[spots[6] - 3:spots[6] + 29])             # a block of subnormals lies under the exponent's clamp
    got = probe.peer_allreduce_arrays([0] * 3, xs, dtype, "twoshot", 1, out, 1.0, wire=WIRE)
    for m, g in enumerate(got):
        bad = mismatches(g, ref)
        assert bad.size == 0, (m, bad[:8].tolist(), pc._bits(g)[bad[:8]].tolist(), pc._bits(ref)[bad[:8]].tolist())


# -- 3. the second packed buffers are reused in order -----------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_alternating_rounds_leave_the_last_rounds_sum(dtype):
    """Rounds alternate between two input sets of values in {-1, 0}, whose sums survive both packings, so a
    phase that ran before or after its turn leaves elements of the other set's sum."""
    r = probe.peer_allreduce([0] * 4, BIG, dtype, "twoshot", iters=3, warmup_iters=1, wire=WIRE)
    assert r["wire"] == WIRE and r["wrong"] == 0 and r["ok"]
    assert r["quantize_us"] > 0 and r["sum_us"] > 0 and r["gather_us"] > 0


# -- 4. thread ranks on the device backend ----------------------------------------------------
def test_thread_ranks_are_bit_equal_twice_in_a_row():
    k = 3
    cases = pc.selftest_cases_q8x2(k, T._small(k))
    plan = []
    for ci, case in enumerate(cases):
        for issue in range(2):
            xs = [pc.case_input(ci, issue, p, case["count"], case["dtype"]) for p in range(k)]
            plan.append((case, xs, allreduce_q8x2_ref(xs, case["dtype"], case["out_dtype"], case["scale"])))

    def body(comm):
        bad = []
        for case, xs, ref in plan:
            before = comm.barriers
            got, _ = pc.run_case(comm, case, xs)
            if comm.barriers - before != 2 or got.dtype != ref.dtype or not np.array_equal(pc._bits(got), pc._bits(ref)):
                bad.append((case, comm.barriers - before))
        return bad

    res = pc.run_thread_ranks([0] * k, body, pc._case_capacity(k, cases), timeout_s=30.0)
    assert res == [[]] * k, [r[:2] for r in res]


def test_thread_ranks_mask_the_stale_window_and_count_launches():
    k = 3
    big, small = Q.stale_window_case(k)
    ref = allreduce_q8x2_ref(small, "bf16")

    def body(comm):
        comm.write(big[comm.rank])
        comm.all_reduce(4096, "bf16", "twoshot", wire=WIRE)
        comm.write(small[comm.rank])
        comm.all_reduce(33, "bf16", "twoshot", wire=WIRE)
        out = comm.read(0, 33, "bf16")
        counts = []
        for algo, wire in (("twoshot", WIRE), ("twoshot", "fp8"), ("oneshot", None)):  # 128 blocks: no rank's slice is empty
            before = comm.launches
            comm.all_reduce(4096, "bf16", algo, wire=wire)
            counts.append(comm.launches - before)
        return out, counts

    for out, counts in pc.run_thread_ranks([0] * k, body, 4096 * 2, timeout_s=30.0):
        assert counts == [3, 3, 1]  # quantize, repack, unpack; quantize, sum, gather; the native reduce alone
        np.testing.assert_array_equal(out, ref)


def test_rank_checks_bounds_before_any_launch():
    from gpu_topology_on_k8s_amd._native import load

    cap = 64 * 4 + 16  # four blocks of bf16 and one vector more
    ranks = [load("_probe").PeerRank(0, r, 2, cap) for r in range(2)]
    try:
        devs, wins, outs = [0, 0], [r.window_ptr() for r in ranks], [r.out_ptr() for r in ranks]
        packs, pouts = [r.packed_ptr() for r in ranks], [r.packed_out_ptr() for r in ranks]
        ranks[0].open_peers(devs, wins, outs, packs)
        for call in (lambda: ranks[0].repack_q8(0, 1, 1.0), lambda: ranks[0].unpack_q8([(0, 1), (1, 2)], "bf16")):
            with pytest.raises(RuntimeError):
                call()
        with pytest.raises(ValueError):
            ranks[0].open_peers(devs, wins, outs, packs, [pouts[1], pouts[0]])
        with pytest.raises(ValueError):
            ranks[0].open_peers(devs, wins, outs, packs, [pouts[0], wins[1] + 16])
        with pytest.raises(ValueError):
            ranks[0].open_peers(devs, wins, outs, None, pouts)
        for r in ranks:
            r.open_peers(devs, wins, outs, packs, pouts)
        for call in (lambda: ranks[0].repack_q8(0, 5, 1.0), lambda: ranks[0].repack_q8(2, 1, 1.0),
                     lambda: ranks[0].unpack_q8([(0, 2), (2, 5)], "bf16"), lambda: ranks[0].unpack_q8([(0, 2), (2, 5)], "fp32"),
                     lambda: ranks[0].unpack_q8([(2, 1), (2, 4)], "fp32"), lambda: ranks[0].unpack_q8([(0, 4)], "bf16"),
                     lambda: ranks[0].unpack_q8([(0, 2), (2, 4)], "fp16")):
            with pytest.raises(ValueError):
                call()
        assert ranks[0].launches == 0
        # the whole capacity in blocks: the last whole block of an fp32 out ends where out ends
        x = bf16_round(np.linspace(-3, 3, 128).astype(np.float32))
        for r in ranks:
            r.write_host(x, 0)
            r.quantize(0, 4, 128, "bf16")
            r.synchronize()
        ranks[0].repack_q8(0, 3, 0.5)
        ranks[1].repack_q8(3, 4, 0.5)
        for r in ranks:
            r.synchronize()
        ranks[0].unpack_q8([(0, 3), (3, 4)], "fp32")
        got = ranks[0].read_host(0, 128 * 4).view(np.float32)
        np.testing.assert_array_equal(got, allreduce_q8x2_ref([x, x], "bf16", "fp32", 0.5))
        assert ranks[0].launches == 3
    finally:
        for r in ranks:
            r.release()


# -- 5. CLI -----------------------------------------------------------------------------------
def test_validate_cli_fp8x2_thread_ranks():
    p = subprocess.run([sys.executable, "-m", "gpu_topology_on_k8s_amd", "validate", "--backend", "peer", "--ranks", "thread", "--wire", WIRE,
                        "--devices", "0,0", "--max-bytes", "1048576"], capture_output=True, text=True, timeout=240, cwd=REPO)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    first, summary, points = lines[0], lines[-1], lines[1:-1]
    assert first["selftest"] is True and first["wrong"] == 0 and first["q8_wrong"] == 0 and first["q8x2_wrong"] == 0
    assert first["barriers_per_collective"] == [2]
    assert first["q8x2_collectives"] == 2 * len(pc.selftest_cases_q8x2(2)) and first["q8x2_launches"] > 0
    assert points and all(p["wire"] == WIRE and p["algo"] == "twoshot" and p["wrong"] == 0 for p in points)
    assert summary["wire"] == WIRE and summary["wrong"] == 0 and summary["selftest_wrong"] == 0
