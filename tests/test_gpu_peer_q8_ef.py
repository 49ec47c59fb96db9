"""GPU tests of error feedback on the K7 fp8 wire (csrc/probe/peer_q8.h: peer_q8_quantize_ef_kernel): the kernel
against the numpy rule (ops/peer_ref.py: q8_quantize_ef_ref), codes, exponents and residual bit for bit over
chained steps; the collectives of the peer communicator's device backend against the chained references, on
every rank, results and residuals; non-finite and huge values; the residual buffer's life; the self-test and
the CLI.

Members repeat device 0.  Inputs and references are made once on the host and left unchanged."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_peer_q8_cpu as Q
import test_peer_q8_ef_cpu as E
from gpu_topology_on_k8s_amd._native import load
from gpu_topology_on_k8s_amd.ops import probe
from gpu_topology_on_k8s_amd.ops.peer_ref import (Q8_BLOCK, allreduce_q8_ef_ref, allreduce_ref, bf16_round, bf16_to_f32, bits, q8_blocks,
                                                  q8_dequantize_ref, q8_quantize_ef_ref, q8_quantize_ref, q8_slices, reduce_scatter_q8_ef_ref)
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3
ELEM = {"bf16": 2, "fp32": 4}


def _wide(x, dtype):
    return bf16_to_f32(x) if dtype == "bf16" else x


def _residual_for(x, dtype, count, seed):
    """A residual for the count's whole blocks: random, up to 1/13 of its element's magnitude, and large past
    the count, where it must not be read."""
    n = q8_blocks(count) * Q8_BLOCK
    v = np.zeros(n, np.float32)
    v[:min(n, x.size)] = _wide(x, dtype)[:n]
    r = (np.random.default_rng(seed).uniform(-1, 1, n) * np.abs(v) / 13).astype(np.float32)
    r[count:] = np.float32(3.0e4)
    return r


def _assert_step(got, want, what):
    """Codes (the NaN code's sign bit masked), exponents and residual of one step, bit for bit."""
    (gc, ge, gr), (wc, we, wr) = got, want
    assert gc.dtype == np.uint8 and gc.shape == wc.shape and ge.shape == we.shape and gr.dtype == np.float32 and gr.shape == wr.shape
    assert ge.tolist() == we.tolist(), what
    nan = (wc & 0x7F) == 0x7F
    bad = np.flatnonzero(np.where(nan, (gc & 0x7F) != 0x7F, gc != wc))
    assert bad.size == 0, (what, "codes", bad.size, [(int(i), hex(gc[i]), hex(wc[i])) for i in bad[:8]])
    bad = np.flatnonzero(bits(gr) != bits(wr))
    assert bad.size == 0, (what, "residual", bad.size, [(int(i), hex(bits(gr)[i]), hex(bits(wr)[i])) for i in bad[:8]])


# -- 1. the kernel against the rule -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_feedback_kernel_matches_the_rule_over_chained_steps(dtype):
    """Crafted blocks and 65536 random values over 2^-43 .. 2^43; the array goes on past the count, so the
    window's tail is non-zero, and so is the residual's."""
    x = Q.as_input(np.concatenate([Q.crafted(dtype), Q.wide_random(65536, dtype)])[:-5], dtype)
    for count in (1, 31, 32, 33, x.size):
        r = _residual_for(x, dtype, count, seed=count)
        for step in range(STEPS):
            want = q8_quantize_ef_ref(x, dtype, r, count=count)
            got = probe.peer_q8_quantize(0, x, dtype, count, residual=r)
            assert len(got) == 3
            _assert_step(got, want, (dtype, count, step))
            assert not bits(got[2])[count:].any()
            r = want[2]
    # without a residual the call is what it was
    plain = probe.peer_q8_quantize(0, x, dtype, 33)
    assert len(plain) == 2 and np.array_equal(plain[0], q8_quantize_ref(x, dtype, count=33)[0])
    with pytest.raises(ValueError):
        probe.peer_q8_quantize(0, x, dtype, 33, residual=np.zeros(63, np.float32))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_feedback_kernel_runs_its_pass_loop_twice_with_a_ragged_last_pass(dtype):
    """A rank with one block per CU and a count just past grid x 256 x 4 vectors: every lane's first pass is
    full, a few lanes make a second one and most of its four vectors lie past the end.  The rank's partner
    packs nothing, so the sum of the two packed buffers is the rank's dequantised packing."""
    P = load("_probe")
    lanes = 16 // ELEM[dtype]
    cus = int(P.device_props(0)["cus"])
    grid = int(P.peer_reduce_grid(cus, 1, 2, 1 << 40))
    count = grid * 256 * 4 * lanes + 2 * Q8_BLOCK + 7
    nb = q8_blocks(count)
    assert int(P.peer_reduce_grid(cus, 1, 2, nb * Q8_BLOCK // lanes)) == grid  # the grid of this very call
    x = Q.as_input(Q.wide_random(nb * Q8_BLOCK, dtype, seed=11), dtype)
    r = _residual_for(x, dtype, count, seed=12)
    ranks = [P.PeerRank(0, i, 2, nb * Q8_BLOCK * ELEM[dtype], 1) for i in range(2)]
    try:
        for q in ranks:
            q.open_peers([0, 0], [a.window_ptr() for a in ranks], [a.out_ptr() for a in ranks], [a.packed_ptr() for a in ranks])
        me = ranks[0]
        me.write_host(x, 0)
        me.write_residual(r, 0)
        assert me.residual_bytes == 2 * me.capacity_bytes
        for step in range(STEPS):
            codes, exps, r = q8_quantize_ef_ref(x, dtype, r, count=count)
            me.quantize(0, nb, count, dtype, True)
            me.reduce_q8(0, nb, "fp32", 1.0)
            got = me.read_host(0, nb * Q8_BLOCK * 4).view(np.float32)
            want = allreduce_ref([q8_dequantize_ref(codes, exps), np.zeros(nb * Q8_BLOCK, np.float32)], "fp32")
            bad = np.flatnonzero(bits(got) != bits(want))
            assert bad.size == 0, (step, "values", bad.size, bad[:8].tolist())
            got_r = me.read_residual(0, nb * Q8_BLOCK)
            bad = np.flatnonzero(bits(got_r) != bits(r))
            assert bad.size == 0, (step, "residual", bad.size, bad[:8].tolist())
        assert me.launches == 2 * STEPS
    finally:
        for q in ranks:
            q.release()


# -- 2. thread ranks --------------------------------------------------------------------------------
COLLECTIVES = (("all_reduce", "oneshot", "fp8"), ("all_reduce", "twoshot", "fp8"), ("all_reduce", "twoshot", "fp8x2"),
               ("reduce_scatter", "oneshot", "fp8"))


def _finish(dqs, k, count, out, scale, op, wire):
    """What every rank holds (a list per rank) from the members' dequantised packings: the sum in member order,
    the scale, for fp8x2 the second packing, the rounding, and for a reduce-scatter the rank's piece."""
    acc = allreduce_ref(dqs, "fp32", "fp32", scale)
    if wire == "fp8x2":
        acc = q8_dequantize_ref(*q8_quantize_ref(acc, "fp32"))[:count]
    full = bf16_round(acc) if out == "bf16" else acc
    if op == "all_reduce":
        return [full] * k
    return [full[min(count, a * Q8_BLOCK):min(count, b * Q8_BLOCK)] for a, b in q8_slices(q8_blocks(count), k)]


@functools.lru_cache(maxsize=None)
def _chain(k, gi, count, dtype):
    """Three issues of k members' inputs with the residual carried from zero: per issue the inputs, the
    members' dequantised packings and their residuals afterwards.  The residual depends on the inputs alone,
    so the four collectives and both output types share one chain."""
    res = [np.zeros(q8_blocks(count) * Q8_BLOCK, np.float32) for _ in range(k)]
    steps = []
    for issue in range(STEPS):
        xs = [pc.case_input(gi, issue, p, count, dtype) for p in range(k)]
        packs = [q8_quantize_ef_ref(x, dtype, r) for x, r in zip(xs, res)]
        res = [p[2] for p in packs]
        steps.append((xs, [q8_dequantize_ref(p[0], p[1])[:count] for p in packs], res))
    return steps


def test_shared_chain_is_the_chained_reference():
    k, count = 3, 512 * 3 + 37
    for gi, (dtype, out, scale) in enumerate((("bf16", "bf16", 1.0), ("fp32", "fp32", 1.0), ("bf16", "fp32", 1.0 / 3))):
        res = [np.zeros(q8_blocks(count) * Q8_BLOCK, np.float32)] * k
        for xs, dqs, after in _chain(k, gi, count, dtype):
            for op, algo, wire in COLLECTIVES:
                if op == "all_reduce":
                    ref, new = allreduce_q8_ef_ref(xs, res, dtype, out, scale, wire=wire)
                    ref = [ref] * k
                else:
                    ref, new = reduce_scatter_q8_ef_ref(xs, res, dtype, out, scale)
                for a, b in zip(_finish(dqs, k, count, out, scale, op, wire), ref):
                    assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b))
                for a, b in zip(after, new):
                    assert np.array_equal(bits(a), bits(b))
            res = after


@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_thread_ranks_match_the_chained_reference_at_no_extra_cost(k):
    counts = pc.selftest_counts_q8(k)
    groups = [(count, dtype, out, scale) for count in counts
              for dtype, out, scale in (("bf16", "bf16", 1.0), ("fp32", "fp32", 1.0), ("bf16", "fp32", 1.0 / k))]
    plan = []
    for count, dtype, out, scale in groups:
        steps = _chain(k, counts.index(count) * 2 + (dtype == "fp32"), count, dtype)
        for op, algo, wire in COLLECTIVES:
            plan.append((op, algo, wire, count, dtype, out, scale,
                         [(xs, _finish(dqs, k, count, out, scale, op, wire), after) for xs, dqs, after in steps]))

    def issue(comm, op, algo, wire, count, dtype, out, scale, fed):
        b0, l0 = comm.barriers, comm.launches
        if op == "all_reduce":
            comm.all_reduce(count, dtype, algo, out, scale, wire=wire, error_feedback=fed)
            got = comm.read(0, count, out)
        else:
            got = comm.read(*comm.reduce_scatter(count, dtype, out, scale, wire=wire, error_feedback=fed), out)
        return got, comm.barriers - b0, comm.launches - l0

    def body(comm):
        bad, r = [], comm.rank
        for op, algo, wire, count, dtype, out, scale, steps in plan:
            what = (op, algo, wire, count, dtype, out)
            n = q8_blocks(count) * Q8_BLOCK
            comm.write(steps[0][0][r])
            _, plain_barriers, plain_launches = issue(comm, op, algo, wire, count, dtype, out, scale, False)
            comm.reset_error_feedback()
            for i, (xs, refs, after) in enumerate(steps):
                comm.write(xs[r])
                got, barriers, launches = issue(comm, op, algo, wire, count, dtype, out, scale, True)
                if (barriers, launches) != (plain_barriers, plain_launches) or barriers != 2:
                    bad.append(("cost", what, i, barriers, launches, plain_launches))
                if got.dtype != refs[r].dtype or got.shape != refs[r].shape or not np.array_equal(bits(got), bits(refs[r])):
                    bad.append(("bits", what, i))
                if not np.array_equal(bits(comm.residual(0, n)), bits(after[r])):
                    bad.append(("residual", what, i))
        return bad

    cap = max(q8_blocks(c) * Q8_BLOCK * 4 for c in counts)
    res = pc.run_thread_ranks([0] * k, body, cap, timeout_s=60.0)
    assert res == [[]] * k, [r[:3] for r in res]


# -- 3. non-finite and huge values ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_feedback_kernel_leaves_no_residual_at_non_finite_elements(dtype):
    x, at = E.special_case(dtype)
    v = _wide(x, dtype)
    r0 = (np.random.default_rng(8).uniform(-1, 1, v.size) * np.abs(v) / 13).astype(np.float32)
    r0[at] = 0
    want1 = q8_quantize_ef_ref(x, dtype, r0)
    got1 = probe.peer_q8_quantize(0, x, dtype, residual=r0)
    _assert_step(got1, want1, (dtype, "first step"))
    assert want1[1][1:5].tolist() == [120] * 4 and not bits(got1[2])[at].any()
    want2 = q8_quantize_ef_ref(x, dtype, want1[2])
    got2 = probe.peer_q8_quantize(0, x, dtype, residual=got1[2])
    _assert_step(got2, want2, (dtype, "second step"))
    plain = probe.peer_q8_quantize(0, x, dtype)
    assert np.array_equal(got2[0][at[3:]], plain[0][at[3:]]) and np.all((got2[0][at[:3]] & 0x7F) == 0x7F)
    assert got2[1][1:5].tolist() == plain[1][1:5].tolist()
    assert not bits(got2[2])[at].any() and np.isfinite(got2[2]).all()


# -- 4. the residual buffer's life ------------------------------------------------------------------
def test_residual_is_allocated_on_demand_checked_and_freed():
    P = load("_probe")
    cap = 64 * 4 + 16  # four blocks of bf16 and one vector more
    ranks = [P.PeerRank(0, r, 2, cap) for r in range(2)]
    try:
        for r in ranks:
            r.open_peers([0, 0], [a.window_ptr() for a in ranks], [a.out_ptr() for a in ranks], [a.packed_ptr() for a in ranks])
        me = ranks[0]
        x = Q.as_input(Q.wide_random(128, "bf16", seed=4), "bf16")
        me.write_host(x, 0)
        assert me.residual_bytes == 0 and not me.read_residual(0, cap // 2).any()
        me.reset_residual()  # nothing to reset: no allocation, no launch
        me.quantize(0, 4, 128, "bf16")
        assert me.residual_bytes == 0 and me.launches == 1
        for call in (lambda: me.quantize(0, 5, 160, "bf16", True), lambda: me.quantize(0, 3, 96, "fp32", True),
                     lambda: me.quantize(2, 1, 32, "bf16", True), lambda: me.quantize(0, 1, 32, "fp16", True),
                     lambda: me.read_residual(0, cap // 2 + 1), lambda: me.read_residual(cap // 2 + 1, 0),
                     lambda: me.write_residual(np.zeros(cap // 2 + 1, np.float32), 0)):
            with pytest.raises(ValueError):
                call()
        assert me.residual_bytes == 0 and me.launches == 1
        me.quantize(0, 4, 128, "bf16", True)
        assert me.residual_bytes == 2 * cap and me.launches == 2 and ranks[1].residual_bytes == 0
        want = q8_quantize_ef_ref(x, "bf16", np.zeros(128, np.float32))[2]
        assert np.array_equal(bits(me.read_residual(0, 128)), bits(want)) and np.count_nonzero(want) > 0
        assert not me.read_residual(128, cap // 2 - 128).any()  # zeroed when it was made
        # blocks outside [b0, b1) keep their residual, and what lies past the count in the last block comes back zero
        me.write_residual(np.full(cap // 2, 7.0, np.float32), 0)
        me.quantize(1, 3, 80, "bf16", True)
        got = me.read_residual(0, cap // 2)
        assert np.all(got[:32] == 7.0) and np.all(got[96:] == 7.0) and not bits(got[80:96]).any()
        np.testing.assert_array_equal(got[32:96], q8_quantize_ef_ref(x[32:96], "bf16", np.full(64, 7.0, np.float32), count=48)[2])
        me.reset_residual()
        assert not bits(me.read_residual(0, cap // 2)).any() and me.residual_bytes == 2 * cap
    finally:
        for r in ranks:
            r.release()
    with pytest.raises(RuntimeError):
        ranks[0].read_residual(0, 1)
    with pytest.raises(RuntimeError):
        ranks[0].reset_residual()


def test_comm_reports_the_residual_and_resets_it_on_a_mismatch():
    def body(comm):
        assert comm.residual_bytes == 0
        with pytest.raises(ValueError, match="error_feedback"):
            comm.all_reduce(100, "bf16", "oneshot", error_feedback=True)
        assert comm.residual_bytes == 0 and comm.barriers == 0 and comm.launches == 0
        comm.write(pc.case_input(0, 0, comm.rank, 100, "bf16"))
        comm.all_reduce(100, "bf16", "oneshot", wire="fp8", error_feedback=True)
        held = np.count_nonzero(comm.residual(0, 128))
        assert comm.residual_bytes == 2 * comm.capacity_bytes and held > 0
        with pytest.raises(pc.PeerCommMismatch):
            comm.all_reduce(100, "bf16", "oneshot", wire="fp8", error_feedback=comm.rank == 0)
        return held, np.count_nonzero(comm.residual(0, 128))

    res = pc.run_thread_ranks([0, 0], body, 4096, timeout_s=30.0)
    assert res[0][1] == 0 and res[1][1] == res[1][0]


# -- 5. the self-test and the CLI -------------------------------------------------------------------
def test_selftest_with_error_feedback():
    st = pc.selftest(devices=[0, 0, 0], error_feedback=True)
    assert st["wrong"] == 0 and st["q8_wrong"] == 0 and st["ef_wrong"] == 0 and st["barriers_per_collective"] == [2]
    assert st["ef_cases"] == len(pc.selftest_cases_ef(3)) and st["ef_collectives"] == 3 * st["ef_cases"] and st["ef_launches"] > 0
    assert "ef_cases" not in pc.selftest(devices=[0, 0], counts=[33])


def _validate(*extra):
    return subprocess.run([sys.executable, "-m", "gpu_topology_on_k8s_amd", "validate", "--backend", "peer", "--ranks", "thread", *extra,
                           "--devices", "0,0,0", "--dtype", "bf16", "--min-bytes", "4096", "--max-bytes", "65536"],
                          capture_output=True, text=True, timeout=240, cwd=REPO)


def test_validate_cli_error_feedback():
    p = _validate("--wire", "fp8", "--error-feedback")
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    first, summary = lines[0], lines[-1]
    assert first["selftest"] is True and first["ef_wrong"] == 0 and first["ef_collectives"] == 3 * len(pc.selftest_cases_ef(3))
    assert summary["wrong"] == 0 and summary["selftest_wrong"] == 0
    p = _validate("--wire", "native", "--error-feedback")
    assert p.returncode != 0 and "--error-feedback" in p.stderr and not p.stdout.strip()
