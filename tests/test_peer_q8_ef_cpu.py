"""CPU tests of error feedback on the K7 fp8 wire: the rule (ops/peer_ref.py: q8_quantize_ef_ref and the chained
collective references), its telescoping sum against the plain wire's drift, non-finite values, the count's
mask, the peer communicator's host backend (bits of results and residuals, the race detector, launch and
barrier counts, mismatched calls, reset) and the CLI's ``--error-feedback``.

Inputs come from tests/test_peer_q8_cpu.py and are read-only."""
import json

import numpy as np
import pytest

import test_peer_q8_cpu as Q
from gpu_topology_on_k8s_amd.ops.peer_ref import (Q8_BLOCK, allreduce_q8_ef_ref, allreduce_q8_ref, bf16_round, bf16_to_f32, bits, q8_blocks,
                                                  q8_dequantize_ref, q8_quantize_ef_ref, q8_quantize_ref, reduce_scatter_q8_ef_ref)
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

PAIRS = (("bf16", "bf16", 1.0), ("fp32", "fp32", 1.0), ("bf16", "fp32", None))  # the wide pair is scaled by 1 / k
STEPS = 16


def _wide(x, dtype):
    return bf16_to_f32(x) if dtype == "bf16" else np.asarray(x, np.float32)


def _blocks_amax(a):
    """|a| padded with zeros to whole blocks: every element's block amax, float64."""
    n = q8_blocks(a.size) * Q8_BLOCK
    full = np.zeros(n)
    full[:a.size] = np.abs(a)
    return np.repeat(full.reshape(-1, Q8_BLOCK).max(axis=1), Q8_BLOCK)


# -- 1. a zero residual is the plain rule, and the new residual is an exact difference -----------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_zero_residual_is_the_plain_rule_and_the_subtraction_is_exact(dtype):
    x = np.concatenate([Q.crafted(dtype), Q.wide_random(8192, dtype)])
    xin = Q.as_input(x, dtype)
    codes, exps, res = q8_quantize_ef_ref(xin, dtype, np.zeros(x.size, np.float32))
    want_c, want_e = q8_quantize_ref(xin, dtype)
    np.testing.assert_array_equal(codes, want_c)
    np.testing.assert_array_equal(exps, want_e)
    assert res.dtype == np.float32 and res.shape == x.shape
    dq = q8_dequantize_ref(codes, exps)
    assert np.all(np.isfinite(dq))
    np.testing.assert_array_equal(res.astype(np.float64), x.astype(np.float64) - dq.astype(np.float64))
    # and with a residual to add: y is one fp32 add, the difference again exact
    r0 = (np.random.default_rng(3).uniform(-1, 1, x.size) * np.abs(x) / 13).astype(np.float32)
    codes, exps, res = q8_quantize_ef_ref(xin, dtype, r0)
    y = np.where(r0 == 0, x, (x + r0).astype(np.float32))
    np.testing.assert_array_equal(codes, q8_quantize_ref(y, "fp32")[0])
    dq = q8_dequantize_ref(codes, exps)
    np.testing.assert_array_equal(res.astype(np.float64), y.astype(np.float64) - dq.astype(np.float64))
    with pytest.raises(ValueError, match="residual"):
        q8_quantize_ef_ref(xin, dtype, np.zeros(x.size - 1, np.float32))
    with pytest.raises(ValueError, match="residual"):
        q8_quantize_ef_ref(xin, dtype, np.zeros(x.size, np.float64))


# -- 2. telescoping -----------------------------------------------------------------------------------
def _gradient(rng, n):
    g = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 4, n))).astype(np.float32)
    return bf16_round(g)


def _feedback_run(inputs, count):
    """The inputs of the steps (bf16 patterns, ``count`` elements of each used) through the rule with the
    residual carried: (sum of dq - sum of g + last residual, the adds' rounding allowance, last residual, the
    blocks' largest input amax), float64 per element of the whole blocks."""
    n = q8_blocks(count) * Q8_BLOCK
    r = np.zeros(n, np.float32)
    s_dq, s_g, allow, amax = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for x in inputs:
        g = np.zeros(n, np.float32)
        g[:count] = bf16_to_f32(x[:count])
        y = np.where(r == 0, g, (g + r).astype(np.float32))
        codes, exps, r = q8_quantize_ef_ref(x, "bf16", r, count=count)
        s_dq += q8_dequantize_ref(codes, exps)
        s_g += g
        allow += 2.0 ** -24 * np.abs(y.astype(np.float64))  # half an ulp of the one add
        amax = np.maximum(amax, _blocks_amax(g))
    return s_dq - s_g + r, allow, r.astype(np.float64), amax


@pytest.mark.parametrize("count", [4133, 33])
def test_feedback_telescopes_where_the_plain_wire_drifts(count):
    x = _gradient(np.random.default_rng(0), 4133)
    off, allow, r, amax = _feedback_run([x] * STEPS, count)
    print("telescoping worst ratio", np.max(np.abs(off)[allow > 0] / allow[allow > 0]), "residual worst ratio", np.max(np.abs(r)[amax > 0] / (amax / 13)[amax > 0]))
    assert np.all(np.abs(off) <= allow)
    assert np.all(np.abs(r) <= amax / 13)
    # the control: the same input on the plain wire is rounded the same way every time
    g = bf16_to_f32(x[:count]).astype(np.float64)
    dq = q8_dequantize_ref(*q8_quantize_ref(x, "bf16", count=count))[:count].astype(np.float64)
    over = np.mean(np.abs(STEPS * (dq - g)) > amax[:count] / 13)
    print("plain wire over the bound", over)
    assert over >= 0.05


def test_feedback_telescopes_on_fresh_inputs():
    rng = np.random.default_rng(0)
    off, allow, r, amax = _feedback_run([_gradient(rng, 4133) for _ in range(STEPS)], 4133)
    assert np.all(np.abs(off) <= allow)
    assert np.all(np.abs(r) <= amax / 13)


# -- 3. non-finite inputs ------------------------------------------------------------------------------
def special_case(dtype):
    """Five blocks of finite values with one special each (NaN, +Inf, -Inf, 248 * 2^120, its negative), then a
    plain block: (input array, the specials' indices)."""
    v = Q.wide_random(6 * Q8_BLOCK, dtype, seed=5).copy()
    big = np.float32(248.0) * np.float32(2.0 ** 120)  # bf16 0x7F78
    at = [3, 32 + 17, 64 + 31, 96 + 0, 128 + 9]
    v[at] = [np.nan, np.inf, -np.inf, big, -big]
    x = Q.as_input(v, dtype)
    if dtype == "bf16":
        assert x[96] == 0x7F78
    return x, np.array(at)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_non_finite_elements_leave_no_residual(dtype):
    x, at = special_case(dtype)
    v = _wide(x, dtype)
    r0 = (np.random.default_rng(8).uniform(-1, 1, v.size) * np.abs(v) / 13).astype(np.float32)
    r0[at] = 0  # the huge values stay exactly on 248 * 2^120
    codes, exps, r1 = q8_quantize_ef_ref(x, dtype, r0)
    assert exps[1:5].tolist() == [120] * 4 and exps[0] < 120
    dq = q8_dequantize_ref(codes, exps)
    assert np.isnan(dq[at[:3]]).all() and np.isinf(dq[at[3:]]).all()
    assert not bits(r1)[at].any()  # +0, not a NaN, an Inf or -0
    rest = np.setdiff1d(np.arange(v.size), at)
    y = np.where(r0 == 0, v, (v + r0).astype(np.float32))
    np.testing.assert_array_equal(r1[rest].astype(np.float64), y[rest].astype(np.float64) - dq[rest].astype(np.float64))
    assert np.count_nonzero(r1[32:160]) > 100  # under e = 120 the neighbours' codes are zero: their values wait in the residual
    # one step later the specials pack as the plain rule packs them, and their blocks' exponents are the plain rule's
    codes2, exps2, r2 = q8_quantize_ef_ref(x, dtype, r1)
    want_c, want_e = q8_quantize_ref(x, dtype)
    assert np.array_equal(codes2[at[3:]], want_c[at[3:]]) and np.all((codes2[at[:3]] & 0x7F) == 0x7F) and np.all((want_c[at[:3]] & 0x7F) == 0x7F)
    assert exps2[1:5].tolist() == want_e[1:5].tolist()
    assert not bits(r2)[at].any() and np.isfinite(r2).all()


# -- 4. the count's mask -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_residual_past_the_count_is_not_read_and_comes_back_zero(dtype):
    x = Q.as_input(Q.wide_random(64, dtype, seed=2), dtype)
    count = 40
    r0 = np.full(64, 3.0e4, np.float32)
    r0[:count] = np.float32(2.0 ** -30)
    clean = r0.copy()
    clean[count:] = 0
    got = q8_quantize_ef_ref(x, dtype, r0, count=count)
    want = q8_quantize_ef_ref(x, dtype, clean, count=count)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    assert not got[0][count:].any() and not bits(got[2])[count:].any()
    assert np.count_nonzero(q8_quantize_ef_ref(x, dtype, r0)[0][count:]) > 0  # with the whole array as data it does count


def test_blocks_outside_the_range_keep_their_residual():
    cap = 4096
    store, fabric = pc.MemoryStore(), pc.HostFabric(2, cap)
    comm = pc.PeerComm(0, 2, 0, store, cap, backend="host", fabric=fabric)
    x = Q.as_input(Q.wide_random(160, "bf16", seed=4), "bf16")
    comm.write(x)
    fabric.residual[0] = np.full(cap // 2, 7.0, np.float32)
    comm._b.quantize(1, 3, 80, "bf16", True)
    res = fabric.residual[0]
    assert np.all(res[:32] == 7.0) and np.all(res[96:] == 7.0)
    assert not bits(res[80:96]).any()
    seven = np.full(64, 7.0, np.float32)
    np.testing.assert_array_equal(res[32:96], q8_quantize_ef_ref(x[32:96], "bf16", seven, count=48)[2])


# -- 5. the host backend -------------------------------------------------------------------------------
def _collectives(k):
    """(op, algo, wire) x the dtype pairs at every count."""
    return [(op, algo, wire, dtype, out, 1.0 / k if scale is None else scale, count)
            for count in Q._counts(k)
            for dtype, out, scale in PAIRS
            for op, algo, wire in (("all_reduce", "oneshot", "fp8"), ("all_reduce", "twoshot", "fp8"), ("all_reduce", "twoshot", "fp8x2"),
                                   ("reduce_scatter", "oneshot", "fp8"))]


def _inputs(ci, issue, k, count, dtype):
    return [Q.as_input(Q.wide_random(count, dtype, seed=1000 * ci + 10 * issue + m) * np.float32(2.0 ** -20), dtype) for m in range(k)]


def _issue(comm, case, fed):
    op, algo, wire, dtype, out, scale, count = case
    if op == "all_reduce":
        comm.all_reduce(count, dtype, algo, out, scale, wire=wire, error_feedback=fed)
        return comm.read(0, count, out)
    first, n = comm.reduce_scatter(count, dtype, out, scale, wire=wire, error_feedback=fed)
    return comm.read(first, n, out)


def _fed_sequence(comm):
    """Every collective three times with the residual carried, reset between collectives: what differs from
    the chained reference, and the barriers and launches the sequence took."""
    k, bad = comm.world, []
    for ci, case in enumerate(_collectives(k)):
        op, algo, wire, dtype, out, scale, count = case
        comm.reset_error_feedback()
        n = q8_blocks(count) * Q8_BLOCK
        res = [np.zeros(n, np.float32) for _ in range(k)]
        for issue in range(3):
            xs = _inputs(ci, issue, k, count, dtype)
            comm.write(xs[comm.rank])
            got = _issue(comm, case, True)
            if op == "all_reduce":
                ref, res = allreduce_q8_ef_ref(xs, res, dtype, out, scale, wire=wire)
            else:
                pieces, res = reduce_scatter_q8_ef_ref(xs, res, dtype, out, scale)
                ref = pieces[comm.rank]
            if got.dtype != ref.dtype or got.shape != ref.shape or not np.array_equal(bits(got), bits(ref)):
                bad.append(("bits", case, issue))
            if not np.array_equal(bits(comm.residual(0, n)), bits(res[comm.rank])):
                bad.append(("residual", case, issue))
        if issue == 2 and not any(np.count_nonzero(r) for r in res):
            bad.append(("no residual at all", case))
    return bad, comm.barriers


def _plain_sequence(comm):
    k = comm.world
    for ci, case in enumerate(_collectives(k)):
        for issue in range(3):
            comm.write(_inputs(ci, issue, k, case[6], case[3])[comm.rank])
            _issue(comm, case, False)
    return [], comm.barriers


@pytest.mark.parametrize("k", [2, 3, 5])
def test_host_backend_matches_the_chained_reference_at_no_extra_cost(k):
    fabric, results, errors = Q._run_threads(k, _fed_sequence)
    assert not errors, errors
    for r in range(k):
        assert not results[r][0], results[r][0][:3]
    assert fabric.conflicts() == []
    touched = [a for a in fabric.log if a[2] == "residual"]
    assert touched and all(a[0] == a[1] for a in touched)  # the owner alone
    assert {a[5] for a in touched} == {"r", "w"}
    plain, plain_results, errors = Q._run_threads(k, _plain_sequence)
    assert not errors, errors
    assert fabric.launches == plain.launches
    assert [results[r][1] for r in range(k)] == [plain_results[r][1] for r in range(k)] == [2 * 3 * len(_collectives(k))] * k
    assert not any(a[2] == "residual" for a in plain.log) and plain.residual == [None] * k


def test_the_helpers_chain_as_the_references_do():
    """``run_case`` with ``residuals`` and ``selftest_cases_ef``: what the self-test and the GPU tests are built on."""
    k = 3
    cases = pc.selftest_cases_ef(k, [33, 512 * k + 37])
    assert all(c["ef"] is True and c["wire"] in ("fp8", "fp8x2") for c in cases) and {c["wire"] for c in cases} == {"fp8", "fp8x2"}
    assert len(cases) == 2 * (9 + 3)

    def body(comm):
        bad = []
        for ci, case in enumerate(cases):
            comm.reset_error_feedback()
            res = []
            for issue in range(3):
                xs = [pc.case_input(ci, issue, p, case["count"], case["dtype"]) for p in range(k)]
                got, ref = pc.run_case(comm, case, xs, res)
                n = q8_blocks(case["count"]) * Q8_BLOCK
                if not np.array_equal(bits(got), bits(ref)) or not np.array_equal(bits(comm.residual(0, n)), bits(res[comm.rank])):
                    bad.append((case, issue))
        return bad

    fabric, results, errors = Q._run_threads(k, body)
    assert not errors, errors
    assert all(not results[r] for r in range(k)), results
    assert fabric.conflicts() == []


# -- 6. arguments and state ----------------------------------------------------------------------------
def test_feedback_on_the_native_wire_is_refused_before_any_barrier():
    store, fabric = pc.MemoryStore(), pc.HostFabric(2, 4096)
    comm = pc.PeerComm(0, 2, 0, store, 4096, backend="host", fabric=fabric)
    for wire in (None, "native"):
        with pytest.raises(ValueError, match="error_feedback"):
            comm.all_reduce(64, "bf16", "oneshot", wire=wire, error_feedback=True)
        with pytest.raises(ValueError, match="error_feedback"):
            comm.reduce_scatter(64, "bf16", wire=wire, error_feedback=True)
    assert comm.barriers == 0 and fabric.launches == 0 and store.num_keys() == 0
    assert comm.residual_bytes == 0 and fabric.residual == [None, None]
    assert not comm.residual(0, 64).any()
    with pytest.raises(ValueError):
        comm.residual(0, 4096 // 2 + 1)


def test_feedback_mismatch_raises_everywhere_and_resets_the_residual():
    seen = {}

    def body(comm):
        comm.write(pc.case_input(0, 0, comm.rank, 100, "bf16"))
        comm.all_reduce(100, "bf16", "oneshot", wire="fp8", error_feedback=True)
        seen[comm.rank] = np.count_nonzero(comm.residual(0, 128))
        comm.barrier()
        try:
            comm.all_reduce(100, "bf16", "oneshot", wire="fp8", error_feedback=comm.rank == 0)
        finally:
            seen[comm.rank] = (seen[comm.rank], comm._b.f.residual[comm.rank].copy())

    fabric, _, errors = Q._run_threads(2, body)
    assert sorted(errors) == [0, 1] and all(isinstance(e, pc.PeerCommMismatch) for e in errors.values()), errors
    assert '"ef": true' in str(errors[1])
    assert seen[0][0] > 0 and seen[1][0] > 0
    assert not bits(seen[0][1]).any()      # the feedback rank's: reset before the exception left
    assert np.count_nonzero(seen[1][1]) == seen[1][0]  # the other's: a call without feedback touches nothing
    assert fabric.conflicts() == []


def test_reset_and_calls_without_feedback_between_feedback_calls():
    k, count = 3, 512 * 3 + 37
    n = q8_blocks(count) * Q8_BLOCK
    xs = [[pc.case_input(1, issue, p, count, "bf16") for p in range(k)] for issue in range(3)]

    def body(comm):
        out = {}
        comm.write(xs[0][comm.rank])
        comm.all_reduce(count, "bf16", "twoshot", wire="fp8", error_feedback=True)
        out["r1"] = comm.residual(0, n)
        comm.write(xs[1][comm.rank])
        comm.all_reduce(count, "bf16", "twoshot", wire="fp8")
        out["plain"], out["r1_after"] = comm.read(0, count, "bf16"), comm.residual(0, n)
        comm.write(xs[2][comm.rank])
        comm.all_reduce(count, "bf16", "twoshot", wire="fp8", error_feedback=True)
        out["fed"], out["r2"] = comm.read(0, count, "bf16"), comm.residual(0, n)
        assert comm.residual_bytes == 2 * comm.capacity_bytes
        comm.reset_error_feedback()
        out["r3"] = comm.residual(0, n)
        return out

    fabric, results, errors = Q._run_threads(k, body)
    assert not errors, errors
    zero = [np.zeros(n, np.float32)] * k
    _, r1 = allreduce_q8_ef_ref(xs[0], zero, "bf16")
    fed, r2 = allreduce_q8_ef_ref(xs[2], r1, "bf16")
    for r in range(k):
        o = results[r]
        assert np.array_equal(bits(o["r1"]), bits(r1[r])) and np.count_nonzero(o["r1"]) > 0
        assert np.array_equal(bits(o["r1_after"]), bits(o["r1"]))
        np.testing.assert_array_equal(o["plain"], allreduce_q8_ref(xs[1], "bf16"))
        np.testing.assert_array_equal(o["fed"], fed)
        assert np.array_equal(bits(o["r2"]), bits(r2[r]))
        assert not bits(o["r3"]).any()
    assert fabric.conflicts() == []


class _Spy(pc.PeerComm):
    def _enter(self, desc):
        self.descs = getattr(self, "descs", []) + [dict(desc)]
        super()._enter(desc)


def test_descriptor_carries_ef_only_when_feedback_is_set():
    def body(comm):
        comm.write(pc.case_input(0, 0, comm.rank, 64, "bf16"))
        comm.all_reduce(64, "bf16", "twoshot", wire="fp8")
        comm.all_reduce(64, "bf16", "twoshot", wire="fp8x2", error_feedback=True)
        comm.reduce_scatter(64, "bf16", wire="fp8", error_feedback=True)
        comm.reduce_scatter(64, "bf16")
        return comm.descs

    _, results, errors = Q._run_threads(2, body, comm_cls=_Spy)
    assert not errors, errors
    plain, fed2, fed, native = results[0]
    assert "ef" not in plain and "ef" not in native
    assert fed2["ef"] is True and fed["ef"] is True
    # a call without feedback publishes the bytes it always did
    assert json.dumps(plain, sort_keys=True) == json.dumps({"op": "all_reduce", "count": 64, "dtype": "bf16", "out_dtype": "bf16",
                                                            "algo": "twoshot", "scale": 1.0, "wire": "fp8"}, sort_keys=True)


# -- 7. CLI --------------------------------------------------------------------------------------------
def test_validate_error_feedback_option():
    common = ("--devices", "0,0", "--resolve-only", "--cpu-bind", "off", "--max-bytes", "1048576")
    for wire in ("fp8", "fp8x2"):
        p = Q._gtk("validate", "--backend", "peer", "--ranks", "thread", "--wire", wire, "--error-feedback", *common)
        assert p.returncode == 0, p.stderr
    p = Q._gtk("validate", "--backend", "peer", "--ranks", "thread", "--wire", "native", "--error-feedback", *common)
    assert p.returncode == 2 and "--error-feedback" in p.stderr and "usage" not in p.stdout
    p = Q._gtk("validate", "--backend", "peer", "--ranks", "thread", "--error-feedback", *common)
    assert p.returncode == 2
    assert Q._gtk("validate", "--backend", "peer", "--wire", "fp8", "--error-feedback", *common).returncode == 2  # the driver's ranks have none


def test_parked_bytes_counts_the_residual():
    class Rank:
        capacity_bytes, packed_bytes, residual_bytes = 1024, 272, 2048

    before = pc.parked_bytes()
    with pc._PARKED_LOCK:
        pc._PARKED.append(Rank())
    try:
        assert pc.parked_bytes() - before == 3 * 1024 + 2 * 272 + 2048
    finally:
        with pc._PARKED_LOCK:
            pc._PARKED.pop()
