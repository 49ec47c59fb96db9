"""CPU tests of the K7 fp8x2 wire, the two-shot all-reduce whose gather phase is packed too: its reference
(ops/peer_ref.py: allreduce_q8x2_ref) against the three-step rule and its error bound, the wire through the
peer communicator's host backend (bits, two barriers, launches, the race detector on the second packed
buffer and on a mutant that does without it, error paths), the CLI's ``--wire fp8x2``, and the register
budget of the two kernels it adds to csrc/probe/peer_q8.h."""
import os
import shutil
import sys

import numpy as np
import pytest

import test_peer_q8_cpu as Q
from gpu_topology_on_k8s_amd.ops.peer_ref import (Q8_BLOCK, allreduce_q8_ref, allreduce_q8x2_ref, bf16_round, bf16_to_f32, q8_blocks,
                                                  q8_dequantize_ref, q8_quantize_ref)
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = (("bf16", "bf16"), ("fp32", "fp32"), ("bf16", "fp32"))
WIRE = "fp8x2"


def _scale(dtype, out, k):
    return 1.0 / k if dtype != out else 1.0


def _normal(k, count, dtype):
    return [pc.case_input(0, 0, m, count, dtype) for m in range(k)]


def integer_inputs(k, count, dtype):
    """Integers in [-8, 7] for every member: exact on the first packing, and their sums over 16 members
    need more than the 4 bits the second packing keeps."""
    xs = [np.random.default_rng([11, m]).integers(-8, 8, count).astype(np.float32) for m in range(k)]
    return [Q.as_input(x, dtype) for x in xs]


# -- 1. the reference -------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 8, 16])
@pytest.mark.parametrize("pair", PAIRS)
def test_reference_is_the_three_step_rule(pair, k):
    dtype, out = pair
    scale = _scale(dtype, out, k)
    for count in (1, 33, 512 * k + 37):
        for xs in (_normal(k, count, dtype),
                   [Q.as_input(Q.wide_random(count, dtype, seed=m + 1) * np.float32(2.0 ** -20), dtype) for m in range(k)]):
            s = allreduce_q8_ref(xs, dtype, "fp32", scale)
            assert s.dtype == np.float32
            back = q8_dequantize_ref(*q8_quantize_ref(s, "fp32"))[:count]
            got = allreduce_q8x2_ref(xs, dtype, out, scale)
            assert got.shape == (count,) and got.dtype == (np.uint16 if out == "bf16" else np.float32)
            # the cast to the output type is exact
            np.testing.assert_array_equal((bf16_to_f32(got) if out == "bf16" else got).view(np.uint32), back.view(np.uint32))


@pytest.mark.parametrize("k", [2, 3, 8, 16])
def test_bf16_and_fp32_outputs_hold_the_same_values(k):
    xs = _normal(k, 512 * k + 37, "bf16")
    for scale in (1.0, 1.0 / k):
        narrow, wide = allreduce_q8x2_ref(xs, "bf16", "bf16", scale), allreduce_q8x2_ref(xs, "bf16", "fp32", scale)
        np.testing.assert_array_equal(bf16_to_f32(narrow).view(np.uint32), wide.view(np.uint32))


@pytest.mark.parametrize("k", [2, 3, 8, 16])
@pytest.mark.parametrize("pair", PAIRS)
def test_second_rounding_stays_within_amax_over_14(pair, k):
    """Per element against the fp32 sum of the fp8 wire: at most amax / 14 of the element's block of that sum
    (2^(e+4) with amax * 2^-e > 224; N(0, 1) sums stay far from the exponent's clamp)."""
    dtype, out = pair
    count = 512 * k + 37
    xs = _normal(k, count, dtype)
    s = allreduce_q8_ref(xs, dtype, "fp32", _scale(dtype, out, k)).astype(np.float64)
    got = allreduce_q8x2_ref(xs, dtype, "fp32", _scale(dtype, out, k)).astype(np.float64)
    full = np.zeros(q8_blocks(count) * Q8_BLOCK)
    full[:count] = np.abs(s)
    amax = np.repeat(full.reshape(-1, Q8_BLOCK).max(axis=1), Q8_BLOCK)[:count]
    assert np.all(np.abs(got - s) <= amax / 14)
    assert np.any(got != s)


@pytest.mark.parametrize("pair", PAIRS)
def test_integer_sums_show_the_second_rounding(pair):
    dtype, out = pair
    k, count = 16, 512 * 16 + 37
    xs = integer_inputs(k, count, dtype)
    once = allreduce_q8_ref(xs, dtype, out, 1.0)
    exact = sum(x.astype(np.float32) if dtype == "fp32" else bf16_to_f32(x) for x in xs)
    np.testing.assert_array_equal(bf16_to_f32(once) if out == "bf16" else once, exact)  # one packing keeps the integers
    twice = allreduce_q8x2_ref(xs, dtype, out, 1.0)
    assert np.count_nonzero(pc._bits(twice) != pc._bits(once)) > 0
    back = q8_dequantize_ref(*q8_quantize_ref(exact, "fp32"))[:count]
    np.testing.assert_array_equal(bf16_to_f32(twice) if out == "bf16" else twice, back)
    # ties go to the even code: under e = -2 (amax in (56, 112]) the quantum of [64, 128) is 8, so 68 -> 64 and 76 -> 80
    codes, exps = q8_quantize_ref(np.array([112.0, 68.0, 76.0, -68.0], np.float32), "fp32")
    assert exps.tolist() == [-2] and q8_dequantize_ref(codes, exps)[:4].tolist() == [112.0, 64.0, 80.0, -64.0]


# -- 2. the protocol on the host backend ------------------------------------------------------
def _sequence(comm):
    """Every fp8x2 case, each issued twice in a row with different inputs."""
    bad, n = [], 0
    for ci, case in enumerate(pc.selftest_cases_q8x2(comm.world, Q._counts(comm.world))):
        for issue in range(2):
            xs = [pc.case_input(ci, issue, p, case["count"], case["dtype"]) for p in range(comm.world)]
            before = comm.barriers
            got, ref = pc.run_case(comm, case, xs)
            n += 1
            if comm.barriers - before != 2:
                bad.append(("barriers", case, comm.barriers - before))
            want = allreduce_q8x2_ref(xs, case["dtype"], case["out_dtype"], case["scale"])
            if got.dtype != want.dtype or got.shape != want.shape or not np.array_equal(pc._bits(got), pc._bits(want)):
                bad.append(("bits", case, issue))
            if not np.array_equal(pc._bits(ref), pc._bits(want)):
                bad.append(("run_case's reference", case, issue))
    return n, bad


@pytest.mark.parametrize("k", [2, 3, 5])
def test_fp8x2_protocol_is_exact_with_two_barriers_and_no_conflict(k):
    cases = pc.selftest_cases_q8x2(k, Q._counts(k))
    assert len(cases) == 6 * 3
    fabric, results, errors = Q._run_threads(k, _sequence)
    assert not errors, errors
    for r in range(k):
        n, bad = results[r]
        assert n == 2 * len(cases) and not bad, bad[:3]
    assert fabric.launches <= 3 * k * 2 * len(cases)
    assert fabric.conflicts() == []
    log = fabric.log
    assert any(a[2] == "packed_out" and a[5] == "r" and a[0] != a[1] for a in log)       # peers read the second packed buffers
    assert all(a[0] == a[1] for a in log if a[2] == "packed_out" and a[5] == "w")        # which their owners alone write
    assert not any(a[2] in ("out", "window") and a[0] != a[1] for a in log)               # and nobody a peer's out or window


@pytest.mark.parametrize("k", [2, 3, 5])
def test_a_call_makes_at_most_three_launches_per_rank(k):
    """A barrier on each side of a reading of the fabric's launch counter, which counts every rank's."""
    counts = [32 * (k - 1), 512 * k + 37]
    seen = {}

    def body(comm):
        marks = []
        for count in counts:
            for issue in range(2):
                comm.write(pc.case_input(0, issue, comm.rank, count, "bf16"))
                comm.barrier()
                marks.append(comm.launches)
                comm.barrier()
                comm.all_reduce(count, "bf16", "twoshot", wire=WIRE)
        comm.barrier()
        marks.append(comm.launches)
        seen[comm.rank] = marks

    fabric, _, errors = Q._run_threads(k, body)
    assert not errors, errors
    assert len({tuple(m) for m in seen.values()}) == 1
    per_call = np.diff(seen[0]).tolist()
    assert len(per_call) == 4 and all(0 < n <= 3 * k for n in per_call), per_call


class _NoSecondBuffer(pc.PeerComm):
    """The repack writes the rank's slice of its *first* packed buffer and phase 2 reads that: the next
    collective's quantize, which comes before barrier A, then rewrites a buffer its peers may still read."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        real = self._b._packed
        self._b._packed = lambda p, b0, b1, mode, name="packed": real(p, b0, b1, mode, "packed")


@pytest.mark.parametrize("k", [2, 3, 5])
def test_gathering_from_the_first_packed_buffer_is_a_conflict(k):
    def body(comm):
        for issue in range(2):
            comm.write(pc.case_input(0, issue, comm.rank, 2048, "bf16"))
            comm.all_reduce(2048, "bf16", "twoshot", wire=WIRE)

    fabric, _, errors = Q._run_threads(k, body, comm_cls=_NoSecondBuffer)
    assert not errors, errors
    found = fabric.conflicts()
    assert found and all(w[2] == "packed" for w, _ in found)
    # the second call's quantize, a write of the whole buffer by its owner, against a peer's phase 2 of the first call
    assert any(w[0] == w[1] and a[5] == "r" and a[0] != w[1] and w[4] - w[3] >= 2 * q8_blocks(2048) for w, a in found)
    fabric, _, errors = Q._run_threads(k, body)
    assert not errors and fabric.conflicts() == []


def test_oneshot_and_reduce_scatter_have_no_gather_phase_to_pack():
    store, fabric = pc.MemoryStore(), pc.HostFabric(2, Q.CAP)
    comm = pc.PeerComm(0, 2, 0, store, Q.CAP, backend="host", fabric=fabric)
    with pytest.raises(ValueError, match="fp8x2"):
        comm.all_reduce(64, "bf16", "oneshot", wire=WIRE)
    with pytest.raises(ValueError, match="fp8x2"):
        comm.reduce_scatter(64, "bf16", wire=WIRE)
    with pytest.raises(ValueError, match="fp8x2"):
        pc.thread_sweep([0, 0], [4096], "bf16", "oneshot", wire=WIRE)
    assert fabric.launches == 0 and comm.barriers == 0 and fabric.log == []


@pytest.mark.parametrize("k", [2, 3, 5])
def test_fp8_against_fp8x2_is_a_mismatch_on_every_rank_before_any_peer_is_read(k):
    seen = {}

    def body(comm):
        comm.write(pc.case_input(0, 0, comm.rank, 100, "bf16"))
        comm.barrier()
        seen[comm.rank] = len(comm._b.f.log)
        comm.barrier()
        comm.all_reduce(100, "bf16", "twoshot", wire=WIRE if comm.rank == 0 else "fp8")

    fabric, _, errors = Q._run_threads(k, body)
    assert sorted(errors) == list(range(k)) and all(isinstance(e, pc.PeerCommMismatch) for e in errors.values()), errors
    assert "fp8x2" in str(errors[k - 1])
    assert fabric.launches == k  # every rank's quantize, on its own buffers, and no phase 1 of any rank
    late = fabric.log[min(seen.values()):]
    assert late and all(a[0] == a[1] for a in late) and not any(a[2] in ("out", "packed_out") for a in late)


def test_block_rounded_count_must_fit_the_window():
    store, fabric = pc.MemoryStore(), pc.HostFabric(2, 1040)
    comm = pc.PeerComm(0, 2, 0, store, 1040, backend="host", fabric=fabric)
    assert 513 * 2 <= 1040 < q8_blocks(513) * 32 * 2
    with pytest.raises(ValueError, match="blocks"):
        comm.all_reduce(513, "bf16", "twoshot", wire=WIRE)
    with pytest.raises(ValueError, match="blocks"):
        comm.all_reduce(257, "fp32", "twoshot", wire=WIRE)
    assert fabric.launches == 0 and comm.barriers == 0
    with pytest.raises(ValueError):
        comm._b.repack_q8(0, 17, 1.0)
    with pytest.raises(ValueError):
        comm._b.unpack_q8([(0, 8), (8, 17)], "bf16")
    with pytest.raises(ValueError):
        comm._b.unpack_q8([(0, 9), (9, 17)], "fp32")
    with pytest.raises(ValueError):
        comm._b.unpack_q8([(3, 2), (9, 16)], "fp32")
    assert fabric.launches == 0


# -- 3. the existing cases stay, the new ones are two-shot all-reduces --------------------------
def test_selftest_case_lists():
    for k in (2, 3, 5):
        assert len(pc.selftest_cases_q8(k)) == 63
        assert all(c["wire"] == "fp8" for c in pc.selftest_cases_q8(k))
        x2 = pc.selftest_cases_q8x2(k)
        assert len(x2) == 7 * 3 and [c["count"] for c in x2[::3]] == pc.selftest_counts_q8(k)
        assert {(c["op"], c["algo"], c["wire"]) for c in x2} == {("all_reduce", "twoshot", WIRE)}
        assert {(c["dtype"], c["out_dtype"]) for c in x2} == set(PAIRS)
        assert pc._case_capacity(k, x2) == q8_blocks(8 * 1024 * k + 11) * Q8_BLOCK * 4
    assert WIRE in pc.WIRES


def test_parked_bytes_counts_both_packed_buffers():
    class Rank:
        capacity_bytes, packed_bytes = 1024, 272

    with pc._PARKED_LOCK:
        pc._PARKED.append(Rank())
    try:
        assert pc.parked_bytes() >= 3 * 1024 + 2 * 272
    finally:
        with pc._PARKED_LOCK:
            pc._PARKED.pop()


# -- 4. CLI -----------------------------------------------------------------------------------
def test_validate_wire_option():
    common = ("--devices", "0,0", "--resolve-only", "--cpu-bind", "off")
    p = Q._gtk("validate", "--backend", "peer", "--wire", WIRE, *common)
    assert p.returncode == 0, p.stderr
    p = Q._gtk("validate", "--backend", "peer", "--wire", WIRE, "--ranks", "thread", "--max-bytes", "1048576", *common)
    assert p.returncode == 0, p.stderr
    p = Q._gtk("validate", "--backend", "rccl", "--wire", WIRE, "--devices", "0,0", "--resolve-only")
    assert p.returncode == 2 and WIRE in p.stderr
    assert Q._gtk("validate", "--backend", "peer", "--wire", WIRE, "--algo", "oneshot", *common).returncode == 2


# -- 5. register budget -----------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_fp8x2_kernels_use_no_scratch(tmp_path):
    """Register budget only, from the kernels' metadata: the repack in every member bucket of the launch
    table and the unpack of both output types keep their loads in registers; the kernels that were there
    keep their number of instantiations."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa

    st = isa.kernel_stats(os.path.join(REPO, "csrc", "probe", "probe.hip"), target="_probe", out=str(tmp_path / "probe.s"))
    repack = {k: v for k, v in st.items() if "peer_q8_repack_kernel" in k}
    unpack = {k: v for k, v in st.items() if "peer_q8_unpack_kernel" in k}
    for name, v in {**repack, **unpack}.items():
        assert v["ScratchSize"] == 0 and v["scratch"] == 0, (name, v)
    assert len(repack) == 4 and len(unpack) == 2, (list(repack), list(unpack))
    for kb, u in ((2, 4), (4, 4), (8, 2), (16, 1)):  # launch_peer_q8_repack's table
        assert sum(f"Li{kb}ELi{u}E" in k for k in repack) == 1, (kb, u, list(repack))
    assert sum("peer_reduce_kernel" in k for k in st) == 12
    assert sum("peer_q8_sum_kernel" in k for k in st) == 8
    assert sum("peer_q8_quantize_kernel" in k for k in st) == 2
