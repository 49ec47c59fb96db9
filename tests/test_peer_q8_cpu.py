"""CPU tests of the K7 fp8 wire: the packed format's reference (ops/peer_ref.py) against torch's e4m3fn
cast and against its derived error bound, the wire through the peer communicator's host backend (bits,
two barriers, the race detector on the packed buffer, mismatched calls, the stale rest of a window), the
CLI's ``--wire``, and the register budget of the kernels of csrc/probe/peer_q8.h."""
import os
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest

from gpu_topology_on_k8s_amd.ops.peer_ref import (Q8_BLOCK, allreduce_q8_ref, bf16_round, bf16_to_f32, q8_blocks, q8_dequantize_ref,
                                                  q8_quantize_ref, q8_slices, reduce_scatter_q8_ref)
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

#: block amax -> (block exponent, code of the amax element), the issue's spot values
SPOTS = ((448.0, 0, 0x7E), (449.0, 1, 0x76), (1.0, -8, 0x78), (2.0 ** -120, -100, 0x00), (3e38, 120, None))


def crafted(dtype):
    """float32 values (bf16-representable for ``bf16``), whole blocks: the spot values, exact ties between
    neighbouring codes of both signs, the subnormal code range, an all-zero block, one large value among
    31 tiny ones, the integer patterns, and blocks whose amax sits on and next to a power of two."""
    blocks = []
    for amax, _, _ in SPOTS:
        b = np.zeros(Q8_BLOCK, np.float32)
        b[3] = amax
        b[7] = -amax / 3
        blocks.append(b)
    # amax 448 gives e = 0, so the block's values are their own scaled values.  Ties lie halfway between
    # two codes: normal codes in [2^-6, 448] (1 + (2 m + 1) / 16) * 2^E, subnormal ones (j + 1/2) * 2^-9.
    ties = [(1 + (2 * m + 1) / 16) * 2.0 ** E for E in range(-6, 9) for m in range(8)]
    ties = [t for t in ties if t < 448] + [(j + 0.5) * 2.0 ** -9 for j in range(8)]
    subs = [j * 2.0 ** -9 for j in range(9)] + [j * 2.0 ** -9 + 2.0 ** -12 for j in range(8)] + [2.0 ** -10, 2.0 ** -11, 3 * 2.0 ** -11]
    for vals in (ties, subs):
        vals = np.array(vals + [-v for v in vals], np.float32)
        for i in range(0, len(vals), Q8_BLOCK - 1):
            b = np.zeros(Q8_BLOCK, np.float32)
            part = vals[i:i + Q8_BLOCK - 1]
            b[:len(part)] = part
            b[-1] = 448.0
            blocks.append(b)
    blocks.append(np.zeros(Q8_BLOCK, np.float32))
    b = np.full(Q8_BLOCK, 2.0 ** -30, np.float32)
    b[::2] *= -1
    b[11] = 5.0e4
    blocks.append(b)
    blocks.append(np.arange(-8, 24, dtype=np.float32) % 16 - 8)  # the probe's integer patterns
    for amax in (256.0, 255.0, 257.0, 2.0 ** -20, 1.75 * 2.0 ** 5, np.nextafter(np.float32(1.75 * 2.0 ** 5), np.float32(1e9)), 1.875):
        b = np.linspace(-1, 1, Q8_BLOCK).astype(np.float32) * np.float32(amax)
        b[0] = amax
        blocks.append(b)
    x = np.concatenate(blocks).astype(np.float32)
    return bf16_to_f32(bf16_round(x)) if dtype == "bf16" else x


def wide_random(n, dtype, seed=0):
    """``n`` random float32 values spanning 2^-43 .. 2^43 (bf16-representable for ``bf16``)."""
    rng = np.random.default_rng([seed, n])
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-43, 44, n))).astype(np.float32)
    return bf16_to_f32(bf16_round(x)) if dtype == "bf16" else x


def as_input(x, dtype):
    """float32 values as the wire's input array: uint16 bit patterns for bf16."""
    return bf16_round(x) if dtype == "bf16" else x


# -- 1. the format ----------------------------------------------------------------------------
def test_spot_values():
    for amax, e_want, code_want in SPOTS:
        x = np.zeros(Q8_BLOCK, np.float32)
        x[5] = amax
        codes, exps = q8_quantize_ref(x, "fp32")
        assert exps.tolist() == [e_want], (amax, exps)
        if code_want is not None:
            assert codes[5] == code_want, (amax, codes[5])
    codes, exps = q8_quantize_ref(np.array([449.0], np.float32), "fp32")
    assert q8_dequantize_ref(codes, exps)[0] == 448.0  # 224.5 rounds to 224
    assert codes.shape == (Q8_BLOCK,) and not codes[1:].any()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_quantize_ref_rounds_as_torch_and_keeps_the_bound(dtype):
    x = np.concatenate([crafted(dtype), wide_random(128000, dtype)])
    codes, exps = q8_quantize_ref(as_input(x, dtype), dtype)
    assert codes.dtype == np.uint8 and codes.shape == x.shape and exps.shape == (x.size // Q8_BLOCK,)
    assert exps.min() >= -100 and exps.max() <= 120
    e = np.repeat(exps, Q8_BLOCK)
    amax = np.abs(x).reshape(-1, Q8_BLOCK).max(axis=1).astype(np.float64)
    free = (exps > -100) & (exps < 120)  # e is the smallest exponent that fits: one less does not
    assert np.all(amax * np.exp2(-exps.astype(np.float64)) <= 448)
    assert np.all(amax[free] * np.exp2(-(exps[free] - 1.0)) > 448)
    back = q8_dequantize_ref(codes, exps)
    assert np.all(np.abs(back.astype(np.float64) - x) <= np.exp2(e + 4.0))
    # amax * 2^-e > 224 wherever the lower clamp does not bind, so 2^(e+4) < amax / 14 there
    loose = np.repeat(free, Q8_BLOCK)
    assert np.all(np.abs(back.astype(np.float64) - x)[loose] <= (np.repeat(amax, Q8_BLOCK) / 14)[loose])
    try:
        import torch

        f8 = torch.float8_e4m3fn
    except (ImportError, AttributeError):
        pytest.skip("no torch.float8_e4m3fn to compare with")
    y = np.ldexp(x, -e).astype(np.float32)
    assert np.array_equal(np.ldexp(y.astype(np.float64), e)[y != 0], x.astype(np.float64)[y != 0])  # the scaling is exact
    want = torch.from_numpy(y).to(f8)
    np.testing.assert_array_equal(codes & 0x7F, want.view(torch.uint8).numpy() & 0x7F)
    np.testing.assert_array_equal(back, np.ldexp(want.to(torch.float32).numpy(), e).astype(np.float32))


def test_ties_round_to_even_and_subnormal_codes_exist():
    x = np.zeros(Q8_BLOCK, np.float32)
    x[0] = 448.0
    x[1:7] = [1.0625, 1.1875, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -9, 0.4375 * 2.0 ** -6 + 2.0 ** -10]
    codes, exps = q8_quantize_ref(x, "fp32")
    assert exps[0] == 0
    # 1.0625 is halfway between 1.0 (0x38, even) and 1.125 (0x39); 1.1875 between 0x39 and 0x3a (even)
    assert codes[1:7].tolist() == [0x38, 0x3A, 0x00, 0x02, 0x01, 0x04]


def test_integer_patterns_and_count():
    p = (np.arange(64) % 16 - 8).astype(np.float32)
    for dtype in ("bf16", "fp32"):
        codes, exps = q8_quantize_ref(as_input(p, dtype), dtype)
        assert exps.tolist() == [-5, -5]
        np.testing.assert_array_equal(q8_dequantize_ref(codes, exps), p)
        assert codes[0] == 0xF8 and codes[8] == 0x00 and codes[9] == 0x60  # -8 * 2^5 = -256, 0 and 1 * 2^5 = 32
    # what lies at or past the count is zero, whatever the array holds there
    x = np.full(100, 3.0e4, np.float32)
    x[:33] = 0.5
    codes, exps = q8_quantize_ref(x, "fp32", count=33)
    assert codes.shape == (64,) and exps.tolist() == [-9, -9] and not codes[33:].any()
    np.testing.assert_array_equal(q8_dequantize_ref(codes, exps)[:33], x[:33])


# -- 2. the collectives' references -----------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("pair", [("bf16", None), ("fp32", None), ("bf16", "fp32")])
def test_q8_references(pair, k):
    dtype, out = pair
    scale = 1.0 / k
    for count in (1, 31, 32, 33, 32 * (k - 1), 512 * k + 37):
        xs = [wide_random(count, dtype, seed=m + 1) * np.float32(2.0 ** -20) for m in range(k)]
        ins = [as_input(x, dtype) for x in xs]
        full = allreduce_q8_ref(ins, dtype, out, scale)
        pieces = reduce_scatter_q8_ref(ins, dtype, out, scale)
        assert len(pieces) == k and full.shape == (count,)
        np.testing.assert_array_equal(np.concatenate(pieces), full)
        assert [len(p) for p in pieces] == [min(count, b * 32) - min(count, a * 32) for a, b in q8_slices(q8_blocks(count), k)]
        # distance to the exact sum: every member's packing error, the fp32 sum's roundings, the output's
        exact = np.float64(np.float32(scale)) * sum(x.astype(np.float64) for x in xs)
        packing = sum(np.exp2(np.repeat(q8_quantize_ref(i, dtype)[1], Q8_BLOCK)[:count] + 4.0) for i in ins)
        mag = sum(np.abs(x.astype(np.float64)) for x in xs) + packing
        got = (bf16_to_f32(full) if full.dtype == np.uint16 else full).astype(np.float64)
        rounding = mag * scale * (k * 2.0 ** -24 + (2.0 ** -8 if full.dtype == np.uint16 else 2.0 ** -24)) + 2.0 ** -126
        assert np.all(np.abs(got - exact) <= scale * packing + rounding)


# -- 3. the protocol on the host backend ------------------------------------------------------
CAP = 1 << 17


def _counts(k):
    return [1, 31, 32, 33, 32 * (k - 1), 512 * k + 37]


def _run_threads(k, body, comm_cls=pc.PeerComm, timeout_s=20.0, cap=CAP):
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
        t.join(60)
    assert not any(t.is_alive() for t in threads)
    return fabric, results, errors


def _sequence(comm):
    """Every fp8 case, each issued twice in a row with different inputs."""
    bad, n = [], 0
    for ci, case in enumerate(pc.selftest_cases_q8(comm.world, _counts(comm.world))):
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
def test_fp8_protocol_is_exact_with_two_barriers_and_no_conflict(k):
    cases = pc.selftest_cases_q8(k, _counts(k))
    assert {c["op"] for c in cases} == {"all_reduce", "reduce_scatter"} and all(c["wire"] == "fp8" for c in cases)
    assert {(c["dtype"], c["out_dtype"]) for c in cases} == {("bf16", "bf16"), ("fp32", "fp32"), ("bf16", "fp32")}
    assert {c["algo"] for c in cases if c["op"] == "all_reduce"} == {"oneshot", "twoshot"}
    fabric, results, errors = _run_threads(k, _sequence)
    assert not errors, errors
    for r in range(k):
        n, bad = results[r]
        assert n == 2 * len(cases) and not bad, bad[:3]
    assert fabric.conflicts() == []
    assert any(a[2] == "packed" and a[5] == "r" and a[0] != a[1] for a in fabric.log)  # peers do read the packed buffers
    assert not any(a[2] == "window" and a[0] != a[1] for a in fabric.log)               # and nobody a peer's window


def test_existing_selftest_cases_are_unchanged():
    for k in (2, 3):
        assert all("wire" not in c for c in pc.selftest_cases(k))
        assert pc.selftest_counts(k) == [1, 7, 8 * (k - 1), 8 * 1024 * k + 11, (1 << 20) + 4113]
        assert len(pc.selftest_cases_q8(k)) == 7 * 9


class _LateQuantize(pc.PeerComm):
    """The quantize moved after barrier A: a rank then rewrites its packed buffer while its peers read it."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._late = None
        real = self._b.quantize
        self._real_quantize = real
        self._b.quantize = lambda *args: setattr(self, "_late", args)

    def _enter(self, desc):
        super()._enter(desc)
        if self._late is not None:
            self._real_quantize(*self._late)
            self._late = None


@pytest.mark.parametrize("k", [2, 3, 5])
def test_quantize_after_barrier_a_is_a_conflict(k):
    def body(comm):
        for issue in range(2):
            comm.write(pc.case_input(0, issue, comm.rank, 2048, "bf16"))
            comm.all_reduce(2048, "bf16", "twoshot", wire="fp8")

    fabric, _, errors = _run_threads(k, body, comm_cls=_LateQuantize)
    assert not errors, errors
    found = fabric.conflicts()
    assert found and all(w[2] == "packed" for w, _ in found)
    fabric, _, errors = _run_threads(k, body)
    assert not errors and fabric.conflicts() == []


@pytest.mark.parametrize("k", [2, 3, 5])
def test_wire_mismatch_raises_on_every_rank_before_any_peer_is_read(k):
    """The descriptors differ in ``wire`` alone.  The ranks that ask for fp8 have made their quantize by
    then, which precedes barrier A and touches their own buffers only; nothing else is launched."""
    seen = {}

    def body(comm):
        comm.write(pc.case_input(0, 0, comm.rank, 100, "bf16"))
        comm.all_reduce(100, "bf16", "oneshot")
        seen[comm.rank] = (comm.launches, len(comm._b.f.log))
        comm.barrier()
        comm.all_reduce(100, "bf16", "oneshot", wire="fp8" if comm.rank == 0 else None)

    fabric, _, errors = _run_threads(k, body)
    assert sorted(errors) == list(range(k)) and all(isinstance(e, pc.PeerCommMismatch) for e in errors.values()), errors
    assert "fp8" in str(errors[k - 1])
    assert {v[0] for v in seen.values()} == {k}
    assert fabric.launches == k + 1  # rank 0's quantize, and no phase 1 of any rank
    late = fabric.log[min(v[1] for v in seen.values()):]
    assert all(a[0] == a[1] for a in late) and not any(a[2] == "out" and a[5] == "w" for a in late)


def test_all_ranks_same_wire_mismatch_free_and_native_untouched():
    """``wire=None`` and ``wire="native"`` are one call, and neither launches a quantize."""
    def body(comm):
        comm.write(pc.case_input(0, 0, comm.rank, 100, "bf16"))
        comm.all_reduce(100, "bf16", "oneshot", wire="native" if comm.rank else None)
        return comm.launches

    fabric, results, errors = _run_threads(3, body)
    assert not errors and fabric.launches == 3 and not any(a[2] == "packed" for a in fabric.log)


def test_block_rounded_count_must_fit_the_window():
    store, fabric = pc.MemoryStore(), pc.HostFabric(2, 1040)
    comm = pc.PeerComm(0, 2, 0, store, 1040, backend="host", fabric=fabric)
    assert 513 * 2 <= 1040 < q8_blocks(513) * 32 * 2
    with pytest.raises(ValueError, match="blocks"):
        comm.all_reduce(513, "bf16", "oneshot", wire="fp8")
    with pytest.raises(ValueError, match="blocks"):
        comm.reduce_scatter(257, "fp32", wire="fp8")
    with pytest.raises(ValueError, match="wire"):
        comm.all_reduce(8, "bf16", "oneshot", wire="fp4")
    assert fabric.launches == 0 and comm.barriers == 0
    with pytest.raises(ValueError):
        comm._b.quantize(0, 17, 513, "bf16")
    with pytest.raises(ValueError):
        comm._b.reduce_q8(0, 17, "bf16", 1.0)


# -- 4. the stale rest of a window ------------------------------------------------------------
def stale_window_case(k):
    """(large first inputs, small second inputs): after 4096 large elements a 33-element call leaves
    large values in the rest of its last block, which ``write`` zeroes only to the end of a vector."""
    big = [bf16_round(np.full(4096, 3.0e4 * (m + 1), np.float32)) for m in range(k)]
    small = [bf16_round(np.random.default_rng([7, m]).standard_normal(33).astype(np.float32) * np.float32(1e-3)) for m in range(k)]
    return big, small


def stale_window_body(big, small):
    def body(comm):
        comm.write(big[comm.rank])
        comm.all_reduce(4096, "bf16", "oneshot", wire="fp8")
        comm.write(small[comm.rank])
        out = []
        for algo in pc.ALGOS:
            comm.all_reduce(33, "bf16", algo, wire="fp8")
            out.append(comm.read(0, 33, "bf16"))
        return out

    return body


def test_stale_window_is_masked_on_the_host_backend():
    k = 3
    big, small = stale_window_case(k)
    fabric, results, errors = _run_threads(k, stale_window_body(big, small))
    assert not errors, errors
    assert fabric.window[0].view(np.uint16)[40] == big[0][40]  # the stale value is there, inside block 1
    ref = allreduce_q8_ref(small, "bf16")
    for r in range(k):
        for got in results[r]:
            np.testing.assert_array_equal(got, ref)
    trusting = allreduce_q8_ref([np.concatenate([s, b[33:64]]) for s, b in zip(small, big)], "bf16")[:33]
    assert np.count_nonzero(trusting != ref) > 0  # a quantize that trusted the window's padding would show


# -- 5. CLI -----------------------------------------------------------------------------------
def _gtk(*args):
    return subprocess.run([sys.executable, "-m", "gpu_topology_on_k8s_amd", *args], capture_output=True, text=True, timeout=60, cwd=REPO)


def test_validate_wire_option():
    p = _gtk("validate", "--backend", "peer", "--wire", "fp8", "--devices", "0,0", "--resolve-only", "--cpu-bind", "off")
    assert p.returncode == 0, p.stderr
    p = _gtk("validate", "--backend", "peer", "--wire", "fp8", "--ranks", "thread", "--max-bytes", "1048576", "--devices", "0,0",
             "--resolve-only", "--cpu-bind", "off")
    assert p.returncode == 0, p.stderr
    assert _gtk("validate", "--backend", "rccl", "--wire", "fp8", "--devices", "0,0", "--resolve-only").returncode == 2
    assert _gtk("validate", "--backend", "peer", "--wire", "fp4", "--devices", "0,0", "--resolve-only").returncode == 2


# -- 6. register budget -----------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_q8_kernels_use_no_scratch(tmp_path):
    """Register budget only: the quantize of both input types and the sum of both output types in every
    member bucket keep their loads in registers; the reduce kernel gained no instantiation."""
    import isa

    st = isa.kernel_stats(os.path.join(REPO, "csrc", "probe", "probe.hip"), target="_probe", out=str(tmp_path / "probe.s"))
    q8 = {k: v for k, v in st.items() if "peer_q8_" in k}
    assert not any("peer_reduce_kernel" in k or "peer_allgather_kernel" in k for k in q8)
    for name, v in q8.items():
        assert v["ScratchSize"] == 0 and v["scratch"] == 0, (name, v)
    assert sum("peer_q8_quantize_kernel" in k for k in q8) == 2
    for kb, u in ((2, 4), (4, 4), (8, 2), (16, 1)):
        assert sum("peer_q8_sum_kernel" in k and f"Li{kb}ELi{u}E" in k for k in q8) == 2, (kb, u, list(q8))
    assert sum("peer_reduce_kernel" in k for k in st) == 12
