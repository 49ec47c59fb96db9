"""GPU tests of the five ZeRO-1 kernels (csrc/probe/peer_zero1.h) with a block walking many tiles: thread ranks of
device 0 on a communicator capped at two blocks (``PeerComm(max_ctas=2)``), at the counts of
tests/test_peer_zero1_loops_cpu.py, where block 0 takes at least two tiles, block 1 fewer, and the remainder loop
runs (twice where U = 4).  With the default grid no affordable count gives a block a second tile, so without the cap
the loop over tiles, the state index ``E * (o - first)`` more than a tile past ``first`` and a lane's second add into
the sum of squares never run under test, though a training step runs little else.

Every test asserts the grid of the launch it is about (``PeerRank.last_grid``), so none can pass on the one-tile path.

  a  the sums inside the fused kernels, bit for bit (lr = beta1 = beta2 = weight_decay = 0)
  b  the fused step under the float64 rule ``assert_adamw`` of tests/test_optim_ref.py
  c  launch 1: the norm of {-1, 0, 1} gradients exactly; the stash bit for bit and the norm within
     (slice_elems / 256 + 32) x 2^-25 on random gradients
  d  launch 2 under the float64 rule, with the factor derived from the norm the step returned
  e  nothing outside [0, count) and its padding is written (0xFFFF poison), clipped and unclipped
  f  a step under the cap has the bits of a step without it: the grid is a neutral parameter (the norm: the bound of c)
  g  the older kernels (reduce, push, fp8 sum and push, repack, quantize with and without feedback) bit for bit
     through the capped communicator

Bit-for-bit references are ops/peer_ref's; inputs and references are made once (tests/test_peer_zero1_loops_cpu.py,
tests/test_peer_zero1_cpu.py) and are read-only.  No tolerance is new."""
import functools
import math

import numpy as np
import pytest

import test_gpu_peer_comm_device as D
import test_gpu_peer_zero1_clip as G
import test_peer_zero1_clip_cpu as C
import test_peer_zero1_cpu as Z
import test_peer_zero1_loops_cpu as L
from gpu_topology_on_k8s_amd.ops.peer_ref import (bf16_round, bits, clip_grad_scale, is_nan_bits, launch_u, launch_walk, peer_slices, q8_blocks,
                                                   q8_slices, zero1_slices)
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

pytestmark = pytest.mark.gpu

KS = list(L.KS)
WIRES = list(L.WIRES)
HP = Z.HP
GRID = L.GRID
EXACT = G.EXACT


class Comm(L.Capped, pc.PeerComm):
    pass


def _ranks(k, body, cap, max_ctas=GRID):
    return pc.run_thread_ranks([0] * k, body, cap, timeout_s=30.0, comm_cls=functools.partial(Comm, max_ctas=max_ctas))


def _grid(comm):
    return comm._b.r.last_grid


# -- a. the sums inside the fused kernels ---------------------------------------------------------------
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_a_the_sum_inside_the_fused_kernel_is_exact_over_many_tiles(k, wire):
    count = L.count_of(k, wire)
    plan = zero1_slices(count, k, wire)

    def body(comm):
        comm.zero1_init(count, Z.weights0(count), wire)
        comm.write(Z.grads(k, count, 0)[comm.rank])
        comm.zero1_step(step=1, **EXACT)
        return comm.zero1_state(), comm.read(0, plan[-1][1], "bf16"), _grid(comm)

    res = _ranks(k, body, Z.capacity(count))
    start, grad = Z.states0(k, count, wire), L.pieces(k, wire)
    for r, (a, b) in enumerate(plan):
        (master, m, v), out, grid = res[r]
        what = f"k={k} {wire} count={count} rank {r}"
        assert grid == GRID, what
        assert not grad[r][min(count, b) - a:].any()  # zeros in the padding
        np.testing.assert_array_equal(bits(m), bits(grad[r]), err_msg="m " + what)
        np.testing.assert_array_equal(bits(v), bits((grad[r] * grad[r]).astype(np.float32)), err_msg="v " + what)
        np.testing.assert_array_equal(bits(master), bits(start[r][0]), err_msg="master " + what)
        np.testing.assert_array_equal(out, np.concatenate([bf16_round(s[0]) for s in start]), err_msg="out " + what)


# -- b. the fused step under the float64 rule -----------------------------------------------------------
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_b_the_fused_step_over_many_tiles_against_float64(k, wire):
    figures, grids, _ = L.step_under_the_rule(k, wire, L.count_of(k, wire), GRID, clipped=False)
    assert all(g == (None, GRID) for g in grids), grids
    print(f"figures b k={k} {wire}: worst err/tol over ranks " + ", ".join(f"{key} {max(f[key] for f in figures):.3f}" for key in figures[0]))


# -- c. launch 1 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_c_the_norm_of_signs_is_exact_over_many_tiles(k, wire):
    """scale = 1 and clip_norm = inf on gradients from {-1, 0, 1}: every fp32 order of summation gives the integer
    total, so the norm is sqrt of it, bit for bit, however many positions a lane adds into its sum."""
    count = L.count_of(k, wire)
    inputs = G.signs(k, count)[0]
    want = math.sqrt(G.exact_total(k, count, wire))

    def body(comm):
        comm.zero1_init(count, Z.weights0(count), wire)
        comm.write(inputs[comm.rank])
        return comm.zero1_step(step=1, scale=1.0, clip_norm=float("inf"), **HP), comm.grid1, _grid(comm)

    for r, (norm, grid1, grid2) in enumerate(_ranks(k, body, Z.capacity(count))):
        assert (grid1, grid2) == (GRID, GRID), (k, wire, r)
        assert isinstance(norm, float) and norm == want, (k, wire, r, norm, want)


@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_c_the_stash_is_exact_and_the_norm_within_its_bound_over_many_tiles(k, wire):
    count = L.count_of(k, wire)
    plan = zero1_slices(count, k, wire)

    def body(comm):
        comm.zero1_init(count, Z.weights0(count), wire)
        comm.write(Z.grads(k, count, 0)[comm.rank])
        norm = comm.zero1_step(step=1, clip_norm=float("inf"), **HP)
        a, b = plan[comm.rank]
        return norm, comm._b.zero1_read_state(3, 0, b - a), comm.grid1

    res = _ranks(k, body, Z.capacity(count))
    grad = L.pieces(k, wire)
    want = clip_grad_scale(L.sqnorm(k, wire), 1.0, float("inf"))[0]
    bound = L.norm_bound(k, wire)
    for r in range(k):
        norm, stash, grid1 = res[r]
        what = f"k={k} {wire} count={count} rank {r}"
        assert grid1 == GRID, what
        np.testing.assert_array_equal(bits(stash), bits(grad[r]), err_msg="stash " + what)
        rel = abs(norm - want) / want
        if r == 0:
            print(f"figures c norm {what}: {norm!r} reference {want!r} relative {rel:.3e} bound {bound:.3e} ratio {rel / bound:.3f}")
        assert rel <= bound, (what, norm, want, rel, bound)
        assert norm == res[0][0], what


# -- d. launch 2 under the float64 rule -----------------------------------------------------------------
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_d_the_clipped_update_over_many_tiles_against_float64(k, wire):
    figures, grids, _ = L.step_under_the_rule(k, wire, L.count_of(k, wire), GRID, clipped=True)
    assert all(g == (GRID, GRID) for g in grids), grids  # the norm is judged on its own in c
    print(f"figures d k={k} {wire}: worst err/tol over ranks " + ", ".join(f"{key} {max(f[key] for f in figures):.3f}" for key in figures[0]))


# -- e. nothing outside is written ----------------------------------------------------------------------
@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", [3, 16])
def test_e_the_padding_is_zero_and_nothing_past_it_is_written(k, wire, clipped):
    """Every byte of out[0, end + 4096 elements) is 0xFF before the step (an all-gather of 0xFFFF patterns); after it
    the count's weights are there, the rest of the last vector (fp8: block) is zero and everything after is 0xFF."""
    unit = 32 if wire == "fp8" else 8
    count = L.count_of(k, wire)
    end = unit * (-(-count // unit))
    per = 8 * (-(-(end + 4096) // (8 * k)))  # elements every rank contributes to the poison
    clip = C.clip_of(k, count, wire, "half") if clipped else None

    def body(comm):
        comm.zero1_init(count, Z.weights0(count), wire)
        comm.write(np.full(per, 0xFFFF, np.uint16), comm.gather_slot(per, "bf16"))
        comm.all_gather(per, "bf16")
        poisoned = comm.read(0, k * per, "bf16")
        comm.write(Z.grads(k, count, 0)[comm.rank])
        comm.zero1_step(step=1, clip_norm=clip, **HP)
        return poisoned, comm.read(0, k * per, "bf16"), comm.grid1, _grid(comm)

    res = _ranks(k, body, max(Z.capacity(count), 2 * k * per))
    for r in range(k):
        poisoned, out, grid1, grid2 = res[r]
        assert (grid1, grid2) == (GRID if clipped else None, GRID), (k, wire, r)
        assert (poisoned == 0xFFFF).all()
        assert not is_nan_bits(out[:count]).any() and (out[:count] != 0xFFFF).all()
        assert end > count and not out[count:end].any(), (k, wire, r)
        assert (out[end:] == 0xFFFF).all() and out[end:].size >= 4096, (k, wire, r)
        np.testing.assert_array_equal(out, res[0][1])


# -- f. the capped grid changes no bit ------------------------------------------------------------------
@pytest.mark.parametrize("clipped", [False, True])
@pytest.mark.parametrize("wire", WIRES)
def test_f_a_step_under_the_cap_has_the_bits_of_a_step_without_it(wire, clipped):
    """Each element is computed by one lane from the same operands, whichever block holds it: master, m, v, out and the
    stash are the same bit for bit.  The norm is not: its summation order follows the grid; both are within the bound."""
    k = 3
    count = L.count_of(k, wire)
    plan = zero1_slices(count, k, wire)
    start = L.planted_states(k, wire)
    clip = 0.5 * clip_grad_scale(L.sqnorm(k, wire), 0.5, float("inf"))[0] if clipped else None

    def body(comm):
        comm.zero1_init(count, Z.weights0(count), wire, state=start[comm.rank])
        comm.write(Z.grads(k, count, 0)[comm.rank])
        norm = comm.zero1_step(step=3, grad_scale=0.5, clip_norm=clip, **HP)
        a, b = plan[comm.rank]
        stash = comm._b.zero1_read_state(3, 0, b - a) if clipped else None
        return comm.zero1_state(), comm.read(0, plan[-1][1], "bf16"), stash, norm, _grid(comm)

    capped, free = _ranks(k, body, Z.capacity(count)), _ranks(k, body, Z.capacity(count), max_ctas=0)
    if clipped:
        # the two norms differ in their last bits; were the factors they round to different too, no bit could be compared
        gs = [np.float32(clip_grad_scale(x[0][3] ** 2 / 0.25, 0.5, clip)[1]) for x in (capped, free)]
        assert gs[0] == gs[1], ("the two grids' norms round to different float32 factors: use another seed", gs)
    for r in range(k):
        what = f"{wire} clipped={clipped} rank {r}"
        assert capped[r][4] == GRID and free[r][4] > GRID, (what, capped[r][4], free[r][4])
        for name, x, y in zip(("master", "m", "v"), capped[r][0], free[r][0]):
            np.testing.assert_array_equal(bits(x), bits(y), err_msg=f"{name} {what}")
        np.testing.assert_array_equal(capped[r][1], free[r][1], err_msg="out " + what)
        if clipped:
            np.testing.assert_array_equal(bits(capped[r][2]), bits(free[r][2]), err_msg="stash " + what)
            want = clip_grad_scale(L.sqnorm(k, wire), 0.5, float("inf"))[0]
            for norm in (capped[r][3], free[r][3]):
                assert abs(norm - want) / want <= L.norm_bound(k, wire), (what, norm, want)


# -- g. the older kernels through the capped communicator -----------------------------------------------
def _older_cases(k, family):
    native, packed = [8 * L.NATIVE_VECS * k - 5], [32 * L.FP8_BLOCKS * k - 5]
    return {"native": lambda: pc.selftest_cases(k, native), "fp8": lambda: pc.selftest_cases_q8(k, packed),
            "fp8x2": lambda: pc.selftest_cases_q8x2(k, packed),
            "push": lambda: pc.selftest_cases_push(k, native)[:3] + pc.selftest_cases_push(k, packed)[3:],
            "ef": lambda: pc.selftest_cases_ef(k, packed)}[family]()


class _Grids(pc.PeerComm):
    """Records (what, grid) of the launches a collective synchronises after: the quantize of a packed wire, the rank's
    last launch when it comes to ``_enter``, and phase 1, its last launch when it comes to ``_leave``."""

    def _enter(self, desc):
        self._op = desc["op"]
        if desc.get("wire") in ("fp8", "fp8x2"):
            self.grids = getattr(self, "grids", set()) | {("quantize", self._b.r.last_grid)}
        super()._enter(desc)

    def _leave(self):
        self.grids = getattr(self, "grids", set()) | {(self._op, self._b.r.last_grid)}
        super()._leave()


@pytest.mark.parametrize("family", ["native", "fp8", "fp8x2", "push", "ef"])
@pytest.mark.parametrize("k", [2, 16])
def test_g_the_older_kernels_are_exact_over_many_tiles(k, family):
    """_assert_exact of tests/test_gpu_peer_comm_device.py on the selftest's case lists, each case issued once: the
    reduce, push, fp8 sum, repack and quantize walks while a block takes several tiles.  The gather and unpack launches
    keep their grids, which the cap does not touch."""
    cases = _older_cases(k, family)
    assert {c.get("wire") for c in cases} == {"native": {None}, "fp8": {"fp8"}, "fp8x2": {"fp8x2"}, "push": {None, "fp8"},
                                              "ef": {"fp8", "fp8x2"}}[family]
    for c in cases:  # the slice a rank reduces takes many tiles on two blocks, in the bf16 and in the fp32 window alike
        if c["op"] != "all_gather":
            packed = c.get("wire") is not None
            n = q8_blocks(c["count"]) if packed else -(-c["count"] * (2 if c["dtype"] == "bf16" else 4) // 16)
            a, b = (q8_slices if packed else peer_slices)(n, k)[0]
            tiles, trips = launch_walk((2 if packed else 1) * (b - a), GRID, launch_u("peer_q8_sum" if packed else "peer_reduce", k))
            assert tiles[0] >= 2 and tiles[1] >= 1 and trips, (c, tiles, trips)
    seen = []

    class Spy(_Grids):
        def close(self):
            seen.append(getattr(self, "grids", set()))
            super().close()

    D._assert_exact([0] * k, None, cases=cases, issues=1, comm_cls=functools.partial(Spy, max_ctas=GRID), run_case=False)
    grids = set().union(*seen)
    launched = {c["op"] for c in cases} | ({"quantize"} if family not in ("native", "push") else set())
    assert len(seen) == k and {what for what, _ in grids} >= launched, grids
    # every reduce and every quantize had two blocks; an all-gather's one launch is a gather, which keeps its grid
    assert all(grid == GRID for what, grid in grids if what != "all_gather"), grids


# -- h. the argument itself -----------------------------------------------------------------------------
def test_h_the_cap_is_checked_and_last_grid_starts_at_zero():
    from gpu_topology_on_k8s_amd._native import load

    P = load("_probe")
    with pytest.raises(ValueError, match="max_ctas"):
        P.PeerRank(0, 0, 2, 4096, max_ctas=-1)
    r = P.PeerRank(0, 0, 2, 4096, max_ctas=GRID)
    assert r.last_grid == 0 and r.launches == 0
    r.release()

    def body(comm):
        comm.write(np.ones(8 * 256 * 40, np.float32))
        comm.all_reduce(8 * 256 * 40, "fp32", "oneshot")
        return _grid(comm), comm.max_ctas

    assert _ranks(2, body, 1 << 20) == [(GRID, GRID)] * 2
    assert all(g > GRID and m == 0 for g, m in _ranks(2, body, 1 << 20, max_ctas=0))  # 20480 vectors: 80 blocks, or the CUs' share
