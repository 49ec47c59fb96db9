"""CPU: which loops of the ZeRO-1 kernels (csrc/probe/peer_zero1.h) a launch reaches, and the shapes, inputs and
references of tests/test_gpu_peer_zero1_loops.py, which imports them from here.

Every bucketed K7 kernel walks its range as ``peer_reduce_range`` does: ``per = ceil(n_tiles / grid)`` whole tiles of
``256 * U`` units per block, then a grid-stride remainder.  With the default grid (thousands of blocks) no count a test
can afford gives a block a second tile, so the GPU tests cap the grid at GRID = 2 blocks (``PeerComm(max_ctas=2)``) and
use one slice size per wire at which, for every U a ZeRO-1 kernel is launched with:

    block 0 takes at least 2 tiles; block 1 takes at least 1 and fewer than block 0; the remainder is not empty;
    where U = 4 the remainder loop makes a second trip, with a partly filled block.

  native   count = 8 * 5891 * k - 5: a slice of 5891 vectors, the last vector partly padding.
           U = 4: 5 tiles, 3 and 2, then 771 vectors in two trips (256 + 256, 256 + 3)
           U = 2: 11 tiles, 6 and 5, then 259            U = 1: 23 tiles, 12 and 11, then 3
  fp8      count = 32 * 1921 * k - 5: a slice of 1921 blocks, the smallest that meets the four conditions for every
           kernel: 3842 code vectors for launch 1 and the fused kernel, 7684 weight vectors for launch 2.
           U = 4: 3 tiles, 2 and 1, then 770 in two trips (256 + 256, 256 + 2)
           U = 2: 7 tiles, 4 and 3, then 258             U = 1: 15 tiles, 8 and 7, then 2
           launch 2 (U = 2): 15 tiles, 8 and 7, then 4

``launch_walk`` of ops/peer_ref.py is the mirror these figures come from; it is checked here against a lane-by-lane
enumeration of the loop, and ``LAUNCH_U`` against the launch lines of the headers.  The host backend runs one step at
the same counts, clipped and unclipped, bit for bit against ``zero1_step_ref``: the inputs and references are sound
before a GPU sees them."""
import functools
import math
import os
import re

import numpy as np
import pytest

import test_peer_zero1_clip_cpu as C
import test_peer_zero1_cpu as Z
from gpu_topology_on_k8s_amd.ops.peer_ref import (LAUNCH_BLOCK, LAUNCH_BUCKETS, LAUNCH_U, clip_grad_scale, launch_u, launch_walk,
                                                   reduce_scatter_q8_ref, reduce_scatter_ref, zero1_slices, zero1_sqnorm_ref, zero1_step_ref)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (2, 3, 8, 16)
WIRES = ("native", "fp8")
GRID = 2             # the cap of the GPU tests
NATIVE_VECS = 5891   # vectors of 8 bf16 in a rank's slice
FP8_BLOCKS = 1921    # blocks of 32 in a rank's slice
HP = Z.HP


def count_of(k, wire):
    return 32 * FP8_BLOCKS * k - 5 if wire == "fp8" else 8 * NATIVE_VECS * k - 5


def slice_elems(k, wire):
    """Elements of every rank's slice at count_of: all ranks hold the same number, none is empty."""
    sizes = {b - a for a, b in zero1_slices(count_of(k, wire), k, wire)}
    assert sizes == {32 * FP8_BLOCKS if wire == "fp8" else 8 * NATIVE_VECS}
    return sizes.pop()


def zero1_launches(k, wire):
    """(kernel, the units of its range) of the fused step, launch 1 and launch 2 of a rank at count_of(k, wire)."""
    n = slice_elems(k, wire)
    if wire == "fp8":  # a code vector holds 16 elements, a weight vector 8
        return (("peer_q8_sum_adamw_push", n // 16), ("peer_q8_sum_sqnorm_stash", n // 16), ("peer_adamw_push", n // 8))
    return (("peer_reduce_adamw_push", n // 8), ("peer_reduce_sqnorm_stash", n // 8), ("peer_adamw_push", n // 8))


def assert_many_tiles(tiles, trips, U, what):
    assert len(tiles) == GRID and tiles[0] >= 2 and 1 <= tiles[1] < tiles[0], (what, tiles)
    assert trips and sum(trips[0]) > 0, (what, trips)
    if U == 4:
        assert len(trips) >= 2 and any(0 < live < LAUNCH_BLOCK for live in trips[1]), (what, trips)


def norm_bound(k, wire):
    """The relative bound of the norm that tests/test_gpu_peer_zero1_clip.py derives: (slice_elems / 256 + 32) x 2^-25."""
    return (slice_elems(k, wire) / 256 + 32) * 2.0 ** -25


# -- inputs and references of the GPU tests: made once, read-only --------------------------------------
def _frozen(arrays):
    out = tuple(arrays)
    for a in out:
        a.setflags(write=False)
    return out


def _padded(pieces, n):
    out = []
    for p in pieces:
        g = np.zeros(n, np.float32)
        g[:p.size] = p
        out.append(g)
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def pieces(k, wire, count=None):
    """Every rank's gradient of the update on Z.grads(k, count, 0), the mean: its piece of the reduce-scatter with an
    fp32 output, zero in the slice's padding."""
    count = count_of(k, wire) if count is None else count
    ref = (reduce_scatter_q8_ref if wire == "fp8" else reduce_scatter_ref)(list(Z.grads(k, count, 0)), "bf16", "fp32", C.mean(k))
    return tuple(_padded([p], b - a)[0] for p, (a, b) in zip(ref, zero1_slices(count, k, wire)))


@functools.lru_cache(maxsize=None)
def sqnorm(k, wire, count=None):
    return zero1_sqnorm_ref(pieces(k, wire, count))


@functools.lru_cache(maxsize=None)
def planted_states(k, wire, count=None):
    """Every rank's start state of tests b and d: master ~ randn, m ~ 0.01 |randn|, v ~ 0.001 |randn|; in the slice's
    first vector m = v = 0 in element 1 and master is +0 and -0 in elements 3 and 4 (exempt from the vacuity cap)."""
    count = count_of(k, wire) if count is None else count
    rng = np.random.default_rng([19, k, count, wire == "fp8"])
    out = []
    for a, b in zero1_slices(count, k, wire):
        s = [rng.standard_normal(b - a, dtype=np.float32), np.abs(rng.standard_normal(b - a, dtype=np.float32)) * np.float32(0.01),
             np.abs(rng.standard_normal(b - a, dtype=np.float32)) * np.float32(0.001)]
        if b - a >= 8:
            s[1][1] = s[2][1] = 0.0
            s[0][3], s[0][4] = 0.0, -0.0
        out.append(_frozen(s))
    return tuple(out)


class Capped:
    """Mixin of a PeerComm in the GPU tests: records the grid of launch 1 of a clipped step, which launch 2 overwrites
    in ``last_grid`` before the step returns.  ``_exchange_sqnorm`` is the first thing a rank does after launch 1."""

    grid1 = None

    def _exchange_sqnorm(self, seq, mine):
        self.grid1 = self._b.r.last_grid
        return super()._exchange_sqnorm(seq, mine)


def step_under_the_rule(k, wire, count, max_ctas, clipped):
    """One step of thread ranks on device 0 from planted_states with grad_scale 0.5 at step 3, held to the float64 rule
    ``assert_adamw`` of tests/test_optim_ref.py over the padding as well as the valid elements; out must be the owner's
    master rounded once and equal on all ranks.  ``clipped``: clip_norm at half the reference norm, so the factor is
    about 0.5; the update's grad_scale is then the one ``PeerComm._zero1_step_clipped`` derives from the norm it
    returned, so the norm's own error (judged elsewhere) neither hides nor causes a failure here.  -> the ranks'
    figures of assert_adamw, and the grids seen (launch 1 or None, the last launch)."""
    import torch

    import test_optim_ref as O
    from gpu_topology_on_k8s_amd.models.optim_ref import adamw_step_ref
    from gpu_topology_on_k8s_amd.ops.peer_ref import bf16_round
    from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

    plan = zero1_slices(count, k, wire)
    start, grad = planted_states(k, wire, count), pieces(k, wire, count)
    gs_in = 0.5
    clip = 0.5 * clip_grad_scale(sqnorm(k, wire, count), gs_in, float("inf"))[0] if clipped else None

    class Comm(Capped, pc.PeerComm):
        pass

    def body(comm):
        comm.zero1_init(count, Z.weights0(count), wire, state=start[comm.rank])
        comm.write(Z.grads(k, count, 0)[comm.rank])
        norm = comm.zero1_step(step=3, grad_scale=gs_in, clip_norm=clip, **HP)
        return comm.zero1_state(), comm.read(0, plan[-1][1], "bf16"), norm, comm.grid1, comm._b.r.last_grid

    res = pc.run_thread_ranks([0] * k, body, Z.capacity(count), timeout_s=30.0, comm_cls=functools.partial(Comm, max_ctas=max_ctas))
    gs = gs_in
    if clipped:
        norm = res[0][2]
        back, gs = clip_grad_scale(norm ** 2 / gs_in ** 2, gs_in, clip)  # sqrt(x * x) == x in binary floating point: the same factor
        assert back == norm, (norm, back)
    hp = Z.hyper(3, grad_scale=gs)
    figures = []
    for r, (a, b) in enumerate(plan):
        state, out, norm, grid1, grid2 = res[r]
        assert norm == res[0][2]
        ref = adamw_step_ref(*(torch.from_numpy(x.copy()) for x in start[r]), torch.from_numpy(grad[r].copy()), hp)
        got = {key: torch.from_numpy(x.copy()) for key, x in zip(("master", "m", "v"), state)}
        exempt = torch.zeros(b - a, dtype=torch.bool)
        exempt[3:5] = True
        n = min(count, b) - min(count, a)  # this rank's parameters; past them the slice is padding without weights
        name = f"zero1 {'clipped ' if clipped else ''}k={k} {wire} count={count} max_ctas={max_ctas} rank {r}"
        O.assert_adamw(name + " padding and all", got, ref, exempt=exempt)
        got["w"] = torch.from_numpy(out[a:b].copy().view(np.int16)).view(torch.bfloat16)
        valid = {key: x[:n] for key, x in got.items()}
        figures.append(O.assert_adamw(name, valid, type(ref)(*(x[:n] for x in ref)), exempt=exempt[:n]))
        np.testing.assert_array_equal(out[a:b], bf16_round(state[0]), err_msg=name + ": out is the owner's master rounded once")
        np.testing.assert_array_equal(out, res[0][1], err_msg=name + " vs rank 0's out")
    return figures, [(x[3], x[4]) for x in res], res[0][2]


# -- 1. the mirror and the table -----------------------------------------------------------------------
def _enumerate_walk(n_units, grid, U):
    """The loop of peer_reduce_range lane by lane: which block visits which unit, in tiles and in remainder trips."""
    tile = LAUNCH_BLOCK * U
    n_tiles = n_units // tile
    per = (n_tiles + grid - 1) // grid
    seen = np.zeros(n_units, np.int64)
    tiles, trips = [], {}
    for b in range(grid):
        t0 = b * per
        t1 = min(n_tiles, t0 + per)
        took = 0
        t = t0
        while t < t1:
            for lane in range(LAUNCH_BLOCK):
                for u in range(U):
                    seen[t * tile + lane + u * LAUNCH_BLOCK] += 1
            took += 1
            t += 1
        tiles.append(took)
        for lane in range(LAUNCH_BLOCK):
            i, trip = n_tiles * tile + b * LAUNCH_BLOCK + lane, 0
            while i < n_units:
                seen[i] += 1
                trips.setdefault(trip, [0] * grid)[b] += 1
                i += grid * LAUNCH_BLOCK
                trip += 1
    assert (seen == 1).all()  # every unit once
    return tiles, [trips[t] for t in sorted(trips)]


@pytest.mark.parametrize("U", (1, 2, 4))
def test_launch_walk_is_the_loop_lane_by_lane(U):
    sizes = [0, 1, 255, 256, 257, 256 * U - 1, 256 * U, 256 * U + 1, 2 * 256 * U + 513, 5 * 256 * U + 771, NATIVE_VECS, 2 * FP8_BLOCKS,
             4 * FP8_BLOCKS]
    for n in sizes:
        for grid in (1, 2, 3, 5, 64):
            assert launch_walk(n, grid, U) == _enumerate_walk(n, grid, U), (n, grid, U)
    tiles, trips = launch_walk(NATIVE_VECS, 5, 1)  # 23 tiles on 5 blocks: per = 5, the last block is cut short by the end
    assert tiles == [5, 5, 5, 5, 3] and trips == [[3, 0, 0, 0, 0]]
    assert launch_walk(40 * 256, 64, 1)[0] == [1] * 40 + [0] * 24  # blocks past the last tile take none
    with pytest.raises(ValueError):
        launch_walk(8, 0, 1)


LAUNCH_LINE = re.compile(r"\b(\w+)_kernel<(?:[^<>;]*?,\s*)?(\d+),\s*(\d+)><<<")


def test_the_table_of_u_is_the_headers():
    """Every ``name_kernel<.., KB, U><<<`` of the two headers, and nothing else, is in LAUNCH_U with that U."""
    found = {}
    for header in ("csrc/probe/peer_zero1.h", "csrc/probe/peer_driver.h"):
        for name, kb, u in LAUNCH_LINE.findall(open(os.path.join(REPO, header)).read()):
            found.setdefault(name, {})[int(kb)] = int(u)
    assert set(found) == set(LAUNCH_U), sorted(set(found) ^ set(LAUNCH_U))
    for name, per_bucket in found.items():
        assert tuple(sorted(per_bucket)) == LAUNCH_BUCKETS, name
        assert tuple(per_bucket[kb] for kb in LAUNCH_BUCKETS) == LAUNCH_U[name], name
    assert [launch_u("peer_reduce_adamw_push", k) for k in (1, 2, 3, 4, 5, 8, 9, 16)] == [4, 4, 2, 2, 2, 2, 1, 1]
    with pytest.raises(ValueError):
        launch_u("peer_reduce", 17)


# -- 2. the shapes of the GPU tests --------------------------------------------------------------------
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_every_zero1_kernel_takes_many_tiles_per_block_at_these_counts(k, wire):
    count = count_of(k, wire)
    assert count <= 32 * FP8_BLOCKS * 16 and count % 8 == 3  # the last vector (fp8: block) is partly padding
    seen = set()
    for kernel, units in zero1_launches(k, wire):
        U = launch_u(kernel, k)
        tiles, trips = launch_walk(units, GRID, U)
        print(f"{kernel} k={k} {wire}: U={U} units={units} tiles per block {tiles} remainder trips {trips}")
        assert_many_tiles(tiles, trips, U, (kernel, k, wire))
        seen.add(U)
    # with the default grid the same launches run per = 1 at most, which is why the cap exists
    assert all(max(launch_walk(units, -(-units // 256), launch_u(kernel, k))[0]) <= 1 for kernel, units in zero1_launches(k, wire))
    if wire == "native":
        assert launch_walk(NATIVE_VECS, 2, 4) == ([3, 2], [[256, 256], [256, 3]])
        assert launch_walk(NATIVE_VECS, 2, 2) == ([6, 5], [[256, 3]]) and launch_walk(NATIVE_VECS, 2, 1) == ([12, 11], [[3, 0]])


def test_the_three_values_of_u_are_all_run():
    for wire in WIRES:
        for i in range(2):  # the fused kernel and launch 1
            assert {launch_u(zero1_launches(k, wire)[i][0], k) for k in KS} >= ({1, 2, 4} if (wire, i) != ("fp8", 0) else {1, 2})
    assert not any(sl[1] == sl[0] for k in KS for wire in WIRES for sl in zero1_slices(count_of(k, wire), k, wire))


@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_a_slice_of_signs_sums_its_squares_exactly_in_any_order(k, wire):
    """exact_total of tests/test_gpu_peer_zero1_clip.py asserts that every slice's sum of squares stays below 2^24."""
    import test_gpu_peer_zero1_clip as G

    count = count_of(k, wire)
    total = G.exact_total(k, count, wire)
    assert 0 < total < k * k * count and math.sqrt(total) > 0


# -- 3. the host backend at these counts ---------------------------------------------------------------
@pytest.mark.parametrize("clipped", (False, True))
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("k", KS)
def test_the_host_backend_follows_the_reference_at_these_counts(k, wire, clipped):
    from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

    count = count_of(k, wire)
    clip = C.clip_of(k, count, wire, "half") if clipped else None

    def body(comm):
        comm.zero1_init(count, Z.weights0(count), wire)
        comm.write(Z.grads(k, count, 0)[comm.rank])
        norm = comm.zero1_step(step=1, clip_norm=clip, **HP)
        return comm.zero1_state(), comm.read(0, count, "bf16"), norm

    # max_ctas is accepted and ignored: the host backend has no grid
    fabric, results, errors = Z._run_threads(k, body, Z.capacity(count), comm_cls=functools.partial(pc.PeerComm, max_ctas=GRID))
    assert not errors, errors
    ref = zero1_step_ref(list(Z.grads(k, count, 0)), Z.states0(k, count, wire), "bf16", C.mean(k), Z.hyper(1), wire, clip_norm=clip)
    for r in range(k):
        state, out, norm = results[r]
        assert all(Z._same(a, b) for a, b in zip(state, ref[0][r])), (k, wire, r)
        assert Z._same(out, ref[1]) and (norm == ref[2] if clipped else norm is None), (k, wire, r)
    assert fabric.conflicts() == []
    # and the gradient the GPU tests hold the update to is the one this step used
    if clipped:
        assert ref[2] == clip_grad_scale(sqnorm(k, wire), 1.0, float("inf"))[0] and clip == 0.5 * ref[2]


def test_max_ctas_is_checked_on_either_backend():
    from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="max_ctas"):
            pc.PeerComm(0, 2, 0, pc.MemoryStore(), 4096, backend="host", fabric=pc.HostFabric(2, 4096), max_ctas=bad)
        with pytest.raises(ValueError, match="max_ctas"):  # before anything is allocated on a device
            pc.PeerComm(0, 2, 0, pc.MemoryStore(), 4096, backend="device", max_ctas=bad)
    comm = pc.PeerComm(0, 2, 0, pc.MemoryStore(), 4096, backend="host", fabric=pc.HostFabric(2, 4096), max_ctas=3)
    assert comm.max_ctas == 3 and pc.PeerComm(0, 2, 0, pc.MemoryStore(), 4096, backend="host", fabric=pc.HostFabric(2, 4096)).max_ctas == 0


# -- 4. the packed references of test g ----------------------------------------------------------------
def test_the_packed_references_of_the_older_kernels_are_ops_peer_refs():
    """tests/test_gpu_peer_comm_device._reference packs every member's input once and composes the packed wires'
    references from that; here it is held to the functions of ops/peer_ref that it stands for."""
    import test_gpu_peer_comm_device as D
    from gpu_topology_on_k8s_amd.ops.peer_ref import (allreduce_q8_ef_ref, allreduce_q8_ref, allreduce_q8x2_ref, reduce_scatter_q8_ef_ref,
                                                       reduce_scatter_q8_ref)

    k, count = 3, 32 * 7 * 3 - 5
    zeros = [np.zeros(32 * 7 * 3, np.float32)] * k
    for dtype, out, scale in (("bf16", "bf16", 1.0), ("fp32", "fp32", 1.0), ("bf16", "fp32", 1.0 / k)):
        xs = list(D._inputs(k, count, dtype, 0))
        ref = lambda op, wire, ef: D._reference(k, count, op, dtype, out, scale, 0, wire, ef)  # noqa: E731
        assert Z._same(ref("all_reduce", "fp8", False)[1], allreduce_q8_ref(xs, dtype, out, scale))
        assert Z._same(ref("all_reduce", "fp8x2", False)[2], allreduce_q8x2_ref(xs, dtype, out, scale))
        assert all(Z._same(a, b) for a, b in zip(ref("reduce_scatter", "fp8", False), reduce_scatter_q8_ref(xs, dtype, out, scale)))
        for wire in ("fp8", "fp8x2"):
            want, after = allreduce_q8_ef_ref(xs, zeros, dtype, out, scale, wire)
            assert Z._same(ref("all_reduce", wire, True)[0], want)
            assert all(Z._same(a, b) for a, b in zip(D._packed_inputs(k, count, dtype, 0, True)[1], after))
        want, after = reduce_scatter_q8_ef_ref(xs, zeros, dtype, out, scale)
        assert all(Z._same(a, b) for a, b in zip(ref("reduce_scatter", "fp8", True), want))
