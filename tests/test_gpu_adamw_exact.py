"""GPU: the AdamW kernels (csrc/ops/adamw.hip, update body adam8_update of csrc/common/adamw_update.h) element by
element against the float64 reference of models/optim_ref.py, and every launch loop on a second trip.  The root of
the AdamW chain: the tile and ranges kernels, the non-finite tests of tests/test_fused_gpu.py and the ZeRO-1 tests
compare bit for bit (or at the old tolerances) with the flat kernel, which is held to the reference here.

Cases, reference and the rule ``assert_adamw`` (master within half an fp32 ulp + 2^-20 of the step's magnitude, m'
and v' within 2^-21 of theirs, W the kernel's own master rounded once) are those of tests/test_optim_ref.py, whose
CPU self-tests pass an fp32 emulation through the same cases and fail ten mutants.  Every comparison with the
reference runs on the CPU; every kernel is called once per case.

1. The flat kernel (adamw_flat_kernel: 256 threads x 8 elements per block, at most 4096 blocks), entry points
   ``adamw_step`` and ``adamw_step_dev`` (clip active; clip off in hp; no partials), bf16 and fp32 gradients:
     n = 8                         one thread; every lane of the vector is planted
     n = 8 * 257                   one vector past a block: the second block's single live thread
                                   both with the three hyper-parameter sets (training; t = 1, lr 0.25, wd 0.5; t = 1000)
     n = 8 * (4096 * 256 + 777)    the grid-stride loop: a second trip for the first 777 threads only, so a ragged
                                   last stride; planted vectors first and last in both trips; training set
2. The tile and ranges kernels at their loops, bit for bit against the flat kernel on one plan (``t_plan``):
     4454 tiles on a 4096-block grid     358 blocks take a second trip through the LDS tile (the trailing
                                         __syncthreads) in matrices of three shapes and the single-tile matrix
     41 transposed matrices, 6 shapes    the binary search over tile_base; 64 x 256 (tiles_c = 1, one tile, the
                                         last index), 51200 x 256 (800 row tiles), 64 x 153600 (600 column tiles)
     ranges of 1024, 8, 4,200,520, 128   shorter than a block; one vector; 2048 x 256 + 777 vectors, the ranges
                                         kernel's second trip with a ragged last stride; one more
     two holes of 56 elements            in no matrix and no range: they keep their bits
   FlatParams lays parameters out in units of 64 elements, so its plan has no range of 8 and covers the buffer;
   the test takes FlatParams' plan and cuts the two ranges short.  For the same reason W^T has no alignment gaps
   (every matrix is a multiple of 64 x 256): master, m, v, W and W^T lie between guard zones instead, which must
   keep their fill, and W^T is prefilled with NaN.
3. The ZeRO-1 fused step (peer_reduce_adamw_push_kernel, peer_q8_sum_adamw_push_kernel), one step under the rule:
   k = 3 and 16 thread ranks of device 0, both wires, count = 8 * 1024 * k + 11 (tiles, a tail, padding), against
   adamw_step_ref of the reduced gradient that ops/peer_ref reproduces bit for bit.
4. Launch 2 of the clipped ZeRO-1 step (peer_adamw_push_kernel, after peer_reduce_sqnorm_stash_kernel or
   peer_q8_sum_sqnorm_stash_kernel has left the gradient in the stash), one clipped step under the rule at the same
   count and ranks with the default grid, where every block takes one tile at most: the reference's grad_scale is the
   factor the step derives from the norm it returned, so the norm's own error (held to its bound in
   tests/test_gpu_peer_zero1_clip.py) plays no part.  tests/test_gpu_peer_zero1_loops.py runs the same body, and
   section 3's, with a block walking many tiles.
"""
import numpy as np
import pytest
import torch

import test_optim_ref as O
from gpu_topology_on_k8s_amd.models.optim_ref import adamw_step_ref

pytestmark = pytest.mark.gpu

KEYS = ("master", "m", "v", "g", "w")
ENTRIES = ("host", "dev clip", "dev clip off in hp", "dev no partials")


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "needs a GPU"
    from gpu_topology_on_k8s_amd.ops.fused import hip as load_hip

    return load_hip()  # raises (fails loudly) if the extension is missing


def _run_flat(hip, c, entry):
    """One launch of the entry point on device copies of case c -> its outputs on the CPU."""
    st = {k: c[k].cuda() for k in KEYS}
    if entry == "host":
        hip.adamw_step(st["master"], st["m"], st["v"], st["g"], st["w"], c["hp"].cuda())
    else:
        clip = -1.0 if entry == "dev clip off in hp" else O.CLIP
        part = None if entry == "dev no partials" else hip.sq_norm_parts(st["g"], None)
        t = torch.tensor([float(O.HYPERS[c["hp_name"]][6])], device="cuda")
        hip.adamw_step_dev(st["master"], st["m"], st["v"], st["g"], st["w"], O.hyper_dev(c["hp_name"], clip).cuda(), part, t)
    torch.cuda.synchronize()
    assert torch.equal(st["g"].cpu(), c["g"])  # the gradient is read only
    return {k: st[k].cpu() for k in ("master", "m", "v", "w")}


def _reference(c, entry, cache=None):
    """(reference, slacks, vacuity cap) of an entry point on case c; ``cache``: a dict that keeps the references of
    a large case (clip off and no partials share theirs with each other, not with the host form: the bias
    corrections differ in their last bits)."""
    if entry == "host":
        key, make = "host", lambda: (adamw_step_ref(c["master"], c["m"], c["v"], c["g"], c["hp"]), O.HOST_SLACKS)
    else:
        clipped = entry == "dev clip"
        key, make = ("dev", clipped), lambda: O.dev_reference(c, O.CLIP if clipped else -1.0, clipped)[:2]
    if cache is None:
        ref, slacks = (c["ref"], O.HOST_SLACKS) if entry == "host" and "ref" in c else make()
    else:
        if key not in cache:
            cache[key] = make()
        ref, slacks = cache[key]
    return ref, slacks, (O.case_cap(c["hp_name"]) if entry == "host" else None)


# -- 1. the flat kernel against float64 ------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("hp_name", list(O.HYPERS))
@pytest.mark.parametrize("gdtype", O.GDTYPES)
@pytest.mark.parametrize("n", O.FLAT_SMALL)
def test_flat_kernel_at_the_smallest_sizes(hip, n, gdtype, hp_name, entry):
    c = O.small_case(n, gdtype, hp_name)
    ref, slacks, cap = _reference(c, entry)
    O.assert_adamw(f"flat {entry} n={n} {str(gdtype)[6:]} {hp_name}", _run_flat(hip, c, entry), ref, slacks, c["exempt"], cap)
    if hp_name == "t1" and entry == "host":
        O.assert_step_sharpness(c, ref)


@pytest.fixture(scope="module")
def large_cases():
    """gdtype -> (case, {entry kind: reference}); made at first use, read-only."""
    return {}


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("gdtype", O.GDTYPES)
def test_flat_kernel_on_the_second_trip_of_its_grid_stride_loop(hip, large_cases, gdtype, entry):
    n = O.FLAT_LARGE
    assert n // 8 == 4096 * 256 + 777
    if gdtype not in large_cases:
        large_cases[gdtype] = (O.make_case(n, gdtype, "train", vectors=O.FLAT_LARGE_VECTORS), {})
    c, cache = large_cases[gdtype]
    assert [int(c["planted"][8 * v]) for v in O.FLAT_LARGE_VECTORS] == [1, 1, 1, 1]
    ref, slacks, cap = _reference(c, entry, cache)
    O.assert_adamw(f"flat {entry} n={n} {str(gdtype)[6:]} train", _run_flat(hip, c, entry), ref, slacks, c["exempt"], cap)


# -- 2. the tile and ranges kernels at their loops --------------------------------------------------------
GUARD = 4096  # elements of fill on either side of every buffer
BIG_RANGE = 8 * (2048 * 256 + 777)
MIDS = [(576, 2304), (1024, 1280), (320, 4096)]  # 9 x 9, 16 x 5 and 5 x 16 tiles


def _t_shapes():
    mid = lambda a, b: [(f"mid{i}", MIDS[i % 3]) for i in range(a, b)]  # noqa: E731
    return ([("v0", (1000,)), ("tall", (64 * 800, 256))] + mid(0, 13) + [("wide", (64, 256 * 600)), ("v1", (64,))] + mid(13, 26)
            + [("big", (BIG_RANGE,))] + mid(26, 38) + [("v2", (128,)), ("one", (64, 256))])


def _guarded(x, fill):
    """x between two guard zones -> (the whole buffer, the view that holds x)."""
    buf = torch.full((x.numel() + 2 * GUARD,), fill, dtype=x.dtype, device=x.device)
    buf[GUARD:GUARD + x.numel()] = x
    return buf, buf[GUARD:GUARD + x.numel()]


def _guards_intact(buf, fill):
    f = torch.tensor(fill, dtype=buf.dtype, device=buf.device)
    same = lambda z: bool((z == f).all()) if fill == fill else bool(torch.isnan(z).all())  # noqa: E731
    return same(buf[:GUARD]) and same(buf[-GUARD:])


@pytest.fixture(scope="module")
def t_plan(hip):
    """The plan of the module docstring, the start state (seeded, on the device, read-only) and a cache of the flat
    kernel's results per (gradient type, device form)."""
    from gpu_topology_on_k8s_amd.models.llama import FlatParams

    flat = FlatParams(_t_shapes(), "cuda")
    names = [n for n, s in _t_shapes() if len(s) == 2]
    assert flat.enable_transposed(names) == names
    mats, tiles, ranges, maxr = flat.adamw_plan()
    assert tiles == 800 + 600 + 1 + 13 * 81 + 13 * 80 + 12 * 80 == 4454 and tiles > 4096 + 300
    assert mats.shape[0] == 41 and len({flat.shapes[n] for n in names}) == 6
    assert sum(R * C for R, C in (flat.shapes[n] for n in names)) == flat.data_t.numel()  # W^T has no gaps
    o = flat.offsets
    assert ranges.cpu().tolist() == [[0, 1024], [o["v1"], 64], [o["big"], BIG_RANGE + 56], [o["v2"], 128]]
    # FlatParams' ranges cut short: one vector of v1, and big without its padding; the two rests are the holes
    ranges = torch.tensor([[0, 1024], [o["v1"], 8], [o["big"], BIG_RANGE], [o["v2"], 128]], dtype=torch.int64, device="cuda")
    hole = torch.zeros(flat.numel, dtype=torch.bool, device="cuda")
    hole[o["v1"] + 8:o["v1"] + 64] = True
    hole[o["big"] + BIG_RANGE:o["big"] + BIG_RANGE + 56] = True
    assert maxr == BIG_RANGE + 56 and BIG_RANGE // 8 == 2048 * 256 + 777
    gen = torch.Generator("cuda").manual_seed(7)
    n = flat.numel
    r = lambda: torch.randn(n, device="cuda", generator=gen)  # noqa: E731
    st = {"master": r(), "m": r().abs() * 0.01, "v": r().abs() * 0.001, "g32": r()}
    st["w"] = st["master"].to(torch.bfloat16)
    return {"flat": flat, "names": names, "mats": mats, "tiles": tiles, "ranges": ranges, "maxr": BIG_RANGE, "hole": hole, "st": st,
            "roots": {}}


def _dev_inputs(hip, g):
    return (torch.tensor(O.hyper_dev("train", O.CLIP).tolist(), device="cuda"), hip.sq_norm_parts(g, None),
            torch.tensor([float(O.HYPERS["train"][6])], device="cuda"))


@pytest.mark.parametrize("dev,ahead,gdtype", [(False, 1, torch.bfloat16), (False, 2, torch.bfloat16), (False, 4, torch.bfloat16),
                                              (True, 1, torch.bfloat16), (False, 2, torch.float32)])
def test_tile_and_ranges_kernels_on_their_second_trips_match_the_flat_kernel(hip, t_plan, dev, ahead, gdtype):
    P = t_plan
    flat, st, hole = P["flat"], P["st"], P["hole"]
    g = st["g32"].to(gdtype)
    hp = O.hyper8("train").cuda()
    if (gdtype, dev) not in P["roots"]:  # the flat kernel over the whole buffer, once; the holes put back
        ref = {k: st[k].clone() for k in ("master", "m", "v", "w")}
        if dev:
            hp_dev, part, t = _dev_inputs(hip, g)
            hip.adamw_step_dev(ref["master"], ref["m"], ref["v"], g, ref["w"], hp_dev, part, t)
        else:
            hip.adamw_step(ref["master"], ref["m"], ref["v"], g, ref["w"], hp)
        for k in ref:
            assert k == "w" or not torch.equal(ref[k][hole], st[k][hole])  # the flat kernel did update them
            ref[k][hole] = st[k][hole]
        P["roots"][(gdtype, dev)] = ref
    ref = P["roots"][(gdtype, dev)]
    fills = {"master": 7.0, "m": 7.0, "v": 7.0, "w": 7.0}
    bufs, got = {}, {}
    for k, f in fills.items():
        bufs[k], got[k] = _guarded(st[k], f)
    wt_buf = torch.full((flat.data_t.numel() + 2 * GUARD,), float("nan"), dtype=torch.bfloat16, device="cuda")
    wt = wt_buf[GUARD:-GUARD]
    g0 = g.clone()
    if dev:
        hp_dev, part, t = _dev_inputs(hip, g)
        hip.adamw_step_t(got["master"], got["m"], got["v"], g, got["w"], wt, hp_dev, P["mats"], P["tiles"], P["ranges"], P["maxr"], part, t, 1)
    else:
        hip.adamw_step_t(got["master"], got["m"], got["v"], g, got["w"], wt, hp, P["mats"], P["tiles"], P["ranges"], P["maxr"], None, None,
                         ahead)
    torch.cuda.synchronize()
    assert torch.equal(g, g0)
    for k in ("master", "m", "v", "w"):
        assert torch.equal(got[k], ref[k]), k  # the flat kernel's bits; the holes keep theirs
        assert torch.equal(got[k][hole], st[k][hole]) and _guards_intact(bufs[k], fills[k]), k
    assert _guards_intact(wt_buf, float("nan")) and not bool(torch.isnan(wt).any())  # every element of W^T written, none outside
    for name in P["names"]:
        R, C = flat.shapes[name]
        o, ot = flat.offsets[name], flat.t_offsets[name]
        assert torch.equal(wt[ot:ot + R * C].view(C, R), got["w"][o:o + R * C].view(R, C).t()), name


# -- 3. the ZeRO-1 fused step under the rule --------------------------------------------------------------
@pytest.mark.parametrize("wire", ["native", "fp8"])
@pytest.mark.parametrize("k", [3, 16])
def test_zero1_fused_step_against_float64(k, wire):
    """One step from a random state (planted in every rank's first vector: m = v = 0, master +0, master -0) with
    grad_scale 0.5 at step 3.  The gradient of the update is the reduce-scatter's fp32 piece, zero in the padding."""
    import test_peer_zero1_cpu as Z
    from gpu_topology_on_k8s_amd.ops.peer_ref import reduce_scatter_q8_ref, reduce_scatter_ref, zero1_slices
    from gpu_topology_on_k8s_amd.parallel import peer_comm as pc

    count = 8 * 1024 * k + 11
    plan = zero1_slices(count, k, wire)
    rng = np.random.default_rng([9, k])
    start = []
    for a, b in plan:
        s = [rng.standard_normal(b - a, dtype=np.float32), np.abs(rng.standard_normal(b - a, dtype=np.float32)) * np.float32(0.01),
             np.abs(rng.standard_normal(b - a, dtype=np.float32)) * np.float32(0.001)]
        if b - a >= 8:
            s[1][1] = s[2][1] = 0.0
            s[0][3], s[0][4] = 0.0, -0.0
        start.append(tuple(s))

    def body(comm):
        comm.zero1_init(count, Z.weights0(count), wire, state=start[comm.rank])
        comm.write(Z.grads(k, count, 0)[comm.rank])
        comm.zero1_step(step=3, grad_scale=0.5, **Z.HP)
        return comm.zero1_state(), comm.read(0, plan[-1][1], "bf16")

    res = pc.run_thread_ranks([0] * k, body, Z.capacity(count), timeout_s=30.0)
    pieces = (reduce_scatter_q8_ref if wire == "fp8" else reduce_scatter_ref)(list(Z.grads(k, count, 0)), "bf16", "fp32",
                                                                             float(np.float32(1.0 / k)))
    hp = Z.hyper(3, grad_scale=0.5)
    for r, (a, b) in enumerate(plan):
        state, out = res[r]
        g = np.zeros(b - a, np.float32)
        g[:pieces[r].size] = pieces[r]
        ref = adamw_step_ref(*(torch.from_numpy(x.copy()) for x in start[r]), torch.from_numpy(g), hp)
        got = {key: torch.from_numpy(x.copy()) for key, x in zip(("master", "m", "v"), state)}
        exempt = torch.zeros(b - a, dtype=torch.bool)
        exempt[3:5] = True
        n = min(count, b) - min(count, a)  # this rank's parameters; past them the slice is padding without weights
        name = f"zero1 k={k} {wire} rank {r}"
        O.assert_adamw(name + " padding and all", got, ref, exempt=exempt)
        got["w"] = torch.from_numpy(out[a:b].copy().view(np.int16)).view(torch.bfloat16)
        valid = {key: x[:n] for key, x in got.items()}
        O.assert_adamw(name, valid, type(ref)(*(x[:n] for x in ref)), exempt=exempt[:n])
        np.testing.assert_array_equal(out, res[0][1], err_msg=name + " vs rank 0's out")


# -- 4. launch 2 of the clipped ZeRO-1 step under the rule ------------------------------------------------
@pytest.mark.parametrize("wire", ["native", "fp8"])
@pytest.mark.parametrize("k", [3, 16])
def test_zero1_clipped_step_against_float64(k, wire):
    """One clipped step from a random planted state with grad_scale 0.5 at step 3 and clip_norm at half the reference
    norm, no cap on the grid: tests/test_peer_zero1_loops_cpu.step_under_the_rule."""
    import test_peer_zero1_loops_cpu as L
    from gpu_topology_on_k8s_amd.ops.peer_ref import launch_u, launch_walk, zero1_slices

    count = 8 * 1024 * k + 11
    figures, grids, _ = L.step_under_the_rule(k, wire, count, 0, clipped=True)
    first = "peer_q8_sum_sqnorm_stash" if wire == "fp8" else "peer_reduce_sqnorm_stash"
    for (a, b), (g1, g2) in zip(zero1_slices(count, k, wire), grids):  # about 1025 vectors on five blocks: no second tile
        one = launch_walk((b - a) // (16 if wire == "fp8" else 8), g1, launch_u(first, k))[0]
        two = launch_walk((b - a) // 8, g2, launch_u("peer_adamw_push", k))[0]
        assert g1 >= 1 and g2 >= 1 and max(one) <= 1 and max(two) <= 1, (grids, one, two)
    print(f"figures 4 k={k} {wire}: worst err/tol over ranks " + ", ".join(f"{key} {max(f[key] for f in figures):.3f}" for key in figures[0]))
