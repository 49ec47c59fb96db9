"""Can the probe's and the all-reduce's self-checks fail?  (real MI355X)

Every entry point below verifies its own destination on the device and reports ``ok`` or a count of wrong
elements; the link matrix, ``bench.py``'s "checked exactly" and ``gtk validate`` rest on those reports.  A
report is worth something only if it fails when the kernel under it did no work, when it mixed its sources
up, or when one element at the edge of the range is wrong.  So:

* ``dry_run=True`` runs an entry point on its real path without its copy, gather, reduce or all-reduce
  launches.  Between two real calls with the same arguments it must fail: the destination is written wrong
  before the launches (the complement of the expected pattern, or ``0xFF`` bytes), so what an earlier call
  left in memory that the allocator hands back, or in a buffer that persists, cannot pass.
* a gather's sources are seeded by slot, so ``[0, 0, 0]`` gives three different segments.
* the pattern verifier and the all-reduce's check count one wrong element at either end of their range, the
  pattern verifier also on both sides of one grid stride where the buffer reaches that far.
"""
import numpy as np
import pytest

from test_gpu_native import COPY_KINDS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe_mod():
    from gpu_topology_on_k8s_amd._native import load

    p = load("_probe")
    assert p.device_count() >= 1, "no HIP device visible"
    return p


@pytest.fixture(scope="module")
def rccl():
    from gpu_topology_on_k8s_amd._native import load

    return load("_rccl")


@pytest.fixture(scope="module")
def comm(rccl):
    c = rccl.Comm(rccl.unique_id(), 1, 0, 0)
    c.self_copy_min_bytes = 0  # every size to the repository's copy kernel
    yield c
    c.destroy()


def _triple(call):
    """real, dry, real: the results of the three calls."""
    return call(False), call(True), call(False)


# ------------------------------------------------------------------------------- stale destinations
@pytest.mark.parametrize("kind,nontemporal,unroll", COPY_KINDS)
def test_copy_dry_run_fails_between_two_real_calls(probe_mod, kind, nontemporal, unroll):
    """The sizes of test_copy_kinds_at_boundary_shapes: the vector tail alone, fewer tiles than blocks, and
    more than one tile per block with a ragged last slice (about 8 MiB)."""
    from gpu_topology_on_k8s_amd.ops.probe import copy_bw

    tile = 256 * unroll * 16
    grid = probe_mod.device_props(0)["cus"]
    tail = 16 * 37
    for nbytes in (tail, 3 * tile + tail, (2 * grid + 5) * tile + tail):
        a, dry, b = _triple(lambda d: copy_bw(0, 0, nbytes, iters=1, warmup_iters=0, kind=kind, nontemporal=nontemporal,
                                              blocks_per_cu=1, dry_run=d))
        assert a["ok"] is True and a["dry_run"] is False, a
        assert dry["ok"] is False and dry["dry_run"] is True, dry
        assert b["ok"] is True and b["dry_run"] is False, b
        assert a["bytes"] == dry["bytes"] == nbytes and dry["grid"] == grid


def test_gather_dry_run_fails_between_two_real_calls(probe_mod):
    from gpu_topology_on_k8s_amd.ops.probe import gather_bw

    a, dry, b = _triple(lambda d: gather_bw(0, [0, 0, 0], (1 << 20) + 4112, dry_run=d))
    assert a["ok"] is True and dry["ok"] is False and b["ok"] is True, (a, dry, b)
    assert dry["dry_run"] is True and a["dry_run"] is False


def test_ring_dry_run_fails_between_two_real_calls(probe_mod):
    from gpu_topology_on_k8s_amd.ops.probe import ring_bw

    a, dry, b = _triple(lambda d: ring_bw([0] * 3, "all", (1 << 20) + 4112, dry_run=d))
    assert a["ok"] is True and dry["ok"] is False and b["ok"] is True, (a, dry, b)
    assert dry["dry_run"] is True and a["dry_run"] is False


@pytest.mark.parametrize("algo", ["oneshot", "twoshot"])
@pytest.mark.parametrize("dtype,elem", [("bf16", 2), ("fp32", 4)])
def test_peer_allreduce_dry_run_counts_every_checked_element(probe_mod, dtype, elem, algo):
    """K7's check walks every member's output, the zero padding up to the last whole 16-byte vector included:
    with no kernel run, all of it is wrong."""
    from gpu_topology_on_k8s_amd.ops.probe import peer_allreduce

    k, count = 3, 8 * 1024 * 3 + 11
    padded = -(-count * elem // 16) * 16 // elem  # a buffer is whole 16-byte vectors
    assert count < padded < count + 16 // elem
    a, dry, b = _triple(lambda d: peer_allreduce([0] * k, count, dtype, algo, dry_run=d))
    assert a["ok"] is True and a["wrong"] == 0, a
    assert dry["ok"] is False and dry["wrong"] == k * padded and dry["dry_run"] is True, dry
    assert b["ok"] is True and b["wrong"] == 0, b


@pytest.mark.parametrize("dtype,elem", [("bf16", 2), ("fp32", 4)])
def test_comm_check_dry_run_counts_every_element(rccl, comm, dtype, elem):
    """The receive buffer persists and has just passed a larger size, so it holds the right value in every
    element the smaller sizes check: T + 16 + 2 bytes (a tile, a vector and the 2-byte tail) and 2 bytes."""
    T = rccl.SELF_COPY_TILE_BYTES
    comm.prepare(2 * T + 64, dtype)
    assert comm.check(False) == 0
    for nbytes in (T + 16 + 2, 2):
        comm.prepare(nbytes, dtype)
        n = comm.bytes // elem
        assert n == max(1, nbytes // elem)
        assert comm.check(False) == 0, nbytes
        assert comm.check(False, dry_run=True) == n, nbytes
        assert comm.check(False) == 0, nbytes
        assert comm.check(True, dry_run=True) == 0  # in place a one-rank sum is its own input: nothing to do


def test_local_sweep_dry_run_counts_every_element(rccl):
    nbytes = (1 << 20) + 6
    run = lambda d: rccl.local_sweep([0], [nbytes], "bf16", 1, 0, False, True, dry_run=d)[0]
    a, dry, b = _triple(run)
    assert a["wrong"] == 0 and a["dry_run"] is False, a
    assert dry["wrong"] == dry["count"] == nbytes // 2 and dry["dry_run"] is True, dry
    assert b["wrong"] == 0, b


# ------------------------------------------------------------------------------- segments are told apart
def test_gather_and_ring_segments_have_distinct_seeds(probe_mod):
    from gpu_topology_on_k8s_amd.ops.probe import gather_bw, ring_bw

    g = gather_bw(0, [0, 0, 0], (1 << 20) + 4112)
    assert g["ok"] is True and len(g["seeds"]) == 3 and len(set(g["seeds"])) == 3, g
    r = ring_bw([0] * 3, "all", (1 << 20) + 4112)
    assert r["ok"] is True and len(r["seeds"]) == 3 and len(set(r["seeds"])) == 3, r


# ------------------------------------------------------------------------------- verifiers count single elements
def _pattern_word(i, seed):
    return ((i * 2654435761) & 0xFFFFFFFF) ^ seed


@pytest.mark.parametrize("beyond_one_stride", [False, True])
def test_pattern_verifier_counts_single_words(probe_mod, beyond_one_stride):
    """pattern_mismatch_kernel on (1 << 20) + 16 bytes: the first word, the last word, then a word on either
    side of one grid stride (256 threads x CUs x BLOCKS_PER_CU words).  On a device whose grid stride exceeds
    that buffer (256 CUs: 2 MiB of words) the two words are those on either side of the first 256-thread block
    instead, and the second case repeats the sequence on a buffer one stride longer, where they fit."""
    seed = 0x5EED
    stride = probe_mod.BLOCK * probe_mod.device_props(0)["cus"] * probe_mod.BLOCKS_PER_CU
    nbytes = (1 << 20) + 16 + (4 * stride if beyond_one_stride else 0)
    words = nbytes // 4
    b = probe_mod.IpcBuffer(0, nbytes, seed=seed)
    assert b.mismatches(seed) == 0 and b.holds(seed)
    edge = stride if stride < words else probe_mod.BLOCK
    assert not beyond_one_stride or edge == stride
    for n, i in enumerate((0, words - 1, edge - 1, edge), start=1):
        b.poke(i, _pattern_word(i, seed) ^ 1)  # one bit off
        assert b.mismatches(seed) == n, (i, n)
        assert not b.holds(seed)
    b.poke(0, _pattern_word(0, seed))
    assert b.mismatches(seed) == 3
    assert b.mismatches(seed ^ 1) == words - 3  # the other seed: every word but the three that are one bit off
    with pytest.raises(IndexError):
        b.poke(words, 0)


def _pattern_bits(i, np_dtype):
    """The bits gtk_fill_kernel gives element i on one rank: (i % 7) + 1, as fp32 or as bf16 (exact)."""
    bits = np.array([(i % 7) + 1], dtype=np.float32).view(np.uint32)
    return bits if np_dtype == np.uint32 else (bits >> 16).astype(np.uint16)


@pytest.mark.parametrize("dtype,np_dtype", [("bf16", np.uint16), ("fp32", np.uint32)])
def test_allreduce_verifier_counts_single_elements(rccl, comm, dtype, np_dtype):
    """gtk_check_kernel after a real step: the last element one unit in the last place off, then the first."""
    T = rccl.SELF_COPY_TILE_BYTES
    comm.prepare(T + 16 + 6, dtype)
    n = comm.count
    assert n == (T + 16 + 6) // np.dtype(np_dtype).itemsize
    comm.step(False)
    comm.synchronize()
    assert comm.verify() == 0
    for wrong, i in enumerate((n - 1, 0), start=1):
        good = _pattern_bits(i, np_dtype)
        assert comm.read_result(i, 1) == good.tobytes()
        comm.write_result(i, (good ^ 1).tobytes())  # differs in the lowest mantissa bit alone
        assert comm.verify() == wrong, i
    comm.write_result(n - 1, _pattern_bits(n - 1, np_dtype).tobytes())
    assert comm.verify() == 1


def test_write_result_is_bounds_checked(comm):
    comm.prepare(64, "fp32")
    n = comm.count
    four = b"\0" * 4
    comm.write_result(n, b"")  # the empty range at the end, as read_result allows it
    for first, data in ((n, four), (n - 1, four * 2), (n + 1, b""), (0, four * (n + 1))):
        with pytest.raises(IndexError):
            comm.write_result(first, data)
    with pytest.raises(ValueError):
        comm.write_result(0, b"\0" * 3)  # not whole elements
    comm.step(False)
    comm.synchronize()
    assert comm.verify() == 0
