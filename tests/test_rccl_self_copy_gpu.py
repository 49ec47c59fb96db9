"""The one-rank all-reduce's own copy kernel (csrc/rccl/self_copy.h) on a real MI355X: exact over every
boundary of the kernel (vector body, tile tail, 2-byte tail, the grid cap, 2^32 bytes), a byte copy and
not merely a passing pattern, identical to RCCL's path, capturable into a hipGraph, and switchable.

By default the kernel takes only the large messages at which it was measured to win
(``SELF_COPY_MIN_BYTES``).  Its boundary cases are small, so the shared communicator sends every size to
it (``Comm.self_copy_min_bytes = 0``); the 64-bit case and the routing test run with the default."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rccl():
    assert "GTK_RCCL_SELF_COPY" not in os.environ, "these tests run with the switch at its default"
    from gpu_topology_on_k8s_amd._native import load

    return load("_rccl")


@pytest.fixture(scope="module")
def comm(rccl):
    c = rccl.Comm(rccl.unique_id(), 1, 0, 0)
    assert c.self_copy and c.self_copy_min_bytes == rccl.SELF_COPY_MIN_BYTES
    c.self_copy_min_bytes = 0
    yield c
    c.destroy()


def _pattern(first, n, np_dtype):
    return ((np.arange(first, first + n, dtype=np.int64) % 7) + 1).astype(np_dtype)


def _read(c, first, n, np_dtype, inplace=False):
    return np.frombuffer(c.read_result(first, n, inplace), dtype=np_dtype)


def test_boundary_sizes_are_exact(rccl, comm):
    T = rccl.SELF_COPY_TILE_BYTES
    cap = comm.self_copy_max_blocks
    assert T % 16 == 0 and cap == rccl.SELF_COPY_BLOCKS_PER_CU * comm.self_copy_cus and cap >= 1
    sizes = [2, 14, 16, 18, T - 2, T, T + 2, T + 16 + 2, cap * T * 2 + T + 6]
    for dt, elem in (("bf16", 2), ("fp32", 4)):
        last = ((1 << 20) + 3) * elem
        for nbytes in sizes + [last]:
            comm.prepare(nbytes, dt)  # whole elements: fp32 rounds a count of 4k + 2 bytes down to 4k (at least 4)
            assert comm.bytes == max(nbytes - nbytes % elem, elem)
            assert comm.check(False) == 0, (dt, nbytes)
            # The receive buffer persists over the walk and, but for the first size, already holds the right
            # value in part or all of the range (the last size is smaller than the one before it): check()
            # fills it with NaN first, so the same check without the all-reduce counts every element.
            if nbytes in (2, 14, last):
                assert comm.check(False, dry_run=True) == comm.bytes // elem, (dt, nbytes)
                assert comm.check(False) == 0, (dt, nbytes)


def test_result_is_a_byte_copy_of_the_pattern(rccl, comm):
    T = rccl.SELF_COPY_TILE_BYTES
    cap = comm.self_copy_max_blocks
    nbytes = cap * T * 2 + T + 16 + 6  # whole tiles past the grid cap, a vector tail and a 2-byte tail
    n = nbytes // 2
    comm.prepare(nbytes, "bf16")
    comm.step(False)
    comm.synchronize()
    u16 = lambda first, m: (_pattern(first, m, np.float32).view(np.uint32) >> 16).astype(np.uint16)  # bf16 bits, exact
    span = T // 2 + 11
    for first in (0, n // 2 - 5, n - span):
        assert np.array_equal(_read(comm, first, span, np.uint16), u16(first, span)), first
    comm.step(True)  # in place: the identity, nothing to move
    comm.synchronize()
    for first in (0, n // 2 - 5, n - span):
        assert np.array_equal(_read(comm, first, span, np.uint16, inplace=True), u16(first, span)), first
    assert comm.check(True) == 0


def test_both_paths_agree_byte_for_byte(comm):
    n = (1 << 20) + 3
    comm.prepare(n * 2, "bf16")
    got = {}
    try:
        for on in (False, True):
            comm.self_copy = on
            assert comm.self_copy is on
            comm.step(False)
            comm.synchronize()
            got[on] = comm.read_result(0, n, False)
    finally:
        comm.self_copy = True
    assert len(got[True]) == n * 2 and got[False] == got[True]


def test_indices_are_64_bit(rccl):
    import torch

    free, _total = torch.cuda.mem_get_info(0)
    if free < 10 << 30:
        pytest.skip(f"needs 10 GiB of free device memory for two 4 GiB buffers, {free >> 30} GiB free")
    c = rccl.Comm(rccl.unique_id(), 1, 0, 0)
    assert (4 << 30) + 18 >= c.self_copy_min_bytes
    try:
        c.prepare((4 << 30) + 18, "bf16")
        assert c.check(False) == 0
    finally:
        c.destroy()


def test_default_routing_is_exact_on_both_sides_of_the_cutoff(rccl):
    """Below SELF_COPY_MIN_BYTES the message goes to RCCL, from it on to the kernel (a multiple of the tile
    plus every tail kind); both are exact, out of place and in place."""
    cut = rccl.SELF_COPY_MIN_BYTES
    c = rccl.Comm(rccl.unique_id(), 1, 0, 0)
    try:
        for nbytes in ([cut - 2, cut + 16 + 2] if cut else [1 << 20]):
            c.prepare(nbytes, "bf16")
            assert c.check(False) == 0 and c.check(True) == 0, nbytes
    finally:
        c.destroy()


def test_graph_capture_replays_the_kernel(rccl, comm):
    for nbytes in (rccl.SELF_COPY_TILE_BYTES + 2, 1 << 20):
        comm.prepare(nbytes, "bf16")
        comm.capture(4, False)
        assert comm.graph_ops == 4
        # capture() ran one eager all-reduce, so the receive buffer is right before any replay: spoil all of it
        comm.synchronize()
        comm.write_result(0, b"\xff" * comm.bytes)
        assert comm.verify() == comm.bytes // 2
        for _ in range(3):
            comm.replay()
        comm.synchronize()
        assert comm.verify() == 0


def test_environment_switch_restores_the_rccl_path():
    code = ("from gpu_topology_on_k8s_amd._native import load\n"
            "r = load('_rccl')\n"
            "c = r.Comm(r.unique_id(), 1, 0, 0)\n"
            "assert c.self_copy is False\n"
            "c.prepare((1 << 20) + 6, 'bf16')\n"
            "assert c.check(False) == 0\n"
            "c.destroy()\n"
            "print('switch ok')\n")
    env = dict(os.environ, GTK_RCCL_SELF_COPY="0")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=REPO, env=env)
    assert p.returncode == 0 and "switch ok" in p.stdout, p.stderr[-4000:]
