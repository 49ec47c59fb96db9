"""GPU tests of the wide (bf16 in, fp32 out) and scaled K7 reduce through the in-process driver.

Every member is device 0, so a one-GPU box runs every member bucket and both algorithms.  Results are
compared bit for bit with ops/peer_ref.py."""
import functools

import numpy as np
import pytest

from gpu_topology_on_k8s_amd.ops.peer_ref import allreduce_ref, bf16_round

pytestmark = pytest.mark.gpu

ALGOS = ["oneshot", "twoshot"]


def _counts(k):  # the five counts of tests/test_gpu_peer_allreduce.py::_counts
    return [1, 7, 8 * (k - 1), 8 * 1024 * k + 11, (1 << 20) + 4113]


@functools.lru_cache(maxsize=None)
def _wide_case(k, count):
    """k members' bf16 inputs and the fp32 mean; made once, read-only."""
    rng = np.random.default_rng(7000 * k + count % 997)
    xs = [bf16_round(rng.standard_normal(count).astype(np.float32)) for _ in range(k)]
    ref = allreduce_ref(xs, "bf16", "fp32", 1.0 / k)
    for a in xs + [ref]:
        a.setflags(write=False)
    return xs, ref


def _assert_bits(outs, ref, what):
    assert len(outs) > 1
    for m, o in enumerate(outs):
        assert o.dtype == ref.dtype and o.shape == ref.shape, (what, m)
        np.testing.assert_array_equal(o.view(np.uint32), ref.view(np.uint32), err_msg=f"{what} member {m}")


@pytest.mark.parametrize("k", [2, 3, 8, 16])
@pytest.mark.parametrize("algo", ALGOS)
def test_wide_mean_is_exact_in_process(algo, k):
    from gpu_topology_on_k8s_amd.ops.probe import peer_allreduce_arrays

    for count in _counts(k):
        xs, ref = _wide_case(k, count)
        outs = peer_allreduce_arrays([0] * k, xs, "bf16", algo, out_dtype="fp32", scale=1.0 / k)
        assert len(outs) == k
        _assert_bits(outs, ref, f"bf16->fp32 {algo} k={k} count={count}")


@pytest.mark.parametrize("algo", ALGOS)
def test_scale_follows_the_sum(algo):
    """fp32, k = 3, scale = 1/3: the inputs on which "sum then scale" and "scale then sum" differ
    (tests/test_peer_comm_cpu.py asserts that they do); the kernel gives the former."""
    from gpu_topology_on_k8s_amd.ops.probe import peer_allreduce_arrays

    rng = np.random.default_rng(20240607)
    xs = [rng.standard_normal(4096).astype(np.float32) for _ in range(3)]
    ref = allreduce_ref(xs, "fp32", None, 1.0 / 3.0)
    other = allreduce_ref([(x * np.float32(1.0 / 3.0)).astype(np.float32) for x in xs], "fp32")
    assert np.count_nonzero(ref.view(np.uint32) != other.view(np.uint32)) >= 1
    _assert_bits(peer_allreduce_arrays([0, 0, 0], xs, "fp32", algo, scale=1.0 / 3.0), ref, f"fp32 scale 1/3 {algo}")
