"""CPU checks of the K7 peer all-reduce: the slice plan and the numpy reference the GPU tests compare
against, the ``gtk validate --backend`` command line, and the register budget of the kernels (hipcc
cross-compiles gfx950)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

from gpu_topology_on_k8s_amd.ops.peer_ref import allreduce_ref, bf16_round, peer_slices  # noqa: E402


def test_slices_are_ordered_disjoint_and_cover_the_range():
    for n_vec in range(0, 71):
        for k in range(2, 17):
            sl = peer_slices(n_vec, k)
            assert len(sl) == k
            at = 0
            for first, end in sl:  # each starts where the one before ended: ordered, disjoint, no gap
                assert first == at and end >= first, (n_vec, k, sl)
                at = end
            assert at == n_vec, (n_vec, k, sl)
            per = -(-n_vec // k)
            assert all(end - first <= per for first, end in sl)


def test_reference_rounding_is_torch_bf16_rounding():
    import torch

    rng = np.random.default_rng(7)
    x = np.concatenate([rng.standard_normal(50_000).astype(np.float32),
                        (rng.standard_normal(50_000) * 10.0 ** rng.uniform(-30, 30, 50_000)).astype(np.float32)])
    # exact halfway cases between neighbouring bf16 values, even and odd kept mantissa, both signs, and
    # the one that carries into the exponent
    hi = np.array([0x3F80, 0x3F81, 0x3FFF, 0x4000, 0x0080, 0x7F00, 0xBF80, 0xBF81, 0xC07F], dtype=np.uint32)
    half = ((hi << 16) | 0x8000).view(np.float32)
    near = np.concatenate([((hi << 16) | 0x7FFF).view(np.float32), ((hi << 16) | 0x8001).view(np.float32)])
    x = np.concatenate([x, half, near, np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32)])
    assert np.isfinite(x).all()
    want = torch.tensor(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(bf16_round(x), want)


def test_reference_sums_in_member_order():
    a, b, c = (np.full(4, v, dtype=np.float32) for v in (2.0 ** 24, 1.0, -(2.0 ** 24)))
    np.testing.assert_array_equal(allreduce_ref([a, b, c], "fp32"), np.zeros(4, np.float32))  # 2^24 + 1 rounds to 2^24
    np.testing.assert_array_equal(allreduce_ref([a, c, b], "fp32"), np.ones(4, np.float32))


def test_reference_bf16_rounds_once_after_the_fp32_sum():
    # 1 + 2^-8 + 2^-8: each partial sum rounded to bf16 would stay 1.0; one rounding of the fp32 sum gives 1 + 2^-7
    one, eps = np.array([0x3F80], np.uint16), np.array([0x3B80], np.uint16)
    np.testing.assert_array_equal(allreduce_ref([one, eps, eps], "bf16"), np.array([0x3F81], np.uint16))


def _gtk(*args):
    return subprocess.run([sys.executable, "-m", "gpu_topology_on_k8s_amd", *args], capture_output=True, text=True, cwd=REPO,
                          timeout=120)


def test_validate_backend_peer_parses():
    p = _gtk("validate", "--backend", "peer", "--devices", "0,0", "--resolve-only", "--cpu-bind", "off")
    assert p.returncode == 0, p.stderr
    assert json.loads(p.stdout.strip().splitlines()[-1]) == {"hip_devices": [0, 0]}
    p = _gtk("validate", "--backend", "peer", "--algo", "twoshot", "--devices", "0,0", "--resolve-only", "--cpu-bind", "off")
    assert p.returncode == 0, p.stderr


def test_validate_unknown_backend_or_algo_exits_2():
    assert _gtk("validate", "--backend", "mpi", "--devices", "0,0", "--resolve-only").returncode == 2
    assert _gtk("validate", "--backend", "peer", "--algo", "ring", "--devices", "0,0", "--resolve-only").returncode == 2


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_peer_kernels_use_no_scratch(tmp_path):
    """Register budget only: every instantiation of the reduce kernel (both element types, every
    member bucket) and the all-gather kernel keeps its k x U loads in registers."""
    import isa

    st = isa.kernel_stats(os.path.join(REPO, "csrc", "probe", "probe.hip"), target="_probe", out=str(tmp_path / "probe.s"))
    reduce_k = {k: v for k, v in st.items() if "peer_reduce_kernel" in k}
    gather_k = {k: v for k, v in st.items() if "peer_allgather_kernel" in k}
    assert reduce_k and gather_k, list(st)
    for name, v in {**reduce_k, **gather_k}.items():
        assert v["ScratchSize"] == 0 and v["scratch"] == 0, (name, v)
