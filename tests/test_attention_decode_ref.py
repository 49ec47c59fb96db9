"""CPU: the float64 reference of decode attention over a ragged KV cache (``attn_decode_ref64``), the CPU path
and the refusals of ``fused.attention_decode``, ``decode_splits_for``, and the scratch-free build of the kernel.
``decode_inputs`` is also the input maker of tests/test_gpu_attention_decode.py."""
import functools
import os
import sys

import pytest
import torch

import test_attention_ref as A
from gpu_topology_on_k8s_amd.models import attention_ref as R
from gpu_topology_on_k8s_amd.ops import fused

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAKS = (30.0, 24.0, 35.0, 19.0, 39.0, 33.0, 27.0)  # log2 units; neighbours differ by less and by more than the slack 8
CPU_CASE = (2, 4, 2, 3, 150, (3, 137))


@functools.lru_cache(maxsize=None)
def decode_inputs(case, family):
    """(B, H, Hkv, Sq, Smax, kv_len) -> bf16 q [B,H,Sq,D], k, v [B,Hkv,Smax,D] with NaN in every cache row at or
    past kv_len[b], int32 kv_len, and the float64 reference in the form ``A.check`` takes.  ``peaked``: as the
    ladder family of test_attention_ref, but key 64 t + 5 of every 64-key tile t carries the score PEAKS[t % 7],
    some 30 log2 units above the others' 0.18 rms: tiles of different waves and splits hold the row's weight."""
    B, H, Hkv, Sq, Smax, lens = case
    g = A._gen("decode", case, family)
    q, k, v = (torch.randn(B, h, s, A.D, generator=g) for h, s in ((H, Sq), (Hkv, Smax), (Hkv, Smax)))
    if family == "peaked":
        c, _ = R.kernel_constants(A.SCALE)
        q = q / 8
        q[..., -2:], k[..., -2:] = 1.0, 0.0
        for t in range(-(-Smax // 64)):
            if 64 * t + 5 < Smax:
                k[:, :, 64 * t + 5, -2], k[:, :, 64 * t + 5, -1] = A._split_bf16(PEAKS[t % 7] / c)
    for b, n in enumerate(lens):
        k[b, :, n:], v[b, :, n:] = float("nan"), float("nan")
    q, k, v, kv_len = A._bf(q), A._bf(k), A._bf(v), torch.tensor(lens, dtype=torch.int32)
    o, lse2, cond = R.attn_decode_ref64(q, k, v, kv_len, A.SCALE)
    assert float(lse2.abs().max()) <= 64.0
    visible = (kv_len.view(B, 1) - Sq + 1 + torch.arange(Sq)).double().view(B, Sq, 1, 1)
    return q, k, v, kv_len, {"o": (o, cond, None, visible), "lse2": lse2}


def test_reference_rows_are_the_last_rows_of_the_causal_reference_on_the_truncated_sequence():
    B, H, Hkv, Sq, Smax, lens = CPU_CASE
    q, k, v, kv_len, ref = decode_inputs(CPU_CASE, "randn")
    for b, n in enumerate(lens):
        qfull = torch.cat([torch.randn(1, H, n - Sq, A.D).bfloat16(), q[b:b + 1]], 2)
        o, lse2, cond = R.attn_fwd_ref64(qfull, k[b:b + 1, :, :n], v[b:b + 1, :, :n], A.SCALE)
        for got, want in ((ref["o"][0][b], o[0, -Sq:]), (ref["lse2"][b], lse2[0, :, -Sq:]), (ref["o"][1][b], cond[0, -Sq:])):
            torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("family", ["randn", "peaked"])
def test_cpu_call_is_the_fp32_reference_and_matches_float64(family):
    q, k, v, kv_len, ref = decode_inputs(CPU_CASE, family)
    o32, lse32 = fused.attention_decode_ref(q.float(), k.float(), v.float(), kv_len, A.SCALE)
    assert o32.dtype == torch.float32 and bool(((o32.double() - ref["o"][0]).abs() <= 1e-5 * ref["o"][1] + 1e-7).all())
    torch.testing.assert_close(lse32.double(), ref["lse2"], rtol=0, atol=1e-4)
    o, lse = fused.attention_decode(q, k, v, kv_len, A.SCALE, kv_splits=3, return_lse=True, check=True)
    want = fused.attention_decode_ref(q, k, v, kv_len, A.SCALE)
    assert o.dtype == torch.bfloat16 and torch.equal(o, want[0]) and torch.equal(lse, want[1])
    assert torch.equal(fused.attention_decode(q, k, v, kv_len, A.SCALE), o)


def test_decode_splits_for_fills_the_chip_without_starving_a_split():
    M = fused.MIN_TILES_PER_DECODE_SPLIT
    assert fused.decode_splits_for(32, 8, 1 << 20) == 1 and fused.decode_splits_for(1, 8, 64 * 32 * M) == 32
    for B, Hkv, Smax in [(1, 8, 1), (1, 8, 2048), (1, 8, 32768), (8, 8, 8192), (1, 1, 1 << 20), (3, 2, 64 * 16 * M - 1), (64, 8, 99)]:
        n, tiles = fused.decode_splits_for(B, Hkv, Smax), -(-Smax // 64)
        assert n in (1, 2, 4, 8, 16, 32, 64) and (n == 1 or (tiles // n >= M and B * Hkv * n // 2 < 256))
        assert n == 64 or B * Hkv * n >= 256 or tiles // (2 * n) < M  # the smallest that fills, or the bound stopped it


@pytest.mark.parametrize("change,msg", [
    (dict(q=lambda t: t.float()), "q must be a bf16"),
    (dict(q=lambda t: t[..., :64]), "head dim must be 128"),
    (dict(q=lambda t: t[0]), "q must be a bf16"),
    (dict(q=lambda t: t.repeat(1, 1, 6, 1)), r"Sq \* \(H / Hkv\) must be between 1 and 32, got 36"),
    (dict(q=lambda t: t[:, :3]), "must be a multiple of kv heads"),
    (dict(k=lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)), "caches must be contiguous"),
    (dict(v=lambda t: t[:, :, :-1]), "one shape"),
    (dict(kv_len=lambda t: t.long()), "kv_len must be an int32"),
    (dict(kv_len=lambda t: t[:1]), "kv_len must be an int32"),
    (dict(kv_len=lambda t: t.to("meta")), "kv_len must be an int32"),
    (dict(q=lambda t: t.clone().requires_grad_(True)), "forward only"),
    (dict(kv_splits=0), "kv_splits must be 'auto' or an int from 1 to 64"),
    (dict(kv_splits=65), "kv_splits must be 'auto' or an int from 1 to 64"),
    (dict(kv_len=lambda t: t + 14, check=True), r"kv_len must lie in \[3, 150\]"),
    (dict(kv_len=lambda t: t - 1, check=True), r"kv_len must lie in \[3, 150\]"),
])
def test_a_call_that_breaks_a_requirement_is_refused(change, msg):
    q, k, v, kv_len, _ = decode_inputs(CPU_CASE, "randn")
    args = {"q": q, "k": k, "v": v, "kv_len": kv_len}
    kw = {key: val for key, val in change.items() if key not in args}
    args.update({key: fn(args[key]) for key, fn in change.items() if key in args})
    with pytest.raises(ValueError, match=msg):
        fused.attention_decode(args["q"], args["k"], args["v"], args["kv_len"], A.SCALE, **kw)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_decode_kernel_is_built_without_scratch(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa

    st = isa.kernel_stats(os.path.join(REPO, "csrc", "ops", "attention_decode.hip"), out=str(tmp_path / "decode.s"))
    (k,) = [v for name, v in st.items() if "attn_decode_kernel" in name]
    assert k["ScratchSize"] == 0 and k["scratch"] == 0 and k["mfma"] == 64 and k["LDSByteSize"] == 128 * 1024, k
