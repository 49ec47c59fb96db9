"""GPU: split-KV flash attention of a query chunk at an offset into longer K/V (``attn_fwd_qoff_split``,
``attn_bwd_qoff_split``, ``fused.attention(..., q_offset=off, kv_splits=n)``).  The references are those of
tests/test_gpu_attention_qoff.py (the window of the full causal case in float64) under the unchanged rule of
tests/test_attention_ref.py.  Before every checked call a block of NaNs of the workspace's size goes back to
the caching allocator, so a merge that read an empty split's partial would show."""
import functools

import pytest
import torch

import test_attention_ref as A
from gpu_topology_on_k8s_amd.ops import fused
from test_gpu_attention_qoff import window

pytestmark = pytest.mark.gpu
NAMES = ("dq", "dk", "dv")
CASES = [  # (B, H, Hkv, Sq, Sk, off, n)
    (1, 2, 1, 128, 128, 0, 1),    # one split through the combine
    (1, 2, 1, 128, 128, 0, 2),    # P = 1: the second split empty
    (2, 4, 2, 128, 256, 128, 2),  # one unmasked split and one diagonal split; batch strides that mix Sq and Sk
    (1, 3, 1, 256, 512, 256, 3),  # P = 3 and 4 in one launch: query block 1 has an empty last split, block 0 none; G = 3
    (1, 4, 1, 256, 768, 384, 4),  # P = 4 and 5: splits of 1, 1, 1, 1 and of 2, 2, 1, 0 key blocks
]
LONG = (1, 8, 2, 256, 2048, 1792)  # (B, H, Hkv, Sq, Sk, off): P = 15 and 16
LONGER = (1, 8, 2, 256, 4096, 3840)  # P = 31 and 32: enough key blocks for "auto" to split


@pytest.fixture(scope="module")
def hip():
    return fused.hip()


def poison(n, B, H, Sq):
    """The allocator's next blocks of the two workspace sizes hold NaNs (each tensor is freed at once)."""
    for m in (A.D, 1):
        torch.full((m * n * B * H * Sq,), float("nan"), device="cuda")


@functools.lru_cache(maxsize=None)
def long_inputs(shape):
    B, H, Hkv, Sq, Sk, _ = shape
    g = torch.Generator(device="cuda").manual_seed(12)
    q = torch.randn(B, H, Sq, A.D, device="cuda", generator=g).bfloat16()
    k, v = (torch.randn(B, Hkv, Sk, A.D, device="cuda", generator=g).bfloat16() for _ in range(2))
    return q, k, v, torch.randn(B, Sq, H, A.D, device="cuda", generator=g).bfloat16()


@pytest.mark.parametrize("family", ["randn", "peaked"])
@pytest.mark.parametrize("case", CASES, ids=lambda s: "x".join(map(str, s)))
def test_split_forward_and_backward_against_float64(hip, case, family):
    """o and lse2 of the split forward, and dq, dk, dv of the split backward from the reference's rounded out
    and lse2.  Worst err / tol on an MI355X: see profiles/attn_splitkv/SUMMARY.md."""
    B, H, Hkv, Sq, Sk, off, n = case
    c, x, refs = window(case[:6], family)
    poison(n, B, H, Sq)
    o, lse2 = hip.attn_fwd_qoff_split(x["q"], x["k"], x["v"], A.SCALE, off, n)
    poison(n, B, H, Sq)
    got = hip.attn_bwd_qoff_split(x["do"], x["q"], x["k"], x["v"], x["out"], x["lse"], A.SCALE, off, n)
    A.check("x".join(map(str, case)) + "-" + family, c, {"o": o, "lse2": lse2, **dict(zip(NAMES, got))}, refs=refs)


def test_split_backward_leaves_dk_and_dv_bit_for_bit(hip):
    shape = CASES[3][:6]
    _, x, _ = window(shape, "randn")
    args = (x["do"], x["q"], x["k"], x["v"], x["out"], x["lse"], A.SCALE, shape[5])
    (_, dk, dv), (_, dk0, dv0) = hip.attn_bwd_qoff_split(*args, 3), hip.attn_bwd_qoff(*args)
    assert torch.equal(dk, dk0) and torch.equal(dv, dv0)


def test_split_attention_is_deterministic_and_reads_no_stale_partial(hip):
    """Four launches of forward and backward at n = 4, the workspace the caching allocator's own (poisoned
    before the second and fourth): bit-identical."""
    q, k, v, do = long_inputs(LONG)
    off, first = LONG[5], None
    for i in range(4):
        if i & 1:
            poison(4, *LONG[:2], LONG[3])
        o, lse2 = hip.attn_fwd_qoff_split(q, k, v, A.SCALE, off, 4)
        got = (o, lse2, *hip.attn_bwd_qoff_split(do, q, k, v, o, lse2, A.SCALE, off, 4))
        first = first or got
        assert all(torch.equal(a, b) for a, b in zip(got, first))


@pytest.mark.parametrize("kv_splits", [None, 1, 3, "auto"])
def test_fused_attention_dispatches_kv_splits_under_autograd(hip, kv_splits):
    """None is attn_fwd_qoff / attn_bwd_qoff bit for bit, an int the split entry points with that n, "auto"
    those with kv_splits_for's n."""
    B, H, Hkv, Sq, Sk, off = LONGER
    q0, k0, v0, do = long_inputs(LONGER)
    n = fused.kv_splits_for(B, H, Sq, Sk, off) if kv_splits == "auto" else kv_splits
    assert n is None or n >= (2 if kv_splits == "auto" else 1)
    if n is None:
        of, lse2 = hip.attn_fwd_qoff(q0, k0, v0, A.SCALE, off)
        want = hip.attn_bwd_qoff(do, q0, k0, v0, of, lse2, A.SCALE, off)
    else:
        of, lse2 = hip.attn_fwd_qoff_split(q0, k0, v0, A.SCALE, off, n)
        want = hip.attn_bwd_qoff_split(do, q0, k0, v0, of, lse2, A.SCALE, off, n)
    q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
    o = fused.attention(q, k, v, A.SCALE, q_offset=off, kv_splits=kv_splits)
    o.backward(do)
    assert torch.equal(o, of) and all(torch.equal(t.grad, w) for t, w in zip((q, k, v), want))
    qc, kc, vc = q0[:, :, :128].cpu(), k0[:, :, :256].cpu(), v0[:, :, :256].cpu()  # the CPU accepts and ignores it
    assert torch.equal(fused.attention(qc, kc, vc, A.SCALE, q_offset=128, kv_splits=kv_splits),
                       fused.attention_ref(qc, kc, vc, A.SCALE, q_offset=128))


def test_kv_splits_for_is_a_function_of_the_shapes():
    M = fused.MIN_KEY_BLOCKS_PER_SPLIT
    assert fused.kv_splits_for(1, 32, 2048, 8192, 0) == 1  # 512 blocks fill the chip
    assert fused.kv_splits_for(1, 32, 512, 8192, 0) == fused.kv_splits_for(1, 32, 512, 4096, 0)  # Sk does not enter
    for B, H, Sq, off in [(1, 32, 512, 7680), (1, 32, 1024, 7168), (1, 8, 256, 1792), (1, 32, 512, 0), (2, 32, 512, 3584)]:
        n, blocks, kmax = fused.kv_splits_for(B, H, Sq, off + Sq, off), B * H * Sq // 128, (off + Sq) // 128
        assert n in (1, 2, 4, 8) and (n == 1 or (blocks * n // 2 < 512 and kmax // n >= M))
        assert n == 8 or blocks * n >= 512 or kmax // (2 * n) < M  # the smallest that fills, or the bound stopped it


@pytest.mark.parametrize("how,kw,msg", [
    ("fused", dict(kv_splits=2), "kv_splits needs q_offset"),
    ("fused", dict(kv_splits=2, q_offset=128, doc=True), "kv_splits cannot be combined with doc"),
    ("fused", dict(kv_splits=2, q_offset=128, Dh=64), "kv_splits needs head dim 128"),
    ("fused", dict(kv_splits=0, q_offset=128), "kv_splits must be None, 'auto' or an int from 1 to 16"),
    ("fused", dict(kv_splits=17, q_offset=128), "kv_splits must be None, 'auto' or an int from 1 to 16"),
    ("fused", dict(kv_splits=True, q_offset=128), "kv_splits must be None, 'auto' or an int from 1 to 16"),
    ("fused", dict(kv_splits="many", q_offset=128), "kv_splits must be None, 'auto' or an int from 1 to 16"),
    ("fused_t", dict(kv_splits=2, q_offset=128), "attention_t: kv_splits is not supported"),
    ("hip", dict(n=0, off=128), "kv_splits must be between 1 and 16, got 0"),
    ("hip", dict(n=17, off=128), "kv_splits must be between 1 and 16, got 17"),
    ("hip", dict(n=2, off=64), "q_offset must be a non-negative multiple of 128"),
    ("hip", dict(n=2, off=256), "exceeds the key length"),
    ("hip", dict(n=2, off=128, Dh=64), "q_offset needs head dim 128"),
])
def test_a_kv_splits_call_that_breaks_a_requirement_is_refused(hip, how, kw, msg):
    kw = dict(kw)
    Dh = kw.pop("Dh", A.D)
    q = torch.ones(1, 2, 128, Dh, dtype=torch.bfloat16, device="cuda")
    k = torch.ones(1, 2, 256, Dh, dtype=torch.bfloat16, device="cuda")
    if how == "hip":
        o, lse = torch.ones(1, 128, 2, Dh, dtype=torch.bfloat16, device="cuda"), torch.ones(1, 2, 128, device="cuda")
        for call in (lambda: hip.attn_fwd_qoff_split(q, k, k, A.SCALE, kw["off"], kw["n"]),
                     lambda: hip.attn_bwd_qoff_split(o, q, k, k, o, lse, A.SCALE, kw["off"], kw["n"])):
            with pytest.raises(RuntimeError, match=msg):
                call()
        return
    if kw.pop("doc", None):
        kw["doc"] = fused.doc_bounds(torch.zeros(1, 128, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match=msg):
        (fused.attention if how == "fused" else fused.attention_t)(q, k, k, A.SCALE, **kw)
