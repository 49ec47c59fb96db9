"""GPU: causal flash attention for a query chunk at an offset into longer K/V (``attn_fwd_qoff``,
``attn_fwd_t_qoff``, ``attn_bwd_qoff``).  The call on Sq queries at ``off`` is a window of the causal problem
on Sk tokens, so every reference is what tests/test_attention_ref.py builds for the case (B, H, Hkv, Sk),
under its rule, unchanged: the forward's rows off .. off + Sq - 1 with their own cond and chain length, and
for the backward ``backward_refs`` of the full case with dO zeroed outside the window (a row with dO = 0 has
delta = 0 and dP = 0 and adds nothing; the full case's chain length bounds the true one from above).  A key
at or after off + Sq has value 0 and cond 0, which admits an exact zero only."""
import functools

import pytest
import torch

import test_attention_ref as A
from gpu_topology_on_k8s_amd.ops import fused

pytestmark = pytest.mark.gpu
NAMES = ("dq", "dk", "dv")
SHAPES = [  # (B, H, Hkv, Sq, Sk, off)
    (1, 2, 1, 128, 128, 0),    # the degenerate window
    (2, 4, 2, 128, 256, 128),  # one fully visible key block below the diagonal; batch strides that mix Sq and Sk
    (2, 2, 2, 128, 384, 128),  # a key block past the window: zeros written
    (2, 2, 1, 128, 384, 0),    # the window at the top, two dead key blocks
    (1, 3, 1, 256, 512, 256),  # G = 3, two query blocks, ring remainders of the full sweep
    (1, 4, 1, 256, 768, 384),  # six main-loop tiles, G = 4, a dead block after two diagonal ones
]


@pytest.fixture(scope="module")
def hip():
    return fused.hip()


def _d(t):
    return t.cuda().contiguous()


@functools.lru_cache(maxsize=None)
def window(shape, family):
    """-> (inputs of the offset call on the GPU, references of its five outputs) from the full case."""
    B, H, Hkv, Sq, Sk, off = shape
    c = A.case((B, H, Hkv, Sk), family, A.SCALE)
    w = slice(off, off + Sq)
    do0 = torch.zeros_like(c["do"])
    do0[:, w] = c["do"][:, w]
    full = A.backward_refs(dict(c, do=do0), c["out"], c["lse"])
    o, cond, _, n = c["ref"]["o"]
    dq, cdq, c2dq, ndq = full["dq"]
    refs = {"o": (o[:, w], cond[:, w], None, n[:, w]), "lse2": c["ref"]["lse2"][:, :, w],
            "dq": (dq[:, :, w], cdq[:, :, w], c2dq[:, :, w], ndq[:, :, w]), "dk": full["dk"], "dv": full["dv"]}
    for value, cnd, _, _ in (full["dk"], full["dv"]):
        assert not value[:, :, off + Sq:].any() and not cnd[:, :, off + Sq:].any()
    ins = {"q": _d(c["q"][:, :, w]), "k": _d(c["k"]), "v": _d(c["v"]), "do": _d(c["do"][:, w]), "out": _d(c["out"][:, w]),
           "lse": _d(c["lse"][:, :, w])}
    return c, ins, refs


@pytest.mark.parametrize("family", ["randn", "peaked"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_offset_attention_forward_and_backward(hip, shape, family):
    """Forward (with O^T: the same O and lse2, O^T the transpose, bit for bit) and the backward from the
    reference's rounded out and lse2."""
    B, H, Hkv, Sq, Sk, off = shape
    c, x, refs = window(shape, family)
    o, lse2 = hip.attn_fwd_qoff(x["q"], x["k"], x["v"], A.SCALE, off)
    o_t, lse2_t, ot = hip.attn_fwd_t_qoff(x["q"], x["k"], x["v"], A.SCALE, off)
    got = hip.attn_bwd_qoff(x["do"], x["q"], x["k"], x["v"], x["out"], x["lse"], A.SCALE, off)
    name = "x".join(map(str, shape)) + "-" + family
    A.check(name, c, {"o": o, "lse2": lse2}, refs=refs)
    assert torch.equal(o_t, o) and torch.equal(lse2_t, lse2) and torch.equal(ot, o.reshape(B * Sq, H * A.D).t())
    A.check(name, c, dict(zip(NAMES, got)), refs=refs)


def test_whole_window_at_offset_zero_is_the_causal_kernels_bit_for_bit(hip):
    c = A.case((2, 4, 2, 384), "randn", A.SCALE)
    q, k, v, do, out, lse = (_d(c[n]) for n in ("q", "k", "v", "do", "out", "lse"))
    got = hip.attn_fwd_t_qoff(q, k, v, A.SCALE, 0) + hip.attn_bwd_qoff(do, q, k, v, out, lse, A.SCALE, 0)
    causal = hip.attn_fwd_t(q, k, v, A.SCALE) + hip.attn_bwd(do, q, k, v, out, lse, A.SCALE)
    assert all(torch.equal(a, b) for a, b in zip(got, causal))


def test_fused_attention_with_q_offset_is_the_three_entry_points_under_autograd(hip):
    shape = SHAPES[-1]
    off = shape[-1]
    c, x, _ = window(shape, "randn")
    q, k, v = (x[n].clone().requires_grad_(True) for n in "qkv")
    o = fused.attention(q, k, v, A.SCALE, q_offset=off)
    o2, ot = fused.attention_t(q, k, v, A.SCALE, q_offset=off)
    o.backward(x["do"])
    of, lse2, otf = hip.attn_fwd_t_qoff(x["q"], x["k"], x["v"], A.SCALE, off)
    want = hip.attn_bwd_qoff(x["do"], x["q"], x["k"], x["v"], of, lse2, A.SCALE, off)
    assert torch.equal(o, of) and torch.equal(o2, of) and torch.equal(ot, otf)
    assert all(torch.equal(t.grad, w) for t, w in zip((q, k, v), want))
    qc, kc, vc = (x[n].cpu() for n in "qkv")
    cpu = fused.attention(qc, kc, vc, A.SCALE, q_offset=off)
    assert torch.equal(cpu, fused.attention_ref(qc, kc, vc, A.SCALE, q_offset=off))
    torch.testing.assert_close(cpu, fused.attention_ref(c["q"], kc, vc, A.SCALE)[:, off:off + shape[3]])


def test_offset_attention_is_deterministic_at_a_context_parallel_shape(hip):
    """B 2, 32 q / 8 kv heads, the second half of 4096 tokens: every output bit-identical over four launches."""
    g = torch.Generator(device="cuda").manual_seed(11)
    q = torch.randn(2, 32, 2048, A.D, device="cuda", generator=g).bfloat16()
    k, v = (torch.randn(2, 8, 4096, A.D, device="cuda", generator=g).bfloat16() for _ in range(2))
    do = torch.randn(2, 2048, 32, A.D, device="cuda", generator=g).bfloat16()
    first = None
    for _ in range(4):
        o, lse2 = hip.attn_fwd_qoff(q, k, v, A.SCALE, 2048)
        got = (o, lse2, *hip.attn_bwd_qoff(do, q, k, v, o, lse2, A.SCALE, 2048))
        first = first or got
        assert all(torch.equal(a, b) for a, b in zip(got, first))


@pytest.mark.parametrize("Sq,Sk,off,Dh,msg", [
    (128, 256, 64, 128, "q_offset must be a non-negative multiple of 128"),
    (128, 256, -128, 128, "q_offset must be a non-negative multiple of 128"),
    (256, 384, 256, 128, "exceeds the key length"),
    (128, 192, 0, 128, "key length must be a multiple of 128"),
    (128, 256, 128, 64, "q_offset needs head dim 128"),
])
def test_a_window_that_breaks_a_requirement_is_refused(hip, Sq, Sk, off, Dh, msg):
    q = torch.ones(1, 2, Sq, Dh, dtype=torch.bfloat16, device="cuda")
    k = torch.ones(1, 2, Sk, Dh, dtype=torch.bfloat16, device="cuda")
    o, lse = torch.ones(1, Sq, 2, Dh, dtype=torch.bfloat16, device="cuda"), torch.ones(1, 2, Sq, device="cuda")
    for call in (lambda: hip.attn_fwd_qoff(q, k, k, A.SCALE, off), lambda: hip.attn_fwd_t_qoff(q, k, k, A.SCALE, off),
                 lambda: hip.attn_bwd_qoff(o, q, k, k, o, lse, A.SCALE, off)):
        with pytest.raises(RuntimeError, match=msg):
            call()
    for f in (fused.attention, fused.attention_t, fused.attention_ref):
        with pytest.raises(ValueError, match=msg):
            f(q, k, k, A.SCALE, q_offset=off)


def test_doc_with_an_offset_and_an_lse_of_the_key_length_are_refused(hip):
    q = torch.ones(1, 2, 128, A.D, dtype=torch.bfloat16, device="cuda")
    k = torch.ones(1, 2, 256, A.D, dtype=torch.bfloat16, device="cuda")
    o = torch.ones(1, 128, 2, A.D, dtype=torch.bfloat16, device="cuda")
    doc = fused.doc_bounds(torch.zeros(1, 128, dtype=torch.int32, device="cuda"))
    for f in (fused.attention, fused.attention_t):
        with pytest.raises(ValueError, match="q_offset cannot be combined with doc"):
            f(q, k, k, A.SCALE, doc=doc, q_offset=128)
    with pytest.raises(RuntimeError, match=r"lse must be a contiguous fp32 \[B, H, Sq\]"):
        hip.attn_bwd_qoff(o, q, k, k, o, torch.ones(1, 2, 256, device="cuda"), A.SCALE, 128)
