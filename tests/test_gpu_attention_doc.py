"""GPU: the document-masked flash attention kernels (``attn_fwd_doc``, ``attn_fwd_t_doc``, ``attn_bwd_doc``)
against the float64 references of models/attention_ref.py under the same mask, element by element under
the rule of tests/test_attention_ref.py, unchanged: N is the causal chain length, which bounds the
document's shorter chain from above.  Layouts and dims are the table of tests/test_attention_doc_ref.py:
whole-tile and whole-slice skips, one-token documents at both ends, boundaries on a 64-key tile edge,
inside a 32-row wave and a 32-key sub-tile and either side of a 128 block edge, a block that skips ten
tiles, sweeps that end early at every ring remainder, G = 3 and 8.  With one document per row, and with
bounds that the clamps bring back to it, the kernels reproduce the causal entry points bit for bit."""
import pytest
import torch

import test_attention_doc_ref as DR
import test_attention_ref as A
from gpu_topology_on_k8s_amd.ops import fused

pytestmark = pytest.mark.gpu
NAMES = ("dq", "dk", "dv")


@pytest.fixture(scope="module")
def hip():
    return fused.hip()


def _d(t):
    return t.cuda().contiguous()


def _bounds(c):
    return fused.doc_bounds(_d(c["doc_start"]))


@pytest.mark.parametrize("family", ["randn", "peaked"])
@pytest.mark.parametrize("layout", list(DR.LAYOUTS))
def test_document_attention_forward_and_backward(hip, layout, family):
    """Forward (with O^T: the same O and lse2, O^T the transpose, bit for bit) and the backward from the
    reference's rounded out and lse2; on ``one`` all of it equals the causal entry points bit for bit."""
    c = DR.doc_case(layout, family)
    B, H, Hkv, S = c["dims"]
    q, k, v, do, (ds, de) = _d(c["q"]), _d(c["k"]), _d(c["v"]), _d(c["do"]), _bounds(c)
    o, lse2 = hip.attn_fwd_doc(q, k, v, c["scale"], ds, de)
    o_t, lse2_t, ot = hip.attn_fwd_t_doc(q, k, v, c["scale"], ds, de)
    got = hip.attn_bwd_doc(do, q, k, v, _d(c["out"]), _d(c["lse"]), c["scale"], ds, de)
    name = f"{layout}-{family}"
    A.check(name, c, {"o": o, "lse2": lse2})
    assert torch.equal(o_t, o) and torch.equal(lse2_t, lse2) and torch.equal(ot, o.reshape(B * S, H * A.D).t())
    A.check(name, c, dict(zip(NAMES, got)))
    if layout == "one":
        causal = hip.attn_fwd_t(q, k, v, c["scale"]) + hip.attn_bwd(do, q, k, v, _d(c["out"]), _d(c["lse"]), c["scale"])
        assert all(torch.equal(a, b) for a, b in zip([o, lse2, ot, *got], causal))


def test_document_backward_chained_to_the_kernels_own_forward(hip):
    c = DR.doc_case("ragged", "peaked")
    q, k, v, (ds, de) = _d(c["q"]), _d(c["k"]), _d(c["v"]), _bounds(c)
    o, lse2 = hip.attn_fwd_doc(q, k, v, c["scale"], ds, de)
    A.check("chained forward", c, {"o": o, "lse2": lse2})
    got = hip.attn_bwd_doc(_d(c["do"]), q, k, v, o, lse2, c["scale"], ds, de)
    A.check("chained", c, dict(zip(NAMES, got)), refs=DR.doc_backward_refs(c, o.cpu(), lse2.cpu()))


def test_fused_attention_with_doc_is_the_three_entry_points_under_autograd(hip):
    c = DR.doc_case("mixed", "randn")
    q, k, v = (_d(c[n]).requires_grad_(True) for n in "qkv")
    doc = _bounds(c)
    o = fused.attention(q, k, v, A.SCALE, doc=doc)
    o2, ot = fused.attention_t(q, k, v, A.SCALE, doc=doc)
    o.backward(_d(c["do"]))
    of, lse2, otf = hip.attn_fwd_t_doc(q.detach(), k.detach(), v.detach(), A.SCALE, *doc)
    want = hip.attn_bwd_doc(_d(c["do"]), q.detach(), k.detach(), v.detach(), of, lse2, A.SCALE, *doc)
    assert torch.equal(o, of) and torch.equal(o2, of) and torch.equal(ot, otf)
    assert all(torch.equal(t.grad, w) for t, w in zip((q, k, v), want))


@pytest.mark.parametrize("starts", [[0], [0, 700, 1999, 2048, 3333]], ids=["one", "five"])
def test_document_attention_is_deterministic_at_the_training_shape(hip, starts):
    """B 2, 32 q / 8 kv heads, S 4096, as tests/test_attention_gpu.py holds the causal kernels: every
    output bit-identical over four launches (a race between a tile's LDS reads and the next tile's
    LDS-DMA, or an unsettled rescale, shows up as launch-to-launch differences)."""
    g = torch.Generator(device="cuda").manual_seed(11)
    q, k, v = (torch.randn(2, h, 4096, A.D, device="cuda", generator=g).bfloat16() for h in (32, 8, 8))
    do = torch.randn(2, 4096, 32, A.D, device="cuda", generator=g).bfloat16()
    doc = fused.doc_bounds(DR.doc_start_of([starts] * 2, 4096).cuda())
    first = None
    for _ in range(4):
        o, lse2 = hip.attn_fwd_doc(q, k, v, A.SCALE, *doc)
        got = (o, lse2, *hip.attn_bwd_doc(do, q, k, v, o, lse2, A.SCALE, *doc))
        first = first or got
        assert all(torch.equal(a, b) for a, b in zip(got, first))


def test_bounds_outside_their_range_are_clamped_to_the_causal_result(hip):
    """doc_start = -5 and doc_end = S + 9 everywhere: clamped to 0 and S, the causal mask."""
    c = A.case((2, 4, 2, 384), "randn", A.SCALE)
    q, k, v, do, out, lse = (_d(c[n]) for n in ("q", "k", "v", "do", "out", "lse"))
    ds = torch.full((2, 384), -5, dtype=torch.int32, device="cuda")
    de = torch.full((2, 384), 384 + 9, dtype=torch.int32, device="cuda")
    got = hip.attn_fwd_t_doc(q, k, v, A.SCALE, ds, de) + hip.attn_bwd_doc(do, q, k, v, out, lse, A.SCALE, ds, de)
    causal = hip.attn_fwd_t(q, k, v, A.SCALE) + hip.attn_bwd(do, q, k, v, out, lse, A.SCALE)
    assert all(torch.equal(a, b) for a, b in zip(got, causal))


def test_document_entry_points_refuse_bounds_of_other_type_shape_or_place(hip):
    """int64 (twice the bytes), [S, B] order (same bytes), one row more, on the CPU (pinned): each at
    least as large as the tensor expected."""
    B, H, S = 2, 2, 128
    q = torch.ones(B, H, S, A.D, dtype=torch.bfloat16, device="cuda")
    o, lse = torch.ones(B, S, H, A.D, dtype=torch.bfloat16, device="cuda"), torch.ones(B, H, S, device="cuda")
    good = torch.zeros(B, S, dtype=torch.int32, device="cuda")
    for bad in (good.long(), good.t().contiguous(), torch.cat([good, good[:1]]), good.cpu().pin_memory()):
        for ds, de in ((bad, good), (good, bad)):
            for call in (lambda: hip.attn_fwd_doc(q, q, q, A.SCALE, ds, de), lambda: hip.attn_fwd_t_doc(q, q, q, A.SCALE, ds, de),
                         lambda: hip.attn_bwd_doc(o, q, q, q, o, lse, A.SCALE, ds, de)):
                with pytest.raises(RuntimeError, match=r"doc_start/doc_end must be contiguous int32 \[B, S\]"):
                    call()
