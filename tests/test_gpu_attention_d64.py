"""GPU: the head-dim-64 flash attention kernels (csrc/ops/attention_d64_kernels.h) through the six entry
points, element by element under the rule of tests/test_attention_ref.py, unchanged: its N + 64 and
2^-16 cond2 terms were derived for 128-term score chains and bound the 64-term ones from above.  The
float64 references are those of models/attention_ref.py, which takes D from its inputs; the inputs are
the last 64 dims of the existing families at scale 64^-0.5 (the ladder's planted dims are the last two)."""
import functools

import pytest
import torch

import test_attention_doc_ref as DR
import test_attention_ref as A
from gpu_topology_on_k8s_amd.models import attention_ref as R
from gpu_topology_on_k8s_amd.ops import fused

pytestmark = pytest.mark.gpu
NAMES = ("dq", "dk", "dv")
D, SCALE = 64, 64 ** -0.5
DIMS = [  # (B, H, Hkv, S): the launch path of the D = 64 kernels the case is there for
    (1, 1, 1, 128),   # one block: both forward / dQ tiles peeled, 4 slices (one of them dead for waves 1-3)
    (1, 3, 1, 256),   # G = 3: an odd number of slices (the unpaired last step of the two-slot slice ring)
    (2, 4, 2, 384),   # B*H = 8 (id permutation of the forward / dQ), both LDS buffer parities in the main loop
    (1, 16, 8, 128),  # kv-head id permutation of dK/dV at B = 1
    (1, 8, 1, 256),   # G = 8
    (3, 2, 1, 640),   # B > 1 with identity ids, an odd number of blocks
    (1, 2, 2, 768),   # four main-loop tiles in a row, the ladder's seven levels (rescales over both buffers)
]


@functools.lru_cache(maxsize=None)
def case64(dims, family, layout=None):
    """A.case / DR.doc_case at head dim 64: the backward takes bf16_round(o_ref) and fp32(lse2_ref)."""
    q, k, v, do = (t[..., 64:].contiguous() for t in A.make_inputs(dims, family, SCALE))
    c = {"dims": dims, "family": family, "scale": SCALE, "q": q, "k": k, "v": v, "do": do}
    if layout:
        c["doc_start"] = DR.doc_start_of(DR.LAYOUTS[layout][1], dims[3])
    o, lse2, cond_o = R.attn_fwd_ref64(q, k, v, SCALE, c.get("doc_start"))
    assert float(lse2.abs().max()) <= 64.0 and bool(torch.isfinite(o).all())
    c["out"], c["lse"] = A.bf16_round(o), lse2.float()
    c["ref"] = {"o": (o, cond_o, None, A._chain_lengths(dims)[0].view(1, -1, 1, 1)), "lse2": lse2}
    c["ref"].update((DR.doc_backward_refs if layout else A.backward_refs)(c, c["out"], c["lse"]))
    return c


@pytest.fixture(scope="module")
def hip():
    return fused.hip()


def _d(t):
    return t.cuda().contiguous()


def _same(got, want):
    return len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))


def _causal(hip, c):
    q, k, v, do = (_d(c[n]) for n in ("q", "k", "v", "do"))
    return hip.attn_fwd_t(q, k, v, SCALE) + hip.attn_bwd(do, q, k, v, _d(c["out"]), _d(c["lse"]), SCALE)


@pytest.mark.parametrize("family", ["randn", "peaked", "ladder"])
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "x".join(map(str, d)))
def test_causal_forward_and_backward(hip, dims, family):
    c = case64(dims, family)
    B, H, Hkv, S = dims
    q, k, v = _d(c["q"]), _d(c["k"]), _d(c["v"])
    o, lse2 = hip.attn_fwd(q, k, v, SCALE)
    assert o.shape == (B, S, H, D)
    o_t, lse2_t, ot, *got = _causal(hip, c)
    A.check(f"{dims}-{family}", c, {"o": o, "lse2": lse2})
    assert torch.equal(o_t, o) and torch.equal(lse2_t, lse2) and torch.equal(ot, o.reshape(B * S, H * D).t())
    A.check(f"{dims}-{family}", c, dict(zip(NAMES, got)))


@pytest.mark.parametrize("family", ["randn", "peaked"])
@pytest.mark.parametrize("layout", list(DR.LAYOUTS))
def test_document_forward_and_backward(hip, layout, family):
    c = case64(DR.LAYOUTS[layout][0], family, layout)
    B, H, Hkv, S = c["dims"]
    q, k, v, do = (_d(c[n]) for n in ("q", "k", "v", "do"))
    ds, de = fused.doc_bounds(_d(c["doc_start"]))
    o, lse2 = hip.attn_fwd_doc(q, k, v, SCALE, ds, de)
    o_t, lse2_t, ot = hip.attn_fwd_t_doc(q, k, v, SCALE, ds, de)
    got = hip.attn_bwd_doc(do, q, k, v, _d(c["out"]), _d(c["lse"]), SCALE, ds, de)
    A.check(f"{layout}-{family}", c, {"o": o, "lse2": lse2})
    assert torch.equal(o_t, o) and torch.equal(lse2_t, lse2) and torch.equal(ot, o.reshape(B * S, H * D).t())
    A.check(f"{layout}-{family}", c, dict(zip(NAMES, got)))
    if layout == "one":
        assert _same([o, lse2, ot, *got], _causal(hip, c))


def test_bounds_outside_their_range_are_clamped_to_the_causal_result(hip):
    """doc_start = -5 and doc_end = S + 9 everywhere: clamped to 0 and S, the causal mask."""
    c = case64((2, 4, 2, 384), "randn")
    q, k, v, do, out, lse = (_d(c[n]) for n in ("q", "k", "v", "do", "out", "lse"))
    ds = torch.full((2, 384), -5, dtype=torch.int32, device="cuda")
    de = torch.full((2, 384), 384 + 9, dtype=torch.int32, device="cuda")
    got = hip.attn_fwd_t_doc(q, k, v, SCALE, ds, de) + hip.attn_bwd_doc(do, q, k, v, out, lse, SCALE, ds, de)
    assert _same(got, _causal(hip, c))


def test_document_backward_chained_to_the_kernels_own_forward(hip):
    c = case64(DR.LAYOUTS["ragged"][0], "peaked", "ragged")
    q, k, v = _d(c["q"]), _d(c["k"]), _d(c["v"])
    ds, de = fused.doc_bounds(_d(c["doc_start"]))
    o, lse2 = hip.attn_fwd_doc(q, k, v, SCALE, ds, de)
    A.check("chained forward", c, {"o": o, "lse2": lse2})
    got = hip.attn_bwd_doc(_d(c["do"]), q, k, v, o, lse2, SCALE, ds, de)
    A.check("chained", c, dict(zip(NAMES, got)), refs=DR.doc_backward_refs(c, o.cpu(), lse2.cpu()))


@pytest.mark.parametrize("masked", [False, True], ids=["causal", "doc"])
def test_fused_attention_is_the_entry_points_under_autograd(hip, masked):
    c = case64(DR.LAYOUTS["mixed"][0], "randn", "mixed")
    q, k, v = (_d(c[n]).requires_grad_(True) for n in "qkv")
    doc = fused.doc_bounds(_d(c["doc_start"])) if masked else None
    o = fused.attention(q, k, v, doc=doc)  # the default scale is 64^-0.5
    o2, ot = fused.attention_t(q, k, v, SCALE, doc=doc)
    o.backward(_d(c["do"]))
    qd, kd, vd = q.detach(), k.detach(), v.detach()
    if masked:
        of, lse2, otf = hip.attn_fwd_t_doc(qd, kd, vd, SCALE, *doc)
        want = hip.attn_bwd_doc(_d(c["do"]), qd, kd, vd, of, lse2, SCALE, *doc)
    else:
        of, lse2, otf = hip.attn_fwd_t(qd, kd, vd, SCALE)
        want = hip.attn_bwd(_d(c["do"]), qd, kd, vd, of, lse2, SCALE)
    assert _same([o, o2, ot], [of, of, otf]) and _same([t.grad for t in (q, k, v)], want)


@pytest.mark.parametrize("starts", [None, [0, 700, 1999, 2048, 3333]], ids=["causal", "five"])
def test_attention_is_deterministic_at_the_1b_training_shape(hip, starts):
    """B 2, 32 q / 8 kv heads, S 4096, D 64: every output bit-identical over four launches (a race
    between a tile's LDS reads and the next tile's LDS-DMA shows up as launch-to-launch differences)."""
    g = torch.Generator(device="cuda").manual_seed(11)
    q, k, v = (torch.randn(2, h, 4096, D, device="cuda", generator=g).bfloat16() for h in (32, 8, 8))
    do = torch.randn(2, 4096, 32, D, device="cuda", generator=g).bfloat16()
    doc = fused.doc_bounds(DR.doc_start_of([starts] * 2, 4096).cuda()) if starts else ()
    fwd, bwd = (hip.attn_fwd_t_doc, hip.attn_bwd_doc) if starts else (hip.attn_fwd_t, hip.attn_bwd)
    first = None
    for _ in range(4):
        o, lse2, ot = fwd(q, k, v, SCALE, *doc)
        got = (o, lse2, ot, *bwd(do, q, k, v, o, lse2, SCALE, *doc))
        first = first or got
        assert _same(got, first)


@pytest.mark.parametrize("packed", [False, True], ids=["causal", "doc"])
def test_model_with_d64_hip_attention_matches_cpu(packed):
    """A head-dim-64 model with ``attn_d64`` on the GPU against the CPU model (float32 attention_ref): loss
    and every parameter's gradient, at the tolerances of tests/test_attention_gpu.py's head-dim-128 test."""
    from gpu_topology_on_k8s_amd.models import Llama, LlamaConfig

    cfg = LlamaConfig(dim=256, n_layers=2, n_heads=4, n_kv_heads=2, vocab=1024, ffn_dim=512, max_seq=512)
    gm = Llama(cfg, device="cuda", seed=5, attn="hip", attn_d64=True)
    cm = Llama(cfg, device="cpu", seed=5)
    cm.flat.data.copy_(gm.flat.data.cpu())
    q, k = (torch.empty(2, h, 128, cfg.head_dim, device="cuda", dtype=torch.bfloat16) for h in (4, 2))
    assert gm.attn_d64 and cfg.head_dim == 64 and fused.flash_attention_supported(q, k, d64=True)
    tok = torch.randint(0, cfg.vocab, (2, 128), generator=A._gen("d64-model"))
    ds = DR.doc_start_of([[0, 37, 64], [0, 100]], 128) if packed else None
    lg = gm(tok.cuda(), torch.roll(tok, -1, 1).cuda(), doc_start=None if ds is None else ds.cuda())
    lc = cm(tok, torch.roll(tok, -1, 1), doc_start=ds)
    assert abs(lg.item() - lc.item()) < 2e-2
    lg.backward()
    lc.backward()
    for n, p in gm.flat.params.items():
        want = cm.flat.params[n].grad.float()
        rel = ((p.grad.cpu().float() - want).norm() / (want.norm() + 1e-12)).item()
        print(f"{n}: rel {rel:.4f}")
        assert rel < 5e-2, (n, rel)


@pytest.mark.parametrize("dh", [32, 96, 256])
def test_other_head_dims_are_refused(hip, dh):
    q = torch.ones(1, 2, 128, dh, dtype=torch.bfloat16, device="cuda")
    o, lse = torch.ones(1, 128, 2, dh, dtype=torch.bfloat16, device="cuda"), torch.ones(1, 2, 128, device="cuda")
    b = torch.zeros(1, 128, dtype=torch.int32, device="cuda")
    for call in (lambda: hip.attn_fwd(q, q, q, SCALE), lambda: hip.attn_fwd_t(q, q, q, SCALE),
                 lambda: hip.attn_bwd(o, q, q, q, o, lse, SCALE), lambda: hip.attn_fwd_doc(q, q, q, SCALE, b, b),
                 lambda: hip.attn_fwd_t_doc(q, q, q, SCALE, b, b), lambda: hip.attn_bwd_doc(o, q, q, q, o, lse, SCALE, b, b)):
        with pytest.raises(RuntimeError, match="head dim must be 64 or 128"):
            call()
    with pytest.raises(ValueError, match="head dim 64 or 128"):
        fused.attention(q, q, q)


def test_flash_attention_supported_needs_the_keyword_at_head_dim_64():
    q = torch.empty(1, 2, 128, 64, dtype=torch.bfloat16, device="cuda")
    assert not fused.flash_attention_supported(q, q) and fused.flash_attention_supported(q, q, d64=True)
    q = torch.empty(1, 2, 128, 128, dtype=torch.bfloat16, device="cuda")
    assert fused.flash_attention_supported(q, q) and fused.flash_attention_supported(q, q, d64=True)
