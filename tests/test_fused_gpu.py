"""HIP fused kernels vs plain PyTorch fp32 references (run on a real MI355X: ``pytest -m gpu``).

The AdamW tests here form a chain: the tile kernel, the ranges kernel, the device form and the non-finite tests
compare with the flat kernel (``adamw_step``) bit for bit or at a stated tolerance.  The root of that chain is
tests/test_gpu_adamw_exact.py, which holds the flat kernel element by element to the float64 reference of
models/optim_ref.py and runs every launch loop on a second trip; ``_flat_adamw_against_torch`` below applies the
same rule (tests/test_optim_ref.py ``assert_adamw``) to this file's own inputs."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "needs a GPU"
    from gpu_topology_on_k8s_amd.ops.fused import hip as load_hip

    return load_hip()  # raises (fails loudly) if the extension is missing


def fused_swiglu_bwd_ref(dh, gu):
    from gpu_topology_on_k8s_amd.ops.fused import swiglu_bwd_ref

    return swiglu_bwd_ref(dh.cpu(), gu.cpu()).cuda()


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@pytest.mark.parametrize("M,D", [(1, 4096), (37, 4096), (513, 4096), (64, 2048), (33, 1000), (8, 8192)])
def test_rmsnorm_fwd_bwd(hip, M, D):
    torch.manual_seed(0)
    x = torch.randn(M, D, device="cuda", dtype=torch.bfloat16)
    w = (torch.rand(D, device="cuda") + 0.5).to(torch.bfloat16)
    dy = torch.randn(M, D, device="cuda", dtype=torch.bfloat16)
    y, rstd = hip.rmsnorm_fwd(x, w, 1e-5)
    xf, wf = x.float().requires_grad_(True), w.float().requires_grad_(True)
    ref = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5) * wf
    assert _rel(y, ref) < 5e-3
    ref.backward(dy.float())
    dx, dw = hip.rmsnorm_bwd(dy, x, w, rstd)
    assert _rel(dx, xf.grad) < 1e-2
    assert _rel(dw, wf.grad) < 1e-2


@pytest.mark.parametrize("M,D", [(1, 4096), (513, 4096), (33, 1000), (8, 8192)])
def test_add_rmsnorm_fwd_bwd(hip, M, D):
    """Fused residual add + RMSNorm vs fp32 autograd of h = x + r, y = rmsnorm(h) * w, with a
    gradient arriving on both outputs (dh from the residual stream, dy from the branch)."""
    torch.manual_seed(2)
    x = torch.randn(M, D, device="cuda", dtype=torch.bfloat16)
    r = torch.randn(M, D, device="cuda", dtype=torch.bfloat16)
    w = (torch.rand(D, device="cuda") + 0.5).to(torch.bfloat16)
    dy = torch.randn(M, D, device="cuda", dtype=torch.bfloat16)
    dh = torch.randn(M, D, device="cuda", dtype=torch.bfloat16)
    h, y, rstd = hip.add_rmsnorm_fwd(x, r, w, 1e-5)
    assert torch.equal(h, x + r)  # bf16 residual stream, bit-identical to the separate add
    xf, rf, wf = (t.float().requires_grad_(True) for t in (x, r, w))
    hf = xf + rf
    ref = hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + 1e-5) * wf
    assert _rel(y, ref) < 5e-3
    torch.autograd.backward([ref, hf], [dy.float(), dh.float()])
    dx, dw = hip.add_rmsnorm_bwd(dy, h, w, rstd, dh)
    assert _rel(dx, xf.grad) < 1e-2 and torch.equal(xf.grad, rf.grad)
    assert _rel(dw, wf.grad) < 1e-2


def test_rmsnorm_weight_grad_is_deterministic(hip):
    """dW is reduced in a fixed order (no atomics): bit-identical launch to launch at the Llama-3-8B
    shape [16384, 4096], and exact against an fp64 column sum of the same bf16 operands to bf16 rounding."""
    torch.manual_seed(3)
    M, D = 16384, 4096
    x = torch.randn(M, D, device="cuda", dtype=torch.bfloat16)
    w = (torch.rand(D, device="cuda") + 0.5).to(torch.bfloat16)
    dy = torch.randn(M, D, device="cuda", dtype=torch.bfloat16)
    _, rstd = hip.rmsnorm_fwd(x, w, 1e-5)
    dws = [hip.rmsnorm_bwd(dy, x, w, rstd)[1] for _ in range(3)]
    assert all(torch.equal(dws[0], d) for d in dws[1:])
    ref = (dy.double() * x.double() * rstd.double()[:, None]).sum(0)
    assert _rel(dws[0], ref) < 4e-3


def test_llama_gradients_accumulate_across_backwards_gpu():
    """Two backwards before zero_grad accumulate, as autograd would: the norm and
    embedding gradients that their kernels write into the flat buffer (Llama.flat_grads) come out
    exactly doubled -- the second pass writes a scratch that is added in, not the slot -- and the
    projection weight gradients (addmm_ into the slot) within bf16 rounding of double."""
    from gpu_topology_on_k8s_amd.models import Llama, LlamaConfig

    cfg = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=2, vocab=1024, ffn_dim=1024, max_seq=512)
    tok = torch.randint(0, cfg.vocab, (2, 256), device="cuda")
    m = Llama(cfg, device="cuda", seed=5)
    assert m.flat_grads and m.flat.direct["tok_emb"] and m.flat.direct["l0.attn_norm"]
    m.flat.zero_grad()
    m(tok, torch.roll(tok, -1, 1)).backward()
    one = m.flat.grad.clone()
    m(tok, torch.roll(tok, -1, 1)).backward()  # no zero_grad
    two = m.flat.grad.clone()
    for n in m.flat.params:
        o, e = m.flat.span(n)
        if n.endswith("norm") or n == "tok_emb":
            assert torch.equal(two[o:e], one[o:e] * 2), n
        else:
            assert torch.allclose(two[o:e].float(), 2 * one[o:e].float(), rtol=2e-2, atol=1e-5), n
    m.flat.zero_grad()
    m(tok, torch.roll(tok, -1, 1)).backward()
    assert torch.equal(m.flat.grad, one)  # zero_grad restarts: the slots are overwritten again


@pytest.mark.parametrize("B,S,H,Hkv,Dh", [(2, 128, 32, 8, 128), (1, 77, 4, 2, 64), (1, 16, 8, 8, 32)])
def test_rope_split_fwd_bwd(hip, B, S, H, Hkv, Dh):
    from gpu_topology_on_k8s_amd.ops.fused import rope_split_ref, rope_tables

    torch.manual_seed(1)
    cos, sin = rope_tables(S + 8, Dh, device="cuda")
    qkv = torch.randn(B * S, (H + 2 * Hkv) * Dh, device="cuda", dtype=torch.bfloat16)
    q, k, v = hip.rope_split_fwd(qkv, cos, sin, B, S, H, Hkv, Dh, 0)
    qr, kr, vr = rope_split_ref(qkv.float(), cos, sin, B, S, H, Hkv, Dh)
    assert _rel(q, qr) < 5e-3 and _rel(k, kr) < 5e-3 and torch.equal(v, vr.to(torch.bfloat16))
    # backward == autograd of the fp32 reference
    x = qkv.float().requires_grad_(True)
    outs = rope_split_ref(x, cos, sin, B, S, H, Hkv, Dh)
    gs = [torch.randn_like(o) for o in outs]
    torch.autograd.backward(outs, gs)
    dqkv = hip.rope_split_bwd(*(g.to(torch.bfloat16).contiguous() for g in gs), cos, sin, 0)
    assert _rel(dqkv, x.grad) < 1e-2
    # offset positions
    q2, _, _ = hip.rope_split_fwd(qkv, cos, sin, B, S, H, Hkv, Dh, 8)
    q2r, _, _ = rope_split_ref(qkv.float(), cos, sin, B, S, H, Hkv, Dh, 8)
    assert _rel(q2, q2r) < 5e-3


@pytest.mark.parametrize("T,F", [(1, 14336), (300, 14336), (17, 64)])
def test_swiglu_fwd_bwd(hip, T, F):
    torch.manual_seed(2)
    gu = torch.randn(T, 2 * F, device="cuda", dtype=torch.bfloat16)
    dh = torch.randn(T, F, device="cuda", dtype=torch.bfloat16)
    x = gu.float().requires_grad_(True)
    g, u = x.chunk(2, dim=-1)
    ref = torch.nn.functional.silu(g) * u
    assert _rel(hip.swiglu_fwd(gu), ref) < 5e-3
    ref.backward(dh.float())
    assert _rel(hip.swiglu_bwd(dh, gu), x.grad) < 1e-2


@pytest.mark.parametrize("T,V", [(5, 128256), (64, 1024), (3, 8)])
def test_cross_entropy_fwd_bwd(hip, T, V):
    torch.manual_seed(3)
    logits = (torch.randn(T, V, device="cuda") * 3).to(torch.bfloat16)
    labels = torch.randint(0, V, (T,), device="cuda")
    labels[0] = -100  # ignored row
    loss_rows, lse = hip.xent_fwd(logits, labels, -100)
    x = logits.float().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(x, labels, ignore_index=-100, reduction="none")
    assert torch.allclose(loss_rows, ref, atol=2e-3, rtol=2e-3)
    assert torch.allclose(lse, torch.logsumexp(logits.float(), -1), atol=1e-3, rtol=1e-4)
    nvalid = (labels != -100).sum()
    ref.sum().div(nvalid).backward()
    g = logits.clone()
    hip.xent_bwd_inplace(g, labels, lse, (1.0 / nvalid.float()).reshape(1), -100)
    assert _rel(g, x.grad) < 1e-2
    assert g[0].float().abs().max() == 0  # ignored row has zero gradient


def test_cross_entropy_autograd_mean(hip):
    from gpu_topology_on_k8s_amd.ops.fused import cross_entropy

    torch.manual_seed(4)
    base = torch.randn(32, 4096, device="cuda")
    labels = torch.randint(0, 4096, (32,), device="cuda")
    a = base.to(torch.bfloat16).requires_grad_(True)
    la = cross_entropy(a * 1, labels)
    la.backward()
    b = base.to(torch.bfloat16).float().requires_grad_(True)
    lb = torch.nn.functional.cross_entropy(b, labels)
    lb.backward()
    assert abs(la.item() - lb.item()) < 1e-3
    assert _rel(a.grad, b.grad) < 1e-2


_ADAMW_KEYS = ("master", "m", "v", "g", "w")


def _flat_adamw_against_torch(hip, n, gdtype):
    """One ``adamw_step`` of n elements under the rule of tests/test_optim_ref.py: m, v and the master against the
    float64 reference of models/optim_ref.py (the master within half an fp32 ulp plus 2^-20 of the step's
    magnitude; the former ``allclose(rtol=1e-5, atol=1e-6)`` against the fp32 torch reference was about 1 % of the
    step), W against the op-by-op fp32 torch reference as before; returns the inputs and the kernel's outputs."""
    from gpu_topology_on_k8s_amd.models.optim_ref import adamw_step_ref
    from test_optim_ref import assert_adamw

    torch.manual_seed(5)
    master = torch.randn(n, device="cuda")
    m = torch.randn(n, device="cuda").abs() * 0.01
    v = torch.randn(n, device="cuda").abs() * 0.001
    g = torch.randn(n, device="cuda", dtype=gdtype)
    w = master.to(torch.bfloat16)
    lr, b1, b2, eps, wd, gs, t = 1e-3, 0.9, 0.95, 1e-8, 0.1, 0.5, 3
    hp = torch.tensor([lr, b1, b2, eps, wd, gs, 1 - b1 ** t, 1 - b2 ** t], device="cuda")
    rm, rv, rp = m.clone(), v.clone(), master.clone()
    gg = g.float() * gs
    rm.mul_(b1).add_(gg, alpha=1 - b1)
    rv.mul_(b2).addcmul_(gg, gg, value=1 - b2)
    rp -= lr * ((rm / (1 - b1 ** t)) / ((rv / (1 - b2 ** t)).sqrt() + eps) + wd * rp)
    before = {k: x.clone() for k, x in zip(_ADAMW_KEYS, (master, m, v, g, w))}
    hip.adamw_step(master, m, v, g, w, hp)
    ref = adamw_step_ref(before["master"], before["m"], before["v"], before["g"], hp)
    assert_adamw(f"adamw_step n={n} {str(gdtype)[6:]}", {"master": master, "m": m, "v": v, "w": w}, ref)
    # W is the kernel's own master rounded once; against torch's op-by-op reference it may differ by
    # one bf16 ulp where an fp32 gradient's update lands next to a rounding boundary (FMA contraction)
    assert torch.equal(w, master.to(torch.bfloat16))
    if gdtype == torch.bfloat16:
        assert torch.equal(w, rp.to(torch.bfloat16))
    else:
        assert (w.float() - rp.to(torch.bfloat16).float()).abs().max() <= 2 ** -7 * rp.abs().max()
    return before, dict(zip(_ADAMW_KEYS, (master, m, v, g, w))), hp


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
def test_adamw_and_sqnorm(hip, gdtype):
    """bf16 gradients, and the fp32 sum a DP reduction in fp32 leaves (parallel/dp.py grad_reduce)."""
    before, _, _ = _flat_adamw_against_torch(hip, 1 << 20, gdtype)
    g = before["g"]
    sq = hip.sq_norm(g)
    assert math.isclose(sq.item(), g.float().pow(2).sum().item(), rel_tol=1e-4)


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", [8, 8 * 257])
def test_adamw_flat_and_single_range_at_the_smallest_sizes(hip, n, gdtype):
    """One vector, and one vector past a block: the flat kernel against the torch reference, and
    ``adamw_step_t`` with no matrix and the single range [0, n] bit for bit against the flat kernel."""
    before, flat, hp = _flat_adamw_against_torch(hip, n, gdtype)
    got = {k: x.clone() for k, x in before.items()}
    mats = torch.zeros(0, 5, dtype=torch.int64, device="cuda")
    ranges = torch.tensor([[0, n]], dtype=torch.int64, device="cuda")
    wt = torch.zeros(8, dtype=torch.bfloat16, device="cuda")
    hip.adamw_step_t(got["master"], got["m"], got["v"], got["g"], got["w"], wt, hp, mats, 0, ranges, n, None, None, 2)
    for k in _ADAMW_KEYS:
        assert torch.equal(got[k], flat[k]), k
    assert not wt.any()


@pytest.mark.parametrize("case", ["clip", "clip_off_in_hp", "no_partials"])
@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", [8 * 257, 1 << 18])
def test_adamw_step_dev_matches_host_form_with_python_hyperparameters(hip, n, gdtype, case):
    """The device-side derivation (clip factor from the partials, 1 - beta^t) against the host form
    fed the same quantities computed in float64.  Integer gradients in [-3, 3]: their sum of squares
    is exact in fp32, so the two differ only by the fp32 sqrtf / powf / division roundings of the
    scalars (the tolerance of test_gpu_mnist.test_fused_dev_optimizer_matches_host_optimizer)."""
    torch.manual_seed(11)
    g = torch.randint(-3, 4, (n,), device="cuda").to(gdtype)
    master = torch.randn(n, device="cuda")
    st = dict(zip(_ADAMW_KEYS, (master, torch.randn(n, device="cuda").abs() * 0.01, torch.randn(n, device="cuda").abs() * 0.001,
                                g, master.to(torch.bfloat16))))
    ref = {k: x.clone() for k, x in st.items()}
    lr, b1, b2, eps, wd, gs, t, clip = 1e-3, 0.9, 0.95, 1e-8, 0.1, 0.5, 3, 1.0
    part = None if case == "no_partials" else hip.sq_norm_parts(g, None)
    hp_dev = torch.tensor([lr, b1, b2, eps, wd, gs, -1.0 if case == "clip_off_in_hp" else clip, 0.0], device="cuda")
    hip.adamw_step_dev(st["master"], st["m"], st["v"], st["g"], st["w"], hp_dev, part, torch.tensor([float(t)], device="cuda"))
    gs_ref = gs
    if case == "clip":
        norm = math.sqrt(g.double().pow(2).sum().item()) * gs
        assert norm > 10 * clip  # the clip is active
        gs_ref = gs * min(1.0, clip / (norm + 1e-6))
    hp = torch.tensor([lr, b1, b2, eps, wd, gs_ref, 1 - b1 ** t, 1 - b2 ** t], dtype=torch.float64).float().cuda()
    hip.adamw_step(ref["master"], ref["m"], ref["v"], ref["g"], ref["w"], hp)
    for k in ("master", "m", "v"):
        assert torch.allclose(st[k], ref[k], rtol=1e-4, atol=1e-6), k
    assert torch.equal(st["w"], st["master"].to(torch.bfloat16))


@pytest.fixture(scope="module")
def ternary():
    """Values from {-1, 0, 1} (every sum of squares an exact integer below 2^24) at a size where the
    1024-block grid runs the four-in-flight loop, the tail loop and a ragged last stride."""
    n = 8 * (5 * 262144 + 777)
    x = torch.randint(-1, 2, (n,), device="cuda", generator=torch.Generator("cuda").manual_seed(13))
    return x, {k: int(x[:k].ne(0).sum().item()) for k in (8, 8 * 257, n)}


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
def test_sum_of_squares_is_exact(hip, ternary, gdtype):
    x, count = ternary
    n = x.numel()
    g = x.to(gdtype)
    assert hip.sq_norm(g).item() == count[n]
    parts = hip.sq_norm_parts(g, None)
    assert parts.shape == (1024,) and parts.dtype == torch.float32 and parts.sum().item() == count[n]
    for k, blocks in ((8, 1), (8 * 257, 2)):
        p = hip.sq_norm_parts(g[:k], None)
        assert p.shape == (blocks,) and p.sum().item() == count[k]
    tick = torch.tensor([6.0], device="cuda")
    assert torch.equal(hip.sq_norm_parts(g, tick), parts)
    assert tick.item() == 7.0
    assert hip.sq_norm(g[:0]).item() == 0.0


def test_sharded_flat_adamw_matches_full_on_gpu():
    """ZeRO-1 optimizer on the HIP kernels: per-shard launches on 8-element-aligned slices of the
    flat buffers (the ranges rank 1 of 4 owns) give bit-identical results to the full update."""
    from types import SimpleNamespace

    from gpu_topology_on_k8s_amd.models.optim import FlatAdamW

    torch.manual_seed(6)
    n = 64 * 1000
    data = torch.randn(n, device="cuda").to(torch.bfloat16)
    grad = torch.randn(n, device="cuda", dtype=torch.bfloat16)
    bounds = [0, 6400, 19200, 44800, n]  # bucket edges (multiples of 64)
    shards = []
    for s, e in zip(bounds, bounds[1:]):
        c = (e - s) // 4
        shards.append((s + c, s + 2 * c))
    full = FlatAdamW(SimpleNamespace(data=data.clone(), grad=grad, numel=n), lr=1e-3)
    part = FlatAdamW(SimpleNamespace(data=data.clone(), grad=grad, numel=n), lr=1e-3, clip_norm=None, shards=shards)
    full.clip_norm = None
    for _ in range(2):
        full.step(grad_scale=0.5)
        part.step(grad_scale=0.5)
    for s, e in shards:
        assert torch.equal(part.flat.data[s:e], full.flat.data[s:e])
    untouched = torch.ones(n, dtype=torch.bool, device="cuda")
    for s, e in shards:
        untouched[s:e] = False
    assert torch.equal(part.flat.data[untouched], data[untouched])
    assert part.state_bytes() * 4 == full.state_bytes()


@pytest.mark.parametrize("R,C", [(64, 64), (128, 4096), (4096, 192), (192, 384), (16384, 6144), (640, 128256)])
def test_transpose_kernel_exact(hip, R, C):
    x = torch.randn(R, C, device="cuda", dtype=torch.bfloat16)
    y = hip.transpose_bf16(x)
    assert y.shape == (C, R) and torch.equal(y, x.t().contiguous())


@pytest.mark.parametrize("T,F", [(64, 64), (192, 128), (256, 14336), (4096, 192), (64, 384), (16384, 256)])
def test_swiglu_bwd_t_matches_bwd_and_transpose(hip, T, F):
    gu = torch.randn(T, 2 * F, device="cuda", dtype=torch.bfloat16)
    dh = torch.randn(T, F, device="cuda", dtype=torch.bfloat16)
    dgu, dgu_t = hip.swiglu_bwd_t(dh, gu, tile=64)
    assert torch.equal(dgu, hip.swiglu_bwd(dh, gu))  # one arithmetic body (swiglu_bwd8) in both kernels
    assert _rel(dgu, fused_swiglu_bwd_ref(dh, gu)) < 1e-2
    assert dgu_t.shape == (2 * F, T) and torch.equal(dgu_t, dgu.t().contiguous())


@pytest.mark.parametrize("T,F", [(64, 64), (256, 512), (16384 // 8, 14336 // 8)])
def test_swiglu_fwd_t_matches_fwd_and_transpose(hip, T, F):
    gu = torch.randn(T, 2 * F, device="cuda", dtype=torch.bfloat16)
    h, ht = hip.swiglu_fwd_t(gu, tile=64)
    ref = hip.swiglu_fwd(gu)
    assert torch.equal(h, ref) and torch.equal(ht, ref.t().contiguous())


@pytest.fixture(scope="module")
def swiglu_flat(hip):
    """(gu, dh, flat forward, flat backward) per F at T = 128, computed once and left unchanged."""
    out = {}
    for F in (192, 256):
        g = torch.Generator(device="cuda").manual_seed(F)
        gu = torch.randn(128, 2 * F, device="cuda", dtype=torch.bfloat16, generator=g)
        dh = torch.randn(128, F, device="cuda", dtype=torch.bfloat16, generator=g)
        out[F] = (gu, dh, hip.swiglu_fwd(gu), hip.swiglu_bwd(dh, gu))
    return out


def test_swiglu_t_tile_widths_agree_with_each_other_and_the_flat_kernels(hip, swiglu_flat):
    gu, dh, h_ref, dgu_ref = swiglu_flat[256]
    for tile in (64, 128):
        h, ht = hip.swiglu_fwd_t(gu, tile=tile)
        assert torch.equal(h, h_ref) and torch.equal(ht, h_ref.t().contiguous()), tile
        dgu, dgut = hip.swiglu_bwd_t(dh, gu, tile=tile)
        assert torch.equal(dgu, dgu_ref) and torch.equal(dgut, dgu_ref.t().contiguous()), tile


def test_swiglu_t_explicit_tile_must_divide_f(hip, swiglu_flat):
    gu, dh, _, _ = swiglu_flat[192]
    with pytest.raises(RuntimeError, match="tile width 128"):
        hip.swiglu_fwd_t(gu, tile=128)
    with pytest.raises(RuntimeError, match="tile width 128"):
        hip.swiglu_bwd_t(dh, gu, tile=128)
    with pytest.raises(RuntimeError, match="tile must be 0, 64 or 128"):
        hip.swiglu_fwd_t(gu, tile=32)


@pytest.mark.parametrize("F", [192, 256])
def test_swiglu_t_auto_tile_matches_the_flat_kernels(hip, swiglu_flat, F):
    """tile=0 (the default): the widest tile that divides F -- 64 at F = 192, 128 at F = 256."""
    gu, dh, h_ref, dgu_ref = swiglu_flat[F]
    h, ht = hip.swiglu_fwd_t(gu)
    assert torch.equal(h, h_ref) and torch.equal(ht, h_ref.t().contiguous())
    dgu, dgut = hip.swiglu_bwd_t(dh, gu, tile=0)
    assert torch.equal(dgu, dgu_ref) and torch.equal(dgut, dgu_ref.t().contiguous())


@pytest.mark.parametrize("T,F", [(64, 128), (256, 512), (16384 // 8, 14336 // 8)])
def test_swiglu_bwd_t128_is_bit_identical(hip, T, F):
    gu = torch.randn(T, 2 * F, device="cuda", dtype=torch.bfloat16)
    dh = torch.randn(T, F, device="cuda", dtype=torch.bfloat16)
    a, at = hip.swiglu_bwd_t(dh, gu, tile=64)
    b, bt = hip.swiglu_bwd_t(dh, gu, tile=128)
    assert torch.equal(a, b) and torch.equal(at, bt)


def test_transpose_wrapper_fallback_shapes():
    from gpu_topology_on_k8s_amd.ops import fused

    x = torch.randn(100, 72, device="cuda", dtype=torch.bfloat16)  # not multiples of 64: torch copy
    assert torch.equal(fused.transpose(x), x.t().contiguous())


def test_llama_nt_layout_matches_native_gpu():
    """NT backward GEMMs (HIP transposes + hipBLASLt NT, W^T written by the optimizer path) vs the
    native layout on the GPU, over two steps with a weight update between; the per-step W^T
    transposes of the round-3 path (persistent_wt=False) give the same bits as the resident W^T."""
    from gpu_topology_on_k8s_amd.models import Llama, LlamaConfig

    cfg = LlamaConfig.tiny()
    tok = torch.randint(0, cfg.vocab, (2, 128), device="cuda")
    grads = {}
    for layout, pwt in (("native", True), ("nt", True), ("nt", False)):
        m = Llama(cfg, device="cuda", seed=3, gemm_layout=layout, persistent_wt=pwt)
        for _ in range(2):  # a weight update between steps: every W^T must follow the new weights
            m.flat.zero_grad()
            m(tok, torch.roll(tok, -1, 1)).backward()
            with torch.no_grad():
                m.flat.data.add_(m.flat.grad, alpha=-1e-2)
        grads[(layout, pwt)] = m.flat.grad.float().clone()
    assert _rel(grads[("nt", True)], grads[("native", True)]) < 1e-2
    assert torch.equal(grads[("nt", False)], grads[("nt", True)])


def test_llama_model_gpu_matches_cpu_reference():
    """Full tiny model: HIP kernels + hipBLASLt on GPU vs the PyTorch reference path on CPU, the whole flat
    gradient and every parameter's own.  ``tiny()`` has head dim 64, so the attention here is torch SDPA, not
    the flash kernel, and ``rope_split_bwd_t`` and the O^T epilogue do not run: the head-dim-128 model is held
    to a float64 reference, parameter by parameter, in tests/test_gpu_llama_model.py."""
    from gpu_topology_on_k8s_amd.models import Llama, LlamaConfig

    cfg = LlamaConfig.tiny()
    gm = Llama(cfg, device="cuda", seed=3)
    cm = Llama(cfg, device="cpu", seed=3)
    cm.flat.data.copy_(gm.flat.data.cpu())
    tok = torch.randint(0, cfg.vocab, (2, 64))
    lg = gm(tok.cuda(), torch.roll(tok, -1, 1).cuda())
    lc = cm(tok, torch.roll(tok, -1, 1))
    assert abs(lg.item() - lc.item()) < 2e-2
    lg.backward()
    lc.backward()
    assert _rel(gm.flat.grad.cpu(), cm.flat.grad) < 5e-2
    for n, p in cm.flat.params.items():
        assert _rel(gm.flat.params[n].grad.cpu(), p.grad) < 5e-2, n


def test_smoke_step_and_training_gpu():
    from gpu_topology_on_k8s_amd.models.llama import smoke_step

    assert math.isfinite(smoke_step("cuda:0"))



def _adamw_t_case(gdtype, seed=7):
    """A flat buffer of 3 matrices (64-multiples) and 2 vectors with alignment gaps, as FlatParams lays
    it out, plus its adamw_step_t plan."""
    from gpu_topology_on_k8s_amd.models.llama import FlatParams

    shapes = [("a", (128,)), ("w1", (192, 256)), ("b", (64,)), ("w2", (64, 512)), ("w3", (256, 768))]
    flat = FlatParams(shapes, "cuda")
    assert flat.enable_transposed(["w1", "w2", "w3"]) == ["w1", "w2", "w3"]
    torch.manual_seed(seed)
    n = flat.numel
    st = {"master": torch.randn(n, device="cuda"), "m": torch.randn(n, device="cuda").abs() * 0.01,
          "v": torch.randn(n, device="cuda").abs() * 0.001, "g": torch.randn(n, device="cuda", dtype=gdtype)}
    st["w"] = st["master"].to(torch.bfloat16)
    return flat, st


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("dev,ahead", [(False, 1), (False, 2), (False, 4), (True, 1)])
def test_adamw_step_t_matches_flat_kernel_and_writes_wt(hip, dev, ahead, gdtype):
    """The tile kernel applies the flat kernel's arithmetic bit for bit (master, m, v, W) and writes
    W^T of every planned matrix; the ranges kernel covers the rest.  Both
    gradient types: bf16, and the fp32 sum of ``--grad-reduce fp32``."""
    flat, st = _adamw_t_case(gdtype)
    mats, tiles, ranges, maxr = flat.adamw_plan()
    assert tiles == 3 * 1 + 1 * 2 + 4 * 3 and ranges.shape[0] >= 2
    ref = {k: v.clone() for k, v in st.items()}
    got = {k: v.clone() for k, v in st.items()}
    wt = torch.full_like(flat.data_t, float("nan"))
    if dev:  # graph form: step count 3, clipping at 1.0 from the gradient's partials
        t = torch.tensor([3.0], device="cuda")
        hp = torch.tensor([1e-3, 0.9, 0.95, 1e-8, 0.1, 0.5, 1.0, 0.0], device="cuda")
        part = hip.sq_norm_parts(st["g"], None)
        hip.adamw_step_dev(ref["master"], ref["m"], ref["v"], ref["g"], ref["w"], hp, part, t)
        hip.adamw_step_t(got["master"], got["m"], got["v"], got["g"], got["w"], wt, hp, mats, tiles, ranges, maxr, part, t, 1)
    else:
        b1, b2, tt = 0.9, 0.95, 3
        hp = torch.tensor([1e-3, b1, b2, 1e-8, 0.1, 0.5, 1 - b1 ** tt, 1 - b2 ** tt], device="cuda")
        hip.adamw_step(ref["master"], ref["m"], ref["v"], ref["g"], ref["w"], hp)
        hip.adamw_step_t(got["master"], got["m"], got["v"], got["g"], got["w"], wt, hp, mats, tiles, ranges, maxr, None, None, ahead)
    for k in ("master", "m", "v", "w"):
        assert torch.equal(got[k], ref[k]), k
    for name in ("w1", "w2", "w3"):
        R, C = flat.shapes[name]
        o, ot = flat.offsets[name], flat.t_offsets[name]
        assert torch.equal(wt[ot:ot + R * C].view(C, R), got["w"][o:o + R * C].view(R, C).t()), name


def test_llama_persistent_wt_is_bit_identical_to_per_step_transposes():
    """Three optimizer steps of the tiny model with W^T kept resident (written by adamw_step_t) and with
    W^T re-made by the transpose kernel every backward: same losses, same weights, same W^T, bit for
    bit; after the first backward no W^T is re-made; a direct in-place write of the weights is seen."""
    from gpu_topology_on_k8s_amd.models import Llama, LlamaConfig
    from gpu_topology_on_k8s_amd.models.optim import FlatAdamW

    cfg = LlamaConfig.tiny()
    tok = torch.randint(0, cfg.vocab, (2, 128), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    runs = {}
    for persistent in (True, False):
        m = Llama(cfg, device="cuda", seed=3, persistent_wt=persistent)
        opt = FlatAdamW(m.flat, lr=1e-3)
        assert opt.fused_t is persistent
        losses = []
        for _ in range(3):
            m.flat.zero_grad()
            loss = m(tok, torch.roll(tok, -1, 1))
            loss.backward()
            m.flat.fill_unwritten()
            opt.step()
            losses.append(loss.item())
        runs[persistent] = (losses, m.flat.data.clone(), m)
    assert runs[True][0] == runs[False][0]
    assert torch.equal(runs[True][1], runs[False][1])
    m = runs[True][2]
    n_mats = len(m.flat.t_offsets)
    assert m.flat.t_refreshes == n_mats  # made once (first backward), then written by the optimizer
    for name in m.flat.t_offsets:
        assert torch.equal(m.flat.weight_t(name), m.flat.params[name].detach().t()), name
    assert m.flat.t_refreshes == n_mats
    with torch.no_grad():
        m.flat.data.mul_(0.5)  # an in-place write the optimizer did not make: W^T is re-made at its next use
    name = next(iter(m.flat.t_offsets))
    assert torch.equal(m.flat.weight_t(name), m.flat.params[name].detach().t()) and m.flat.t_refreshes == n_mats + 1



def test_comm_shadow_holds_its_ctas_for_the_collective_duration(hip):
    """The k-GPU collective's shadow (csrc/ops/comm_shadow.hip): copies exactly the requested bytes and
    does not finish before the collective's duration; with few CTAs it leaves the rest of the GPU to
    a concurrent kernel."""
    src = torch.randint(0, 255, (64 << 20,), dtype=torch.uint8, device="cuda")
    dst = torch.zeros_like(src)
    nb = 48 << 20
    hip.comm_shadow(src, dst, nb, 32, 10.0)  # warm
    torch.cuda.synchronize()
    dst.zero_()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    hip.comm_shadow(src, dst, nb, 32, 2000.0)  # 2 ms
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    copied = nb // 16 // 32 // 16 * 16 * 32 * 16  # whole vectors per workgroup and chunk
    assert torch.equal(dst[:copied], src[:copied]) and not dst[copied + 4096:].any()
    assert 2.0 <= ms < 4.0, ms


def test_comm_shadow_timing_reports_achieved_and_exposed_time(hip):
    """parallel/dp.py CommShadow.timing(): per step, the summed collective time (at least the paced
    target) and the exposed tail when the compute stream waits right after the last launch."""
    from gpu_topology_on_k8s_amd.parallel.dp import CommShadow

    sh = CommShadow(torch.device("cuda", 0), ctas=64, k=8, busbw_gbps=350.0, max_bucket_bytes=16 << 20)
    for _ in range(2):
        sh.launch(16 << 20)
        sh.launch(8 << 20)
        sh.wait()
    t = sh.timing()
    target_ms = sh.micros / 2 / 1e3
    assert t["steps_timed"] == 2
    assert target_ms <= t["achieved_ms_per_step"] < target_ms * 1.5 + 0.2, (t, target_ms)
    # nothing else ran: the whole second collective (at least) is exposed
    assert t["exposed_ms_per_step"] >= 0.9 * ring_ms(8 << 20), t


def ring_ms(nbytes, k=8, busbw=350.0):
    return nbytes * 2 * (k - 1) / k / (busbw * 1e9) * 1e3


def test_training_with_the_default_rccl_cta_cap_initialises_its_communicator():
    """models/train.py passes --comm-ctas N (here parallel/dp.py DEFAULT_COMM_CTAS) to RCCL as
    ncclConfig_t maxCTAs through the process group's options; at world 1 the barrier and the timing
    all-reduce still create the communicator, so the capped config is exercised on one GPU.  (The
    default, auto, picks among capped communicators at world > 1: tests/test_dp_check.py.)"""
    import json
    import os
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, "-m", "gpu_topology_on_k8s_amd.models.train", "--model", "tiny", "--batch", "2",
                        "--seq", "128", "--steps", "2", "--warmup", "1", "--gemm-tuning", "off", "--comm-ctas", "64"],
                       capture_output=True, text=True, timeout=300, cwd=repo, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert r["comm_ctas"] == 64 and r["n_gpus"] == 1 and r["comm_ctas_tuning"] is None


@pytest.mark.parametrize("T,F", [(64, 128), (256, 512), (16384 // 8, 14336 // 8)])
def test_swiglu_fwd_t128_is_bit_identical(hip, T, F):
    """64 x 128-tile forward-with-transpose: h equals swiglu_fwd's bits, h^T its transpose, and the
    64 x 64 tile gives the same pair."""
    gu = torch.randn(T, 2 * F, device="cuda", dtype=torch.bfloat16)
    h, ht = hip.swiglu_fwd_t(gu, tile=128)
    ref = hip.swiglu_fwd(gu)
    assert torch.equal(h, ref) and torch.equal(ht, ref.t().contiguous())
    a, at = hip.swiglu_fwd_t(gu, tile=64)
    assert torch.equal(a, h) and torch.equal(at, ht)


@pytest.mark.parametrize("T,V", [(64, 128), (256, 1024), (512, 128256)])
def test_xent_bwd_t_matches_in_place_backward_and_its_transpose(hip, T, V):
    """csrc/ops/fused_ops.hip xent_bwd_t: the same dlogits bits as xent_bwd_inplace (ignored rows
    included) plus dlogits^T [V, T]."""
    logits = (torch.randn(T, V, device="cuda") * 3).to(torch.bfloat16)
    labels = torch.randint(0, V, (T,), device="cuda")
    labels[::7] = -100
    _, lse = hip.xent_fwd(logits, labels, -100)
    scale = torch.tensor([0.37], device="cuda")
    a = logits.clone()
    hip.xent_bwd_inplace(a, labels, lse, scale, -100)
    b = logits.clone()
    bt = hip.xent_bwd_t(b, labels, lse, scale, -100)
    assert torch.equal(a, b) and torch.equal(bt, a.t().contiguous())
    assert not b[::7].any()


@pytest.mark.parametrize("B,H,Hkv,S", [(1, 4, 2, 128), (2, 8, 2, 512)])
def test_attention_forward_writes_o_transpose(hip, B, H, Hkv, S):
    """attn_fwd_t: O and lse bit-identical to attn_fwd, and O^T [H*D, B*S] is O's exact transpose."""
    q = torch.randn(B, H, S, 128, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hkv, S, 128, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, Hkv, S, 128, device="cuda", dtype=torch.bfloat16)
    o, lse = hip.attn_fwd(q, k, v, 128 ** -0.5)
    o2, lse2, ot = hip.attn_fwd_t(q, k, v, 128 ** -0.5)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    assert torch.equal(ot, o.reshape(B * S, H * 128).t().contiguous())


def test_llama_fused_transposes_are_bit_identical():
    """The transposed activations written by their producers (SwiGLU h^T, attention O^T, RoPE dqkv^T
    and dlogits^T; the backward ones handed on through ops/fused.py offer_t/take_t) give the same
    losses and gradients, bit for bit, as transposing every operand in the backward (the producers
    switched off on the model: FlatParams.producer_xt / Llama.attn_ot)."""
    from gpu_topology_on_k8s_amd.models import Llama, LlamaConfig
    from gpu_topology_on_k8s_amd.ops import fused

    cfg = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=2, vocab=1024, ffn_dim=1024, max_seq=512)
    tok = torch.randint(0, cfg.vocab, (2, 256), device="cuda")
    out = {}
    for producers in (True, False):
        m = Llama(cfg, device="cuda", seed=5)
        assert m.attn_ot and m.flat.producer_xt
        m.flat.producer_xt = m.attn_ot = producers
        losses = []
        for _ in range(2):
            m.flat.zero_grad()
            loss = m(tok, torch.roll(tok, -1, 1))
            loss.backward()
            losses.append(loss.item())
            assert not fused._PENDING_T  # every offered transpose was taken
            with torch.no_grad():
                m.flat.data.add_(m.flat.grad, alpha=-1e-2)
                m.flat.invalidate_t()
        out[producers] = (losses, m.flat.grad.float().clone())
    assert out[True][0] == out[False][0]
    assert torch.equal(out[True][1], out[False][1])


@pytest.mark.parametrize("B,H,Hkv,S", [(1, 4, 2, 64), (2, 8, 2, 256), (4, 32, 8, 512)])
def test_rope_bwd_t_is_bit_identical_and_transposed(hip, B, H, Hkv, S):
    """rope_split_bwd_t: dqkv bit-identical to rope_split_bwd, dqkv^T its exact transpose."""
    from gpu_topology_on_k8s_amd.ops import fused

    cos, sin = fused.rope_tables(S + 8, 128, device="cuda")
    dq = torch.randn(B, H, S, 128, device="cuda", dtype=torch.bfloat16)
    dk = torch.randn(B, Hkv, S, 128, device="cuda", dtype=torch.bfloat16)
    dv = torch.randn(B, Hkv, S, 128, device="cuda", dtype=torch.bfloat16)
    ref = hip.rope_split_bwd(dq, dk, dv, cos, sin, 3)
    got, got_t = hip.rope_split_bwd_t(dq, dk, dv, cos, sin, 3)
    assert torch.equal(got, ref) and torch.equal(got_t, ref.t().contiguous())


def test_norm_backward_into_the_flat_slot_is_bit_identical(hip):
    """rmsnorm_bwd_into / add_rmsnorm_bwd_into: the same dx and dW bits as the allocating kernels, dW
    landing in the given view (a slice of a larger buffer) and nowhere else."""
    M, D = 1024, 4096
    x = torch.randn(M, D, device="cuda", dtype=torch.bfloat16)
    r = torch.randn(M, D, device="cuda", dtype=torch.bfloat16)
    w = (1 + 0.1 * torch.randn(D, device="cuda")).to(torch.bfloat16)
    dy = torch.randn(M, D, device="cuda", dtype=torch.bfloat16)
    dres = torch.randn(M, D, device="cuda", dtype=torch.bfloat16)
    h, _, rstd = hip.add_rmsnorm_fwd(x, r, w, 1e-5)
    buf = torch.full((3 * D,), 7.0, device="cuda", dtype=torch.bfloat16)
    view = buf[D:2 * D]
    dx_ref, dw_ref = hip.add_rmsnorm_bwd(dy, h, w, rstd, dres)
    dx = hip.add_rmsnorm_bwd_into(dy, h, w, rstd, dres, view)
    assert torch.equal(dx, dx_ref) and torch.equal(view, dw_ref)
    assert (buf[:D] == 7).all() and (buf[2 * D:] == 7).all()
    dx_ref, dw_ref = hip.rmsnorm_bwd(dy, h, w, rstd)
    dx = hip.rmsnorm_bwd_into(dy, h, w, rstd, view)
    assert torch.equal(dx, dx_ref) and torch.equal(view, dw_ref)


def test_embedding_backward_into_the_flat_slot(hip):
    """embed_bwd_into: per-token sums of dx rows (repeated tokens, out-of-range ids skipped) match an
    fp32 reference within one bf16 rounding, untouched rows stay zero, and two runs give the same bits."""
    V, D, T = 1000, 512, 4096
    tok = torch.randint(0, 64, (T,), device="cuda")  # many repeats
    tok[::97] = torch.randint(64, V, (tok[::97].numel(),), device="cuda")
    dx = torch.randn(T, D, device="cuda", dtype=torch.bfloat16)
    ref = torch.zeros(V, D, device="cuda").index_add_(0, tok, dx.float())
    outs = []
    for _ in range(2):
        out = torch.zeros(V, D, device="cuda", dtype=torch.bfloat16)
        srt, perm = torch.sort(tok, stable=True)
        hip.embed_bwd_into(srt, perm, dx, out)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    assert torch.allclose(outs[0].float(), ref, rtol=8e-3, atol=1e-2)
    used = torch.zeros(V, dtype=torch.bool, device="cuda")
    used[tok] = True
    assert not outs[0][~used].any()


# -- non-finite and subnormal gradients through the optimizer ---------------------------------
def _bad_values(gdtype):
    """name -> (value, what the sum of squares must be): a NaN, an Inf, and 3e38, whose square overflows."""
    big = torch.tensor(3.0e38, dtype=gdtype).item()
    assert math.isfinite(big) and big > 2.0e38
    return {"nan": (float("nan"), "nan"), "inf": (float("inf"), "inf"), "-inf": (float("-inf"), "inf"), "3e38": (big, "inf")}


def _is(x, what):
    return math.isnan(x) if what == "nan" else x == float("inf")


@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
def test_sum_of_squares_carries_nan_inf_and_overflow(hip, ternary, gdtype):
    """One bad element in the first vector, inside the four-in-flight loop, in the tail loop and in the
    ragged last stride of the 1024-block grid (the strides are 262144 vectors), and at the sizes 8 and
    8 * 257: a NaN makes the sum NaN, an Inf or a square that overflows makes it +Inf, a NaN next to an
    Inf makes it NaN; the step counter advances all the same.  A gradient of subnormals only, whose
    squares all underflow, sums to exactly 0."""
    x, _ = ternary
    n, stride = x.numel(), 262144
    assert n // 8 == 5 * stride + 777
    g = x.to(gdtype)
    spots = {n: [3, 8 * (2 * stride + 12345) + 7, 8 * (4 * stride + 999), 8 * (5 * stride + 776) + 7], 8: [0, 7], 8 * 257: [5, 8 * 255 + 7, 8 * 256]}
    for name, (bad, what) in _bad_values(gdtype).items():
        for k, where in spots.items():
            for i in where:
                old = g[i].item()
                g[i] = bad
                tick = torch.tensor([6.0], device="cuda")
                parts = hip.sq_norm_parts(g[:k], tick)
                assert _is(parts.sum().item(), what) and tick.item() == 7.0, (name, k, i)
                assert int((~torch.isfinite(parts)).sum().item()) == 1  # one block saw it
                assert _is(hip.sq_norm(g[:k]).item(), what), (name, k, i)
                g[i] = old
    for k, where in spots.items():  # a NaN and an Inf in one gradient: NaN
        old = g[where[0]].item(), g[where[-1]].item()
        g[where[0]], g[where[-1]] = float("inf"), float("nan")
        assert math.isnan(hip.sq_norm(g[:k]).item()) and math.isnan(hip.sq_norm_parts(g[:k], None).sum().item())
        g[where[0]], g[where[-1]] = float("nan"), float("-inf")
        assert math.isnan(hip.sq_norm(g[:k]).item()) and math.isnan(hip.sq_norm_parts(g[:k], None).sum().item())
        g[where[0]], g[where[-1]] = old
    assert torch.equal(g, x.to(gdtype))
    # subnormals only: bf16 0x0001 .. 0x007F, fp32 0x00000001 .. 0x007FFFFF, both signs
    i = torch.arange(n, device="cuda")
    if gdtype == torch.bfloat16:  # the sign bit as the most negative integer added to the magnitude
        sub = ((i % 127 + 1) - (i & 1) * 0x8000).to(torch.int16).view(torch.bfloat16)
    else:
        sub = ((i * 2654435761 % 0x7FFFFF + 1) - (i & 1) * 0x80000000).to(torch.int32).view(torch.float32)
    assert sub.float().abs().max().item() < 2.0 ** -126
    for k in (8, 8 * 257, n):
        tick = torch.tensor([1.0], device="cuda")
        parts = hip.sq_norm_parts(sub[:k], tick)
        assert not parts.any() and tick.item() == 2.0
        assert hip.sq_norm(sub[:k]).item() == 0.0


@pytest.mark.parametrize("bad", ["nan", "inf"])
@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n", [8 * 257, 1 << 18])
def test_adamw_step_dev_follows_the_host_form_on_a_non_finite_norm(hip, n, gdtype, bad):
    """Clip on, one NaN or one Inf in the gradient.  The host form gets the factor torch computes in
    ``FlatAdamW.step``.  A NaN norm: the factor is NaN and every element of master, m, v and W is NaN in
    both forms, so the event stays loud.  An Inf norm: the factor is exactly 0; where the gradient is
    finite the forms agree within the bound of the fp32 ``powf`` of the bias corrections, where it is
    Inf (Inf * 0) the elements are NaN in both."""
    torch.manual_seed(11)
    g = torch.randint(-3, 4, (n,), device="cuda").to(gdtype)
    at = n // 2 + 3
    g[at] = float(bad)
    master = torch.randn(n, device="cuda")
    st = dict(zip(_ADAMW_KEYS, (master, torch.randn(n, device="cuda").abs() * 0.01, torch.randn(n, device="cuda").abs() * 0.001,
                                g, master.to(torch.bfloat16))))
    ref = {k: x.clone() for k, x in st.items()}
    lr, b1, b2, eps, wd, gs, t, clip = 1e-3, 0.9, 0.95, 1e-8, 0.1, 0.5, 3, 1.0
    part = hip.sq_norm_parts(g, None)
    hp_dev = torch.tensor([lr, b1, b2, eps, wd, gs, clip, 0.0], device="cuda")
    hip.adamw_step_dev(st["master"], st["m"], st["v"], st["g"], st["w"], hp_dev, part, torch.tensor([float(t)], device="cuda"))
    norm = part.sum().sqrt() * gs
    factor = torch.clamp(clip / (norm + 1e-6), max=1.0) * torch.tensor(gs, dtype=torch.float32, device="cuda")
    hp = torch.tensor([lr, b1, b2, eps, wd, 0.0, 1 - b1 ** t, 1 - b2 ** t], dtype=torch.float64).float().cuda()
    hp[5:6].copy_(factor.reshape(1))
    hip.adamw_step(ref["master"], ref["m"], ref["v"], ref["g"], ref["w"], hp)
    if bad == "nan":
        assert math.isnan(factor.item())
        for k in ("master", "m", "v", "w"):
            assert bool(torch.isnan(ref[k]).all()), ("host", k)
            assert bool(torch.isnan(st[k]).all()), ("dev", k)
        return
    assert factor.item() == 0.0
    hit = torch.isinf(g.float())
    assert int(hit.sum().item()) == 1
    for k in ("master", "m", "v", "w"):
        assert torch.equal(torch.isnan(ref[k]), hit) and torch.equal(torch.isnan(st[k]), hit), k
    for k in ("master", "m", "v"):
        assert torch.allclose(st[k][~hit], ref[k][~hit], rtol=1e-4, atol=1e-6), k
    assert torch.equal(st["w"][~hit], st["master"][~hit].to(torch.bfloat16))


def _poison(g, where, value):
    out = g.clone()
    out[torch.tensor(where, device=g.device)] = value
    return out


def _assert_isolated(got, base, where, bad, what):
    """``got`` (the run with ``bad`` at ``where``) against ``base`` (the run with 1.0 there): a NaN gradient
    makes master, m, v and W NaN at its index; an Inf gradient makes m and v +Inf (they are sums with it)
    and master and W NaN (Inf / Inf); every other element has the other run's bits."""
    idx = torch.tensor(where, device="cuda")
    hit = torch.zeros(base["master"].numel(), dtype=torch.bool, device="cuda")
    hit[idx] = True
    for k in ("master", "m", "v", "w"):
        assert not bool(torch.isfinite(got[k][idx]).any()), (what, k)
        if bad == "nan" or k in ("master", "w"):
            assert bool(torch.isnan(got[k][idx]).all()), (what, k)
        else:
            assert bool((got[k][idx] == float("inf")).all()), (what, k)
        assert bool(torch.isfinite(base[k]).all()), (what, k)
        view = torch.int16 if got[k].dtype == torch.bfloat16 else torch.int32
        assert torch.equal(got[k].view(view)[~hit], base[k].view(view)[~hit]), (what, k)


@pytest.mark.parametrize("bad", ["nan", "inf"])
@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("form", ["host", "dev"])
def test_adamw_flat_isolates_one_bad_gradient_element(hip, form, gdtype, bad):
    """Clip off, n = 8 * 257: a bad element at the first and at the last element of an 8-vector, in the first
    vector, in the last vector of the first block and in the one vector of the second block."""
    n = 8 * 257
    where = [0, 8 * 100, 8 * 100 + 7, 8 * 255 + 7, 8 * 256, n - 1]
    torch.manual_seed(5)
    st = {"master": torch.randn(n, device="cuda"), "m": torch.randn(n, device="cuda").abs() * 0.01,
          "v": torch.randn(n, device="cuda").abs() * 0.001, "g": torch.randn(n, device="cuda", dtype=gdtype)}
    st["w"] = st["master"].to(torch.bfloat16)
    b1, b2, tt = 0.9, 0.95, 3
    runs = {}
    for name, value in (("base", 1.0), ("bad", float(bad))):
        run = {k: x.clone() for k, x in st.items()}
        run["g"] = _poison(st["g"], where, value)
        if form == "dev":
            hp = torch.tensor([1e-3, b1, b2, 1e-8, 0.1, 0.5, -1.0, 0.0], device="cuda")
            hip.adamw_step_dev(run["master"], run["m"], run["v"], run["g"], run["w"], hp, None, torch.tensor([float(tt)], device="cuda"))
        else:
            hp = torch.tensor([1e-3, b1, b2, 1e-8, 0.1, 0.5, 1 - b1 ** tt, 1 - b2 ** tt], device="cuda")
            hip.adamw_step(run["master"], run["m"], run["v"], run["g"], run["w"], hp)
        runs[name] = run
    _assert_isolated(runs["bad"], runs["base"], where, bad, (form, gdtype))


@pytest.mark.parametrize("bad", ["nan", "inf"])
@pytest.mark.parametrize("gdtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("dev,ahead", [(False, 1), (False, 2), (False, 4), (True, 1)])
def test_adamw_step_t_isolates_one_bad_gradient_element_and_its_transpose(hip, dev, ahead, gdtype, bad):
    """Clip off, the plan of ``_adamw_t_case``: a bad element at the first and last element of an 8-vector,
    in the first and last row of a tile (and of the tile next to it), in the last column tile of a
    matrix, and inside both ranges.  W^T is NaN exactly at the transposed positions."""
    flat, st = _adamw_t_case(gdtype)
    mats, tiles, ranges, maxr = flat.adamw_plan()
    o = flat.offsets
    rc = {"w1": [(0, 0), (0, 7), (63, 255), (64, 8), (191, 248)], "w2": [(0, 256), (63, 511)], "w3": [(63, 511), (128, 767), (255, 0)]}
    where = [o[name] + r * flat.shapes[name][1] + c for name, cells in rc.items() for r, c in cells]
    where += [o["a"] + 5, o["a"] + 127, o["b"], o["b"] + 63]
    b1, b2, tt = 0.9, 0.95, 3
    runs, wts = {}, {}
    for name, value in (("base", 1.0), ("bad", float(bad))):
        run = {k: x.clone() for k, x in st.items()}
        run["g"] = _poison(st["g"], where, value)
        wt = torch.zeros_like(flat.data_t)
        if dev:
            hp = torch.tensor([1e-3, b1, b2, 1e-8, 0.1, 0.5, -1.0, 0.0], device="cuda")
            hip.adamw_step_t(run["master"], run["m"], run["v"], run["g"], run["w"], wt, hp, mats, tiles, ranges, maxr, None,
                             torch.tensor([float(tt)], device="cuda"), 1)
        else:
            hp = torch.tensor([1e-3, b1, b2, 1e-8, 0.1, 0.5, 1 - b1 ** tt, 1 - b2 ** tt], device="cuda")
            hip.adamw_step_t(run["master"], run["m"], run["v"], run["g"], run["w"], wt, hp, mats, tiles, ranges, maxr, None, None, ahead)
        runs[name], wts[name] = run, wt
    _assert_isolated(runs["bad"], runs["base"], where, bad, (dev, ahead, gdtype))
    assert int(torch.isnan(wts["bad"]).sum().item()) == sum(len(c) for c in rc.values()) and not bool(torch.isnan(wts["base"]).any())
    for name, cells in rc.items():
        R, C = flat.shapes[name]
        ot = flat.t_offsets[name]
        wt_bad, wt_base = wts["bad"][ot:ot + R * C].view(C, R), wts["base"][ot:ot + R * C].view(C, R)
        w_bad = runs["bad"]["w"][o[name]:o[name] + R * C].view(R, C)
        assert torch.equal(wt_bad.view(torch.int16), w_bad.t().contiguous().view(torch.int16)), name
        hit = torch.zeros(C, R, dtype=torch.bool, device="cuda")
        for r, c in cells:
            hit[c, r] = True
        assert torch.equal(torch.isnan(wt_bad), hit), name
        assert torch.equal(wt_bad.view(torch.int16)[~hit], wt_base.view(torch.int16)[~hit]), name
