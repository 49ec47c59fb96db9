"""GPU: the flat Llama-step kernels of csrc/ops/fused_ops.hip (RMSNorm and add+RMSNorm, RoPE+split,
SwiGLU, cross-entropy, the embedding backward), called one by one and compared ELEMENT BY ELEMENT with
the float64 references of models/llama_ref.py.  The transposed and ``*_into`` variants are compared bit
for bit with these flat kernels in tests/test_fused_gpu.py, so the flat kernels are the root of that chain.

An element passes iff it lies within half a bf16 ulp of the exact value plus a derived slack of 2^-18
or 2^-16 times the magnitude of the terms its fp32 arithmetic adds (``assert_rounded_once``); copies
and exact sums must match bit for bit.  The rule, the slacks and their derivation, the inputs and the
case tables (with the launch path each case is there for) live in tests/test_llama_ref.py, which checks
on the CPU that an fp32 emulation passes every case here, that mutants (truncation instead of rounding,
one wrong vector, a dropped row, a shifted table or one-hot, a forgotten eps) fail, and that the slack
term exceeds the rounding term on at most 5 % of any output.

Backward kernels get ``rstd`` / ``lse`` from the REFERENCE (rounded to fp32), not from the forward
kernel: a forward fault cannot leak into a backward comparison.
"""
import pytest
import torch

import test_llama_ref as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from gpu_topology_on_k8s_amd.ops.fused import hip as _hip

    return _hip()


def _d(t):
    return t.cuda().contiguous()


# ------------------------------------------------------------------------------------ RMSNorm
@pytest.mark.parametrize("M,D", L.NORM_CASES)
def test_rmsnorm_forward(hip, M, D):
    """rmsnorm_fwd (y, rstd) and add_rmsnorm_fwd (h bit-exact, y, rstd) with eps = 1e-5; planted rows:
    all zero (y = 0, rstd = eps^-1/2), scaled by 2^-10 (eps dominates) and 2^10, a single non-zero."""
    c = L.norm_case(M, D)
    x, r, w = _d(c["x"]), _d(c["r"]), _d(c["w"])
    got = {}
    got["y"], got["rstd"] = hip.rmsnorm_fwd(x, w, L.EPS)
    got["add.h"], got["add.y"], got["add.rstd"] = hip.add_rmsnorm_fwd(x, r, w, L.EPS)
    assert got["y"].shape == (M, D) and got["rstd"].shape == (M,) and got["rstd"].dtype == torch.float32
    L.check_outputs(f"norm {M}x{D}", c, got)


@pytest.mark.parametrize("M,D", L.NORM_CASES)
def test_rmsnorm_backward(hip, M, D):
    """rmsnorm_bwd and add_rmsnorm_bwd (dx, dW) from the reference's rstd; on the all-zero row
    dx = r dy w.  dW is the sum over all rows: a wave without a row must have written zero partials."""
    c = L.norm_case(M, D)
    dy, x, w, rstd, dres = (_d(c[n]) for n in ("dy", "x", "w", "rstd", "dres"))
    got = {}
    got["dx"], got["dw"] = hip.rmsnorm_bwd(dy, x, w, rstd)
    got["add.dx"], got["add.dw"] = hip.add_rmsnorm_bwd(dy, x, w, rstd, dres)
    L.check_outputs(f"norm {M}x{D}", c, got)


# ------------------------------------------------------------------------------------ RoPE + split
@pytest.mark.parametrize("dims", L.ROPE_CASES)
def test_rope_split_forward_and_backward(hip, dims):
    """rope_split_fwd (q, k rotated at position s + pos_offset, v a bit-exact copy) and rope_split_bwd
    against the float64 inverse rotation at the same, in most cases non-zero, offset."""
    B, S, H, Hkv, Dh, off = dims
    c = L.rope_case(*dims)
    cos, sin = _d(c["cos"]), _d(c["sin"])
    got = dict(zip(("q", "k", "v"), hip.rope_split_fwd(_d(c["qkv"]), cos, sin, B, S, H, Hkv, Dh, off)))
    assert got["q"].shape == (B, H, S, Dh) and got["k"].shape == got["v"].shape == (B, Hkv, S, Dh)
    got["dqkv"] = hip.rope_split_bwd(_d(c["dq"]), _d(c["dk"]), _d(c["dv"]), cos, sin, off)
    assert got["dqkv"].shape == (B * S, (H + 2 * Hkv) * Dh)
    L.check_outputs(f"rope {dims}", c, got)


def test_rope_split_bwd_t_against_float64(hip):
    """rope_split_bwd_t with a non-zero offset against the same float64 reference (elsewhere it is only
    compared with rope_split_bwd, which shares its rotation body); its second output is the transpose."""
    dims = L.ROPE_T_CASE
    off = dims[5]
    c = L.rope_case(*dims)
    dqkv, dqkv_t = hip.rope_split_bwd_t(_d(c["dq"]), _d(c["dk"]), _d(c["dv"]), _d(c["cos"]), _d(c["sin"]), off)
    L.check_outputs(f"rope_t {dims}", c, {"dqkv": dqkv})
    assert torch.equal(dqkv_t, dqkv.t())


# ------------------------------------------------------------------------------------ SwiGLU
@pytest.mark.parametrize("T,F", L.SWIGLU_CASES)
def test_swiglu_forward_and_backward(hip, T, F):
    """swiglu_fwd and swiglu_bwd; row 0 holds gates +-20, +-80, +-150 and +-0.  The cond of the
    backward's gate half carries a term for the cancellation in 1 + g (1 - sigmoid(g)), derived in
    tests/test_llama_ref.py: with cond = |value| (1 + |g|) alone 16 of the 8,601,600 gate gradients of
    (600, 14336) missed on MI355X, worst err / tol 1.001, all at g = -1.28125 or -1.2734375, the two
    bf16 values next to that factor's zero."""
    c = L.swiglu_case(T, F)
    gu = _d(c["gu"])
    dgu = hip.swiglu_bwd(_d(c["dh"]), gu)
    assert dgu.shape == (T, 2 * F)
    got = {"h": hip.swiglu_fwd(gu), "dgate": dgu[:, :F], "dup": dgu[:, F:]}
    assert got["h"].shape == (T, F)
    L.check_outputs(f"swiglu {T}x{F}", c, got)


# ------------------------------------------------------------------------------------ cross-entropy
@pytest.mark.parametrize("T,V", L.XENT_CASES)
def test_cross_entropy_forward_and_backward(hip, T, V):
    """xent_fwd (lse, loss rows) and xent_bwd_inplace with gscale 0.37 from the reference's lse.  Labels
    0, V - 1, ignore_index, V and -7 (the last three: loss 0 and an all-zero gradient row); rows with all
    logits equal, with one +80 among -80, and with whole vectors of -inf."""
    c = L.xent_case(T, V)
    labels = _d(c["labels"])
    loss, lse = hip.xent_fwd(_d(c["logits"]), labels, L.IGNORE)
    assert loss.dtype == lse.dtype == torch.float32
    g = _d(c["logits"])
    hip.xent_bwd_inplace(g, labels, _d(c["lse"]), _d(c["gscale"]), L.IGNORE)
    L.check_outputs(f"xent {T}x{V}", c, {"lse": lse, "loss_rows": loss, "dlogits": g})
    ignored = [i for i, y in enumerate(c["labels"].tolist()) if y == L.IGNORE or y < 0 or y >= V]
    assert T < 4 or ignored
    assert not loss[ignored].any() and not g[ignored].any()


def test_cross_entropy_bwd_t_against_float64(hip):
    """xent_bwd_t against the same reference; all three kinds of ignored label are present."""
    T, V = L.XENT_T_CASE
    c = L.xent_case(T, V)
    assert {L.IGNORE, V, -7} <= set(c["labels"].tolist())
    g = _d(c["logits"])
    g_t = hip.xent_bwd_t(g, _d(c["labels"]), _d(c["lse"]), _d(c["gscale"]), L.IGNORE)
    L.check_outputs(f"xent_t {T}x{V}", c, {"dlogits": g})
    assert torch.equal(g_t, g.t())


# ------------------------------------------------------------------------------------ embedding backward
@pytest.mark.parametrize("V,D,T", L.EMBED_CASES)
@pytest.mark.parametrize("integer", [True, False], ids=["integer", "randn"])
def test_embedding_backward(hip, V, D, T, integer):
    """embed_bwd_into into a buffer prefilled with 7.0: rows no token owns still hold 7.0, ids outside
    [0, V) are skipped.  Integer dx: every sum is exact, the result equals bf16_round(sum) bit for bit
    (a 2000-position segment included); randn dx: the rule with RED."""
    c = L.embed_case(V, D, T, integer)
    if T > 1:
        tok = c["tok"].tolist()
        assert tok.count(7) >= 2000 and {0, V - 1, -1, V, V + 5} <= set(tok) and not bool(c["owned"].all())
    srt, perm = torch.sort(c["tok"], stable=True)
    out = torch.full((V, D), L.EMBED_FILL, dtype=torch.bfloat16, device="cuda")
    hip.embed_bwd_into(_d(srt), _d(perm), _d(c["dx"]), out)
    L.check_outputs(f"embed {V}x{D}x{T}", c, {"dW": out})


# ------------------------------------------------------------------------------------ argument checks
# Every input below is one for which the kernel, launched without the check, would still have stayed
# inside every buffer: neither this tree nor one without the checks can read or write out of bounds.
def _bf(*shape):
    return torch.ones(*shape, dtype=torch.bfloat16, device="cuda")


def _f32(*shape):
    return torch.ones(*shape, dtype=torch.float32, device="cuda")


def test_swiglu_bwd_rejects_f_not_multiple_of_8(hip):
    """F = 12: the kernel handles F / 8 vectors per row and would leave 4 columns of dgu unwritten."""
    with pytest.raises(RuntimeError, match="multiple of 16"):
        hip.swiglu_bwd(_bf(2, 12), _bf(2, 24))


def test_rmsnorm_bwd_rejects_wide_rows_and_mismatched_weight(hip):
    """D = 8200 > 8192 (columns past 8192 of dx would stay unwritten) and a w that is too long."""
    with pytest.raises(RuntimeError, match="rmsnorm_bwd: D must be"):
        hip.rmsnorm_bwd(_bf(2, 8200), _bf(2, 8200), _bf(8200), _f32(2))
    with pytest.raises(RuntimeError, match="rmsnorm_bwd: D must be"):
        hip.rmsnorm_bwd(_bf(2, 64), _bf(2, 64), _bf(72), _f32(2))
    with pytest.raises(RuntimeError, match="rmsnorm_bwd: D must be"):
        hip.add_rmsnorm_bwd(_bf(2, 64), _bf(2, 64), _bf(72), _f32(2), _bf(2, 64))


def test_xent_bwd_rejects_bad_vocabulary_and_entry_counts(hip):
    """V = 12 (not a multiple of 8); lse or labels with more than T entries; logits that are not [T, V]."""
    labels = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 8"):
        hip.xent_bwd_inplace(_bf(4, 12), labels, _f32(4), _f32(1), -100)
    with pytest.raises(RuntimeError, match="T entries"):
        hip.xent_bwd_inplace(_bf(4, 16), labels, _f32(5), _f32(1), -100)
    with pytest.raises(RuntimeError, match="T entries"):
        hip.xent_bwd_inplace(_bf(3, 16), labels, _f32(3), _f32(1), -100)
    with pytest.raises(RuntimeError, match=r"\[T, V\]"):
        hip.xent_bwd_inplace(_bf(2, 2, 16), labels, _f32(4), _f32(1), -100)


def test_rope_split_bwd_rejects_dk_with_other_head_count(hip):
    """dk with 1 head where dv has 2, but with more elements: the kernel takes the head count from dk
    and would read a third of dk and half of dv."""
    from gpu_topology_on_k8s_amd.ops.fused import rope_tables

    cos, sin = rope_tables(16, 32, device="cuda")
    with pytest.raises(RuntimeError, match="rope_split_bwd: shapes"):
        hip.rope_split_bwd(_bf(1, 4, 8, 32), _bf(1, 1, 24, 32), _bf(1, 2, 8, 32), cos, sin, 0)
