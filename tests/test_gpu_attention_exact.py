"""GPU: the flash attention kernels of csrc/ops/attention.hip (forward with and without O^T, the
pre-kernel, dK/dV and dQ behind ``attn_bwd``), called directly and compared ELEMENT BY ELEMENT with the
float64 references of models/attention_ref.py.

An element passes iff |got - value| <= ulp_bf16(value) / 2 + (2^-8 + 2^-24 (N + 64)) cond
(+ 2^-16 cond2 for dq and dk), N the number of terms of its fp32 chain; lse2 iff within
2^-15 + 2^-22 |value|; on non-negative inputs the mean of (got - value) / cond of O and dV stays within
0.25 * 2^-9 of zero (a truncating pack of P gives -1.2 * 2^-9 and worse).  The rule is derived in
models/attention_ref.py.  The case table (one case per launch path: ring tails and head wraps of the
dK/dV slice ring, both workgroup-id permutations with B > 1, G = 1, 2, 3 and 8), the input families
(randn, peaked, non-negative, uniform, a ladder of maxima around the forward's slack of 8, underflowing
keys, a second scale) and the rule itself live in tests/test_attention_ref.py, which checks on the CPU
that an fp32 emulation of the kernels passes every run here and that eight mutants of it fail.

The backward gets out = bf16_round(o_ref) and lse = fp32(lse2_ref) from the REFERENCE: a forward fault
can neither hide nor cause a backward failure.  One run chains the kernel's own forward outputs.
"""
import pytest
import torch

import test_attention_ref as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from gpu_topology_on_k8s_amd.ops.fused import hip as _hip

    return _hip()


def _d(t):
    return t.cuda().contiguous()


@pytest.mark.parametrize("run", A.RUNS, ids=A.run_id)
def test_attention_forward(hip, run):
    """attn_fwd under the rule; attn_fwd_t gives the same O and lse2 bit for bit, and its O^T
    [H*D, B*S] is O transposed bit for bit."""
    c = A.case(*run)
    B, H, Hkv, S = c["dims"]
    q, k, v = _d(c["q"]), _d(c["k"]), _d(c["v"])
    o, lse2 = hip.attn_fwd(q, k, v, c["scale"])
    assert o.shape == (B, S, H, A.D) and lse2.shape == (B, H, S)
    o_t, lse2_t, ot = hip.attn_fwd_t(q, k, v, c["scale"])
    A.check(A.run_id(run), c, {"o": o, "lse2": lse2})
    assert torch.equal(o_t, o) and torch.equal(lse2_t, lse2)
    assert ot.shape == (H * A.D, B * S) and torch.equal(ot, o.reshape(B * S, H * A.D).t())


@pytest.mark.parametrize("run", A.RUNS, ids=A.run_id)
def test_attention_backward(hip, run):
    """attn_bwd (pre-kernel, dK/dV, dQ) from the reference's rounded O and lse2."""
    c = A.case(*run)
    got = hip.attn_bwd(_d(c["do"]), _d(c["q"]), _d(c["k"]), _d(c["v"]), _d(c["out"]), _d(c["lse"]), c["scale"])
    assert got[0].shape == c["q"].shape and got[1].shape == got[2].shape == c["k"].shape
    A.check(A.run_id(run), c, dict(zip(("dq", "dk", "dv"), got)))


def test_attention_backward_chained_to_the_kernels_own_forward(hip):
    """The backward from the forward kernel's O and lse2 (what training runs), against the reference
    evaluated at exactly those: it is a function of the out and lse2 it is given."""
    c = A.case(*A.CHAINED)
    q, k, v = _d(c["q"]), _d(c["k"]), _d(c["v"])
    o, lse2 = hip.attn_fwd(q, k, v, c["scale"])
    A.check("chained forward", c, {"o": o, "lse2": lse2})
    got = hip.attn_bwd(_d(c["do"]), q, k, v, o, lse2, c["scale"])
    A.check("chained", c, dict(zip(("dq", "dk", "dv"), got)), refs=A.backward_refs(c, o.cpu(), lse2.cpu()))


# ------------------------------------------------------------------------------------ argument checks
# Every rejected tensor holds at least as many bytes as the one expected and every rejected scale is a
# number the kernels would have run to the end with: neither this tree nor one without a check can read
# or write out of bounds.
B_, H_, S_ = 2, 2, 128


def _args():
    bf = lambda *s: torch.ones(*s, dtype=torch.bfloat16, device="cuda")  # noqa: E731
    return {"dout": bf(B_, S_, H_, A.D), "q": bf(B_, H_, S_, A.D), "k": bf(B_, H_, S_, A.D), "v": bf(B_, H_, S_, A.D),
            "out": bf(B_, S_, H_, A.D), "lse": torch.ones(B_, H_, S_, dtype=torch.float32, device="cuda"), "scale": A.SCALE}


def _bwd(hip, **kw):
    a = {**_args(), **kw}
    return hip.attn_bwd(a["dout"], a["q"], a["k"], a["v"], a["out"], a["lse"], a["scale"])


def test_attn_bwd_accepts_the_baseline_arguments(hip):
    dq, dk, dv = _bwd(hip)
    assert dq.shape == (B_, H_, S_, A.D) and all(bool(torch.isfinite(t).all()) for t in (dq, dk, dv))


@pytest.mark.parametrize("name", ["dout", "out"])
def test_attn_bwd_rejects_dout_and_out_of_other_type_order_or_place(hip, name):
    """fp32 (twice the bytes, read as bf16 before), head-major [B, H, S, D] order (same bytes), one
    batch more, a CPU tensor (in pinned memory, which the GPU can address)."""
    good = _args()[name]
    for bad in (good.float(), good.transpose(1, 2).contiguous(), torch.cat([good, good[:1]]), good.cpu().pin_memory()):
        with pytest.raises(RuntimeError, match=r"dout/out must be contiguous bf16 \[B, S, H, D\]"):
            _bwd(hip, **{name: bad})


def test_attn_bwd_rejects_lse_of_other_shape_type_or_place(hip):
    """[B, S, H] order (same bytes), flat, fp64 (twice the bytes), on the CPU (pinned)."""
    good = _args()["lse"]
    for bad in (good.transpose(1, 2).contiguous(), good.reshape(-1), good.double(), good.cpu().pin_memory()):
        with pytest.raises(RuntimeError, match=r"lse must be a contiguous fp32 \[B, H, S\] GPU tensor"):
            _bwd(hip, lse=bad)


@pytest.mark.parametrize("scale", [0.0, -A.SCALE, float("inf"), float("nan"), 1e-60])
def test_attention_rejects_a_scale_that_is_not_finite_and_positive(hip, scale):
    """The forward takes its running max on raw scores, which is only right for c > 0; 1e-60 is
    positive as a double and 0 as the fp32 number the kernels get."""
    a = _args()
    for fn in (hip.attn_fwd, hip.attn_fwd_t):
        with pytest.raises(RuntimeError, match="scale must be finite and greater than 0"):
            fn(a["q"], a["k"], a["v"], scale)
    with pytest.raises(RuntimeError, match="scale must be finite and greater than 0"):
        _bwd(hip, scale=scale)
