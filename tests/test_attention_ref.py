"""CPU: the float64 references of models/attention_ref.py, the acceptance rule, and the case table and
input families of tests/test_gpu_attention_exact.py (which imports all of them from here, so the GPU
tests and these self-tests cannot drift apart).

  * each reference equals ``torch.autograd`` of a plain float64 softmax attention;
  * the closed forms of the ``uniform`` family (q = 0): lse2 = log2(i + 1), O = the running mean of V;
  * the rule against itself: an fp32 emulation of the kernels' arithmetic (64-key tiles, the slack-8
    running max, round-to-nearest bf16 packs of P and dS, dK/dV's chains started from -lse/c and
    -delta) passes the rule and the bias check on every (case, family) the GPU tests run, and each of
    eight mutants of that emulation fails at a named case.

The rule is derived in the docstring of models/attention_ref.py.  With u = 2^-8 and N the number of
terms of an element's fp32 chain (the visible keys for O and dQ, G times the visible queries for dK, dV):

    |got - value| <= ulp_bf16(value) / 2 + (u + 2^-24 (N + 64)) cond  [+ 2^-16 cond2 for dq, dk]
    |got - value| <= 2^-15 + 2^-22 |value|                             for lse2 (fp32)

Every case asserts |lse2| <= 64 and ``isfinite`` on all outputs.  On the non-negative family the mean
over a case's elements of (got - value) / cond must lie within 0.25 * 2^-9 of zero for O and dV: with
every term of one sign a truncating pack biases that statistic by more than 2^-9, round to nearest by
a fiftieth of that, which the per-element bound cannot tell apart on signed data.
"""
import functools
import math
import zlib

import pytest
import torch

import test_llama_ref as L
from gpu_topology_on_k8s_amd.models import attention_ref as R
from gpu_topology_on_k8s_amd.models.attention_ref import bf16_round

D = 128
U = 2.0 ** -8
SCALE = 128 ** -0.5
BIAS_CAP = 0.25 * 2.0 ** -9
SLACK = 8.0  # kMaxSlack of the forward

# ================================================================================ the case table
CASES = [  # (B, H, Hkv, S): the launch path the case is there for
    (1, 1, 1, 128),   # one block, every tile peeled, nslice = 4
    (1, 2, 1, 128),   # nslice = 8: both ring tail steps, head wrap inside the ring
    (1, 3, 1, 128),   # nslice = 12: no tail
    (1, 4, 4, 256),   # MHA, the forward main loop runs, key blocks with 8 and 4 slices
    (2, 4, 2, 384),   # forward / dQ id permutation with H no multiple of 8 (B*H = 8), both LDS buffer parities
    (4, 2, 2, 128),   # dK/dV id permutation with B > 1 (B*Hkv = 8)
    (1, 16, 8, 128),  # dK/dV permutation at B = 1
    (1, 8, 1, 256),   # G = 8
    (3, 2, 1, 640),   # identity ids with B > 1, five key blocks with ring remainders 1, 2, 0
    (1, 2, 2, 768),
]
FAMILY_CASES = [(1, 2, 1, 128), (2, 4, 2, 384), (1, 2, 2, 768)]
FAMILIES = ("peaked", "nonneg", "uniform", "ladder", "underflow")
QUARTER = 0.25 * SCALE
RUNS = ([(c, "randn", SCALE) for c in CASES] + [(c, f, SCALE) for f in FAMILIES for c in FAMILY_CASES]
        + [(c, "randn", QUARTER) for c in FAMILY_CASES[:2]])
CHAINED = ((2, 4, 2, 384), "peaked", SCALE)  # the backward once more from the kernel's own forward outputs


def run_id(run):
    (B, H, Hkv, S), fam, scale = run
    return f"{B}x{H}x{Hkv}x{S}-{fam}" + ("" if scale == SCALE else "-quarter")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _bf(t):
    return t.to(torch.bfloat16)


LADDER_TILES = 7  # planted levels 1, 9, .. 49 log2 units: |lse2| stays below 64
UNDERFLOW_LEVEL = -150.0


def _split_bf16(x):
    """x as the sum of two bf16 numbers (relative error 2^-17)."""
    hi = _bf(torch.tensor(x)).float()
    return float(hi), float(_bf(torch.tensor(x) - hi).float())


def make_inputs(dims, family, scale):
    """bf16 CPU q [B,H,S,D], k, v [B,Hkv,S,D], dout [B,S,H,D].

    randn      all four ~ N(0, 1).
    peaked     q times 4: scores of 5.8 log2 units rms, a few keys carry each row.
    nonneg     |q|, |k|, |v|, |dout|: no cancellation in any output but dS, every term of O and dV positive.
    uniform    q = 0: every visible key weighs 1 / (i + 1).
    ladder     the last two dims of q are 1 and of k 0, except one key per 64-key tile t < 7 (position
               64 t + 5) whose last two dims sum to (1 + 8 t) / c: the planted score is 1 + 8 t log2 units.
               The other 126 dims are q ~ N(0, 1) / 8 and k ~ N(0, 1), 0.18 log2 units rms, so a row's
               maximum rises from tile to tile by 8 +- 0.25 (both planted scores carry the noise): just
               under the forward's slack for some rows of a wave (their max stays, P reaches 2^8) and
               just over it for others (O and l are rescaled).  The planted dims are the LAST of the
               score's fp32 chain: a raw score of up to 390 is rounded once at that magnitude, not 128
               times, which is what the lse2 bound's 2^-22 |value| (four roundings) presumes.
    underflow  dim 0 of q is 1; dim 0 of k is 0 for the first half of the keys and -150 / c for the second:
               those scores lie 140 and more log2 units below the row's maximum, 2^x underflows."""
    B, H, Hkv, S = dims
    g = _gen("attn", dims, family, scale)
    q, k = torch.randn(B, H, S, D, generator=g), torch.randn(B, Hkv, S, D, generator=g)
    v, do = torch.randn(B, Hkv, S, D, generator=g), torch.randn(B, S, H, D, generator=g)
    c, _ = R.kernel_constants(scale)
    if family == "peaked":
        q = q * 4
    elif family == "nonneg":
        q, k, v, do = q.abs(), k.abs(), v.abs(), do.abs()
    elif family == "uniform":
        q = torch.zeros_like(q)
    elif family == "ladder":
        q = q / 8
        q[..., -2:], k[..., -2:] = 1.0, 0.0
        for t in range(min(S // 64, LADDER_TILES)):
            k[:, :, 64 * t + 5, -2], k[:, :, 64 * t + 5, -1] = _split_bf16((1.0 + 8.0 * t) / c)
    elif family == "underflow":
        q[..., 0], k[..., 0] = 1.0, 0.0
        k[:, :, S // 2:, 0] = UNDERFLOW_LEVEL / c
    else:
        assert family == "randn", family
    return _bf(q), _bf(k), _bf(v), _bf(do)


def _chain_lengths(dims):
    """N of the rule: (visible keys per query [S], G * visible queries per key [S])."""
    B, H, Hkv, S = dims
    i = torch.arange(S, dtype=torch.float64)
    return i + 1, (H // Hkv) * (S - i)


def backward_refs(c, out, lse):
    """The backward's entries of a case's ``ref`` dict for a given out (bf16) and lse (fp32)."""
    dq, dk, dv, cdq, cdk, cdv, c2dq, c2dk = R.attn_bwd_ref64(c["do"], c["q"], c["k"], c["v"], out, lse, c["scale"])
    nk, nq = _chain_lengths(c["dims"])
    row = lambda n: n.view(1, 1, -1, 1)  # noqa: E731
    return {"dq": (dq, cdq, c2dq, row(nk)), "dk": (dk, cdk, c2dk, row(nq)), "dv": (dv, cdv, None, row(nq))}


@functools.lru_cache(maxsize=None)
def case(dims, family, scale):
    """Inputs and float64 references of one run.  The backward takes out = bf16_round(o_ref) and
    lse = fp32(lse2_ref): a forward fault can neither hide nor cause a backward failure."""
    q, k, v, do = make_inputs(dims, family, scale)
    c = {"dims": dims, "family": family, "scale": scale, "q": q, "k": k, "v": v, "do": do}
    o, lse2, cond_o = R.attn_fwd_ref64(q, k, v, scale)
    assert float(lse2.abs().max()) <= 64.0, float(lse2.abs().max())
    c["out"], c["lse"] = bf16_round(o), lse2.float()
    nk, _ = _chain_lengths(dims)
    c["ref"] = {"o": (o, cond_o, None, nk.view(1, -1, 1, 1)), "lse2": lse2}
    c["ref"].update(backward_refs(c, c["out"], c["lse"]))
    return c


# ================================================================================ the rule
AXES = {"o": ("batch", "query", "head", "dim"), "dq": ("batch", "head", "query", "dim"),
        "dk": ("batch", "kv head", "key", "dim"), "dv": ("batch", "kv head", "key", "dim"),
        "lse2": ("batch", "head", "query")}


def tolerance(value, cond, cond2, n):
    _, e = torch.frexp(value.abs().clamp_min(2.0 ** -126))  # |value| = m 2^e, m in [0.5, 1): ulp = 2^(e - 8)
    tol = torch.ldexp(torch.ones_like(value), e - 9) + (U + 2.0 ** -24 * (n + 64)) * cond
    return tol if cond2 is None else tol + 2.0 ** -16 * cond2


def compare(name, got, ref):
    """-> (bad mask, worst err / tol, mean of (got - value) / cond, report or None) for one output."""
    out = name.split()[-1]
    got = got.detach().cpu()
    if out == "lse2":
        assert got.dtype == torch.float32 and got.shape == ref.shape, (name, got.dtype, tuple(got.shape))
        value, tol, cond = ref, 2.0 ** -15 + 2.0 ** -22 * ref.abs(), None
    else:
        value, cond, cond2, n = ref
        assert got.dtype == torch.bfloat16 and got.shape == value.shape, (name, got.dtype, tuple(got.shape))
        assert bool((cond >= value.abs() * (1 - 1e-12)).all()), name
        tol = tolerance(value, cond, cond2, n)
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    diff = got.double() - value
    err = diff.abs()
    bad = ~(err <= tol)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    bias = float((diff / cond).mean()) if out in ("o", "dv") else 0.0  # both conds are positive sums
    rep = L._report(name, bad, got.double(), value, tol, AXES[out], "outside the rule") if bool(bad.any()) else None
    return bad, float(ratio.max()), bias, rep


def check(name, c, got, refs=None):
    """Assert the rule on every output in ``got`` (and the bias check on the non-negative family);
    prints each worst err / tol and bias first.  -> {output: worst err / tol}."""
    worst, fails = {}, []
    for n, t in got.items():
        bad, w, bias, rep = compare(f"{name} {n}", t, (refs or c["ref"])[n])
        biased = c["family"] == "nonneg" and n in ("o", "dv")
        print(f"{name} {n}: worst err/tol {w:.3f}" + (f", mean (got - value)/cond {bias / 2.0 ** -9:+.3f} * 2^-9" if biased else ""))
        worst[n] = w
        if rep:
            print(rep)
            fails.append(rep)
        if biased and not abs(bias) <= BIAS_CAP:
            fails.append(f"{name} {n}: biased, mean (got - value)/cond = {bias / 2.0 ** -9:+.3f} * 2^-9 (cap 0.25)")
    if fails:
        pytest.fail("\n".join(fails), pytrace=False)
    return worst


# ================================================================================ the fp32 emulation
def _fma(a, b, c):
    """fp32 fma: the product of two fp32 numbers is exact in float64."""
    return (a.double() * b + c.double()).float()


def _pack(t32, trunc):
    return (L.bf16_trunc(t32) if trunc else _bf(t32)).float()


def _rep(t, G):
    return t.repeat_interleave(G, dim=1)


def emulate_fwd(c, mut=()):
    """attn_fwd2_kernel in fp32 torch, all (batch, head) rows at once, one 64-key tile at a time: a tile
    is visible to a 32-query wave iff its first key is (that is, to the queries >= its first key).
    -> (o bf16 [B,S,H,D], lse2 fp32 [B,H,S]).  Mutants: "trunc_p", "ge_half" (k >= q for k > q in the
    mask on lane half 1: keys 4..7 mod 8), "skip_tile2" (the block's second diagonal tile skipped for
    waves 2, 3), "no_rescale" (alpha = 1 when the max moves)."""
    B, H, Hkv, S = c["dims"]
    cc, _ = R.kernel_constants(c["scale"])
    q, k, v = c["q"].float(), _rep(c["k"].float(), H // Hkv), _rep(c["v"].float(), H // Hkv)
    m = torch.full((B, H, S), float("-inf"))
    l, acc = torch.zeros(B, H, S), torch.zeros(B, H, S, D)
    for kt in range(S // 64):
        k0 = 64 * kt
        qi, ki = torch.arange(k0, S).view(-1, 1), torch.arange(k0, k0 + 64).view(1, -1)
        s = q[:, :, k0:] @ k[:, :, k0:k0 + 64].transpose(-1, -2)
        hidden = ki > qi
        if "ge_half" in mut:
            hidden = hidden | ((ki == qi) & (ki % 8 >= 4))
        s = s.masked_fill(hidden, float("-inf"))
        live = torch.ones(S - k0, dtype=torch.bool)
        if "skip_tile2" in mut:  # tile [128 qb + 64, 128 qb + 128) of the queries' own block qb
            live = ~((qi.view(-1) // 128 == k0 // 128) & (k0 % 128 == 64) & (qi.view(-1) % 128 >= 64))
        mo, lo, ao = m[:, :, k0:], l[:, :, k0:], acc[:, :, k0:]
        mrow = s.amax(-1) * cc
        mnew = torch.where(mrow > mo + SLACK, mrow, mo)
        p = torch.exp2(_fma(s, cc, -mnew[..., None]))
        alpha = torch.ones_like(mo) if "no_rescale" in mut else torch.exp2(mo - mnew)
        ln = lo * alpha + p.sum(-1)
        an = ao * alpha[..., None] + _pack(p, "trunc_p" in mut) @ v[:, :, k0:k0 + 64]
        m[:, :, k0:] = torch.where(live, mnew, mo)
        l[:, :, k0:] = torch.where(live, ln, lo)
        acc[:, :, k0:] = torch.where(live[:, None], an, ao)
    return _bf(acc * (1.0 / l)[..., None]).transpose(1, 2).contiguous(), m + torch.log2(l)


def emulate_bwd(c, out=None, lse=None, mut=()):
    """The three backward kernels in fp32 torch -> (dq, dk, dv) bf16.

    pre-kernel: delta = rowsum(dout * out) in fp32, -lse / c as -lse * (1 / c).
    dK/dV: q-head by q-head, 32-query slice by slice: S' = -lse/c + Q K^T, p = 2^(c S'), dS = p (-delta
    + dO V^T), masked above the diagonal, both packed to bf16, dV += P^T dO, dK += dS^T Q in fp32.
    dQ: 64-key tile by tile, p = 2^(fma(s, c, -lse)), dS = p (dO V^T - delta) packed, dQ += dS K.
    Mutants: "trunc_ds", "no_diag_mask" (dK/dV: the mask of the slice on a wave's own diagonal not applied
    for waves >= 1 of a key block), "drop_last" (the last slice's dV/dK products dropped), "delta_raw"
    (``out`` is then the unrounded O the caller passes)."""
    B, H, Hkv, S = c["dims"]
    G = H // Hkv
    cc, sc = R.kernel_constants(c["scale"])
    out = c["out"] if out is None else out
    lse = (c["lse"] if lse is None else lse).float()
    q, k, v = c["q"].float(), c["k"].float(), c["v"].float()
    do = c["do"].float().transpose(1, 2)  # [B, H, S, D]
    delta = (do * out.float().transpose(1, 2)).sum(-1)
    nls = -lse * (torch.tensor(1.0) / torch.tensor(cc))
    trunc = "trunc_ds" in mut
    dk, dv = torch.zeros(B, Hkv, S, D), torch.zeros(B, Hkv, S, D)
    for g in range(G):
        hs = slice(g, H, G)  # q-head hk * G + g of every kv-head hk
        for j in range(S // 32):
            if "drop_last" in mut and g == G - 1 and j == S // 32 - 1:
                continue
            qs, nk = slice(32 * j, 32 * j + 32), 32 * j + 32
            qi, ki = torch.arange(32 * j, nk).view(-1, 1), torch.arange(nk).view(1, -1)
            hidden = ki > qi
            if "no_diag_mask" in mut:
                hidden = hidden & ~((ki >= 32 * j) & (ki % 128 >= 32))
            sp = nls[:, hs, qs, None] + q[:, hs, qs] @ k[:, :, :nk].transpose(-1, -2)
            p = torch.exp2(sp * cc).masked_fill(hidden, 0.0)
            ds = p * (-delta[:, hs, qs, None] + do[:, hs, qs] @ v[:, :, :nk].transpose(-1, -2))
            dv[:, :, :nk] += _pack(p, "trunc_p" in mut).transpose(-1, -2) @ do[:, hs, qs]
            dk[:, :, :nk] += _pack(ds, trunc).transpose(-1, -2) @ q[:, hs, qs]
    kr, vr = _rep(k, G), _rep(v, G)
    dq = torch.zeros(B, H, S, D)
    for kt in range(S // 64):
        k0 = 64 * kt
        qi, ki = torch.arange(k0, S).view(-1, 1), torch.arange(k0, k0 + 64).view(1, -1)
        s = q[:, :, k0:] @ kr[:, :, k0:k0 + 64].transpose(-1, -2)
        p = torch.exp2(_fma(s, cc, -lse[:, :, k0:, None])).masked_fill(ki > qi, 0.0)
        ds = p * (do[:, :, k0:] @ vr[:, :, k0:k0 + 64].transpose(-1, -2) - delta[:, :, k0:, None])
        dq[:, :, k0:] += _pack(ds, trunc) @ kr[:, :, k0:k0 + 64]
    return _bf(dq * sc), _bf(dk * sc), _bf(dv)


def emulate(c, mut=()):
    o, lse2 = emulate_fwd(c, mut)
    raw = R.attn_fwd_ref64(c["q"], c["k"], c["v"], c["scale"])[0] if "delta_raw" in mut else None
    dq, dk, dv = emulate_bwd(c, out=raw, mut=mut)
    return {"o": o, "lse2": lse2, "dq": dq, "dk": dk, "dv": dv}


# ================================================================================ the references
def _plain_attention(q, k, v, factor):
    """softmax(factor QK^T + causal mask) V in float64, q-head h on kv-head h // G -> [B, S, H, D]."""
    G, S = q.shape[1] // k.shape[1], q.shape[2]
    s = factor * (q @ _rep(k, G).transpose(-1, -2))
    s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ _rep(v, G)).transpose(1, 2), torch.logsumexp(s, -1)


@pytest.mark.parametrize("B,H,Hkv,S,scale", [(1, 2, 1, 8, 0.3), (2, 6, 2, 24, SCALE)])
def test_references_are_autograd_of_plain_attention(B, H, Hkv, S, scale):
    g = _gen("ag-attn", B, H, Hkv, S)
    q, k, v = (torch.randn(B, h, S, D, generator=g, dtype=torch.float64).requires_grad_(True) for h in (H, Hkv, Hkv))
    do = torch.randn(B, S, H, D, generator=g, dtype=torch.float64)
    cc, sc = R.kernel_constants(scale)
    factor = cc * math.log(2.0)  # the kernel's softmax factor: c is rounded to fp32, scale separately
    o_plain, lse_plain = _plain_attention(q, k, v, factor)
    o, lse2, cond_o = R.attn_fwd_ref64(q.detach(), k.detach(), v.detach(), scale)
    torch.testing.assert_close(o, o_plain.detach(), rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(lse2, lse_plain.detach() / math.log(2.0), rtol=1e-12, atol=1e-14)
    assert bool((cond_o >= o.abs()).all())
    gq, gk, gv = torch.autograd.grad(o_plain, (q, k, v), do)
    dq, dk, dv, cdq, cdk, cdv, c2dq, c2dk = R.attn_bwd_ref64(do, q.detach(), k.detach(), v.detach(), o, lse2, scale)
    # the kernel multiplies dS by fp32(scale), autograd by the softmax factor: compare per unit factor
    torch.testing.assert_close(dq / sc, gq / factor, rtol=1e-10, atol=1e-13)
    torch.testing.assert_close(dk / sc, gk / factor, rtol=1e-10, atol=1e-13)
    torch.testing.assert_close(dv, gv, rtol=1e-10, atol=1e-13)
    for val, cond in ((dq, cdq), (dk, cdk), (dv, cdv), (dq, c2dq), (dk, c2dk)):
        assert bool((cond >= val.abs() * (1 - 1e-12)).all())
    assert abs(sc / factor - 1) < 2.0 ** -22  # two fp32 roundings apart


def test_backward_reference_is_a_function_of_the_out_and_lse_it_is_given():
    c = case((1, 2, 1, 128), "randn", SCALE)
    base = c["ref"]["dq"][0]
    moved = backward_refs(c, c["out"], c["lse"] + 0.5)["dq"][0]  # P scales by 2^-0.5 (lse + 0.5 is rounded to fp32)
    torch.testing.assert_close(moved, base * 2.0 ** -0.5, rtol=1e-5, atol=1e-9)
    assert not torch.equal(backward_refs(c, _bf(c["out"].float() * 1.5), c["lse"])["dq"][0], base)


@pytest.mark.parametrize("dims", FAMILY_CASES)
def test_uniform_family_closed_forms(dims):
    c = case(dims, "uniform", SCALE)
    B, H, Hkv, S = dims
    o, lse2 = c["ref"]["o"][0], c["ref"]["lse2"]
    n = torch.arange(1, S + 1, dtype=torch.float64)
    torch.testing.assert_close(lse2, torch.log2(n).expand(B, H, S), rtol=0, atol=1e-13)
    mean = _rep(c["v"].double(), H // Hkv).cumsum(2) / n.view(1, 1, S, 1)
    torch.testing.assert_close(o, mean.transpose(1, 2), rtol=1e-12, atol=1e-14)


def _running_max_events(c):
    """From the reference scores (log2 units): per (row, 64-key tile after the row's first) how far the
    tile's maximum lies above the forward's running max m, and whether m moves."""
    B, H, Hkv, S = c["dims"]
    cc, _ = R.kernel_constants(c["scale"])
    s2 = cc * (c["q"].double() @ _rep(c["k"].double(), H // Hkv).transpose(-1, -2))
    s2 = s2.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    tmax = s2.view(B, H, S, S // 64, 64).amax(-1)
    m, rise = tmax[..., 0].clone(), []
    for t in range(1, S // 64):
        rise.append(tmax[..., t] - m)  # -inf where the tile is invisible
        m = torch.where(tmax[..., t] > m + SLACK, tmax[..., t], m)
    return torch.stack(rise, -1)  # [B, H, S, tiles - 1]


@pytest.mark.parametrize("dims", FAMILY_CASES)
def test_ladder_family_takes_both_branches_of_the_max_slack(dims):
    """Maxima that rise by just under 8 (kept: P up to 2^8) and just over 8 (moved: O and l rescaled),
    several times along a row, and both within one 32-query wave at one tile."""
    rise = _running_max_events(case(dims, "ladder", SCALE))
    under, over = (rise > 7.0) & (rise <= SLACK), (rise > SLACK) & (rise < 9.0)
    assert int(under.sum()) >= 30 and int(over.sum()) >= 30, (int(under.sum()), int(over.sum()))
    B, H, S, Tm = rise.shape
    wu, wo = under.view(B, H, S // 32, 32, Tm).any(3), over.view(B, H, S // 32, 32, Tm).any(3)
    assert int((wu & wo).sum()) >= 1  # some rows of a wave move and others do not
    if S >= 384:
        assert int((rise > SLACK).sum(-1).max()) >= 2  # one row rescales more than once


@pytest.mark.parametrize("dims", FAMILY_CASES)
def test_underflow_family_has_keys_140_log2_units_below_the_row_max(dims):
    c = case(dims, "underflow", SCALE)
    B, H, Hkv, S = dims
    cc, _ = R.kernel_constants(SCALE)
    s2 = cc * (c["q"].double() @ _rep(c["k"].double(), H // Hkv).transpose(-1, -2))
    late = s2[:, :, S // 2:, S // 2:]
    rowmax = s2[:, :, S // 2:, :S // 2].amax(-1, keepdim=True)
    assert float((late - rowmax).max()) <= -140.0


def test_rule_tolerance_terms():
    value = torch.tensor([1.0, -3.0, 0.0], dtype=torch.float64)
    cond, n = torch.tensor([2.0, 3.0, 1.0], dtype=torch.float64), torch.tensor([1.0, 64.0, 192.0], dtype=torch.float64)
    tol = tolerance(value, cond, None, n)
    want = [2.0 ** -8 + (U + 2.0 ** -24 * 65) * 2, 2.0 ** -7 + (U + 2.0 ** -24 * 128) * 3, 2.0 ** -134 + (U + 2.0 ** -24 * 256)]
    assert tol.tolist() == want
    assert tolerance(value, cond, cond, n).tolist() == [w + 2.0 ** -16 * float(x) for w, x in zip(want, cond)]
    ref = (value.view(1, 1, 3, 1), cond.view(1, 1, 3, 1), None, n.view(1, 1, 3, 1))
    ok = _bf(torch.tensor([1.0078125, -3.0, 0.0])).view(1, 1, 3, 1)
    assert compare("t dv", ok, ref)[3] is None
    bad, _, _, rep = compare("t dv", _bf(torch.tensor([1.015625, -3.0, 0.0078125])).view(1, 1, 3, 1), ref)
    assert bad.view(-1).tolist() == [True, False, True] and "key: 2 distinct, [0, 2]" in rep
    lse = torch.tensor([[[10.0, -3.0]]], dtype=torch.float64)
    assert compare("t lse2", (lse + 2.0 ** -16).float(), lse)[3] is None
    assert compare("t lse2", (lse + 2.0 ** -14).float(), lse)[0].view(-1).tolist() == [True, True]


# ================================================================================ the rule against itself
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_emulation_passes_the_rule_and_the_bias_check(run):
    c = case(*run)
    worst = check(run_id(run), c, emulate(c))
    assert worst["lse2"] < 0.2  # the fp32 emulation stays below 5e-6 of the 3e-5 bound


def _mutant(run, mut):
    c = case(*run)
    return c, {n: compare(f"{mut} {n}", t, c["ref"][n]) for n, t in emulate(c, (mut,)).items()}


def _failed(res):
    return sorted(n for n, (bad, _, _, rep) in res.items() if rep is not None)


def _touched(bad, dim):
    return bad.nonzero()[:, dim].unique().tolist()


PEAKED_384 = ((2, 4, 2, 384), "peaked", SCALE)
NONNEG_768 = ((1, 2, 2, 768), "nonneg", SCALE)


def test_mutant_truncated_p_pack_fails_per_element_on_peaked_and_by_bias_on_nonneg():
    c, res = _mutant(PEAKED_384, "trunc_p")
    assert _failed(res) == ["dv", "o"] and int(res["o"][0].sum()) >= 100 and int(res["dv"][0].sum()) >= 100
    c, res = _mutant(NONNEG_768, "trunc_p")
    assert -1.6 * 2.0 ** -9 < res["o"][2] < -1.0 * 2.0 ** -9, res["o"][2] / 2.0 ** -9
    with pytest.raises(pytest.fail.Exception, match="biased"):
        check("trunc_p", c, {"o": emulate_fwd(c, ("trunc_p",))[0]})


def test_mutant_truncated_ds_pack_fails_on_peaked_dq_and_dk():
    c, res = _mutant(PEAKED_384, "trunc_ds")
    assert _failed(res) == ["dk", "dq"]
    assert int(res["dq"][0].sum()) >= 100 and int(res["dk"][0].sum()) >= 100


def test_mutant_causal_ge_on_one_lane_half_fails_on_the_rows_that_lose_their_diagonal():
    c, res = _mutant(((1, 1, 1, 128), "randn", SCALE), "ge_half")
    assert _failed(res) == ["lse2", "o"]
    rows = _touched(res["o"][0], 1)
    assert rows and all(r % 8 >= 4 for r in rows) and 4 in rows and 5 in rows  # early rows: the diagonal weighs most
    assert all(r % 8 >= 4 for r in _touched(res["lse2"][0], 2))


def test_mutant_second_diagonal_tile_skipped_for_waves_2_and_3_fails_there_only():
    c, res = _mutant(((1, 4, 4, 256), "randn", SCALE), "skip_tile2")
    assert _failed(res) == ["lse2", "o"]
    rows = _touched(res["o"][0], 1)
    assert rows and all(r % 128 >= 64 for r in rows) and any(r < 128 for r in rows) and any(r >= 128 for r in rows)
    assert len(_touched(res["lse2"][0], 2)) >= 100


@pytest.mark.parametrize("run,seen", [(((1, 2, 1, 128), "ladder", SCALE), True), (PEAKED_384, True),
                                       (((2, 4, 2, 384), "randn", SCALE), False)])
def test_mutant_rescale_skipped_is_seen_by_ladder_and_peaked_only(run, seen):
    c, res = _mutant(run, "no_rescale")
    assert _failed(res) == (["lse2", "o"] if seen else []), _failed(res)


def test_mutant_diagonal_slice_unmasked_for_waves_1_to_3_fails_on_their_keys():
    c, res = _mutant(((1, 2, 1, 128), "randn", SCALE), "no_diag_mask")
    assert _failed(res) == ["dk", "dv"]
    for n in ("dk", "dv"):
        keys = _touched(res[n][0], 2)
        assert keys and min(keys) >= 32, (n, keys[:8])


def test_mutant_last_slice_products_dropped_fails_on_dk_and_dv():
    c, res = _mutant(((1, 3, 1, 128), "randn", SCALE), "drop_last")
    assert _failed(res) == ["dk", "dv"]
    assert int(res["dv"][0].sum()) >= 1000 and int(res["dk"][0].sum()) >= 1000


def test_mutant_delta_from_unrounded_o_fails_on_nonneg():
    """On non-negative inputs delta = sum(dO * O) has 128 terms of one sign: O's rounding moves it by
    2^-9 / sqrt(128) relative, far above the 2^-16 the rule grants the difference dP - delta."""
    c, res = _mutant(((1, 2, 1, 128), "nonneg", SCALE), "delta_raw")
    assert set(_failed(res)) & {"dq", "dk"}, _failed(res)
