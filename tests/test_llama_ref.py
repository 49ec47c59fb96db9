"""CPU: the float64 references of models/llama_ref.py, the comparison rule ``assert_rounded_once`` and
the case tables of tests/test_gpu_llama_kernels.py (which imports all three from here, so the GPU
tests and these self-tests cannot drift apart).

  * every backward reference equals ``torch.autograd`` of its own forward in float64;
  * the rule against itself: an fp32 torch emulation of each kernel's formula, rounded once to bf16,
    passes every GPU case, and each mutant (truncated rounding, eight wrong columns, a dropped row, a
    shifted RoPE table, the forward's sign, a shifted one-hot, a forgotten eps, a short embedding
    segment) fails and is reported at exactly the indices it touches;
  * the tolerance is not vacuous: per output at most 5 % of the elements have a slack term above the
    half-ulp term (a condition on the inputs of a case).

The rule.  A bf16 output element passes iff |got - ref| <= ulp_bf16(ref) / 2 + slack * cond, an fp32
output element iff |got - ref| <= slack * cond; ``ref`` is the exact float64 value and ``cond`` >= |ref|
the sum of the magnitudes of the terms the fp32 arithmetic adds (|ref| itself where nothing cancels).
The half-ulp term is 2^-9 .. 2^-8 relative, the slacks are at least 2^7 times smaller:

  ELEM = 2^-18  SwiGLU, RoPE, cross-entropy backward: chains of <= 16 fp32 roundings with ``__expf``
                and a division at <= 2 ulp each: <= 32 * 2^-24 = 2^-19, doubled.
                One cond carries a term beyond the magnitude of its value: the gate half of the
                SwiGLU backward, d gate = dh u sg f with f = 1 + g (1 - sg).  f crosses zero at
                g = -1.27846: the sum cancels and its absolute error stays.  Counted from swiglu_bwd8
                with u = 2^-24: e = __expf(-g) <= 5 u relative (argument product |g| u, exp2 2 u, the
                constant), 1 + e <= 5 u, the division 2 ulp = 4 u: sg = 0.218 to 9 u relative = 2 u
                absolute; 1 - sg to 2.5 u; g (1 - sg) ~ -1 to 1.29 * 2.5 u + u = 4.2 u; the final
                1 + (.) is exact.  So cond = |value| (1 + |g|) + |dh u sg| / 8: 8 u = ELEM / 8 of absolute
                error for f, the count doubled.  Gates are bf16 numbers, so |f| >= 0.002786 (g = -1.28125;
                0.005024 at -1.2734375) and the term is at most 19.7 times the first: an effective slack
                below 2^-13.6, under the 2^-12 cap.  Without the term 16 of 8,601,600 gate gradients
                missed on the GPU, all at these two gates (profiles/llama_exact/SUMMARY.md).
  RED  = 2^-16  everything behind a long fp32 reduction (rstd, y, dx, dW of the norms, the embedding
                sums): the longest dependent chain is D / 512 * 8 = 128 adds per lane at D = 8192 plus 6
                shuffle levels; for dW two rows per wave plus 16 and 64 terms in the column sum.
  LSE  = 2^-15  absolute, for lse and the loss rows: at V = 128256 a thread does 63 online merges of
                <= 4 roundings, then 6 shuffle and 3 wave merges: relative error of the sum <= 2^-16 =
                the absolute error of its logarithm, doubled for M + __logf(S).
"""
import functools
import zlib
from typing import NamedTuple, Optional, Tuple

import pytest
import torch

from gpu_topology_on_k8s_amd.models import llama_ref as R
from gpu_topology_on_k8s_amd.models.llama_ref import bf16_round

ELEM, RED, LSE = 2.0 ** -18, 2.0 ** -16, 2.0 ** -15
EPS = 1e-5
IGNORE = -100
GSCALE = 0.37
VACUITY_CAP = 0.05

# ================================================================================ the case tables
NORM_CASES = [  # (M, D): the launch path the case is there for
    (1, 8),        # one vector, three idle waves
    (5, 512),      # NV 1, full
    (3, 520),      # NV 2 with one lane in the second pass
    (33, 1000),    # ragged D
    (7, 4104),     # smallest NV 16
    (4, 8192),     # largest D
    (1023, 64),    # 1024 waves, the last with no row: it must still write zero partials
    (1025, 64),    # wave 0 walks two rows
    (2049, 520),   # wave 0 prefetches twice
]
ROPE_CASES = [  # (B, S, H, Hkv, Dh, pos_offset)
    (1, 3, 1, 1, 16, 0),        # one thread per head
    (3, 5, 3, 1, 48, 2),        # vec_per_head = 3
    (1, 16, 8, 8, 32, 0),       # no grouped heads
    (2, 77, 4, 2, 64, 5),       # odd S with B > 1
    (3, 1111, 32, 4, 128, 1),   # 1,066,560 threads: the grid-stride loop (34 MB)
]
ROPE_T_CASE = (2, 128, 4, 2, 128, 5)  # rope_split_bwd_t (head dim 128, S multiple of 64)
SWIGLU_CASES = [(1, 8), (17, 64), (3, 14336), (600, 14336)]  # the last: 1,075,200 threads, the grid-stride loop
XENT_CASES = [  # (T, V)
    (3, 8),        # one thread
    (4, 2048),     # every thread has exactly one vector
    (4, 2056),     # thread 0 has two
    (5, 128256),   # the Llama-3 vocabulary: 63 vectors per thread
]
XENT_T_CASE = (64, 256)  # xent_bwd_t (T multiple of 64, V of 128)
EMBED_CASES = [(50, 8, 1), (1000, 4096, 4099)]  # (V, D, T): one position; eight passes of the c += 64 loop, ragged last block

SWIGLU_GATES = (20.0, -20.0, 80.0, -80.0, 150.0, -150.0, 0.0, -0.0)  # none in (-104, -88.7): see swiglu_case


class Out(NamedTuple):
    """One kernel output of a case: exact value, condition magnitude (None = |ref|), slack (None = the
    output is a copy or an exact sum and must equal bf16_round(ref) bit for bit), names of its axes."""
    ref: torch.Tensor
    cond: Optional[torch.Tensor]
    slack: Optional[float]
    axes: Tuple[str, ...]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _bf(t):
    return t.to(torch.bfloat16)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ------------------------------------------------------------------------------------ RMSNorm
def _plant_rows(t):
    """Rows 1..4 as far as M allows (row 0 stays ordinary): all zero; scaled by 2^-10 (eps dominates
    mean(x^2)); scaled by 2^10; a single non-zero element."""
    M, D = t.shape
    if M > 1:
        t[1] = 0.0
    if M > 2:
        t[2] *= 2.0 ** -10
    if M > 3:
        t[3] *= 2.0 ** 10
    if M > 4:
        keep = t[4, D // 3].clone()
        t[4] = 0.0
        t[4, D // 3] = keep + 1.0
    return t


@functools.lru_cache(maxsize=None)
def norm_case(M, D):
    """Inputs (bf16, CPU) and references of the four norm kernels.  dy = randn + x / 8 (x before the
    planted scales), so that dW's terms do not cancel to nothing: the vacuity condition on dW.  The
    backward takes the reference's rstd rounded to fp32, and the add-backward the same x and rstd plus
    the residual gradient dres: a forward fault cannot reach a backward comparison."""
    g = _gen("norm", M, D)
    x0, r0 = _randn(g, M, D), _randn(g, M, D)
    c = {"M": M, "D": D}
    c["x"], c["r"] = _bf(_plant_rows(x0.clone())), _bf(_plant_rows(r0.clone()))
    c["w"] = _bf(torch.rand(D, generator=g) + 0.5)
    c["dy"], c["dres"] = _bf(_randn(g, M, D) + 0.125 * x0), _bf(_randn(g, M, D))
    y, rstd = R.rmsnorm_ref(c["x"], c["w"], EPS)
    h, hy, hrstd = R.add_rmsnorm_ref(c["x"], c["r"], c["w"], EPS)
    c["rstd"] = rstd.float()
    dx, dw, cdx, cdw = R.rmsnorm_bwd_ref(c["dy"], c["x"], c["w"], c["rstd"])
    ax, adw, acdx, acdw = R.rmsnorm_bwd_ref(c["dy"], c["x"], c["w"], c["rstd"], c["dres"])
    rc, col = ("row", "column"), ("column",)
    c["out"] = {
        "y": Out(y, None, RED, rc), "rstd": Out(rstd, None, RED, ("row",)),
        "add.h": Out(h, None, None, rc), "add.y": Out(hy, None, RED, rc), "add.rstd": Out(hrstd, None, RED, ("row",)),
        "dx": Out(dx, cdx, RED, rc), "dw": Out(dw, cdw, RED, col),
        "add.dx": Out(ax, acdx, RED, rc), "add.dw": Out(adw, acdw, RED, col),
    }
    return c


def norm_emulate(c):
    """The kernels' formulas in fp32 torch, rounded once."""
    x, r, w, dy, dres, D = c["x"].float(), c["r"].float(), c["w"].float(), c["dy"].float(), c["dres"].float(), c["D"]
    eps = torch.tensor(EPS, dtype=torch.float32)

    def fwd(t):
        rs = torch.rsqrt((t * t).sum(-1) / D + eps)
        return _bf(t * rs[:, None] * w), rs

    got = {}
    got["y"], got["rstd"] = fwd(x)
    got["add.h"] = _bf(x + r)
    got["add.y"], got["add.rstd"] = fwd(got["add.h"].float())
    rs = c["rstd"][:, None]
    k = rs * rs * rs * (dy * w * x).sum(-1, keepdim=True) / D
    got["dx"], got["add.dx"] = _bf(rs * dy * w - x * k), _bf(rs * dy * w - x * k + dres)
    got["dw"] = got["add.dw"] = _bf((dy * x * rs).sum(0))
    return got


# ------------------------------------------------------------------------------------ RoPE + split
Q_AXES = ("batch", "head", "position", "dim")


@functools.lru_cache(maxsize=2)
def rope_case(B, S, H, Hkv, Dh, off):
    """qkv and the three incoming gradients ~ randn (bf16); tables from ``rope_tables(S + 8, Dh)``."""
    from gpu_topology_on_k8s_amd.ops.fused import rope_tables

    g = _gen("rope", B, S, H, Hkv, Dh, off)
    c = {"dims": (B, S, H, Hkv, Dh, off)}
    c["cos"], c["sin"] = rope_tables(S + 8, Dh)
    c["qkv"] = _bf(_randn(g, B * S, (H + 2 * Hkv) * Dh))
    c["dq"], c["dk"], c["dv"] = _bf(_randn(g, B, H, S, Dh)), _bf(_randn(g, B, Hkv, S, Dh)), _bf(_randn(g, B, Hkv, S, Dh))
    q, k, v, cq, ck = R.rope_split_ref64(c["qkv"], c["cos"], c["sin"], B, S, H, Hkv, Dh, off)
    dqkv, cd = R.rope_split_bwd_ref64(c["dq"], c["dk"], c["dv"], c["cos"], c["sin"], off)
    heads = H + 2 * Hkv
    shape = (B, S, heads, Dh)
    c["out"] = {
        "q": Out(q, cq, ELEM, Q_AXES), "k": Out(k, ck, ELEM, Q_AXES), "v": Out(v, None, None, Q_AXES),
        "dqkv": Out(dqkv.view(shape), cd.view(shape), ELEM, ("batch", "position", "head of q|k|v", "dim")),
    }
    return c


def rope_emulate(c, bwd_offset_shift=0, bwd_sign=-1.0):
    """fp32 emulation; ``bwd_offset_shift`` / ``bwd_sign`` = +1 make the two backward mutants."""
    B, S, H, Hkv, Dh, off = c["dims"]
    half = Dh // 2

    def rot(t, o, sign):  # t [B, S, heads, Dh]
        cs, sn = c["cos"][o:o + S].view(1, S, 1, half), c["sin"][o:o + S].view(1, S, 1, half) * sign
        a, b = t[..., :half], t[..., half:]
        return torch.cat([a * cs - b * sn, b * cs + a * sn], -1)

    x = c["qkv"].float().view(B, S, H + 2 * Hkv, Dh)
    got = {"q": _bf(rot(x[:, :, :H], off, 1.0)).transpose(1, 2), "k": _bf(rot(x[:, :, H:H + Hkv], off, 1.0)).transpose(1, 2),
           "v": c["qkv"].view(B, S, -1, Dh)[:, :, H + Hkv:].transpose(1, 2)}
    d = [c[n].float().transpose(1, 2) for n in ("dq", "dk")]
    o = off + bwd_offset_shift
    got["dqkv"] = torch.cat([_bf(rot(d[0], o, bwd_sign)), _bf(rot(d[1], o, bwd_sign)), c["dv"].transpose(1, 2)], 2)
    return got


# ------------------------------------------------------------------------------------ SwiGLU
@functools.lru_cache(maxsize=2)
def swiglu_case(T, F):
    """gates ~ 3 randn, ups and dh ~ randn.  Row 0, columns 0..7: gates +-20, +-80, +-150, +-0 with
    |up| <= 4 (saturation, fp32 overflow of exp(-g), signed zero).  No gate is planted in (-104, -88.7):
    there fp32 exp(-g) overflows and the kernel returns 0 where the exact value is still a normal bf16
    number; a known, harmless flush, and not what these tests are about."""
    g = _gen("swiglu", T, F)
    gate, up = 3.0 * _randn(g, T, F), _randn(g, T, F)
    gate[0, :8] = torch.tensor(SWIGLU_GATES)
    up[0] = up[0].clamp(-4.0, 4.0)
    c = {"T": T, "F": F, "gu": _bf(torch.cat([gate, up], 1)), "dh": _bf(_randn(g, T, F))}
    h, ch = R.swiglu_ref64(c["gu"])
    d, cd = R.swiglu_bwd_ref64(c["dh"], c["gu"])
    rc = ("row", "column")
    c["out"] = {"h": Out(h, ch, ELEM, rc), "dgate": Out(d[:, :F], cd[:, :F], ELEM, rc), "dup": Out(d[:, F:], cd[:, F:], ELEM, rc)}
    return c


def swiglu_emulate32(c):
    """The kernel's formulas in fp32, BEFORE the output rounding."""
    g, u = c["gu"].float().chunk(2, -1)
    d = c["dh"].float()
    sg = 1.0 / (1.0 + torch.exp(-g))
    return {"h": g / (1.0 + torch.exp(-g)) * u, "dgate": d * u * sg * (1.0 + g * (1.0 - sg)), "dup": d * (g * sg)}


def swiglu_emulate(c):
    return {n: _bf(t) for n, t in swiglu_emulate32(c).items()}


# ------------------------------------------------------------------------------------ cross-entropy
@functools.lru_cache(maxsize=None)
def xent_case(T, V):
    """logits ~ 3 randn (bf16).  Rows as far as T allows:
      0  all logits equal, label V - 1
      1  one logit +80, the rest -80, labelled at the +80
      2  columns 8..15 and 2048..2055 (where V allows) -inf, label 0
      3  ordinary row with an ignored label: ignore_index, V or -7 (all three mean loss 0 and an
         all-zero gradient row; which one depends on the case, row 4 and 5 take the next ones)
      6+ ordinary rows, random labels
    """
    g = _gen("xent", T, V)
    x = 3.0 * _randn(g, T, V)
    labels = torch.randint(0, V, (T,), generator=g)
    x[0], labels[0] = 1.5, V - 1
    hot = (V // 2 + 1) % V
    if T > 1:
        x[1], labels[1] = -80.0, hot
        x[1, hot] = 80.0
    if T > 2:
        labels[2] = 0
        for lo in (8, 2048):
            if V >= lo + 8 and V > 16:
                x[2, lo:lo + 8] = float("-inf")
    ignored = [IGNORE, V, -7]
    rot = XENT_CASES.index((T, V)) if (T, V) in XENT_CASES else 0
    for i in range(3, min(T, 6)):
        labels[i] = ignored[(rot + i) % 3]
    c = {"T": T, "V": V, "logits": _bf(x), "labels": labels, "gscale": torch.tensor([GSCALE])}
    loss, lse = R.xent_ref64(c["logits"], labels, IGNORE)
    c["lse"] = lse.float()
    d, cd = R.xent_bwd_ref64(c["logits"], labels, c["lse"], c["gscale"], IGNORE)
    one = torch.ones(T, dtype=torch.float64)
    c["out"] = {"lse": Out(lse, one, LSE, ("row",)), "loss_rows": Out(loss, one, LSE, ("row",)),
                "dlogits": Out(d, cd, ELEM, ("row", "column"))}
    return c


def xent_emulate(c, onehot_shift=0):
    x, labels, V = c["logits"].float(), c["labels"], c["V"]
    ok = (labels != IGNORE) & (labels >= 0) & (labels < V)
    lse = torch.logsumexp(x, -1)
    picked = x.gather(1, labels.where(ok, torch.zeros_like(labels))[:, None]).squeeze(1)
    onehot = torch.zeros_like(x)
    onehot[ok.nonzero().squeeze(1), (labels[ok] + onehot_shift) % V] = 1.0
    sc = torch.where(ok, c["gscale"][0], torch.tensor(0.0))[:, None]
    return {"lse": lse, "loss_rows": torch.where(ok, lse - picked, torch.zeros_like(lse)),
            "dlogits": _bf((torch.exp(x - c["lse"][:, None]) - onehot) * sc)}


# ------------------------------------------------------------------------------------ embedding backward
EMBED_FILL = 7.0  # the output is prefilled with it: rows no token owns must still hold it


@functools.lru_cache(maxsize=None)
def embed_case(V, D, T, integer):
    """Token ids: one id (7) at 2000 positions (a long sequential segment), ids 0 and V - 1, and the
    ids -1, V and V + 5, which are skipped; the rest random.  ``integer``: dx in {-3..3}, every sum is
    an exact fp32 integer (<= 6000 < 2^24) and the result must equal bf16_round(sum) bit for bit;
    otherwise dx ~ randn under the rule with RED."""
    g = _gen("embed", V, D, T)
    tok = torch.randint(0, V, (T,), generator=g)
    if T > 2100:
        pos = torch.randperm(T, generator=g)
        tok[pos[:2000]] = 7
        for i, t in enumerate((0, V - 1, -1, V, V + 5)):
            tok[pos[2000 + i]] = t
    dx = torch.randint(-3, 4, (T, D), generator=g).float() if integer else _randn(g, T, D)
    c = {"V": V, "D": D, "T": T, "tok": tok, "dx": _bf(dx)}
    rows, cond, owned = R.embed_bwd_ref64(tok, c["dx"], V)
    fill = torch.full_like(rows, EMBED_FILL)
    c["owned"] = owned
    c["out"] = {"dW": Out(torch.where(owned[:, None], rows, fill), torch.where(owned[:, None], cond, fill),
                          None if integer else RED, ("token id", "column"))}
    return c


def embed_emulate(c, drop_last_of=None):
    """Segment sums in fp32, in position order; ``drop_last_of`` = a token id whose last position is
    left out (the mutant)."""
    tok, dx = c["tok"].clone(), c["dx"].float()
    if drop_last_of is not None:
        tok[(tok == drop_last_of).nonzero()[-1]] = -1
    ok = (tok >= 0) & (tok < c["V"])
    out = torch.zeros(c["V"], c["D"]).index_add_(0, tok[ok], dx[ok])
    return {"dW": _bf(torch.where(c["owned"][:, None], out, torch.tensor(EMBED_FILL)))}


# ================================================================================ the comparison rule
def _tolerance(ref, cond, slack, bf16):
    """-> (tolerance, share of elements whose slack term exceeds the half-ulp term)."""
    cond = ref.abs() if cond is None else cond
    if not bf16:
        return slack * cond, 0.0
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -126))  # |ref| = m 2^e, m in [0.5, 1): ulp = 2^(e - 8)
    half = torch.ldexp(torch.ones_like(ref), e - 9)
    return half + slack * cond, float((slack * cond > half).double().mean())


def slack_share(out: Out) -> float:
    return _tolerance(out.ref, out.cond, out.slack, True)[1] if out.slack is not None else 0.0


def _report(name, bad, got, ref, tol, axes, note):
    idx = bad.nonzero()
    lines = [f"{name}: {len(idx)} of {ref.numel()} elements {note}; first ones:"]
    for i in idx[:12]:
        where = ", ".join(f"{a} {int(v)}" for a, v in zip(axes, i))
        t = tuple(i)
        lines.append(f"  {where}: got {got[t].item()!r} want {ref[t].item()!r}" + ("" if tol is None else f" tol {tol[t].item():.3e}"))
    for d, a in enumerate(axes):  # which indices of each axis are touched at all
        u = idx[:, d].unique()
        lines.append(f"  {a}: {len(u)} distinct, {u[:16].tolist()}{' ...' if len(u) > 16 else ''}")
    return "\n".join(lines)


def compare_rounded_once(name, got, out: Out):
    """-> (bad [mask over ref's shape], worst err / tol, slack share, report or None)."""
    ref, axes = out.ref, out.axes
    assert len(axes) == ref.dim(), (name, axes, ref.shape)
    got = got.detach().cpu()
    assert got.numel() == ref.numel(), (name, tuple(got.shape), tuple(ref.shape))
    got = got.reshape(ref.shape)
    if out.slack is None:  # a copy or an exact sum: the bits of bf16_round(ref)
        assert got.dtype == torch.bfloat16, (name, got.dtype)
        want = bf16_round(ref)
        bad = (got != want) | (got != got)
        rep = _report(name, bad, got, want, None, axes, "differ") if bool(bad.any()) else None
        return bad, float(bad.any()), 0.0, rep
    assert got.dtype in (torch.bfloat16, torch.float32), (name, got.dtype)
    tol, share = _tolerance(ref, out.cond, out.slack, got.dtype == torch.bfloat16)
    assert share <= VACUITY_CAP, f"{name}: the slack term dominates {share:.2%} of the elements: change the inputs"
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)  # a NaN is bad
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    worst = float(ratio.nan_to_num(nan=float("inf")).max()) if ratio.numel() else 0.0
    rep = _report(name, bad, got.double(), ref, tol, axes, "outside half an ulp + slack") if bool(bad.any()) else None
    return bad, worst, share, rep


def assert_rounded_once(name, got, ref64, cond64, slack, axes):
    """The rule of the module docstring; on failure the count, the first dozen elements with named
    indices and the touched indices of every axis.  Prints the worst err / tol and the slack share."""
    _, worst, share, rep = compare_rounded_once(name, got, Out(ref64, cond64, slack, axes))
    print(f"{name}: worst err/tol {worst:.3f}, slack-dominated {share:.3%}")
    if rep:
        print(rep)
        pytest.fail(rep, pytrace=False)


def check_outputs(case_name, c, got):
    for n, t in got.items():
        o = c["out"][n]
        assert_rounded_once(f"{case_name} {n}", t, o.ref, o.cond, o.slack, o.axes)


def bf16_trunc(t32):
    """fp32 -> bf16 by dropping the low 16 bits (the rounding-mode mutant)."""
    return (t32.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


# ================================================================================ the references
def _close(a, b):
    torch.testing.assert_close(a, b, rtol=1e-12, atol=0.0)


def _leaf(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64).requires_grad_(True)


@pytest.mark.parametrize("M,D", [(3, 8), (6, 40)])
def test_rmsnorm_bwd_ref_is_autograd_of_forward(M, D):
    g = _gen("ag-norm", M, D)
    x, w = _leaf(g, M, D), _leaf(g, D)
    dy, dres = _randn(g, M, D).double(), _randn(g, M, D).double()
    y, rstd = R.rmsnorm_ref(x, w, EPS)
    gx, gw = torch.autograd.grad(y, (x, w), dy, retain_graph=True)
    dx, dw, cdx, cdw = R.rmsnorm_bwd_ref(dy, x.detach(), w.detach(), rstd.detach())
    _close(dx, gx), _close(dw, gw)
    assert bool((cdx >= dx.abs()).all()) and bool((cdw >= dw.abs()).all())
    # the residual stream: h feeds the norm and carries its own gradient dres
    gx2, = torch.autograd.grad([y, x], (x,), [dy, dres])
    _close(R.rmsnorm_bwd_ref(dy, x.detach(), w.detach(), rstd.detach(), dres)[0], gx2)


def test_add_rmsnorm_ref_normalises_the_rounded_sum():
    g = _gen("add")
    x, r, w = _bf(_randn(g, 4, 16)), _bf(_randn(g, 4, 16) * 2.0 ** -6), _bf(torch.rand(16, generator=g) + 0.5)
    h, y, rstd = R.add_rmsnorm_ref(x, r, w, EPS)
    assert torch.equal(h, (x + r).double()) and not torch.equal(h, x.double() + r.double())
    y2, rstd2 = R.rmsnorm_ref(x + r, w, EPS)
    assert torch.equal(y, y2) and torch.equal(rstd, rstd2)


@pytest.mark.parametrize("B,S,H,Hkv,Dh,off", [(1, 3, 1, 1, 16, 2), (2, 5, 4, 2, 32, 3)])
def test_rope_bwd_ref_is_autograd_of_forward(B, S, H, Hkv, Dh, off):
    from gpu_topology_on_k8s_amd.ops.fused import rope_tables

    g = _gen("ag-rope", B, S, Dh)
    cos, sin = rope_tables(S + 8, Dh)
    x = _leaf(g, B * S, (H + 2 * Hkv) * Dh)
    q, k, v, cq, ck = R.rope_split_ref64(x, cos, sin, B, S, H, Hkv, Dh, off)
    grads = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in (q, k, v)]
    gx, = torch.autograd.grad([q, k, v], (x,), grads)
    d, cd = R.rope_split_bwd_ref64(*grads, cos, sin, off)
    _close(d, gx)
    assert bool((cq >= q.abs()).all()) and bool((cd >= d.abs()).all())


@pytest.mark.parametrize("T,F", [(2, 8), (5, 24)])
def test_swiglu_bwd_ref_is_autograd_of_forward(T, F):
    g = _gen("ag-swiglu", T, F)
    gu, dh = _leaf(g, T, 2 * F), _randn(g, T, F).double()
    h, ch = R.swiglu_ref64(gu)
    ggu, = torch.autograd.grad(h, (gu,), dh)
    d, cd = R.swiglu_bwd_ref64(dh, gu.detach())
    _close(d, ggu)
    assert bool((ch >= h.abs()).all()) and bool((cd >= d.abs()).all())


@pytest.mark.parametrize("T,V", [(4, 8), (7, 40)])
def test_xent_bwd_ref_is_autograd_of_forward(T, V):
    g = _gen("ag-xent", T, V)
    x = _leaf(g, T, V)
    labels = torch.randint(0, V, (T,), generator=g)
    labels[1], labels[2], labels[3] = IGNORE, V, -7
    loss, lse = R.xent_ref64(x, labels, IGNORE)
    assert loss.detach()[1:4].tolist() == [0.0, 0.0, 0.0]
    _close(loss[0], torch.nn.functional.cross_entropy(x[:1], labels[:1]))
    gx, = torch.autograd.grad(loss.sum() * GSCALE, (x,))
    d, cd = R.xent_bwd_ref64(x.detach(), labels, lse.detach(), GSCALE, IGNORE)
    torch.testing.assert_close(d, gx, rtol=1e-12, atol=1e-16)  # (p - 1) at the label cancels: a few ulps of 1
    assert not d[1:4].any() and bool((cd >= d.abs()).all())


@pytest.mark.parametrize("V,D,T", [(5, 8, 1), (9, 16, 40)])
def test_embed_bwd_ref_is_autograd_of_embedding(V, D, T):
    g = _gen("ag-embed", V, D, T)
    w, dx = _leaf(g, V, D), _randn(g, T, D).double()
    tok = torch.randint(-2, V + 2, (T,), generator=g) if T > 1 else torch.tensor([3])
    ok = (tok >= 0) & (tok < V)
    gw, = torch.autograd.grad(torch.nn.functional.embedding(tok[ok], w), (w,), dx[ok])
    rows, cond, owned = R.embed_bwd_ref64(tok, dx, V)
    torch.testing.assert_close(rows, gw, rtol=1e-12, atol=1e-15)  # index_add_ sums in another order
    assert torch.equal(owned, torch.bincount(tok[ok], minlength=V) > 0) and bool((cond >= rows.abs()).all())


# ================================================================================ the rule against itself
def test_swiglu_gate_cond_stays_under_the_cap_on_bf16_gates():
    """The cancellation term of d gate's cond (module docstring): over all finite bf16 g the factor
    f = 1 + g (1 - sigmoid(g)) has |f| >= 0.002786, so cond / (|value| (1 + |g|)) <= 20.7 and the
    effective slack stays below 2^-13.6; elsewhere the term is small against the value's own."""
    g = (torch.arange(0, 65536, dtype=torch.int32) << 16).view(torch.float32)
    g = g[torch.isfinite(g) & (g != 0)].reshape(-1, 1)
    f = (1 + g.double() * torch.sigmoid(-g.double())).abs()
    i = int(f.argmin())
    assert float(g[i]) == -1.28125 and 0.002786 < float(f[i]) < 0.002787
    val, cond = R.swiglu_bwd_ref64(torch.ones_like(g), torch.cat([g, torch.ones_like(g)], 1))
    ok = val[:, 0] != 0  # sigmoid underflows in float64 below g = -745
    factor = cond[ok, 0] / (val[ok, 0].abs() * (1 + g[ok, 0].double().abs()))
    assert 20.6 < float(factor.max()) < 20.7 and ELEM * float(factor.max()) < 2.0 ** -13.6 < 2.0 ** -12
    assert float(factor.median()) < 1.13 and bool((factor >= 1).all())
    assert torch.equal(cond[:, 1], val[:, 1].abs() * (1 + g[:, 0].double().abs()))  # d up: no such term


def test_rule_tolerance_is_half_an_ulp_plus_slack():
    ref = torch.tensor([1.0, 1.99, 0.0, -3.0, 2.0 ** -140], dtype=torch.float64)
    tol, share = _tolerance(ref, None, 0.0, True)
    assert tol.tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -134, 2.0 ** -7, 2.0 ** -134] and share == 0.0
    out = Out(ref, None, 0.0, ("i",))
    ok = _bf(torch.tensor([1.0, 1.9921875, -0.0, -3.0, 0.0]))
    assert compare_rounded_once("t", ok, out)[3] is None
    bad, worst, _, rep = compare_rounded_once("t", _bf(torch.tensor([1.0078125, 1.9921875, 0.0, float("nan"), 0.0])), out)
    assert bad.tolist() == [True, False, False, True, False] and "i: 2 distinct, [0, 3]" in rep
    with pytest.raises(pytest.fail.Exception, match="2 of 5 elements"):
        assert_rounded_once("t", _bf(torch.tensor([1.0078125, 1.9921875, 0.0, float("nan"), 0.0])), ref, None, 0.0, ("i",))
    with pytest.raises(AssertionError, match="change the inputs"):  # vacuous: cond >> |ref|
        compare_rounded_once("t", ok, Out(ref, ref.abs() * 1e6 + 1.0, ELEM, ("i",)))


def _all_pass(case_name, c, got):
    for n, t in got.items():
        bad, worst, share, rep = compare_rounded_once(f"{case_name} {n}", t, c["out"][n])
        print(f"{case_name} {n}: emulation worst err/tol {worst:.3f}, slack-dominated {share:.3%}")
        assert rep is None, rep
        o = c["out"][n]
        if o.cond is not None and o.slack not in (None, LSE):
            assert bool((o.cond >= o.ref.abs() * (1 - 1e-15)).all()), n


def _touched(bad, dim):
    return bad.nonzero()[:, dim].unique().tolist()


@pytest.mark.parametrize("M,D", NORM_CASES)
def test_norm_cases_emulation_passes_and_tolerance_is_tight(M, D):
    _all_pass(f"norm {M}x{D}", norm_case(M, D), norm_emulate(norm_case(M, D)))


@pytest.mark.parametrize("dims", ROPE_CASES + [ROPE_T_CASE])
def test_rope_cases_emulation_passes_and_tolerance_is_tight(dims):
    _all_pass(f"rope {dims}", rope_case(*dims), rope_emulate(rope_case(*dims)))


@pytest.mark.parametrize("T,F", SWIGLU_CASES)
def test_swiglu_cases_emulation_passes_and_tolerance_is_tight(T, F):
    _all_pass(f"swiglu {T}x{F}", swiglu_case(T, F), swiglu_emulate(swiglu_case(T, F)))


@pytest.mark.parametrize("T,V", XENT_CASES + [XENT_T_CASE])
def test_xent_cases_emulation_passes_and_tolerance_is_tight(T, V):
    _all_pass(f"xent {T}x{V}", xent_case(T, V), xent_emulate(xent_case(T, V)))


@pytest.mark.parametrize("V,D,T", EMBED_CASES)
@pytest.mark.parametrize("integer", [True, False])
def test_embed_cases_emulation_passes_and_tolerance_is_tight(V, D, T, integer):
    c = embed_case(V, D, T, integer)
    if integer:
        assert float(c["out"]["dW"].cond.max()) < 2 ** 24  # every partial sum is an exact integer
    _all_pass(f"embed {V}x{D}x{T}", c, embed_emulate(c))


def test_mutant_truncated_rounding_fails():
    c = swiglu_case(3, 14336)
    for n, t in swiglu_emulate32(c).items():
        bad, _, _, rep = compare_rounded_once(n, bf16_trunc(t), c["out"][n])
        assert rep is not None and 0.3 < float(bad.double().mean()) < 0.6, (n, float(bad.double().mean()))
    c = norm_case(33, 1000)
    x, w, rs = c["x"].float(), c["w"].float(), c["rstd"][:, None]
    bad = compare_rounded_once("y", bf16_trunc(x * rs * w), c["out"]["y"])[0]
    assert 0.3 < float(bad.double().mean()) < 0.6


def test_mutant_last_eight_columns_wrong_is_reported_there():
    M, D = 33, 1000
    c = norm_case(M, D)
    got = norm_emulate(c)
    for n in ("y", "dx", "add.dx"):
        t = got[n].clone()
        t[:, D - 8:] = t[:, D - 16:D - 8]  # the neighbouring vector's values
        bad, _, _, rep = compare_rounded_once(n, t, c["out"][n])
        assert _touched(bad, 1) == list(range(D - 8, D)), n
        assert f"column: 8 distinct, {list(range(D - 8, D))}" in rep
    c = swiglu_case(17, 64)
    t = swiglu_emulate(c)["h"].clone()
    t[5, 56:] = t[4, 56:]
    bad = compare_rounded_once("h", t, c["out"]["h"])[0]
    assert _touched(bad, 0) == [5] and set(_touched(bad, 1)) <= set(range(56, 64)) and int(bad.sum()) >= 6


@pytest.mark.parametrize("M,D,least", [(7, 4104, 3900), (2049, 520, 130)])
def test_mutant_dw_without_its_last_row_fails(M, D, least):
    """At M = 7 one row is a seventh of the sum: nearly every column fails.  At M = 2049 a column's sum
    is about 290 (bf16 ulp 2) and the dropped term about 0.6: a rounding boundary is crossed in roughly
    0.6 / 2 of the columns, so at least a quarter of them must fail."""
    c = norm_case(M, D)
    x, dy, rs = c["x"].float(), c["dy"].float(), c["rstd"][:, None]
    t = _bf((dy * x * rs)[:-1].sum(0))
    for n in ("dw", "add.dw"):
        bad, _, _, rep = compare_rounded_once(n, t, c["out"][n])
        assert rep is not None and int(bad.sum()) >= least, (n, int(bad.sum()))


def test_mutant_backward_rope_off_by_one_position_or_forward_sign_fails():
    dims = ROPE_CASES[3]
    c = rope_case(*dims)
    B, S, H, Hkv, Dh, off = dims
    rotated = list(range(H + Hkv))  # the v heads are copies: neither mutant touches them
    for kw in ({"bwd_offset_shift": 1}, {"bwd_sign": 1.0}):
        bad, _, _, rep = compare_rounded_once("dqkv", rope_emulate(c, **kw)["dqkv"], c["out"]["dqkv"])
        assert _touched(bad, 2) == rotated and _touched(bad, 0) == [0, 1], kw
        # the slow half of the frequencies moves an element by less than half an ulp per position
        assert float(bad[:, :, :H + Hkv].double().mean()) > 0.35, kw
        if "bwd_sign" in kw:  # position 0 + offset 5 still rotates; with offset 0 its sin would be 0
            assert _touched(bad, 1) == list(range(S))
        assert f"head of q|k|v: {H + Hkv} distinct" in rep


def test_mutant_onehot_one_column_off_is_reported_at_both_columns():
    T, V = 4, 2056
    c = xent_case(T, V)
    bad, _, _, rep = compare_rounded_once("dlogits", xent_emulate(c, onehot_shift=1)["dlogits"], c["out"]["dlogits"])
    want = sorted((i, int(y) + d) for i, y in enumerate(c["labels"].tolist()) if 0 <= y < V and y != IGNORE for d in (0, 1))
    assert sorted(map(tuple, bad.nonzero().tolist())) == sorted((i, col % V) for i, col in want)
    assert "row: 3 distinct, [0, 1, 2]" in rep


def test_mutant_eps_left_out_fails_on_rstd_of_the_small_row():
    M, D = 5, 512
    c = norm_case(M, D)
    x = c["x"].float()
    rs = torch.rsqrt((x * x).sum(-1) / D + torch.tensor(EPS))
    rs[2] = torch.rsqrt((x[2] * x[2]).sum() / D)  # the row scaled by 2^-10
    bad, _, _, rep = compare_rounded_once("rstd", rs, c["out"]["rstd"])
    assert bad.tolist() == [False, False, True, False, False] and "row 2:" in rep
    # and on an ordinary row (mean(x^2) ~ 1) leaving eps out is 5e-6 relative: below RED, as ISSUE says
    rs[2], rs[0] = c["rstd"][2], torch.rsqrt((x[0] * x[0]).sum() / D)
    assert compare_rounded_once("rstd", rs, c["out"]["rstd"])[3] is None


@pytest.mark.parametrize("integer", [True, False])
def test_mutant_embedding_segment_without_its_last_position_fails(integer):
    c = embed_case(1000, 4096, 4099, integer)
    bad, _, _, rep = compare_rounded_once("dW", embed_emulate(c, drop_last_of=7)["dW"], c["out"]["dW"])
    assert _touched(bad, 0) == [7] and "token id: 1 distinct, [7]" in rep
    assert int(bad.sum()) > 1500, int(bad.sum())
