"""CPU: the float64 AdamW reference of models/optim_ref.py, the comparison rule ``assert_adamw`` and the case
tables of tests/test_gpu_adamw_exact.py (which imports all three from here, so the GPU tests and these self-tests
cannot drift apart).  ``Out``, ``compare_rounded_once``, ``_report`` and ``VACUITY_CAP`` are those of
tests/test_llama_ref.py.

  * the rule against itself: an fp32 torch emulation of ``adam8_update`` (csrc/common/adamw_update.h) passes every
    case, with every multiply-add rounded twice and with the two moment updates, ``upd + wd p`` and the final
    ``p - lr (...)`` contracted into FMAs; each mutant of MUTANTS fails and is reported at the elements it touches;
  * one test records which mutants the former ``allclose`` tolerances of tests/test_fused_gpu.py accept;
  * the tolerance is not vacuous: the slack term exceeds the half-ulp term on at most 5 % of the master elements.

The rule.  With ``ref`` and ``cond`` of ``adamw_step_ref`` (cond = the sum of the magnitudes the fp32 arithmetic
adds; for the master the magnitude of the STEP) and u = 2^-24, the relative error bound of one correctly rounded
fp32 operation:

    m', v'     |got - ref| <= slack * cond
    master'    |got - ref| <= ulp_fp32 / 2 + slack * cond
    W (bf16)   bits == bf16_round(the kernel's own master'), and
               |W - ref master'| <= ulp_bf16 / 2 + (ulp_fp32 / 2 + slack * cond)

Both ulps are taken at |ref| + slack * cond, the largest magnitude the unrounded value can have (it differs from
the ulp at |ref| only where the slack carries the value over a power of two).  W is the second rounding of a value
that was already rounded to fp32, so its bound is the master's plus half a bf16 ulp: without the fp32 term a
kernel master within 2^-25 of a bf16 tie (one element in 2^16, more than a hundred of the 8.4 M of the largest
case) would round away from a reference on the tie's other side and fail with nothing wrong.

The slacks, counted from ``adam8_update`` as the build compiles it (hipcc -O3, no fast-math: fp32 division is the
v_div_scale / v_div_fmas / v_div_fixup sequence and ``sqrtf`` is refined, both correctly rounded, u each; fp32
denormals are kept).  First-order bounds; where the compiler contracts a multiply-add one rounding falls away, so
the uncontracted count covers both forms:

  SLACK_M = 2^-21   gr = g gs (u); 1 - b1 (u; exact for b1 in [1/2, 1], counted all the same); (1 - b1) gr (u):
                    the second term to 3 u; b1 m (u); the sum (u of |m'| <= cond): <= 4 u cond_m.
  SLACK_V = 2^-21   1 - b2 (u), times gr (its u, and one), times gr (again): the second term to 5 u in either
                    association; b2 v (u); the sum (u): <= 6 u cond_v.
  SLACK_P = 2^-20   m' carries 4 u cond_m; m' / bc1 (u): 5 u cond_m / bc1.  v' carries 6 u; v' / bc2 (u): 7 u;
                    sqrtf halves it and adds its own: 4.5 u; + eps (u; eps > 0, so the summands' relative errors
                    do not grow): the denominator to 5.5 u.  The quotient (u): upd to (5 + 5.5 + 1) u = 11.5 u of
                    CU = cond_m / bc1 / den.  wd p (u); upd + wd p (u of the sum); lr (...) (u): the step to
                    lr ((11.5 + 2) u CU + 3 u wd |p|) <= 13.5 u cond.  The rounding of p - step is the half-ulp
                    term.
Each count is rounded up to the next power of two (4 u and 6 u -> 8 u, 13.5 u -> 16 u), which also covers the
second-order terms (below 2^-20 of the first-order ones).

The device form (``hyper<true>`` of csrc/ops/adamw.hip) derives three scalars in fp32 that the reference has in
float64; ``dev_slacks`` adds their relative errors d_gs, d_1, d_2 (of grad_scale', bias_c1, bias_c2):

    m': + d_gs      v': + 2 d_gs      master': + 2 d_gs + d_1 + d_2 / 2
        (m' and sqrt(v') each carry d_gs into upd; upd is inversely proportional to bc1 and to sqrt(bc2))
    d_i  = 2 u beta^t / bias_c + u   powf is good to 1 ulp = 2 u (the HIP math API's table), the subtraction
                                     from 1 rounds once and divides the absolute error by bias_c
    d_gs = d_ss / 2 + 5 u            clip on and partials given, else 0: sqrtf (u), times grad_scale (u), + 1e-6
                                     (u), clip / (.) (u), grad_scale f (u)
    d_ss = (8 trips + 9 + ceil(grid / 256) + 9 [+ 1]) u
                                     the sum of squares as ``sq_norm_parts`` and ``hyper`` add it: a thread's 8
                                     squares per grid-stride trip in sequence, 6 shuffle levels and 3 adds across
                                     the waves, then the same over the grid's partials; the square of a bf16 value
                                     is exact, of an fp32 value one more rounding ([+ 1]).
``dev_slacks`` computes these from the case's n, beta, t and gradient type; nothing is measured.

The vacuity condition is on the inputs: per case the slack term may exceed the half-ulp term on at most 5 % of
the master elements outside the planted small masters (the 2^-12 randn band and the planted +-0, where the step is
larger than the value and is therefore measured at the slack itself).  It holds for the training set and t = 1000
with the host form's slack.  It cannot hold for the set t = 1, lr = 0.25, wd = 0.5 with ANY slack of 4 u or more:
there lr wd = 1/8, the decay term alone is an eighth of the master, and 4 u / 8 of the master is already half an
ulp of it.  That set is the opposite of vacuous (the step is a large part of the value and is measured to 2^-20 of
itself); its cases assert instead that the whole tolerance stays below 2^-18 of the step's magnitude on 95 % of the
elements (the training set: about 2^-14).  The device form's larger slack is printed, not capped.
"""
import functools
import math

import pytest
import torch

from gpu_topology_on_k8s_amd.models.optim_ref import AdamWRef, adamw_step_ref, dev_hyper_ref, sum_of_squares_ref
from test_llama_ref import VACUITY_CAP, Out, _gen, _report, bf16_trunc, compare_rounded_once

U = 2.0 ** -24
SLACK_M, SLACK_V, SLACK_P = 2.0 ** -21, 2.0 ** -21, 2.0 ** -20
HOST_SLACKS = (SLACK_M, SLACK_V, SLACK_P)
STEP_SHARPNESS = 2.0 ** -18  # set "t1": tolerance / step magnitude on 95 % of the elements (module docstring)

# name -> (lr, beta1, beta2, eps, weight_decay, grad_scale, t)
HYPERS = {
    "train": (1e-3, 0.9, 0.95, 1e-8, 0.1, 0.5, 3),      # the hyper-parameters of tests/test_fused_gpu.py
    "t1": (0.25, 0.9, 0.95, 1e-8, 0.5, 0.5, 1),         # small bias corrections, a visible decay term
    "t1000": (1e-3, 0.9, 0.95, 1e-8, 0.1, 0.5, 1000),   # bias corrections 1 (bias_c2 rounds to 1.0f)
}
GDTYPES = (torch.bfloat16, torch.float32)
CLIP = 1.0  # the device form's clip_norm where clipping is on

# ================================================================================ the case tables
# Flat kernel (adamw_flat_kernel: 256 threads x 8 elements per block, at most 4096 blocks, grid-stride beyond):
FLAT_SMALL = [
    8,          # one thread
    8 * 257,    # one vector past a block: the second block has one live thread
]
TRIP = 4096 * 256  # vectors per trip of the full grid
FLAT_LARGE = 8 * (TRIP + 777)  # a full second trip for the first 777 threads only: 8,394,824 elements
FLAT_LARGE_VECTORS = (0, TRIP - 1, TRIP, TRIP + 776)  # first and last vector of both trips

# what the eight lanes of a planted vector hold
PLANTS = ("g=0", "m=v=g=0", "m=v=0 g gs=+eps", "master=+0", "master=-0", "g=+2^-120", "g=-2^-120", "m=v=0 g gs=-2eps")


def hyper8(name):
    """The host form's hp tensor: the eight values in fp32, the bias corrections computed in float64 first."""
    lr, b1, b2, eps, wd, gs, t = HYPERS[name]
    return torch.tensor([lr, b1, b2, eps, wd, gs, 1 - b1 ** t, 1 - b2 ** t], dtype=torch.float64).float()


def hyper_dev(name, clip):
    lr, b1, b2, eps, wd, gs, _ = HYPERS[name]
    return torch.tensor([lr, b1, b2, eps, wd, gs, clip, 0.0], dtype=torch.float64).float()


def make_case(n, gdtype, hp_name, vectors=None, plain=False):
    """master ~ randn, m ~ 0.01 |randn|, v ~ 0.001 |randn|, g ~ randn (seeded, CPU).  Unless ``plain``: every
    vector of ``vectors`` (default: the first and the last) holds PLANTS in its eight lanes, and from n = 512 an
    eighth of the elements (a band that starts at n / 4) has master = 2^-12 randn.  ``exempt`` marks the planted
    small masters (the band and the planted zeros), ``planted`` every planted lane by its PLANTS index + 1."""
    assert n % 8 == 0
    gen = _gen("adamw", n, str(gdtype), hp_name, plain)
    r = lambda: torch.randn(n, generator=gen)  # noqa: E731
    master, m, v, g = r(), r().abs() * 0.01, r().abs() * 0.001, r()
    gs = HYPERS[hp_name][5]
    eps = HYPERS[hp_name][3]
    planted = torch.zeros(n, dtype=torch.int8)
    exempt = torch.zeros(n, dtype=torch.bool)
    if not plain:
        if n >= 512:
            lo = n // 4 // 8 * 8
            hi = lo + n // 8 // 8 * 8
            master[lo:hi] = 2.0 ** -12 * torch.randn(hi - lo, generator=gen)
            exempt[lo:hi] = True
        nv = n // 8
        for vi in sorted(set(vectors if vectors is not None else (0, nv - 1))):
            b = 8 * vi
            assert 0 <= vi < nv and not bool(exempt[b:b + 8].any())
            planted[b:b + 8] = torch.arange(1, 9, dtype=torch.int8)
            g[b + 0] = 0.0
            m[b + 1] = v[b + 1] = g[b + 1] = 0.0
            m[b + 2] = v[b + 2] = 0.0
            g[b + 2] = eps / gs
            master[b + 3] = 0.0
            master[b + 4] = -0.0
            g[b + 5], g[b + 6] = 2.0 ** -120, -2.0 ** -120
            m[b + 7] = v[b + 7] = 0.0
            g[b + 7] = -2.0 * eps / gs
            exempt[b + 3] = exempt[b + 4] = True
    c = {"n": n, "gdtype": gdtype, "hp_name": hp_name, "hp": hyper8(hp_name), "master": master, "m": m, "v": v,
         "g": g.to(gdtype), "w": master.to(torch.bfloat16), "planted": planted, "exempt": exempt}
    return c


@functools.lru_cache(maxsize=None)
def small_case(n, gdtype, hp_name, plain=False):
    """A cached case with its host-form reference; read-only."""
    c = make_case(n, gdtype, hp_name, plain=plain)
    c["ref"] = adamw_step_ref(c["master"], c["m"], c["v"], c["g"], c["hp"])
    return c


def sqnorm_adds(n, gdtype):
    """d_ss / u of the module docstring for ``sq_norm_parts`` over n elements."""
    nv = n // 8
    grid = max(1, min((nv + 255) // 256, 1024))
    trips = -(-nv // (grid * 256))
    return 8 * trips + 9 + -(-grid // 256) + 9 + (gdtype == torch.float32)


def dev_slacks(n, gdtype, hp_name, clipped):
    """(slack m', v', master') of the device form; ``clipped``: partials were given and clip_norm > 0."""
    _, b1, b2, _, _, _, t = HYPERS[hp_name]
    b1, b2 = float(torch.tensor(b1, dtype=torch.float32)), float(torch.tensor(b2, dtype=torch.float32))
    d1 = 2 * U * b1 ** t / (1 - b1 ** t) + U
    d2 = 2 * U * b2 ** t / (1 - b2 ** t) + U
    dgs = (sqnorm_adds(n, gdtype) / 2 + 5) * U if clipped else 0.0
    return SLACK_M + dgs, SLACK_V + 2 * dgs, SLACK_P + 2 * dgs + d1 + d2 / 2


def dev_reference(c, clip, partials):
    """Reference and slacks of ``adamw_step_dev`` on case c: ``clip`` = hp[6], ``partials`` = whether the sum of
    squares is handed over."""
    t = HYPERS[c["hp_name"]][6]
    clipped = bool(partials and clip > 0)
    hp = dev_hyper_ref(hyper_dev(c["hp_name"], clip), float(t), sum_of_squares_ref(c["g"]) if clipped else None)
    return adamw_step_ref(c["master"], c["m"], c["v"], c["g"], hp), dev_slacks(c["n"], c["gdtype"], c["hp_name"], clipped), hp


# ================================================================================ the comparison rule
def _half_ulp(x, mant_bits):
    """Half an ulp at magnitude x of a format with ``mant_bits`` stored mantissa bits (fp32 23, bf16 7), never
    below the formats' common smallest normal binade."""
    _, e = torch.frexp(x.clamp_min(2.0 ** -126))  # x = f 2^e, f in [0.5, 1): ulp = 2^(e - 1 - mant_bits)
    return torch.ldexp(torch.ones_like(x), e - 2 - mant_bits)


def master_tolerance(ref: AdamWRef, slack):
    """-> (tolerance of master', tolerance of W, the slack term, the fp32 half-ulp term)."""
    s = slack * ref.cond_master
    top = ref.master.abs() + s
    h32, h16 = _half_ulp(top, 23), _half_ulp(top, 7)
    return h32 + s, h16 + h32 + s, s, h32


def _compare(name, got, ref, tol, note):
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)  # a NaN is bad
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    worst = float(ratio.nan_to_num(nan=float("inf")).max()) if ratio.numel() else 0.0
    rep = _report(name, bad, got.double(), ref, tol, ("element",), note) if bool(bad.any()) else None
    return bad, worst, rep


def compare_adamw(name, got, ref: AdamWRef, slacks=HOST_SLACKS, exempt=None, cap=VACUITY_CAP):
    """``got``: the kernel's master, m, v (fp32) and, where there is one, w (bf16), flat.  -> {output: (bad mask, worst err / tol,
    report or None)} for m, v, master, w and "w bits", and the share of master elements (outside ``exempt``) whose
    slack term exceeds the half-ulp term, asserted <= ``cap`` unless that is None."""
    sm, sv, sp = slacks
    g = {k: got[k].detach().cpu().reshape(-1) for k in ("master", "m", "v", "w") if k in got}
    assert g["master"].dtype == g["m"].dtype == g["v"].dtype == torch.float32, name
    res = {}
    for k, r, cond, s in (("m", ref.m, ref.cond_m, sm), ("v", ref.v, ref.cond_v, sv)):
        bad, worst, _, rep = compare_rounded_once(f"{name} {k}", g[k], Out(r, cond, s, ("element",)))
        res[k] = (bad, worst, rep)
    tol_p, tol_w, s, h32 = master_tolerance(ref, sp)
    keep = torch.ones_like(s, dtype=torch.bool) if exempt is None else ~exempt
    share = float((s > h32)[keep].double().mean()) if bool(keep.any()) else 0.0
    if cap is not None and int(keep.sum()) >= 100:  # the share of the six ordinary masters of n = 8 says nothing
        assert share <= cap, f"{name}: the slack term dominates {share:.2%} of the master elements: change the inputs"
    res["master"] = _compare(f"{name} master", g["master"], ref.master, tol_p, "outside half an fp32 ulp + slack")
    if "w" in g:  # absent: a caller that holds no weights for these elements (the padding of a ZeRO-1 slice)
        assert g["w"].dtype == torch.bfloat16, name
        res["w"] = _compare(f"{name} w", g["w"], ref.master, tol_w, "outside half a bf16 ulp + the master's tolerance")
        want = g["master"].to(torch.bfloat16)  # round to nearest even
        bits_bad = g["w"].view(torch.int16) != want.view(torch.int16)
        rep = _report(f"{name} w bits", bits_bad, g["w"].double(), want.double(), None, ("element",),
                      "are not the kernel's own master rounded to bf16") if bool(bits_bad.any()) else None
        res["w bits"] = (bits_bad, float(bits_bad.any()), rep)
    # how much of the slack the master uses: what of the error is left after the half ulp, over the slack term
    over = ((g["master"].double() - ref.master).abs() - h32).clamp_min(0.0)
    use = torch.where(over > 0, over / s, torch.zeros_like(s)).nan_to_num(nan=float("inf"))
    return res, share, float(use.max()) if use.numel() else 0.0


def assert_adamw(name, got, ref, slacks=HOST_SLACKS, exempt=None, cap=VACUITY_CAP):
    """The rule of the module docstring; prints the worst err / tol of every output and the slack share, and fails
    with the count, the first dozen elements and the touched indices of every output that misses.  -> the figures:
    worst err / tol per output, and "slack use": the largest share of its slack term a master element needs once
    half an ulp is taken off its error (err / tol of the master and of W come close to 1 by construction: a
    rounding's error reaches half an ulp)."""
    res, share, use = compare_adamw(name, got, ref, slacks, exempt, cap)
    figures = {k: r[1] for k, r in res.items()}
    figures["slack use"] = use
    print(f"{name}: worst err/tol " + ", ".join(f"{k} {w:.3f}" for k, w in figures.items() if k not in ("w bits", "slack use"))
          + f"; master slack use {use:.3f}, slack-dominated {share:.3%}")
    reps = [r[2] for r in res.values() if r[2]]
    if reps:
        print("\n".join(reps))
        pytest.fail("\n".join(reps), pytrace=False)
    return figures


def assert_within_the_counts(figures):
    """The emulation stays within the first-order counts of the module docstring, which the slacks round up: 4 of
    8 u for m', 6 of 8 u for v', 13.5 of 16 u for the master's slack term (the device form adds to count and slack
    alike, so the shares only fall)."""
    assert figures["m"] <= 4 / 8 and figures["v"] <= 6 / 8 and figures["slack use"] <= 13.5 / 16, figures
    assert figures["master"] <= 1 and figures["w"] <= 1 and figures["w bits"] == 0, figures


def case_cap(hp_name):
    """The vacuity cap of a host-form case (module docstring: set "t1" cannot meet it, see assert_step_sharpness)."""
    return None if hp_name == "t1" else VACUITY_CAP


def assert_step_sharpness(c, ref, slack=SLACK_P):
    """Set "t1": the whole master tolerance is below STEP_SHARPNESS of the step's magnitude on 95 % of the
    elements with a step."""
    tol_p, _, _, _ = master_tolerance(ref, slack)
    has = ref.cond_master > 0
    share = float((tol_p[has] <= STEP_SHARPNESS * ref.cond_master[has]).double().mean())
    assert share >= 1 - VACUITY_CAP, (c["hp_name"], share)
    return share


# ================================================================================ the emulation and its mutants
MUTANTS = ("eps omitted", "eps under the square root", "weight decay x 1.05", "decay from the bf16 weight",
           "decay of the updated master", "bc1 and bc2 swapped", "grad_scale after squaring", "bf16 weight truncated",
           "one vector stale", "last vector of a block skipped")
STALE_VECTOR = 100  # an ordinary vector of the 8 * 257 cases


def _fma(a, b, c):
    """round_fp32(a b + c) with the product exact (float64 holds it; the sum's own float64 rounding is 2^-29 of
    an fp32 ulp)."""
    return (a.double() * b.double() + c.double()).float()


def emulate(c, contract=False, mutant=None, hp=None):
    """``adam8_update`` in fp32 torch, one rounding per operation; ``contract``: both moment updates, upd + wd p and
    p - lr (...) as FMAs.  ``mutant``: one of MUTANTS.  ``hp``: eight fp32 values instead of the case's."""
    lr, b1, b2, eps, wd, gs, bc1, bc2 = (c["hp"] if hp is None else hp).float().unbind()
    p, m, v, g = c["master"], c["m"], c["v"], c["g"].float()
    one = torch.tensor(1.0)
    if mutant == "bc1 and bc2 swapped":
        bc1, bc2 = bc2, bc1
    if mutant == "weight decay x 1.05":
        wd = wd * torch.tensor(1.05)
    gr = g * gs
    a1 = (one - b1) * gr
    m2 = _fma(b1, m, a1) if contract else b1 * m + a1
    a2 = (one - b2) * (g if mutant == "grad_scale after squaring" else gr)  # the mutant: (1 - b2) g (g gs), the scale once
    gq = gr
    v2 = _fma(a2, gq, b2 * v) if contract else b2 * v + a2 * gq
    q = v2 / bc2
    if mutant == "eps omitted":
        den = q.sqrt()
    elif mutant == "eps under the square root":
        den = (q + eps).sqrt()
    else:
        den = q.sqrt() + eps
    upd = (m2 / bc1) / den
    pd = p.to(torch.bfloat16).float() if mutant == "decay from the bf16 weight" else p
    if mutant == "decay of the updated master":
        p1 = p - lr * upd
        p2 = p1 - lr * (wd * p1)
    else:
        x = _fma(wd, pd, upd) if contract else upd + wd * pd
        p2 = _fma(-lr, x, p) if contract else p - lr * x
    out = {"master": p2, "m": m2, "v": v2, "w": bf16_trunc(p2) if mutant == "bf16 weight truncated" else p2.to(torch.bfloat16)}
    stale = {"one vector stale": STALE_VECTOR, "last vector of a block skipped": 255}.get(mutant)
    if stale is not None:
        assert 8 * stale + 8 <= c["n"] and not bool(c["planted"][8 * stale:8 * stale + 8].any())
        for k in out:
            out[k] = out[k].clone()
            out[k][8 * stale:8 * stale + 8] = c[k][8 * stale:8 * stale + 8]
    return out


# ================================================================================ the reference
def test_reference_is_the_formula_in_float64_and_its_conds_bound_the_values():
    c = small_case(8 * 257, torch.bfloat16, "train")
    ref = c["ref"]
    lr, b1, b2, eps, wd, gs, bc1, bc2 = c["hp"].double().tolist()
    i = 1234  # an ordinary element, by hand
    assert int(c["planted"][i]) == 0
    p, m, v, g = (float(c[k][i]) for k in ("master", "m", "v", "g"))
    m2 = b1 * m + (1 - b1) * g * gs
    v2 = b2 * v + (1 - b2) * (g * gs) ** 2
    p2 = p - lr * (m2 / bc1 / (math.sqrt(v2 / bc2) + eps) + wd * p)
    assert math.isclose(float(ref.m[i]), m2, rel_tol=1e-14) and math.isclose(float(ref.v[i]), v2, rel_tol=1e-14)
    assert math.isclose(float(ref.master[i]), p2, rel_tol=1e-14)
    assert bool((ref.cond_m >= ref.m.abs()).all()) and torch.equal(ref.cond_v, ref.v)
    assert bool((ref.cond_master >= (ref.master - c["master"].double()).abs() * (1 - 1e-9)).all())
    # the planted lanes of the first vector
    assert float(ref.m[1]) == 0.0 and float(ref.v[1]) == 0.0  # m = v = g = 0: update 0 / eps = 0, decay only
    assert float(ref.master[1]) == float(c["master"][1].double() * (1 - lr * wd)) or math.isclose(
        float(ref.master[1]), float(c["master"][1]) * (1 - lr * wd), rel_tol=1e-15)
    den = math.sqrt(float(ref.v[2]) / bc2)
    assert 0.3 * eps < den < 3 * eps  # eps decides: the other summand of the denominator is of its order
    assert float(c["master"][3]) == 0.0 and 0 < abs(float(ref.master[3])) <= float(ref.cond_master[3])  # the step alone
    assert float(c["master"][4]) == 0.0 and math.copysign(1.0, float(c["master"][4])) == -1.0


def test_dev_hyper_ref_matches_the_host_quantities():
    g = torch.tensor([3.0, -4.0] + [0.0] * 6)
    hp = dev_hyper_ref([1e-3, 0.9, 0.95, 1e-8, 0.1, 0.5, 1.0, 0.0], 3.0, sum_of_squares_ref(g))
    assert sum_of_squares_ref(g) == 25.0
    assert math.isclose(hp[5], 0.5 * 1.0 / (2.5 + 1e-6), rel_tol=1e-9)  # norm 5 * 0.5 > clip
    assert math.isclose(hp[6], 1 - 0.9 ** 3, rel_tol=1e-15) and math.isclose(hp[7], 1 - 0.95 ** 3, rel_tol=1e-15)
    assert dev_hyper_ref([1e-3, 0.9, 0.95, 1e-8, 0.1, 0.5, 1.0, 0.0], 3.0, None)[5] == 0.5  # no partials: no clipping
    assert dev_hyper_ref([1e-3, 0.9, 0.95, 1e-8, 0.1, 0.5, -1.0, 0.0], 3.0, 25.0)[5] == 0.5  # clip off in hp
    assert dev_hyper_ref([1e-3, 0.9, 0.95, 1e-8, 0.1, 0.5, 100.0, 0.0], 3.0, 25.0)[5] == 0.5  # the factor is capped at 1
    sm, sv, sp = dev_slacks(8 * 257, torch.bfloat16, "train", True)
    assert sqnorm_adds(8 * 257, torch.bfloat16) == 27 and sqnorm_adds(FLAT_LARGE, torch.float32) == 63
    assert math.isclose(sm, SLACK_M + 18.5 * U) and math.isclose(sv, SLACK_V + 37 * U) and SLACK_P + 37 * U < sp < 2.0 ** -17
    assert dev_slacks(8, torch.bfloat16, "t1000", False)[2] < SLACK_P + 2 * U  # bias corrections 1: one rounding each


def test_tolerances_are_half_an_ulp_plus_slack():
    ref = AdamWRef(*(torch.tensor(x, dtype=torch.float64) for x in ([0.0], [0.0], [1.5], [0.0], [0.0], [2.0 ** -10])))
    tol_p, tol_w, s, h32 = master_tolerance(ref, SLACK_P)
    assert float(h32) == 2.0 ** -24 and float(s) == 2.0 ** -30 and float(tol_p) == 2.0 ** -24 + 2.0 ** -30
    assert float(tol_w) == 2.0 ** -8 + float(tol_p)
    near = AdamWRef(*(torch.tensor(x, dtype=torch.float64) for x in ([0.0], [0.0], [2.0 - 2.0 ** -40], [0.0], [0.0], [1.0])))
    assert float(master_tolerance(near, SLACK_P)[3]) == 2.0 ** -23  # the slack carries the value over 2.0


# ================================================================================ the rule against itself
@pytest.mark.parametrize("hp_name", list(HYPERS))
@pytest.mark.parametrize("gdtype", GDTYPES)
@pytest.mark.parametrize("n", FLAT_SMALL + [1 << 16])
def test_emulation_passes_in_both_contraction_forms_and_the_tolerance_is_tight(n, gdtype, hp_name):
    c = small_case(n, gdtype, hp_name)
    for contract in (False, True):
        name = f"adamw n={n} {str(gdtype)[6:]} {hp_name} {'fma' if contract else 'mul+add'}"
        figures = assert_adamw(name, emulate(c, contract), c["ref"], exempt=c["exempt"], cap=case_cap(hp_name))
        assert_within_the_counts(figures)
    if hp_name == "t1":
        print(f"  step sharpness: tolerance <= 2^-18 of the step on {assert_step_sharpness(c, c['ref']):.2%}")


@pytest.mark.parametrize("clip,partials", [(CLIP, True), (-1.0, True), (CLIP, False)])
@pytest.mark.parametrize("gdtype", GDTYPES)
def test_emulation_of_the_device_form_passes_its_slack(gdtype, clip, partials):
    """The device form's scalars in fp32 (sum of squares by an fp32 ``sum``, sqrt, the division, ``pow``) and the
    update with them, against the float64 derivation."""
    c = small_case(8 * 257, gdtype, "train")
    ref, slacks, hp64 = dev_reference(c, clip, partials)
    lr, b1, b2, eps, wd, gs, t = HYPERS["train"]
    f = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    gsf = f(gs)
    if partials and clip > 0:
        norm = (c["g"].float() ** 2).sum().sqrt() * gsf
        assert float(norm) > 10 * clip  # the clip is active
        fac = f(clip) / (norm + f(1e-6))
        gsf = gsf * torch.where(fac > 1, f(1.0), fac)
    else:
        assert hp64[5] == gs
    hp = torch.stack([f(lr), f(b1), f(b2), f(eps), f(wd), gsf, 1 - f(b1) ** f(float(t)), 1 - f(b2) ** f(float(t))])
    for contract in (False, True):
        figures = assert_adamw(f"adamw dev clip={clip} partials={partials} {str(gdtype)[6:]}", emulate(c, contract, hp=hp), ref, slacks,
                               exempt=c["exempt"], cap=None)
        assert_within_the_counts(figures)


def _mutant_run(c, mutant):
    res, _, _ = compare_adamw(mutant, emulate(c, mutant=mutant), c["ref"], exempt=c["exempt"], cap=None)
    return {k: r[0] for k, r in res.items()}, {k: r[2] for k, r in res.items()}


@pytest.mark.parametrize("hp_name", list(HYPERS))
@pytest.mark.parametrize("gdtype", GDTYPES)
def test_every_mutant_fails_at_the_elements_it_touches(gdtype, hp_name):
    n = 8 * 257
    c = small_case(n, gdtype, hp_name)
    ref, planted = c["ref"], c["planted"]
    ordinary = (planted == 0) & ~c["exempt"]
    band = c["exempt"] & (planted == 0)
    none = torch.zeros(n, dtype=torch.bool)
    lane = lambda i: planted == i + 1  # noqa: E731
    share = lambda bad, where: float(bad[where].double().mean())  # noqa: E731
    summary = []

    def run(mutant, touched_state, touched_p):
        """bad must stay inside the touched elements: m and v inside ``touched_state`` (None = untouched outputs),
        master and w inside ``touched_p``; and the mutant must fail."""
        bad, rep = _mutant_run(c, mutant)
        for k in ("m", "v"):
            assert not bool((bad[k] & ~(none if touched_state is None else touched_state[k])).any()), (mutant, k)
        for k in ("master", "w"):
            assert not bool((bad[k] & ~touched_p).any()), (mutant, k)
        assert any(bool(b.any()) for b in bad.values()), mutant
        summary.append(f"{mutant}: " + ", ".join(f"{k} {int(b.sum())}" for k, b in bad.items()))
        return bad, rep

    everywhere = torch.ones(n, dtype=torch.bool)
    # eps left out: 0 / 0 where m = v = g = 0, and a denominator off by its own size where eps decides
    bad, rep = run("eps omitted", None, everywhere)
    for i in (1, 2, 7):
        assert bool(bad["master"][lane(i)].all()), PLANTS[i]
    assert "element 1:" in rep["master"]
    bad, _ = run("eps under the square root", None, everywhere)
    assert bool(bad["master"][lane(2) | lane(7)].all())  # sqrt(eps) = 1e-4 against a denominator of the order of 1e-8
    # the decay term: only where the master is not zero (bf16: where it is no bf16 number)
    bad, _ = run("weight decay x 1.05", None, c["master"] != 0)
    assert share(bad["master"], ordinary) > 0.9 and not bool(bad["master"][lane(3) | lane(4)].any())
    bad, _ = run("decay from the bf16 weight", None, c["master"].to(torch.bfloat16).float() != c["master"])
    assert share(bad["master"], ordinary) > 0.5
    bad, _ = run("decay of the updated master", None, ref.m != 0)
    assert share(bad["master"], band) > 0.9 and not bool(bad["master"][lane(1)].any())
    if hp_name == "t1000":  # both corrections are 1.0f: the swap changes nothing, and nothing may fail
        same, swapped = emulate(c), emulate(c, mutant="bc1 and bc2 swapped")
        assert all(torch.equal(same[k], swapped[k]) for k in same) and float(c["hp"][6]) == float(c["hp"][7]) == 1.0
    else:
        bad, _ = run("bc1 and bc2 swapped", None, ref.m != 0)
        assert share(bad["master"], ordinary) > 0.9
    gnz = c["g"].float() != 0
    bad, _ = run("grad_scale after squaring", {"m": none, "v": gnz}, gnz)
    assert share(bad["v"], ordinary) > 0.9 and share(bad["master"], ordinary) > 0.9
    bad, rep = _mutant_run(c, "bf16 weight truncated")
    assert not any(bool(bad[k].any()) for k in ("m", "v", "master")) and 0.3 < share(bad["w bits"], everywhere) < 0.6
    assert "not the kernel's own master rounded" in rep["w bits"]
    summary.append(f"bf16 weight truncated: w bits {int(bad['w bits'].sum())}, w {int(bad['w'].sum())}")
    for mutant, vec in (("one vector stale", STALE_VECTOR), ("last vector of a block skipped", 255)):
        at = torch.zeros(n, dtype=torch.bool)
        at[8 * vec:8 * vec + 8] = True
        bad, rep = run(mutant, {"m": at, "v": at}, at)
        for k in ("m", "v", "master"):
            assert int(bad[k].sum()) >= 7, (mutant, k, int(bad[k].sum()))
        assert f"element {8 * vec}:" in rep["m"] and not bool(bad["w bits"].any())  # old w = old master rounded
    print(f"mutants n={n} {str(gdtype)[6:]} {hp_name} (bad elements per output):\n  " + "\n  ".join(summary))


OLD_TOL = {"m": (1e-5, 1e-6), "v": (1e-5, 1e-7), "master": (1e-5, 1e-6)}  # (rtol, atol) of the former root test


@pytest.mark.parametrize("gdtype", GDTYPES)
def test_the_former_allclose_tolerances_accept_wrong_kernels(gdtype):
    """Why the rule exists.  The former root of the AdamW chain (tests/test_fused_gpu.py) held the kernel to an
    op-by-op fp32 reference with ``allclose(rtol=1e-5, atol=1e-6)``: with lr = 1e-3 and |master| ~ 1 that is about
    1 % of the step.  On inputs of its kind (plain seeded randn, the training hyper-parameters) it accepts every
    mutant that changes the step by less than that; the rule rejects each of them on the same inputs."""
    c = small_case(1 << 16, gdtype, "train", plain=True)
    base = emulate(c)
    accepted, rejected_by_rule = [], []
    for mutant in MUTANTS[:7]:  # the arithmetic mutants; the last three are about W's bits and untouched vectors
        got = emulate(c, mutant=mutant)
        if all(torch.allclose(got[k], base[k], rtol=r, atol=a) for k, (r, a) in OLD_TOL.items()):
            accepted.append(mutant)
        res, _, _ = compare_adamw(mutant, got, c["ref"], cap=None)
        if any(r[2] for r in res.values()):
            rejected_by_rule.append(mutant)
    print(f"former allclose tolerances, n=65536 {str(gdtype)[6:]}: accept {accepted}")
    assert {"eps omitted", "weight decay x 1.05", "decay from the bf16 weight", "decay of the updated master"} <= set(accepted)
    assert not {"bc1 and bc2 swapped", "grad_scale after squaring"} & set(accepted)  # changes of the step's own size
    assert rejected_by_rule == list(MUTANTS[:7])
