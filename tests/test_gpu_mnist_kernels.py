"""GPU: the MNIST conv-stack and head kernels (csrc/ops/mnist_conv.hip), called one by one and
compared BIT FOR BIT with the float64 references of models/mnist_ref.py.

The kernels multiply bf16 operands, accumulate in fp32 and round an output once (bf16, nearest even).
With small-integer inputs and a dropout scale of 2 (or 1) every intermediate is an exactly
representable integer, so the correct output does not depend on the summation order: a missing row,
tap, channel, window or partial sum cannot hide behind a tolerance.  Each case asserts that condition
(``conv_exactness_bound`` < 2^24) and that it is not vacuous (most windows positive, tied windows
present, about half the elements dropped).

Batches and the path each one is there for (n1 = 7B dgrad blocks, n2 = min(2B, 128) wgrad blocks of
ceil(24B / n2) rows, the forward handles 32 windows per block of 144B):
  1    smallest launch: n2 = 2, reducer tails only (n1 = 7, n2 = 2), forward tail block (144 = 4*32 + 16)
  2    even batch without a forward tail, n1 = 14, n2 = 4
  3, 5 odd batches: forward tail block; reducer (21, 6) and (35, 10): the 8-deep round once + tail
  64   the README's batch: 128 wgrad blocks of 12 rows (half an image), reducer (448, 128)
  65   wgrad runs of 13 rows that straddle images, last run short (1560 = 120*13), 8 empty blocks
  100  wgrad runs of 19 rows over up to 3 images (2400 = 126*19 + 6), 1 empty block, reducer (700, 128)
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SEED, STEP = 0x7F4A7C15, 7.0
EXACT = float(1 << 24)
CONV_CASES = [(B, 0.5) for B in (1, 2, 3, 5, 64, 65, 100)] + [(B, 0.0) for B in (1, 5, 65)]


@pytest.fixture(scope="module")
def hip():
    from gpu_topology_on_k8s_amd.ops.fused import hip as _hip

    return _hip()


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float64)


def _dev(t, dtype=torch.bfloat16):
    return t.to(dtype).cuda().contiguous()


def _check_equal(name, got, want, axes):
    """``torch.equal`` with a report of where the tensors differ (``axes`` names ``want``'s dims)."""
    got = got.cpu().reshape(want.shape)
    assert got.dtype == want.dtype, (name, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = ((got != want) | (got != got)).nonzero()
    lines = [f"{name}: {len(bad)} of {want.numel()} elements differ; first ones:"]
    for i in bad[:12]:
        where = ", ".join(f"{a} {int(v)}" for a, v in zip(axes, i))
        lines.append(f"  {where}: got {got[tuple(i)].item()} want {want[tuple(i)].item()}")
    for d, a in enumerate(axes):  # which indices of each axis are touched at all
        u = bad[:, d].unique()
        lines.append(f"  {a}: {len(u)} distinct, {u[:16].tolist()}{' ...' if len(u) > 16 else ''}")
    msg = "\n".join(lines)
    print(msg)
    pytest.fail(msg, pytrace=False)


FWD_AXES = ("image", "window", "channel")   # window = 12 * py + px within the image
W2_AXES = ("output channel", "tap", "input channel")  # tap = 3 * ky + kx


@functools.lru_cache(maxsize=None)
def _conv_case(B, p):
    """Integer inputs, the float64 reference of forward and backward, and the case's own checks
    (computed once per (B, p), shared by the forward and the backward test, never modified)."""
    from gpu_topology_on_k8s_amd.models import mnist_ref as R

    g = torch.Generator().manual_seed(1000 + B)
    c = {"B": B, "p": p}
    c["x"], c["w1"], c["b1"] = _ints(g, -2, 2, B, 28, 28), _ints(g, -1, 1, 32, 3, 3), _ints(g, -1, 1, 32)
    c["w2"], c["b2"], c["dp"] = _ints(g, -1, 1, 64, 3, 3, 32), _ints(g, -2, 2, 64), _ints(g, -2, 2, B, 12, 12, 64)
    c["pre"] = [_ints(g, -3, 3, *s) for s in ((32, 3, 3), (32,), (64, 3, 3, 32), (64,))]
    keep = R.dropout_keep(SEED, STEP, B * 9216, p)
    c["keep_frac"] = float(keep.float().mean())
    h1, pooled, code = R.conv_stack_ref(c["x"], c["w1"], c["b1"], c["w2"], c["b2"], keep, p)
    *grads, mid = R.conv_stack_grads_ref(c["x"], h1, c["w2"], code, c["dp"], p, with_intermediates=True)
    c["h1"], c["pooled"], c["code"], c["grads"] = h1, pooled, code, grads
    c["bounds"] = R.conv_exactness_bound(c["x"], c["w1"], c["b1"], c["w2"], c["b2"], h1, mid["dy2"], mid["dz1"], p, preload=3.0)
    c["bounds"]["gradients"] = max(float(t.abs().max()) for t in grads) + 3.0
    c["pos_frac"] = float(((code >> 2) & 1).float().mean())
    # tied windows: recompute the pre-pool stack and count windows whose maximum occurs more than once
    win = R._windows(R._conv2(h1, c["w2"]))
    c["tied"] = int(((win == win.max(0).values).sum(0) > 1).sum())
    c["argmax_hist"] = torch.bincount((code & 3).flatten().long(), minlength=4).tolist()
    return c


def _check_case(c):
    """The exactness condition and the non-vacuity conditions, on the reference side."""
    for what, bound in c["bounds"].items():
        assert bound < EXACT, (what, bound)
    assert all(float(t.abs().max()) > 0 for t in c["grads"])
    assert c["pos_frac"] >= 0.5, c["pos_frac"]
    assert c["tied"] >= 1
    assert min(c["argmax_hist"]) > 0, c["argmax_hist"]
    if c["p"] == 0.5:
        assert 0.45 <= c["keep_frac"] <= 0.55, c["keep_frac"]
    else:
        assert c["keep_frac"] == 1.0


@pytest.mark.parametrize("B,p", CONV_CASES)
def test_conv_forward_exact(hip, B, p):
    """conv1_fwd and conv2_pool_fwd: h1, the pooled map and the code bytes (argmax | pos | keep, the
    keep bit from ``dropout_keep``) equal the reference exactly."""
    from gpu_topology_on_k8s_amd.models.mnist_ref import bf16_round

    c = _conv_case(B, p)
    _check_case(c)
    step = torch.tensor([STEP], device="cuda")
    h1 = hip.mnist_conv1_fwd(_dev(c["x"]), _dev(c["w1"]), _dev(c["b1"]))
    assert h1.shape == (B, 26, 26, 32) and h1.dtype == torch.bfloat16
    want_h1 = bf16_round(c["h1"])
    assert torch.equal(want_h1.double(), c["h1"])  # h1 itself is representable: conv2's input is exact
    _check_equal("h1", h1, want_h1, ("image", "y", "x", "channel"))
    # conv2 on the REFERENCE h1: a conv1 fault cannot leak into this comparison
    pooled, code = hip.mnist_conv2_pool_fwd(_dev(c["h1"]), _dev(c["w2"]), _dev(c["b2"]), step, SEED, p)
    assert pooled.shape == code.shape == (B, 12, 12, 64) and code.dtype == torch.uint8
    _check_equal("code", code.view(B, 144, 64), c["code"].view(B, 144, 64), FWD_AXES)
    _check_equal("pooled", pooled.view(B, 144, 64), bf16_round(c["pooled"]).view(B, 144, 64), FWD_AXES)
    # the seed is taken mod 2^32 and the step as uint32(float)
    pooled2, code2 = hip.mnist_conv2_pool_fwd(h1, _dev(c["w2"]), _dev(c["b2"]), step + 0.25, SEED + (1 << 32), p)
    assert torch.equal(code2, code) and torch.equal(pooled2, pooled)


@pytest.mark.parametrize("B,p", CONV_CASES)
def test_conv_backward_exact(hip, B, p):
    """conv_bwd (dgrad + conv1 wgrad, conv2 wgrad, partials reducer) from the reference's h1 and code
    bytes: all four gradients equal bf16(reference) exactly, written into NaN-filled buffers; a second
    call with accumulate=True into preloaded buffers equals bf16(preload + exact sum)."""
    from gpu_topology_on_k8s_amd.models.mnist_ref import bf16_round

    c = _conv_case(B, p)
    _check_case(c)
    names = ("conv1.w grad", "conv1.b grad", "conv2.w grad", "conv2.b grad")
    shapes = ((32, 9), (32,), (64, 9, 32), (64,))
    axes = (("output channel", "tap"), ("output channel",), W2_AXES, ("output channel",))
    args = [_dev(c["dp"]), c["code"].cuda(), _dev(c["x"]), _dev(c["h1"]), _dev(c["w1"]), _dev(c["b1"]), _dev(c["w2"]), _dev(c["b2"])]
    out = [torch.full(t.shape, float("nan"), dtype=torch.bfloat16, device="cuda") for t in c["grads"]]
    hip.mnist_conv_bwd(*args, *out, p, False)
    for n, s, a, got, want in zip(names, shapes, axes, out, c["grads"]):
        _check_equal(n, got.view(s), bf16_round(want).view(s), a)
    out = [_dev(t) for t in c["pre"]]
    hip.mnist_conv_bwd(*args, *out, p, True)
    for n, s, a, got, want, pre in zip(names, shapes, axes, out, c["grads"], c["pre"]):
        _check_equal(n + " (accumulate)", got.view(s), bf16_round(want + pre).view(s), a)
    if B == 65 and p == 0.5:  # rounding is exercised: many entries are not representable in bf16
        w = c["grads"][2]
        assert float((bf16_round(w).double() != w).float().mean()) > 0.02


# ------------------------------------------------------------------------------ classifier head
@pytest.mark.parametrize("p", [0.5, 0.0])
@pytest.mark.parametrize("B", [1, 15, 17, 300])  # relu_dropout_bwd: 16 row slices -> below, at +-1, many strides
def test_relu_dropout_exact(hip, B, p):
    from gpu_topology_on_k8s_amd.models import mnist_ref as R

    g = torch.Generator().manual_seed(2000 + B)
    h, dy, pre = _ints(g, -3, 3, B, 128), _ints(g, -3, 3, B, 128), _ints(g, -3, 3, 128)
    seed = SEED ^ R.HEAD_SEED_XOR
    keep = R.dropout_keep(seed, STEP, B * 128, p)
    y_ref, mask_ref = R.relu_dropout_ref(h, keep, p)
    dh_ref, gb_ref = R.relu_dropout_bwd_ref(dy, mask_ref, p)
    assert float(gb_ref.abs().max()) + 3 < EXACT and (B < 15 or 0 < int(mask_ref.sum()) < mask_ref.numel())
    if p == 0.0:
        assert torch.equal(mask_ref.bool(), h > 0)
    y, mask = hip.mnist_relu_dropout_fwd(_dev(h), torch.tensor([STEP], device="cuda"), seed, p)
    ax = ("row", "column")
    _check_equal("mask", mask, mask_ref, ax)
    _check_equal("y", y, R.bf16_round(y_ref), ax)
    gb = torch.full((128,), float("nan"), dtype=torch.bfloat16, device="cuda")
    dh = hip.mnist_relu_dropout_bwd(_dev(dy), mask_ref.cuda(), gb, p, False)
    _check_equal("dh", dh, R.bf16_round(dh_ref), ax)
    _check_equal("fc1.b grad", gb, R.bf16_round(gb_ref), ("column",))
    gb = _dev(pre)
    dh = hip.mnist_relu_dropout_bwd(_dev(dy), mask_ref.cuda(), gb, p, True)
    _check_equal("dh (accumulate)", dh, R.bf16_round(dh_ref), ax)
    _check_equal("fc1.b grad (accumulate)", gb, R.bf16_round(gb_ref + pre), ("column",))


XENT_B = [1, 24, 26, 257, 300]  # xent10_bwd: 25 row slices; xent10_fwd: one block of 256 threads striding rows


@pytest.mark.parametrize("B", XENT_B)
def test_xent10_bwd_exact(hip, B):
    """dlogits = g * dlog and fc2's bias gradient: dlog = integers x 2^-6 (7 bits), g = 0.5: every
    product is a bf16 value and every sum an exact fp32 value."""
    from gpu_topology_on_k8s_amd.models import mnist_ref as R

    g = torch.Generator().manual_seed(3000 + B)
    dlog, pre = _ints(g, -127, 127, B, 10) / 64.0, _ints(g, -3, 3, 10)
    d_ref, gb_ref = R.xent10_bwd_ref(dlog, 0.5)
    assert torch.equal(R.bf16_round(d_ref).double(), d_ref) and float(gb_ref.abs().max()) * 128 + 3 * 128 < EXACT
    gs = torch.tensor([0.5], device="cuda")
    gb = torch.full((10,), float("nan"), dtype=torch.bfloat16, device="cuda")
    d = hip.mnist_xent10_bwd(_dev(dlog, torch.float32), gs, gb, False)
    _check_equal("dlogits", d, R.bf16_round(d_ref), ("row", "class"))
    _check_equal("fc2.b grad", gb, R.bf16_round(gb_ref), ("class",))
    gb = _dev(pre)
    d = hip.mnist_xent10_bwd(_dev(dlog, torch.float32), gs, gb, True)
    _check_equal("dlogits (accumulate)", d, R.bf16_round(d_ref), ("row", "class"))
    _check_equal("fc2.b grad (accumulate)", gb, R.bf16_round(gb_ref + pre), ("class",))


XENT_DLOG_BOUND = 1.8e-6  # 8 x the largest error measured on MI355X (2.251e-7, at B = 257)


@pytest.mark.parametrize("B", XENT_B)
def test_xent10_fwd_matches_float64(hip, B):
    """Loss and dlog of ``xent10_fwd`` (fast-math exp / log, so not exact) against float64 on the same
    bf16 logits ~ 3 * randn, every label value present (B >= 10).  Loss: the project's cross-entropy
    bound (atol = rtol = 2e-3).  dlog: max |dlog * B - (softmax - onehot)|, measured on MI355X as
    5.5e-8 (B = 1), 1.21e-7 (24), 1.15e-7 (26), 2.25e-7 (257), 1.44e-7 (300) - a few fp32 ulps of a
    softmax value; the bound is 8 x the largest, a margin for the fast-math ulps varying with the
    inputs.  (The loss differed from float64 by at most 5.5e-7.)"""
    from gpu_topology_on_k8s_amd.models import mnist_ref as R

    g = torch.Generator().manual_seed(4000 + B)
    logits = (torch.randn(B, 10, generator=g) * 3).to(torch.bfloat16)
    labels = (torch.arange(B) % 10)[torch.randperm(B, generator=g)]
    assert B < 10 or len(set(labels.tolist())) == 10
    loss_ref, dlog_ref = R.xent10_ref(logits, labels)
    loss, dlog = hip.mnist_xent10_fwd(logits.cuda(), labels.cuda())
    assert dlog.shape == (B, 10) and dlog.dtype == torch.float32 and loss.dtype == torch.float32
    err_loss = abs(float(loss) - float(loss_ref))
    err = float((dlog.double().cpu() * B - dlog_ref * B).abs().max())
    print(f"xent10_fwd B={B}: loss {float(loss):.6f} ref {float(loss_ref):.6f} err {err_loss:.3e}; max |dlog*B - ref| = {err:.3e}")
    assert err_loss <= 2e-3 + 2e-3 * abs(float(loss_ref)), (float(loss), float(loss_ref))
    assert math.isfinite(err) and err < XENT_DLOG_BOUND, err
