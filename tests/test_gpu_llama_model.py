"""The Llama training step on the GPU (models/llama.py + ops/fused.py: the composition of the HIP kernels)
against the float64 reference of the whole model, parameter by parameter (run on a real MI355X:
``pytest -m gpu``).  The rule, the cases, their inputs and the proof that the rule can fail are in
tests/test_llama_model_ref.py; every figure is printed before it is asserted (``pytest -s``).

What the rule cannot see is held bit for bit here: the causal mask (a future token cannot reach an earlier
logit or any gradient), and ``checkpoint=True`` against ``checkpoint=False``.
"""
import pytest
import torch

from test_llama_model_ref import (CASES, IGNORE, RESIDENT_WT, assert_rule, case_inputs, case_reference, reference, split)

pytestmark = pytest.mark.gpu


def _model(cfg, data, **kw):
    """The GPU model on the given flat weights, with the constructor's defaults unless ``kw`` says otherwise."""
    from gpu_topology_on_k8s_amd.models.llama import Llama

    assert torch.cuda.is_available(), "needs a GPU"
    m = Llama(cfg, device="cuda", **kw)
    with torch.no_grad():
        m.flat.data.copy_(data)
    m.flat.invalidate_t()
    assert m.flat_grads and m.training
    return m


def _step(m, tokens, labels):
    """zero_grad, forward, backward -> (loss, {name: gradient on the CPU}); no offered transpose is left over."""
    from gpu_topology_on_k8s_amd.ops import fused

    m.flat.zero_grad()
    loss = m(tokens.cuda(), labels.cuda())
    loss.backward()
    torch.cuda.synchronize()
    assert not fused._PENDING_T
    return float(loss.detach()), split(m.cfg, m.flat.grad.cpu())


def _assert_paths(m, case, tokens, nt=True):
    """The case runs the paths it is there for; a later change of a threshold cannot quietly move it."""
    from gpu_topology_on_k8s_amd.ops import fused

    cfg = m.cfg
    B, S = tokens.shape
    q = torch.empty(B, cfg.n_heads, S, cfg.head_dim, device="cuda", dtype=torch.bfloat16)
    k = torch.empty(B, cfg.n_kv_heads, S, cfg.head_dim, device="cuda", dtype=torch.bfloat16)
    assert fused.flash_attention_supported(q, k) and m.attn == "hip"
    if not nt:
        assert not m.flat.t_offsets and not m.flat.producer_xt and not m.attn_ot
        return
    assert m.flat.producer_xt and m.attn_ot and m.persistent_wt
    want = {f"l{i}.{p}" for i in range(cfg.n_layers) for p in RESIDENT_WT[case] if p != "lm_head"}
    want |= {"lm_head"} & set(RESIDENT_WT[case])
    assert set(m.flat.t_offsets) == want
    flat_fallbacks = cfg.vocab % 128 != 0 and cfg.ffn_dim % 64 != 0  # flat xent / SwiGLU kernels, torch-copy transposes
    assert flat_fallbacks == (case == "F")


# ================================================================================ a. the per-parameter rule
@pytest.mark.parametrize("case,layout", [(c, "nt") for c in CASES] + [("P", "native")])
def test_every_parameter_gradient_against_float64(case, layout):
    cfg, data, tokens, labels = case_inputs(case)
    m = _model(cfg, data, gemm_layout=layout)
    _assert_paths(m, case, tokens, nt=layout == "nt")
    loss, g = _step(m, tokens, labels)
    assert_rule(f"gpu {case} {layout}", loss, g, case_reference(case))


# ================================================================================ b. after an optimizer step
def test_gradient_after_an_optimizer_step_against_float64_at_the_new_weights():
    """Backward, one FlatAdamW step (which writes W and the resident W^T), forward and backward again: the
    second gradient against the float64 step at the weights read back from the GPU.  A W^T that did not
    follow the update fails at every parameter upstream of it."""
    from gpu_topology_on_k8s_amd.models.optim import FlatAdamW

    cfg, data, tokens, labels = case_inputs("P")
    m = _model(cfg, data)
    opt = FlatAdamW(m.flat, lr=1e-3)
    assert opt.fused_t
    _step(m, tokens, labels)
    m.flat.fill_unwritten()
    opt.step()
    made = m.flat.t_refreshes
    new = m.flat.data.cpu()
    moved = float((new.float() - data.float()).norm() / data.float().norm())
    print(f"weights moved by {moved:.4f} of their norm")
    assert moved > 0.01  # far above the rule's allowance: stale weights cannot pass
    loss, g = _step(m, tokens, labels)
    assert m.flat.t_refreshes == made == len(m.flat.t_offsets)  # the W^T the optimizer wrote is what backward read
    assert_rule("gpu P after AdamW", loss, g, reference(cfg, new, tokens, labels))


# ================================================================================ c. the causal mask, bit for bit
@pytest.mark.parametrize("cut", [128, 192])
def test_future_tokens_reach_no_earlier_logit_and_no_gradient(cut):
    """Other ids at every position >= cut: the logits before the cut keep their bits (GEMM rows are
    independent, the attention's online softmax is per row), and with every label from the cut on ignored
    the whole flat gradient keeps its bits (every dlogits row there is exactly zero and adds exact zeros
    to every sum; 0.0 is added to clear the sign of zero).  128 is a tile boundary of the attention
    kernels, 192 is not: there the diagonal tile's mask separates the halves."""
    cfg, data, tokens, labels = case_inputs("P")
    g = torch.Generator().manual_seed(cut)
    other = tokens.clone()
    other[:, cut:] = (tokens[:, cut:] + 1 + torch.randint(0, cfg.vocab - 1, tokens[:, cut:].shape, generator=g)) % cfg.vocab
    assert bool((other[:, cut:] != tokens[:, cut:]).all()) and torch.equal(other[:, :cut], tokens[:, :cut])
    m = _model(cfg, data)
    m.eval()
    with torch.no_grad():
        a, b = m(tokens.cuda()), m(other.cuda())
    assert a.shape == (*tokens.shape, cfg.vocab)
    assert torch.equal(a[:, :cut], b[:, :cut])
    assert not torch.equal(a[:, cut:], b[:, cut:])
    m.train()
    masked = labels.clone()
    masked[:, cut:] = IGNORE
    grads = []
    for t in (tokens, other):
        _step(m, t, masked)
        grads.append(m.flat.grad.clone() + 0.0)
    assert bool(grads[0].any()) and torch.equal(grads[0], grads[1])


# ================================================================================ d. activation checkpointing
def test_checkpointed_layers_give_the_same_bits_and_really_recompute(monkeypatch):
    """``Llama(checkpoint=True)`` (models/train.py --checkpoint) re-runs every layer inside backward: loss and
    flat gradient equal ``checkpoint=False`` bit for bit over two steps with a weight update between, no
    offered transpose is left over, and the attention forward runs twice per layer and step, not once."""
    from gpu_topology_on_k8s_amd.models.optim import FlatAdamW
    from gpu_topology_on_k8s_amd.ops import fused

    cfg, data, tokens, labels = case_inputs("P")
    native = fused.hip()
    calls = [0]
    inner = native.attn_fwd_t

    def counted(*args):
        calls[0] += 1
        return inner(*args)

    monkeypatch.setattr(native, "attn_fwd_t", counted)
    runs = {}
    for ckpt in (False, True):
        m = _model(cfg, data, checkpoint=ckpt)
        opt = FlatAdamW(m.flat, lr=1e-3)
        out = []
        for _ in range(2):
            calls[0] = 0
            loss, _ = _step(m, tokens, labels)
            assert calls[0] == cfg.n_layers * (2 if ckpt else 1), (ckpt, calls[0])
            out.append((loss, m.flat.grad.clone()))
            m.flat.fill_unwritten()
            opt.step()
        runs[ckpt] = out
    for (la, ga), (lb, gb) in zip(runs[False], runs[True]):
        assert la == lb and torch.equal(ga, gb)
    assert not torch.equal(runs[True][0][1], runs[True][1][1])  # the update between the steps took place


# ================================================================================ e. ignored rows
def test_a_sample_of_ignored_labels_is_inert():
    """Case MHA with every label of sample 1 ignored: the mean is over the valid labels, so the gradient is
    that of the batch without the sample, scaled by nothing -- every parameter under the rule against the
    float64 step of the two-sample batch."""
    cfg, data, tokens, labels = case_inputs("MHA")
    masked = labels.clone()
    masked[1] = IGNORE
    m = _model(cfg, data)
    loss, g = _step(m, tokens, masked)
    assert_rule("gpu MHA, sample 1 ignored", loss, g, reference(cfg, data, tokens[[0, 2]], labels[[0, 2]]))
