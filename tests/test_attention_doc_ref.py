"""CPU, float64: the document-masked references of models/attention_ref.py and the bounds helpers of
ops/fused.py.  The layouts and dims here are the table tests/test_gpu_attention_doc.py runs on the GPU.

Under the document mask query i sees key j iff doc_start[b, i] <= j <= i, so a packed row is its
documents side by side: every reference output equals the causal reference run on each document alone,
concatenated (to 1e-12; the backward from the same out and lse2)."""
import functools

import pytest
import torch

import test_attention_ref as A
from gpu_topology_on_k8s_amd.models import attention_ref as R
from gpu_topology_on_k8s_amd.ops import fused

LAYOUTS = {  # name: (dims (B, H, Hkv, S), document starts per batch row)
    "one": ((2, 4, 2, 384), [[0], [0]]),
    "aligned": ((2, 4, 2, 384), [[0, 128, 256]] * 2),
    "ragged": ((2, 4, 2, 384), [[0, 1, 37, 64, 127, 129, 200, 383]] * 2),
    "mixed": ((2, 4, 2, 384), [[0, 1, 37, 64, 127, 129, 200, 383], [0]]),
    "late": ((1, 8, 1, 768), [[0, 640]]),
    "short-G3": ((1, 3, 1, 256), [[0, 96, 160]]),
}


def doc_start_of(starts, S):
    """int32 [B, S] from each row's list of document starts."""
    pos = torch.arange(S)
    return torch.stack([torch.tensor(s)[torch.bucketize(pos, torch.tensor(s), right=True) - 1] for s in starts]).int()


@functools.lru_cache(maxsize=None)
def doc_case(layout, family):
    """A.case for a layout: the same inputs, the references under the document mask, the backward from
    the reference's rounded out and lse2.  N of the rule stays the causal chain length, which bounds the
    document's shorter chain from above (that term is 2^-24 N against u = 2^-8)."""
    dims, starts = LAYOUTS[layout]
    c = dict(A.case(dims, family, A.SCALE))
    c["doc_start"] = ds = doc_start_of(starts, dims[3])
    o, lse2, cond_o = R.attn_fwd_ref64(c["q"], c["k"], c["v"], c["scale"], ds)
    assert float(lse2.abs().max()) <= 64.0
    c["out"], c["lse"] = A.bf16_round(o), lse2.float()
    c["ref"] = {"o": (o, cond_o, None, c["ref"]["o"][3]), "lse2": lse2}
    c["ref"].update(doc_backward_refs(c, c["out"], c["lse"]))
    return c


def doc_backward_refs(c, out, lse):
    """A.backward_refs under the case's document mask."""
    base = A.backward_refs(c, out, lse)
    got = R.attn_bwd_ref64(c["do"], c["q"], c["k"], c["v"], out, lse, c["scale"], c["doc_start"])
    dq, dk, dv, cdq, cdk, cdv, c2dq, c2dk = got
    return {"dq": (dq, cdq, c2dq, base["dq"][3]), "dk": (dk, cdk, c2dk, base["dk"][3]), "dv": (dv, cdv, None, base["dv"][3])}


@pytest.mark.parametrize("layout", ["ragged", "mixed", "short-G3"])
def test_document_references_are_the_causal_references_of_each_document(layout):
    c = doc_case(layout, "randn")
    (B, H, Hkv, S), starts = LAYOUTS[layout]
    for b in range(B):
        for s0, s1 in zip(starts[b], starts[b][1:] + [S]):
            cut = lambda t, dim: t[b:b + 1].narrow(dim, s0, s1 - s0)  # noqa: E731
            q, k, v, do = cut(c["q"], 2), cut(c["k"], 2), cut(c["v"], 2), cut(c["do"], 1)
            o, lse2, _ = R.attn_fwd_ref64(q, k, v, c["scale"])
            back = R.attn_bwd_ref64(do, q, k, v, cut(c["out"], 1), cut(c["lse"], 2), c["scale"])
            for name, want, dim in (("o", o, 1), ("lse2", lse2, 2), ("dq", back[0], 2), ("dk", back[1], 2), ("dv", back[2], 2)):
                ref = c["ref"][name]
                torch.testing.assert_close(cut(ref if name == "lse2" else ref[0], dim), want, rtol=1e-12, atol=1e-12)


def test_doc_bounds_gives_doc_end_and_rejects_what_is_no_document_layout():
    ds = doc_start_of([[0, 1, 5], [0]], 8)
    start, end = fused.doc_bounds(ds)
    assert start.dtype == end.dtype == torch.int32 and start.is_contiguous() and end.is_contiguous()
    assert torch.equal(start, ds) and end.tolist() == [[1, 5, 5, 5, 5, 8, 8, 8], [8] * 8]
    for bad in ([0, 1, 1, 0, 0, 0, 0, 0],   # decreasing
                [0, 2, 2, 2, 2, 2, 2, 2],   # above i at i = 1
                [0, 0, 0, 2, 2, 2, 2, 2]):  # token 2 is in document 0, so 2 starts none: not constant inside
        with pytest.raises(ValueError, match="doc_start must satisfy"):
            fused.doc_bounds(torch.tensor([bad]))
    assert fused.doc_bounds(torch.tensor([[0, 2, 2]]), check=False)[0].tolist() == [[0, 2, 2]]


def test_doc_start_from_eos_on_a_hand_written_row():
    tokens = torch.tensor([[5, 9, 7, 9, 9, 3], [9, 1, 1, 1, 1, 9]])
    assert fused.doc_start_from_eos(tokens, 9).tolist() == [[0, 0, 2, 2, 4, 5], [0, 1, 1, 1, 1, 1]]
    assert fused.doc_start_from_eos(tokens, 9).dtype == torch.int32


@pytest.mark.parametrize("attn,checkpoint", [("hip", False), ("hip", True), ("sdpa", False), ("sdpa-expand", False)])
def test_llama_forward_keeps_documents_apart(attn, checkpoint):
    """Llama.forward(tokens, doc_start=...) on the CPU (attention_ref or the dense SDPA mask), with real
    boundaries: replacing the tokens of the first document leaves the logits of the later documents
    bit for bit as they were (every other op is per token), and moves them without ``doc_start``."""
    from gpu_topology_on_k8s_amd.models.llama import Llama, LlamaConfig

    m = Llama(LlamaConfig.tiny(), device="cpu", attn=attn, checkpoint=checkpoint).train(checkpoint)
    tokens = torch.randint(1, 1024, (2, 48), generator=A._gen("doc-llama"))
    tokens[:, [9, 30]] = 0  # EOS: documents [0, 10), [10, 31), [31, 48)
    other = tokens.clone()
    other[:, :9] = (tokens[:, :9] + 17) % 1023 + 1
    ds = fused.doc_start_from_eos(tokens, 0)
    assert ds[0].unique().tolist() == [0, 10, 31] and torch.equal(ds, fused.doc_start_from_eos(other, 0))
    with torch.no_grad():
        a, b = m(tokens, doc_start=ds), m(other, doc_start=ds)
        assert torch.equal(a[:, 10:], b[:, 10:]) and not torch.equal(a[:, :10], b[:, :10])
        assert not torch.equal(m(tokens)[:, 10:], m(other)[:, 10:])
    if checkpoint:  # the checkpointed layer takes the bounds too
        m(tokens, tokens.roll(-1, 1), doc_start=ds).backward()


def test_cpu_attention_fallback_applies_the_document_mask():
    c = doc_case("short-G3", "randn")
    o = fused.attention(c["q"].float(), c["k"].float(), c["v"].float(), doc=fused.doc_bounds(c["doc_start"]))
    torch.testing.assert_close(o.double(), c["ref"]["o"][0], rtol=1e-4, atol=1e-5)
