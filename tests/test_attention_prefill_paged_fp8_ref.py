"""CPU: prefill attention and the ragged chunk append over the fp8 paged KV cache.  The references against the bf16
ones on dequantised pools, the append byte for byte against ``kv_quantize_ref``, its skips, the refusals of the two
public functions, and the build of the kernel."""
import os
import sys

import pytest
import torch

import test_attention_ref as A
from gpu_topology_on_k8s_amd.ops import fused
from test_attention_prefill_paged_ref import CPU_CASE, REPO, prefill_inputs

BF = torch.bfloat16


def fp8_inputs(family="randn"):
    """-> (q, k_codes, v_codes, k_exp, v_exp, table, kv_len, q_len) of CPU_CASE, and its bf16 pools and slabs."""
    (q, kp, vp, table, kv_len, q_len), slabs, _ = prefill_inputs(CPU_CASE, family)
    (kc, ke), (vc, ve) = fused.kv_quantize_ref(kp), fused.kv_quantize_ref(vp)
    return (q, kc, vc, ke, ve, table, kv_len, q_len), (kp, vp), slabs


@pytest.mark.parametrize("family", ["randn", "peaked"])
def test_cpu_call_and_reference_equal_the_bf16_reference_on_dequantised_pools(family):
    (q, kc, vc, ke, ve, table, kv_len, q_len), _, _ = fp8_inputs(family)
    want = fused.attention_prefill_paged_ref(q, fused.kv_dequantize_ref(kc, ke), fused.kv_dequantize_ref(vc, ve), table, kv_len, q_len, A.SCALE)
    for got in (fused.attention_prefill_paged_fp8_ref(q, kc, vc, ke, ve, table, kv_len, q_len, A.SCALE),
                fused.attention_prefill_paged_fp8(q, kc, vc, ke, ve, table, kv_len, q_len, A.SCALE, return_lse=True, check=True)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert bool((want[0][1, 17:] == 0).all()) and bool(torch.isfinite(want[0][1, :17].float()).all())


def test_append_in_two_ragged_chunks_gives_the_quantised_pools_byte_for_byte():
    (_, kc, vc, ke, ve, table, kv_len, q_len), (kp, vp), (k, v) = fp8_inputs()
    pools = [torch.full_like(x, 0x7F) for x in (kc, vc, ke, ve)]
    first = kv_len - q_len  # (60, 113, 9): pure prefill of three different lengths, then the case's own chunk
    for lens, qls in ((first, first), (kv_len, q_len)):
        Sq = int(qls.max())
        new = [torch.stack([torch.cat([x[b, :, n - m:n], x.new_full((x.size(1), Sq - m, A.D), float("nan"))], 1)
                            for b, (n, m) in enumerate(zip(lens.tolist(), qls.tolist()))]) for x in (k, v)]
        fused.kv_cache_append_prefill_fp8(*new, *pools, table, lens, qls, check=True)
    used = ~kp.isnan().all(-1)  # an unused row is all NaN: its codes quantise to 0x7f, its exponent byte was never written
    assert int(used.sum()) == 2 * (100 + 130 + 9)
    for got, want in zip(pools, (kc, vc, torch.where(used, ke, 0x7F), torch.where(used, ve, 0x7F))):
        assert torch.equal(got, want)
    new = torch.randn(3, 2, 5, A.D, generator=A._gen("fp8 chunk")).to(BF)  # a full chunk of Sq <= 32: the decode append's reference
    ref = [x.clone() for x in pools]
    fused.kv_cache_append_fp8_ref(new, -new, *ref, table, kv_len)
    fused.kv_cache_append_prefill_fp8(new, -new, *pools, table, kv_len)
    assert all(torch.equal(a, b) for a, b in zip(pools, ref)) and not torch.equal(pools[0], kc)


def test_append_skips_touch_no_other_byte():
    (_, kc, vc, ke, ve, table, _, _), _, _ = fp8_inputs()
    pools = [x.clone() for x in (kc, vc, ke, ve)]
    new = torch.ones(3, 2, 5, A.D, dtype=BF)
    bad = table.clone()
    bad[1, 2] = kc.size(0)  # rows 128, 129 of sequence 1 have no page; sequence 0's length is below its q_len; 2 is idle
    fused.kv_cache_append_prefill_fp8(new, new, *pools, bad, torch.tensor([2, 130, 9], dtype=torch.int32), torch.tensor([3, 4, 0], dtype=torch.int32))
    page = int(table[1, 1])
    for codes, exp, c0, e0 in ((pools[0], pools[2], kc, ke), (pools[1], pools[3], vc, ve)):
        assert (codes != c0).any(-1).nonzero().tolist() == [[page, h, r] for h in (0, 1) for r in (62, 63)]  # positions 126, 127
        assert bool((codes[page, :, 62:] == 0x78).all()) and bool((exp[page, :, 62:] == 119).all())  # 1 = 256 * 2^-8
        exp[page, :, 62:] = e0[page, :, 62:]
        assert torch.equal(exp, e0)


@pytest.mark.parametrize("change,msg", [
    (dict(x=lambda t: t.float()), "must be a bf16"),
    (dict(kc=lambda t: t.to(torch.int8)), "k_codes must be a uint8"),
    (dict(ke=lambda t: t[:, :, :-1]), "k_exp and v_exp must be"),
    (dict(**{n: (lambda t: t.repeat_interleave(2, 2)[:, :, :96].contiguous()) for n in ("kc", "vc", "ke", "ve")}),
     "page_size must be a multiple of 64"),
    (dict(x=lambda t: t.repeat(1, 1, 5, 1)), r"Sq must be between 1 and max_pages \* page_size = 192, got 200"),
    (dict(q_len=lambda t: t.long()), "q_len must be an int32"),
    (dict(kv_len=lambda t: t + 63, check=True), r"kv_len must lie in \[q_len, 192\]"),
])
def test_a_call_that_breaks_a_requirement_is_refused(change, msg):
    args = dict(zip(("x", "kc", "vc", "ke", "ve", "table", "kv_len", "q_len"), fp8_inputs()[0]))
    kw = {key: val for key, val in change.items() if key not in args}
    new = torch.ones(3, 2, 40, A.D, dtype=BF)
    args, app = dict(args), dict(args, x=new)
    args.update({key: fn(args[key]) for key, fn in change.items() if key in args})
    app.update({key: fn(app[key]) for key, fn in change.items() if key in app})
    with pytest.raises(ValueError, match="attention_prefill_paged_fp8: .*" + msg):
        fused.attention_prefill_paged_fp8(*args.values(), A.SCALE, **kw)
    with pytest.raises(ValueError, match="kv_cache_append_prefill_fp8: .*" + msg):
        fused.kv_cache_append_prefill_fp8(app["x"], app["x"], *list(app.values())[1:], **kw)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_fp8_prefill_kernel_is_built_without_scratch_for_two_workgroups_a_cu(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa

    st = isa.kernel_stats(os.path.join(REPO, "csrc", "ops", "attention_prefill_paged_fp8.hip"), out=str(tmp_path / "prefill8.s"))
    (k,) = [v for name, v in st.items() if "attn_prefill_paged_fp8_kernel" in name]
    assert k["ScratchSize"] == 0 and k["scratch"] == 0 and k["Occupancy"] == 2 and k["LDSByteSize"] <= 80 * 1024, k
