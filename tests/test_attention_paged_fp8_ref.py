"""CPU: the fp8 paged KV cache.  The row rule of ``kv_quantize_ref`` on hand-picked rows, the references of the fp8
decode and append against the bf16 ones on dequantised pools, the append's skips, the refusals of the two public
functions, and the scratch-free build of the kernel."""
import os
import sys

import pytest
import torch

import test_attention_ref as A
from gpu_topology_on_k8s_amd.ops import fused
from test_attention_paged_ref import CPU_CASE, P, REPO, TABLE, paged_inputs

BF = torch.bfloat16


def quantize_pools(kp, vp):
    """-> (k_codes, v_codes, k_exp, v_exp) of bf16 pools, the argument order of the fp8 calls."""
    (kc, ke), (vc, ve) = fused.kv_quantize_ref(kp), fused.kv_quantize_ref(vp)
    return kc, vc, ke, ve


def fp8_inputs():
    (q, kp, vp, table, kv_len), _ = paged_inputs()
    return q, *quantize_pools(kp, vp), table, kv_len


def row_of(amax):
    x = torch.zeros(128, dtype=BF)
    x[5], x[77] = -amax, amax / 4
    return x


def test_quantize_rule_on_hand_picked_rows():
    up = lambda v: (torch.tensor(v, dtype=BF).view(torch.int16) + 1).view(BF).item()  # noqa: E731  the next bf16 above
    for k in (-20, 0, 3):  # amax = 448 * 2^k keeps e = k and codes +-0x7e; the next bf16 above it takes e = k + 1
        for amax, e in ((448.0 * 2.0 ** k, k), (up(448.0 * 2.0 ** k), k + 1)):
            codes, exp = fused.kv_quantize_ref(row_of(amax))
            assert exp.item() == e + 127 and codes[5].item() == (0xFE if e == k else 0xF6), (k, amax, codes[5], exp)
            assert codes[77].item() == (0x6E if e == k else 0x66)  # amax / 4: two binades down, the same mantissa
    for amax, e in ((1.75, -8), (up(1.75), -7), (1.0, -8), (2.0, -7)):  # 448 = 1.75 * 2^8: the mantissa's boundary
        assert fused.kv_quantize_ref(row_of(amax))[1].item() == e + 127
    codes, exp = fused.kv_quantize_ref(torch.zeros(2, 128, dtype=BF))
    assert exp.tolist() == [27, 27] and not codes.any()  # e = -100
    x = row_of(3.0)
    x[0], x[1], x[2] = float("nan"), float("inf"), float("-inf")
    codes, exp = fused.kv_quantize_ref(x)
    assert exp.item() == 247 and (codes[:3] & 0x7F).tolist() == [0x7F] * 3 and not (codes[3:] & 0x7F).any()  # an Inf counts: e = 120
    x[1], x[2] = 0, 0
    codes, exp = fused.kv_quantize_ref(x)  # a NaN does not: the row keeps the e of amax 3 and its finite codes
    assert exp.item() == 127 - 7 and codes[0].item() & 0x7F == 0x7F and codes[5].item() == 0xFC and codes[77].item() == 0x6C
    assert torch.isnan(fused.kv_dequantize_ref(codes, exp)[0])


def test_quantize_error_bound_and_exact_dequantisation():
    g = A._gen("kv fp8 rule")
    x = (torch.randn(512, 128, generator=g) * torch.exp2(torch.randint(-30, 30, (512, 1), generator=g).float())).to(BF)
    codes, exp = fused.kv_quantize_ref(x)
    deq = fused.kv_dequantize_ref(codes, exp)
    amax = x.double().abs().amax(-1, keepdim=True)
    assert bool(((x.double() - deq.double()).abs() <= amax / 14).all())
    exact = fused._E4M3[codes.long()].double() * torch.exp2(exp.double() - 127).unsqueeze(-1)  # float(code) * 2^e in float64
    assert torch.equal(deq.double(), exact)


def test_cpu_call_and_reference_equal_the_bf16_reference_on_dequantised_pools():
    q, kc, vc, ke, ve, table, kv_len = fp8_inputs()
    want = fused.attention_decode_paged_ref(q, fused.kv_dequantize_ref(kc, ke), fused.kv_dequantize_ref(vc, ve), table, kv_len, A.SCALE)
    for got in (fused.attention_decode_paged_fp8_ref(q, kc, vc, ke, ve, table, kv_len, A.SCALE),
                fused.attention_decode_paged_fp8(q, kc, vc, ke, ve, table, kv_len, A.SCALE, kv_splits=3, return_lse=True, check=True)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_append_then_decode_equals_decode_on_pools_quantised_whole():
    (q, kp, vp, table, kv_len), slab = paged_inputs()
    whole = quantize_pools(kp, vp)
    k_new, v_new = (torch.stack([x[b, :, n - 3:n] for b, n in enumerate(CPU_CASE[5])]) for x in slab[1:3])
    pools = [x.clone() for x in whole]
    for b, n in enumerate(CPU_CASE[5]):  # the pools before the step: other bytes from kv_len - Sq on
        for pos in range(n - 3, n):
            for x in pools:
                x[table[b, pos // P], :, pos % P] = 0x7F
    assert not torch.equal(pools[0], whole[0])
    fused.kv_cache_append_fp8(k_new, v_new, *pools, table, kv_len, check=True)
    assert all(torch.equal(a, b) for a, b in zip(pools, whole))
    got = fused.attention_decode_paged_fp8(q, *pools, table, kv_len, A.SCALE, return_lse=True)
    want = fused.attention_decode_paged_fp8_ref(q, *whole, table, kv_len, A.SCALE)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_append_skips_a_bad_length_and_a_bad_page_id_without_touching_another_byte():
    q, kc, vc, ke, ve, table, kv_len = fp8_inputs()
    before = [x.clone() for x in (kc, vc, ke, ve)]
    new = torch.ones(2, 2, 3, A.D, dtype=BF)
    bad = table.clone()
    bad[1, 2] = kc.size(0)  # row 129 of sequence 1 has no page; sequence 0's length is out of range
    fused.kv_cache_append_fp8_ref(new, new, kc, vc, ke, ve, bad, torch.tensor([2, 130], dtype=torch.int32))
    for codes, exp, c0, e0 in ((kc, ke, before[0], before[2]), (vc, ve, before[1], before[3])):
        assert (codes != c0).any(-1).nonzero().tolist() == [[0, 0, 63], [0, 1, 63]]  # position 127 alone
        assert bool((codes[0, :, 63] == 0x78).all()) and exp[0, :, 63].tolist() == [119, 119]  # 1 = 256 * 2^-8
        exp[0, :, 63] = e0[0, :, 63]
        assert torch.equal(exp, e0)


@pytest.mark.parametrize("change,msg", [
    (dict(q=lambda t: t.float()), "q must be a bf16"),
    (dict(kc=lambda t: t.to(torch.int8)), "k_codes must be a uint8"),
    (dict(kc=lambda t: fused.kv_dequantize_ref(t, t[..., 0]), vc=lambda t: fused.kv_dequantize_ref(t, t[..., 0])), "k_codes must be a uint8"),
    (dict(ve=lambda t: t.float()), "v_exp must be a uint8"),
    (dict(vc=lambda t: t[:-1]), "k_codes and v_codes must be"),
    (dict(ke=lambda t: t[:, :, :-1]), "k_exp and v_exp must be"),
    (dict(ve=lambda t: t.unsqueeze(-1)), "k_exp and v_exp must be"),
    (dict(**{n: (lambda t: t.repeat_interleave(2, 2)[:, :, :96].contiguous()) for n in ("kc", "vc", "ke", "ve")}),
     "page_size must be a multiple of 64"),
    (dict(kc=lambda t: t.transpose(0, 1).contiguous().transpose(0, 1)), "pools must be contiguous"),
    (dict(table=lambda t: t.long()), "block_table must be an int32"),
    (dict(q=lambda t: t.repeat(1, 1, 6, 1)), r"Sq \* \(H / Hkv\) must be between 1 and 32, got 36"),
    (dict(q=lambda t: t.clone().requires_grad_(True)), "forward only"),
    (dict(kv_splits=0), "kv_splits must be 'auto' or an int from 1 to 64"),
    (dict(kv_splits=65), "kv_splits must be 'auto' or an int from 1 to 64"),
    (dict(kv_len=lambda t: t + 63, check=True), r"kv_len must lie in \[3, 192\]"),
    (dict(table=lambda t: t + 3, check=True), r"a needed block_table entry lies outside \[0, 8\)"),
])
def test_a_call_that_breaks_a_requirement_is_refused(change, msg):
    args = dict(zip(("q", "kc", "vc", "ke", "ve", "table", "kv_len"), fp8_inputs()))
    kw = {key: val for key, val in change.items() if key not in args}
    args.update({key: fn(args[key]) for key, fn in change.items() if key in args})
    with pytest.raises(ValueError, match=msg):
        fused.attention_decode_paged_fp8(*args.values(), A.SCALE, **kw)
    if "q" not in change and "kv_splits" not in change:  # the append takes the same pools, table and lengths
        new = torch.ones(2, 2, 3, A.D, dtype=BF)
        with pytest.raises(ValueError, match=msg):
            fused.kv_cache_append_fp8(new, new, *list(args.values())[1:], check=kw.get("check", False))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_fp8_kernel_is_built_without_scratch(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa

    st = isa.kernel_stats(os.path.join(REPO, "csrc", "ops", "attention_decode_paged_fp8.hip"), out=str(tmp_path / "fp8.s"))
    (k,) = [v for name, v in st.items() if "attn_decode_paged_fp8_kernel" in name]
    assert k["ScratchSize"] == 0 and k["scratch"] == 0 and k["mfma"] == 64 and k["LDSByteSize"] == 68 * 1024, k
