"""GPU: decode attention over the fp8 paged KV cache (``_fused.attn_decode_paged_fp8``,
``fused.attention_decode_paged_fp8``) and the quantising append (``_fused.kv_append_paged_fp8``,
``fused.kv_cache_append_fp8``).  Inputs are the pools of tests/test_gpu_attention_paged.py with K rows multiplied by
2^(row % 3 - 1) and V rows by 2^(row % 9 - 4), so a tile's exponents differ widely and K's from V's, quantised by
``kv_quantize_ref``: the NaN pages and the NaN rows past kv_len[b] become NaN codes.  Each case is held, bit for bit,
to ``_fused.attn_decode_paged`` on the dequantised pools at the same n, and to the float64 reference on the
dequantised slab under the unchanged rule of tests/test_attention_ref.py."""
import functools

import pytest
import torch

import test_attention_ref as A
from gpu_topology_on_k8s_amd.models import attention_ref as R
from gpu_topology_on_k8s_amd.ops import fused
from test_gpu_attention_decode import poison
from test_gpu_attention_paged import CASES, paged_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return fused.hip()


@functools.lru_cache(maxsize=None)
def fp8_inputs(case, family):
    """-> (q, k_codes, v_codes, k_exp, v_exp, block_table, kv_len), the dequantised bf16 pools, the float64 reference."""
    (q, kp, vp, table, kv_len), _, ref = paged_inputs(case, family)
    row = torch.arange(case[4], device="cuda")
    kp = kp * torch.exp2((row % 3 - 1).float()).to(kp.dtype).view(1, 1, -1, 1)
    vp = vp * torch.exp2((row % 9 - 4).float()).to(vp.dtype).view(1, 1, -1, 1)
    (kc, ke), (vc, ve) = fused.kv_quantize_ref(kp), fused.kv_quantize_ref(vp)
    kd, vd = fused.kv_dequantize_ref(kc, ke), fused.kv_dequantize_ref(vc, ve)
    o, lse2, cond = R.attn_decode_ref64(q.cpu(), fused._gather_pages(kd, table).cpu(), fused._gather_pages(vd, table).cpu(),
                                        kv_len.cpu(), A.SCALE)
    return (q, kc, vc, ke, ve, table, kv_len), (kd, vd), {"o": (o, cond) + ref["o"][2:], "lse2": lse2}


def unused(case, table, kv_len):
    """bool [num_pages, 1, page_size]: the rows of unused pages and the rows at or past kv_len[b] of used ones."""
    P, pages = case[4], int(table.max()) + 3
    free = torch.ones(pages, 1, P, dtype=torch.bool, device="cuda")
    for b, n in enumerate(kv_len.tolist()):
        for p in range(-(-n // P)):
            free[table[b, p], 0, :min(P, n - p * P)] = False
    return free


@pytest.mark.parametrize("family", ["randn", "peaked"])
@pytest.mark.parametrize("case", CASES, ids=lambda s: "x".join(map(str, s[:6])) + f"-n{s[7]}")
def test_fp8_decode_against_the_bf16_paged_kernel_and_float64(hip, case, family):
    """Worst err / tol on an MI355X: see profiles/attn_paged_fp8/SUMMARY.md."""
    fp8, (kd, vd), ref = fp8_inputs(case, family)
    n = case[7]
    poison(case[:4] + (None, None, n))
    o, lse2 = hip.attn_decode_paged_fp8(*fp8, A.SCALE, n)
    want = hip.attn_decode_paged(fp8[0], kd, vd, fp8[5], fp8[6], A.SCALE, n)
    print("differing o, lse2:", int((o != want[0]).sum()), int((lse2 != want[1]).sum()))
    A.check(f"fp8 paged decode {case} {family}", {"family": family}, {"o": o, "lse2": lse2}, refs=ref)
    assert torch.equal(o, want[0]) and torch.equal(lse2, want[1])


@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=["Sq1", "Sq4"])
def test_result_does_not_depend_on_unused_bytes(hip, case):
    q, kc, vc, ke, ve, table, kv_len = fp8_inputs(case, "randn")[0]
    want = hip.attn_decode_paged_fp8(q, kc, vc, ke, ve, table, kv_len, A.SCALE, case[7])
    free = unused(case, table, kv_len).expand(-1, case[2], -1)
    for codes, exps in ((0x7F, 0xFF), (0x38, 0x80)):
        pools = [torch.where(free.unsqueeze(-1), codes, x) for x in (kc, vc)] + [torch.where(free, exps, x) for x in (ke, ve)]
        assert not torch.equal(pools[2], ke) and not torch.equal(pools[3], ve)  # the NaN rows' own codes are 0x7f already
        got = hip.attn_decode_paged_fp8(q, *(x.to(torch.uint8) for x in pools), table, kv_len, A.SCALE, case[7])
        assert all(torch.equal(a, b) for a, b in zip(want, got))


@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=["Sq1", "Sq8-across-a-page-edge"])
def test_append_quantises_the_new_rows_and_touches_nothing_else(hip, case):
    (q, kc, vc, ke, ve, table, kv_len), (kd, vd), _ = fp8_inputs(case, "randn")
    B, _, Hkv, Sq, P = case[:5]
    pos = (kv_len.long().view(B, 1) - Sq + torch.arange(Sq, device="cuda"))  # [B, Sq]: where the new rows live
    page, row = table.long().gather(1, pos // P), pos % P
    k_new, v_new = (x[page, :, row].transpose(1, 2).contiguous() for x in (kd, vd))
    k_new[0, 0, 0], v_new[-1, -1, -1] = 0, 0                       # a zero row: e = -100, codes 0
    k_new[-1, 0, -1, :2] = torch.tensor([1.75, 0.4], dtype=k_new.dtype)  # amax at the mantissa's boundary, then just above
    v_new[0, 0, 0, :2] = torch.tensor([-1.7578125, 0.4], dtype=k_new.dtype)
    k_new[-1, 0, -1, 2:], v_new[0, 0, 0, 2:] = k_new[-1, 0, -1, 2:].clamp(-1, 1), v_new[0, 0, 0, 2:].clamp(-1, 1)
    whole = [x.clone() for x in (kc, vc, ke, ve)]  # the four pools with the new rows quantised by the reference
    for new, codes, exps in ((k_new, whole[0], whole[2]), (v_new, whole[1], whole[3])):
        c, e = fused.kv_quantize_ref(new)
        codes[page, :, row], exps[page, :, row] = c.transpose(1, 2), e.transpose(1, 2)
    assert whole[2][page[0, 0], 0, row[0, 0]] == 27 and whole[2][page[-1, -1], 0, row[-1, -1]] == 119 and whole[3][page[0, 0], 0, row[0, 0]] == 120
    before = [x.clone() for x in whole]
    for x in before:
        x[page, :, row] = 0x7F
    got, ref = [x.clone() for x in before], [x.clone() for x in before]
    fused.kv_cache_append_fp8_ref(k_new, v_new, *ref, table, kv_len)
    fused.kv_cache_append_fp8(k_new, v_new, *got, table, kv_len, check=True)
    for g, r, w in zip(got, ref, whole):  # byte for byte the reference's, and nothing outside the new rows moved
        assert torch.equal(g, r) and torch.equal(g, w)
    want = fused.attention_decode_paged_fp8(q, *whole, table, kv_len, A.SCALE, kv_splits=case[7], return_lse=True)
    out = fused.attention_decode_paged_fp8(q, *got, table, kv_len, A.SCALE, kv_splits=case[7], return_lse=True)
    assert all(torch.equal(a, b) for a, b in zip(want, out))


@pytest.mark.parametrize("kv_splits", [1, 3, "auto"])
def test_fused_attention_decode_paged_fp8_dispatches_kv_splits(hip, kv_splits):
    fp8 = fp8_inputs(CASES[4], "randn")[0]
    n = fused.decode_splits_for(1, 8, 5 * 256) if kv_splits == "auto" else kv_splits
    want = hip.attn_decode_paged_fp8(*fp8, A.SCALE, n)
    o, lse2 = fused.attention_decode_paged_fp8(*fp8, A.SCALE, kv_splits=kv_splits, return_lse=True, check=True)
    assert torch.equal(o, want[0]) and torch.equal(lse2, want[1])
    assert torch.equal(fused.attention_decode_paged_fp8(*fp8, A.SCALE, kv_splits=kv_splits), o)


@pytest.mark.parametrize("kw,msg", [
    (dict(n=65), "kv_splits must be between 1 and 64, got 65"),
    (dict(P=96), "page_size must be a multiple of 64 from 64 to 1024, got 96"),
    (dict(long=True), "block_table must be a contiguous int32"),
    (dict(exp_rows=32), "k_exp and v_exp must be"),
])
def test_a_native_call_that_breaks_a_requirement_is_refused(hip, kw, msg):
    q = torch.ones(1, 2, 1, A.D, dtype=torch.bfloat16, device="cuda")
    P = kw.get("P", 64)
    codes = torch.zeros(2, 1, P, A.D, dtype=torch.uint8, device="cuda")
    exps = torch.full((2, 1, kw.get("exp_rows", P)), 127, dtype=torch.uint8, device="cuda")
    table = torch.zeros(1, 1, dtype=torch.int64 if kw.get("long") else torch.int32, device="cuda")
    kv_len = torch.full((1,), 8, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match=msg):
        hip.attn_decode_paged_fp8(q, codes, codes, exps, exps, table, kv_len, A.SCALE, kw.get("n", 1))
    if "n" not in kw:
        with pytest.raises(RuntimeError, match=msg):
            hip.kv_append_paged_fp8(q[:, :1], q[:, :1], codes, codes.clone(), exps, exps.clone(), table, kv_len)
