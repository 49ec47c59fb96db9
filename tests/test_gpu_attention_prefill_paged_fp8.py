"""GPU: prefill attention over the fp8 paged KV cache (``_fused.attn_prefill_paged_fp8``,
``fused.attention_prefill_paged_fp8``) and the quantising chunk append (``_fused.kv_append_paged_chunk_fp8``,
``fused.kv_cache_append_prefill_fp8``).  The shapes are those of tests/test_gpu_attention_prefill_paged.py, already the
smallest at which this walk can go wrong (one key; offset 37 with the diagonal over three tiles; ragged chunks across
page edges with an idle slot; two and three tiles a page; 71 tiles, past one id vector; shared pages), and lengths 165
and 333 leave the exponent descriptor's round-up-to-4 a partial dword.  The pools are made as the fp8 decode test makes
them: K rows times 2^(row % 3 - 1), V rows times 2^(row % 9 - 4), quantised by ``kv_quantize_ref``, so the NaN pages and
the NaN rows at or past kv_len[b] become NaN codes.  Each case is held, bit for bit, to ``_fused.attn_prefill_paged`` on
the dequantised pools, and to a float64 reference on the dequantised slab under the unchanged rule of
tests/test_attention_ref.py."""
import functools

import pytest
import torch

import test_attention_ref as A
from gpu_topology_on_k8s_amd.models import attention_ref as R
from gpu_topology_on_k8s_amd.ops import fused
from test_attention_prefill_paged_ref import check_rows, prefill_inputs
from test_gpu_attention_prefill_paged import CASES, LONG_CHUNK, RAGGED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return fused.hip()


@functools.lru_cache(maxsize=None)
def fp8_inputs(case, family="randn"):
    """-> (q, k_codes, v_codes, k_exp, v_exp, table, kv_len, q_len) on the GPU, the dequantised bf16 pools, and per
    sequence the float64 reference of its real rows on the dequantised slab, in the form ``check_rows`` takes."""
    (q, kp, vp, table, kv_len, q_len), _, _ = prefill_inputs(case, family)
    row = torch.arange(case[4])
    kp = kp * torch.exp2((row % 3 - 1).float()).to(kp.dtype).view(1, 1, -1, 1)
    vp = vp * torch.exp2((row % 9 - 4).float()).to(vp.dtype).view(1, 1, -1, 1)
    (kc, ke), (vc, ve) = fused.kv_quantize_ref(kp), fused.kv_quantize_ref(vp)
    kd, vd = fused.kv_dequantize_ref(kc, ke), fused.kv_dequantize_ref(vc, ve)
    k, v = fused._gather_pages(kd, table), fused._gather_pages(vd, table)
    refs = []
    for b, (n, m) in enumerate(zip(case[6], case[7])):
        if m:
            o, lse2, cond = R.attn_decode_ref64(q[b:b + 1, :, :m], k[b:b + 1], v[b:b + 1], kv_len[b:b + 1], A.SCALE)
            refs.append({"o": (o, cond, None, (n - m + 1 + torch.arange(m)).double().view(1, m, 1, 1)), "lse2": lse2})
        else:
            refs.append(None)
    return tuple(x.cuda() for x in (q, kc, vc, ke, ve, table, kv_len, q_len)), (kd.cuda(), vd.cuda()), refs


@pytest.mark.parametrize("family", ["randn", "peaked"])
@pytest.mark.parametrize("case", CASES, ids=lambda s: "x".join(map(str, s[:6])))
def test_fp8_prefill_against_the_bf16_paged_kernel_and_float64(hip, case, family):
    """Worst err / tol on an MI355X and of the fp32 reference on the CPU: see profiles/attn_prefill_paged_fp8/SUMMARY.md."""
    fp8, (kd, vd), refs = fp8_inputs(case, family)
    o, lse2 = hip.attn_prefill_paged_fp8(*fp8, A.SCALE)
    want = hip.attn_prefill_paged(fp8[0], kd, vd, *fp8[5:], A.SCALE)
    print("differing o, lse2:", int((o != want[0]).sum()), int((lse2 != want[1]).sum()))
    check_rows("fp8 paged prefill", case, family, o.cpu(), lse2.cpu(), refs)
    assert torch.equal(o, want[0]) and torch.equal(lse2, want[1])
    got = fused.attention_prefill_paged_fp8(*fp8, A.SCALE, return_lse=True, check=True)
    assert torch.equal(got[0], o) and torch.equal(got[1], lse2)


def test_result_does_not_depend_on_unused_bytes(hip):
    q, kc, vc, ke, ve, table, kv_len, q_len = fp8_inputs(RAGGED)[0]
    want = hip.attn_prefill_paged_fp8(q, kc, vc, ke, ve, table, kv_len, q_len, A.SCALE)
    P = RAGGED[4]
    free = torch.ones(kc.size(0), 1, P, dtype=torch.bool, device="cuda")  # unused pages, and rows at or past kv_len[b]
    for b, n in enumerate(RAGGED[6]):
        for p in range(-(-n // P)):
            free[table[b, p], 0, :min(P, n - p * P)] = False
    free = free.expand(-1, RAGGED[2], -1)
    for codes, exps in ((0x7F, 0xFF), (0x38, 0x80)):
        pools = [torch.where(free.unsqueeze(-1), codes, x) for x in (kc, vc)] + [torch.where(free, exps, x) for x in (ke, ve)]
        assert not torch.equal(pools[2], ke) and not torch.equal(pools[3], ve)
        got = hip.attn_prefill_paged_fp8(q, *(x.to(torch.uint8) for x in pools), table, kv_len, q_len, A.SCALE)
        assert all(torch.equal(a, b) for a, b in zip(want, got))


@pytest.mark.parametrize("case", [RAGGED, LONG_CHUNK], ids=["ragged", "Sq300"])
def test_chunk_append_quantises_the_new_rows_and_touches_nothing_else(hip, case):
    (q, kc, vc, ke, ve, table, kv_len, q_len), (kd, vd), _ = fp8_inputs(case)
    Sq, P = case[3], case[4]
    i = torch.arange(Sq, device="cuda").view(1, Sq)
    real = i < q_len.view(-1, 1)
    pos = ((kv_len - q_len).long().view(-1, 1) + i).clamp(0, case[5] * P - 1)  # [B, Sq]: where the rows live
    pages, rows = table.long().gather(1, pos // P), pos % P
    k_new, v_new = (torch.where(real.view(-1, 1, Sq, 1), x[pages, :, rows].transpose(1, 2), float("nan")).contiguous() for x in (kd, vd))
    k_new[0, 0, 0], v_new[1, -1, 5] = 0, 0                                # a zero row: e = -100, codes 0
    k_new[1, 0, 7, :2] = torch.tensor([1.75, 0.4], dtype=k_new.dtype)     # amax at the mantissa's boundary, then just above
    v_new[0, 0, 0, :2] = torch.tensor([-1.7578125, 0.4], dtype=k_new.dtype)
    k_new[1, 0, 7, 2:], v_new[0, 0, 0, 2:] = k_new[1, 0, 7, 2:].clamp(-1, 1), v_new[0, 0, 0, 2:].clamp(-1, 1)
    page, row = pages[real], rows[real]
    whole = [x.clone() for x in (kc, vc, ke, ve)]  # the four pools with the new rows quantised by the reference
    for new, codes, exps in ((k_new, whole[0], whole[2]), (v_new, whole[1], whole[3])):
        c, e = fused.kv_quantize_ref(new.transpose(1, 2)[real])
        codes[page, :, row], exps[page, :, row] = c, e
    assert whole[2][pages[0, 0], 0, rows[0, 0]] == 27 and whole[2][pages[1, 7], 0, rows[1, 7]] == 119 and whole[3][pages[0, 0], 0, rows[0, 0]] == 120
    before = [x.clone() for x in whole]
    for x in before:
        x[page, :, row] = 0x7F
    got, ref = [x.clone() for x in before], [x.clone() for x in before]
    fused.kv_cache_append_prefill_fp8_ref(k_new, v_new, *ref, table, kv_len, q_len)
    fused.kv_cache_append_prefill_fp8(k_new, v_new, *got, table, kv_len, q_len, check=True)
    for g, r, w in zip(got, ref, whole):  # byte for byte the reference's, and nothing outside the new rows moved
        assert torch.equal(g, r) and torch.equal(g, w)
    want = fused.attention_prefill_paged_fp8(q, *whole, table, kv_len, q_len, A.SCALE, return_lse=True)
    out = fused.attention_prefill_paged_fp8(q, *got, table, kv_len, q_len, A.SCALE, return_lse=True)
    assert all(torch.equal(a, b) for a, b in zip(want, out))


@pytest.mark.parametrize("kw,msg", [
    (dict(long=True), "q_len must be a contiguous int32"),
    (dict(Sq=65), r"Sq must be between 1 and max_pages \* page_size, got 65"),
    (dict(exp_rows=32), "k_exp and v_exp must be"),
])
def test_a_native_call_that_breaks_a_requirement_is_refused(hip, kw, msg):
    q = torch.ones(1, 2, kw.get("Sq", 4), A.D, dtype=torch.bfloat16, device="cuda")
    codes = torch.zeros(2, 1, 64, A.D, dtype=torch.uint8, device="cuda")
    exps = torch.full((2, 1, kw.get("exp_rows", 64)), 127, dtype=torch.uint8, device="cuda")
    table = torch.zeros(1, 1, dtype=torch.int32, device="cuda")
    kv_len = torch.full((1,), 8, dtype=torch.int32, device="cuda")
    q_len = torch.full((1,), 4, dtype=torch.int64 if kw.get("long") else torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match=msg):
        hip.attn_prefill_paged_fp8(q, codes, codes, exps, exps, table, kv_len, q_len, A.SCALE)
    with pytest.raises(RuntimeError, match=msg):
        hip.kv_append_paged_chunk_fp8(q[:, :1], q[:, :1], codes, codes.clone(), exps, exps.clone(), table, kv_len, q_len)
