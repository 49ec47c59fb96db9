"""GPU: prefill attention over a paged KV cache (``_fused.attn_prefill_paged``, ``fused.attention_prefill_paged``) and
the chunk append (``_fused.kv_append_paged_chunk``, ``fused.kv_cache_append_prefill``).  Inputs are ``prefill_inputs``
cases: every unused page, every row at or past kv_len[b] and every padded q row holds NaN.  Each sequence's real rows
are held to the float64 reference under the unchanged rule of tests/test_attention_ref.py (N = the row's visible
keys), padded rows to exactly 0 and -inf; aligned cases to ``_fused.attn_fwd_qoff`` on the gathered slab bit for bit."""
import pytest
import torch

import test_attention_ref as A
from gpu_topology_on_k8s_amd.ops import fused
from test_attention_prefill_paged_ref import SHARED, check_rows, prefill_inputs

pytestmark = pytest.mark.gpu
CASES = [  # (B, H, Hkv, Sq, page_size, max_pages, kv_len, q_len)
    (1, 1, 1, 1, 64, 1, (1,), (1,)),                          # one key: o is that v row
    (1, 1, 1, 128, 64, 3, (165,), (128,)),                    # offset 37: the diagonal over three tiles, every wave its own pattern
    (3, 4, 2, 200, 64, 6, (200, 333, 64), (200, 77, 0)),      # partial last block; pure prefill; ragged across page edges; idle slot
    (2, 8, 2, 256, 128, 6, (320, 700), (256, 130)),           # G = 4, two tiles a page, both buffer parities, the main loop runs
    (1, 1, 1, 130, 192, 24, (4500,), (130,)),                 # 71 tiles: past the 64 page ids of one vector load; three tiles a page
    SHARED,
]
RAGGED, LONG_CHUNK = CASES[2], (2, 2, 2, 300, 64, 6, (300, 384), (300, 290))  # the append's: 300 rows a sequence in one launch


@pytest.fixture(scope="module")
def hip():
    return fused.hip()


def gpu_inputs(case, family="randn"):
    paged, slabs, refs = prefill_inputs(case, family)
    return tuple(x.cuda() for x in paged), tuple(x.cuda() for x in slabs), refs


@pytest.mark.parametrize("family", ["randn", "peaked"])
@pytest.mark.parametrize("case", CASES, ids=lambda s: "x".join(map(str, s[:6])))
def test_paged_prefill_against_float64(hip, case, family):
    """Worst err / tol on an MI355X: see profiles/attn_prefill_paged/SUMMARY.md."""
    paged, (k, v), refs = gpu_inputs(case, family)
    o, lse2 = hip.attn_prefill_paged(*paged, A.SCALE)
    check_rows("paged prefill", case, family, o.cpu(), lse2.cpu(), refs)
    if case == CASES[0]:
        assert torch.equal(o.view(-1), v[0, 0, 0])
    got = fused.attention_prefill_paged(*paged, A.SCALE, return_lse=True, check=True)
    assert torch.equal(got[0], o) and torch.equal(got[1], lse2)


@pytest.mark.parametrize("prefix", [128, 256])
def test_aligned_chunks_equal_the_offset_kernel_on_the_gathered_slab_bit_for_bit(hip, prefix):
    case = (2, 4, 2, 256, 128, 4, (256 + prefix, 256 + prefix), (256, 256))
    (q, kp, vp, table, kv_len, q_len), (k, v), _ = gpu_inputs(case)
    o, lse2 = hip.attn_prefill_paged(q, kp, vp, table, kv_len, q_len, A.SCALE)
    for b in range(2):  # the offset kernel takes one offset and keys in multiples of 128
        want = hip.attn_fwd_qoff(q[b:b + 1], k[b:b + 1, :, :256 + prefix].contiguous(), v[b:b + 1, :, :256 + prefix].contiguous(), A.SCALE, prefix)
        assert torch.equal(o[b:b + 1], want[0]) and torch.equal(lse2[b:b + 1], want[1])


def test_a_decode_sized_chunk_agrees_with_the_paged_decode_kernel_under_the_rule(hip):
    case = (2, 8, 2, 8, 64, 5, (65, 257), (8, 8))  # Sq * G = 32
    paged, _, refs = gpu_inputs(case)
    o, lse2 = hip.attn_decode_paged(*paged[:5], A.SCALE, 1)
    check_rows("paged decode", case, "randn", o.cpu(), lse2.cpu(), refs)
    o, lse2 = hip.attn_prefill_paged(*paged, A.SCALE)
    check_rows("paged prefill", case, "randn", o.cpu(), lse2.cpu(), refs)


def test_result_does_not_depend_on_the_nans_of_the_pool_or_of_padded_rows(hip):
    q, kp, vp, table, kv_len, q_len = gpu_inputs(RAGGED)[0]
    want = hip.attn_prefill_paged(q, kp, vp, table, kv_len, q_len, A.SCALE)
    got = hip.attn_prefill_paged(torch.nan_to_num(q, nan=2.0), torch.nan_to_num(kp, nan=3.0), torch.nan_to_num(vp, nan=-7.0), table,
                                 kv_len, q_len, A.SCALE)
    assert all(torch.equal(a, b) for a, b in zip(want, got))


@pytest.mark.parametrize("case", [RAGGED, LONG_CHUNK], ids=["ragged", "Sq300"])
def test_chunk_append_fills_the_pages_and_nothing_else(hip, case):
    (q, kp, vp, table, kv_len, q_len), (k, v), _ = gpu_inputs(case)
    Sq = case[3]
    i = torch.arange(Sq, device="cuda").view(1, Sq)
    real = i < q_len.view(-1, 1)
    pos = ((kv_len - q_len).long().view(-1, 1) + i).clamp(0, k.size(2) - 1)  # [B, Sq]: where the rows live
    idx = pos.view(-1, 1, Sq, 1).expand(-1, k.size(1), -1, A.D)
    k_new, v_new = (torch.where(real.view(-1, 1, Sq, 1), x.gather(2, idx), float("nan")) for x in (k, v))
    page, row = table.long().gather(1, pos // case[4])[real], (pos % case[4])[real]
    kp0, vp0 = kp.clone(), vp.clone()
    kp0[page, :, row], vp0[page, :, row] = float("nan"), float("nan")
    kref, vref = kp0.clone(), vp0.clone()
    fused.kv_cache_append_prefill_ref(k_new, v_new, kref, vref, table, kv_len, q_len)
    fused.kv_cache_append_prefill(k_new, v_new, kp0, vp0, table, kv_len, q_len, check=True)
    for got, ref, full in ((kp0, kref, kp), (vp0, vref, vp)):
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16)) and torch.equal(got.view(torch.int16), full.view(torch.int16))
    want = fused.attention_prefill_paged(q, kp, vp, table, kv_len, q_len, A.SCALE, return_lse=True)
    got = fused.attention_prefill_paged(q, kp0, vp0, table, kv_len, q_len, A.SCALE, return_lse=True)
    assert all(torch.equal(a, b) for a, b in zip(want, got))


@pytest.mark.parametrize("kw,msg", [
    (dict(long=True), "q_len must be a contiguous int32"),
    (dict(Sq=65), r"Sq must be between 1 and max_pages \* page_size, got 65"),
])
def test_a_native_call_that_breaks_a_requirement_is_refused(hip, kw, msg):
    q = torch.ones(1, 2, kw.get("Sq", 4), A.D, dtype=torch.bfloat16, device="cuda")
    pool = torch.ones(2, 1, 64, A.D, dtype=torch.bfloat16, device="cuda")
    table = torch.zeros(1, 1, dtype=torch.int32, device="cuda")
    kv_len = torch.full((1,), 8, dtype=torch.int32, device="cuda")
    q_len = torch.full((1,), 4, dtype=torch.int64 if kw.get("long") else torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match=msg):
        hip.attn_prefill_paged(q, pool, pool, table, kv_len, q_len, A.SCALE)
    with pytest.raises(RuntimeError, match=msg):
        hip.kv_append_paged_chunk(q[:, :1], q[:, :1], pool, pool.clone(), table, kv_len, q_len)
