"""GPU: decode attention over a paged KV cache (``_fused.attn_decode_paged``, ``fused.attention_decode_paged``) and
the page append (``_fused.kv_append_paged``, ``fused.kv_cache_append``).  Inputs are ``decode_inputs`` cases scattered
into a pool by a seeded permutation: the pool has three pages more than the sequences need, every unused page and
every row at or past kv_len[b] holds NaN, and every table entry past ceil(kv_len[b] / page_size) names an all-NaN
page.  Each case is held to the float64 reference under the unchanged rule of tests/test_attention_ref.py (N = the
row's visible keys) and, bit for bit, to ``_fused.attn_decode`` on the slab at the same n."""
import functools

import pytest
import torch

import test_attention_ref as A
from gpu_topology_on_k8s_amd.models import attention_ref as R
from gpu_topology_on_k8s_amd.ops import fused
from test_attention_decode_ref import decode_inputs
from test_attention_paged_ref import paginate
from test_gpu_attention_decode import poison

pytestmark = pytest.mark.gpu
SHARED = (2, 8, 2, 1, 64, 4, (200, 250), 1)  # both sequences' first two table entries name the same two pool pages
CASES = [  # (B, H, Hkv, Sq, page_size, max_pages, kv_len, n)
    (1, 1, 1, 1, 64, 1, (1,), 1),              # one key, three idle waves: o is that v row
    (3, 8, 2, 1, 64, 5, (1, 64, 300), 3),      # lengths at, below and across page edges; the short sequences leave splits empty
    (2, 8, 1, 4, 128, 2, (4, 130), 2),         # two tiles a page; kv_len == Sq; the last tile is page 1's first and holds 2 keys
    (2, 4, 4, 8, 64, 5, (65, 257), 5),         # Sq = 8 across a page edge; more splits than tiles
    (1, 32, 8, 1, 256, 5, (1100,), 2),         # four tiles a page, nine tiles a split, both buffer parities
    SHARED,
    (1, 1, 1, 1, 192, 90, (17000,), 1),        # 266 tiles: each wave walks past the 64 page ids one vector load fetches; three tiles a page
]


@pytest.fixture(scope="module")
def hip():
    return fused.hip()


@functools.lru_cache(maxsize=None)
def paged_inputs(case, family):
    """-> (q, k_pool, v_pool, block_table, kv_len) and (k, v) slabs on the GPU, and the float64 reference."""
    B, H, Hkv, Sq, P, MP, lens, _ = case
    slab = (B, H, Hkv, Sq, MP * P, lens)
    q, k, v, kv_len, ref = decode_inputs(slab, family)
    need = [-(-n // P) for n in lens]
    perm = torch.randperm(sum(need) + 1, generator=A._gen("paged", case)).int()
    table = perm[-1].repeat(B, MP)  # the entries no sequence needs: a page paginate leaves (or fills with) NaN
    at = 0
    for b, m in enumerate(need):
        table[b, :m], at = perm[at:at + m], at + m
    if case == SHARED:  # a common prompt of two pages: the slab reference is built with the prefix copied
        k, v = k.clone(), v.clone()
        k[1, :, :2 * P], v[1, :, :2 * P], table[1, :2] = k[0, :, :2 * P], v[0, :, :2 * P], table[0, :2]
        o, lse2, cond = R.attn_decode_ref64(q, k, v, kv_len, A.SCALE)
        ref = {"o": (o, cond) + ref["o"][2:], "lse2": lse2}
    kp, vp = paginate(k, v, P, table)
    return tuple(x.cuda() for x in (q, kp, vp, table, kv_len)), (k.cuda(), v.cuda()), ref


@pytest.mark.parametrize("family", ["randn", "peaked"])
@pytest.mark.parametrize("case", CASES, ids=lambda s: "x".join(map(str, s[:6])) + f"-n{s[7]}")
def test_paged_decode_against_float64_and_the_contiguous_kernel(hip, case, family):
    """Worst err / tol on an MI355X: see profiles/attn_paged/SUMMARY.md."""
    paged, (k, v), ref = paged_inputs(case, family)
    n = case[7]
    poison(case[:4] + (None, None, n))
    o, lse2 = hip.attn_decode_paged(*paged, A.SCALE, n)
    A.check(f"paged decode {case} {family}", {"family": family}, {"o": o, "lse2": lse2}, refs=ref)
    want = hip.attn_decode(paged[0], k, v, paged[4], A.SCALE, n)
    assert torch.equal(o, want[0]) and torch.equal(lse2, want[1])
    if case == CASES[0]:
        assert torch.equal(o.view(-1), v[0, 0, 0])


@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=["Sq1", "Sq4"])
def test_result_does_not_depend_on_the_nans_of_the_pool(hip, case):
    q, kp, vp, table, kv_len = paged_inputs(case, "randn")[0]
    want = hip.attn_decode_paged(q, kp, vp, table, kv_len, A.SCALE, case[7])
    got = hip.attn_decode_paged(q, torch.nan_to_num(kp, nan=3.0), torch.nan_to_num(vp, nan=-7.0), table, kv_len, A.SCALE, case[7])
    assert all(torch.equal(a, b) for a, b in zip(want, got))


@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=["Sq1", "Sq8-across-a-page-edge"])
def test_append_fills_the_pages_and_nothing_else(hip, case):
    q, kp, vp, table, kv_len = paged_inputs(case, "randn")[0]
    B, _, Hkv, Sq, P = case[:5]
    pos = (kv_len.long().view(B, 1) - Sq + torch.arange(Sq, device="cuda"))  # [B, Sq]: where the new rows live
    page, row = table.long().gather(1, pos // P), pos % P
    k_new, v_new = (x[page, :, row].transpose(1, 2).contiguous() for x in (kp, vp))
    kp0, vp0 = kp.clone(), vp.clone()
    kp0[page, :, row], vp0[page, :, row] = float("nan"), float("nan")
    kref, vref = kp0.clone(), vp0.clone()
    fused.kv_cache_append_ref(k_new, v_new, kref, vref, table, kv_len)
    fused.kv_cache_append(k_new, v_new, kp0, vp0, table, kv_len, check=True)
    for got, ref, full in ((kp0, kref, kp), (vp0, vref, vp)):
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16)) and torch.equal(got.view(torch.int16), full.view(torch.int16))
    want = fused.attention_decode_paged(q, kp, vp, table, kv_len, A.SCALE, kv_splits=case[7], return_lse=True)
    got = fused.attention_decode_paged(q, kp0, vp0, table, kv_len, A.SCALE, kv_splits=case[7], return_lse=True)
    assert all(torch.equal(a, b) for a, b in zip(want, got))


@pytest.mark.parametrize("kv_splits", [1, 3, "auto"])
def test_fused_attention_decode_paged_dispatches_kv_splits(hip, kv_splits):
    paged = paged_inputs(CASES[4], "randn")[0]
    n = fused.decode_splits_for(1, 8, 5 * 256) if kv_splits == "auto" else kv_splits
    want = hip.attn_decode_paged(*paged, A.SCALE, n)
    o, lse2 = fused.attention_decode_paged(*paged, A.SCALE, kv_splits=kv_splits, return_lse=True, check=True)
    assert torch.equal(o, want[0]) and torch.equal(lse2, want[1])
    assert torch.equal(fused.attention_decode_paged(*paged, A.SCALE, kv_splits=kv_splits), o)


@pytest.mark.parametrize("kw,msg", [
    (dict(n=65), "kv_splits must be between 1 and 64, got 65"),
    (dict(P=96), "page_size must be a multiple of 64 from 64 to 1024, got 96"),
    (dict(long=True), "block_table must be a contiguous int32"),
])
def test_a_native_call_that_breaks_a_requirement_is_refused(hip, kw, msg):
    q = torch.ones(1, 2, 1, A.D, dtype=torch.bfloat16, device="cuda")
    pool = torch.ones(2, 1, kw.get("P", 64), A.D, dtype=torch.bfloat16, device="cuda")
    table = torch.zeros(1, 1, dtype=torch.int64 if kw.get("long") else torch.int32, device="cuda")
    kv_len = torch.full((1,), 8, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match=msg):
        hip.attn_decode_paged(q, pool, pool, table, kv_len, A.SCALE, kw.get("n", 1))
    if "n" not in kw:
        with pytest.raises(RuntimeError, match=msg):
            hip.kv_append_paged(q[:, :1], q[:, :1], pool, pool.clone(), table, kv_len)
