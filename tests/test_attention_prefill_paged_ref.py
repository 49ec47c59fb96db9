"""CPU: prefill attention over a paged KV cache.  ``attention_prefill_paged_ref`` and ``kv_cache_append_prefill_ref``
against the float64 and the slab references, the refusals of the two public functions, and the build of the kernel.
``prefill_inputs`` and ``check_rows`` are also the input maker and the rule of tests/test_gpu_attention_prefill_paged.py."""
import functools
import os
import sys

import pytest
import torch

import test_attention_ref as A
from gpu_topology_on_k8s_amd.models import attention_ref as R
from gpu_topology_on_k8s_amd.ops import fused
from test_attention_decode_ref import decode_inputs
from test_attention_paged_ref import paged_inputs, paginate

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SHARED = (2, 4, 2, 96, 64, 4, (200, 250), (70, 96))  # both sequences' first two table entries name the same two pool pages
CPU_CASE = (3, 4, 2, 40, 64, 3, (100, 130, 9), (40, 17, 0))  # a chunk across a page edge, a ragged one, an idle slot


@functools.lru_cache(maxsize=None)
def prefill_inputs(case, family):
    """(B, H, Hkv, Sq, page_size, max_pages, kv_len, q_len) -> CPU (q, k_pool, v_pool, block_table, kv_len, q_len), the
    slabs (k, v), and per sequence the float64 reference of its q_len[b] real rows in the form ``A.check`` takes.
    ``decode_inputs`` values scattered into a pool by a seeded page permutation; NaN in every unused page, every row at
    or past kv_len[b] and every padded q row; table entries no sequence needs name an all-NaN page."""
    B, H, Hkv, Sq, P, MP, lens, qls = case
    q, k, v, _, _ = decode_inputs((B, H, Hkv, Sq, MP * P, tuple(max(n, Sq) for n in lens)), family)
    q, k, v = q.clone(), k.clone(), v.clone()
    kv_len, q_len = torch.tensor(lens, dtype=torch.int32), torch.tensor(qls, dtype=torch.int32)
    need = [-(-n // P) for n in lens]
    perm = torch.randperm(sum(need) + 1, generator=A._gen("prefill", case)).int()
    table = perm[-1].repeat(B, MP)
    at = 0
    for b, m in enumerate(need):
        table[b, :m], at = perm[at:at + m], at + m
        k[b, :, lens[b]:], v[b, :, lens[b]:] = NAN, NAN
    if case == SHARED:
        k[1, :, :2 * P], v[1, :, :2 * P], table[1, :2] = k[0, :, :2 * P], v[0, :, :2 * P], table[0, :2]
    refs = []
    for b, (n, m) in enumerate(zip(lens, qls)):
        if m:
            o, lse2, cond = R.attn_decode_ref64(q[b:b + 1, :, :m], k[b:b + 1], v[b:b + 1], kv_len[b:b + 1], A.SCALE)
            assert float(lse2.abs().max()) <= 64.0
            refs.append({"o": (o, cond, None, (n - m + 1 + torch.arange(m)).double().view(1, m, 1, 1)), "lse2": lse2})
        else:
            refs.append(None)
        q[b, :, m:] = NAN
    return (q, *paginate(k, v, P, table), table, kv_len, q_len), (k, v), refs


def check_rows(name, case, family, o, lse2, refs):
    """The unchanged rule on every sequence's real rows (N = the row's visible keys); padded rows exactly 0 and -inf."""
    for b, m in enumerate(case[7]):
        if m:
            A.check(f"{name} {case} {family} seq {b}", {"family": family}, {"o": o[b:b + 1, :m], "lse2": lse2[b:b + 1, :, :m]}, refs=refs[b])
        assert bool((o[b, m:] == 0).all()) and bool((lse2[b, :, m:] == float("-inf")).all()), (name, b)


@pytest.mark.parametrize("family", ["randn", "peaked"])
def test_cpu_call_is_the_fp32_reference_and_matches_float64(family):
    paged, _, refs = prefill_inputs(CPU_CASE, family)
    o, lse2 = fused.attention_prefill_paged(*paged, A.SCALE, return_lse=True, check=True)
    check_rows("cpu prefill", CPU_CASE, family, o, lse2, refs)
    want = fused.attention_prefill_paged_ref(*paged, A.SCALE)
    assert o.dtype == torch.bfloat16 and torch.equal(o, want[0]) and torch.equal(lse2, want[1])
    assert torch.equal(fused.attention_prefill_paged(*paged, A.SCALE), o)


def test_full_chunks_of_a_decode_step_equal_the_paged_decode_reference():
    (q, kp, vp, table, kv_len), _ = paged_inputs()  # Sq = 3, every row real
    want = fused.attention_decode_paged_ref(q, kp, vp, table, kv_len, A.SCALE)
    for q_len in (None, torch.full((2,), 3, dtype=torch.int32)):
        got = fused.attention_prefill_paged(q, kp, vp, table, kv_len, q_len, A.SCALE, return_lse=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_append_in_two_ragged_chunks_then_prefill_reference_equals_the_slab_reference():
    (q, kp, vp, table, kv_len, q_len), (k, v), _ = prefill_inputs(CPU_CASE, "randn")
    kp0, vp0 = torch.full_like(kp, NAN), torch.full_like(vp, NAN)
    first = kv_len - q_len  # (60, 113, 9): pure prefill of three different lengths, then the case's own chunk
    for lens, qls in ((first, first), (kv_len, q_len)):
        Sq = int(qls.max())
        new = [torch.stack([torch.cat([x[b, :, n - m:n], x.new_full((x.size(1), Sq - m, A.D), NAN)], 1)
                            for b, (n, m) in enumerate(zip(lens.tolist(), qls.tolist()))]) for x in (k, v)]
        fused.kv_cache_append_prefill(*new, kp0, vp0, table, lens, qls, check=True)
    assert torch.equal(kp0.view(torch.int16), kp.view(torch.int16)) and torch.equal(vp0.view(torch.int16), vp.view(torch.int16))
    got = fused.attention_prefill_paged_ref(q, kp0, vp0, table, kv_len, q_len, A.SCALE)
    for b, m in enumerate(CPU_CASE[7]):
        if m:
            want = fused.attention_decode_ref(q[b:b + 1, :, :m], k[b:b + 1], v[b:b + 1], kv_len[b:b + 1], A.SCALE)
            assert torch.equal(got[0][b, :m], want[0][0]) and torch.equal(got[1][b, :, :m], want[1][0])


def test_append_skips_touch_no_other_byte():
    (_, kp, vp, table, _, _), _, _ = prefill_inputs(CPU_CASE, "randn")
    kp, vp, before = kp.clone(), vp.clone(), kp.clone()
    new = torch.ones(3, 2, 5, A.D, dtype=torch.bfloat16)
    bad = table.clone()
    bad[1, 2] = kp.size(0)  # rows 128, 129 of sequence 1 have no page; sequence 0's length is below its q_len; 2 is idle
    fused.kv_cache_append_prefill_ref(new, new, kp, vp, bad, torch.tensor([2, 130, 9], dtype=torch.int32), torch.tensor([3, 4, 0], dtype=torch.int32))
    changed = (kp.view(torch.int16) != before.view(torch.int16)).any(-1).nonzero().tolist()
    page = int(table[1, 1])
    assert changed == [[page, h, r] for h in (0, 1) for r in (62, 63)] and bool((vp[page, :, 62:] == 1).all())  # positions 126, 127


@pytest.mark.parametrize("change,msg", [
    (dict(q=lambda t: t.float()), "q must be a bf16"),
    (dict(kp=lambda t: t.repeat(1, 1, 2, 1)[:, :, :96].contiguous(), vp=lambda t: t.repeat(1, 1, 2, 1)[:, :, :96].contiguous()),
     "page_size must be a multiple of 64"),
    (dict(table=lambda t: t.long()), "block_table must be an int32"),
    (dict(q=lambda t: t[:, :3]), "must be a multiple of kv heads"),
    (dict(q=lambda t: t.repeat(1, 1, 5, 1)), "Sq must be between 1 and max_pages \\* page_size = 192, got 200"),
    (dict(q=lambda t: t.clone().requires_grad_(True)), "forward only"),
    (dict(q_len=lambda t: t.long()), "q_len must be an int32"),
    (dict(q_len=lambda t: t[:2]), "q_len must be an int32"),
    (dict(q_len=lambda t: t + 1, check=True), r"q_len must lie in \[0, 40\]"),
    (dict(kv_len=lambda t: t - 84, check=True), r"kv_len must lie in \[q_len, 192\]"),
    (dict(kv_len=lambda t: t + 63, check=True), r"kv_len must lie in \[q_len, 192\]"),
    (dict(table=lambda t: t + 10, check=True), r"a needed block_table entry lies outside \[0, 9\)"),
])
def test_a_call_that_breaks_a_requirement_is_refused(change, msg):
    args = dict(zip(("q", "kp", "vp", "table", "kv_len", "q_len"), prefill_inputs(CPU_CASE, "randn")[0]))
    kw = {key: val for key, val in change.items() if key not in args}
    args.update({key: fn(args[key]) for key, fn in change.items() if key in args})
    with pytest.raises(ValueError, match=msg):
        fused.attention_prefill_paged(*args.values(), A.SCALE, **kw)
    if "q" not in change:  # the append takes the same pools, table and lengths
        new = torch.ones(3, 2, 40, A.D, dtype=torch.bfloat16)
        with pytest.raises(ValueError, match=msg):
            fused.kv_cache_append_prefill(new, new, *list(args.values())[1:], **kw)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_prefill_kernel_is_built_without_scratch(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa

    st = isa.kernel_stats(os.path.join(REPO, "csrc", "ops", "attention_prefill_paged.hip"), out=str(tmp_path / "prefill.s"))
    (k,) = [v for name, v in st.items() if "attn_prefill_paged_kernel" in name]
    assert k["ScratchSize"] == 0 and k["scratch"] == 0 and k["LDSByteSize"] == 64 * 1024, k
