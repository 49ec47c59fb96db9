"""CPU: decode attention over a paged KV cache.  ``attention_decode_paged_ref`` and ``kv_cache_append_ref`` against
the slab reference on ``decode_inputs`` cases scattered into a pool, the refusals of the two public functions, and
the scratch-free build of the kernel.  ``paginate`` is also the pool maker of tests/test_gpu_attention_paged.py."""
import os
import sys

import pytest
import torch

import test_attention_ref as A
from gpu_topology_on_k8s_amd.ops import fused
from test_attention_decode_ref import decode_inputs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 64
CPU_CASE = (2, 4, 2, 3, 3 * P, (3, 130))  # Smax = 3 pages; sequence 1's three new rows 127, 128, 129 cross a page edge
TABLE = torch.tensor([[5, 1, 4], [2, 0, 3]], dtype=torch.int32)


def paginate(k, v, page_size, table):
    """Slabs [B, Hkv, max_pages * page_size, D] -> pools [table.max() + 3, Hkv, page_size, D]: page p of sequence b at
    pool page table[b, p], every other page NaN."""
    B, Hkv, _, D = k.shape
    pools = []
    for x in (k, v):
        pool = torch.full((int(table.max()) + 3, Hkv, page_size, D), float("nan"), dtype=x.dtype, device=x.device)
        pool[table.long().flatten()] = x.view(B, Hkv, -1, page_size, D).transpose(1, 2).flatten(0, 1)
        pools.append(pool)
    return pools


def paged_inputs():
    q, k, v, kv_len, _ = decode_inputs(CPU_CASE, "randn")
    return (q, *paginate(k, v, P, TABLE), TABLE, kv_len), (q, k, v, kv_len)


def test_paged_reference_and_cpu_call_equal_the_slab_reference():
    paged, slab = paged_inputs()
    want = fused.attention_decode_ref(*slab, A.SCALE)
    for got in (fused.attention_decode_paged_ref(*paged, A.SCALE),
                fused.attention_decode_paged(*paged, A.SCALE, kv_splits=3, return_lse=True, check=True)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_append_then_paged_reference_equals_the_slab_reference():
    paged, slab = paged_inputs()
    q, kp, vp, table, kv_len = paged
    k_new, v_new = (torch.stack([x[b, :, n - 3:n] for b, n in enumerate(CPU_CASE[5])]) for x in slab[1:3])
    kp0, vp0 = paginate(*(x.clone() for x in slab[1:3]), P, table)
    for b, n in enumerate(CPU_CASE[5]):  # the pools before the step: NaN from kv_len - Sq on
        for pos in range(n - 3, n):
            kp0[table[b, pos // P], :, pos % P], vp0[table[b, pos // P], :, pos % P] = float("nan"), float("nan")
    assert not torch.equal(kp0.view(torch.int16), kp.view(torch.int16))
    fused.kv_cache_append(k_new, v_new, kp0, vp0, table, kv_len, check=True)
    assert torch.equal(kp0.view(torch.int16), kp.view(torch.int16)) and torch.equal(vp0.view(torch.int16), vp.view(torch.int16))
    got, want = fused.attention_decode_paged_ref(q, kp0, vp0, table, kv_len, A.SCALE), fused.attention_decode_ref(*slab, A.SCALE)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_append_skips_a_bad_length_and_a_bad_page_id_without_touching_another_page():
    (q, kp, vp, table, kv_len), _ = paged_inputs()
    before = kp.clone()
    new = torch.ones(2, 2, 3, A.D, dtype=torch.bfloat16)
    bad = table.clone()
    bad[1, 2] = kp.size(0)  # row 129 of sequence 1 has no page; sequence 0's length is out of range
    fused.kv_cache_append_ref(new, new, kp, vp, bad, torch.tensor([2, 130], dtype=torch.int32))
    changed = (kp.view(torch.int16) != before.view(torch.int16)).any(-1).nonzero().tolist()
    assert changed == [[0, 0, 63], [0, 1, 63]] and bool((kp[0, :, 63] == 1).all())  # position 127 alone


@pytest.mark.parametrize("change,msg", [
    (dict(q=lambda t: t.float()), "q must be a bf16"),
    (dict(kp=lambda t: t.float()), "k_pool must be a bf16"),
    (dict(kp=lambda t: t.repeat(1, 1, 2, 1)[:, :, :96].contiguous(), vp=lambda t: t.repeat(1, 1, 2, 1)[:, :, :96].contiguous()),
     "page_size must be a multiple of 64"),
    (dict(vp=lambda t: t[:-1]), "one shape"),
    (dict(kp=lambda t: t.transpose(0, 1).contiguous().transpose(0, 1)), "pools must be contiguous"),
    (dict(table=lambda t: t.long()), "block_table must be an int32"),
    (dict(table=lambda t: t[:1]), "block_table must be an int32"),
    (dict(q=lambda t: t.repeat(1, 1, 6, 1)), r"Sq \* \(H / Hkv\) must be between 1 and 32, got 36"),
    (dict(q=lambda t: t.clone().requires_grad_(True)), "forward only"),
    (dict(kv_splits=0), "kv_splits must be 'auto' or an int from 1 to 64"),
    (dict(kv_splits=65), "kv_splits must be 'auto' or an int from 1 to 64"),
    (dict(kv_len=lambda t: t + 63, check=True), r"kv_len must lie in \[3, 192\]"),
    (dict(kv_len=lambda t: t - 1, check=True), r"kv_len must lie in \[3, 192\]"),
    (dict(table=lambda t: t + 3, check=True), r"a needed block_table entry lies outside \[0, 8\)"),
    (dict(table=lambda t: t - 1, check=True), r"a needed block_table entry lies outside \[0, 8\)"),
])
def test_a_call_that_breaks_a_requirement_is_refused(change, msg):
    (q, kp, vp, table, kv_len), _ = paged_inputs()
    args = {"q": q, "kp": kp, "vp": vp, "table": table, "kv_len": kv_len}
    kw = {key: val for key, val in change.items() if key not in args}
    args.update({key: fn(args[key]) for key, fn in change.items() if key in args})
    with pytest.raises(ValueError, match=msg):
        fused.attention_decode_paged(*args.values(), A.SCALE, **kw)
    if "q" not in change and "kv_splits" not in change:  # the append takes the same pools, table and lengths
        new = torch.ones(2, 2, 3, A.D, dtype=torch.bfloat16)
        with pytest.raises(ValueError, match=msg.replace("q must", "k_new must")):
            fused.kv_cache_append(new, new, *list(args.values())[1:], check=kw.get("check", False))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_paged_kernel_is_built_without_scratch(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa

    st = isa.kernel_stats(os.path.join(REPO, "csrc", "ops", "attention_decode_paged.hip"), out=str(tmp_path / "paged.s"))
    (k,) = [v for name, v in st.items() if "attn_decode_paged_kernel" in name]
    assert k["ScratchSize"] == 0 and k["scratch"] == 0 and k["mfma"] == 64 and k["LDSByteSize"] == 128 * 1024, k
