"""GPU: decode attention over a ragged KV cache (``_fused.attn_decode``, ``fused.attention_decode``) against the
float64 reference ``attn_decode_ref64`` under the unchanged rule of tests/test_attention_ref.py, N = the row's
visible keys.  Every cache row at or past kv_len[b] holds NaN, and before each checked call a block of NaNs of
the workspace's size goes back to the caching allocator."""
import pytest
import torch

import test_attention_ref as A
from gpu_topology_on_k8s_amd.ops import fused
from test_attention_decode_ref import decode_inputs

pytestmark = pytest.mark.gpu
CASES = [  # (B, H, Hkv, Sq, Smax, kv_len, n)
    (1, 1, 1, 1, 1, (1,), 1),             # one key: o is v[0]; one wave has work, three are empty
    (1, 2, 1, 1, 70, (70,), 2),           # two rows through the merge's rounded-up grid; split 1 is a 6-key tail tile alone
    (3, 8, 2, 1, 300, (1, 64, 300), 1),   # lengths at, below and across tile edges in one launch
    (3, 8, 2, 1, 300, (1, 64, 300), 3),   # the short sequences leave splits empty, the long one fills all three
    (2, 8, 1, 4, 200, (4, 130), 2),       # all 32 columns real; kv_len == Sq; 130 = 2 * 64 + 2: rows 0, 1 see no key of the last tile
    (2, 4, 4, 8, 257, (65, 257), 5),      # G = 1, Sq = 8 across a tile edge: two masked tiles; more splits than tiles
    (1, 32, 8, 1, 1100, (1100,), 2),      # nine tiles a split: two or three per wave, both buffer parities, unequal counts
]
LAST = CASES[-1]


@pytest.fixture(scope="module")
def hip():
    return fused.hip()


def poison(case):
    """The allocator's next blocks of the two workspace sizes hold NaNs (each tensor is freed at once)."""
    B, H, _, Sq, _, _, n = case
    for m in (A.D, 1):
        torch.full((m * n * B * H * Sq,), float("nan"), device="cuda")


def on_gpu(case, family):
    q, k, v, kv_len, ref = decode_inputs(case[:6], family)
    return q.cuda(), k.cuda(), v.cuda(), kv_len.cuda(), ref


@pytest.mark.parametrize("family", ["randn", "peaked"])
@pytest.mark.parametrize("case", CASES, ids=lambda s: "x".join(map(str, s[:5])) + f"-n{s[6]}")
def test_decode_against_float64(hip, case, family):
    """Worst err / tol on an MI355X: see profiles/attn_decode/SUMMARY.md."""
    q, k, v, kv_len, ref = on_gpu(case, family)
    poison(case)
    o, lse2 = hip.attn_decode(q, k, v, kv_len, A.SCALE, case[6])
    A.check(f"decode {case} {family}", {"family": family}, {"o": o, "lse2": lse2}, refs=ref)
    if case == CASES[0]:
        assert torch.equal(o.view(-1), v[0, 0, 0])


def test_decode_is_deterministic_and_reads_no_stale_partial(hip):
    q, k, v, kv_len, _ = on_gpu(LAST, "randn")
    first = hip.attn_decode(q, k, v, kv_len, A.SCALE, 2)
    poison(LAST)
    again = hip.attn_decode(q, k, v, kv_len, A.SCALE, 2)
    assert all(torch.equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("case", [CASES[3], CASES[4]], ids=["Sq1", "Sq4"])
def test_result_does_not_depend_on_cache_rows_past_kv_len(hip, case):
    q, k, v, kv_len, _ = on_gpu(case, "randn")
    want = hip.attn_decode(q, k, v, kv_len, A.SCALE, case[6])
    k2, v2 = torch.nan_to_num(k, nan=3.0), torch.nan_to_num(v, nan=-7.0)
    got = hip.attn_decode(q, k2, v2, kv_len, A.SCALE, case[6])
    assert all(torch.equal(a, b) for a, b in zip(want, got))


@pytest.mark.parametrize("kv_splits", [1, 3, "auto"])
def test_fused_attention_decode_dispatches_kv_splits(hip, kv_splits):
    q, k, v, kv_len, _ = on_gpu(LAST, "randn")
    n = fused.decode_splits_for(1, 8, 1100) if kv_splits == "auto" else kv_splits
    want = hip.attn_decode(q, k, v, kv_len, A.SCALE, n)
    o, lse2 = fused.attention_decode(q, k, v, kv_len, A.SCALE, kv_splits=kv_splits, return_lse=True, check=True)
    assert torch.equal(o, want[0]) and torch.equal(lse2, want[1])
    assert torch.equal(fused.attention_decode(q, k, v, kv_len, A.SCALE, kv_splits=kv_splits), o)


@pytest.mark.parametrize("kw,msg", [
    (dict(n=0), "kv_splits must be between 1 and 64, got 0"),
    (dict(n=65), "kv_splits must be between 1 and 64, got 65"),
    (dict(H=33), r"Sq \* \(H / Hkv\) must be between 1 and 32, got 33"),
    (dict(Dh=64), "head dim must be 128, got 64"),
    (dict(long=True), "kv_len must be a contiguous int32"),
])
def test_a_native_call_that_breaks_a_requirement_is_refused(hip, kw, msg):
    q = torch.ones(1, kw.get("H", 2), 1, kw.get("Dh", A.D), dtype=torch.bfloat16, device="cuda")
    k = torch.ones(1, 1, 8, kw.get("Dh", A.D), dtype=torch.bfloat16, device="cuda")
    kv_len = torch.full((1,), 8, dtype=torch.int64 if kw.get("long") else torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match=msg):
        hip.attn_decode(q, k, k, kv_len, A.SCALE, kw.get("n", 1))
