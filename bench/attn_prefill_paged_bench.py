#!/usr/bin/env python3
"""Prefill over the paged KV cache next to what a user had before it: a chunk of 2048 queries (H 32, Hkv 8) at
prefix 0, 2048 and 8192 (aligned, so all three contestants can run), B 1 and 4, page sizes 64 and 256.

    paged    fused.attention_prefill_paged straight over the block table (pages in a seeded random order);
    slab     fused.attention(q, k, v, q_offset=prefix) on a slab gathered beforehand: the existing kernel's own
             speed, the bar;
    gather   gathering the slab from the pages, then ``slab``: what a user had to do.

One ragged batch (B 4, chunk lengths 2048, 1500, 333, 0 at prefixes 0, 1000, 8192, 77, page size 64) runs on the new
kernel alone.  The chunk append is timed at 4096 rows a sequence next to ``copy_`` of the same bytes.  One process,
warm-up first, the contestants interleaved round by round with the order alternating; every contestant is measured
as two series (even and odd rounds) and the spread between the two medians is reported beside the median of all.
Prints one JSON line and a markdown table (profiles/attn_prefill_paged/SUMMARY.md keeps a run's output).

With ``--kv-fp8`` every shape also gets the pools quantised by ``fused.kv_quantize_ref`` and two more contestants in
the same interleaved rounds:

    fp8      fused.attention_prefill_paged_fp8 straight over the four fp8 pools;
    deq      ``fused.kv_dequantize_ref`` of the four pools in torch, then ``paged`` on the result: what a user of the fp8
             cache had to do, at twice the cache's memory.

and ``fused.kv_cache_append_prefill_fp8`` is timed next to the bf16 chunk append at the same 4 x 4096 rows
(profiles/attn_prefill_paged_fp8/SUMMARY.md keeps a run's output).

    python bench/attn_prefill_paged_bench.py [--iters 10] [--rounds 6] [--kv-fp8]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_topology_on_k8s_amd.ops import fused  # noqa: E402

H, HKV, D, CHUNK = 32, 8, 128, 2048


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def cache(B, lens, P, g):
    """Pools of random rows with the sequences' pages in a seeded random order -> (k_pool, v_pool, table, kv_len)."""
    MP = -(-max(lens) // P)
    table = torch.randperm(B * MP, generator=g, device="cuda").int().view(B, MP)
    kp, vp = (torch.randn(B * MP, HKV, P, D, generator=g, device="cuda").to(torch.bfloat16) for _ in range(2))
    return kp, vp, table, torch.tensor(lens, dtype=torch.int32, device="cuda")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--kv-fp8", action="store_true", help="also time the fp8 cache: the fp8 kernel, and dequantise + paged")
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    sc = D ** -0.5
    fns = {}
    for B in (1, 4):
        for prefix in (0, 2048, 8192):
            for P in (64, 256):
                kp, vp, table, kv_len = cache(B, [prefix + CHUNK] * B, P, g)
                q = torch.randn(B, H, CHUNK, D, generator=g, device="cuda").to(torch.bfloat16)
                k, v = fused._gather_pages(kp, table).contiguous(), fused._gather_pages(vp, table).contiguous()
                o = fused.attention_prefill_paged(q, kp, vp, table, kv_len, scale=sc)
                assert torch.equal(o, fused.attention(q, k, v, sc, q_offset=prefix or None)), (B, prefix, P)
                key = f"B{B} prefix{prefix} P{P}"
                fns[f"paged {key}"] = lambda q=q, kp=kp, vp=vp, table=table, kv_len=kv_len: fused.attention_prefill_paged(
                    q, kp, vp, table, kv_len, scale=sc)
                fns[f"slab {key}"] = lambda q=q, k=k, v=v, prefix=prefix: fused.attention(q, k, v, sc, q_offset=prefix or None)
                fns[f"gather {key}"] = lambda q=q, kp=kp, vp=vp, table=table, prefix=prefix: fused.attention(
                    q, fused._gather_pages(kp, table).contiguous(), fused._gather_pages(vp, table).contiguous(), sc, q_offset=prefix or None)
                if a.kv_fp8:
                    (kc, ke), (vc, ve) = fused.kv_quantize_ref(kp), fused.kv_quantize_ref(vp)
                    o8 = fused.attention_prefill_paged_fp8(q, kc, vc, ke, ve, table, kv_len, scale=sc)
                    want = fused.attention_prefill_paged(q, fused.kv_dequantize_ref(kc, ke), fused.kv_dequantize_ref(vc, ve), table, kv_len, scale=sc)
                    assert torch.equal(o8, want), (B, prefix, P)
                    fns[f"fp8 {key}"] = lambda q=q, kc=kc, vc=vc, ke=ke, ve=ve, table=table, kv_len=kv_len: fused.attention_prefill_paged_fp8(
                        q, kc, vc, ke, ve, table, kv_len, scale=sc)
                    fns[f"deq {key}"] = lambda q=q, kc=kc, vc=vc, ke=ke, ve=ve, table=table, kv_len=kv_len: fused.attention_prefill_paged(
                        q, fused.kv_dequantize_ref(kc, ke), fused.kv_dequantize_ref(vc, ve), table, kv_len, scale=sc)
    qls, pre = [2048, 1500, 333, 0], [0, 1000, 8192, 77]
    kp, vp, table, kv_len = cache(4, [p + n for p, n in zip(pre, qls)], 64, g)
    q_len = torch.tensor(qls, dtype=torch.int32, device="cuda")
    q = torch.randn(4, H, CHUNK, D, generator=g, device="cuda").to(torch.bfloat16)
    fns["paged ragged"] = lambda: fused.attention_prefill_paged(q, kp, vp, table, kv_len, q_len, sc)
    ak, av, atab, alen = cache(4, [4096] * 4, 64, g)
    new = torch.randn(4, HKV, 4096, D, generator=g, device="cuda").to(torch.bfloat16)
    dst = torch.empty_like(new)
    fns["append 4x4096"] = lambda: fused.kv_cache_append_prefill(new, new, ak, av, atab, alen)
    fns["copy 4x4096"] = lambda: (dst.copy_(new), dst.copy_(new))
    if a.kv_fp8:
        codes = [torch.zeros(ak.shape, dtype=torch.uint8, device="cuda") for _ in range(2)]
        exps = [torch.zeros(ak.shape[:3], dtype=torch.uint8, device="cuda") for _ in range(2)]
        fns["append8 4x4096"] = lambda: fused.kv_cache_append_prefill_fp8(new, new, *codes, *exps, atab, alen)
    names = list(fns)
    for fn in fns.values():
        timed(fn, 2)
    times = {n: [] for n in names}
    for r in range(a.rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            times[n].append(timed(fns[n], a.iters))
    med = {n: statistics.median(t) for n, t in times.items()}
    spread = {n: abs(statistics.median(t[0::2]) - statistics.median(t[1::2])) / med[n] for n, t in times.items()}
    print(json.dumps({"heads": [H, HKV], "chunk": CHUNK, "iters": a.iters, "rounds": a.rounds, "median_us": med, "spread": spread}))
    print("| B | prefix | page | paged us | slab us | gather + slab us | paged / slab | paged / (gather + slab) | spread of slab |\n"
          "|---|---|---|---|---|---|---|---|---|")
    for B in (1, 4):
        for prefix in (0, 2048, 8192):
            for P in (64, 256):
                key = f"B{B} prefix{prefix} P{P}"
                pa, sl, ga = med[f"paged {key}"], med[f"slab {key}"], med[f"gather {key}"]
                print(f"| {B} | {prefix} | {P} | {pa:.0f} | {sl:.0f} | {ga:.0f} | {pa / sl:.3f} | {pa / ga:.3f} | {100 * spread['slab ' + key]:.1f} % |")
    print(f"ragged batch (q_len {qls} at prefixes {pre}, page 64): {med['paged ragged']:.0f} us, spread {100 * spread['paged ragged']:.1f} %")
    nbytes = 2 * 2 * new.numel() * 2  # K and V, read and written
    print(f"append of 4 x 4096 rows: {med['append 4x4096']:.0f} us = {nbytes / med['append 4x4096'] / 1e3:.0f} GB/s; "
          f"copy_ of the same bytes {med['copy 4x4096']:.0f} us = {nbytes / med['copy 4x4096'] / 1e3:.0f} GB/s")
    if a.kv_fp8:
        print("| B | prefix | page | fp8 us | deq + paged us | paged (bf16 pools) us | fp8 / (deq + paged) | fp8 / paged | spread fp8 | spread deq | beats deq by more than the spreads |\n"
              "|---|---|---|---|---|---|---|---|---|---|---|")
        for B in (1, 4):
            for prefix in (0, 2048, 8192):
                for P in (64, 256):
                    key = f"B{B} prefix{prefix} P{P}"
                    f8, dq, pa = med[f"fp8 {key}"], med[f"deq {key}"], med[f"paged {key}"]
                    s8, sd = spread["fp8 " + key], spread["deq " + key]
                    print(f"| {B} | {prefix} | {P} | {f8:.0f} | {dq:.0f} | {pa:.0f} | {f8 / dq:.3f} | {f8 / pa:.3f} | {100 * s8:.1f} % | "
                          f"{100 * sd:.1f} % | {f8 / dq < 1 - max(s8, sd)} |")
        print(f"fp8 append of 4 x 4096 rows: {med['append8 4x4096']:.0f} us, spread {100 * spread['append8 4x4096']:.1f} %; "
              f"the bf16 append {med['append 4x4096']:.0f} us")
    return 0


if __name__ == "__main__":
    sys.exit(main())
