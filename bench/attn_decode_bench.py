#!/usr/bin/env python3
"""Decode attention over a ragged KV cache (``fused.attention_decode``) against torch, one new token per sequence
(Sq 1) at 32 q-heads over 8 KV heads: B in {1, 8, 64} with every sequence at kv_len in {2048, 8192, 32768}, and B 8
once more with mixed lengths in a cache of 32768 rows.

Callers per shape, all interleaved round by round in one process after a warm-up, order alternating: the HIP
kernel at every power of two n from 1 to 64 that leaves a split a tile (which covers n = 1, ``"auto"`` and its
neighbours), the ``"auto"`` n a second time (the two series give the run-to-run spread), and torch's
``scaled_dot_product_attention`` on the cache sliced to kv_len and repeated to 32 heads (repeated outside the
timed window; the mixed shape takes a boolean key mask instead of the slice).  Each caller rotates over enough
copies of the cache to exceed the 256 MiB Infinity Cache, so a small shape is not timed out of cache.

Printed: one JSON line; per shape the median us per call and the K/V bytes read per second, 2 * B * Hkv *
kv_len * 256 bytes over the time; and for each candidate MIN_TILES_PER_DECODE_SPLIT the shapes where the n that
``decode_splits_for`` would pick is slower than n = 1 by more than the spread.

With ``--page-size P`` (repeatable) every shape also times ``fused.attention_decode_paged`` over the same K/V laid
out in pages of P rows, in the same rounds as the contiguous callers and at the same ``"auto"`` n: under a block
table that is a seeded random permutation of the pool (the worst locality; two series, which give that caller's
spread), under the identity table, and the only route without the kernel, a torch gather of the pages into a slab
followed by the contiguous call.  Before timing, the paged result is compared bit for bit with the contiguous one.
A second table reports paged / contiguous per shape and page size next to the spreads.

With ``--kv-fp8`` next to ``--page-size`` every shape also times ``fused.attention_decode_paged_fp8`` on the quantised
copy (``kv_quantize_ref``) of the permuted pools, two series in the same rounds, and one-token appends into the bf16
and the fp8 pools.  Before timing, the fp8 result is compared by ``torch.equal`` with the bf16 paged call on the
dequantised pools.  A third table reports fp8 / bf16 paged per shape with both callers' spreads.  ``--shape I``
(repeatable) keeps only ``SHAPES[I]``.

    python bench/attn_decode_bench.py [--iters 10] [--rounds 5] [--page-size 64 --page-size 256] [--kv-fp8] [--shape 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_topology_on_k8s_amd.ops import fused  # noqa: E402

H, HKV, D = 32, 8, 128
MIXED = (700, 2048, 5000, 8192, 12000, 20000, 32768, 1)
SHAPES = [(B, (L,) * B, L) for B in (1, 8, 64) for L in (2048, 8192, 32768)] + [(8, MIXED, 32768)]  # (B, kv_len, Smax)
SPLITS = (1, 2, 4, 8, 16, 32, 64)
CANDIDATES = (1, 2, 4, 8, 16, 32, 64)  # minimum tiles per split
ROTATE_BYTES = 768 << 20


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def auto_for(B, Smax, min_tiles):
    """decode_splits_for under a candidate minimum."""
    saved, fused.MIN_TILES_PER_DECODE_SPLIT = fused.MIN_TILES_PER_DECODE_SPLIT, min_tiles
    try:
        return fused.decode_splits_for(B, HKV, Smax)
    finally:
        fused.MIN_TILES_PER_DECODE_SPLIT = saved


def quantize_pool(pool, pages=128):
    """kv_quantize_ref over a pool, ``pages`` pages at a time (the rule works in float64) -> (codes, exp)."""
    parts = [fused.kv_quantize_ref(pool[i:i + pages]) for i in range(0, pool.size(0), pages)]
    return torch.cat([c for c, _ in parts]), torch.cat([e for _, e in parts])


def fp8_callers(fns, q, kv_len, pools, table, auto, P):
    """Adds the fp8 callers of page size P (two series) over the quantised copies of ``pools`` under ``table``, and the
    append's; -> whether the fp8 result equals the bf16 paged call on the dequantised pools bit for bit."""
    copies, q8 = len(pools), []
    for kp, vp in pools:
        (kc, ke), (vc, ve) = quantize_pool(kp), quantize_pool(vp)
        q8.append((kc, vc, ke, ve))
    call = lambda i: fused.attention_decode_paged_fp8(q, *q8[i % copies], table, kv_len, kv_splits=auto)  # noqa: E731
    fns[f"fp8_{P}"] = call
    fns[f"fp8_{P}_2"] = lambda i: call(i)
    new = torch.randn(q.size(0), HKV, 1, D, device="cuda").to(torch.bfloat16)  # the step's token lands on row kv_len - 1
    fns[f"append8_{P}"] = lambda i: fused.kv_cache_append_fp8(new, new, *q8[i % copies], table, kv_len)
    fns[f"append{P}"] = lambda i: fused.kv_cache_append(new, new, *pools[i % copies], table, kv_len)
    kc, vc, ke, ve = q8[0]
    deq = [torch.cat([fused.kv_dequantize_ref(c[i:i + 128], e[i:i + 128]) for i in range(0, c.size(0), 128)]) for c, e in ((kc, ke), (vc, ve))]
    return torch.equal(call(0), fused.attention_decode_paged(q, *deq, table, kv_len, kv_splits=auto))


def paged_callers(fns, q, kv_len, caches, auto, P, Smax, kv_fp8=False):
    """Adds the callers of page size P to ``fns``; -> whether the paged result equals the contiguous one bit for bit
    (and, with ``kv_fp8``, whether the fp8 result equals the bf16 paged one on the dequantised pools)."""
    B, MP, copies = q.size(0), Smax // P, len(caches)
    g = torch.Generator(device="cuda").manual_seed(P)
    tables = {"perm": torch.randperm(B * MP, generator=g, device="cuda").int().view(B, MP),
              "ident": torch.arange(B * MP, dtype=torch.int32, device="cuda").view(B, MP)}
    pools = {}
    for name, tab in tables.items():  # pool[tab[b, p]] = page p of sequence b
        pools[name] = []
        for k, v in caches:
            kp, vp = (torch.empty(B * MP, HKV, P, D, dtype=torch.bfloat16, device="cuda") for _ in range(2))
            kp[tab.long().flatten()] = k.view(B, HKV, MP, P, D).transpose(1, 2).flatten(0, 1)
            vp[tab.long().flatten()] = v.view(B, HKV, MP, P, D).transpose(1, 2).flatten(0, 1)
            pools[name].append((kp, vp))
    call = lambda name, i: fused.attention_decode_paged(q, *pools[name][i % copies], tables[name], kv_len, kv_splits=auto)  # noqa: E731
    fns[f"perm{P}"] = lambda i: call("perm", i)
    fns[f"perm{P}_2"] = lambda i: call("perm", i)
    fns[f"ident{P}"] = lambda i: call("ident", i)
    fns[f"gather{P}"] = lambda i: fused.attention_decode(
        q, fused._gather_pages(pools["perm"][i % copies][0], tables["perm"]), fused._gather_pages(pools["perm"][i % copies][1], tables["perm"]),
        kv_len, kv_splits=auto)
    want = fused.attention_decode(q, *caches[0], kv_len, kv_splits=auto)
    equal = all(torch.equal(fns[f"{name}{P}"](0), want) for name in ("perm", "ident", "gather"))
    return (equal, fp8_callers(fns, q, kv_len, pools["perm"], tables["perm"], auto, P)) if kv_fp8 else equal


def bench_shape(B, lens, Smax, iters, rounds, page_sizes=(), kv_fp8=False):
    g = torch.Generator(device="cuda").manual_seed(0)
    bf = lambda *s: torch.randn(*s, generator=g, device="cuda").to(torch.bfloat16)  # noqa: E731
    kv_bytes = 2 * HKV * sum(lens) * D * 2
    copies = max(1, min(64, -(-ROTATE_BYTES // kv_bytes)))
    q, kv_len = bf(B, H, 1, D), torch.tensor(lens, dtype=torch.int32, device="cuda")
    caches = [(bf(B, HKV, Smax, D), bf(B, HKV, Smax, D)) for _ in range(copies)]
    uniform = len(set(lens)) == 1
    reps = [(k.repeat_interleave(H // HKV, 1), v.repeat_interleave(H // HKV, 1)) for k, v in caches]
    mask = None if uniform else (torch.arange(Smax, device="cuda").view(1, 1, 1, Smax) < kv_len.view(B, 1, 1, 1))
    auto = fused.decode_splits_for(B, HKV, Smax)
    fns = {"torch": lambda i: F.scaled_dot_product_attention(q, *reps[i % copies], attn_mask=mask)}
    for n in [s for s in SPLITS if -(-Smax // 64) >= s]:
        fns[n] = lambda i, n=n: fused.attention_decode(q, *caches[i % copies], kv_len, kv_splits=n)
    fns["auto2"] = lambda i: fused.attention_decode(q, *caches[i % copies], kv_len, kv_splits=auto)
    paged_equal = {P: paged_callers(fns, q, kv_len, caches, auto, P, Smax, kv_fp8) for P in page_sizes}
    fp8_equal = {P: eq[1] for P, eq in paged_equal.items()} if kv_fp8 else {}
    if kv_fp8:
        paged_equal = {P: eq[0] for P, eq in paged_equal.items()}
    o = fused.attention_decode(q, *caches[0], kv_len, kv_splits=auto).transpose(1, 2).float()
    err = float((o - fns["torch"](0).float()).abs().max())
    keys = list(fns)
    times = {key: [] for key in keys}
    for fn in fns.values():  # warm-up
        timed(fn, 2)
    for r in range(rounds):
        for key in (keys if r % 2 == 0 else keys[::-1]):
            times[key].append(timed(fns[key], iters))
    med = {key: statistics.median(t) for key, t in times.items()}
    return {"B": B, "kv_len": lens[0] if uniform else "mixed", "Smax": Smax, "auto": auto, "copies": copies, "kv_bytes": kv_bytes,
            "max_abs_diff_vs_torch": err, "median_us": {str(k): round(t, 2) for k, t in med.items()},
            "spread": abs(med[auto] - med["auto2"]) / med[auto],
            "paged": {str(P): {"bit_equal": paged_equal[P], "perm": med[f"perm{P}"] / med[auto], "ident": med[f"ident{P}"] / med[auto],
                               "gather": med[f"gather{P}"] / med[auto], "perm_over_ident": med[f"perm{P}"] / med[f"ident{P}"],
                               "spread": abs(med[f"perm{P}"] - med[f"perm{P}_2"]) / med[f"perm{P}"]} for P in page_sizes},
            # the fp8 cache against the bf16 paged caller on the same table; the spreads of the two callers' two series
            "fp8": {str(P): {"bit_equal": fp8_equal[P], "fp8_over_paged": med[f"fp8_{P}"] / med[f"perm{P}"],
                             "spread_fp8": abs(med[f"fp8_{P}"] - med[f"fp8_{P}_2"]) / med[f"fp8_{P}"],
                             "spread_paged": abs(med[f"perm{P}"] - med[f"perm{P}_2"]) / med[f"perm{P}"],
                             "append_fp8_us": med[f"append8_{P}"], "append_bf16_us": med[f"append{P}"]} for P in fp8_equal}}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--page-size", type=int, action="append", default=[], help="also time the paged kernel at this page size (repeatable)")
    ap.add_argument("--kv-fp8", action="store_true", help="with --page-size: also time the fp8 cache against the bf16 paged caller")
    ap.add_argument("--shape", type=int, action="append", default=[], help="only this shape, an index into SHAPES (repeatable)")
    a = ap.parse_args()
    if a.kv_fp8 and not a.page_size:
        ap.error("--kv-fp8 needs --page-size")
    fused.hip()
    res = [bench_shape(B, lens, Smax, a.iters, a.rounds, tuple(a.page_size), a.kv_fp8)
           for i, (B, lens, Smax) in enumerate(SHAPES) if not a.shape or i in a.shape]
    spread = max(r["spread"] for r in res)
    print(json.dumps({"heads": [H, HKV], "iters": a.iters, "rounds": a.rounds, "spread_max": spread, "shapes": res}))
    print(f"run-to-run spread of the auto n (two interleaved series), max over shapes: {100 * spread:.2f} %")
    print("\n| B | kv_len | auto n | torch us | " + " | ".join(f"n={n}" for n in SPLITS) + " | auto us | spread | GB/s at auto | torch / auto |\n"
          + "|---" * (len(SPLITS) + 9) + "|")
    for r in res:
        m = r["median_us"]
        t = m[str(r["auto"])]
        print(f"| {r['B']} | {r['kv_len']} | {r['auto']} | {m['torch']:.1f} | " + " | ".join(f"{m[str(n)]:.1f}" if str(n) in m else "-" for n in SPLITS)
              + f" | {t:.1f} | {100 * r['spread']:.2f} % | {r['kv_bytes'] / t / 1e3:.0f} | {m['torch'] / t:.2f} |")
    print("\n| min tiles per split | shapes with n > 1 | slower than n = 1 by more than the spread (B/kv_len n ratio) | sum over shapes, auto / n = 1 |\n"
          "|---|---|---|---|")
    for c in CANDIDATES:
        picked = [(r, auto_for(r["B"], r["Smax"], c)) for r in res]
        picked = [(r, n) for r, n in picked if str(n) in r["median_us"]]
        bad = [f"{r['B']}/{r['kv_len']} n={n} {r['median_us'][str(n)] / r['median_us']['1']:.3f}" for r, n in picked
               if n > 1 and r["median_us"][str(n)] > r["median_us"]["1"] * (1 + spread)]
        tot = sum(r["median_us"][str(n)] for r, n in picked) / sum(r["median_us"]["1"] for r, _ in picked)
        print(f"| {c} | {sum(n > 1 for _, n in picked)} | {'; '.join(bad) or 'none'} | {tot:.3f} |")
    if a.page_size:
        print("\nratios to the contiguous kernel at the auto n, same rounds; spread c / p: two interleaved series of the contiguous / the paged caller"
              "\n| B | kv_len | page | bit-equal | paged perm / contig | paged ident / contig | gather + contig / contig | perm / ident | spread c | spread p |\n"
              + "|---" * 10 + "|")
        for r in res:
            for P, x in r["paged"].items():
                print(f"| {r['B']} | {r['kv_len']} | {P} | {x['bit_equal']} | {x['perm']:.3f} | {x['ident']:.3f} | {x['gather']:.2f} | "
                      f"{x['perm_over_ident']:.3f} | {100 * r['spread']:.2f} % | {100 * x['spread']:.2f} % |")
    if a.kv_fp8:
        print("\nthe fp8 cache against the bf16 paged kernel, both under the permuted table at the auto n, same rounds; bit-equal: to the bf16 paged "
              "call on the dequantised pools; append: one token per sequence, us\n"
              "| B | kv_len | page | bit-equal | paged us | fp8 us | fp8 / paged | spread paged | spread fp8 | faster by more than both | append bf16 | append fp8 |\n"
              + "|---" * 12 + "|")
        for r in res:
            for P, x in r["fp8"].items():
                m = r["median_us"]
                print(f"| {r['B']} | {r['kv_len']} | {P} | {x['bit_equal']} | {m[f'perm{P}']:.1f} | {m[f'fp8_{P}']:.1f} | {x['fp8_over_paged']:.3f} | "
                      f"{100 * x['spread_paged']:.2f} % | {100 * x['spread_fp8']:.2f} % | "
                      f"{x['fp8_over_paged'] < 1 - max(x['spread_paged'], x['spread_fp8'])} | {x['append_bf16_us']:.1f} | {x['append_fp8_us']:.1f} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
