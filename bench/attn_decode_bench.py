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

    python bench/attn_decode_bench.py [--iters 10] [--rounds 5]
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


def bench_shape(B, lens, Smax, iters, rounds):
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
            "spread": abs(med[auto] - med["auto2"]) / med[auto]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    fused.hip()
    res = [bench_shape(B, lens, Smax, a.iters, a.rounds) for B, lens, Smax in SHAPES]
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
    return 0


if __name__ == "__main__":
    sys.exit(main())
