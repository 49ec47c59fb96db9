#!/usr/bin/env python3
"""Split-KV flash attention against the unsplit offset-window call, at the shapes of bench/attn_qoff_bench.py:
one sequence of Sk = 8192 tokens (B 1, H 32, Hkv 8), K and V whole on every rank, the queries cut into 2, 4, 8
and 16 chunks.  Chunk j of C is one call, Sq = Sk / C at q_offset = j Sq: rank j of a plain split over a world
of C, and with chunk C - 1 - j the two calls of rank j of a zigzag split over a world of C / 2.

Every call is timed unsplit (``attn_fwd_qoff`` / ``attn_bwd_qoff``: what ``kv_splits=None`` runs, the path of
before the split kernels) twice and with n = 1, 2, 4, 8 splits (``attn_*_qoff_split``), forward and backward
(from the unsplit forward's outputs), all series interleaved round by round in one process, order alternating.
The two unsplit series of a call give its run-to-run spread.  A rank's time is the sum of its calls' medians.

Printed: one JSON line; the table per call; for each candidate minimum of key blocks per split what
``fused.kv_splits_for`` would pick and where that pick is slower than the unsplit call by more than the
spread; and the sum over ranks against the whole causal call with ``kv_splits=None`` and ``"auto"``
(profiles/attn_splitkv/SUMMARY.md keeps a run's output).

    python bench/attn_splitkv_bench.py [--iters 20] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_topology_on_k8s_amd.ops import fused  # noqa: E402

B, H, HKV, SK, D = 1, 32, 8, 8192, 128
CHUNKS = (2, 4, 8, 16)
SPLITS = (1, 2, 4, 8)
CANDIDATES = (1, 2, 4, 6, 8, 9, 10, 12, 16, 32)  # minimum key blocks per split


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def auto_for(sq, off, min_blocks):
    """kv_splits_for under a candidate minimum."""
    saved, fused.MIN_KEY_BLOCKS_PER_SPLIT = fused.MIN_KEY_BLOCKS_PER_SPLIT, min_blocks
    try:
        return fused.kv_splits_for(B, H, sq, SK, off)
    finally:
        fused.MIN_KEY_BLOCKS_PER_SPLIT = saved


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    hip = fused.hip()
    g = torch.Generator(device="cuda").manual_seed(0)
    bf = lambda *s: torch.randn(*s, generator=g, device="cuda").to(torch.bfloat16)  # noqa: E731
    q, k, v, do = bf(B, H, SK, D), bf(B, HKV, SK, D), bf(B, HKV, SK, D), bf(B, SK, H, D)
    sc = D ** -0.5
    o, lse = hip.attn_fwd(q, k, v, sc)
    fns = {("fwd", "causal"): lambda: hip.attn_fwd(q, k, v, sc), ("bwd", "causal"): lambda: hip.attn_bwd(do, q, k, v, o, lse, sc)}
    calls = [(c, j) for c in CHUNKS for j in range(c)]
    for c, j in calls:
        sq, off = SK // c, j * (SK // c)
        qc, dc = q[:, :, off:off + sq].contiguous(), do[:, off:off + sq].contiguous()
        oc, lc = hip.attn_fwd_qoff(qc, k, v, sc, off)
        for tag in ("none", "none2"):
            fns[("fwd", c, j, tag)] = lambda qc=qc, off=off: hip.attn_fwd_qoff(qc, k, v, sc, off)
            fns[("bwd", c, j, tag)] = lambda qc=qc, dc=dc, oc=oc, lc=lc, off=off: hip.attn_bwd_qoff(dc, qc, k, v, oc, lc, sc, off)
        for n in SPLITS:
            fns[("fwd", c, j, n)] = lambda qc=qc, off=off, n=n: hip.attn_fwd_qoff_split(qc, k, v, sc, off, n)
            fns[("bwd", c, j, n)] = lambda qc=qc, dc=dc, oc=oc, lc=lc, off=off, n=n: hip.attn_bwd_qoff_split(dc, qc, k, v, oc, lc, sc,
                                                                                                            off, n)
    keys = list(fns)
    times = {key: [] for key in keys}
    for fn in fns.values():  # warm-up
        timed(fn, 2)
    for r in range(a.rounds):
        for key in (keys if r % 2 == 0 else keys[::-1]):
            times[key].append(timed(fns[key], a.iters))
    med = {key: statistics.median(t) for key, t in times.items()}
    spreads = {p: [abs(med[(p, c, j, "none")] - med[(p, c, j, "none2")]) / med[(p, c, j, "none")] for c, j in calls]
               for p in ("fwd", "bwd")}
    spread = {p: max(s) for p, s in spreads.items()}
    print(json.dumps({"shape": [B, H, HKV, SK], "iters": a.iters, "rounds": a.rounds,
                      "median_us": {" ".join(map(str, key)): round(t, 2) for key, t in med.items()},
                      "spread_max": spread, "spread_median": {p: statistics.median(s) for p, s in spreads.items()}}))
    print(f"whole causal call at S = {SK}: fwd {med[('fwd', 'causal')]:.0f} us, bwd {med[('bwd', 'causal')]:.0f} us")
    print(f"unsplit run-to-run spread over the {len(calls)} calls: " + ", ".join(
        f"{p} median {100 * statistics.median(spreads[p]):.2f} % max {100 * spread[p]:.2f} %" for p in ("fwd", "bwd")))
    print("\n| chunks | chunk | Sq | q_offset | blocks | key blocks | pass | unsplit us | n=1 | n=2 | n=4 | n=8 | best n (/ unsplit) |\n"
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for c, j in calls:
        sq, off = SK // c, j * (SK // c)
        for p in ("fwd", "bwd"):
            t = [med[(p, c, j, n)] for n in SPLITS]
            best = min(range(len(SPLITS)), key=t.__getitem__)
            print(f"| {c} | {j} | {sq} | {off} | {H * sq // 128} | {(off + sq) // 128} | {p} | {med[(p, c, j, 'none')]:.0f} | "
                  + " | ".join(f"{x:.0f}" for x in t) + f" | {SPLITS[best]} ({t[best] / med[(p, c, j, 'none')]:.2f}) |")

    def auto_time(p, c, j, m):
        n = auto_for(SK // c, j * (SK // c), m)
        return med[(p, c, j, "none" if n == 1 else n)], n

    print("\n| min key blocks per split | calls with n > 1 | slower than unsplit by more than the spread (chunks/chunk pass n ratio) | "
          "sum of all calls, auto / unsplit: fwd | bwd |\n|---|---|---|---|---|")
    for m in CANDIDATES:
        picked = [(c, j, auto_for(SK // c, j * (SK // c), m)) for c, j in calls]
        bad = [f"{c}/{j} {p} n={n} {med[(p, c, j, n)] / med[(p, c, j, 'none')]:.3f}" for c, j, n in picked if n > 1
               for p in ("fwd", "bwd") if med[(p, c, j, n)] > med[(p, c, j, "none")] * (1 + spread[p])]
        tot = [sum(auto_time(p, c, j, m)[0] for c, j in calls) / sum(med[(p, c, j, "none")] for c, j in calls) for p in ("fwd", "bwd")]
        print(f"| {m} | {sum(n > 1 for _, _, n in picked)} | {'; '.join(bad) or 'none'} | {tot[0]:.3f} | {tot[1]:.3f} |")
    m = fused.MIN_KEY_BLOCKS_PER_SPLIT
    print(f"\nwith MIN_KEY_BLOCKS_PER_SPLIT = {m}:\n| world | split | pass | per-rank us, unsplit | per-rank us, auto (n per call) | "
          "sum / whole call, unsplit | sum / whole call, auto |\n|---|---|---|---|---|---|---|")
    for world in (2, 4, 8):
        for split, c in (("plain", world), ("zigzag", 2 * world)):
            rank_calls = [[r] if split == "plain" else [r, c - 1 - r] for r in range(world)]
            for p in ("fwd", "bwd"):
                t0 = [sum(med[(p, c, j, "none")] for j in js) for js in rank_calls]
                t1 = [sum(auto_time(p, c, j, m)[0] for j in js) for js in rank_calls]
                ns = ["+".join(str(auto_time(p, c, j, m)[1]) for j in js) for js in rank_calls]
                whole = med[(p, "causal")]
                print(f"| {world} | {split} | {p} | {' '.join(f'{x:.0f}' for x in t0)} | "
                      + " ".join(f"{x:.0f} ({n})" for x, n in zip(t1, ns)) + f" | {sum(t0) / whole:.3f} | {sum(t1) / whole:.3f} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
