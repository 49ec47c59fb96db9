#!/usr/bin/env python3
"""Document-masked flash attention against the causal kernels at config 5's shape (B 4, H 32, Hkv 8,
S 4096): forward and backward times of the causal entry points next to the document ones with
doc_start = 0 and with uniform documents of 4096, 1024, 512 and 128 tokens.

One process, warm-up first, the variants interleaved round by round (order alternating) so that clock
and thermal drift falls on all of them alike; the causal pair runs twice per round, and the spread
between those two series is the noise floor any gap has to be read against.  Prints one JSON line and a
markdown table (profiles/attn_doc/SUMMARY.md keeps a run's output).

    python bench/attn_doc_bench.py [--iters 20] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_topology_on_k8s_amd.ops import fused  # noqa: E402

B, H, HKV, S, D = 4, 32, 8, 4096, 128
DOCS = (4096, 1024, 512, 128)


def visible_tiles(doc: int) -> float:
    """Visible 64 x 64 score tiles of a row of S tokens in documents of ``doc`` tokens, over the causal count."""
    per = lambda n: (n // 64) * (n // 64 + 1) // 2  # noqa: E731
    return (S // doc) * per(doc) / per(S)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated variants to run, e.g. 'causal,doc_start=0' under a kernel "
                    "trace (rocprofv3 --kernel-trace --stats), whose per-kernel times split the backward between dK/dV and dQ")
    a = ap.parse_args()
    hip = fused.hip()
    g = torch.Generator(device="cuda").manual_seed(0)
    bf = lambda *s: torch.randn(*s, generator=g, device="cuda").to(torch.bfloat16)  # noqa: E731
    q, k, v, do = bf(B, H, S, D), bf(B, HKV, S, D), bf(B, HKV, S, D), bf(B, S, H, D)
    sc = D ** -0.5
    pos = torch.arange(S, device="cuda", dtype=torch.int32).expand(B, S)
    variants = {"causal": None, "causal-again": None, "doc_start=0": fused.doc_bounds(torch.zeros_like(pos))}
    for n in DOCS:
        variants[f"doc {n}"] = fused.doc_bounds(pos - pos % n)
    if a.only:
        variants = {n: d for n, d in variants.items() if n in a.only.split(",") or n.startswith("causal")}
    fwd, bwd = {}, {}
    for name, doc in variants.items():
        if doc is None:
            o, lse = hip.attn_fwd(q, k, v, sc)
            fwd[name] = lambda: hip.attn_fwd(q, k, v, sc)
            bwd[name] = lambda o=o, lse=lse: hip.attn_bwd(do, q, k, v, o, lse, sc)
        else:
            o, lse = hip.attn_fwd_doc(q, k, v, sc, *doc)
            fwd[name] = lambda doc=doc: hip.attn_fwd_doc(q, k, v, sc, *doc)
            bwd[name] = lambda o=o, lse=lse, doc=doc: hip.attn_bwd_doc(do, q, k, v, o, lse, sc, *doc)
    times = {(p, n): [] for p in ("fwd", "bwd") for n in variants}
    for fns in (fwd, bwd):  # warm-up
        for fn in fns.values():
            timed(fn, 3)
    for r in range(a.rounds):
        order = list(variants) if r % 2 == 0 else list(variants)[::-1]
        for p, fns in (("fwd", fwd), ("bwd", bwd)):
            for n in order:
                times[(p, n)].append(timed(fns[n], a.iters))
    med = {f"{p} {n}": statistics.median(t) for (p, n), t in times.items()}
    spread = {p: abs(med[f"{p} causal"] - med[f"{p} causal-again"]) / med[f"{p} causal"] for p in ("fwd", "bwd")}
    print(json.dumps({"shape": [B, H, HKV, S], "iters": a.iters, "rounds": a.rounds, "median_us": med, "causal_spread": spread}))
    print("| variant | fwd us | fwd / causal | bwd us | bwd / causal | visible tiles / causal |\n|---|---|---|---|---|---|")
    for n in variants:
        vis = "" if n.startswith("causal") else f"{visible_tiles(S if n == 'doc_start=0' else int(n.split()[1])):.3f}"
        print(f"| {n} | {med['fwd ' + n]:.0f} | {med['fwd ' + n] / med['fwd causal']:.3f} | {med['bwd ' + n]:.0f} | "
              f"{med['bwd ' + n] / med['bwd causal']:.3f} | {vis} |")
    print(f"causal run-to-run spread: fwd {100 * spread['fwd']:.2f} %, bwd {100 * spread['bwd']:.2f} %")
    return 0


if __name__ == "__main__":
    sys.exit(main())
