#!/usr/bin/env python3
"""Offset-window flash attention as the ranks of a context-parallel job would call it: one sequence of
Sk = 8192 tokens (B 1, H 32, Hkv 8), K and V whole on every rank (after the all-gather), the queries split
over a world of 2, 4 and 8 ranks in two ways:

    plain    rank r holds chunk r of k chunks: one call, Sq = Sk / k at q_offset = r Sq;
    zigzag   rank r holds chunks r and 2k - 1 - r of 2k chunks: two calls, Sq = Sk / 2k each.

Each rank's share (forward, and backward from its own forward's outputs) is timed on one GPU, next to the
whole causal call at S = 8192 and to SDPA with the equivalent boolean [Sq, Sk] mask on the plain split's last
rank.  Reported per world and split: each rank's time, the slowest rank over the mean (what a step waits
for against a perfect balance) and the sum over ranks against the whole call (the overhead of splitting).

One process, warm-up first, the variants interleaved round by round (order alternating) so that clock and
thermal drift falls on all of them alike; the causal call runs twice per round, and the spread between those
two series is the noise floor.  Prints one JSON line and a markdown table (profiles/attn_qoff/SUMMARY.md
keeps a run's output).

    python bench/attn_qoff_bench.py [--iters 20] [--rounds 5] [--no-sdpa]
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
WORLDS = (2, 4, 8)


def chunks_of(world: int, split: str, rank: int):
    """(Sq, [q_offset, ...]) of a rank's calls."""
    if split == "plain":
        return SK // world, [rank * (SK // world)]
    sq = SK // (2 * world)
    return sq, [rank * sq, (2 * world - 1 - rank) * sq]


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
    ap.add_argument("--no-sdpa", action="store_true")
    a = ap.parse_args()
    hip = fused.hip()
    g = torch.Generator(device="cuda").manual_seed(0)
    bf = lambda *s: torch.randn(*s, generator=g, device="cuda").to(torch.bfloat16)  # noqa: E731
    q, k, v, do = bf(B, H, SK, D), bf(B, HKV, SK, D), bf(B, HKV, SK, D), bf(B, SK, H, D)
    sc = D ** -0.5
    fwd, bwd = {}, {}
    o, lse = hip.attn_fwd(q, k, v, sc)
    for name in ("causal", "causal-again"):
        fwd[name] = lambda: hip.attn_fwd(q, k, v, sc)
        bwd[name] = lambda o=o, lse=lse: hip.attn_bwd(do, q, k, v, o, lse, sc)
    for world in WORLDS:
        for split in ("plain", "zigzag"):
            for rank in range(world):
                sq, offs = chunks_of(world, split, rank)
                calls = []
                for off in offs:
                    qc, dc = q[:, :, off:off + sq].contiguous(), do[:, off:off + sq].contiguous()
                    oc, lc = hip.attn_fwd_qoff(qc, k, v, sc, off)
                    calls.append((qc, dc, oc, lc, off))
                name = f"{split} {world} r{rank}"
                fwd[name] = lambda calls=calls: [hip.attn_fwd_qoff(qc, k, v, sc, off) for qc, _, _, _, off in calls]
                bwd[name] = lambda calls=calls: [hip.attn_bwd_qoff(dc, qc, k, v, oc, lc, sc, off) for qc, dc, oc, lc, off in calls]
        if not a.no_sdpa:  # the plain split's last rank through SDPA with the materialised mask, K/V repeated per q-head view
            sq, off = SK // world, SK - SK // world
            qs = q[:, :, off:].detach().clone().requires_grad_(True)
            ks, vs = (t.detach().clone().requires_grad_(True) for t in (k, v))
            mask = ~torch.ones(sq, SK, dtype=torch.bool, device="cuda").triu(1 + off)  # True: j <= off + i
            dos = do[:, off:].transpose(1, 2).contiguous()

            def sdpa(qs=qs, ks=ks, vs=vs, mask=mask):
                return torch.nn.functional.scaled_dot_product_attention(qs, ks, vs, attn_mask=mask, scale=sc, enable_gqa=True)

            def sdpa_fb(qs=qs, ks=ks, vs=vs, dos=dos, f=sdpa):
                qs.grad = ks.grad = vs.grad = None
                f().backward(dos)

            fwd[f"sdpa {world} r{world - 1}"] = sdpa
            bwd[f"sdpa {world} r{world - 1}"] = sdpa_fb  # forward + backward: subtract the forward's time
    names = list(fwd)
    times = {(p, n): [] for p in ("fwd", "bwd") for n in names}
    for fns in (fwd, bwd):  # warm-up
        for fn in fns.values():
            timed(fn, 2)
    for r in range(a.rounds):
        order = names if r % 2 == 0 else names[::-1]
        for p, fns in (("fwd", fwd), ("bwd", bwd)):
            for n in order:
                times[(p, n)].append(timed(fns[n], a.iters))
    med = {f"{p} {n}": statistics.median(t) for (p, n), t in times.items()}
    for n in names:
        if n.startswith("sdpa"):
            med[f"bwd {n}"] -= med[f"fwd {n}"]
    spread = {p: abs(med[f"{p} causal"] - med[f"{p} causal-again"]) / med[f"{p} causal"] for p in ("fwd", "bwd")}
    print(json.dumps({"shape": [B, H, HKV, SK], "iters": a.iters, "rounds": a.rounds, "median_us": med, "causal_spread": spread}))
    print(f"whole causal call at S = {SK}: fwd {med['fwd causal']:.0f} us, bwd {med['bwd causal']:.0f} us")
    print("| world | split | pass | per-rank us | slowest / mean | sum / whole call | SDPA, plain last rank us (/ ours) |\n"
          "|---|---|---|---|---|---|---|")
    for world in WORLDS:
        for split in ("plain", "zigzag"):
            for p in ("fwd", "bwd"):
                t = [med[f"{p} {split} {world} r{r}"] for r in range(world)]
                s = med.get(f"{p} sdpa {world} r{world - 1}") if split == "plain" else None
                print(f"| {world} | {split} | {p} | {' '.join(f'{x:.0f}' for x in t)} | {max(t) / statistics.mean(t):.3f} | "
                      f"{sum(t) / med[p + ' causal']:.3f} | {f'{s:.0f} ({s / t[-1]:.1f}x)' if s else ''} |")
    print(f"causal run-to-run spread: fwd {100 * spread['fwd']:.2f} %, bwd {100 * spread['bwd']:.2f} %")
    return 0


if __name__ == "__main__":
    sys.exit(main())
