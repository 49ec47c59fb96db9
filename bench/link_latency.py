#!/usr/bin/env python3
"""K8 latency chase over the self path and every reachable peer, as a table and one JSON line:

    python bench/link_latency.py [--dst 0] [--srcs 0,1,...] [--hops 4096] [--iters 5] [--model]
                                 [--out FILE] [--md FILE]

Per source device (the reader ``--dst`` itself first, then every peer it can access):
  * the working-set sweep at one chain: 64 KiB, 128 KiB ... 1 GiB, stride 128.  Sets under 1 GiB are
    walked warm (one untimed lap first, ``evict=False``): the curve steps from L2 to the Infinity Cache
    to HBM as the set outgrows each.  The 1 GiB point is evicted first: a miss all the way.
  * the concurrency sweep at the evicted 1 GiB set: 1, 2, 4 ... 64 independent chains in one wave.
    ns per hop stays flat while the memory system takes the loads side by side, so chains / ns is
    the loads in flight per time (Little's law); where it stops scaling is the concurrency one wave gets.
``--model`` also times ``measure_latency`` (the stage behind ``gtk probe --latency``) on the node.
Every point is checked against the chain's closed form; the exit status is 1 when one is not exact.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpu_topology_on_k8s_amd.ops import probe  # noqa: E402

STRIDE = 128
WS_SWEEP = [1 << s for s in range(16, 31)]  # 64 KiB .. 1 GiB
CHAINS_SWEEP = [1, 2, 4, 8, 16, 32, 64]
KEYS = ("ns_per_hop", "ns_min", "ns_max", "ok", "n_nodes", "evicted")


def point(src, dst, ws, chains, hops, iters, evict):
    r = probe.chase_latency(src, dst, ws, STRIDE, hops, chains, iters, 1, evict)
    p = {k: r[k] for k in KEYS}
    p.update(ws_bytes=ws, chains=chains, hops=hops,
             event_us_per_launch=round(1e3 * sorted(r["event_ms"])[len(r["event_ms"]) // 2], 1),
             spread=round((r["ns_max"] - r["ns_min"]) / r["ns_per_hop"], 4) if r["ns_per_hop"] else None)
    print(json.dumps(p), file=sys.stderr, flush=True)
    return p


def measure(src, dst, hops, iters):
    ws = [point(src, dst, b, 1, hops, iters, evict=(b == WS_SWEEP[-1])) for b in WS_SWEEP]
    ch = [point(src, dst, WS_SWEEP[-1], c, hops, iters, evict=True) for c in CHAINS_SWEEP]
    for p in ch:
        p["loads_per_us"] = round(1e3 * p["chains"] / p["ns_per_hop"], 2)
    return {"src": src, "dst": dst, "self": src == dst, "stride": STRIDE, "working_set": ws, "chains": ch}


def size(b):
    return f"{b >> 20} MiB" if b >= 1 << 20 else f"{b >> 10} KiB"


def markdown(run) -> str:
    what = "self (own HBM)" if run["self"] else "peer"
    out = [f"### chain on device {run['src']}, walked by device {run['dst']}: {what}", "",
           "| working set | nodes | state | ns per hop (median) | min | max | spread |", "|---|---|---|---|---|---|---|"]
    for p in run["working_set"]:
        out.append(f"| {size(p['ws_bytes'])} | {p['n_nodes']} | {'evicted' if p['evicted'] else 'warm'} | {p['ns_per_hop']:.1f} "
                   f"| {p['ns_min']:.1f} | {p['ns_max']:.1f} | {100 * p['spread']:.1f} % |")
    out += ["", "| chains (1 GiB, evicted) | ns per hop (median) | min | max | loads per µs |", "|---|---|---|---|---|"]
    for p in run["chains"]:
        out.append(f"| {p['chains']} | {p['ns_per_hop']:.1f} | {p['ns_min']:.1f} | {p['ns_max']:.1f} | {p['loads_per_us']:.2f} |")
    return "\n".join(out + [""])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dst", type=int, default=0, help="HIP ordinal that walks the chains")
    ap.add_argument("--srcs", default="", help="HIP ordinals that own a chain (default: --dst and every peer it can access)")
    ap.add_argument("--hops", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--model", action="store_true", help="also time measure_latency over the node's topology")
    ap.add_argument("--out", default="", help="also write the JSON document here")
    ap.add_argument("--md", default="", help="also write the tables as Markdown here")
    a = ap.parse_args()
    if a.srcs:
        srcs = [int(x) for x in a.srcs.split(",")]
    else:
        p = probe._p()
        srcs = [a.dst] + [d for d in range(probe.device_count()) if d != a.dst and p.can_access_peer(a.dst, d)]
    probe.warmup(a.dst, 100.0)
    doc = {"device": probe.device_props(a.dst)["name"], "unit": "ns per dependent load, in-kernel wall clock",
           "runs": [measure(s, a.dst, a.hops, a.iters) for s in srcs]}
    if a.model:
        from gpu_topology_on_k8s_amd.topology.discovery import DiscoveryError, discover, fake_topology

        try:
            topo = discover("auto")
        except DiscoveryError:
            topo = fake_topology(probe.device_count())
        t0 = time.time()
        rows = probe.measure_latency(topo, list(range(topo.n)))
        doc["measure_latency"] = {"n": topo.n, "source": topo.source, "wall_s": round(time.time() - t0, 3), "latency_us": rows,
                                  "meta": topo.probe["latency_meta"]}
    text = json.dumps(doc)
    for r in doc["runs"]:
        print(markdown(r))
    print(text)
    for path, body in ((a.out, text + "\n"), (a.md, "\n".join(markdown(r) for r in doc["runs"]))):
        if path:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            with open(path, "w") as f:
                f.write(body)
    return 0 if all(p["ok"] for r in doc["runs"] for p in r["working_set"] + r["chains"]) else 1


if __name__ == "__main__":
    sys.exit(main())
