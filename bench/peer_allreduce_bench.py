#!/usr/bin/env python3
"""K7 peer all-reduce next to its comparators, on given members and sizes, as one JSON document:

    python bench/peer_allreduce_bench.py [--members 0,0,0,0] [--sizes-mib 1,4,16,64,256,1024]
                                         [--dtype bf16] [--iters 5] [--out FILE] [--md FILE]

Per size N (bytes per member):
  * the peer all-reduce under both algorithms (algBW, busBW, and the bytes each member moves:
    oneshot reads k x N and writes N; twoshot reads (2 - 1/k) x N and writes N);
  * K6 ``ring_bw(members, "all")`` in the same process, each member reading as many bytes as twoshot
    does ((2 - 1/k) x N over its k - 1 peers) and writing them: the copy-only rate of the same traffic;
  * RCCL's ``local_sweep`` when the members are distinct devices (RCCL refuses a repeated device).
Members that repeat a device give HBM rates of that one GPU, not xGMI rates.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpu_topology_on_k8s_amd.ops import probe  # noqa: E402

ELEM = {"bf16": 2, "fp32": 4}


def member_bytes(algo: str, k: int, n: int) -> dict:
    """Bytes one member reads and writes in one all-reduce of n bytes."""
    return {"read": k * n if algo == "oneshot" else (2 * k - 1) * n // k, "written": n}


def measure(devs, sizes, dtype, iters, warmup):
    k = len(devs)
    distinct = len(set(devs)) == k
    rows = []
    for n in sizes:
        row = {"bytes": n}
        for algo in probe.PEER_ALGOS:
            r = probe.peer_allreduce(devs, n // ELEM[dtype], dtype, algo, iters, warmup)
            mv = member_bytes(algo, k, n)
            secs = r["time_us"] * 1e-6
            row[algo] = {"time_us": r["time_us"], "algbw_gbps": r["algbw_gbps"], "busbw_gbps": r["busbw_gbps"],
                         "wrong": r["wrong"], "member_read_bytes": mv["read"], "member_written_bytes": mv["written"],
                         "member_read_gbps": mv["read"] / secs / 1e9,
                         "member_traffic_gbps": (mv["read"] + mv["written"]) / secs / 1e9}
        row["faster"] = min(probe.PEER_ALGOS, key=lambda a: row[a]["time_us"])
        per_peer = max(16, member_bytes("twoshot", k, n)["read"] // (k - 1) // 16 * 16)
        r6 = probe.ring_bw(devs, "all", per_peer, iters, warmup)
        row["k6_all"] = {"bytes_per_peer": per_peer, "member_read_bytes": per_peer * (k - 1), "ok": r6["ok"],
                         "ingress_bound_gbps": r6["bound_gbps"], "member_traffic_gbps": 2 * r6["bound_gbps"]}
        if distinct:
            from gpu_topology_on_k8s_amd._native import load

            p = load("_rccl").local_sweep(list(devs), [n], dtype, iters, warmup, False, True)[0]
            row["rccl"] = {k_: p[k_] for k_ in ("time_us", "algbw_gbps", "busbw_gbps", "wrong")}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    crossover = next((r["bytes"] for i, r in enumerate(rows) if all(q["faster"] == "twoshot" for q in rows[i:])), None)
    return {"members": list(devs), "k": k, "distinct_devices": distinct, "dtype": dtype, "iters": iters, "warmup": warmup,
            "sizes": rows, "twoshot_faster_from_bytes": crossover}


def markdown(res) -> str:
    k = res["k"]
    out = [f"### members {res['members']} (k = {k}), {res['dtype']}, {res['iters']} timed rounds", "",
           "| N per member | oneshot algBW | oneshot member read + written | twoshot algBW | twoshot member read + written | "
           "twoshot traffic | K6 `all` ingress (same bytes read) | K6 traffic | faster |",
           "|---|---|---|---|---|---|---|---|---|"]
    mib = lambda b: f"{b / 2**20:.1f} MiB"  # noqa: E731
    for r in res["sizes"]:
        o, t, k6 = r["oneshot"], r["twoshot"], r["k6_all"]
        out.append(f"| {mib(r['bytes'])} | {o['algbw_gbps']:.1f} | {mib(o['member_read_bytes'])} + {mib(o['member_written_bytes'])} "
                   f"| {t['algbw_gbps']:.1f} | {mib(t['member_read_bytes'])} + {mib(t['member_written_bytes'])} "
                   f"| {t['member_traffic_gbps']:.1f} | {k6['ingress_bound_gbps']:.1f} | {k6['member_traffic_gbps']:.1f} | {r['faster']} |")
    c = res["twoshot_faster_from_bytes"]
    out += ["", f"twoshot is the faster algorithm from {mib(c)} up." if c else "twoshot is not the faster algorithm at the largest size.", ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", action="append", default=[], help="HIP ordinals, comma-separated; may be given more than once")
    ap.add_argument("--sizes-mib", default="1,4,16,64,256,1024")
    ap.add_argument("--dtype", default="bf16", choices=sorted(ELEM))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="", help="also write the JSON document here")
    ap.add_argument("--md", default="", help="also write the tables as Markdown here")
    a = ap.parse_args()
    groups = [[int(x) for x in m.split(",")] for m in (a.members or ["0,0,0,0"])]
    sizes = [int(float(x) * (1 << 20)) for x in a.sizes_mib.split(",")]
    probe.warmup(groups[0][0], 100.0)
    doc = {"device": probe.device_props(groups[0][0])["name"], "rates": "GB/s (1e9 bytes/s)",
           "runs": [measure(g, sizes, a.dtype, a.iters, a.warmup) for g in groups]}
    text = json.dumps(doc)
    print(text)
    for path, body in ((a.out, text + "\n"), (a.md, "\n".join(markdown(r) for r in doc["runs"]))):
        if path:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            with open(path, "w") as f:
                f.write(body)
    return 1 if any(r[al]["wrong"] for run in doc["runs"] for r in run["sizes"] for al in probe.PEER_ALGOS) else 0


if __name__ == "__main__":
    sys.exit(main())
