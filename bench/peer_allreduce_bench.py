#!/usr/bin/env python3
"""K7 peer all-reduce next to its comparators, on given members and sizes, as one JSON document:

    python bench/peer_allreduce_bench.py [--members 0,0,0,0] [--sizes-mib 1,4,16,64,256,1024]
                                         [--dtype bf16] [--iters 5] [--wire native|fp8|both|fp8x2|all] [--push [--reps 3]]
                                         [--out FILE] [--md FILE]

Per size N (bytes per member):
  * the peer all-reduce under both algorithms (algBW, busBW, and the bytes each member moves:
    oneshot reads k x N and writes N; twoshot reads (2 - 1/k) x N and writes N);
  * K6 ``ring_bw(members, "all")`` in the same process, each member reading as many bytes as twoshot
    does ((2 - 1/k) x N over its k - 1 peers) and writing them: the copy-only rate of the same traffic;
  * RCCL's ``local_sweep`` when the members are distinct devices (RCCL refuses a repeated device).
``--wire both`` measures the fp8 wire (``csrc/probe/peer_q8.h``: every member packs its input into e4m3
codes with a scale per 32 elements, the members read that) right after the native one at every size and
algorithm, in the same process, and reports it under ``<algo>_fp8`` with the bytes its two kernels move
and the rate each reaches alone on member 0.
``--wire fp8x2`` measures the two-shot whose gather phase is packed too (``twoshot_fp8x2``: quantize, repack,
unpack), and ``--wire all`` the two-shot on the native wire, then on ``fp8``, then on ``fp8x2`` at every size,
interleaved in one process, with the three kernels of ``fp8x2`` alone on member 0.
``--push`` measures something else: the push algorithm (one launch per member stores its slice of the sum into
every member's out) against the two-shot, on the native and on the fp8 wire, the two alternated ``--reps`` times
at every size in one process and the quicker repetition of each reported (``twoshot``, ``push``, ``twoshot_fp8``,
``push_fp8``).  No K6 or RCCL run is made.
Members that repeat a device give HBM rates of that one GPU, not xGMI rates: no store of a push then crosses a link.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpu_topology_on_k8s_amd.ops import probe  # noqa: E402

ELEM = {"bf16": 2, "fp32": 4}


def member_bytes(algo: str, k: int, n: int, wire: str = "native", elem: int = 2, out_elem: int = 0) -> dict:
    """Bytes one member reads and writes in one all-reduce of n bytes of ``elem``-byte elements.

    On the fp8 wire 32 elements pack into 33 bytes, P = 33 / (32 elem) x n per member.  The quantize
    reads n and writes P; phase 1 reads k x P (one-shot) or k x P / k = P (two-shot) and writes n or
    n / k; phase 2 of a two-shot is the native one: it reads and writes (k - 1) / k x n.

    On the fp8x2 wire (two-shot only) the quantize is the same; the repack reads k x P / k = P and writes
    P / k; the unpack reads all k slices, P, and writes the whole result, n x ``out_elem`` / ``elem``
    (``out_elem`` 0: the input's)."""
    if wire == "native":
        if algo == "push":  # slice m of every input in, slice m of every out written: n / k x k each way
            return {"read": n, "written": n}
        return {"read": k * n if algo == "oneshot" else (2 * k - 1) * n // k, "written": n}
    packed = n // elem * 33 // 32
    quantize = {"read": n, "written": packed}
    if algo == "push":  # the sum reads slice m of every packed buffer and writes slice m of every out
        return {"read": n + packed, "written": packed + n, "quantize": quantize, "sum": {"read": packed, "written": n}}
    if wire == "fp8x2":
        if algo != "twoshot":
            raise ValueError("the fp8x2 wire is a two-shot")
        repack = {"read": packed, "written": packed // k}
        unpack = {"read": packed, "written": n * (out_elem or elem) // elem}
        return {"read": n + 2 * packed, "written": packed + packed // k + unpack["written"], "quantize": quantize, "sum": repack,
                "gather": unpack}
    total = (k if algo == "oneshot" else 1) * packed
    phase1 = {"read": total, "written": n if algo == "oneshot" else n // k}
    gather = 0 if algo == "oneshot" else (k - 1) * n // k
    return {"read": n + total + gather, "written": packed + n, "quantize": quantize, "sum": phase1}


def key(algo: str, wire: str) -> str:
    return algo if wire == "native" else f"{algo}_{wire}"


def plan(wire: str):
    """The (algorithm, wire) points of one size, in the order they are measured: with ``both`` the fp8 wire
    right after the native one under each algorithm, with ``all`` the two-shot on the three wires."""
    if wire == "fp8x2":
        return [("twoshot", "fp8x2")]
    if wire == "all":
        return [("twoshot", w) for w in ("native", "fp8", "fp8x2")]
    return [(a, w) for a in probe.PEER_ALGOS for w in ("native", "fp8") if wire in (w, "both")]


def point(devs, n, dtype, algo, iters, warmup, wire):
    k = len(devs)
    r = probe.peer_allreduce(devs, n // ELEM[dtype], dtype, algo, iters, warmup, wire=wire)
    mv = member_bytes(algo, k, n, wire, ELEM[dtype])
    secs = r["time_us"] * 1e-6
    p = {"time_us": r["time_us"], "algbw_gbps": r["algbw_gbps"], "busbw_gbps": r["busbw_gbps"],
         "wrong": r["wrong"], "member_read_bytes": mv["read"], "member_written_bytes": mv["written"],
         "member_read_gbps": mv["read"] / secs / 1e9,
         "member_traffic_gbps": (mv["read"] + mv["written"]) / secs / 1e9}
    if wire != "native":  # member 0's kernels alone on the device: the bytes each moves over its own time
        for name in ("quantize", "sum") + (("gather",) if wire == "fp8x2" else ()):
            b = mv[name]["read"] + mv[name]["written"]
            p[name] = {"time_us": r[name + "_us"], "bytes": b, "gbps": b / (r[name + "_us"] * 1e-6) / 1e9}
    return p


def measure(devs, sizes, dtype, iters, warmup, wire="native"):
    k = len(devs)
    distinct = len(set(devs)) == k
    rows = []
    for n in sizes:
        row = {"bytes": n}
        for algo, w in plan(wire):
            row[key(algo, w)] = point(devs, n, dtype, algo, iters, warmup, w)
        first = plan(wire)[0][1]  # the algorithms are compared on one wire, the first one measured
        row["faster"] = min((key(a, w) for a, w in plan(wire) if w == first), key=lambda a: row[a]["time_us"])
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
    both_algos = len({a for a, _ in plan(wire)}) > 1  # fp8x2 and all measure the two-shot alone: no crossover to report
    crossover = next((r["bytes"] for i, r in enumerate(rows) if both_algos and all(q["faster"].startswith("twoshot") for q in rows[i:])), None)
    return {"members": list(devs), "k": k, "distinct_devices": distinct, "dtype": dtype, "iters": iters, "warmup": warmup,
            "wire": wire, "sizes": rows, "twoshot_faster_from_bytes": crossover}


PUSH_PAIRS = (("twoshot", "native"), ("push", "native"), ("twoshot", "fp8"), ("push", "fp8"))


def measure_push(devs, sizes, dtype, iters, warmup, reps):
    """Push against two-shot on both wires: per size the four points in the order of PUSH_PAIRS, ``reps`` times
    over, so the two algorithms alternate; the quicker repetition of each is the point reported."""
    k = len(devs)
    rows = []
    for n in sizes:
        runs = {key(a, w): [] for a, w in PUSH_PAIRS}
        for _ in range(reps):
            for a, w in PUSH_PAIRS:
                runs[key(a, w)].append(point(devs, n, dtype, a, iters, warmup, w))
        row = {"bytes": n}
        for name, pts in runs.items():
            best = min(pts, key=lambda p: p["time_us"])
            row[name] = {**best, "time_us_reps": [p["time_us"] for p in pts], "wrong": sum(p["wrong"] for p in pts)}
        for sfx in ("", "_fp8"):
            row["push_over_twoshot" + sfx] = row["push" + sfx]["time_us"] / row["twoshot" + sfx]["time_us"]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return {"members": list(devs), "k": k, "distinct_devices": len(set(devs)) == k, "dtype": dtype, "iters": iters, "warmup": warmup,
            "reps": reps, "push": True, "derived_traffic_ratio": (3 - 1 / k) / 2, "sizes": rows}


def markdown_push(res) -> str:
    mib = lambda b: f"{b / 2**20:.1f}"  # noqa: E731
    out = [f"### push against two-shot, driver, members {res['members']} (k = {res['k']}), {res['dtype']}, {res['iters']} timed rounds, "
           f"best of {res['reps']} alternated repetitions", "",
           "| N per member MiB | wire | twoshot us | push us | push / twoshot time | twoshot / push time | twoshot MiB read + written | "
           "push MiB read + written | wrong |", "|---|---|---|---|---|---|---|---|---|"]
    for r in res["sizes"]:
        for sfx, wire in (("", "native"), ("_fp8", "fp8")):
            t, p = r["twoshot" + sfx], r["push" + sfx]
            out.append(f"| {mib(r['bytes'])} | {wire} | {t['time_us']:.1f} | {p['time_us']:.1f} | {p['time_us'] / t['time_us']:.2f} "
                       f"| {t['time_us'] / p['time_us']:.2f} | {mib(t['member_read_bytes'])} + {mib(t['member_written_bytes'])} "
                       f"| {mib(p['member_read_bytes'])} + {mib(p['member_written_bytes'])} | {t['wrong'] + p['wrong']} |")
    out += ["", f"Derived traffic of one member on the native wire, two-shot over push: (3 - 1/k) / 2 = {res['derived_traffic_ratio']:.3f}.", ""]
    return "\n".join(out)


def markdown_fp8(res) -> str:
    """The fp8 wire next to the native one: one line per size and algorithm."""
    mib = lambda b: f"{b / 2**20:.1f}"  # noqa: E731
    native = res["wire"] == "both"
    out = [f"### fp8 wire, members {res['members']} (k = {res['k']}), {res['dtype']}, {res['iters']} timed rounds", "",
           "| N per member MiB | algorithm | native us | native algBW | fp8 us | fp8 algBW | fp8 / native time | native MiB read + written | "
           "fp8 MiB read + written | quantize us | quantize GB/s | sum us | sum GB/s | wrong |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["sizes"]:
        for algo in probe.PEER_ALGOS:
            f, o = r[algo + "_fp8"], r.get(algo)
            nat = [f"{o['time_us']:.1f}", f"{o['algbw_gbps']:.1f}"] if native else ["", ""]
            ratio = f"{f['time_us'] / o['time_us']:.2f}" if native else ""
            moved = f"{mib(o['member_read_bytes'])} + {mib(o['member_written_bytes'])}" if native else ""
            out.append(f"| {mib(r['bytes'])} | {algo} | {nat[0]} | {nat[1]} | {f['time_us']:.1f} | {f['algbw_gbps']:.1f} | {ratio} | {moved} "
                       f"| {mib(f['member_read_bytes'])} + {mib(f['member_written_bytes'])} | {f['quantize']['time_us']:.1f} "
                       f"| {f['quantize']['gbps']:.0f} | {f['sum']['time_us']:.1f} | {f['sum']['gbps']:.0f} | {f['wrong'] + (o['wrong'] if native else 0)} |")
    out.append("")
    return "\n".join(out)


def markdown_fp8x2(res) -> str:
    """The two-shot on the fp8x2 wire, next to the native and the fp8 one where they were measured: one line per size."""
    mib = lambda b: f"{b / 2**20:.1f}"  # noqa: E731
    others = [w for w in ("native", "fp8") if res["wire"] == "all"]
    head = ["N per member MiB"] + [f"{w} us" for w in others] + ["fp8x2 us", "fp8x2 algBW"] + [f"fp8x2 / {w} time" for w in others]
    head += [f"{w} MiB read + written" for w in others + ["fp8x2"]]
    head += [f"{name} {unit}" for name in ("quantize", "repack", "unpack") for unit in ("us", "GB/s")]
    head += (["fp8 sum us", "fp8 sum GB/s"] if others else []) + ["wrong"]  # the sum kernel in the repack's position
    out = [f"### fp8x2 wire, two-shot, members {res['members']} (k = {res['k']}), {res['dtype']}, {res['iters']} timed rounds", "",
           "| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in res["sizes"]:
        x, o = r["twoshot_fp8x2"], [r[key("twoshot", w)] for w in others]
        cells = [mib(r["bytes"])] + [f"{p['time_us']:.1f}" for p in o] + [f"{x['time_us']:.1f}", f"{x['algbw_gbps']:.1f}"]
        cells += [f"{x['time_us'] / p['time_us']:.2f}" for p in o]
        cells += [f"{mib(p['member_read_bytes'])} + {mib(p['member_written_bytes'])}" for p in o + [x]]
        for name in ("quantize", "sum", "gather"):
            cells += [f"{x[name]['time_us']:.1f}", f"{x[name]['gbps']:.0f}"]
        if others:
            cells += [f"{o[1]['sum']['time_us']:.1f}", f"{o[1]['sum']['gbps']:.0f}"]
        out.append("| " + " | ".join(cells + [str(x["wrong"] + sum(p["wrong"] for p in o))]) + " |")
    out.append("")
    return "\n".join(out)


def markdown(res) -> str:
    if res.get("push"):
        return markdown_push(res)
    if res["wire"] == "fp8":
        return markdown_fp8(res)
    if res["wire"] in ("fp8x2", "all"):
        return markdown_fp8x2(res)
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
    return "\n".join(out) + ("\n" + markdown_fp8(res) if res["wire"] == "both" else "")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", action="append", default=[], help="HIP ordinals, comma-separated; may be given more than once")
    ap.add_argument("--sizes-mib", default="1,4,16,64,256,1024")
    ap.add_argument("--dtype", default="bf16", choices=sorted(ELEM))
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--wire", default="native", choices=["native", "fp8", "both", "fp8x2", "all"],
                    help="fp8: the block-scaled e4m3 wire alone; both: it next to the native wire, interleaved; fp8x2: the "
                         "two-shot with its gather phase packed too; all: the two-shot on native, fp8 and fp8x2, interleaved")
    ap.add_argument("--push", action="store_true", help="the push algorithm against the two-shot on the native and the fp8 wire, alternated")
    ap.add_argument("--reps", type=int, default=3, help="--push: alternated repetitions of each measurement")
    ap.add_argument("--out", default="", help="also write the JSON document here")
    ap.add_argument("--md", default="", help="also write the tables as Markdown here")
    a = ap.parse_args()
    groups = [[int(x) for x in m.split(",")] for m in (a.members or ["0,0,0,0"])]
    sizes = [int(float(x) * (1 << 20)) for x in a.sizes_mib.split(",")]
    probe.warmup(groups[0][0], 100.0)
    doc = {"device": probe.device_props(groups[0][0])["name"], "rates": "GB/s (1e9 bytes/s)",
           "runs": [measure_push(g, sizes, a.dtype, a.iters, a.warmup, max(1, a.reps)) if a.push else
                    measure(g, sizes, a.dtype, a.iters, a.warmup, a.wire) for g in groups]}
    text = json.dumps(doc)
    print(text)
    for path, body in ((a.out, text + "\n"), (a.md, "\n".join(markdown(r) for r in doc["runs"]))):
        if path:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            with open(path, "w") as f:
                f.write(body)
    measured = [al + sfx for al in probe.PEER_ALGOS + (probe.PEER_PUSH,) for sfx in ("", "_fp8", "_fp8x2")]
    return 1 if any(r[al]["wrong"] for run in doc["runs"] for r in run["sizes"] for al in measured if al in r) else 0


if __name__ == "__main__":
    sys.exit(main())
