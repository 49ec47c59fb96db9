"""One-rank all-reduce A/B on one MI355X: RCCL's path (the HIP runtime's copy) against this
repository's copy kernel (csrc/rccl/self_copy.h), from ``Comm.step()`` as bench.py times it
(profiles/k1_self_copy).

    python bench/allreduce_k1_ab.py [--sizes 65536,16M,128M,1G,2G,8G] [--rounds 5] [--min-ms 20] [--dtype bf16]
                                    [--cutoff 0]

One process, one ``Comm``.  For every size the two arms alternate (``Comm.self_copy`` off, on) for
``--rounds`` rounds; one run of an arm is K out-of-place steps between two ``synchronize()`` calls, K
grown per size and arm until the run lasts at least ``--min-ms`` (a shorter run is repeated with more).
Prints one JSON line per run, then per size and arm the median and the min-max of the copied GB/s, and a
verdict line per size.  ``--cutoff 0`` (the default) sends every size of the ``self_copy`` arm to the
kernel, which is what the choice of ``kSelfCopyMinBytes`` rests on; ``--cutoff build`` measures the
routing as built.
There is no CPU path: without a GPU the communicator cannot be built and the script fails."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpu_topology_on_k8s_amd._native import load  # noqa: E402

DEFAULT_SIZES = "65536,16M,128M,1G,2G,8G"


def parse_size(s: str) -> int:
    mul = {"K": 1 << 10, "M": 1 << 20, "G": 1 << 30}.get(s[-1].upper())
    return int(float(s[:-1]) * mul) if mul else int(s)


def run(c, k: int) -> float:
    """Seconds for k steps, the stream idle before and after."""
    c.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        c.step(False)
    c.synchronize()
    return time.perf_counter() - t0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default=DEFAULT_SIZES)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-ms", type=float, default=20.0)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--cutoff", default="0", help="smallest message of the self_copy arm that goes to the kernel: "
                                                   "bytes, or 'build' for the built-in SELF_COPY_MIN_BYTES")
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds must be at least 5")
    rccl = load("_rccl")
    c = rccl.Comm(rccl.unique_id(), 1, 0, a.device)
    if a.cutoff != "build":
        c.self_copy_min_bytes = parse_size(a.cutoff)
    print(json.dumps({"cutoff_bytes": c.self_copy_min_bytes, "built_in_cutoff_bytes": rccl.SELF_COPY_MIN_BYTES,
                      "tile_bytes": rccl.SELF_COPY_TILE_BYTES, "max_blocks": c.self_copy_max_blocks}), flush=True)
    arms = (("rccl", False), ("self_copy", True))
    for nbytes in [parse_size(s) for s in a.sizes.split(",") if s]:
        c.prepare(nbytes, a.dtype)
        steps = {}
        for name, on in arms:  # warm the path, then grow K until one run of it lasts 1.25 x --min-ms
            c.self_copy = on
            if c.check(False) != 0:
                print(json.dumps({"bytes": c.bytes, "arm": name, "error": "wrong result"}))
                return 1
            k, target = 5, 1.25e-3 * a.min_ms
            s = run(c, k)
            while s < target:
                k = max(k + 1, int(k * target / s * 1.1))
                s = run(c, k)
            steps[name] = k
        got = {name: [] for name, _ in arms}
        for rnd in range(a.rounds):
            for name, on in arms:
                c.self_copy = on
                s = run(c, steps[name])
                while s < a.min_ms * 1e-3:  # a run shorter than asked for is not kept: more steps, again
                    steps[name] = int(steps[name] * 1.25) + 1
                    s = run(c, steps[name])
                gbps = c.bytes * steps[name] / s / 1e9
                got[name].append(gbps)
                print(json.dumps({"bytes": c.bytes, "arm": name, "round": rnd, "steps": steps[name],
                                  "ms": round(s * 1e3, 3), "us_per_step": round(s / steps[name] * 1e6, 2),
                                  "gbps": round(gbps, 3)}), flush=True)
        row = {"bytes": c.bytes, "dtype": a.dtype}
        for name, _ in arms:
            v = got[name]
            row[name] = {"median_gbps": round(statistics.median(v), 3), "min_gbps": round(min(v), 3),
                         "max_gbps": round(max(v), 3)}
        row["gain"] = round(statistics.median(got["self_copy"]) / statistics.median(got["rccl"]), 4)
        # a win or a loss only when the two arms' ranges do not overlap
        row["verdict"] = ("self_copy" if min(got["self_copy"]) > max(got["rccl"]) else
                          "rccl" if min(got["rccl"]) > max(got["self_copy"]) else "within spread")
        print(json.dumps(row), flush=True)
    c.self_copy = True
    c.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
