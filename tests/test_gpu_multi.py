"""GPU, k >= 2: the multi-device paths the 8-GPU scaling run depends on (VERDICT r1 "next" #2).

Every test here needs at least two visible MI355X and skips with the reason on a 1-GPU box; on the
8-GPU node they localise a failure of the scaling curve to one component: the p2p probe kernels
across a real xGMI pair (K1 read, K2 write), the all-peer gather (K5), the RCCL communicator at
k=2 (bench.py, native backend, exact check, busBW bounded by the probe), hipGraph capture at k=2,
and 2-rank Llama DP / ZeRO-1 and MNIST DP against the 1-rank run.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ndev() -> int:
    import torch

    return int(torch.cuda.device_count())  # counts without initialising HIP on this image


needs2 = pytest.mark.skipif(_ndev() < 2, reason="needs >= 2 visible GPUs (single-GPU box)")


def _run(args, timeout=900, env=None):
    e = dict(os.environ, **(env or {}))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    p = subprocess.run([sys.executable, *args], capture_output=True, text=True, timeout=timeout, cwd=REPO, env=e)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def _topo():
    from gpu_topology_on_k8s_amd.topology.discovery import discover

    return discover("auto")


def _hip_to_topo(t):
    """HIP ordinal -> topology index (by PCI address; identity when the node shows all its GPUs)."""
    from gpu_topology_on_k8s_amd.ops import probe

    bdf = {g.bdf.lower(): g.index for g in t.gpus if g.bdf}
    out = {}
    for h in range(_ndev()):
        b = str(probe.device_props(h).get("pci_bus_id", "")).lower()
        out[h] = bdf.get(b, h)
    return out


@needs2
@pytest.mark.parametrize("mode", ["read", "write"])
def test_p2p_pair_copy(mode):
    from gpu_topology_on_k8s_amd.ops import probe

    n = _ndev()
    assert probe.device_props(0)["pci_bus_id"] != probe.device_props(1)["pci_bus_id"]
    res = {}
    for s in range(n):  # every link of device 0, both directions
        for a, b in ((s, 0), (0, s)):
            if a != b:
                r = probe.copy_bw(a, b, 256 << 20, iters=3, warmup_iters=1, mode=mode)
                assert r["ok"], r
                res[(a, b)] = r["gbps"]
    # absolute floors: half the link's amdsmi-rated per-direction rate AND half the median,
    # so links that all fell to host staging fail even though they match each other
    from gpu_topology_on_k8s_amd.ops.checks import check_pairs, pair_floors

    t = _topo()
    h2t = _hip_to_topo(t)
    rates = {(h2t[a], h2t[b]): v for (a, b), v in res.items()}
    floors = pair_floors(t, rates)
    print(json.dumps({"mode": mode, "amdsmi_max_bw_mbps": t.probe.get("amdsmi_max_bw_mbps"),
                      "pairs": {f"{a}->{b}": [round(v, 1), round(floors[(a, b)], 1)] for (a, b), v in rates.items()}}))
    probs = check_pairs(t, rates)
    assert not probs, probs


@needs2
def test_gather_over_real_peers_beats_one_link():
    from gpu_topology_on_k8s_amd.ops import probe

    from gpu_topology_on_k8s_amd.ops.checks import check_gather

    n = _ndev()
    peers = list(range(1, n))
    single = [probe.copy_bw(s, 0, 64 << 20, iters=3, warmup_iters=1)["gbps"] for s in peers]
    g = probe.gather_bw(0, peers, 64 << 20, iters=3, warmup_iters=1)
    assert g["ok"], g
    print(json.dumps({"gather_gbps": g["gbps"], "single_gbps": single}))
    # all k-1 links at once: at least half of (k-1) x the median single read (a gather that
    # serialises its sources reaches about one link's worth)
    probs = check_gather(g["gbps"], single)
    assert not probs, probs


@needs2
def test_probe_matrix_all_pairs():
    from gpu_topology_on_k8s_amd.ops.probe import probe_topology
    from gpu_topology_on_k8s_amd.topology.discovery import discover

    from gpu_topology_on_k8s_amd.ops.checks import check_pairs, matrix_rates

    t = probe_topology(discover("auto"), preset="quick")
    assert t.probe["device_map"] == "bdf"
    assert "amdsmi_max_bw_mbps" in t.probe  # discovery's rated link rates survive the probe
    probs = check_pairs(t, matrix_rates(t, t.probe["devices"]))
    assert not probs, probs


@needs2
def test_ring_probe_bounded_by_its_links():
    """K6 on the whole node: every member pulling from all the others at once cannot beat the sum of
    its single-pair reads (K1, idle links) and must keep a fair share of it; the bidirectional-ring
    pattern (2 links per member) stays below the all-links pattern."""
    import numpy as np

    from gpu_topology_on_k8s_amd.ops.probe import ingress_bound, measure_ring, probe_topology
    from gpu_topology_on_k8s_amd.topology.discovery import discover

    t = probe_topology(discover("auto"), preset="quick")
    devs = t.probe["devices"]
    r = measure_ring([t.probe["hip_ordinals"][devs.index(d)] for d in devs], "quick")
    pair_sum = ingress_bound(t, devs)
    print(json.dumps({"ring": r, "pair_sum_bound": pair_sum}))
    from gpu_topology_on_k8s_amd.ops.checks import check_ring

    assert pair_sum is not None and np.isfinite(pair_sum)
    probs = check_ring(r["ring_bound_gbps"], pair_sum)  # 0.6x..1.1x the pair-sum bound
    assert not probs, probs
    if len(devs) > 3:
        assert r["ring"]["bound_gbps"] <= 1.05 * r["all"]["bound_gbps"], r


@needs2
def test_bench_two_gpus_native_exact_and_bounded():
    out = _run(["bench.py", "--gpus", "2", "--steps", "5", "--warmup", "2", "--size-mb", "256", "--sweep", "8:64M:64",
                "--ctas", "default", "--full"])
    assert out["n_gpus"] == 2 and out["value_kind"].startswith("aggregate busbw") and out["config"]["backend"] == "native"
    assert out["size_sweep"]["all_exact"]
    assert len(set(out["config"]["hip_devices"])) == 2
    # RCCL's own log: every ring edge rides xGMI peer access (no SHM / host staging, no NET)
    rccl = out["rccl"]
    assert rccl and rccl.get("p2p_only") is True, rccl
    # the K6 ring probe of the same subset (both directions of the link loaded at once) bounds busBW
    # from above and below: a ring that fell back to host staging, or a wrong bus factor, fails
    assert out["probe_bound_kind"] == "k6-ring", (out["probe_bound_kind"], out["ring_probe"])
    bound = out["ring_probe"]["ring_bound_gbps"]
    # the bound is a READ probe (64 MiB); RCCL pushes with writes, which may run somewhat faster
    assert 0.5 * bound <= out["busbw_gbps"] <= 1.5 * bound, (out["busbw_gbps"], bound)
    assert out["phase_s"]["headline"] > 0 and out["skipped_phases"] == []


@needs2
def test_bench_two_gpus_graph_capture():
    out = _run(["bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1", "--size-mb", "16", "--sweep", "8:4K:8",
                "--graph", "on", "--ctas", "default", "--probe", "off", "--full"])
    g = out["graph_latency"]
    assert g and g.get("all_exact"), g


@needs2
def test_bench_two_gpus_ctas_tuning():
    out = _run(["bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1", "--size-mb", "64", "--sweep", "off", "--probe", "off"])
    assert out["ctas_tuning"] and all(r["ms_per_step"] > 0 for r in out["ctas_tuning"])


def _rel(a, b):
    import math

    d = math.sqrt(sum((x - y) ** 2 for x, y in zip(a, b)))
    return d / max(1e-30, math.sqrt(sum(y * y for y in b)))


# different data on every rank, so a reduction that did not run, ran late or ran on
# stale buckets changes the result.  The 2-rank job checks its first reduction against the fp64 sum of
# both ranks' local gradients (--check-reduction; exit 3 on failure) and trains with plain SGD, whose
# update -- unlike AdamW's -- is linear in the averaged gradient: its weight-update fingerprint must
# match a 1-rank job on the concatenated batch (--data-ranks 2).  tests/test_dp_check.py shows on CPU
# that a skipped bucket and a removed wait fail both checks.
DP_CASES = {
    "llama": ["--model", "tiny", "--batch", "2", "--seq", "128", "--bucket-mb", "1"],
    "llama-zero1": ["--model", "tiny", "--batch", "2", "--seq", "128", "--bucket-mb", "1", "--zero1"],
    "llama-fp32": ["--model", "tiny", "--batch", "2", "--seq", "128", "--bucket-mb", "1", "--grad-reduce", "fp32"],
    "mnist": ["--model", "mnist-cnn", "--batch", "64", "--graph", "off", "--dropout", "off"],
    "mnist-graph": ["--model", "mnist-cnn", "--batch", "64", "--graph", "on", "--dropout", "off"],
}
DP_COMMON = ["--steps", "2", "--warmup", "1", "--gemm-tuning", "off", "--optimizer", "sgd", "--lr", "0.5", "--fingerprint"]


@needs2
@pytest.mark.parametrize("case", sorted(DP_CASES))
def test_two_rank_dp_reduction_and_sgd_parity(case):
    args = DP_CASES[case] + DP_COMMON
    one = _run(["-m", "gpu_topology_on_k8s_amd.models.train", *args, "--data-ranks", "2"])
    two = _run(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr=127.0.0.1",
                "--master-port=29611", "-m", "gpu_topology_on_k8s_amd.models.train", *args, "--check-reduction"])
    cr = two["check_reduction"]
    print(json.dumps({"case": case, "check_reduction": cr, "fp_two": two["update_fingerprint"],
                      "fp_one": one["update_fingerprint"]}))
    assert two["n_gpus"] == 2 and cr["ok"] and cr["world"] == 2, cr
    assert cr["mode"] == ("graph-replay" if case.endswith("graph") else "eager")
    assert _rel(two["update_fingerprint"], one["update_fingerprint"]) < 2e-2
    if case.endswith("graph"):
        assert two["graph"]
