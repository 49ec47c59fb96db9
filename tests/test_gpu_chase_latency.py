"""GPU tests of the K8 latency chase (csrc/probe/chase_latency.h and its driver in probe.hip), with
device 0 as both ends: the chain in its own HBM.

The exact tests compare every lane's final node with the pure-Python closed form (ops/chase_ref.py).
The timing tests assert no latency value: only that the numbers are coherent, two orderings the
cache hierarchy gives, and a bracket that catches a loop that was optimised away or a wrong clock rate
(not a performance floor): at least 10 ns per hop, half the ~50 cycles of a dependent LDS read, which
no global load beats; at most 50 us, more than 100 times the ~900 cycles of an idle-chip HBM miss."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_topology_on_k8s_amd.ops.chase_ref import chain_skip, chain_starts

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS_LO, NS_HI = 10.0, 50_000.0


def _ndev() -> int:
    import torch

    return int(torch.cuda.device_count())  # counts without initialising HIP on this image


# (working set, stride): two nodes; 512 nodes a cache line apart; 4096 nodes a page apart
@pytest.mark.parametrize("ws,stride", [(8, 4), (64 << 10, 128), (16 << 20, 4096)])
def test_every_lane_ends_where_the_closed_form_puts_it(ws, stride):
    from gpu_topology_on_k8s_amd.ops.probe import chase_latency

    n = ws // stride
    for chains in (1, 3, 64):
        starts = chain_starts(n, chains)
        for hops in (1, 7, 8, 4099):  # under, at and over the unroll of 8; 4099 wraps the small cycles
            r = chase_latency(0, 0, ws, stride, hops, chains, iters=2, warmup_iters=1, evict=False)
            what = (ws, stride, chains, hops)
            assert r["ok"] is True, (what, r)
            assert (r["n_nodes"], r["hops"], r["chains"], r["stride"], r["ws_bytes"], r["evicted"]) == \
                (n, hops, chains, stride, ws, False), (what, r)
            # three launches (one warm-up, two timed), each continuing the one before
            want = [chain_skip(s, 3 * hops, n) for s in starts]
            assert list(r["end"]) == want, (what, r["end"], want)
            assert len(r["event_ms"]) == 2 and len(r["kernel_ns"]) == 2


def test_evicted_run_is_exact_too():
    r = _timed(1 << 30, True)
    assert r["ok"] is True and r["evicted"] is True and r["n_nodes"] == (1 << 30) // 128
    assert list(r["end"]) == [chain_skip(0, 6 * 4096, r["n_nodes"])]


def test_argument_checks():
    from gpu_topology_on_k8s_amd.ops.probe import chase_latency

    ok = dict(ws_bytes=64 << 10, stride=128, hops=8, chains=1, iters=1, warmup_iters=0, evict=False)
    assert chase_latency(0, 0, **ok)["ok"] is True
    for bad in (dict(ws_bytes=96 << 10), dict(ws_bytes=3 * 128), dict(stride=96), dict(stride=2), dict(stride=64 << 10),
                dict(ws_bytes=8 << 30), dict(chains=0), dict(chains=65), dict(hops=0), dict(hops=(1 << 18) + 1),
                dict(iters=0), dict(iters=64, warmup_iters=1), dict(warmup_iters=-1)):
        with pytest.raises(ValueError):
            chase_latency(0, 0, **{**ok, **bad})
    # checked before anything is allocated: a 4 GiB chain with a bad lane count is an argument error
    with pytest.raises(ValueError):
        chase_latency(0, 0, ws_bytes=4 << 30, stride=128, hops=8, chains=65)
    for src, dst in ((0, 99), (99, 0), (-1, 0)):
        with pytest.raises(ValueError):
            chase_latency(src, dst, **ok)


@functools.lru_cache(maxsize=None)
def _timed(ws, evict):
    """hops=4096, chains=1, five timed launches; measured once, shared by the timing tests."""
    from gpu_topology_on_k8s_amd.ops.probe import chase_latency

    r = chase_latency(0, 0, ws, 128, 4096, 1, iters=5, warmup_iters=1, evict=evict)
    print(json.dumps({k: r[k] for k in ("ws_bytes", "evicted", "ns_per_hop", "ns_min", "ns_max", "event_ms", "ok")}))
    return r


@pytest.mark.parametrize("ws,evict", [(256 << 10, False), (1 << 30, True)])
def test_timing_is_coherent(ws, evict):
    r = _timed(ws, evict)
    assert r["ok"] is True
    assert r["ns_min"] <= r["ns_per_hop"] <= r["ns_max"]
    assert len(r["kernel_ns"]) == len(r["event_ms"]) == 5
    assert r["ns_per_hop"] == pytest.approx(float(np.median([k / 4096 for k in r["kernel_ns"]])))
    for k_ns, e_ms in zip(r["kernel_ns"], r["event_ms"]):  # the in-kernel interval lies inside the event interval
        assert 0 < k_ns <= e_ms * 1e6, (k_ns, e_ms)
    for k in ("ns_per_hop", "ns_min", "ns_max"):
        assert NS_LO <= r[k] <= NS_HI, (k, r[k])


def test_a_warm_small_set_is_quicker_than_an_evicted_large_one():
    warm, cold = _timed(256 << 10, False), _timed(1 << 30, True)
    assert warm["ns_per_hop"] < cold["ns_per_hop"], (warm["ns_per_hop"], cold["ns_per_hop"])


def test_measure_latency_fills_the_model_as_data_only():
    from gpu_topology_on_k8s_amd.ops import probe
    from gpu_topology_on_k8s_amd.topology.codec import decode_v2, encode_v2
    from gpu_topology_on_k8s_amd.topology.discovery import DiscoveryError, discover, fake_topology

    ndev = probe.device_count()
    try:
        topo = discover("auto")
    except DiscoveryError:
        topo = fake_topology(ndev)
    topo.probe = dict(topo.probe, kept="yes")
    cost = topo.cost.copy()
    bw = None if topo.bw_gbps is None else topo.bw_gbps.copy()
    dmap = probe._device_map(topo, None)
    visible = dmap.visible_indices()
    rows = probe.measure_latency(topo, list(range(topo.n)))
    assert rows is not None and topo.probe["latency_us"] == rows and topo.probe["kept"] == "yes"
    assert len(rows) == topo.n and all(len(r) == topo.n for r in rows)
    for d in visible:
        assert rows[d][d] is not None and math.isfinite(rows[d][d])
        assert NS_LO / 1e3 <= rows[d][d] <= NS_HI / 1e3
    if ndev == 1:  # nothing to read over a link: every other entry stays unmeasured
        assert all(rows[i][j] is None for i in range(topo.n) for j in range(topo.n) if i != j)
    for i in range(topo.n):
        for j in range(topo.n):
            if i not in visible or j not in visible:
                assert rows[i][j] is None
    meta = topo.probe["latency_meta"]
    assert (meta["hops"], meta["stride"], meta["ws"], meta["preset"]) == (4096, 128, 1 << 30, "quick") and meta["seconds"] > 0
    # data only
    assert topo.cost.tobytes() == cost.tobytes()
    assert (topo.bw_gbps is None) if bw is None else np.array_equal(topo.bw_gbps, bw, equal_nan=True)
    back = decode_v2(json.loads(json.dumps(encode_v2(topo))))
    for i in range(topo.n):
        for j in range(topo.n):
            assert back.probe["latency_us"][i][j] == (None if rows[i][j] is None else float(np.float16(rows[i][j])))
    assert back.probe["latency_meta"] == meta
    assert np.array_equal(np.round(back.cost, 6), np.round(topo.cost, 6))


def test_latency_cli():
    """``gtk latency`` in a child process: one JSON line, exact, exit status 0."""
    p = subprocess.run([sys.executable, "-m", "gpu_topology_on_k8s_amd", "latency", "--src", "0", "--dst", "0", "--ws", "1048576",
                        "--hops", "4096"], capture_output=True, text=True, timeout=120, cwd=REPO)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["ok"] is True and r["ws_bytes"] == 1048576 and r["hops"] == 4096 and r["chains"] == 1 and r["evicted"] is True
    assert r["end"] == [chain_skip(0, 6 * 4096, 1048576 // 128)]
    assert NS_LO <= r["ns_per_hop"] <= NS_HI


@pytest.mark.skipif(_ndev() < 2, reason="needs >= 2 visible GPUs (single-GPU box): the xGMI path of K8 is not run")
def test_two_distinct_devices():
    """A peer read crosses the link and then misses the same HBM: exact, and slower than the self path."""
    from gpu_topology_on_k8s_amd.ops.probe import chase_latency

    peer = chase_latency(1, 0, 1 << 30, 128, 4096, 1, iters=5, warmup_iters=1, evict=True)
    own = _timed(1 << 30, True)
    assert peer["ok"] is True and list(peer["end"]) == list(own["end"])
    assert NS_LO <= peer["ns_per_hop"] <= NS_HI
    assert peer["ns_per_hop"] > own["ns_per_hop"], (peer["ns_per_hop"], own["ns_per_hop"])
