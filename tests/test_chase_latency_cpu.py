"""CPU checks of the K8 latency chase: the chain's pure-Python reference, the wire codec's ``latency_us``
matrix, the ``gtk latency`` command line, and the ISA of ``chase_kernel`` (hipcc cross-compiles gfx950):
vector loads, no scratch, and the second clock read after the wait for the last load."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

from gpu_topology_on_k8s_amd.ops.chase_ref import CHAIN_A, CHAIN_C, chain_next, chain_skip, chain_starts  # noqa: E402
from gpu_topology_on_k8s_amd.topology import fixtures as fx  # noqa: E402
from gpu_topology_on_k8s_amd.topology.codec import decode_v2, encode_v2  # noqa: E402
from gpu_topology_on_k8s_amd.topology.model import Topology  # noqa: E402


# ---------------------------------------------------------------------------------------- reference
def test_constants_meet_hull_dobell():
    assert (CHAIN_A, CHAIN_C) == (1664525, 1013904223)
    assert CHAIN_C % 2 == 1 and CHAIN_A % 4 == 1


def test_chain_is_one_cycle_through_every_node():
    for k in range(1, 17):
        n = 1 << k
        seen = np.zeros(n, dtype=bool)
        i = 0
        for _ in range(n):
            assert not seen[i], (n, i)
            seen[i] = True
            i = chain_next(i, n)
        assert i == 0 and seen.all(), n


def test_skip_equals_the_plain_walk():
    n = 1 << 23
    for start in (0, 5, n - 1):
        i = start
        for hops in range(2001):
            assert chain_skip(start, hops, n) == i, (start, hops)
            i = chain_next(i, n)
    assert chain_skip(3, n, n) == 3  # a whole lap
    assert chain_skip(3, 5 * n + 7, n) == chain_skip(3, 7, n)


def test_starts_spread_the_lanes_evenly_over_the_cycle():
    for n in (2, 8, 512, 1 << 23):
        for chains in (1, 2, 3, 7, 64):
            want = []
            for lane in range(chains):
                i = 0
                if n <= 512:
                    for _ in range((lane * n) // chains):
                        i = chain_next(i, n)
                else:
                    i = chain_skip(0, (lane * n) // chains, n)
                want.append(i)
            assert chain_starts(n, chains) == want, (n, chains)
    assert chain_starts(1 << 20, 1) == [0]
    s = chain_starts(1 << 20, 64)
    assert len(set(s)) == 64


def test_reference_rejects_what_is_not_a_power_of_two():
    for bad in (0, 1, 3, 6, 1000):
        with pytest.raises(ValueError):
            chain_next(0, bad)
        with pytest.raises(ValueError):
            chain_skip(0, 1, bad)
        with pytest.raises(ValueError):
            chain_starts(bad, 1)
    with pytest.raises(ValueError):
        chain_starts(8, 0)


# -------------------------------------------------------------------------------------------- codec
def _latency_rows(n):
    rng = np.random.default_rng(11)
    rows = [[round(float(v), 4) for v in row] for row in rng.uniform(0.3, 3.0, (n, n))]
    rows[0][1] = rows[3][2] = rows[n - 1][n - 1] = None
    rows[1][1] = 0.7312  # not a float16 value: comes back rounded
    return rows


def _without_latency():
    return fx.f7_degraded()


def _with_latency():
    t = fx.f7_degraded()
    t.probe = dict(t.probe, latency_us=_latency_rows(t.n), latency_meta={"hops": 4096, "stride": 128, "ws": 1 << 30,
                                                                         "preset": "quick", "seconds": 1.5})
    return t


def test_latency_survives_the_wire_codec():
    t = _with_latency()
    rows = t.probe["latency_us"]
    cost_before = t.cost.copy()
    d = json.loads(json.dumps(encode_v2(t)))  # through JSON text, as the annotation travels
    assert "latency_us" in d["m"] and d["m"]["latency_us"].startswith("f16:")
    assert "latency_us" not in d["probe"]  # packed once, not carried twice
    back = decode_v2(d)
    got = back.probe["latency_us"]
    assert len(got) == t.n and all(len(r) == t.n for r in got)
    holes = 0
    for i in range(t.n):
        for j in range(t.n):
            if rows[i][j] is None:
                assert got[i][j] is None, (i, j)
                holes += 1
            else:
                assert got[i][j] == float(np.float16(rows[i][j])), (i, j)
    assert holes == 3
    assert back.probe["latency_meta"] == t.probe["latency_meta"]
    assert back.probe["method"] == "fixture"  # nothing else of the probe is dropped
    # latency is data only: the cost matrix is bit-identical before, after and across the wire
    assert np.array_equal(t.cost, cost_before)
    assert back.cost.tobytes() == t.cost.tobytes()
    assert back.cost.tobytes() == decode_v2(encode_v2(_without_latency())).cost.tobytes()
    assert Topology.from_json(t.to_wire()).probe["latency_us"] == got


def test_a_topology_without_latency_encodes_as_before():
    text = json.dumps(encode_v2(_without_latency()))
    assert "latency" not in text
    d = encode_v2(_with_latency())
    # and the latency adds its own key and nothing else
    d["m"].pop("latency_us")
    d["probe"].pop("latency_meta")
    assert json.dumps(d) == text


def test_latency_round_trips_through_readable_json():
    t = _with_latency()
    back = Topology.from_json(t.to_json())
    assert back.probe["latency_us"] == t.probe["latency_us"]  # v1 JSON carries the rows as they are
    assert back.probe["latency_meta"] == t.probe["latency_meta"]
    assert np.array_equal(back.cost, np.round(t.cost, 6))
    plain = Topology.from_json(_without_latency().to_json())
    assert "latency_us" not in plain.probe and "latency_us" not in _without_latency().to_json()


# ---------------------------------------------------------------------------------------------- CLI
_RUN_MAIN = ("import sys; from gpu_topology_on_k8s_amd.cli import main; rc = main(sys.argv[1:]); "
             "print('PROBE_LOADED' if any(m.endswith('._probe') for m in sys.modules) else 'PROBE_NOT_LOADED'); sys.exit(rc)")


def _gtk(*args):
    return subprocess.run([sys.executable, "-c", _RUN_MAIN, *args], capture_output=True, text=True, cwd=REPO, timeout=120)


def test_latency_command_parses_its_arguments():
    from gpu_topology_on_k8s_amd import cli

    seen = {}
    ap_args = ["latency", "--src", "1", "--dst", "0", "--ws", "1048576", "--stride", "256", "--hops", "77", "--chains", "3",
               "--no-evict"]

    def fake(a):
        seen.update(vars(a))
        return 0

    orig = cli.cmd_latency
    cli.cmd_latency = fake  # main() looks the handler up when it builds the parser
    try:
        assert cli.main(ap_args) == 0
    finally:
        cli.cmd_latency = orig
    assert (seen["src"], seen["dst"], seen["ws"], seen["stride"], seen["hops"], seen["chains"], seen["no_evict"]) == \
        (1, 0, 1048576, 256, 77, 3, True)
    seen.clear()
    cli.cmd_latency = fake
    try:
        assert cli.main(["latency", "--src", "0", "--dst", "0"]) == 0
    finally:
        cli.cmd_latency = orig
    assert (seen["ws"], seen["stride"], seen["hops"], seen["chains"], seen["no_evict"]) == (1 << 30, 128, 4096, 1, False)


@pytest.mark.parametrize("bad", [["--ws", "1000000"], ["--ws", str(3 << 20)], ["--stride", "96"], ["--stride", "2"],
                                 ["--chains", "65"], ["--chains", "0"], ["--hops", "0"], ["--hops", str((1 << 18) + 1)],
                                 ["--ws", str(8 << 30)], ["--iters", "64", "--warmup", "1"]])
def test_latency_command_rejects_bad_arguments_before_loading_the_probe(bad):
    p = _gtk("latency", "--src", "0", "--dst", "0", *bad)
    assert p.returncode == 2, (p.stdout, p.stderr)
    assert "PROBE_NOT_LOADED" in p.stdout and "gtk latency:" in p.stderr
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


def test_latency_command_needs_both_ends():
    assert _gtk("latency", "--src", "0").returncode == 2


def test_probe_command_takes_the_latency_stage():
    p = _gtk("probe", "--latency", "--bogus")
    assert p.returncode == 2 and "unrecognized arguments: --bogus" in p.stderr, p.stderr


# ---------------------------------------------------------------------------------------------- ISA
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


@pytest.fixture(scope="module")
def chase_isa(tmp_path_factory):
    import isa

    out = tmp_path_factory.mktemp("isa") / "probe.s"
    st = isa.kernel_stats(os.path.join(REPO, "csrc", "probe", "probe.hip"), target="_probe", out=str(out))
    names = [k for k in st if "chase_kernel" in k]
    assert len(names) == 1, list(st)
    text = out.read_text()
    m = re.search(rf"^{re.escape(names[0])}:[^\n]*$(.*?)^\s*\.size\s+{re.escape(names[0])},", text, re.S | re.M)
    body = [ln.strip() for ln in m.group(1).splitlines()]
    return st, names[0], [ln for ln in body if ln and not ln.startswith((";", "."))]


@needs_hipcc
def test_chase_kernel_walks_with_vector_loads_and_no_scratch(chase_isa):
    st, name, _ = chase_isa
    v = st[name]
    assert v["ScratchSize"] == 0 and v["scratch"] == 0, v
    # the unrolled chain; a chain the compiler moved to the scalar cache has none of these
    assert v["global_load"] >= 8, v
    fill = [k for k in st if "chase_fill_kernel" in k]
    assert len(fill) == 1 and st[fill[0]]["ScratchSize"] == 0
    # existing keys of kernel_stats are still there
    assert {"mfma", "ds_read", "s_waitcnt", "total", "NumVgprs", "s_load"} <= set(v)


@needs_hipcc
def test_chain_loads_are_plain_and_masked(chase_isa):
    _, _, ins = chase_isa
    loads = [ln for ln in ins if ln.startswith("global_load")]
    for ln in loads:  # no cache-policy bits: the loads ordinary code issues
        assert not re.search(r"\b(nt|sc0|sc1|glc|slc)\b", ln), ln
    # one mask per load: of the lane's start and of every hop
    assert sum(ln.startswith("v_and_b32") for ln in ins) >= len(loads) >= 10, ins


@needs_hipcc
def test_second_clock_read_waits_for_the_last_load(chase_isa):
    _, _, ins = chase_isa
    clocks = [i for i, ln in enumerate(ins) if ln.startswith("s_memrealtime")]
    assert len(clocks) == 2, ins
    before = [ln for ln in ins[:clocks[-1]] if ln.startswith("global_load") or ln.startswith("s_waitcnt vmcnt(0)")]
    assert before and before[-1].startswith("s_waitcnt vmcnt(0)"), before[-3:]
    # and the first one is read after the load of the lane's start and before the chain's first load
    loads = [i for i, ln in enumerate(ins) if ln.startswith("global_load")]
    assert loads[0] < clocks[0] < loads[1], ins
