"""CPU tests around the peer communicator's device backend (parallel/peer_comm.py): what is refused
before any native module is loaded, the ``validate --ranks`` arguments, and ``run_thread_ranks`` on a
stand-in communicator.  The backend itself runs in tests/test_gpu_peer_comm_device.py."""
import subprocess
import sys
import threading
import time

import pytest

from gpu_topology_on_k8s_amd import cli
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc


def test_device_backend_takes_no_host_fabric():
    with pytest.raises(ValueError, match="HostFabric"):
        pc.PeerComm(0, 2, 0, pc.MemoryStore(), 256, backend="device", fabric=pc.HostFabric(2, 256))


def test_an_unknown_backend_names_both():
    with pytest.raises(ValueError, match=r"host.*device"):
        pc.PeerComm(0, 2, 0, pc.MemoryStore(), 256, backend="process")
    assert pc.BACKENDS == ("host", "device")
    assert {"run_thread_ranks", "selftest", "parked_bytes"} <= set(pc.__all__) and pc.parked_bytes() == 0


def _parse(*argv):
    """The ``validate`` arguments as the CLI parses them, the command itself not run."""
    seen = []
    real = cli.cmd_validate
    cli.cmd_validate = lambda a: seen.append(a) or 0
    try:
        assert cli.main(["validate", "--backend", "peer", "--devices", "0,0", *argv]) == 0
    finally:
        cli.cmd_validate = real
    return seen[0]


def test_ranks_argument(capsys):
    assert _parse().ranks == "driver"
    assert _parse("--ranks", "driver").ranks == "driver"
    assert _parse("--ranks", "thread").ranks == "thread"
    with pytest.raises(SystemExit) as e:
        _parse("--ranks", "process")
    assert e.value.code == 2 and "--ranks" in capsys.readouterr().err


def test_thread_ranks_refuse_large_buffers_before_loading_anything():
    code = ("import sys\n"
            "from gpu_topology_on_k8s_amd import cli\n"
            "try:\n"
            "    cli.main(['validate', '--backend', 'peer', '--ranks', 'thread', '--devices', '0,0', '--max-bytes', str((256 << 20) + 1)])\n"
            "except SystemExit as e:\n"
            "    print('EXIT', e.code)\n"
            "print('NATIVE', sorted(m for m in sys.modules if '_native._' in m or m == 'torch'))\n")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "EXIT --ranks thread" in p.stdout and "256 MiB" in p.stdout and "NATIVE []" in p.stdout, p.stdout
    # at the limit it is the devices' turn: nothing to refuse in the arguments
    assert cli.THREAD_RANKS_MAX_BYTES == 256 << 20
    with pytest.raises(SystemExit, match="--backend peer"):
        cli.main(["validate", "--ranks", "thread", "--devices", "0,0"])


class _StandIn:
    """What ``run_thread_ranks`` needs of a communicator."""

    made, lock = [], threading.Lock()

    def __init__(self, rank, world, device, store, capacity_bytes, timeout_s=60.0, backend="host"):
        self.rank, self.world, self.device, self.store, self.backend = rank, world, device, store, backend
        self.capacity_bytes, self.timeout_s, self.broken, self.closed = capacity_bytes, timeout_s, False, 0
        with self.lock:
            self.made.append(self)

    def close(self):
        self.closed += 1


@pytest.fixture
def stand_ins():
    _StandIn.made = []
    return _StandIn.made


def test_run_thread_ranks_gives_every_rank_its_device_and_closes(stand_ins):
    res = pc.run_thread_ranks([3, 5, 3], lambda c: (c.rank, c.device, threading.current_thread().name), 4096, timeout_s=7.0,
                              comm_cls=_StandIn)
    assert res == [(0, 3, "peer-rank-0"), (1, 5, "peer-rank-1"), (2, 3, "peer-rank-2")]
    assert len(stand_ins) == 3 and all(c.closed == 1 and c.backend == "device" and c.world == 3 for c in stand_ins)
    assert all(c.capacity_bytes == 4096 and c.timeout_s == 7.0 and c.store is stand_ins[0].store for c in stand_ins)
    assert isinstance(stand_ins[0].store, pc.MemoryStore)


def test_run_thread_ranks_joins_and_reraises(stand_ins):
    def body(comm):
        if comm.rank == 1:
            raise KeyError("rank 1 fails")
        return comm.rank

    with pytest.raises(KeyError, match="rank 1 fails"):
        pc.run_thread_ranks([0, 0, 0], body, 4096, comm_cls=_StandIn)
    assert len(stand_ins) == 3 and all(c.closed == 1 for c in stand_ins)  # every rank ran to its end and closed
    assert not [t for t in threading.enumerate() if t.name.startswith("peer-rank-")]


def test_run_thread_ranks_turns_a_join_that_runs_out_into_an_error(stand_ins):
    release = threading.Event()

    def body(comm):
        if comm.rank == 0:
            while not comm.broken and not release.is_set():  # a rank that ends only once its comm is broken
                time.sleep(0.01)
        return comm.rank

    t0 = time.monotonic()
    try:
        with pytest.raises(pc.PeerCommError, match="peer-rank-0"):
            pc.run_thread_ranks([0, 0], body, 4096, timeout_s=1.0, join_s=0.2, comm_cls=_StandIn)
    finally:
        release.set()
    assert time.monotonic() - t0 < 3.0
    assert all(c.broken and c.closed == 1 for c in stand_ins)
    assert not [t for t in threading.enumerate() if t.name.startswith("peer-rank-")]
