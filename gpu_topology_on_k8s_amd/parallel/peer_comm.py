"""Peer communicator: the protocol of the K7 collectives with one rank per process, on its host backend.

Every rank owns a *window* (inputs) and an *out* buffer (results) and reads its peers'.  The phases are
K7's (``csrc/probe/peer_allreduce.h``): a rank reads every window, sums in fp32 in rank order, scales,
rounds once and writes its own out, so every rank holds the same bits and ``ops/peer_ref.py``
reproduces them.

Cross-rank ordering is **host-side only**: ``synchronize()`` of the rank's stream, then a counting
barrier on a c10d-style store, with a timeout.  It is the cross-process form of K7's stream events.
No GPU code ever waits on another rank, so a dead rank can never hang a GPU: the others time out on
the host (``PeerCommTimeout``).  Every collective is

    barrier A -> phase 1 -> synchronize -> barrier B (-> phase 2 -> synchronize, for two-shot)

and never more than those two barriers.  The price is that every collective is host-synchronous: two
store round trips and two (two-shot: three) stream synchronisations per call.

Only ``backend="host"`` exists so far: numpy buffers shared between threads of one process, the phases
computed by ``ops/peer_ref.py``, every access logged; two ranks touching overlapping vectors of one
buffer inside the same barrier epoch, one of them writing, is a *conflict*.  That is the protocol's
race detector, and it runs on the CPU.  The native backend (buffers exported by HIP IPC handle and
mapped by every other rank, the K7 kernels on the mappings) is not part of the package: two ranks that
mapped each other's buffers at the same time did not return from ``hipIpcOpenMemHandle``, and the
cause has not been found.
"""
from __future__ import annotations

import datetime
import json
import threading
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..ops.peer_ref import allreduce_ref, bf16_round, peer_slices

__all__ = ["PeerComm", "PeerCommError", "PeerCommTimeout", "PeerCommMismatch", "HostFabric", "MemoryStore",
           "selftest_cases", "case_input", "run_case", "MAX_WORLD"]

MAX_WORLD = 16  # kMaxSrc of probe.hip
_ELEM = {"bf16": 2, "fp32": 4}
_NP = {"bf16": np.uint16, "fp32": np.float32}
ALGOS = ("oneshot", "twoshot")


class PeerCommError(RuntimeError):
    pass


class PeerCommTimeout(PeerCommError):
    """A barrier did not fill within ``timeout_s``: some rank is late or dead.  The comm is broken."""


class PeerCommMismatch(PeerCommError):
    """The ranks entered one collective with different arguments; raised on every rank, before any launch."""


def _out_dtype(dtype: str, out_dtype: Optional[str]) -> str:
    if dtype not in _ELEM:
        raise ValueError(f"dtype must be bf16|fp32, got {dtype!r}")
    out = dtype if out_dtype is None else out_dtype
    if out not in _ELEM:
        raise ValueError(f"out_dtype must be bf16|fp32, got {out!r}")
    if dtype == "fp32" and out == "bf16":
        raise ValueError("fp32 inputs reduce to fp32 only")
    return out


def _n_vec(count: int, dtype: str) -> int:
    return -(-int(count) * _ELEM[dtype] // 16)


class MemoryStore:
    """The c10d Store's ``set`` / ``get`` / ``add`` / ``wait`` for ranks that are threads of one process."""

    def __init__(self, timeout_s: float = 30.0):
        self._d: Dict[str, bytes] = {}
        self._cv = threading.Condition()
        self._timeout = timeout_s
        self.ops = {"set": 0, "get": 0, "add": 0, "wait": 0, "delete_key": 0}

    def set(self, key: str, value) -> None:
        with self._cv:
            self.ops["set"] += 1
            self._d[key] = value if isinstance(value, bytes) else str(value).encode()
            self._cv.notify_all()

    def add(self, key: str, amount: int) -> int:
        with self._cv:
            self.ops["add"] += 1
            n = int(self._d.get(key, b"0")) + int(amount)
            self._d[key] = str(n).encode()
            self._cv.notify_all()
            return n

    def wait(self, keys: Sequence[str], timeout: Optional[datetime.timedelta] = None) -> None:
        limit = self._timeout if timeout is None else timeout.total_seconds()
        with self._cv:
            self.ops["wait"] += 1
            if not self._cv.wait_for(lambda: all(k in self._d for k in keys), limit):
                raise TimeoutError(f"store keys {list(keys)} not set within {limit:.1f}s")

    def delete_key(self, key: str) -> bool:
        with self._cv:
            self.ops["delete_key"] += 1
            return self._d.pop(key, None) is not None

    def num_keys(self) -> int:
        with self._cv:
            return len(self._d)

    def get(self, key: str) -> bytes:
        self.wait([key])
        with self._cv:
            self.ops["get"] += 1
            return self._d[key]


class HostFabric:
    """The buffers of ``backend="host"`` (one window and one out per rank, shared by the ranks'
    threads) and the access log the conflict check reads."""

    def __init__(self, world: int, capacity_bytes: int):
        self.world, self.capacity_bytes = world, capacity_bytes
        self.window = [np.zeros(capacity_bytes, np.uint8) for _ in range(world)]
        self.out = [np.zeros(2 * capacity_bytes, np.uint8) for _ in range(world)]
        self.lock = threading.Lock()
        #: (accessor, owner, buffer, v0, v1, "r" | "w", the accessor's barrier count)
        self.log: List[Tuple[int, int, str, int, int, str, int]] = []
        self.launches = 0

    def access(self, accessor: int, owner: int, buf: str, v0: int, v1: int, mode: str, epoch: int) -> None:
        if v1 > v0:
            with self.lock:
                self.log.append((accessor, owner, buf, v0, v1, mode, epoch))

    def conflicts(self) -> List[Tuple[tuple, tuple]]:
        """Pairs of logged accesses by two ranks to overlapping vectors of one buffer inside the same
        barrier epoch, at least one a write.  Accesses of different epochs are ordered by a barrier."""
        groups: Dict[Tuple[int, str, int], List[tuple]] = {}
        for a in self.log:
            groups.setdefault((a[1], a[2], a[6]), []).append(a)
        found = []
        for accs in groups.values():
            writes = [a for a in accs if a[5] == "w"]
            for w in writes:
                for a in accs:
                    if a[0] != w[0] and a[3] < w[4] and w[3] < a[4] and (a[5] == "r" or a[0] > w[0]):
                        found.append((w, a))
        return found


class _HostBackend:
    """One rank's phase calls (reduce, gather, gather_windows, host copies) on a :class:`HostFabric`,
    computed by ``ops/peer_ref.py``."""

    def __init__(self, rank: int, world: int, fabric: HostFabric):
        self.rank, self.world, self.f = rank, world, fabric
        self.epoch = 0  # barriers this rank has passed; PeerComm._barrier advances it

    def _win(self, p: int, v0: int, v1: int, mode: str) -> np.ndarray:
        self.f.access(self.rank, p, "window", v0, v1, mode, self.epoch)
        return self.f.window[p][v0 * 16:v1 * 16]

    def _out(self, p: int, v0: int, v1: int, mode: str) -> np.ndarray:
        self.f.access(self.rank, p, "out", v0, v1, mode, self.epoch)
        return self.f.out[p][v0 * 16:v1 * 16]

    def open_peers(self) -> None:
        pass

    def close_peers(self) -> None:
        pass

    def synchronize(self) -> None:
        pass

    def reduce(self, v0: int, v1: int, in_dtype: str, out_dtype: str, scale: float) -> None:
        with self.f.lock:
            self.f.launches += 1
        if v0 == v1:
            return
        xs = [self._win(p, v0, v1, "r").view(_NP[in_dtype]).copy() for p in range(self.world)]
        ratio = _ELEM[out_dtype] // _ELEM[in_dtype]
        self._out(self.rank, v0 * ratio, v1 * ratio, "w")[:] = allreduce_ref(xs, in_dtype, out_dtype, scale).view(np.uint8)

    def gather(self, slices: Sequence[Tuple[int, int]]) -> None:
        with self.f.lock:
            self.f.launches += 1
        for p, (a, b) in enumerate(slices):
            if p != self.rank and b > a:
                self._out(self.rank, a, b, "w")[:] = self._out(p, a, b, "r").copy()

    def gather_windows(self, n_vec: int) -> None:
        with self.f.lock:
            self.f.launches += 1
        for p in range(self.world):
            if n_vec:
                self._out(self.rank, p * n_vec, (p + 1) * n_vec, "w")[:] = self._win(p, p * n_vec, (p + 1) * n_vec, "r").copy()

    def write_host(self, a: np.ndarray, first_byte: int = 0) -> None:
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        padded = -(-raw.size // 16) * 16
        w = self._win(self.rank, first_byte // 16, (first_byte + padded) // 16, "w")
        w[:raw.size] = raw
        w[raw.size:] = 0

    def read_host(self, first: int, n: int, dtype: str) -> np.ndarray:
        e = _ELEM[dtype]
        self.f.access(self.rank, self.rank, "out", first * e // 16, -(-(first + n) * e // 16), "r", self.epoch)
        return self.f.out[self.rank][first * e:(first + n) * e].view(_NP[dtype]).copy()


class PeerComm:
    """One rank of a ``world``-rank communicator on HIP device ``device``.

    ``store`` is any object with the c10d Store's ``set``, ``get``, ``add`` and ``wait`` (a
    ``torch.distributed.TCPStore`` between processes, :class:`MemoryStore` between threads); where it
    also has ``delete_key``, the keys of a barrier and of a call's descriptors are deleted two barriers
    later, so the store does not grow with the number of collectives.  Inputs go to the window
    (:meth:`write`), a collective leaves its result in out (:meth:`read`).  Every rank must issue the
    same collectives in the same order; the arguments are compared at the first barrier.  Any store
    error or timeout breaks the comm (``PeerCommTimeout``); later calls then raise at once.
    """

    def __init__(self, rank: int, world: int, device: int, store, capacity_bytes: int, timeout_s: float = 60.0,
                 backend: str = "host", fabric: Optional[HostFabric] = None, prefix: str = "peer_comm"):
        if not 2 <= world <= MAX_WORLD:
            raise ValueError(f"2..{MAX_WORLD} ranks, got {world}")
        if not 0 <= rank < world:
            raise ValueError("rank out of range")
        if capacity_bytes < 16 or capacity_bytes % 16:
            raise ValueError("capacity_bytes must be a positive multiple of 16")
        self.rank, self.world, self.device = rank, world, device
        self.capacity_bytes, self.timeout_s = capacity_bytes, float(timeout_s)
        self._store, self._prefix = store, prefix
        self.barriers = 0       # barriers passed
        self.barrier_s = 0.0    # host time spent in them
        self._seq = 0           # collectives issued
        self.broken = False
        self._closed = False
        self._stale: List[List[str]] = [[], []]  # store keys to delete after the next barrier / the one after
        if backend != "host":
            raise ValueError(f'only backend="host" exists, got {backend!r}')
        if fabric is None:
            raise ValueError('backend="host" shares a HostFabric between the ranks: pass fabric=')
        self._b = _HostBackend(rank, world, fabric)
        self.backend = backend
        self._b.open_peers()  # no barrier: nothing reads a peer before barrier A of the first collective

    # -- the host barrier ---------------------------------------------------------------------
    def _barrier(self) -> None:
        """Counting barrier number ``self.barriers`` on the store: the last rank to arrive sets the
        key the others wait for.  A timeout breaks the comm."""
        t0 = time.perf_counter()
        key = f"{self._prefix}/barrier/{self.barriers}"
        if self.rank == 0:
            self._stale[1] += [key, key + "/full"]

        def arrive():
            if int(self._store.add(key, 1)) == self.world:
                self._store.set(key + "/full", "1")
            else:
                self._store.wait([key + "/full"], datetime.timedelta(seconds=self.timeout_s))

        self._store_call(arrive, f"barrier {self.barriers} did not fill within {self.timeout_s:.1f}s")
        self.barriers += 1
        self._b.epoch = self.barriers
        # A key written before barrier b is last read before its reader arrives at barrier b + 1 (a
        # barrier's own keys: before it arrives at all), so once this rank has passed b + 1 nobody needs it.
        delete = getattr(self._store, "delete_key", None)
        if delete is not None and self._stale[0]:
            self._store_call(lambda: [delete(k) for k in self._stale[0]], "deleting old keys failed")
        self._stale = [self._stale[1], []]
        self.barrier_s += time.perf_counter() - t0

    def _store_call(self, fn, what: str):
        """``fn()``, a store operation; any error or timeout of the store breaks the comm."""
        try:
            return fn()
        except Exception as e:
            self.broken = True
            raise PeerCommTimeout(f"rank {self.rank}: {what} ({type(e).__name__}: {e})") from e

    def _check(self) -> None:
        if self._closed:
            raise PeerCommError("the communicator is closed")
        if self.broken:
            raise PeerCommTimeout(f"rank {self.rank}: the communicator is broken by an earlier barrier timeout")

    def _enter(self, desc: Dict[str, object]) -> None:
        """Barrier A of a collective, carrying the call's descriptor.

        Hazards it covers: every rank's window is written (each rank synchronised its stream before
        it arrived), and last round's readers of my out (phase 2 of a two-shot) are done, so phase 1
        may read any window and overwrite my out."""
        desc = {**desc, "seq": self._seq}
        self._seq += 1
        self._b.synchronize()
        mine = json.dumps(desc, sort_keys=True)
        keys = [f"{self._prefix}/desc/{desc['seq']}/{p}" for p in range(self.world)]
        self._stale[1].append(keys[self.rank])
        self._store_call(lambda: self._store.set(keys[self.rank], mine), "publishing the call descriptor failed")
        self._barrier()
        theirs = self._store_call(lambda: [bytes(self._store.get(k)).decode() for k in keys], "reading the call descriptors failed")
        if any(t != mine for t in theirs):
            raise PeerCommMismatch(f"rank {self.rank}: the ranks disagree on collective {desc['seq']}: " + " | ".join(theirs))

    def _leave(self) -> None:
        """Barrier B.  One-shot, reduce-scatter and all-gather: nobody is still reading any window, so
        the caller may refill its own.  Two-shot: every slice of out that phase 2 is about to read is
        final (and, again, no window is still being read)."""
        self._b.synchronize()
        self._barrier()

    # -- collectives --------------------------------------------------------------------------
    def _reduce_args(self, op: str, count: int, dtype: str, algo: str, out_dtype: Optional[str], scale: float):
        self._check()
        out = _out_dtype(dtype, out_dtype)
        if algo not in ALGOS:
            raise ValueError(f"algo must be oneshot|twoshot, got {algo!r}")
        if count < 1:
            raise ValueError("count >= 1")
        n = _n_vec(count, dtype)
        if n * 16 > self.capacity_bytes:
            raise ValueError(f"{count} {dtype} elements exceed the window of {self.capacity_bytes} bytes")
        scale = float(np.float32(scale))
        return n, out, scale, {"op": op, "count": int(count), "dtype": dtype, "out_dtype": out, "algo": algo, "scale": scale}

    def all_reduce(self, count: int, dtype: str = "bf16", algo: str = "twoshot", out_dtype: Optional[str] = None,
                   scale: float = 1.0) -> None:
        """out[0, count) of every rank = ``scale`` x the sum over ranks of window[0, count), in ``out_dtype``."""
        n, out, scale, desc = self._reduce_args("all_reduce", count, dtype, algo, out_dtype, scale)
        ratio = _ELEM[out] // _ELEM[dtype]
        plan = peer_slices(n, self.world)
        self._enter(desc)
        if algo == "oneshot":
            self._b.reduce(0, n, dtype, out, scale)
            self._leave()
            return
        a, b = plan[self.rank]
        self._b.reduce(a, b, dtype, out, scale)
        self._leave()
        # phase 2 needs no barrier after it: the other ranks may still read my slice of out when I return,
        # and nothing writes my out before barrier A of the next collective
        self._b.gather([(a * ratio, b * ratio) for a, b in plan])
        self._b.synchronize()

    def reduce_scatter(self, count: int, dtype: str = "bf16", out_dtype: Optional[str] = None, scale: float = 1.0) -> Tuple[int, int]:
        """Rank r reduces slice r of ``peer_slices`` only.  Returns the ``(first, n)`` elements of out,
        in ``out_dtype``, that hold this rank's piece (``n`` may be 0)."""
        n, out, scale, desc = self._reduce_args("reduce_scatter", count, dtype, "oneshot", out_dtype, scale)
        a, b = peer_slices(n, self.world)[self.rank]
        self._enter(desc)
        self._b.reduce(a, b, dtype, out, scale)
        self._leave()
        per = 16 // _ELEM[dtype]
        first, end = min(count, a * per), min(count, b * per)
        return first, end - first

    def gather_slot(self, count: int, dtype: str) -> int:
        """Byte offset in the window at which this rank's all-gather contribution of ``count`` elements goes."""
        return self.rank * _n_vec(count, dtype) * 16

    def all_gather(self, count: int, dtype: str = "bf16") -> int:
        """Every rank contributes ``count`` elements, written at :meth:`gather_slot` of its window; rank
        p's land in every rank's out from vector ``p * n_vec`` on.  Returns ``n_vec``, the vectors per rank."""
        self._check()
        if dtype not in _ELEM:
            raise ValueError(f"dtype must be bf16|fp32, got {dtype!r}")
        if count < 1:
            raise ValueError("count >= 1")
        n = _n_vec(count, dtype)
        if n * self.world * 16 > self.capacity_bytes:
            raise ValueError(f"{self.world} x {count} {dtype} elements exceed the window of {self.capacity_bytes} bytes")
        self._enter({"op": "all_gather", "count": int(count), "dtype": dtype, "out_dtype": dtype, "algo": "", "scale": 1.0})
        self._b.gather_windows(n)
        self._leave()
        return n

    # -- data movement ------------------------------------------------------------------------
    def write(self, array: np.ndarray, first_byte: int = 0) -> None:
        """Host array (uint16 bit patterns for bf16, float32) into the window, the last vector's rest zeroed."""
        self._check()
        raw = np.ascontiguousarray(array)
        if first_byte % 16 or first_byte + -(-raw.nbytes // 16) * 16 > self.capacity_bytes:
            raise ValueError("write: past the end of the window, or first_byte is no multiple of 16")
        self._b.write_host(raw, first_byte)

    def read(self, first: int, n: int, dtype: str) -> np.ndarray:
        """Elements ``[first, first + n)`` of out as a host array."""
        self._check()
        if dtype not in _ELEM or first < 0 or n < 0 or (first + n) * _ELEM[dtype] > 2 * self.capacity_bytes:
            raise ValueError("read: bad dtype, or past the end of out")
        return self._b.read_host(first, n, dtype)

    def synchronize(self) -> None:
        self._b.synchronize()

    def close(self) -> None:
        """sync, barrier (nobody still reads a peer), close_peers, barrier (nobody still maps my buffers),
        free; at last the keys this rank still owes the store are deleted.  A broken comm skips the barriers."""
        if self._closed:
            return
        self._closed = True
        try:
            self._b.synchronize()
            if not self.broken:
                self._barrier()
            self._b.close_peers()
            if not self.broken:
                self._barrier()
            delete = getattr(self._store, "delete_key", None)
            if delete is not None and not self.broken and self.rank != 0:  # rank 0's are the last barriers' own keys,
                for k in self._stale[0] + self._stale[1]:                 # which a slower rank may still wait for
                    delete(k)
        except Exception:
            pass
        finally:
            self._b = None


def selftest_counts(k: int) -> List[int]:
    # one element; under one vector; k - 1 bf16 vectors (the last slice is empty); tiles, a tail and
    # padding; and more than one tile for every block
    return [1, 7, 8 * (k - 1), 8 * 1024 * k + 11, (1 << 20) + 4113]


def selftest_cases(k: int, counts: Optional[Sequence[int]] = None) -> List[Dict[str, object]]:
    """Every op, both algorithms, the three dtype pairs (the wide one with ``scale = 1 / k``), at every count."""
    cases: List[Dict[str, object]] = []
    for count in (selftest_counts(k) if counts is None else counts):
        for dtype, out, scale in (("bf16", "bf16", 1.0), ("fp32", "fp32", 1.0), ("bf16", "fp32", 1.0 / k)):
            for algo in ALGOS:
                cases.append({"op": "all_reduce", "count": count, "dtype": dtype, "out_dtype": out, "algo": algo, "scale": scale})
            cases.append({"op": "reduce_scatter", "count": count, "dtype": dtype, "out_dtype": out, "algo": "oneshot", "scale": scale})
        for dtype in ("bf16", "fp32"):
            cases.append({"op": "all_gather", "count": count, "dtype": dtype, "out_dtype": dtype, "algo": "", "scale": 1.0})
    return cases


def case_input(case_index: int, issue: int, rank: int, count: int, dtype: str) -> np.ndarray:
    """Rank ``rank``'s N(0, 1) input of the ``issue``-th issue of case ``case_index``; any rank can make any rank's."""
    rng = np.random.default_rng([case_index, issue, rank, count])
    x = rng.standard_normal(count, dtype=np.float32)
    return bf16_round(x) if dtype == "bf16" else x


def run_case(comm: PeerComm, case: Dict[str, object], inputs: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """Issues one case on ``comm`` with ``inputs[comm.rank]`` as this rank's data; returns (got, reference),
    both computed by this rank, the reference from every rank's input."""
    from ..ops.peer_ref import reduce_scatter_ref

    op, count, dtype, out = case["op"], int(case["count"]), case["dtype"], case["out_dtype"]
    k, r = comm.world, comm.rank
    if op == "all_gather":
        comm.write(inputs[r], comm.gather_slot(count, dtype))
        n = comm.all_gather(count, dtype)
        per = 16 // _ELEM[dtype]
        got = np.concatenate([comm.read(p * n * per, count, dtype) for p in range(k)])
        return got, np.concatenate(list(inputs))
    comm.write(inputs[r])
    if op == "all_reduce":
        comm.all_reduce(count, dtype, case["algo"], out, case["scale"])
        return comm.read(0, count, out), allreduce_ref(inputs, dtype, out, case["scale"])
    first, n = comm.reduce_scatter(count, dtype, out, case["scale"])
    return comm.read(first, n, out), reduce_scatter_ref(inputs, dtype, out, case["scale"])[r]


def _bits(a: np.ndarray) -> np.ndarray:
    return a.view(np.uint16 if a.dtype == np.uint16 else np.uint32)
