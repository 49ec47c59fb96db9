"""Peer communicator: the per-rank protocol of the K7 collectives, on a host and on a device backend.

Every rank owns a *window* (inputs) and an *out* buffer (results) and reads its peers'.  The phases are
K7's (``csrc/probe/peer_allreduce.h``, launched through ``csrc/probe/peer_driver.h``): a rank reads
every window, sums in fp32 in rank order, scales, rounds once and writes its own out, so every rank
holds the same bits and ``ops/peer_ref.py`` reproduces them.

Cross-rank ordering is **host-side only**: ``synchronize()`` of the rank's stream, then a counting
barrier on a c10d-style store, with a timeout.  It is the cross-process form of K7's stream events.
No GPU code ever waits on another rank, so a dead rank can never hang a GPU: the others time out on
the host (``PeerCommTimeout``).  Every collective is

    barrier A -> phase 1 -> synchronize -> barrier B (-> phase 2 -> synchronize, for two-shot)

and never more than those two barriers.  The price is that every collective is host-synchronous: two
store round trips and two (two-shot: three) stream synchronisations per call.

``algo="push"`` (``all_reduce``) is the two-shot without its second phase: rank r sums slice r of every window
and stores the result into slice r of **every** rank's out, its own first and the others in ring order
(``peer_reduce_push_kernel``), so a call is

    barrier A -> push -> synchronize -> barrier B

one launch and two stream synchronisations, with the two-shot's link bytes and the two-shot's bits.  A rank's
out is now written by its peers, between barrier A and barrier B of a push, and that is the one new hazard.
Every reader of that out has synchronised before it entered barrier A: the rank's own ``read``, and a
peer's two-shot phase 2 of the previous collective, which that peer synchronises before it returns.  The
writers of one push never overlap, slice r being rank r's alone.  The pushed slices are final once every rank
has synchronised and passed barrier B, so ``read`` after the call sees them, and the next writer of any out,
whatever the collective, comes after the next barrier A.  On ``wire="fp8"`` the sum reads the packed buffers
and the quantize stays before barrier A; ``wire="fp8x2"`` is refused, a push having no gather phase to pack.

``wire="fp8"`` (``all_reduce``, ``reduce_scatter``) adds a third buffer per rank, *packed*: the rank's
window as e4m3 codes with one power-of-two scale per 32 elements (``csrc/probe/peer_q8.h``,
``ops/peer_ref.q8_quantize_ref``), 33 bytes per 32 elements.  Peers read that instead of the window, and a
rank's own contribution is its packed form too, so every rank still holds the same bits
(``ops/peer_ref.allreduce_q8_ref``).  The quantize reads only the rank's own window and writes only its
own packed buffer, whose last readers finished before the previous collective's barrier B, so it runs
before barrier A and the collective still costs two barriers:

    quantize -> synchronize -> barrier A -> phase 1 on packed -> synchronize -> barrier B (-> phase 2)

Phase 1 works on blocks of 32 elements, sliced by ``q8_slices``; with ``wire="fp8"`` phase 2 of a two-shot is
the same gather of out at the output precision.  Per element and member the packed value is off by at most ``amax / 14``
of its block (``2^(e+4)`` with ``amax * 2^-e > 224``).  The wire fits ``reduce_scatter`` best, where every
byte that crosses a link is packed: the ZeRO-1 gradient path.  Because the quantize comes before the
descriptors are compared, a rank that asks for ``wire="fp8"`` in a mismatched call has made that one
launch, on its own buffers alone, when ``PeerCommMismatch`` is raised; no rank has touched a peer.

``wire="fp8x2"`` (``all_reduce`` with ``algo="twoshot"`` alone: nothing else has a gather phase) packs that
gather too.  Phase 1 packs the scaled fp32 sums of the rank's slice by the same block rule into a fourth
buffer per rank, *packed_out*, and phase 2 unpacks every rank's slice of those buffers, the rank's own
included, into out, so every rank holds the same bits (``ops/peer_ref.allreduce_q8x2_ref``) and both phases
move 33 bytes per 32 elements over the links:

    quantize -> synchronize -> barrier A -> repack -> synchronize -> barrier B -> unpack -> synchronize

Phase 2 cannot read the first packed buffer: that one is rewritten by the next collective's quantize
*before* barrier A, which is safe only because its last readers finish before barrier B, and phase 2 runs
after barrier B.  *packed_out* is written by its owner alone, in phase 1, after barrier A; every rank reads
it in phase 2, after barrier B; and it is next written after the next barrier A, which a rank enters only
after synchronising its own phase 2.  The second rounding costs at most ``amax / 14`` of the block of the
scaled sum per element; an Inf in the sum comes out as NaN, since e4m3fn has no infinity, and a magnitude of
at least ``248 * 2^120`` comes out Inf.

``error_feedback=True`` (``all_reduce`` and ``reduce_scatter`` on ``wire="fp8"`` or ``"fp8x2"``) makes the wire fit
for gradients that keep their value from call to call.  Every rank keeps a *residual*, fp32, one value per
element of its window: what its last packing dropped.  The quantize adds it to the window before it packs
and leaves ``y - dq`` behind (``ops/peer_ref.q8_quantize_ef_ref``), so over any number of calls the sum of what
a rank has sent differs from the sum of what it was given by the last residual alone, at most ``amax / 13`` of
its block; the plain wire's error grows with the number of calls.  The residual is read and written by its
owner alone, in the quantize, before barrier A: it is never published and no peer ever opens it, so no new
hazard exists, and a collective still has two barriers and the same number of launches.  It costs no link
byte.  It is allocated on the first feedback call (twice the window's bytes); a communicator that never asks
for feedback holds none.  Feedback covers the sender's packing only: the second rounding of ``fp8x2``, phase 1
packing the sum again, is the slice owner's and stays in the result.

The residual is positional: value i belongs to element i of the window, whatever the caller put there.  A
caller who changes what the window holds (another tensor, another layout, another count's tail) calls
:meth:`PeerComm.reset_error_feedback` first.  A call with ``error_feedback=False`` neither reads nor writes it.
Because the quantize runs before the descriptors are compared, a mismatched feedback call would have advanced
the residual with data that no one summed: when barrier A of a feedback call raises (``PeerCommMismatch``, or a
timeout), the rank's residual is therefore reset to zero before the exception leaves.

``zero1_step`` is a ZeRO-1 optimizer step as one push (``csrc/probe/peer_zero1.h``).  The optimizer state is split
over the ranks: rank r keeps the fp32 master weights, m and v of slice r of the parameters (:meth:`PeerComm.zero1_init`).
Every rank's window holds the bf16 gradient of all parameters; rank r sums slice r of every window as a push does,
applies AdamW to its state with that sum as the gradient (``ops/peer_ref.zero1_step_ref``) and stores the new bf16
weights into slice r of **every** rank's out:

    (quantize -> synchronize ->) barrier A -> fused launch -> synchronize -> barrier B

one launch and two barriers, where ``reduce_scatter``, an AdamW launch and ``all_gather`` take three launches and four,
write and re-read the fp32 gradient shard and read the new weights once more to gather them.  The hazards are the
push's: out is written by peers between barrier A and barrier B, exactly as in a push, every reader of it having
synchronised before it entered barrier A and the slices of one step never overlapping.  The optimizer state is
touched by its owner alone, in that launch: like the residual it is never published and no peer ever opens it, so it
adds no hazard.  A rank whose slice is empty launches nothing and still takes both barriers.  On ``wire="fp8"`` the
quantize stays before barrier A, with or without error feedback, and the residual is reset when barrier A raises, as
for every feedback call.  All eight hyper-parameters travel in the call's descriptor, so ranks that disagree on one
of them get ``PeerCommMismatch`` before any rank has touched a peer.

``zero1_step(clip_norm=c)`` clips by the global norm, which is the norm of the summed gradient: a sum the fused launch
holds in registers and never writes.  The clipped step splits the launch in two and keeps every gradient byte to one
trip over a link:

    (quantize -> synchronize ->) barrier A -> sum, stash, square -> synchronize -> barrier N -> AdamW from the stash,
    pushed -> synchronize -> barrier B

Launch 1 sums the rank's slice exactly as the fused step does, stores the scaled fp32 sum into a rank-local *stash*
(a fourth array next to master, m and v) and returns the sum of its squares, which the host adds up in float64.
Barrier N carries every rank's value through the store, as barrier A carries the descriptors; every rank adds the k
values in rank order and derives the one factor (``ops/peer_ref.clip_grad_scale``), so all ranks hold the same bits.
Launch 2 reads the stash and the state, rank-local memory only, and pushes the new weights.  Two launches and three
barriers; per element of n on the native wire ``4 + 32 / k`` bytes against the fused step's ``4 + 24 / k``, where a
first pass that read every window again only to square it would move ``6 + 24 / k``.  The stash is its owner's alone,
written between barriers A and N and read between N and B, so it adds no hazard; the windows and packed buffers are
read before barrier N only, every out is written after it only.  It is allocated by the first clipped step after
:meth:`PeerComm.zero1_init`, before barrier A, is scratch and no part of :meth:`PeerComm.zero1_state`.

``zero1_accumulate`` and ``zero1_step(accumulated=True)`` accumulate the gradient of a batch that is split into
micro-batches, in fp32: summing the micro-batches in the bf16 window would round the partial sum after every one.  The
accumulator is the stash, so it is split over the ranks, ``4 n / k`` bytes each, which is ZeRO-2's gradient partition.
Every micro-batch but the last is one call

    (quantize -> synchronize ->) barrier A -> sum, store or add to the stash -> synchronize -> barrier B

after which the windows may be rewritten: one launch, two barriers.  The first call after :meth:`PeerComm.zero1_init`, a
step or :meth:`PeerComm.zero1_reset_accumulated` is launch 1 of the clipped step with its partials ignored, ``acc = piece``;
every later one is the adding launch (``peer_reduce_sqnorm_accum_kernel``, ``peer_q8_sum_sqnorm_accum_kernel``), ``acc =
float32(acc + piece)`` with the piece rounded before the add (``ops/peer_ref.zero1_accumulate_ref``).  The last micro-batch
goes to ``zero1_step(accumulated=True)``: its launch 1 is the adding launch, which stores the total back and squares it, and
its launch 2 the clipped step's.  With ``clip_norm`` that is the clipped step as it stands, three barriers, the norm being
that of the total.  Without it the two launches follow each other on the rank's stream,

    (quantize -> synchronize ->) barrier A -> add to the stash -> AdamW from the stash, pushed -> synchronize -> barrier B

two launches and two barriers: launch 2 reads the rank's own stash and state alone, so only the stream orders it after
launch 1, and every out is written between barriers A and B, as in a push.  Every micro-batch's gradient byte crosses a link
once.  Per element of n and rank on the native wire the first accumulate moves ``2 + 4 / k`` bytes, a later one ``2 + 8 /
k`` and the accumulated step ``4 + 36 / k``, against the clipped step's ``4 + 32 / k``.  The hazards are those above: the
stash is read and written by its owner alone.  What is new is that the stash is **state between calls**: from the first
accumulate to the step that ends the accumulation it holds gradient that exists nowhere else.  So the number of micro-batches
accumulated (:attr:`PeerComm.zero1_accumulated`) travels in the descriptor of every accumulate and every step, and ranks that
disagree get ``PeerCommMismatch`` before any launch; a plain step while something is accumulated is refused, since it would
overwrite the stash (clipped) or leave it behind (fused) and drop gradient silently; :meth:`PeerComm.zero1_init` frees the
stash and with it the accumulation.  The accumulator is no part of :meth:`PeerComm.zero1_state`: checkpoint after a step.

Two backends exist, both with the ranks as threads of one process:

``backend="host"``: numpy buffers, the phases computed by ``ops/peer_ref.py``, every access logged; two
ranks touching overlapping vectors of one buffer inside the same barrier epoch, one of them writing,
is a *conflict*.  That is the protocol's race detector, and it runs on the CPU.

``backend="device"``: every rank has its own device, stream and device buffers (``_probe.PeerRank``,
``csrc/probe/peer_rank.h``) and launches the K7 kernels over its peers' device addresses, which the
ranks publish through the store; across devices the access is ``hipDeviceEnablePeerAccess``, so no IPC
call is made.  A pod gets its GPUs in one container, so one process with a thread per GPU validates an
allocation (:func:`run_thread_ranks`, :func:`selftest`, ``gtk validate --backend peer --ranks thread``).

The process backend (one rank per process, buffers exported by HIP IPC handle and mapped by every other
rank, the K7 kernels on the mappings) is not part of the package: two ranks that mapped each other's
buffers at the same time did not return from ``hipIpcOpenMemHandle``, and the cause has not been found.
It would differ from the device backend in one step, publishing a handle and mapping it where the
device backend publishes an address.
"""
from __future__ import annotations

import datetime
import json
import os
import threading
import time
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..ops.peer_ref import (ELEM as _ELEM, Q8_BLOCK, allreduce_q8_ef_ref, allreduce_q8_ref, allreduce_q8x2_ref, allreduce_ref, bf16_round,
                            bits as _bits, out_dtype_of as _out_dtype, peer_slices, q8_blocks, q8_dequantize_ref, q8_quantize_ef_ref,
                            q8_quantize_ref, q8_slices, reduce_scatter_q8_ef_ref, adamw_ref, bf16_to_f32, zero1_slices, clip_grad_scale,
                            zero1_sqnorm_ref)

__all__ = ["PeerComm", "PeerCommError", "PeerCommTimeout", "PeerCommMismatch", "HostFabric", "MemoryStore",
           "selftest_cases", "selftest_cases_q8", "selftest_cases_q8x2", "selftest_cases_ef", "selftest_cases_push", "case_input", "run_case", "run_thread_ranks", "selftest", "thread_sweep", "timed_all_reduce", "parked_bytes", "zero1_hyper",
           "MAX_WORLD"]

MAX_WORLD = 16  # kMaxSrc of csrc/probe/probe_common.h
BACKENDS = ("host", "device")
_NP = {"bf16": np.uint16, "fp32": np.float32}
ALGOS = ("oneshot", "twoshot")
PUSH = "push"  # all_reduce alone, opt-in: rank r stores slice r of the sum into every rank's out
WIRES = (None, "native", "fp8", "fp8x2")  # None and "native" are the same call: the windows as they are
_WIRE_REF = {None: allreduce_ref, "native": allreduce_ref, "fp8": allreduce_q8_ref, "fp8x2": allreduce_q8x2_ref}
_Q8_BIAS = 127  # a block's stored exponent byte is e + 127, as in csrc/probe/peer_q8.h


class PeerCommError(RuntimeError):
    pass


class PeerCommTimeout(PeerCommError):
    """A barrier did not fill within ``timeout_s``: some rank is late or dead.  The comm is broken."""


class PeerCommMismatch(PeerCommError):
    """The ranks entered one collective with different arguments; raised on every rank, before any launch."""


def _n_vec(count: int, dtype: str) -> int:
    return -(-int(count) * _ELEM[dtype] // 16)


def _max_blocks(capacity_bytes: int) -> int:
    """Blocks a rank's packed buffer holds: a window full of bf16."""
    return capacity_bytes // (2 * Q8_BLOCK)


def _packed_bytes(capacity_bytes: int) -> int:
    """Bytes of a rank's packed buffer: 32 code bytes per block, then one exponent byte per block, in vectors."""
    nb = _max_blocks(capacity_bytes)
    return max(16, (2 * nb + -(-nb // 16)) * 16)


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
    """The buffers of ``backend="host"`` (one window, one out and two packed buffers per rank, shared by
    the ranks' threads; a rank's error-feedback residual, float32, made when it first asks for one) and the
    access log the conflict check reads."""

    def __init__(self, world: int, capacity_bytes: int):
        self.world, self.capacity_bytes = world, capacity_bytes
        self.window = [np.zeros(capacity_bytes, np.uint8) for _ in range(world)]
        self.out = [np.zeros(2 * capacity_bytes, np.uint8) for _ in range(world)]
        self.packed = [np.zeros(_packed_bytes(capacity_bytes), np.uint8) for _ in range(world)]
        self.packed_out = [np.zeros(_packed_bytes(capacity_bytes), np.uint8) for _ in range(world)]
        self.residual: List[Optional[np.ndarray]] = [None] * world  # capacity_bytes // 2 floats each, once made
        self.zero1: List[Optional[np.ndarray]] = [None] * world  # a rank's ZeRO-1 state, float32 [3, n]: master, m, v
        self.stash: List[Optional[np.ndarray]] = [None] * world  # a rank's clipped-step stash, float32 [n], once made; logged as row 3
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
    """One rank's phase calls (reduce, reduce_push, quantize, reduce_q8, reduce_q8_push, repack_q8, unpack_q8, gather, gather_windows,
    reduce_adamw_push, reduce_q8_adamw_push, reduce_sqnorm_stash, reduce_q8_sqnorm_stash, reduce_sqnorm_accum,
    reduce_q8_sqnorm_accum, adamw_push, host copies) on a
    :class:`HostFabric`, computed by ``ops/peer_ref.py``."""

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

    def release(self, broken: bool = False) -> None:
        pass

    @property
    def launches(self) -> int:
        return self.f.launches  # of every rank: the fabric counts them together

    def reduce(self, v0: int, v1: int, in_dtype: str, out_dtype: str, scale: float) -> None:
        with self.f.lock:
            self.f.launches += 1
        if v0 == v1:
            return
        xs = [self._win(p, v0, v1, "r").view(_NP[in_dtype]).copy() for p in range(self.world)]
        ratio = _ELEM[out_dtype] // _ELEM[in_dtype]
        self._out(self.rank, v0 * ratio, v1 * ratio, "w")[:] = allreduce_ref(xs, in_dtype, out_dtype, scale).view(np.uint8)

    def reduce_push(self, v0: int, v1: int, in_dtype: str, out_dtype: str, scale: float) -> None:
        with self.f.lock:
            self.f.launches += 1
        if v0 == v1:
            return
        xs = [self._win(p, v0, v1, "r").view(_NP[in_dtype]).copy() for p in range(self.world)]
        ratio = _ELEM[out_dtype] // _ELEM[in_dtype]
        res = allreduce_ref(xs, in_dtype, out_dtype, scale).view(np.uint8)
        for j in range(self.world):  # every owner's out, this rank's first: a peer write is logged like any other
            self._out((self.rank + j) % self.world, v0 * ratio, v1 * ratio, "w")[:] = res

    def _packed(self, p: int, b0: int, b1: int, mode: str, name: str = "packed") -> Tuple[np.ndarray, np.ndarray]:
        """Blocks ``[b0, b1)`` of rank p's packed buffer ``name`` (``packed`` or ``packed_out``): its code bytes and
        its exponent bytes, logged in vectors under that name."""
        nb = _max_blocks(self.f.capacity_bytes)
        buf = getattr(self.f, name)[p]
        self.f.access(self.rank, p, name, 2 * b0, 2 * b1, mode, self.epoch)
        self.f.access(self.rank, p, name, 2 * nb + b0 // 16, 2 * nb + -(-b1 // 16), mode, self.epoch)
        return buf[Q8_BLOCK * b0:Q8_BLOCK * b1], buf[Q8_BLOCK * nb + b0:Q8_BLOCK * nb + b1]

    def _residual(self, first: int, end: int, mode: str) -> np.ndarray:
        """Floats ``[first, end)`` of this rank's own residual, made on first use, logged in vectors."""
        if self.f.residual[self.rank] is None:
            self.f.residual[self.rank] = np.zeros(self.f.capacity_bytes // 2, np.float32)
        self.f.access(self.rank, self.rank, "residual", first * 4 // 16, -(-end * 4 // 16), mode, self.epoch)
        return self.f.residual[self.rank][first:end]

    @property
    def residual_bytes(self) -> int:
        return 0 if self.f.residual[self.rank] is None else 2 * self.f.capacity_bytes

    def reset_residual(self) -> None:
        if self.f.residual[self.rank] is not None:
            self._residual(0, self.f.capacity_bytes // 2, "w")[:] = 0

    def read_residual(self, first: int, n: int) -> np.ndarray:
        if self.f.residual[self.rank] is None:
            return np.zeros(n, np.float32)
        return self._residual(first, first + n, "r").copy()

    def quantize(self, b0: int, b1: int, count: int, in_dtype: str, error_feedback: bool = False) -> None:
        e = _ELEM[in_dtype]
        if b0 > b1 or b1 * Q8_BLOCK * e > self.f.capacity_bytes:
            raise ValueError("quantize: blocks past the end of the window")
        with self.f.lock:
            self.f.launches += 1
        if b0 == b1:
            return
        first = b0 * Q8_BLOCK
        n = max(0, min(int(count), b1 * Q8_BLOCK) - first)  # the elements of the range before the count: no others are read
        x = np.zeros((b1 - b0) * Q8_BLOCK, _NP[in_dtype])
        x[:n] = self._win(self.rank, first * e // 16, -(-(first + n) * e // 16), "r").view(_NP[in_dtype])[:n]
        if error_feedback:
            res = np.zeros(x.size, np.float32)  # past the count the residual is not read, and comes back zero
            res[:n] = self._residual(first, first + n, "r")
            codes, exps, new = q8_quantize_ef_ref(x, in_dtype, res)
            self._residual(first, b1 * Q8_BLOCK, "w")[:] = new
        else:
            codes, exps = q8_quantize_ref(x, in_dtype)
        c, x8 = self._packed(self.rank, b0, b1, "w")
        c[:], x8[:] = codes, (exps + _Q8_BIAS).astype(np.uint8)

    def reduce_q8(self, b0: int, b1: int, out_dtype: str, scale: float) -> None:
        e = _ELEM[out_dtype]
        if b0 > b1 or b1 > _max_blocks(self.f.capacity_bytes) or b1 * Q8_BLOCK * e > 2 * self.f.capacity_bytes:
            raise ValueError("reduce_q8: blocks past the end of the packed buffer or of out")
        with self.f.lock:
            self.f.launches += 1
        if b0 == b1:
            return
        acc = self._sum_q8(b0, b1, scale)
        res = bf16_round(acc) if out_dtype == "bf16" else acc
        self._out(self.rank, b0 * Q8_BLOCK * e // 16, b1 * Q8_BLOCK * e // 16, "w")[:] = res.view(np.uint8)

    def reduce_q8_push(self, b0: int, b1: int, out_dtype: str, scale: float) -> None:
        e = _ELEM[out_dtype]
        if b0 > b1 or b1 > _max_blocks(self.f.capacity_bytes) or b1 * Q8_BLOCK * e > 2 * self.f.capacity_bytes:
            raise ValueError("reduce_q8_push: blocks past the end of the packed buffer or of out")
        with self.f.lock:
            self.f.launches += 1
        if b0 == b1:
            return
        acc = self._sum_q8(b0, b1, scale)
        res = (bf16_round(acc) if out_dtype == "bf16" else acc).view(np.uint8)
        for j in range(self.world):
            self._out((self.rank + j) % self.world, b0 * Q8_BLOCK * e // 16, b1 * Q8_BLOCK * e // 16, "w")[:] = res

    def _sum_q8(self, b0: int, b1: int, scale: float) -> np.ndarray:
        """``scale`` x the fp32 sum in rank order of blocks ``[b0, b1)`` of every rank's packed buffer."""
        xs = []
        for p in range(self.world):
            c, x8 = self._packed(p, b0, b1, "r")
            xs.append(q8_dequantize_ref(c.copy(), x8.astype(np.int32) - _Q8_BIAS))
        return allreduce_ref(xs, "fp32", "fp32", scale)

    # -- the ZeRO-1 step: the state is this rank's own, logged under "zero1" like the residual ------------
    def zero1_alloc(self, n_elems: int) -> None:
        if n_elems % 8 or n_elems > self.f.capacity_bytes // 2:
            raise ValueError("zero1_alloc: whole vectors of 8 elements, at most a window full of bf16")
        self.f.zero1[self.rank] = np.zeros((3, n_elems), np.float32) if n_elems else None
        self.f.stash[self.rank] = None  # it has the state's size: the next clipped step makes a new one

    def _zero1(self, which: int, first: int, end: int, mode: str) -> np.ndarray:
        st = self.f.zero1[self.rank]
        n = 0 if st is None else st.shape[1]
        have = n if which != 3 or self.f.stash[self.rank] is not None else 0
        if which not in (0, 1, 2, 3) or first < 0 or end < first or end > have:
            raise ValueError("zero1 state: which is 0 (master), 1 (m), 2 (v) or 3 (the stash, once a clipped step has made it), "
                             "and the range lies inside it")
        if st is None:
            return np.zeros(0, np.float32)
        self.f.access(self.rank, self.rank, "zero1", (which * n + first) * 4 // 16, -(-(which * n + end) * 4 // 16), mode, self.epoch)
        return self.f.stash[self.rank][first:end] if which == 3 else st[which, first:end]

    @property
    def zero1_bytes(self) -> int:
        st, stash = self.f.zero1[self.rank], self.f.stash[self.rank]
        return (0 if st is None else int(st.nbytes)) + (0 if stash is None else int(stash.nbytes))

    # -- the clipped step: launch 1 fills the rank's own stash, launch 2 reads it and writes every out ------
    def zero1_stash_alloc(self) -> None:
        st = self.f.zero1[self.rank]
        if st is not None and self.f.stash[self.rank] is None:
            self.f.stash[self.rank] = np.zeros(st.shape[1], np.float32)

    def _sqnorm_stash(self, g: np.ndarray) -> float:
        """The scaled gradient sum ``g`` into stash floats ``[0, g.size)``; its sum of squares in float64."""
        self._zero1(3, 0, g.size, "w")[:] = g
        return zero1_sqnorm_ref([g])

    def reduce_sqnorm_stash(self, v0: int, v1: int, scale: float) -> float:
        if v0 > v1 or v1 * 16 > self.f.capacity_bytes or 8 * (v1 - v0) > self._stash_elems():
            raise ValueError("reduce_sqnorm_stash: vectors past the end of the window or of the stash")
        if v0 == v1:
            return 0.0
        with self.f.lock:
            self.f.launches += 1
        xs = [self._win(p, v0, v1, "r").view(np.uint16).copy() for p in range(self.world)]
        return self._sqnorm_stash(allreduce_ref(xs, "bf16", "fp32", scale))

    def reduce_q8_sqnorm_stash(self, b0: int, b1: int, scale: float) -> float:
        if b0 > b1 or b1 > _max_blocks(self.f.capacity_bytes) or Q8_BLOCK * (b1 - b0) > self._stash_elems():
            raise ValueError("reduce_q8_sqnorm_stash: blocks past the end of the packed buffer or of the stash")
        if b0 == b1:
            return 0.0
        with self.f.lock:
            self.f.launches += 1
        return self._sqnorm_stash(self._sum_q8(b0, b1, scale))

    # -- gradient accumulation: the adding form of launch 1 reads the rank's own stash and writes it back ------
    def _sqnorm_accum(self, g: np.ndarray) -> float:
        """The scaled gradient sum ``g`` added, one fp32 add per element, to stash floats ``[0, g.size)``; the sum of
        squares of the totals in float64."""
        with np.errstate(over="ignore", invalid="ignore"):  # Inf and NaN are results here, not faults
            total = (self._zero1(3, 0, g.size, "r") + g).astype(np.float32)
        self._zero1(3, 0, g.size, "w")[:] = total
        return zero1_sqnorm_ref([total])

    def reduce_sqnorm_accum(self, v0: int, v1: int, scale: float) -> float:
        if v0 > v1 or v1 * 16 > self.f.capacity_bytes or 8 * (v1 - v0) > self._stash_elems():
            raise ValueError("reduce_sqnorm_accum: vectors past the end of the window or of the stash")
        if v0 == v1:
            return 0.0
        with self.f.lock:
            self.f.launches += 1
        xs = [self._win(p, v0, v1, "r").view(np.uint16).copy() for p in range(self.world)]
        return self._sqnorm_accum(allreduce_ref(xs, "bf16", "fp32", scale))

    def reduce_q8_sqnorm_accum(self, b0: int, b1: int, scale: float) -> float:
        if b0 > b1 or b1 > _max_blocks(self.f.capacity_bytes) or Q8_BLOCK * (b1 - b0) > self._stash_elems():
            raise ValueError("reduce_q8_sqnorm_accum: blocks past the end of the packed buffer or of the stash")
        if b0 == b1:
            return 0.0
        with self.f.lock:
            self.f.launches += 1
        return self._sqnorm_accum(self._sum_q8(b0, b1, scale))

    def adamw_push(self, v0: int, v1: int, hyper: Sequence[float]) -> None:
        if v0 > v1 or v1 * 16 > self.f.capacity_bytes or 8 * (v1 - v0) > self._stash_elems():
            raise ValueError("adamw_push: vectors past the end of a window's worth of out or of the stash")
        if v0 == v1:
            return
        with self.f.lock:
            self.f.launches += 1
        self._adamw_push(self._zero1(3, 0, 8 * (v1 - v0), "r").copy(), hyper, v0, v1)

    def _stash_elems(self) -> int:
        return 0 if self.f.stash[self.rank] is None else int(self.f.stash[self.rank].size)

    def zero1_write_state(self, which: int, floats: np.ndarray, first: int = 0) -> None:
        a = np.ascontiguousarray(floats, dtype=np.float32).reshape(-1)
        self._zero1(which, first, first + a.size, "w")[:] = a

    def zero1_read_state(self, which: int, first: int, n: int) -> np.ndarray:
        return self._zero1(which, first, first + n, "r").copy()

    def _adamw_push(self, g: np.ndarray, hyper: Sequence[float], v0: int, v1: int) -> None:
        """AdamW on state floats ``[0, g.size)`` with the gradient ``g``; the new weights to vectors ``[v0, v1)`` of
        every owner's out, this rank's first."""
        new = adamw_ref(*(self._zero1(a, 0, g.size, "r") for a in range(3)), g, hyper)
        for a in range(3):
            self._zero1(a, 0, g.size, "w")[:] = new[a]
        for j in range(self.world):
            self._out((self.rank + j) % self.world, v0, v1, "w")[:] = new[3].view(np.uint8)

    def reduce_adamw_push(self, v0: int, v1: int, scale: float, hyper: Sequence[float]) -> None:
        if v0 > v1 or v1 * 16 > self.f.capacity_bytes or 8 * (v1 - v0) > self.zero1_bytes // 12:
            raise ValueError("reduce_adamw_push: vectors past the end of the window or of the state")
        if v0 == v1:
            return
        with self.f.lock:
            self.f.launches += 1
        xs = [self._win(p, v0, v1, "r").view(np.uint16).copy() for p in range(self.world)]
        self._adamw_push(allreduce_ref(xs, "bf16", "fp32", scale), hyper, v0, v1)

    def reduce_q8_adamw_push(self, b0: int, b1: int, scale: float, hyper: Sequence[float]) -> None:
        if b0 > b1 or b1 > _max_blocks(self.f.capacity_bytes) or Q8_BLOCK * (b1 - b0) > self.zero1_bytes // 12:
            raise ValueError("reduce_q8_adamw_push: blocks past the end of the packed buffer or of the state")
        if b0 == b1:
            return
        with self.f.lock:
            self.f.launches += 1
        self._adamw_push(self._sum_q8(b0, b1, scale), hyper, b0 * Q8_BLOCK * 2 // 16, b1 * Q8_BLOCK * 2 // 16)

    def repack_q8(self, b0: int, b1: int, scale: float) -> None:
        if b0 > b1 or b1 > _max_blocks(self.f.capacity_bytes):
            raise ValueError("repack_q8: blocks past the end of the packed buffers")
        with self.f.lock:
            self.f.launches += 1
        if b0 == b1:
            return
        codes, exps = q8_quantize_ref(self._sum_q8(b0, b1, scale), "fp32")
        c, x8 = self._packed(self.rank, b0, b1, "w", "packed_out")
        c[:], x8[:] = codes, (exps + _Q8_BIAS).astype(np.uint8)

    def unpack_q8(self, slices: Sequence[Tuple[int, int]], out_dtype: str) -> None:
        e = _ELEM[out_dtype]
        if any(a > b or b > _max_blocks(self.f.capacity_bytes) or b * Q8_BLOCK * e > 2 * self.f.capacity_bytes for a, b in slices):
            raise ValueError("unpack_q8: blocks past the end of the packed buffers or of out")
        with self.f.lock:
            self.f.launches += 1
        for p, (a, b) in enumerate(slices):
            if b > a:
                c, x8 = self._packed(p, a, b, "r", "packed_out")
                res = q8_dequantize_ref(c.copy(), x8.astype(np.int32) - _Q8_BIAS)
                res = bf16_round(res) if out_dtype == "bf16" else res
                self._out(self.rank, a * Q8_BLOCK * e // 16, b * Q8_BLOCK * e // 16, "w")[:] = res.view(np.uint8)

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


#: ``_probe.PeerRank`` objects of broken communicators, kept alive (see :meth:`_DeviceBackend.release`)
_PARKED: List[object] = []
_PARKED_LOCK = threading.Lock()


def parked_bytes() -> int:
    """Device memory held by ranks of broken ``backend="device"`` communicators that were closed but
    not freed, in bytes (a window, an out of twice its size, two packed buffers and, where the rank had asked
    for error feedback, its residual, and where it had a ZeRO-1 state, that, per rank)."""
    with _PARKED_LOCK:
        return sum(3 * int(r.capacity_bytes) + 2 * int(r.packed_bytes) + int(getattr(r, "residual_bytes", 0))
                   + int(getattr(r, "zero1_bytes", 0)) for r in _PARKED)


class _DeviceBackend:
    """One rank's phase calls on its own device: ``_probe.PeerRank`` holds the window, the out, the two packed
    buffers and the stream, and launches the K7 kernels over the peers' addresses."""

    def __init__(self, rank: int, world: int, device: int, capacity_bytes: int, max_ctas: int = 0):
        from .._native import load

        self.rank, self.world, self.device = rank, world, int(device)
        self.epoch = 0  # kept for PeerComm._barrier; nothing here reads it
        self.r = load("_probe").PeerRank(self.device, rank, world, capacity_bytes, max_ctas=int(max_ctas))

    def record(self) -> Dict[str, int]:
        """What this rank publishes to its peers.  ``pid`` says whose address space the addresses are in."""
        return {"pid": os.getpid(), "device": self.device, "window": int(self.r.window_ptr()), "out": int(self.r.out_ptr()),
                "packed": int(self.r.packed_ptr()), "packed_out": int(self.r.packed_out_ptr())}

    def open_peers(self, records: Sequence[Dict[str, int]]) -> None:
        self.r.open_peers([int(p["device"]) for p in records], [int(p["window"]) for p in records], [int(p["out"]) for p in records],
                          [int(p["packed"]) for p in records], [int(p["packed_out"]) for p in records])

    def close_peers(self) -> None:
        self.r.close_peers()

    def synchronize(self) -> None:
        self.r.synchronize()

    def release(self, broken: bool = False) -> None:
        """Frees the rank's stream and buffers, unless the communicator is broken.  A broken comm skipped
        the barriers of ``close()``, so a peer's kernel may still be reading this rank's window or out,
        and freeing them under it would turn a host timeout into a GPU fault.  The ``PeerRank`` is then
        parked on a module-level list instead, and its memory stays allocated until the process ends
        (:func:`parked_bytes`)."""
        r, self.r = self.r, None
        if r is None:
            return
        if broken:
            with _PARKED_LOCK:
                _PARKED.append(r)
        else:
            r.release()

    @property
    def launches(self) -> int:
        return int(self.r.launches)

    def reduce(self, v0: int, v1: int, in_dtype: str, out_dtype: str, scale: float) -> None:
        self.r.reduce(v0, v1, in_dtype, out_dtype, scale)

    def reduce_push(self, v0: int, v1: int, in_dtype: str, out_dtype: str, scale: float) -> None:
        self.r.reduce_push(v0, v1, in_dtype, out_dtype, scale)

    def quantize(self, b0: int, b1: int, count: int, in_dtype: str, error_feedback: bool = False) -> None:
        self.r.quantize(b0, b1, count, in_dtype, bool(error_feedback))

    @property
    def residual_bytes(self) -> int:
        return int(self.r.residual_bytes)

    def reset_residual(self) -> None:
        self.r.reset_residual()

    def read_residual(self, first: int, n: int) -> np.ndarray:
        return self.r.read_residual(first, n)

    def reduce_q8(self, b0: int, b1: int, out_dtype: str, scale: float) -> None:
        self.r.reduce_q8(b0, b1, out_dtype, scale)

    def reduce_q8_push(self, b0: int, b1: int, out_dtype: str, scale: float) -> None:
        self.r.reduce_q8_push(b0, b1, out_dtype, scale)

    def repack_q8(self, b0: int, b1: int, scale: float) -> None:
        self.r.repack_q8(b0, b1, scale)

    def zero1_alloc(self, n_elems: int) -> None:
        self.r.zero1_alloc(n_elems)

    @property
    def zero1_bytes(self) -> int:
        return int(self.r.zero1_bytes)

    def zero1_write_state(self, which: int, floats: np.ndarray, first: int = 0) -> None:
        self.r.zero1_write_state(which, np.ascontiguousarray(floats, dtype=np.float32).reshape(-1), first)

    def zero1_read_state(self, which: int, first: int, n: int) -> np.ndarray:
        return self.r.zero1_read_state(which, first, n)

    def reduce_adamw_push(self, v0: int, v1: int, scale: float, hyper: Sequence[float]) -> None:
        self.r.reduce_adamw_push(v0, v1, scale, [float(x) for x in hyper])

    def reduce_q8_adamw_push(self, b0: int, b1: int, scale: float, hyper: Sequence[float]) -> None:
        self.r.reduce_q8_adamw_push(b0, b1, scale, [float(x) for x in hyper])

    def zero1_stash_alloc(self) -> None:
        self.r.zero1_stash_alloc()

    def reduce_sqnorm_stash(self, v0: int, v1: int, scale: float) -> float:
        return float(self.r.reduce_sqnorm_stash(v0, v1, scale))

    def reduce_q8_sqnorm_stash(self, b0: int, b1: int, scale: float) -> float:
        return float(self.r.reduce_q8_sqnorm_stash(b0, b1, scale))

    def reduce_sqnorm_accum(self, v0: int, v1: int, scale: float) -> float:
        return float(self.r.reduce_sqnorm_accum(v0, v1, scale))

    def reduce_q8_sqnorm_accum(self, b0: int, b1: int, scale: float) -> float:
        return float(self.r.reduce_q8_sqnorm_accum(b0, b1, scale))

    def adamw_push(self, v0: int, v1: int, hyper: Sequence[float]) -> None:
        self.r.adamw_push(v0, v1, [float(x) for x in hyper])

    def unpack_q8(self, slices: Sequence[Tuple[int, int]], out_dtype: str) -> None:
        self.r.unpack_q8([(int(a), int(b)) for a, b in slices], out_dtype)

    def gather(self, slices: Sequence[Tuple[int, int]]) -> None:
        self.r.gather([(int(a), int(b)) for a, b in slices])

    def gather_windows(self, n_vec: int) -> None:
        self.r.gather_windows(n_vec)

    def write_host(self, a: np.ndarray, first_byte: int = 0) -> None:
        self.r.write_host(np.ascontiguousarray(a).view(np.uint8).reshape(-1), first_byte)

    def read_host(self, first: int, n: int, dtype: str) -> np.ndarray:
        e = _ELEM[dtype]
        return self.r.read_host(first * e, n * e).view(_NP[dtype])


def zero1_hyper(lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int, grad_scale: float = 1.0) -> List[float]:
    """The AdamW kernels' host form of the hyper-parameters of step ``step`` (from 1), as ``models.optim.FlatAdamW`` makes it:
    ``[lr, beta1, beta2, eps, weight_decay, grad_scale, 1 - beta1^step, 1 - beta2^step]``, each rounded to float32."""
    if step < 1:
        raise ValueError("step >= 1")
    return [float(x) for x in np.array([lr, beta1, beta2, eps, weight_decay, grad_scale, 1 - beta1 ** step, 1 - beta2 ** step], np.float32)]


class PeerComm:
    """One rank of a ``world``-rank communicator on HIP device ``device``.

    ``store`` is any object with the c10d Store's ``set``, ``get``, ``add`` and ``wait`` (a
    ``torch.distributed.TCPStore`` between processes, :class:`MemoryStore` between threads); where it
    also has ``delete_key``, the keys of a barrier and of a call's descriptors are deleted two barriers
    later, so the store does not grow with the number of collectives.  Inputs go to the window
    (:meth:`write`), a collective leaves its result in out (:meth:`read`).  Every rank must issue the
    same collectives in the same order; the arguments are compared at the first barrier.  Any store
    error or timeout breaks the comm (``PeerCommTimeout``); later calls then raise at once.

    ``backend="host"`` takes the :class:`HostFabric` the ranks share.  ``backend="device"`` takes none: the
    rank allocates on ``device`` and the constructor exchanges addresses through the store, waiting up to
    ``timeout_s`` for every rank; all ranks must be threads of this process (``PeerCommError`` otherwise).

    ``max_ctas`` (keyword, 0: no cap) bounds the blocks of every reduce, push, quantize, repack and ZeRO-1 launch of
    ``backend="device"``, and with them the CUs the communicator takes from the compute it runs beside.  It changes no
    result bit; only the norm a clipped ``zero1_step`` returns follows the grid's summation order.  The gather and
    unpack launches keep their grids, which must stay a multiple of the source count.  ``backend="host"`` has no grid
    and ignores the value.  Negative: ``ValueError``.
    """

    def __init__(self, rank: int, world: int, device: int, store, capacity_bytes: int, timeout_s: float = 60.0,
                 backend: str = "host", fabric: Optional[HostFabric] = None, prefix: str = "peer_comm", *, max_ctas: int = 0):
        if not 2 <= world <= MAX_WORLD:
            raise ValueError(f"2..{MAX_WORLD} ranks, got {world}")
        if not 0 <= rank < world:
            raise ValueError("rank out of range")
        if capacity_bytes < 16 or capacity_bytes % 16:
            raise ValueError("capacity_bytes must be a positive multiple of 16")
        if int(max_ctas) != max_ctas or max_ctas < 0:
            raise ValueError(f"max_ctas must be an integer >= 0 (0: no cap), got {max_ctas!r}")
        self.rank, self.world, self.device = rank, world, device
        self.max_ctas = int(max_ctas)
        self.capacity_bytes, self.timeout_s = capacity_bytes, float(timeout_s)
        self._store, self._prefix = store, prefix
        self.barriers = 0       # barriers passed
        self.barrier_s = 0.0    # host time spent in them
        self._seq = 0           # collectives issued
        self.broken = False
        self._closed = False
        self._stale: List[List[str]] = [[], []]  # store keys to delete after the next barrier / the one after
        self._zero1: Optional[Tuple[int, Optional[str]]] = None  # (count, wire) of zero1_init
        self._zero1_acc = 0  # micro-batches accumulated in the stash since the last step, reset or init
        if backend not in BACKENDS:
            raise ValueError(f'backend must be "host" or "device", got {backend!r}')
        self.backend = backend
        if backend == "device":
            if fabric is not None:
                raise ValueError('a HostFabric belongs to backend="host": backend="device" allocates on the device')
            self._b = _DeviceBackend(rank, world, device, capacity_bytes, self.max_ctas)
            try:
                self._b.open_peers(self._exchange_pointers())
            except BaseException:
                # no peer can have launched on these buffers: that takes a barrier this rank never joined
                b, self._b = self._b, None
                b.release()
                raise
            return
        if fabric is None:
            raise ValueError('backend="host" shares a HostFabric between the ranks: pass fabric=')
        self._b = _HostBackend(rank, world, fabric)
        self._b.open_peers()  # no barrier: nothing reads a peer before barrier A of the first collective

    def _exchange_pointers(self) -> List[Dict[str, int]]:
        """Publishes this rank's device and buffer addresses and reads every rank's, through the store
        (a process backend would publish an IPC handle here and map what it reads).  No barrier is needed:
        nothing reads a peer before barrier A of the first collective.  The keys are deleted like the
        descriptors', two barriers later, when every rank has long read them."""
        keys = [f"{self._prefix}/ptr/{p}" for p in range(self.world)]
        self._stale[1].append(keys[self.rank])
        mine = json.dumps(self._b.record(), sort_keys=True)
        self._store_call(lambda: self._store.set(keys[self.rank], mine), "publishing the buffer addresses failed")

        def read():
            self._store.wait(keys, datetime.timedelta(seconds=self.timeout_s))
            return [json.loads(bytes(self._store.get(k)).decode()) for k in keys]

        records = self._store_call(read, f"not every rank published its buffers within {self.timeout_s:.1f}s")
        foreign = [p for p, rec in enumerate(records) if rec.get("pid") != os.getpid()]
        if foreign:
            raise PeerCommError(f'rank {self.rank}: backend="device" joins threads of one process, but ranks {foreign} '
                                f"published addresses of another process (this one is {os.getpid()})")
        return records

    @property
    def launches(self) -> int:
        """Kernel launches made so far: this rank's on the device backend, every rank's on the host backend."""
        return self._b.launches

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
        may read any window and overwrite my out, and a push may overwrite its slice of every rank's out:
        the owner's own ``read`` of it is synchronous and lies before the owner's arrival too."""
        desc = {**desc, "seq": self._seq}
        self._seq += 1
        try:
            self._b.synchronize()
            mine = json.dumps(desc, sort_keys=True)
            keys = [f"{self._prefix}/desc/{desc['seq']}/{p}" for p in range(self.world)]
            self._stale[1].append(keys[self.rank])
            self._store_call(lambda: self._store.set(keys[self.rank], mine), "publishing the call descriptor failed")
            self._barrier()
            theirs = self._store_call(lambda: [bytes(self._store.get(k)).decode() for k in keys], "reading the call descriptors failed")
            if any(t != mine for t in theirs):
                raise PeerCommMismatch(f"rank {self.rank}: the ranks disagree on collective {desc['seq']}: " + " | ".join(theirs))
        except BaseException:
            if desc.get("ef"):  # the quantize has advanced the residual with data that no one will sum
                try:
                    self._b.reset_residual()
                except Exception:  # the error that brought us here is the one to report
                    pass
            raise

    def _leave(self) -> None:
        """Barrier B.  One-shot, reduce-scatter and all-gather: nobody is still reading any window, so
        the caller may refill its own.  Two-shot: every slice of out that phase 2 is about to read is
        final (and, again, no window is still being read).  Push and ZeRO-1 step: every rank's stores into
        every out are complete, so each rank may read its own."""
        self._b.synchronize()
        self._barrier()

    # -- collectives --------------------------------------------------------------------------
    def _reduce_args(self, op: str, count: int, dtype: str, algo: str, out_dtype: Optional[str], scale: float,
                     wire: Optional[str] = None, error_feedback: bool = False):
        """The checked arguments of a reduce: its units (vectors of the window; blocks of 32 elements on the
        fp8 wire), the output dtype, the scale as the kernel gets it, and the call's descriptor (``"ef"`` in it
        only when feedback is set, so the descriptors of every other call are what they were)."""
        self._check()
        out = _out_dtype(dtype, out_dtype)
        if algo not in ALGOS and not (algo == PUSH and op == "all_reduce"):
            raise ValueError(f"algo must be oneshot|twoshot|push, got {algo!r}")
        if wire not in WIRES:
            raise ValueError(f'wire must be None, "native", "fp8" or "fp8x2", got {wire!r}')
        if wire == "fp8x2" and (op != "all_reduce" or algo != "twoshot"):
            raise ValueError('wire="fp8x2" packs the gather phase of all_reduce(algo="twoshot"): nothing else has one, '
                             'a push least of all')
        if error_feedback and wire not in ("fp8", "fp8x2"):
            raise ValueError('error_feedback=True belongs to wire="fp8" or "fp8x2": the native wire drops nothing')
        if count < 1:
            raise ValueError("count >= 1")
        scale = float(np.float32(scale))
        desc = {"op": op, "count": int(count), "dtype": dtype, "out_dtype": out, "algo": algo, "scale": scale}
        if wire in ("fp8", "fp8x2"):
            n = q8_blocks(count)
            if n * Q8_BLOCK * _ELEM[dtype] > self.capacity_bytes:
                raise ValueError(f"{count} {dtype} elements, rounded up to blocks of {Q8_BLOCK}, exceed the window of "
                                 f"{self.capacity_bytes} bytes")
            return n, out, scale, {**desc, "wire": wire, **({"ef": True} if error_feedback else {})}
        n = _n_vec(count, dtype)
        if n * 16 > self.capacity_bytes:
            raise ValueError(f"{count} {dtype} elements exceed the window of {self.capacity_bytes} bytes")
        return n, out, scale, desc

    def all_reduce(self, count: int, dtype: str = "bf16", algo: str = "twoshot", out_dtype: Optional[str] = None,
                   scale: float = 1.0, wire: Optional[str] = None, error_feedback: bool = False) -> None:
        """out[0, count) of every rank = ``scale`` x the sum over ranks of window[0, count), in ``out_dtype``.
        ``wire="fp8"``: of the windows' packed forms; ``wire="fp8x2"`` (two-shot only): the same, packed once more
        for the gather (see the module docstring).  ``error_feedback=True`` (those two wires; ``ValueError`` on the
        native one, before any barrier or launch): this rank's residual is added to its window before the packing
        and keeps what the packing dropped.  ``algo="push"``: one launch, this rank's slice of the sum stored into
        every rank's out (native and ``"fp8"`` wires; ``"fp8x2"`` is a ``ValueError`` before any barrier or launch)."""
        n, out, scale, desc = self._reduce_args("all_reduce", count, dtype, algo, out_dtype, scale, wire, error_feedback)
        if wire == "fp8x2":
            plan = q8_slices(n, self.world)
            self._b.quantize(0, n, count, dtype, error_feedback)
            self._enter(desc)
            self._b.repack_q8(*plan[self.rank], scale)
            self._leave()
            # every slice comes from its owner's packed_out, this rank's own too; as below, no barrier after it
            self._b.unpack_q8(plan, out)
            self._b.synchronize()
            return
        if wire == "fp8":
            per = Q8_BLOCK * _ELEM[out] // 16  # output vectors per block
            plan = q8_slices(n, self.world)
            self._b.quantize(0, n, count, dtype, error_feedback)
            self._enter(desc)
            if algo == PUSH:
                self._b.reduce_q8_push(*plan[self.rank], out, scale)
                self._leave()
                return
            a, b = (0, n) if algo == "oneshot" else plan[self.rank]
            self._b.reduce_q8(a, b, out, scale)
            self._leave()
            if algo == "twoshot":  # as below
                self._b.gather([(a * per, b * per) for a, b in plan])
                self._b.synchronize()
            return
        ratio = _ELEM[out] // _ELEM[dtype]
        plan = peer_slices(n, self.world)
        self._enter(desc)
        if algo == "oneshot":
            self._b.reduce(0, n, dtype, out, scale)
            self._leave()
            return
        a, b = plan[self.rank]
        if algo == PUSH:  # my slice of the sum into every rank's out; after barrier B every out is whole
            self._b.reduce_push(a, b, dtype, out, scale)
            self._leave()
            return
        self._b.reduce(a, b, dtype, out, scale)
        self._leave()
        # phase 2 needs no barrier after it: the other ranks may still read my slice of out when I return,
        # and nothing writes my out before barrier A of the next collective
        self._b.gather([(a * ratio, b * ratio) for a, b in plan])
        self._b.synchronize()

    def reduce_scatter(self, count: int, dtype: str = "bf16", out_dtype: Optional[str] = None, scale: float = 1.0,
                       wire: Optional[str] = None, error_feedback: bool = False) -> Tuple[int, int]:
        """Rank r reduces slice r of ``peer_slices`` only (``wire="fp8"``: of ``q8_slices``, over blocks of the
        packed forms).  Returns the ``(first, n)`` elements of out, in ``out_dtype``, that hold this rank's
        piece (``n`` may be 0).  ``error_feedback=True`` (``wire="fp8"`` only): as in :meth:`all_reduce`; every
        rank packs, and feeds back, its whole window."""
        n, out, scale, desc = self._reduce_args("reduce_scatter", count, dtype, "oneshot", out_dtype, scale, wire, error_feedback)
        if wire == "fp8":
            a, b = q8_slices(n, self.world)[self.rank]
            self._b.quantize(0, n, count, dtype, error_feedback)
            self._enter(desc)
            self._b.reduce_q8(a, b, out, scale)
            self._leave()
            first, end = min(count, a * Q8_BLOCK), min(count, b * Q8_BLOCK)
            return first, end - first
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

    # -- the ZeRO-1 step -----------------------------------------------------------------------
    def zero1_init(self, count: int, weights: np.ndarray, wire: Optional[str] = None,
                   state: Optional[Sequence[np.ndarray]] = None) -> Tuple[int, int]:
        """Makes this rank's optimizer state for ``count`` parameters: slice ``self.rank`` of ``zero1_slices`` (whole
        vectors of ``peer_slices`` on the native wire, whole blocks of ``q8_slices`` on ``wire="fp8"``).  ``weights``
        are the bf16 bit patterns (uint16) of all ``count`` parameters: the rank widens its own slice into its fp32
        master and zeroes m and v.  ``state``, what :meth:`zero1_state` returned, restores master, m and v instead.
        Local: no barrier, no peer.  Returns the ``(first, n)`` parameters this rank owns (``n`` may be 0).
        ``ValueError``: ``wire="fp8x2"`` (a push has no gather phase to pack), a count past the window."""
        self._check()
        if wire not in (None, "native", "fp8"):
            raise ValueError(f'zero1: wire must be None, "native" or "fp8", got {wire!r}: a push has no gather phase for "fp8x2" to pack')
        if count < 1:
            raise ValueError("count >= 1")
        units = q8_blocks(count) * Q8_BLOCK if wire == "fp8" else _n_vec(count, "bf16") * 8
        if units * 2 > self.capacity_bytes:
            raise ValueError(f"{count} bf16 elements, in whole units of the wire, exceed the window of {self.capacity_bytes} bytes")
        w = np.ascontiguousarray(weights)
        if w.dtype != np.uint16 or w.shape != (count,):
            raise ValueError("weights: the uint16 bit patterns of all count bf16 parameters")
        a, b = zero1_slices(count, self.world, wire)[self.rank]
        n = b - a
        if state is None:
            master = np.zeros(n, np.float32)
            mine = bf16_to_f32(w[a:min(b, count)])
            master[:mine.size] = mine
            new = (master, None, None)  # zero1_alloc zeroes m and v
        else:
            new = tuple(np.ascontiguousarray(x, dtype=np.float32) for x in state)
            if len(new) != 3 or any(x.shape != (n,) for x in new):
                raise ValueError(f"state: master, m and v, {n} float32 each, as zero1_state returns them")
        self._zero1 = None
        self._zero1_acc = 0  # zero1_alloc frees the stash, and what was accumulated with it
        self._b.zero1_alloc(n)
        for which, x in enumerate(new):
            if x is not None and n:
                self._b.zero1_write_state(which, x, 0)
        self._zero1 = (int(count), wire)
        first, end = min(count, a), min(count, b)
        return first, end - first

    def zero1_state(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """This rank's master, m and v as float32 host arrays, the slice's padding included.  A gradient accumulated by
        :meth:`zero1_accumulate` is no part of it: checkpointing in the middle of an accumulation is out of scope, so
        take the state after a step, when nothing is accumulated."""
        self._check()
        if self._zero1 is None:
            raise ValueError("zero1_state: zero1_init first")
        a, b = zero1_slices(self._zero1[0], self.world, self._zero1[1])[self.rank]
        return tuple(self._b.zero1_read_state(which, 0, b - a) for which in range(3))

    def zero1_step(self, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int, grad_scale: float = 1.0,
                   scale: Optional[float] = None, error_feedback: bool = False, clip_norm: Optional[float] = None,
                   accumulated: bool = False) -> Optional[float]:
        """One AdamW step of the parameters of :meth:`zero1_init`.  Every rank's window holds its bf16 gradient in
        ``[0, count)``; the gradient of the update is ``scale`` (default ``1 / world``: the mean) x the sum over ranks,
        times ``grad_scale``.  ``step`` is the number of this step, from 1; the bias corrections ``1 - beta^step`` are
        computed here, on the host.  Afterwards out[0, count) of **every** rank holds the same new bf16 weights and this
        rank's state is advanced.  One launch, two barriers; returns ``None``.

        ``clip_norm=c`` clips by the global norm (``ops/peer_ref.clip_grad_scale``): the update's ``grad_scale`` becomes
        ``grad_scale * min(1, c / (norm + 1e-6))`` with ``norm = grad_scale * |scale x the sum|`` over all parameters,
        and ``norm`` is returned, the same float on every rank.  ``float("inf")`` measures the norm and never clips.  A
        NaN anywhere in the summed gradient makes every weight NaN; an Inf makes the factor 0.  Two launches, three
        barriers (see the module docstring); the first clipped step after :meth:`zero1_init` allocates the rank's stash.

        ``accumulated=True`` ends a gradient accumulation (:meth:`zero1_accumulate`): the window holds the **last**
        micro-batch, and the gradient of the update is ``grad_scale x float32(acc + scale x the sum over ranks)``, ``acc``
        being what the earlier micro-batches left in the rank's stash.  Launch 1 is the adding launch, which stores the
        total back to the stash and squares it; launch 2 applies AdamW from the stash and pushes.  Without ``clip_norm``
        the two follow each other on the rank's stream, two launches and two barriers; with it the step is the clipped
        one, three barriers, and the norm is that of the accumulated total.  The step ends the accumulation.

        ``ValueError``, before any barrier or launch: no :meth:`zero1_init`; ``error_feedback`` on the native wire;
        ``clip_norm`` that is not above 0 (a NaN is not); ``accumulated=True`` with nothing accumulated;
        ``accumulated=False`` while something is, which would silently drop gradient
        (:meth:`zero1_reset_accumulated` drops it on purpose)."""
        self._check()
        if self._zero1 is None:
            raise ValueError("zero1_step: zero1_init first")
        count, wire = self._zero1
        if error_feedback and wire != "fp8":
            raise ValueError('error_feedback=True belongs to wire="fp8": the native wire drops nothing')
        accumulated = bool(accumulated)
        if accumulated and not self._zero1_acc:
            raise ValueError("zero1_step(accumulated=True): nothing is accumulated, zero1_accumulate first")
        if not accumulated and self._zero1_acc:
            raise ValueError(f"zero1_step(accumulated=False) while {self._zero1_acc} micro-batches are accumulated would drop their "
                             "gradient: pass accumulated=True, or zero1_reset_accumulated() to drop it on purpose")
        if clip_norm is not None:
            clip_norm = float(clip_norm)
            if not clip_norm > 0.0:
                raise ValueError(f"clip_norm must be above 0 (inf: measure the norm, never clip), got {clip_norm!r}")
        scale = float(np.float32(1.0 / self.world if scale is None else scale))
        hyper = zero1_hyper(lr, beta1, beta2, eps, weight_decay, step, grad_scale)
        # the hyper of the descriptor keeps the caller's grad_scale: the clipped one is not known at barrier A
        desc = {"op": "zero1_step", "count": count, "wire": wire or "native", "scale": scale, "ef": bool(error_feedback), "hyper": hyper,
                "clip": clip_norm, "accumulated": accumulated, "micro": self._zero1_acc}
        if clip_norm is not None:
            norm = self._zero1_step_clipped(desc, count, wire, scale, hyper, error_feedback, clip_norm, accumulated)
            self._zero1_acc = 0
            return norm
        if accumulated:
            v0, v1 = self._zero1_sum_to_stash(desc, count, wire, scale, error_feedback, add=True)[:2]
            self._b.adamw_push(v0, v1, hyper)  # the stash is this rank's own: no barrier between the two launches
            self._leave()  # every rank's stores into every out are complete
            self._zero1_acc = 0
            return None
        if wire == "fp8":
            n = q8_blocks(count)
            self._b.quantize(0, n, count, "bf16", error_feedback)
            self._enter(desc)
            self._b.reduce_q8_adamw_push(*q8_slices(n, self.world)[self.rank], scale, hyper)
        else:
            self._enter(desc)
            self._b.reduce_adamw_push(*peer_slices(_n_vec(count, "bf16"), self.world)[self.rank], scale, hyper)
        self._leave()  # every rank's stores into every out are complete
        return None

    def _zero1_sum_to_stash(self, desc: Dict[str, object], count: int, wire: Optional[str], scale: float, error_feedback: bool,
                            add: bool) -> Tuple[int, int, float]:
        """(quantize -> synchronize ->) barrier A -> launch 1: ``scale`` x the sum over ranks of this rank's slice, stored
        to its stash or, with ``add``, added to what the stash holds.  Returns the slice in weight vectors of 8 and the sum
        of squares of what the launch stored (0.0, and no launch, for an empty slice)."""
        self._b.zero1_stash_alloc()  # before barrier A: no allocation inside a barrier epoch
        if wire == "fp8":
            n = q8_blocks(count)
            b0, b1 = q8_slices(n, self.world)[self.rank]
            self._b.quantize(0, n, count, "bf16", error_feedback)
            self._enter(desc)
            mine = (self._b.reduce_q8_sqnorm_accum if add else self._b.reduce_q8_sqnorm_stash)(b0, b1, scale)
            return b0 * Q8_BLOCK // 8, b1 * Q8_BLOCK // 8, mine
        v0, v1 = peer_slices(_n_vec(count, "bf16"), self.world)[self.rank]
        self._enter(desc)
        return v0, v1, (self._b.reduce_sqnorm_accum if add else self._b.reduce_sqnorm_stash)(v0, v1, scale)

    def zero1_accumulate(self, scale: Optional[float] = None, error_feedback: bool = False) -> None:
        """Adds one micro-batch to this rank's gradient accumulator.  Every rank's window holds the micro-batch's bf16
        gradient in ``[0, count)``; rank r adds ``scale`` (default ``1 / world``) x the sum over ranks of slice r to its
        accumulator, fp32, the rank's stash (``ops/peer_ref.zero1_accumulate_ref``).  The first call after
        :meth:`zero1_init`, after a step or after :meth:`zero1_reset_accumulated` stores the piece, every later one adds
        to it with one fp32 add per element.  One launch, two barriers; after the call the window may be rewritten.  The
        last micro-batch is not accumulated but given to ``zero1_step(accumulated=True)``.  A rank whose slice is empty
        launches nothing and takes both barriers.  ``ValueError``, before any barrier or launch: no :meth:`zero1_init`;
        ``error_feedback`` on the native wire."""
        self._check()
        if self._zero1 is None:
            raise ValueError("zero1_accumulate: zero1_init first")
        count, wire = self._zero1
        if error_feedback and wire != "fp8":
            raise ValueError('error_feedback=True belongs to wire="fp8": the native wire drops nothing')
        scale = float(np.float32(1.0 / self.world if scale is None else scale))
        desc = {"op": "zero1_accumulate", "count": count, "wire": wire or "native", "scale": scale, "ef": bool(error_feedback),
                "accumulated": self._zero1_acc}
        self._zero1_sum_to_stash(desc, count, wire, scale, error_feedback, add=self._zero1_acc > 0)
        self._leave()  # nobody is still reading any window
        self._zero1_acc += 1

    @property
    def zero1_accumulated(self) -> int:
        """Micro-batches accumulated since the last step, :meth:`zero1_reset_accumulated` or :meth:`zero1_init`."""
        return self._zero1_acc

    def zero1_reset_accumulated(self) -> None:
        """Drops what is accumulated: the next :meth:`zero1_accumulate` stores again.  Local, no barrier and no launch;
        it serves a skipped step, and every rank must skip alike, the count being part of the next call's descriptor."""
        self._zero1_acc = 0

    def _zero1_step_clipped(self, desc: Dict[str, object], count: int, wire: Optional[str], scale: float, hyper: List[float],
                            error_feedback: bool, clip_norm: float, accumulated: bool = False) -> float:
        """barrier A -> sum, stash, square -> barrier N, carrying every rank's sum of squares -> AdamW from the stash,
        pushed -> barrier B.  Only the first launch reads a peer, so every gradient byte crosses a link once.  With
        ``accumulated`` launch 1 adds to the stash, and the squares are those of the total."""
        v0, v1, mine = self._zero1_sum_to_stash(desc, count, wire, scale, error_feedback, add=accumulated)
        total = 0.0
        for x in self._exchange_sqnorm(self._seq - 1, mine):  # this call's number; float64, in rank order, on every rank alike
            total += x
        norm, gs = clip_grad_scale(total, hyper[5], clip_norm)
        self._b.adamw_push(v0, v1, hyper[:5] + [float(np.float32(gs))] + hyper[6:])
        self._leave()  # every rank's stores into every out are complete
        return norm

    def _exchange_sqnorm(self, seq: int, mine: float) -> List[float]:
        """Barrier N of a clipped step: publishes this rank's sum of squares and returns every rank's, in rank order.  It
        is the pattern by which :meth:`_enter` carries the descriptor, with its timeout and its key cleanup.  The value
        travels as ``float.hex()``, which is exact and keeps NaN and Inf.  Hazards the barrier covers: no window or packed
        buffer is read after it, and nothing has yet been written to any out."""
        self._b.synchronize()
        keys = [f"{self._prefix}/sqnorm/{seq}/{p}" for p in range(self.world)]
        self._stale[1].append(keys[self.rank])
        self._store_call(lambda: self._store.set(keys[self.rank], float(mine).hex()), "publishing the sum of squares failed")
        self._barrier()
        return self._store_call(lambda: [float.fromhex(bytes(self._store.get(k)).decode()) for k in keys], "reading the sums of squares failed")

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

    def reset_error_feedback(self) -> None:
        """This rank's residual back to zero (nothing, if it never asked for feedback).  To be called whenever
        the window is about to hold something else than the calls so far fed back on."""
        self._check()
        self._b.reset_residual()

    def residual(self, first: int, n: int) -> np.ndarray:
        """Values ``[first, first + n)`` of this rank's residual as a float32 host array, value i belonging to
        element i of the window; zeros before the first feedback call."""
        self._check()
        if first < 0 or n < 0 or (first + n) * 4 > 2 * self.capacity_bytes:
            raise ValueError("residual: past the end of the residual")
        return self._b.read_residual(first, n)

    @property
    def residual_bytes(self) -> int:
        """Bytes of this rank's residual buffer: 0 until its first feedback call, then twice the window's."""
        return self._b.residual_bytes

    def synchronize(self) -> None:
        self._b.synchronize()

    def barrier(self) -> None:
        """Synchronises this rank's stream and meets every rank at a barrier of its own, between collectives."""
        self._check()
        self._b.synchronize()
        self._barrier()

    def close(self) -> None:
        """sync, barrier (nobody still reads a peer), close_peers, barrier (nobody still maps my buffers),
        free; at last the keys this rank still owes the store are deleted.  A broken comm skips the barriers,
        and the device backend then keeps its buffers allocated (:func:`parked_bytes`): a peer may still read them."""
        if self._closed:
            return
        self._closed = True
        b = self._b
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
            if b is not None:
                b.release(self.broken)


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


def selftest_counts_q8(k: int) -> List[int]:
    # one element; under one block; one block; a block and an element; k - 1 blocks (the last slice is empty);
    # past a 16-block exponent vector with a ragged end; and whole tiles with a tail.  The host packs every
    # member's input of every case again for the reference, so the largest count stays moderate.
    return [1, 31, 32, 33, 32 * (k - 1), 512 * k + 37, 8 * 1024 * k + 11]


def selftest_cases_q8(k: int, counts: Optional[Sequence[int]] = None) -> List[Dict[str, object]]:
    """The fp8 wire's cases: ``all_reduce`` under both algorithms and ``reduce_scatter``, the three dtype pairs
    (the wide one with ``scale = 1 / k``), at every count."""
    cases: List[Dict[str, object]] = []
    for count in (selftest_counts_q8(k) if counts is None else counts):
        for dtype, out, scale in (("bf16", "bf16", 1.0), ("fp32", "fp32", 1.0), ("bf16", "fp32", 1.0 / k)):
            for algo in ALGOS:
                cases.append({"op": "all_reduce", "count": count, "dtype": dtype, "out_dtype": out, "algo": algo, "scale": scale,
                              "wire": "fp8"})
            cases.append({"op": "reduce_scatter", "count": count, "dtype": dtype, "out_dtype": out, "algo": "oneshot", "scale": scale,
                          "wire": "fp8"})
    return cases


def selftest_cases_q8x2(k: int, counts: Optional[Sequence[int]] = None) -> List[Dict[str, object]]:
    """The fp8x2 wire's cases: the two-shot ``all_reduce``, the three dtype pairs (the wide one with
    ``scale = 1 / k``), at every count of :func:`selftest_counts_q8`."""
    return [{"op": "all_reduce", "count": count, "dtype": dtype, "out_dtype": out, "algo": "twoshot", "scale": scale, "wire": "fp8x2"}
            for count in (selftest_counts_q8(k) if counts is None else counts)
            for dtype, out, scale in (("bf16", "bf16", 1.0), ("fp32", "fp32", 1.0), ("bf16", "fp32", 1.0 / k))]


def selftest_cases_push(k: int, counts: Optional[Sequence[int]] = None) -> List[Dict[str, object]]:
    """The push ``all_reduce``'s cases: the three dtype pairs (the wide one with ``scale = 1 / k``) on the native wire at
    every count of :func:`selftest_counts`, then bf16 -> bf16 and bf16 -> fp32 on the fp8 wire at every count of
    :func:`selftest_counts_q8`; ``counts``, when given, serves both."""
    cases: List[Dict[str, object]] = []
    for count in (selftest_counts(k) if counts is None else counts):
        for dtype, out, scale in (("bf16", "bf16", 1.0), ("fp32", "fp32", 1.0), ("bf16", "fp32", 1.0 / k)):
            cases.append({"op": "all_reduce", "count": count, "dtype": dtype, "out_dtype": out, "algo": PUSH, "scale": scale})
    for count in (selftest_counts_q8(k) if counts is None else counts):
        for dtype, out, scale in (("bf16", "bf16", 1.0), ("bf16", "fp32", 1.0 / k)):
            cases.append({"op": "all_reduce", "count": count, "dtype": dtype, "out_dtype": out, "algo": PUSH, "scale": scale,
                          "wire": "fp8"})
    return cases


def case_input(case_index: int, issue: int, rank: int, count: int, dtype: str) -> np.ndarray:
    """Rank ``rank``'s N(0, 1) input of the ``issue``-th issue of case ``case_index``; any rank can make any rank's."""
    rng = np.random.default_rng([case_index, issue, rank, count])
    x = rng.standard_normal(count, dtype=np.float32)
    return bf16_round(x) if dtype == "bf16" else x


def run_case(comm: PeerComm, case: Dict[str, object], inputs: Sequence[np.ndarray],
             residuals: Optional[List[np.ndarray]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Issues one case on ``comm`` with ``inputs[comm.rank]`` as this rank's data; returns (got, reference),
    both computed by this rank, the reference from every rank's input.

    A case with ``"ef": True`` is issued with error feedback.  ``residuals`` is then the reference's residual
    of every rank before this issue (float32, the count's whole blocks; none: zeros, a communicator just
    reset), and the list is given the residuals after it, so issues chain: ``comm.residual(0, n)`` must equal
    ``residuals[comm.rank]`` afterwards."""
    from ..ops.peer_ref import reduce_scatter_q8_ref, reduce_scatter_ref

    op, count, dtype, out = case["op"], int(case["count"]), case["dtype"], case["out_dtype"]
    k, r = comm.world, comm.rank
    if case.get("ef"):
        n = q8_blocks(count) * Q8_BLOCK
        before = [np.zeros(n, np.float32) for _ in range(k)] if not residuals else list(residuals)
        comm.write(inputs[r])
        if op == "all_reduce":
            comm.all_reduce(count, dtype, case["algo"], out, case["scale"], wire=case["wire"], error_feedback=True)
            got = comm.read(0, count, out)
            ref, after = allreduce_q8_ef_ref(inputs, before, dtype, out, case["scale"], wire=case["wire"])
        else:
            first, m = comm.reduce_scatter(count, dtype, out, case["scale"], wire="fp8", error_feedback=True)
            got = comm.read(first, m, out)
            pieces, after = reduce_scatter_q8_ef_ref(inputs, before, dtype, out, case["scale"])
            ref = pieces[r]
        if residuals is not None:
            residuals[:] = after
        return got, ref
    if case.get("wire") == "fp8x2":
        comm.write(inputs[r])
        comm.all_reduce(count, dtype, case["algo"], out, case["scale"], wire="fp8x2")
        return comm.read(0, count, out), allreduce_q8x2_ref(inputs, dtype, out, case["scale"])
    if case.get("wire") == "fp8":
        comm.write(inputs[r])
        if op == "all_reduce":
            comm.all_reduce(count, dtype, case["algo"], out, case["scale"], wire="fp8")
            return comm.read(0, count, out), allreduce_q8_ref(inputs, dtype, out, case["scale"])
        first, n = comm.reduce_scatter(count, dtype, out, case["scale"], wire="fp8")
        return comm.read(first, n, out), reduce_scatter_q8_ref(inputs, dtype, out, case["scale"])[r]
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


def run_thread_ranks(devices: Sequence[int], body: Callable[[PeerComm], object], capacity_bytes: int, timeout_s: float = 60.0,
                     store=None, join_s: float = 600.0, comm_cls: Callable[..., PeerComm] = PeerComm) -> List[object]:
    """One thread per rank, rank r on HIP device ``devices[r]`` (a device may repeat): each builds its
    ``PeerComm(backend="device")`` on a shared :class:`MemoryStore`, runs ``body(comm)`` and always
    closes.  Returns the ranks' results in rank order; if any rank raised, the error raised first in
    time is re-raised (a later one is usually the others timing out on the rank that failed).

    The threads are joined for at most ``join_s`` seconds in all.  When that runs out every
    communicator is marked broken, so a rank's next call raises at once and a barrier it waits in ends
    after ``timeout_s``; the threads get that long again and ``PeerCommError`` is raised.  ``comm_cls``
    stands in for :class:`PeerComm` in tests."""
    k = len(devices)
    store = MemoryStore(timeout_s=timeout_s) if store is None else store
    results: List[object] = [None] * k
    errors: List[Tuple[int, BaseException]] = []
    comms: List[Optional[PeerComm]] = [None] * k
    lock = threading.Lock()

    def run(r: int) -> None:
        try:
            comms[r] = comm = comm_cls(r, k, int(devices[r]), store, capacity_bytes, timeout_s=timeout_s, backend="device")
            try:
                results[r] = body(comm)
            finally:
                comm.close()
        except BaseException as e:  # handed to the caller's thread
            with lock:
                errors.append((r, e))

    threads = [threading.Thread(target=run, args=(r,), name=f"peer-rank-{r}", daemon=True) for r in range(k)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + join_s
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    late = [t.name for t in threads if t.is_alive()]
    if late:
        for c in comms:
            if c is not None:
                c.broken = True
        deadline = time.monotonic() + timeout_s + 5.0
        for t in threads:
            t.join(max(0.0, deadline - time.monotonic()))
        still = [t.name for t in threads if t.is_alive()]
        raise PeerCommError(f"rank threads {late} did not end within {join_s:.0f}s" + (f"; {still} are still running" if still else ""))
    if errors:
        raise errors[0][1]
    return results


class _Once:
    """``get(key, make)``: ``make()`` by the first rank that asks, the same object for the others."""

    def __init__(self):
        self._lock = threading.Lock()
        self._made: Dict[object, object] = {}

    def get(self, key, make, keep: Callable[[object], bool] = lambda k: True):
        with self._lock:
            if key not in self._made:
                for old in [o for o in self._made if not keep(o)]:
                    del self._made[old]
                self._made[key] = make()
            return self._made[key]


def timed_all_reduce(comm: PeerComm, count: int, dtype: str, algo: str, iters: int, warmup_iters: int = 1,
                     wire: Optional[str] = None) -> Tuple[float, float]:
    """``warmup_iters`` untimed and ``iters`` timed ``all_reduce`` calls of what the window holds, on one
    rank (every rank calls this).  Returns this rank's host seconds per call and, of those, the seconds
    spent inside the call's two barriers.  The clock starts after a barrier and stops when the last call
    has returned, which is after its last stream synchronise."""
    for _ in range(warmup_iters):
        comm.all_reduce(count, dtype, algo, wire=wire)
    comm.barrier()
    in_barriers, t0 = comm.barrier_s, time.perf_counter()
    for _ in range(iters):
        comm.all_reduce(count, dtype, algo, wire=wire)
    return (time.perf_counter() - t0) / iters, (comm.barrier_s - in_barriers) / iters


def thread_sweep(devices: Sequence[int], sizes: Sequence[int], dtype: str = "bf16", algo: str = "both", iters: int = 3,
                 warmup_iters: int = 1, timeout_s: float = 60.0, wire: Optional[str] = None) -> List[Dict[str, object]]:
    """``all_reduce`` on thread ranks over ``devices`` at every size (bytes) under ``algo`` (``oneshot``,
    ``twoshot``, ``push``, ``both`` for the first two or ``all`` for the three): one dict per size and algorithm, in size order, with the keys of
    ``ops.probe.peer_sweep`` and ``barrier_us``.

    At each point every rank writes a seeded input, makes ``warmup_iters + iters`` calls and reads the
    result back.  ``time_us`` is host time per call, the slowest rank's: the clock starts after a barrier
    and stops when the last call has returned.  ``barrier_us`` is the mean over ranks of the host time
    per call spent inside the call's two barriers.  ``wrong`` counts, over all ranks, the elements
    whose bits differ from ``allreduce_ref`` (``wire="fp8"``: from ``allreduce_q8_ref``, ``wire="fp8x2"``: from
    ``allreduce_q8x2_ref``, and the rows carry ``"wire"``; ``"fp8x2"`` runs the two-shot alone, so ``algo`` must be
    ``twoshot``, ``both`` or ``all``); the check runs on the host, so sizes should stay moderate."""
    if algo not in ("both", "all", PUSH) and algo not in ALGOS:
        raise ValueError(f"algo must be oneshot|twoshot|push|both|all, got {algo!r}")
    if dtype not in _ELEM:
        raise ValueError(f"dtype must be bf16|fp32, got {dtype!r}")
    if iters < 1 or warmup_iters < 0:
        raise ValueError("iters >= 1, warmup_iters >= 0")
    if wire not in WIRES:
        raise ValueError(f'wire must be None, "native", "fp8" or "fp8x2", got {wire!r}')
    if wire == "fp8x2" and algo in ("oneshot", PUSH):
        raise ValueError('wire="fp8x2" packs the gather phase of a twoshot: algo must be twoshot, both or all')
    fp8 = wire in ("fp8", "fp8x2")
    algos = ("twoshot",) if wire == "fp8x2" else ALGOS if algo == "both" else ALGOS + (PUSH,) if algo == "all" else (algo,)
    k, elem = len(devices), _ELEM[dtype]
    points = [(max(1, int(nbytes) // elem), a) for nbytes in sizes for a in algos]
    if not points:
        return []
    once = _Once()

    def body(comm: PeerComm):
        rows = []
        for count, a in points:
            xs = once.get(("in", count), lambda: [case_input(0, 0, p, count, dtype) for p in range(k)], lambda o: o[1] == count)
            ref = once.get(("ref", count), lambda: _WIRE_REF[wire](xs, dtype), lambda o: o[1] == count)
            comm.write(xs[comm.rank])
            secs, in_barriers = timed_all_reduce(comm, count, dtype, a, iters, warmup_iters, wire)
            got = comm.read(0, count, dtype)
            rows.append((secs, in_barriers, int(np.count_nonzero(_bits(got) != _bits(ref)))))
        return rows

    most = max(c for c, _ in points)
    res = run_thread_ranks(devices, body, q8_blocks(most) * Q8_BLOCK * elem if fp8 else -(-most * elem // 16) * 16, timeout_s=timeout_s)
    out: List[Dict[str, object]] = []
    for i, (count, a) in enumerate(points):
        secs = max(r[i][0] for r in res)
        gbps = count * elem / secs / 1e9
        out.append({"bytes": count * elem, "count": count, "time_us": secs * 1e6, "algbw_gbps": gbps,
                    "busbw_gbps": gbps * 2.0 * (k - 1) / k, "wrong": sum(r[i][2] for r in res), "backend": "peer", "algo": a,
                    "ranks": "thread", "barrier_us": sum(r[i][1] for r in res) / k * 1e6, **({"wire": wire} if fp8 else {})})
    return out


def _case_capacity(k: int, cases: Sequence[Dict[str, object]]) -> int:
    """Window bytes the largest of ``cases`` needs (an all-gather holds every rank's slot)."""
    def vecs(c):
        if c.get("wire") in ("fp8", "fp8x2"):  # whole blocks
            return q8_blocks(int(c["count"])) * Q8_BLOCK * _ELEM[c["dtype"]] // 16
        return _n_vec(int(c["count"]), c["dtype"]) * (k if c["op"] == "all_gather" else 1)

    return max(16, max(vecs(c) for c in cases) * 16)


def selftest_cases_ef(k: int, counts: Optional[Sequence[int]] = None) -> List[Dict[str, object]]:
    """The error-feedback cases: those of :func:`selftest_cases_q8` and :func:`selftest_cases_q8x2`, each with ``"ef": True``."""
    return [{**c, "ef": True} for c in selftest_cases_q8(k, counts) + selftest_cases_q8x2(k, counts)]


def selftest(devices: Sequence[int], counts: Optional[Sequence[int]] = None, timeout_s: float = 60.0,
             wire: Optional[str] = None, error_feedback: bool = False, push: bool = False) -> Dict[str, object]:
    """Every case of :func:`selftest_cases`, each issued twice in a row with different inputs, on
    thread ranks over ``devices`` (:func:`run_thread_ranks`), compared bit for bit with ``ops/peer_ref.py``.

    ``wrong`` counts the collectives whose dtype, shape or bits differ from the reference on any rank;
    ``barriers_per_collective`` lists the distinct numbers of barriers a collective took (``[2]``), and
    ``launches`` is the kernel launches of all ranks together.  Those keys describe the cases of
    :func:`selftest_cases`; the fp8 wire's (:func:`selftest_cases_q8`, at their own counts when ``counts`` is
    none) run after them on the same communicators and are reported as ``q8_cases``, ``q8_collectives``,
    ``q8_wrong`` and ``q8_launches``.  ``wire="fp8x2"`` adds the cases of :func:`selftest_cases_q8x2` after those,
    reported as ``q8x2_cases``, ``q8x2_collectives``, ``q8x2_wrong`` and ``q8x2_launches``.
    ``barriers_per_collective`` covers every set.

    ``error_feedback=True`` adds the cases of :func:`selftest_cases_ef` (both packed wires) after all of those.  Each is
    issued three times in a row on the one communicator with different inputs and the residual carried from
    issue to issue; the residual is reset before each case.  Every result, and after every issue the rank's
    whole residual, is compared bit for bit with the chained reference.  Reported as ``ef_cases``,
    ``ef_collectives``, ``ef_wrong`` and ``ef_launches``.

    ``push=True`` adds the cases of :func:`selftest_cases_push` after every other set, each issued twice like the plain
    ones; reported as ``push_cases``, ``push_collectives``, ``push_wrong`` and ``push_launches``."""
    if wire not in WIRES:
        raise ValueError(f'wire must be None, "native", "fp8" or "fp8x2", got {wire!r}')
    k = len(devices)
    native = selftest_cases(k, counts)
    q8 = selftest_cases_q8(k, counts)
    plain = native + q8 + (selftest_cases_q8x2(k, counts) if wire == "fp8x2" else [])
    fed_end = len(plain) + (len(selftest_cases_ef(k, counts)) if error_feedback else 0)
    cases = plain + (selftest_cases_ef(k, counts) if error_feedback else []) + (selftest_cases_push(k, counts) if push else [])
    once = _Once()  # every rank's inputs of (case, issue), made by the first rank that asks

    def inputs(ci: int, issue: int) -> List[np.ndarray]:
        make = lambda: [case_input(ci, issue, p, int(cases[ci]["count"]), cases[ci]["dtype"]) for p in range(k)]  # noqa: E731
        return once.get((ci, issue), make, lambda o: o[0] >= ci - 1)  # ranks are never more than a collective apart

    def body(comm: PeerComm):
        wrong, barriers, marks = set(), set(), {}
        for ci, case in enumerate(cases):
            if ci in (len(native), len(native) + len(q8), len(plain), fed_end):
                marks[ci] = comm.launches
            fed = bool(case.get("ef"))
            residuals: List[np.ndarray] = []
            if fed:
                comm.reset_error_feedback()
            for issue in range(3 if fed else 2):
                before = comm.barriers
                got, ref = run_case(comm, case, inputs(ci, issue), residuals if fed else None)
                barriers.add(comm.barriers - before)
                if got.dtype != ref.dtype or got.shape != ref.shape or not np.array_equal(_bits(got), _bits(ref)):
                    wrong.add((ci, issue))
                elif fed and not np.array_equal(_bits(comm.residual(0, residuals[comm.rank].size)), _bits(residuals[comm.rank])):
                    wrong.add((ci, issue))
        end_fed = marks.get(fed_end, comm.launches)  # where the push cases start
        end = marks.get(len(plain), end_fed)
        first_q8, end_q8 = marks[len(native)], marks.get(len(native) + len(q8), end)
        return wrong, barriers, first_q8, end_q8 - first_q8, end - end_q8, end_fed - end, comm.launches - end_fed

    res = run_thread_ranks(devices, body, _case_capacity(k, cases), timeout_s=timeout_s)
    bad = set().union(*(r[0] for r in res))
    n, nq = len(native), len(q8)
    rep = {"cases": n, "collectives": 2 * n, "wrong": sum(ci < n for ci, _ in bad),
           "barriers_per_collective": sorted(set().union(*(r[1] for r in res))), "launches": sum(r[2] for r in res),
           "q8_cases": nq, "q8_collectives": 2 * nq, "q8_wrong": sum(n <= ci < n + nq for ci, _ in bad),
           "q8_launches": sum(r[3] for r in res)}
    if wire == "fp8x2":
        nx = len(plain) - n - nq
        rep.update({"q8x2_cases": nx, "q8x2_collectives": 2 * nx, "q8x2_wrong": sum(n + nq <= ci < len(plain) for ci, _ in bad),
                    "q8x2_launches": sum(r[4] for r in res)})
    if error_feedback:
        ne = fed_end - len(plain)
        rep.update({"ef_cases": ne, "ef_collectives": 3 * ne, "ef_wrong": sum(len(plain) <= ci < fed_end for ci, _ in bad),
                    "ef_launches": sum(r[5] for r in res)})
    if push:
        npush = len(cases) - fed_end
        rep.update({"push_cases": npush, "push_collectives": 2 * npush, "push_wrong": sum(ci >= fed_end for ci, _ in bad),
                    "push_launches": sum(r[6] for r in res)})
    return rep
