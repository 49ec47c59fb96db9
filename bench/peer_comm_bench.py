#!/usr/bin/env python3
"""The peer communicator's thread-rank all_reduce next to the in-process driver's, as one JSON document:

    python bench/peer_comm_bench.py [--members 0,0,0,0] [--sizes-mib 1,4,16,64,256] [--dtype bf16]
                                    [--iters 20] [--warmup 2] [--wire native|fp8|fp8x2] [--error-feedback] [--push] [--zero1]
                                    [--clip-norm C] [--accumulate M]
                                    [--out FILE] [--md FILE]

Both run the same K7 kernels on the same members at the same count, in one process:
  * thread ranks (``PeerComm(backend="device")``, one thread per member): host time per ``all_reduce``
    call, each ending in a stream synchronise, the slowest rank's; and the part of it spent inside the
    call's two host barriers;
  * the in-process driver (``ops.probe.peer_allreduce``): one call enqueues every member's launches,
    ordered by stream events; event-timed per round.
Per size and algorithm the two are measured alternately, ``--reps`` times each, and the quicker
repetition of each is reported.  Their ratio is the price of host-synchronous ordering: two store round
trips and two (two-shot: three) stream synchronisations per call.  Members that repeat a device give
HBM rates of that one GPU, not xGMI rates.  ``--wire fp8`` runs both on the fp8 wire: every rank packs its
window first and the ranks read the packed forms; ``--wire fp8x2`` the two-shot alone, its gather phase packed too.

``--error-feedback`` measures something else: the thread ranks' fp8 ``reduce_scatter`` and two-shot ``all_reduce``
with and without error feedback, the two alternated ``--reps`` times in one process, the quicker repetition of
each reported.  The feedback form's quantize reads and writes the rank's fp32 residual next to the window; the
link bytes, the launches and the barriers are the plain call's.  No driver run is made.

``--push`` measures the push algorithm (``all_reduce(algo="push")``: one launch stores the rank's slice of the sum
into every rank's out; two stream synchronisations per call where the two-shot has three) against the two-shot
on thread ranks, on the native and on the fp8 wire, the two alternated ``--reps`` times in one process, the
quicker repetition of each reported.  Up to ``--check-max-mib`` the push result is compared with the host
reference; at every size it is compared bit for bit with the two-shot's.  No driver run is made.

``--zero1`` measures the ZeRO-1 step (``PeerComm.zero1_step``: one launch sums the rank's slice of every window, applies
AdamW to the rank's own fp32 state and stores the new bf16 weights into every rank's out) against the same communication
with no optimizer at all: ``reduce_scatter(out_dtype="fp32")`` followed by ``all_gather`` of count / k bf16 elements, two
launches and four barriers.  The two are alternated ``--reps`` times in one process on thread ranks, on the native and on
the fp8 wire, the quicker repetition of each reported; the number of interest is how far the fused step exceeds the bare
communication, if at all.  After the timed steps every rank's weights must be rank 0's and its own master rounded once,
and up to ``--check-max-mib`` the first step is compared with the host reference at the GPU tests' tolerances.
``--clip-norm C`` alternates the clipped step (``zero1_step(clip_norm=C)``: two launches and three barriers) with those
two, checks its first step and its norm against the reference, and reports the host time each step spends in barriers.

``--zero1 --accumulate M`` measures gradient accumulation over M micro-batches: ``M - 1`` ``zero1_accumulate`` calls followed
by ``zero1_step(accumulated=True)``, against ``M - 1`` ``reduce_scatter(out_dtype="fp32")`` calls followed by the plain step,
which move the same link bytes and accumulate nothing.  The two are alternated ``--reps`` times in one process, without and
(``--clip-norm C``) with clipping, the quicker repetition of each reported per optimizer step.  Up to ``--check-max-mib``
the first accumulated step is compared with the host reference: the accumulator bit for bit, the state at the GPU tests'
tolerances.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpu_topology_on_k8s_amd.ops import probe  # noqa: E402
from gpu_topology_on_k8s_amd.ops.peer_ref import Q8_BLOCK, q8_blocks  # noqa: E402
from gpu_topology_on_k8s_amd.parallel import peer_comm as pc  # noqa: E402

ELEM = {"bf16": 2, "fp32": 4}


def measure(devs, sizes, dtype, iters, warmup, reps, wire="native"):
    k, elem = len(devs), ELEM[dtype]
    fp8 = wire in ("fp8", "fp8x2")
    algos = ("twoshot",) if wire == "fp8x2" else pc.ALGOS  # the one algorithm with a gather phase to pack
    counts = [max(1, n // elem) for n in sizes]
    once = pc._Once()
    driver = {}  # (count, algo, rep) -> the driver's result, measured by rank 0 while the other ranks wait

    def body(comm):
        rows = []
        for count in counts:
            xs = once.get(("in", count), lambda: [pc.case_input(0, 0, p, count, dtype) for p in range(k)], lambda o: o[1] == count)
            ref = once.get(("ref", count), lambda: pc._WIRE_REF[wire](xs, dtype), lambda o: o[1] == count)
            comm.write(xs[comm.rank])
            for algo in algos:
                for rep in range(reps):
                    secs, in_barriers = pc.timed_all_reduce(comm, count, dtype, algo, iters, warmup, wire)
                    wrong = int(np.count_nonzero(pc._bits(comm.read(0, count, dtype)) != pc._bits(ref))) if rep == 0 else 0
                    rows.append((count, algo, rep, secs, in_barriers, wrong))
                    comm.barrier()  # every rank's stream is idle: the driver has the device to itself
                    if comm.rank == 0:
                        driver[(count, algo, rep)] = probe.peer_allreduce(devs, count, dtype, algo, iters, warmup, wire=wire)
                    comm.barrier()
        return rows

    cap = q8_blocks(max(counts)) * Q8_BLOCK * elem if fp8 else -(-max(counts) * elem // 16) * 16
    res = pc.run_thread_ranks(devs, body, cap, timeout_s=300.0, join_s=3000.0)
    out = []
    for count in counts:
        row = {"bytes": count * elem, "count": count}
        for algo in algos:
            mine = [[r for r in rank_rows if r[:2] == (count, algo)] for rank_rows in res]
            t_reps = [max(rows[rep][3] for rows in mine) * 1e6 for rep in range(reps)]  # the slowest rank of each repetition
            best = min(range(reps), key=lambda i: t_reps[i])
            d_reps = [driver[(count, algo, rep)] for rep in range(reps)]
            d = min(d_reps, key=lambda r: r["time_us"])
            thread_us = t_reps[best]
            row[algo] = {
                "thread_time_us": thread_us, "thread_barrier_us": sum(rows[best][4] for rows in mine) / k * 1e6,
                "thread_algbw_gbps": count * elem / (thread_us * 1e-6) / 1e9, "thread_time_us_reps": t_reps,
                "thread_wrong": sum(r[5] for rows in mine for r in rows),
                "driver_time_us": d["time_us"], "driver_algbw_gbps": d["algbw_gbps"], "driver_time_us_reps": [r["time_us"] for r in d_reps],
                "driver_wrong": sum(int(r["wrong"]) for r in d_reps), "thread_over_driver": thread_us / d["time_us"]}
        out.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return {"members": list(devs), "k": k, "distinct_devices": len(set(devs)) == k, "dtype": dtype, "iters": iters, "warmup": warmup,
            "reps": reps, "wire": wire, "sizes": out}


def measure_push(devs, sizes, dtype, iters, warmup, reps, check_max_bytes):
    """Host seconds per ``all_reduce`` call of the two-shot and of the push on thread ranks, alternated, on both wires."""
    k, elem = len(devs), ELEM[dtype]
    counts = [max(1, n // elem) for n in sizes]
    once = pc._Once()

    def body(comm):
        rows = []
        for count in counts:
            xs = once.get(("in", count), lambda: [pc.case_input(0, 0, p, count, dtype) for p in range(k)], lambda o: o[1] == count)
            comm.write(xs[comm.rank])
            for wire in ("native", "fp8"):
                checked = count * elem <= check_max_bytes
                ref = once.get(("ref", count, wire), lambda: pc._WIRE_REF[wire](xs, dtype), lambda o: o[1] == count) if checked else None
                for r in range(reps):
                    two, two_barriers = pc.timed_all_reduce(comm, count, dtype, "twoshot", iters, warmup, wire)
                    kept = comm.read(0, count, dtype) if r == 0 else None
                    comm.barrier()  # no rank checks a result, holding the interpreter, while another still reads its clock
                    push, push_barriers = pc.timed_all_reduce(comm, count, dtype, "push", iters, warmup, wire)
                    wrong = differ = 0
                    if r == 0:
                        got = comm.read(0, count, dtype)
                        differ = int(np.count_nonzero(pc._bits(got) != pc._bits(kept)))
                        wrong = int(np.count_nonzero(pc._bits(got) != pc._bits(ref))) if checked else 0
                    comm.barrier()
                    rows.append((count, wire, r, two, push, two_barriers, push_barriers, wrong, differ, checked))
        return rows

    res = pc.run_thread_ranks(devs, body, q8_blocks(max(counts)) * Q8_BLOCK * elem, timeout_s=300.0, join_s=3000.0)
    out = []
    for count in counts:
        row = {"bytes": count * elem, "count": count}
        for wire in ("native", "fp8"):
            mine = [[r for r in rank_rows if r[:2] == (count, wire)] for rank_rows in res]
            two = [max(rows[r][3] for rows in mine) * 1e6 for r in range(reps)]  # the slowest rank of each repetition
            push = [max(rows[r][4] for rows in mine) * 1e6 for r in range(reps)]
            bt, bp = min(range(reps), key=lambda i: two[i]), min(range(reps), key=lambda i: push[i])
            row[wire] = {"twoshot_time_us": two[bt], "push_time_us": push[bp], "push_over_twoshot": push[bp] / two[bt],
                         "twoshot_barrier_us": sum(rows[bt][5] for rows in mine) / k * 1e6,
                         "push_barrier_us": sum(rows[bp][6] for rows in mine) / k * 1e6,
                         "twoshot_time_us_reps": two, "push_time_us_reps": push, "checked_against_reference": bool(mine[0][0][9]),
                         "push_wrong": sum(r[7] for rows in mine for r in rows), "push_differs_from_twoshot": sum(r[8] for rows in mine for r in rows)}
        out.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return {"members": list(devs), "k": k, "distinct_devices": len(set(devs)) == k, "dtype": dtype, "iters": iters, "warmup": warmup,
            "reps": reps, "push": True, "sizes": out}


def markdown_push(res) -> str:
    out = [f"### push against two-shot, thread ranks, members {res['members']} (k = {res['k']}), {res['dtype']}, {res['iters']} timed calls, "
           f"best of {res['reps']} alternated repetitions", "",
           "| N per member | wire | twoshot us / call | of it in barriers | push us / call | of it in barriers | push / twoshot | wrong | differs from twoshot |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in res["sizes"]:
        for wire in ("native", "fp8"):
            a = r[wire]
            out.append(f"| {r['bytes'] / 2**20:.1f} MiB | {wire} | {a['twoshot_time_us']:.1f} | {a['twoshot_barrier_us']:.1f} | {a['push_time_us']:.1f} "
                       f"| {a['push_barrier_us']:.1f} | {a['push_over_twoshot']:.2f} | {a['push_wrong'] if a['checked_against_reference'] else 'n/a'} "
                       f"| {a['push_differs_from_twoshot']} |")
    out.append("")
    return "\n".join(out)


ZERO1_HP = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1)


def measure_zero1(devs, sizes, iters, warmup, reps, check_max_bytes, clip_norm=None):
    """Host seconds per call of the fused ZeRO-1 step and of reduce_scatter (fp32 out) + all_gather (count / k bf16), alternated;
    with ``clip_norm`` the clipped step (two launches, three barriers) is alternated with them, and the host seconds each
    step spends inside its barriers are reported next to its time."""
    import time

    from gpu_topology_on_k8s_amd.ops.peer_ref import bf16_round, bf16_to_f32, zero1_slices, zero1_step_ref

    k = len(devs)
    counts = [max(1, n // 2) for n in sizes]
    once = pc._Once()
    scale = float(np.float32(1.0 / k))

    def start(w0, plan):  # what zero1_init makes of the weights: every rank's master widened, m and v zero
        out = []
        for p, q in plan:
            master = np.zeros(q - p, np.float32)
            master[:max(0, min(q, w0.size) - p)] = bf16_to_f32(w0[p:q])
            out.append((master, np.zeros(q - p, np.float32), np.zeros(q - p, np.float32)))
        return out

    def timed(comm, call):
        for i in range(warmup):
            call(i)
        comm.barrier()
        in_barriers, t0 = comm.barrier_s, time.perf_counter()
        for i in range(iters):
            call(warmup + i)
        secs, waited = (time.perf_counter() - t0) / iters, (comm.barrier_s - in_barriers) / iters
        comm.barrier()  # no rank goes on to check its result, holding the interpreter, while another still reads its clock
        return secs, waited

    def body(comm):
        rows = []
        for count in counts:
            xs = once.get(("in", count), lambda: [pc.case_input(0, 0, p, count, "bf16") for p in range(k)], lambda o: o[1] == count)
            w0 = once.get(("w", count), lambda: pc.case_input(1, 0, 0, count, "bf16"), lambda o: o[1] == count)
            per = -(-count // k)  # elements every rank contributes to the all-gather of the weights
            for wire in ("native", "fp8"):
                checked = count * 2 <= check_max_bytes
                plan = zero1_slices(count, k, wire)
                a, b = plan[comm.rank]
                comm.write(xs[comm.rank])
                comm.zero1_init(count, w0, wire)
                wrong = 0
                if checked:  # the first step against the host reference
                    ref = once.get(("ref", count, wire), lambda: zero1_step_ref(xs, start(w0, plan), "bf16", scale,
                                                                                 pc.zero1_hyper(step=1, **ZERO1_HP), wire), lambda o: o[1] == count)
                    comm.zero1_step(step=1, **ZERO1_HP)
                    wrong = sum(int(np.count_nonzero(~np.isclose(g, r, rtol=1e-5, atol=tol)))
                                for g, r, tol in zip(comm.zero1_state(), ref[0][comm.rank], (1e-6, 1e-6, 1e-7)))
                    comm.zero1_init(count, w0, wire)
                clip_wrong, norm_rel = 0, 0.0
                if checked and clip_norm is not None:  # the first clipped step against the host reference, its norm too
                    ref = once.get(("clip", count, wire), lambda: zero1_step_ref(xs, start(w0, plan), "bf16", scale, pc.zero1_hyper(step=1, **ZERO1_HP),
                                                                                  wire, clip_norm=clip_norm), lambda o: o[1] == count)
                    norm = comm.zero1_step(step=1, clip_norm=clip_norm, **ZERO1_HP)
                    clip_wrong = sum(int(np.count_nonzero(~np.isclose(g, r, rtol=1e-5, atol=tol)))
                                     for g, r, tol in zip(comm.zero1_state(), ref[0][comm.rank], (1e-6, 1e-6, 1e-7)))
                    norm_rel = abs(norm - ref[2]) / ref[2]
                    comm.zero1_init(count, w0, wire)
                for r in range(reps):
                    clipped = (0.0, 0.0)
                    if clip_norm is not None:
                        clipped = timed(comm, lambda i: comm.zero1_step(step=i + 1, clip_norm=clip_norm, **ZERO1_HP))
                        comm.zero1_init(count, w0, wire)  # the fused step starts where the clipped one did, and without a stash
                    fused, fused_waited = timed(comm, lambda i: comm.zero1_step(step=i + 1, **ZERO1_HP))
                    out = comm.read(0, count, "bf16")
                    unrounded = int(np.count_nonzero(out[min(count, a):min(count, b)] != bf16_round(comm.zero1_state()[0])[:max(0, min(count, b) - a)]))
                    comm.barrier()

                    def bare(i):
                        comm.reduce_scatter(count, "bf16", "fp32", scale, wire=None if wire == "native" else wire)
                        comm.all_gather(per, "bf16")

                    comm.write(xs[comm.rank])
                    two, _ = timed(comm, bare)
                    rows.append((count, wire, r, fused, two, wrong if r == 0 else 0, unrounded, out if r == 0 else None, checked,
                                 clipped[0], clipped[1], fused_waited, clip_wrong if r == 0 else 0, norm_rel))
                    comm.zero1_init(count, w0, wire)  # the same trajectory for every repetition
        return rows

    cap = max(q8_blocks(max(counts)) * Q8_BLOCK * 2, 16 * k * -(-(-(-max(counts) // k)) * 2 // 16))
    res = pc.run_thread_ranks(devs, body, cap, timeout_s=300.0, join_s=3000.0)
    out = []
    for count in counts:
        row = {"bytes": count * 2, "count": count}
        for wire in ("native", "fp8"):
            mine = [[r for r in rank_rows if r[:2] == (count, wire)] for rank_rows in res]
            fused = [max(rows[r][3] for rows in mine) * 1e6 for r in range(reps)]  # the slowest rank of each repetition
            two = [max(rows[r][4] for rows in mine) * 1e6 for r in range(reps)]
            row[wire] = {"fused_step_time_us": min(fused), "reduce_scatter_all_gather_time_us": min(two),
                         "fused_over_bare_communication": min(fused) / min(two), "fused_step_time_us_reps": fused,
                         "reduce_scatter_all_gather_time_us_reps": two, "checked_against_reference": bool(mine[0][0][8]),
                         "state_outside_tolerance": sum(r[5] for rows in mine for r in rows),
                         "weights_not_the_rounded_master": sum(r[6] for rows in mine for r in rows),
                         "weights_differ_between_ranks": sum(int(np.count_nonzero(rows[0][7] != mine[0][0][7])) for rows in mine)}
            if clip_norm is not None:
                clipped = [max(rows[r][9] for rows in mine) * 1e6 for r in range(reps)]
                best = clipped.index(min(clipped))
                row[wire].update({"clipped_step_time_us": min(clipped), "clipped_step_time_us_reps": clipped,
                                  "clipped_over_fused": min(clipped) / min(fused), "clipped_over_bare_communication": min(clipped) / min(two),
                                  "clipped_step_barrier_us": float(np.mean([rows[best][10] for rows in mine])) * 1e6,  # three barriers, mean over ranks
                                  "fused_step_barrier_us": float(np.mean([rows[fused.index(min(fused))][11] for rows in mine])) * 1e6,  # two
                                  "clipped_state_outside_tolerance": sum(r[12] for rows in mine for r in rows),
                                  "clipped_norm_relative_error": max(r[13] for rows in mine for r in rows)})
        out.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return {"members": list(devs), "k": k, "distinct_devices": len(set(devs)) == k, "dtype": "bf16", "iters": iters, "warmup": warmup,
            "reps": reps, "zero1": True, "hyper": ZERO1_HP, **({} if clip_norm is None else {"clip_norm": clip_norm}), "sizes": out}


def measure_zero1_accum(devs, sizes, iters, warmup, reps, check_max_bytes, micro, clip_norm=None):
    """Host seconds per optimizer step of ``micro`` micro-batches: ``micro - 1`` accumulates and the accumulated step, against
    ``micro - 1`` reduce_scatter calls (fp32 out) and the plain step; with ``clip_norm`` both pairs once more, clipped."""
    import time

    from gpu_topology_on_k8s_amd.ops.peer_ref import bf16_to_f32, zero1_accumulate_ref, zero1_slices, zero1_step_ref

    k = len(devs)
    counts = [max(1, n // 2) for n in sizes]
    once = pc._Once()
    scale = float(np.float32(1.0 / k))
    clips = (None,) if clip_norm is None else (None, clip_norm)

    def start(w0, plan):
        out = []
        for p, q in plan:
            master = np.zeros(q - p, np.float32)
            master[:max(0, min(q, w0.size) - p)] = bf16_to_f32(w0[p:q])
            out.append((master, np.zeros(q - p, np.float32), np.zeros(q - p, np.float32)))
        return out

    def reference(xs, w0, plan, wire, clip):
        acc = None
        for j in range(micro - 1):
            acc = zero1_accumulate_ref(acc, xs[j], "bf16", scale, wire)
        return acc, zero1_step_ref(xs[micro - 1], start(w0, plan), "bf16", scale, pc.zero1_hyper(step=1, **ZERO1_HP), wire, clip_norm=clip,
                                   accumulated=acc)

    def timed(comm, call):
        for i in range(warmup):
            call(i)
        comm.barrier()
        t0 = time.perf_counter()
        for i in range(iters):
            call(warmup + i)
        secs = (time.perf_counter() - t0) / iters
        comm.barrier()  # no rank goes on to check its result, holding the interpreter, while another still reads its clock
        return secs

    def body(comm):
        rows = []
        for count in counts:
            xs = once.get(("in", count), lambda: [[pc.case_input(0, j, p, count, "bf16") for p in range(k)] for j in range(micro)],
                          lambda o: o[1] == count)
            w0 = once.get(("w", count), lambda: pc.case_input(1, 0, 0, count, "bf16"), lambda o: o[1] == count)
            for wire in ("native", "fp8"):
                checked = count * 2 <= check_max_bytes
                plan = zero1_slices(count, k, wire)
                a, b = plan[comm.rank]
                wrong = {}
                for clip in clips if checked else ():  # the first accumulated step against the host reference
                    acc, ref = once.get(("ref", count, wire, clip), lambda: reference(xs, w0, plan, wire, clip), lambda o: o[1] == count)
                    comm.zero1_init(count, w0, wire)
                    for j in range(micro - 1):
                        comm.write(xs[j][comm.rank])
                        comm.zero1_accumulate()
                    acc_wrong = int(np.count_nonzero(pc._bits(comm._b.zero1_read_state(3, 0, b - a)) != pc._bits(acc[comm.rank])))
                    comm.write(xs[micro - 1][comm.rank])
                    norm = comm.zero1_step(step=1, clip_norm=clip, accumulated=True, **ZERO1_HP)
                    state_wrong = sum(int(np.count_nonzero(~np.isclose(g, r, rtol=1e-5, atol=tol)))
                                      for g, r, tol in zip(comm.zero1_state(), ref[0][comm.rank], (1e-6, 1e-6, 1e-7)))
                    wrong[clip] = (acc_wrong, state_wrong, 0.0 if clip is None else abs(norm - ref[2]) / ref[2])
                comm.write(xs[0][comm.rank])
                for r in range(reps):
                    for clip in clips:
                        def accumulated(i):
                            for _ in range(micro - 1):
                                comm.zero1_accumulate()
                            comm.zero1_step(step=i + 1, clip_norm=clip, accumulated=True, **ZERO1_HP)

                        def plain(i):
                            for _ in range(micro - 1):
                                comm.reduce_scatter(count, "bf16", "fp32", scale, wire=None if wire == "native" else wire)
                            comm.zero1_step(step=i + 1, clip_norm=clip, **ZERO1_HP)

                        comm.zero1_init(count, w0, wire)
                        acc_s = timed(comm, accumulated)
                        comm.zero1_init(count, w0, wire)
                        plain_s = timed(comm, plain)
                        rows.append((count, wire, r, clip, acc_s, plain_s, wrong.get(clip, (0, 0, 0.0)) if r == 0 else (0, 0, 0.0), checked))
        return rows

    cap = q8_blocks(max(counts)) * Q8_BLOCK * 2
    res = pc.run_thread_ranks(devs, body, cap, timeout_s=300.0, join_s=3000.0)
    out = []
    for count in counts:
        row = {"bytes": count * 2, "count": count}
        for wire in ("native", "fp8"):
            row[wire] = {}
            for clip in clips:
                mine = [[r for r in rank_rows if r[:2] == (count, wire) and r[3] == clip] for rank_rows in res]
                acc = [max(rows[r][4] for rows in mine) * 1e6 for r in range(reps)]  # the slowest rank of each repetition
                plain = [max(rows[r][5] for rows in mine) * 1e6 for r in range(reps)]
                row[wire]["unclipped" if clip is None else "clipped"] = {
                    "accumulated_step_time_us": min(acc), "reduce_scatters_and_plain_step_time_us": min(plain),
                    "accumulated_over_plain": min(acc) / min(plain), "accumulated_step_time_us_reps": acc,
                    "reduce_scatters_and_plain_step_time_us_reps": plain, "checked_against_reference": bool(mine[0][0][7]),
                    "accumulator_bits_wrong": sum(r[6][0] for rows in mine for r in rows),
                    "state_outside_tolerance": sum(r[6][1] for rows in mine for r in rows),
                    "norm_relative_error": max(r[6][2] for rows in mine for r in rows)}
        out.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return {"members": list(devs), "k": k, "distinct_devices": len(set(devs)) == k, "dtype": "bf16", "iters": iters, "warmup": warmup,
            "reps": reps, "zero1": True, "accumulate": micro, "hyper": ZERO1_HP, **({} if clip_norm is None else {"clip_norm": clip_norm}),
            "sizes": out}


def markdown_zero1_accum(res) -> str:
    m = res["accumulate"]
    out = [f"### {m} micro-batches per optimizer step: {m - 1} zero1_accumulate + zero1_step(accumulated=True) against {m - 1} reduce_scatter "
           f"(fp32 out) + the plain step, thread ranks, members {res['members']} (k = {res['k']}), {res['iters']} timed optimizer steps, best of "
           f"{res['reps']} alternated repetitions", "",
           "| gradient per member | wire | step | accumulated us / optimizer step | reduce_scatters + plain step us | accumulated / plain | failed checks |",
           "|---|---|---|---|---|---|---|"]
    for r in res["sizes"]:
        for wire in ("native", "fp8"):
            for name, a in r[wire].items():
                out.append(f"| {r['bytes'] / 2**20:.1f} MiB | {wire} | {name} | {a['accumulated_step_time_us']:.1f} "
                           f"| {a['reduce_scatters_and_plain_step_time_us']:.1f} | {a['accumulated_over_plain']:.2f} "
                           f"| {a['accumulator_bits_wrong'] + a['state_outside_tolerance']} |")
    out.append("")
    return "\n".join(out)


ZERO1_CHECKS = ("state_outside_tolerance", "weights_not_the_rounded_master", "weights_differ_between_ranks")


def markdown_zero1(res) -> str:
    out = [f"### ZeRO-1 step against reduce_scatter (fp32 out) + all_gather, thread ranks, members {res['members']} (k = {res['k']}), "
           f"{res['iters']} timed calls, best of {res['reps']} alternated repetitions", "",
           "| gradient per member | wire | fused step us / call | reduce_scatter + all_gather us / call | fused / bare communication | failed checks |",
           "|---|---|---|---|---|---|"]
    for r in res["sizes"]:
        for wire in ("native", "fp8"):
            a = r[wire]
            out.append(f"| {r['bytes'] / 2**20:.1f} MiB | {wire} | {a['fused_step_time_us']:.1f} | {a['reduce_scatter_all_gather_time_us']:.1f} "
                       f"| {a['fused_over_bare_communication']:.2f} | {sum(a[c] for c in ZERO1_CHECKS)} |")
    out.append("")
    if "clip_norm" in res:
        out += [f"### Clipped ZeRO-1 step (clip_norm = {res['clip_norm']}: two launches, three barriers) against the unclipped fused step and "
                f"reduce_scatter (fp32 out) + all_gather, members {res['members']} (k = {res['k']})", "",
                "| gradient per member | wire | clipped us / call | fused us / call | reduce_scatter + all_gather us / call | clipped / fused "
                "| in barriers, clipped us | in barriers, fused us | failed checks |", "|---|---|---|---|---|---|---|---|---|"]
        for r in res["sizes"]:
            for wire in ("native", "fp8"):
                a = r[wire]
                out.append(f"| {r['bytes'] / 2**20:.1f} MiB | {wire} | {a['clipped_step_time_us']:.1f} | {a['fused_step_time_us']:.1f} "
                           f"| {a['reduce_scatter_all_gather_time_us']:.1f} | {a['clipped_over_fused']:.2f} | {a['clipped_step_barrier_us']:.1f} "
                           f"| {a['fused_step_barrier_us']:.1f} | {a['clipped_state_outside_tolerance']} |")
        out.append("")
    return "\n".join(out)


EF_CALLS = ("reduce_scatter", "twoshot")


def measure_ef(devs, sizes, dtype, iters, warmup, reps):
    """Host seconds per call of the fp8 ``reduce_scatter`` and two-shot ``all_reduce`` on thread ranks, without and
    with error feedback, alternated.  The plain result is checked against the reference; after the feedback
    calls every residual must lie within 1/13 of its block's input amax."""
    import time

    from gpu_topology_on_k8s_amd.ops.peer_ref import allreduce_q8_ref, bf16_to_f32

    k, elem = len(devs), ELEM[dtype]
    counts = [max(1, n // elem) for n in sizes]
    once = pc._Once()

    def call(comm, what, count, fed):
        if what == "reduce_scatter":
            comm.reduce_scatter(count, dtype, wire="fp8", error_feedback=fed)
        else:
            comm.all_reduce(count, dtype, "twoshot", wire="fp8", error_feedback=fed)

    def timed(comm, what, count, fed):
        for _ in range(warmup):
            call(comm, what, count, fed)
        comm.barrier()
        t0 = time.perf_counter()
        for _ in range(iters):
            call(comm, what, count, fed)
        secs = (time.perf_counter() - t0) / iters
        comm.barrier()  # no rank goes on to check its result, holding the interpreter, while another still reads its clock
        return secs

    def body(comm):
        rows = []
        for count in counts:
            xs = once.get(("in", count), lambda: [pc.case_input(0, 0, p, count, dtype) for p in range(k)], lambda o: o[1] == count)
            ref = once.get(("ref", count), lambda: allreduce_q8_ref(xs, dtype), lambda o: o[1] == count)
            comm.write(xs[comm.rank])
            n = q8_blocks(count) * Q8_BLOCK
            mine = np.zeros(n, np.float32)
            mine[:count] = np.abs(bf16_to_f32(xs[comm.rank]) if dtype == "bf16" else xs[comm.rank])
            bound = np.repeat(mine.reshape(-1, Q8_BLOCK).max(axis=1), Q8_BLOCK) / np.float32(13)
            for what in EF_CALLS:
                for r in range(reps):
                    plain = timed(comm, what, count, False)
                    wrong = int(np.count_nonzero(pc._bits(comm.read(0, count, dtype)) != pc._bits(ref))) if what == "twoshot" and r == 0 else 0
                    comm.reset_error_feedback()
                    fed = timed(comm, what, count, True)
                    over = int(np.count_nonzero(np.abs(comm.residual(0, n)) > bound))
                    rows.append((count, what, r, plain, fed, wrong, over))
        return rows

    res = pc.run_thread_ranks(devs, body, q8_blocks(max(counts)) * Q8_BLOCK * elem, timeout_s=300.0, join_s=3000.0)
    out = []
    for count in counts:
        row = {"bytes": count * elem, "count": count}
        for what in EF_CALLS:
            mine = [[r for r in rank_rows if r[:2] == (count, what)] for rank_rows in res]
            plain = [max(rows[r][3] for rows in mine) * 1e6 for r in range(reps)]  # the slowest rank of each repetition
            fed = [max(rows[r][4] for rows in mine) * 1e6 for r in range(reps)]
            row[what] = {"plain_time_us": min(plain), "ef_time_us": min(fed), "ef_over_plain": min(fed) / min(plain),
                         "plain_time_us_reps": plain, "ef_time_us_reps": fed, "plain_wrong": sum(r[5] for rows in mine for r in rows),
                         "residual_over_bound": sum(r[6] for rows in mine for r in rows)}
        out.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return {"members": list(devs), "k": k, "distinct_devices": len(set(devs)) == k, "dtype": dtype, "iters": iters, "warmup": warmup,
            "reps": reps, "wire": "fp8", "error_feedback": True, "sizes": out}


def markdown_ef(res) -> str:
    out = [f"### members {res['members']} (k = {res['k']}), {res['dtype']}, fp8 wire, thread ranks, {res['iters']} timed calls, best of {res['reps']} alternated repetitions", "",
           "| N per member | call | plain us / call | with feedback us / call | feedback / plain |", "|---|---|---|---|---|"]
    for r in res["sizes"]:
        for what in EF_CALLS:
            a = r[what]
            out.append(f"| {r['bytes'] / 2**20:.1f} MiB | {what} | {a['plain_time_us']:.1f} | {a['ef_time_us']:.1f} | {a['ef_over_plain']:.2f} |")
    out.append("")
    return "\n".join(out)


def markdown(res) -> str:
    out = [f"### members {res['members']} (k = {res['k']}), {res['dtype']}, {res['wire']} wire, {res['iters']} timed calls, best of {res['reps']} alternated repetitions", "",
           "| N per member | algorithm | thread ranks us / call | of it in barriers | thread algBW | driver us / round | driver algBW | thread / driver |",
           "|---|---|---|---|---|---|---|---|"]
    for r in res["sizes"]:
        for algo in (al for al in pc.ALGOS if al in r):
            a = r[algo]
            out.append(f"| {r['bytes'] / 2**20:.1f} MiB | {algo} | {a['thread_time_us']:.1f} | {a['thread_barrier_us']:.1f} | {a['thread_algbw_gbps']:.1f} "
                       f"| {a['driver_time_us']:.1f} | {a['driver_algbw_gbps']:.1f} | {a['thread_over_driver']:.2f} |")
    out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", action="append", default=[], help="HIP ordinals, comma-separated; may be given more than once")
    ap.add_argument("--sizes-mib", default="1,4,16,64,256")
    ap.add_argument("--dtype", default="bf16", choices=sorted(ELEM))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--wire", default="native", choices=["native", "fp8", "fp8x2"],
                    help="fp8: the block-scaled e4m3 wire of csrc/probe/peer_q8.h; fp8x2: the two-shot with its gather phase packed too")
    ap.add_argument("--error-feedback", action="store_true",
                    help="thread ranks alone: the fp8 reduce_scatter and two-shot all_reduce without and with error feedback, alternated")
    ap.add_argument("--push", action="store_true", help="thread ranks alone: the push all_reduce against the two-shot on the native and the fp8 wire, alternated")
    ap.add_argument("--zero1", action="store_true",
                    help="thread ranks alone: the fused ZeRO-1 step against reduce_scatter (fp32 out) + all_gather, on the native and the fp8 wire, alternated")
    ap.add_argument("--clip-norm", type=float, default=None,
                    help="--zero1: also time zero1_step(clip_norm=C), alternated with the unclipped step and the bare communication")
    ap.add_argument("--accumulate", type=int, default=0, metavar="M",
                    help="--zero1: M micro-batches per optimizer step, M - 1 zero1_accumulate and the accumulated step against M - 1 "
                         "reduce_scatter (fp32 out) and the plain step, alternated; with --clip-norm both pairs clipped as well")
    ap.add_argument("--check-max-mib", type=float, default=64.0, help="--push, --zero1: the largest size whose result is compared with the host reference")
    ap.add_argument("--reps", type=int, default=2, help="alternated repetitions of each measurement")
    ap.add_argument("--out", default="", help="also write the JSON document here")
    ap.add_argument("--md", default="", help="also write the tables as Markdown here")
    a = ap.parse_args()
    groups = [[int(x) for x in m.split(",")] for m in (a.members or ["0,0,0,0"])]
    sizes = [int(float(x) * (1 << 20)) for x in a.sizes_mib.split(",")]
    if a.accumulate and (not a.zero1 or a.accumulate < 2):
        ap.error("--accumulate M belongs to --zero1 and needs M >= 2")
    probe.warmup(groups[0][0], 100.0)
    if a.zero1 and a.accumulate:
        doc = {"device": probe.device_props(groups[0][0])["name"],
               "runs": [measure_zero1_accum(g, sizes, a.iters, a.warmup, max(1, a.reps), int(a.check_max_mib * (1 << 20)), a.accumulate,
                                            a.clip_norm) for g in groups]}
        text = json.dumps(doc)
        print(text)
        for path, body in ((a.out, text + "\n"), (a.md, "\n".join(markdown_zero1_accum(r) for r in doc["runs"]))):
            if path:
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
                with open(path, "w") as f:
                    f.write(body)
        return 1 if any(c[key] for run in doc["runs"] for r in run["sizes"] for w in ("native", "fp8") for c in r[w].values()
                        for key in ("accumulator_bits_wrong", "state_outside_tolerance")) else 0
    if a.zero1:
        doc = {"device": probe.device_props(groups[0][0])["name"],
               "runs": [measure_zero1(g, sizes, a.iters, a.warmup, max(1, a.reps), int(a.check_max_mib * (1 << 20)), a.clip_norm) for g in groups]}
        text = json.dumps(doc)
        print(text)
        for path, body in ((a.out, text + "\n"), (a.md, "\n".join(markdown_zero1(r) for r in doc["runs"]))):
            if path:
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
                with open(path, "w") as f:
                    f.write(body)
        return 1 if any(r[w][key] for run in doc["runs"] for r in run["sizes"] for w in ("native", "fp8") for key in ZERO1_CHECKS) else 0
    if a.push:
        doc = {"device": probe.device_props(groups[0][0])["name"],
               "runs": [measure_push(g, sizes, a.dtype, a.iters, a.warmup, max(1, a.reps), int(a.check_max_mib * (1 << 20))) for g in groups]}
        text = json.dumps(doc)
        print(text)
        for path, body in ((a.out, text + "\n"), (a.md, "\n".join(markdown_push(r) for r in doc["runs"]))):
            if path:
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
                with open(path, "w") as f:
                    f.write(body)
        return 1 if any(r[w][key] for run in doc["runs"] for r in run["sizes"] for w in ("native", "fp8")
                        for key in ("push_wrong", "push_differs_from_twoshot")) else 0
    if a.error_feedback:
        if a.wire == "fp8x2":
            ap.error("--error-feedback compares the calls of the fp8 wire")
        doc = {"device": probe.device_props(groups[0][0])["name"],
               "runs": [measure_ef(g, sizes, a.dtype, a.iters, a.warmup, max(1, a.reps)) for g in groups]}
        text = json.dumps(doc)
        print(text)
        for path, body in ((a.out, text + "\n"), (a.md, "\n".join(markdown_ef(r) for r in doc["runs"]))):
            if path:
                os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
                with open(path, "w") as f:
                    f.write(body)
        return 1 if any(r[w][key] for run in doc["runs"] for r in run["sizes"] for w in EF_CALLS for key in ("plain_wrong", "residual_over_bound")) else 0
    doc = {"device": probe.device_props(groups[0][0])["name"], "rates": "GB/s (1e9 bytes/s)",
           "runs": [measure(g, sizes, a.dtype, a.iters, a.warmup, max(1, a.reps), a.wire) for g in groups]}
    text = json.dumps(doc)
    print(text)
    for path, body in ((a.out, text + "\n"), (a.md, "\n".join(markdown(r) for r in doc["runs"]))):
        if path:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            with open(path, "w") as f:
                f.write(body)
    return 1 if any(r[al][w] for run in doc["runs"] for r in run["sizes"] for al in pc.ALGOS if al in r
                    for w in ("thread_wrong", "driver_wrong")) else 0


if __name__ == "__main__":
    sys.exit(main())
