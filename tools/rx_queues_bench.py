#!/usr/bin/env python3
"""Measurement of xsk_gpu_rx_queues_dev against the sequence of calls it replaces: one gate, the rest
recorded.

Q independent queues, each with rings, pool, UMEM, workspace and outputs of its own (tools/rx_loop_fused_bench.py's
state, Q times).  Legs over the same states, interleaved in alternating order, five runs of ten repetitions:
  queues  ONE rx_queues_dev call over a block prepared once, outside the clock;
  seq     Q rx_loop_fused_dev calls on one stream, queue after queue: what a caller with Q queues does today (code this
          build shares with its parent);
  spread  the same Q calls dealt over 4 streams; enqueued only, never captured; reported, not gated.
Rows: Q in 1, 2, 8, 64, 256 x 64 mixed frames a queue and 1024 frames of 64 B a queue (max_batch the same), 8 ports and 9
completion rings with 64 entries each, at opts 0x17 and at opts 0; `queues` and `seq` as a graph replay (device events
around the replay) and all three as enqueued calls (the host clock from the first call to the end of a synchronisation,
when the rings are final).  Every repetition starts every queue from the same state (restored outside the clock) and the
tool asserts that the legs leave identical rings, words, pools, counters, results and UMEMs in every queue.

The gate: at Q = 8, 64 mixed frames, opts 0x17, graph replay, the median of `queues` (the median of the five runs'
medians) lies below the minimum of `seq`.  -> queues.jsonl; the lines carry the build id.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rx_step_steer_bench as B  # noqa: E402
from rx_loop_fused_bench import Both, host_timed, use_traffic  # noqa: E402
from rx_pass_bench import emit, same  # noqa: E402
from rx_step_steer_bench import X, in_turn, summary, timed  # noqa: E402

N_PORTS, USED, N_STREAMS = 8, 64, 4


class Queues:
    """Q states of n frames each, their workspaces, and the blocks of one call over all of them (one per option word)."""

    def __init__(self, q_n, n):
        self.n, self.s = n, [Both(n, N_PORTS, USED) for _ in range(q_n)]
        size = X.rx_pass_step_dev_workspace_size(n, N_PORTS)
        self.ws = [torch.zeros(size, dtype=torch.uint8, device=B.DEV) for _ in self.s]
        self.streams = [torch.cuda.Stream(device=B.DEV) for _ in range(N_STREAMS)]
        self.blocks = {}

    def block(self, opts):
        if opts not in self.blocks:
            recs = [X.rx_queue(s.umem, s.rx, s.fq, s.tx, s.stack, s.pl, self.n, s.table, s.n_entries, 0, s.c.rings, s.c.used,
                               ws, stats=s.stats, port_stats=s.port_stats, res=s.res, moved=s.c.moved, pushed=s.c.pushed)
                    for s, ws in zip(self.s, self.ws)]
            self.blocks[opts] = torch.from_numpy(X.rx_queues_prepare(recs, opts)).to(B.DEV)
        return self.blocks[opts]

    def queues(self, opts):
        X.rx_queues_dev(self.block(opts), len(self.s), opts)

    def seq(self, opts):
        for s, ws in zip(self.s, self.ws):
            s.call(X.rx_loop_fused_dev, self.n, ws, opts)

    def spread(self, opts):
        for k, (s, ws) in enumerate(zip(self.s, self.ws)):
            with torch.cuda.stream(self.streams[k % N_STREAMS]):
                s.call(X.rx_loop_fused_dev, self.n, ws, opts)

    def restore(self):
        for s in self.s:
            s.restore()

    def left(self):
        return [t for s in self.s for t in s.left()]


def measure(legs, qs, runs, reps, graph):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per_run = {k: [] for k in legs}
    for _ in range(runs):
        t = {k: [] for k in legs}
        for i in range(reps):
            left = {}
            for k, f in in_turn(legs, i):
                qs.restore()
                t[k].append(timed(f, e0, e1) if graph else host_timed(f))
                left[k] = qs.left()
            for k in legs:
                assert same(left["seq"], left[k]), f"{k} differs from seq"
        for k in legs:
            per_run[k].append(statistics.median(t[k]))
    return per_run


def row(qs, opts, graph, length, runs, reps, out):
    calls = {"queues": lambda: qs.queues(opts), "seq": lambda: qs.seq(opts)}
    if not graph:
        calls["spread"] = lambda: qs.spread(opts)
    legs = {}
    for k, f in calls.items():  # the kernels are loaded before the clock runs, and before a capture
        qs.restore()
        f()
        torch.cuda.synchronize()
        if graph:
            qs.restore()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                f()
            legs[k] = g.replay
        else:
            legs[k] = f
    per_run = measure(legs, qs, runs, reps, graph)
    line = dict(queues_n=len(qs.s), frames=qs.n, ports=N_PORTS, comp_rings=N_PORTS + 1, used=USED,
                entries=qs.s[0].n_entries, opts=opts, mode="graph" if graph else "enqueue",
                frame_bytes=length or "mixed", runs=runs, reps=reps, **{k: summary(v) for k, v in per_run.items()})
    emit(out, **line)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--queues", default="1,2,8,64,256")
    ap.add_argument("--shapes", default="64:0,1024:64", help="frames:frame bytes (0: the mixed batch), comma separated")
    ap.add_argument("--out", default="profiles/rx_queues")
    ap.add_argument("--append", action="store_true", help="add to queues.jsonl instead of starting it")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    gate, lines = None, []
    with open(os.path.join(a.out, "queues.jsonl"), "a" if a.append else "w") as f:
        for shape in a.shapes.split(","):
            n, length = (int(x) for x in shape.split(":"))
            use_traffic(length)
            for q_n in [int(x) for x in a.queues.split(",")]:
                qs = Queues(q_n, n)
                for opts in (0x17, 0):
                    for graph in (True, False):
                        line = row(qs, opts, graph, length, a.runs, a.reps, f)
                        lines.append(line)
                        if (q_n, n, length, opts, graph) == (8, 64, 0, 0x17, True):
                            gate = line
                del qs
                torch.cuda.empty_cache()
    for line in lines:  # t(Q) / t(1) of the new call, per shape, options and mode
        one = next((x for x in lines if x["queues_n"] == 1 and all(x[k] == line[k] for k in ("frames", "frame_bytes", "opts", "mode"))), None)
        if one is not None and line["queues_n"] > 1:
            print(f"t({line['queues_n']}) / t(1), {line['frames']} x {line['frame_bytes']}, opts {line['opts']:#x}, "
                  f"{line['mode']}: {line['queues']['median_us'] / one['queues']['median_us']:.2f}", flush=True)
    if gate is not None:
        ok = gate["queues"]["median_us"] < gate["seq"]["min_us"]
        print(f"gate (8 queues, 64 mixed frames, 8 ports, 9 rings, opts 0x17, graph replay): queues median "
              f"{gate['queues']['median_us']} us against seq min {gate['seq']['min_us']} us: {'met' if ok else 'MISSED'}",
              flush=True)
        if not ok:
            sys.exit(1)


if __name__ == "__main__":
    main()
