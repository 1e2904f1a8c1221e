#!/usr/bin/env python3
"""Measurement of xsk_gpu_rx_fused_loop_dev against xsk_gpu_rx_loop_dev: one gate, the rest recorded.

Two legs over the same state, interleaved in alternating order, five runs of ten repetitions:
  loop   rx_loop_dev, the chain of launches (code this build shares with its parent);
  fused  rx_loop_fused_dev, the one launch.
Rows: 64 and 1024 frames on the RX ring (max_batch the same) x 8 ports with 9 completion rings and 64 ports with 65, 64
entries on every completion ring; at opts 0x17 and at opts 0; as a graph replay (device events around the replay) and as
enqueued calls (the host clock from the call to the end of a synchronisation, when the rings are final).  Traffic: the
mixed dual-stack batch of tools/rx_pass_bench.py; the 1024-frame rows also with frames of 64 B and of 1500 B (IPv4 and
IPv6 echo requests in turn, one destination per family).  Every repetition starts from the same state (restored outside
the clock) and the tool asserts that both legs leave identical rings, words, pool, counters, results and UMEM.

The gate: at 64 frames, 8 ports, 9 rings, opts 0x17, mixed traffic, graph replay, the fused call's median of the five
runs' medians lies below the loop call's minimum.  -> loop.jsonl; the lines carry the build id.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rx_step_steer_bench as B  # noqa: E402
from rx_pass_bench import emit, same  # noqa: E402
from rx_step_steer_bench import STRIDE, X, in_turn, summary, timed  # noqa: E402
from tx_complete_rings_bench import LoopState  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import steer_spec as SS  # noqa: E402
from tests import stream_paths as S  # noqa: E402


def use_traffic(length):
    """The base batch the states tile from: tools/rx_step_steer_bench.py's mixed one (length 0), or 1024 echo requests
    of `length` bytes, IPv4 and IPv6 in turn."""
    B._BASE.clear()
    if not length:
        return
    frames = [S.frame(bool(i & 1), length, "random", length, i) for i in range(1024)]
    umem, descs = S.place(frames, [0] * len(frames), STRIDE)
    descs = np.ascontiguousarray(descs, X.DESC_DTYPE)
    B._BASE.update(umem=umem, descs=descs, keys=SS.destinations(umem, descs, B.OPTS))


class Both(LoopState):
    """tools/tx_complete_rings_bench.py's loop state, either call with every output given."""

    def call(self, fn, n, ws, opts):
        fn(self.umem, self.rx, self.fq, self.tx, self.stack, self.pl, n, self.table, self.n_entries, 0, self.c.rings,
           self.c.used, ws, stats=self.stats, port_stats=self.port_stats, res=self.res, moved=self.c.moved,
           pushed=self.c.pushed, opts=opts)

    def left(self):
        return self.everything() + [self.res.clone(), self.c.moved.clone(), self.c.pushed.clone()]


def host_timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def measure(legs, s, runs, reps, graph):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per_run = {k: [] for k in legs}
    for _ in range(runs):
        t = {k: [] for k in legs}
        for i in range(reps):
            left = {}
            for k, f in in_turn(legs, i):
                s.restore()
                t[k].append(timed(f, e0, e1) if graph else host_timed(f))
                left[k] = s.left()
            assert same(left["loop"], left["fused"]), "the legs differ"
        for k in legs:
            per_run[k].append(statistics.median(t[k]))
    return per_run


def row(n, n_ports, opts, graph, length, runs, reps, out):
    s = Both(n, n_ports, 64)
    ws = torch.zeros(X.rx_pass_step_dev_workspace_size(n, n_ports), dtype=torch.uint8, device=B.DEV)
    calls = {"loop": lambda: s.call(X.rx_loop_dev, n, ws, opts), "fused": lambda: s.call(X.rx_loop_fused_dev, n, ws, opts)}
    legs = {}
    for k, f in calls.items():  # the kernels are loaded before the clock runs, and before a capture
        s.restore()
        f()
        torch.cuda.synchronize()
        if graph:
            s.restore()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                f()
            legs[k] = g.replay
        else:
            legs[k] = f
    per_run = measure(legs, s, runs, reps, graph)
    res = s.res.cpu().numpy().view(np.uint32)
    line = dict(frames=n, ports=n_ports, comp_rings=n_ports + 1, used=64, entries=s.n_entries, opts=opts,
                mode="graph" if graph else "enqueue", frame_bytes=length or "mixed", received=int(res[0]),
                redirected=int(res[1]), replied=int(res[2]), runs=runs, reps=reps,
                **{k: summary(v) for k, v in per_run.items()})
    emit(out, **line)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", default="64,1024")
    ap.add_argument("--out", default="profiles/rx_loop_fused")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    gate = None
    with open(os.path.join(a.out, "loop.jsonl"), "w") as f:
        for n in [int(x) for x in a.frames.split(",")]:
            for length in ((0,) if n < 1024 else (0, 64, 1500)):
                use_traffic(length)
                for n_ports in (8, 64):
                    for opts in (0x17, 0):
                        for graph in (True, False):
                            line = row(n, n_ports, opts, graph, length, a.runs, a.reps, f)
                            if (n, n_ports, opts, graph, length) == (64, 8, 0x17, True, 0):
                                gate = line
    if gate is not None:
        ok = gate["fused"]["median_us"] < gate["loop"]["min_us"]
        print(f"gate (64 frames, 8 ports, 9 rings, opts 0x17, graph replay): fused median {gate['fused']['median_us']} us "
              f"against loop min {gate['loop']['min_us']} us: {'met' if ok else 'MISSED'}", flush=True)
        if not ok:
            sys.exit(1)


if __name__ == "__main__":
    main()
