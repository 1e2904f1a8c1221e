#!/usr/bin/env python3
"""Measurement of xsk_gpu_responder_dev and xsk_gpu_responder_queues_dev against the calls they replace (DESIGN.md
§9.15): recorded, no gate, no number fixed in advance -- the comparison is with the existing calls of the same build, in
the same process.

One queue's world: 64 mixed frames offered, 8 of them ARP requests or neighbour solicitations for table addresses, the
rest echo requests; 8 ports, 16 entries in the steering table and 16 in the neighbour table, 4 completion rings, 2048-B
chunks, opts 0x17 (tests/responder_dev.hand_world, the GPU tests' own state).

  row "one"     one queue: `two` is rx_loop_fused_dev followed by neigh_serve_dev, `one` is responder_dev.
  row "queues"  the same world per queue at Q queues: `two` is ONE rx_queues_dev call followed by Q neigh_serve_dev calls
                on one stream, `one` is ONE responder_queues_dev call; both blocks prepared once, outside the clock.
Each row twice: mode "enqueue" (the host clock from the first call to the end of a synchronisation) and mode "graph"
(each leg captured once; `*_dev` is the time between device events around the replay, the plain name the host clock
around replay and synchronise).  Legs interleaved in alternating order, five runs of ten repetitions, the median of the
runs' medians with min .. max.  Every repetition starts from the same state (restored outside the clock) and the tool
asserts that the legs leave identical rings, index words, pools, outputs and UMEMs.  -> responder.jsonl; the lines carry
the build id.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rx_step_steer_bench import X, emit, in_turn, summary, timed  # noqa: E402
from tests.responder_dev import RLeg, echo4, hand_world, responder_block, solicit, who_has  # noqa: E402
from tests.test_gpu_rx_queues import block_of  # noqa: E402

OPTS, FRAMES, REQUESTS = 0x17, 64, 8


def offer(k):
    """64 frames, every eighth a request (ARP and solicitation in turn), the ports interleaved; k shifts the ports."""
    return [(who_has if (i // 8) % 2 else solicit)((i // 8 + k) % 8) if i % 8 == 3 else echo4((i + k) % 8, i)
            for i in range(FRAMES)]


class Queues:
    """Q worlds on the device, what restores them, and the two blocks."""

    def __init__(self, q_n):
        self.legs = [RLeg(hand_world(offer(k), n_comp=4)) for k in range(q_n)]
        self.recs = [leg.responder_record() for leg in self.legs]
        self.block = responder_block(self.legs, OPTS)
        self.rq_block = block_of(self.legs, self.legs, [leg.umem.data for leg in self.legs], OPTS)
        torch.cuda.synchronize()
        self.bufs = [g.buf for leg in self.legs for g in leg.guards()]
        self.kept = [g.buf for leg in self.legs for g in leg.guards() if g is not leg.ws]  # all but the workspaces
        self.saved = [b.clone() for b in self.bufs]

    def restore(self):
        for b, s in zip(self.bufs, self.saved):
            b.copy_(s)
        torch.cuda.synchronize()

    def left(self):
        return [b.clone() for b in self.kept]

    def two_one_queue(self):
        self.legs[0].fused()

    def one_one_queue(self):
        X.responder_dev(self.recs[0], OPTS)

    def two(self):
        X.rx_queues_dev(self.rq_block, len(self.legs), OPTS)
        for leg in self.legs:
            leg.serve()

    def one(self):
        X.responder_queues_dev(self.block, len(self.legs), OPTS)


def host_timed(f):
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def row(name, qs, calls, graph, runs, reps, out):
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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    keys = list(legs) + ([k + "_dev" for k in legs] if graph else [])
    per_run = {k: [] for k in keys}
    for _ in range(runs):
        t = {k: [] for k in keys}
        for i in range(reps):
            left = {}
            for k, f in in_turn(legs, i):
                qs.restore()
                t[k].append(host_timed(f))
                left[k] = qs.left()
                if graph:
                    qs.restore()
                    t[k + "_dev"].append(timed(f, e0, e1))
            assert all(torch.equal(a, b) for a, b in zip(left["two"], left["one"])), "the legs leave different state"
        for k in keys:
            per_run[k].append(statistics.median(t[k]))
    res = qs.legs[0].nres.get(X.NEIGH_RESULT_DTYPE)[0]
    assert int(res["consumed"]) == REQUESTS and int(res["arp_replies"]) + int(res["na_replies"]) == REQUESTS
    emit(out, row=name, queues_n=len(qs.legs) if name == "queues" else 1, frames=FRAMES, requests=REQUESTS, ports=8,
         comp_rings=4, opts=OPTS, mode="graph" if graph else "enqueue", runs=runs, reps=reps,
         launches_two=(2 if name == "one" else 1 + len(qs.legs)), launches_one=1,
         **{k: summary(v) for k, v in per_run.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--queues", default="8,64")
    ap.add_argument("--out", default="profiles/responder")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "responder.jsonl"), "w") as f:
        qs = Queues(1)
        for graph in (False, True):
            row("one", qs, {"two": qs.two_one_queue, "one": qs.one_one_queue}, graph, a.runs, a.reps, f)
        for q_n in [int(x) for x in a.queues.split(",")]:
            del qs
            torch.cuda.empty_cache()
            qs = Queues(q_n)
            for graph in (False, True):
                row("queues", qs, {"two": qs.two, "one": qs.one}, graph, a.runs, a.reps, f)


if __name__ == "__main__":
    main()
