#!/usr/bin/env python3
"""Measurement of xsk_gpu_rx_pass_step_dev: recorded, no gate.

(a) One steered RX loop step that keeps the frames the filter passes to the kernel stack, host clock from the first
    call until the rings are final (a synchronisation), three legs interleaved:
      host    what a caller needed before the stack ring existed: rx_step_steer_dev with d_actions given, synchronise,
              D2H of the result, the actions and the batch's RX entries, the list of PASS descriptors built in numpy,
              H2D onto the stack ring and its producer word, synchronise;
      enq     rx_pass_step_dev enqueued;
      graph   rx_pass_step_dev as a graph replay.
    Every repetition starts from the same state (restored outside the clock) and the tool asserts that the three legs
    leave identical rings (the stack ring among them), words, counters and UMEM.  The pool is compared among enq and
    graph only: in the host leg the PASS frames' chunks are on the stack ring AND back on the pool, which is the hole
    the stack ring closes.  -> step.jsonl
(b) The price of the stack ring: device events around back-to-back calls over a ring holding that many batches,
    rx_pass_step_dev (a stack ring with room for every PASS frame) against rx_step_steer_dev in the same build; the
    legs leave the same RX, fill and TX rings, counters and UMEM.  -> price.jsonl
--trace runs each leg of (b) 21 times at every size and port count given, a restore and a synchronise between calls, and
nothing else: the workload of a `rocprofv3 --kernel-trace --stats` run of its own (the legs' end kernels have names of
their own, rx_end_ports_* and rx_pass_end_*; everything in front of them is the same four calls).
Traffic, tables, rings, runs and repetitions are those of tools/rx_step_steer_bench.py (opts 0x17, default port 0);
the lines carry the build id and the number of PASS frames.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rx_step_steer_bench import DEV, OPTS, State, X, in_turn, pow2_at_least, put_words, summary, timed, words  # noqa: E402

PASS = 2


class PassState(State):
    """State with an empty stack ring of stack_size descriptors and a d_actions array of n_frames bytes."""

    def __init__(self, n_frames, size, tx_size, n_ports, stack_size, fill_used=None):
        super().__init__(n_frames, size, tx_size, n_ports, fill_used)
        self.stack_size = stack_size
        self.stack_w = words(0, 0)
        self.stack_ent = torch.zeros(stack_size * 16, dtype=torch.uint8, device=DEV)
        self.actions = torch.zeros(n_frames, dtype=torch.uint8, device=DEV)
        self.mutable += [self.stack_w, self.stack_ent]
        torch.cuda.synchronize()
        self.saved += [self.stack_w.clone(), self.stack_ent.clone()]
        self.stack = X.RingDev.of(self.stack_w[0:1], self.stack_w[1:2], self.stack_ent, stack_size)

    def common(self):
        """What every leg must leave alike, as device copies: State.final() without the pool, and the stack ring last."""
        return [t.clone() for t in (self.rx_w, self.fq_w, self.tx_w, self.fq_ent, self.tx_ent, self.umem, self.stats,
                                    self.port_stats, self.stack_w, self.stack_ent)]

    def pass_step(self, max_batch, ws):
        X.rx_pass_step_dev(self.umem, self.rx, self.fq, self.tx, self.stack, self.pl, max_batch, self.table,
                           self.n_entries, 0, ws, stats=self.stats, port_stats=self.port_stats, res=self.res, opts=OPTS)

    def steer_step(self, max_batch, ws, actions=None):
        X.rx_step_steer_dev(self.umem, self.rx, self.fq, self.tx, self.pl, max_batch, self.table, self.n_entries, 0, ws,
                            actions=actions, stats=self.stats, port_stats=self.port_stats, res=self.res, opts=OPTS)


def host_leg(s: PassState, n, ws):
    """The steered step, then the PASS list by way of the host."""
    rx_cons = 0  # (every repetition starts there; a caller tracks its ring's consumer index)
    s.steer_step(n, ws, s.actions)
    torch.cuda.synchronize()
    rcvd = int(s.res.cpu().numpy().view(np.uint32)[0])
    if rcvd == 0:
        return
    act = s.actions[:rcvd].cpu().numpy()
    descs = s.rx_ent.cpu().numpy().view(X.DESC_DTYPE)[(rx_cons + np.arange(rcvd)) & (s.size - 1)]
    sw = s.stack_w.cpu().numpy().view(np.uint32).astype(np.int64)
    room = s.stack_size - min(int((sw[0] - sw[1]) & 0xFFFFFFFF), s.stack_size)
    keep = np.ascontiguousarray(descs[act == PASS][:room])
    if len(keep):
        lo = int(sw[0]) & (s.stack_size - 1)
        assert lo + len(keep) <= s.stack_size  # (the ring starts empty at index 0: one contiguous copy)
        s.stack_ent[lo * 16:(lo + len(keep)) * 16].copy_(torch.from_numpy(keep.view(np.uint8).reshape(-1)))
        put_words(s.stack_w, sw[0] + len(keep), sw[1])
    torch.cuda.synchronize()


def emit(out, **line):
    line["build_id"] = X.build_id()
    out.write(json.dumps(line) + "\n")
    out.flush()
    print(json.dumps(line), flush=True)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def row_a(n, n_ports, runs, reps, out):
    s = PassState(n, pow2_at_least(2 * n), pow2_at_least(n), n_ports, pow2_at_least(n))
    ws = torch.zeros(X.rx_pass_step_dev_workspace_size(n, n_ports), dtype=torch.uint8, device=DEV)

    def enq():
        s.pass_step(n, ws)
        torch.cuda.synchronize()

    s.restore()
    enq()
    s.restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.pass_step(n, ws)

    def rep():
        graph.replay()
        torch.cuda.synchronize()

    legs = {"host": lambda: host_leg(s, n, ws), "enq": enq, "graph": rep}
    per_run = {k: [] for k in legs}
    for _ in range(runs):
        t = {k: [] for k in legs}
        for i in range(reps):
            common, pools = {}, {}
            for k, f in in_turn(legs, i):
                s.restore()
                t0 = time.perf_counter()
                f()
                t[k].append((time.perf_counter() - t0) * 1e6)
                common[k], pools[k] = s.common(), s.final()[-1]
            for k in ("enq", "graph"):
                assert same(common["host"], common[k]), f"{k} differs from the host leg"
            assert torch.equal(pools["enq"], pools["graph"]), "the replay's pool differs from the enqueued call's"
        for k in legs:
            per_run[k].append(statistics.median(t[k]))
    s.restore()
    enq()
    r = s.res.cpu().numpy().view(np.uint32)
    emit(out, row="a", frames=n, ports=n_ports, entries=s.n_entries, opts=OPTS, ring=s.size, runs=runs, reps=reps,
         redirected=int(r[1]), replied=int(r[2]), freed=int(r[5]), passed=int(r[6]), pass_full=int(r[7]),
         **{k: summary(v) for k, v in per_run.items()})


def row_b(n, n_ports, runs, reps, out, calls):
    size = pow2_at_least(calls * n)
    s = PassState(calls * n, size, size, n_ports, size, fill_used=size)  # a full fill ring: no refill inside the window
    ws = torch.zeros(X.rx_pass_step_dev_workspace_size(n, n_ports), dtype=torch.uint8, device=DEV)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def steer():
        for _ in range(calls):
            s.steer_step(n, ws)

    def stack():
        for _ in range(calls):
            s.pass_step(n, ws)

    legs = {"steer": steer, "pass": stack}
    per_run = {k: [] for k in legs}
    passed = 0
    for _ in range(runs):
        t = {k: [] for k in legs}
        for i in range(reps):
            common = {}
            for k, f in in_turn(legs, i):
                s.restore()
                t[k].append(timed(f, e0, e1) / calls)
                assert int(s.rx_w.cpu().numpy().view(np.uint32)[1]) == calls * n  # every call had a full batch
                common[k] = s.common()[:-2]  # (the stack ring is the difference)
                if k == "pass":
                    passed = int(s.stack_w.cpu().numpy().view(np.uint32)[0])
            assert same(common["steer"], common["pass"]), "the stack ring changed what the step leaves elsewhere"
        for k in legs:
            per_run[k].append(statistics.median(t[k]))
    emit(out, row="b", frames=n, ports=n_ports, entries=s.n_entries, opts=OPTS, calls=calls, runs=runs, reps=reps,
         passed_per_call=passed / calls, **{k: summary(v) for k, v in per_run.items()})


def trace(n, n_ports, calls=21):
    s = PassState(n, pow2_at_least(2 * n), pow2_at_least(n), n_ports, pow2_at_least(n))
    ws = torch.zeros(X.rx_pass_step_dev_workspace_size(n, n_ports), dtype=torch.uint8, device=DEV)
    for leg in (s.steer_step, s.pass_step):
        for _ in range(calls):
            s.restore()
            leg(n, ws)
            torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024,65536")
    ap.add_argument("--ports", default="1,8,64")
    ap.add_argument("--rows", default="a,b")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="profiles/rx_pass")
    ap.add_argument("--trace", action="store_true", help="run both legs of (b) a few times and exit (for rocprofv3)")
    a = ap.parse_args()
    sizes, ports, rows = [int(x) for x in a.sizes.split(",")], [int(x) for x in a.ports.split(",")], a.rows.split(",")
    if a.trace:
        for n in sizes:
            for p in ports:
                trace(n, p)
        return
    os.makedirs(a.out, exist_ok=True)
    if "a" in rows:
        with open(os.path.join(a.out, "step.jsonl"), "w") as f:
            for n in sizes:
                for p in ports:
                    row_a(n, p, a.runs, a.reps, f)
    if "b" in rows:
        with open(os.path.join(a.out, "price.jsonl"), "w") as f:
            for n in sizes:
                for p in ports:
                    if n * p <= 65536 * 8:  # (64 ports at 65 536 frames: rings for all the calls' replies are not held)
                        row_b(n, p, a.runs, a.reps, f, calls=10 if n <= 1024 else 4)


if __name__ == "__main__":
    main()
