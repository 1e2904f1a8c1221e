#!/usr/bin/env python3
"""Measurement of xsk_gpu_tx_complete_rings_dev and xsk_gpu_rx_loop_dev: one gate, the rest recorded.

(a) Every completion ring of a caller drained into the pool, device events around the calls, two legs interleaved:
      single  n calls of tx_complete_dev, ring after ring (code this build shares with its parent);
      rings   the one call of tx_complete_rings_dev.
    1, 8 and 65 rings x 64 and 1024 used entries per ring (max 1024: the one-workgroup path), 65 x 1300 (max 1300: the
    copy grid and the publish launch), a pool with room for all; one row (65 x 64) with a pool that cuts the list in
    half.  Every repetition starts from the same state (restored outside the clock) and the tool asserts that the legs
    leave identical consumer words, pool count and pool entries.  The gate: at 65 rings x 64 entries the median of
    `rings` lies below the minimum of `single`.  -> complete.jsonl
(b) The whole loop body as a graph replay: rx_loop_dev against rx_pass_step_dev followed by a tx_complete_dev node per
    ring, at 8 ports (9 completion rings) and 64 ports (65), 64 entries on every completion ring; device events around
    the replay; the legs leave identical rings, words, counters, pool and UMEM.  -> loop.jsonl
Traffic, tables, rings, runs and repetitions of (b) are those of tools/rx_pass_bench.py; the lines carry the build id.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rx_pass_bench import PassState, emit, same  # noqa: E402
from rx_step_steer_bench import DEV, OPTS, X, in_turn, pow2_at_least, summary, timed  # noqa: E402


class Comps:
    """n_rings completion rings of `size` entries holding `used` each (consumer words three below 2^32), and a pool of
    `below` frames with `room` free entries."""

    def __init__(self, n_rings, used, room, below=16):
        self.n, self.used, size = n_rings, used, pow2_at_least(used)
        cons = np.full(n_rings, 0xFFFFFFFD, np.uint64)
        w = np.stack([(cons + used) & 0xFFFFFFFF, cons], 1).astype(np.uint32).reshape(-1)
        self.words = torch.from_numpy(w.view(np.int32)).to(DEV)
        self.ent = (torch.arange(n_rings * size, dtype=torch.int64, device=DEV) + (1 << 24)) * 2048
        self.cap = below + room
        self.pool = (torch.arange(self.cap, dtype=torch.int64, device=DEV) + (1 << 20)) * 4096
        self.pool_w = torch.tensor([below], dtype=torch.int32, device=DEV)
        self.moved = torch.zeros(n_rings, dtype=torch.int32, device=DEV)
        self.pushed = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.mutable = [self.words, self.pool, self.pool_w]
        torch.cuda.synchronize()
        self.saved = [t.clone() for t in self.mutable]
        self.rings = [X.RingDev.of(self.words[2 * q:2 * q + 1], self.words[2 * q + 1:2 * q + 2],
                                   self.ent[q * size:(q + 1) * size], size) for q in range(n_rings)]
        self.pl = X.PoolDev.of(self.pool, self.pool_w, self.cap)

    def restore(self):
        for t, s in zip(self.mutable, self.saved):
            t.copy_(s)
        self.moved.zero_()
        torch.cuda.synchronize()

    def final(self):
        n = int(self.pool_w.cpu().numpy().view(np.uint32)[0])
        return [self.words.clone(), self.pool_w.clone(), self.moved.clone(), self.pool[:n].clone()]

    def single(self, mx):
        for q, r in enumerate(self.rings):
            X.tx_complete_dev(r, self.pl, mx, moved=self.moved[q:q + 1])

    def all_rings(self, mx):
        X.tx_complete_rings_dev(self.rings, self.pl, mx, moved=self.moved, pushed=self.pushed)


def measure(legs, restore, final, runs, reps):
    """Five runs of ten repetitions by default: per leg the median of every run; the legs' final states compared every
    repetition."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per_run = {k: [] for k in legs}
    for _ in range(runs):
        t = {k: [] for k in legs}
        for i in range(reps):
            left = {}
            for k, f in in_turn(legs, i):
                restore()
                t[k].append(timed(f, e0, e1))
                left[k] = final()
            first = next(iter(legs))
            for k in legs:
                assert same(left[first], left[k]), f"{k} differs from {first}"
        for k in legs:
            per_run[k].append(statistics.median(t[k]))
    return per_run


def row_a(n_rings, used, mx, cut, runs, reps, out):
    total = n_rings * min(used, mx)
    c = Comps(n_rings, used, total // 2 if cut else total + 64)
    legs = {"single": lambda: c.single(mx), "rings": lambda: c.all_rings(mx)}
    for f in legs.values():  # the kernels are loaded before the clock runs
        c.restore()
        f()
    per_run = measure(legs, c.restore, c.final, runs, reps)
    pushed = int(c.pushed.cpu().numpy().view(np.uint32)[0])
    assert pushed == (total // 2 if cut else total)
    line = dict(row="a", n_rings=n_rings, used=used, max=mx, pool_cut=cut, pushed=pushed, runs=runs, reps=reps,
                **{k: summary(v) for k, v in per_run.items()})
    emit(out, **line)
    return line


class LoopState(PassState):
    """rx_pass_bench's state with a completion ring per port and the stack consumer's, `used` entries on each, and a
    pool grown by room for all of them."""

    def __init__(self, n_frames, n_ports, used):
        super().__init__(n_frames, pow2_at_least(2 * n_frames), pow2_at_least(n_frames), n_ports, pow2_at_least(n_frames))
        self.c = Comps(n_ports + 1, used, 0, below=0)
        cap = 2 * self.size + (n_ports + 1) * used
        pool = (torch.arange(cap, dtype=torch.int64, device=DEV) + (1 << 20)) * 4096
        at = next(i for i, t in enumerate(self.mutable) if t is self.pool)
        self.pool = self.mutable[at] = pool
        self.mutable.append(self.c.words)
        torch.cuda.synchronize()
        self.saved[at] = pool.clone()
        self.saved.append(self.c.words.clone())
        self.pl = X.PoolDev.of(self.pool, self.pool_w, cap)

    def everything(self):
        return self.common() + self.final()[-1:] + [self.pool_w.clone(), self.c.words.clone()]

    def steps(self, n, ws):
        self.pass_step(n, ws)
        for r in self.c.rings:
            X.tx_complete_dev(r, self.pl, self.c.used)

    def loop(self, n, ws):
        X.rx_loop_dev(self.umem, self.rx, self.fq, self.tx, self.stack, self.pl, n, self.table, self.n_entries, 0,
                      self.c.rings, self.c.used, ws, stats=self.stats, port_stats=self.port_stats, res=self.res, opts=OPTS)


def row_b(n, n_ports, used, runs, reps, out):
    s = LoopState(n, n_ports, used)
    ws = torch.zeros(X.rx_pass_step_dev_workspace_size(n, n_ports), dtype=torch.uint8, device=DEV)
    graphs = {}
    for k, f in (("step_then_singles", s.steps), ("loop", s.loop)):
        s.restore()
        f(n, ws)
        torch.cuda.synchronize()
        s.restore()
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            f(n, ws)
    legs = {k: g.replay for k, g in graphs.items()}
    per_run = measure(legs, s.restore, s.everything, runs, reps)
    emit(out, row="b", frames=n, ports=n_ports, comp_rings=n_ports + 1, used=used, entries=s.n_entries, opts=OPTS,
         runs=runs, reps=reps, **{k: summary(v) for k, v in per_run.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="a,b")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", default="64,1024")
    ap.add_argument("--out", default="profiles/tx_complete_rings")
    a = ap.parse_args()
    rows = a.rows.split(",")
    os.makedirs(a.out, exist_ok=True)
    gate = None
    if "a" in rows:
        with open(os.path.join(a.out, "complete.jsonl"), "w") as f:
            for n_rings in (1, 8, 65):
                for used in (64, 1024):
                    line = row_a(n_rings, used, 1024, False, a.runs, a.reps, f)
                    if (n_rings, used) == (65, 64):
                        gate = line
            row_a(65, 1300, 1300, False, a.runs, a.reps, f)
            row_a(65, 64, 1024, True, a.runs, a.reps, f)
    if "b" in rows:
        with open(os.path.join(a.out, "loop.jsonl"), "w") as f:
            for n in [int(x) for x in a.frames.split(",")]:
                for n_ports in (8, 64):
                    row_b(n, n_ports, 64, a.runs, a.reps, f)
    if gate is not None:
        ok = gate["rings"]["median_us"] < gate["single"]["min_us"]
        print(f"gate (65 rings x 64 entries): rings median {gate['rings']['median_us']} us against single min "
              f"{gate['single']['min_us']} us: {'met' if ok else 'MISSED'}", flush=True)
        if not ok:
            sys.exit(1)


if __name__ == "__main__":
    main()
