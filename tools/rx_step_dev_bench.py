#!/usr/bin/env python3
"""Measurement of xsk_gpu_rx_step_dev: recorded, no gate.

(a) One RX loop step with rings, pool and UMEM in device memory, host clock from the first call until the rings are
    final (a synchronisation), three legs interleaved:
      host    what the library offered before: synchronise, D2H of the index words and RX entries, host linearisation
              (numpy), H2D, echo_dev(opts) + egress_dev, synchronise, D2H of the lists, ring and pool writes on the
              host, H2D;
      enq     rx_step_dev enqueued;
      graph   rx_step_dev as a graph replay.
    Every repetition starts from the same state (restored outside the clock) and the tool asserts that the three legs
    leave identical rings, words and pool.
(b) The price of the ring glue: device events around 20 back-to-back rx_step_dev calls over a ring holding 20 batches,
    against echo_dev_indirect + egress_dev alone over the same frames.
Five runs of ten repetitions; the lines go to <out>/step.jsonl and <out>/glue.jsonl with the build id.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import xsknet_amd as X  # noqa: E402

STRIDE = 2048
DEV = torch.device("cuda:0")


def pow2_at_least(n):
    p = 1
    while p < n:
        p *= 2
    return p


def words(*v):
    return torch.tensor(np.array(v, np.uint32).view(np.int32), dtype=torch.int32, device=DEV)


class State:
    """n_frames mixed frames on an RX ring of `size` entries, empty TX ring, half-full fill ring, a pool of size frames."""

    def __init__(self, n_frames, size, opts):
        self.size, self.opts = size, opts
        self.umem = torch.zeros(n_frames * STRIDE, dtype=torch.uint8, device=DEV)
        self.rx_ent = torch.zeros(size * 16, dtype=torch.uint8, device=DEV)
        X.synth_dev(self.umem, self.rx_ent, n_frames, 0, STRIDE, 0x5EED0001, 0, 1, 1, 20, 1500)
        self.rx_w, self.fq_w, self.tx_w = words(n_frames, 0), words(size // 2, 0), words(0, 0)
        self.fq_ent = torch.zeros(size * 8, dtype=torch.uint8, device=DEV)
        self.tx_ent = torch.zeros(size * 16, dtype=torch.uint8, device=DEV)
        self.pool = (torch.arange(size, dtype=torch.int64, device=DEV) + (1 << 20)) * 4096
        self.pool_w = words(size // 2)
        self.stats = torch.zeros(40, dtype=torch.uint8, device=DEV)
        self.res = torch.zeros(16, dtype=torch.uint8, device=DEV)
        self.mutable = [self.umem, self.rx_w, self.fq_w, self.tx_w, self.fq_ent, self.tx_ent, self.pool, self.pool_w]
        torch.cuda.synchronize()
        self.saved = [t.clone() for t in self.mutable]
        self.rx = X.RingDev.of(self.rx_w[0:1], self.rx_w[1:2], self.rx_ent, size)
        self.fq = X.RingDev.of(self.fq_w[0:1], self.fq_w[1:2], self.fq_ent, size)
        self.tx = X.RingDev.of(self.tx_w[0:1], self.tx_w[1:2], self.tx_ent, size)
        self.pl = X.PoolDev.of(self.pool, self.pool_w, size)

    def restore(self):
        for t, s in zip(self.mutable, self.saved):
            t.copy_(s)
        self.stats.zero_()
        torch.cuda.synchronize()

    def final(self):
        """Everything a step leaves, as device copies (the pool below its count)."""
        n = int(self.pool_w.cpu().numpy().view(np.uint32)[0])
        return [t.clone() for t in (self.rx_w, self.fq_w, self.tx_w, self.fq_ent, self.tx_ent, self.pool_w, self.umem,
                                    self.stats)] + [self.pool[:n].clone()]


def host_leg(s: State, n, bufs):
    """The step as a caller of the earlier API had to do it."""
    size, mask = s.size, s.size - 1
    torch.cuda.synchronize()
    rxw, fqw, txw = (t.cpu().numpy().view(np.uint32) for t in (s.rx_w, s.fq_w, s.tx_w))
    pool_n = int(s.pool_w.cpu().numpy().view(np.uint32)[0])
    rcvd = min(int((int(rxw[0]) - int(rxw[1])) & 0xFFFFFFFF), n)
    if rcvd == 0:
        return
    ring = s.rx_ent.cpu().numpy().view(X.DESC_DTYPE)
    descs = ring[(int(rxw[1]) + np.arange(rcvd)) & mask]          # linearise
    stock = min(size - int((int(fqw[0]) - int(fqw[1])) & 0xFFFFFFFF), pool_n)
    room = size - int((int(txw[0]) - int(txw[1])) & 0xFFFFFFFF)
    d_descs, d_verd, d_tx, d_free, d_counts, d_room, ews = bufs
    d_descs[:rcvd * 16].copy_(torch.from_numpy(descs.view(np.uint8).reshape(-1)))
    d_room.copy_(torch.from_numpy(np.array([room], np.uint32).view(np.int32)))
    X.echo_dev(s.umem, d_descs, rcvd, d_verd, None, s.stats, bufs_ws(s, rcvd), opts=s.opts)
    X.egress_dev(d_descs, d_verd, rcvd, d_tx, d_free, d_counts, tx_room=d_room, stats=s.stats, workspace=ews)
    torch.cuda.synchronize()
    c = d_counts.cpu().numpy().view(np.uint32)
    n_tx, n_free = int(c[1]), int(c[3])
    tx_list = d_tx[:n_tx * 16].cpu().numpy().view(X.DESC_DTYPE)
    free_list = d_free[:n_free * 8].cpu().numpy().view(np.uint64)
    pool = s.pool.cpu().numpy().view(np.uint64).copy()
    fq = s.fq_ent.cpu().numpy().view(np.uint64).copy()
    txr = s.tx_ent.cpu().numpy().view(X.DESC_DTYPE).copy()
    fq[(int(fqw[0]) + np.arange(stock)) & mask] = pool[pool_n - 1 - np.arange(stock)]
    pool_n -= stock
    txr[(int(txw[0]) + np.arange(n_tx)) & mask] = tx_list
    pushed = min(n_free, size - pool_n)
    pool[pool_n:pool_n + pushed] = free_list[:pushed]
    pool_n += pushed
    s.fq_ent.copy_(torch.from_numpy(fq.view(np.uint8)))
    s.tx_ent.copy_(torch.from_numpy(txr.view(np.uint8).reshape(-1)))
    s.pool.copy_(torch.from_numpy(pool.view(np.int64)))
    s.pool_w.copy_(torch.from_numpy(np.array([pool_n], np.uint32).view(np.int32)))
    s.fq_w.copy_(torch.from_numpy(np.array([int(fqw[0]) + stock, fqw[1]], np.uint32).view(np.int32)))
    s.tx_w.copy_(torch.from_numpy(np.array([int(txw[0]) + n_tx, txw[1]], np.uint32).view(np.int32)))
    s.rx_w.copy_(torch.from_numpy(np.array([rxw[0], int(rxw[1]) + rcvd], np.uint32).view(np.int32)))
    torch.cuda.synchronize()


_WS = {}


def bufs_ws(s, n):
    if n not in _WS:
        _WS[n] = torch.zeros(max(X.workspace_size(0, n), 16), dtype=torch.uint8, device=DEV)
    return _WS[n]


def summary(v):
    return dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))


def row_a(n, opts, runs, reps, out):
    s = State(n, pow2_at_least(2 * n), opts)
    ws = torch.zeros(X.rx_step_dev_workspace_size(n), dtype=torch.uint8, device=DEV)
    bufs = (torch.zeros(n * 16, dtype=torch.uint8, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV),
            torch.zeros(n * 16, dtype=torch.uint8, device=DEV), torch.zeros(n * 8, dtype=torch.uint8, device=DEV),
            torch.zeros(16, dtype=torch.uint8, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
            torch.zeros(max(X.egress_workspace_size(n), 4), dtype=torch.uint8, device=DEV))

    def enq():
        X.rx_step_dev(s.umem, s.rx, s.fq, s.tx, s.pl, n, ws, stats=s.stats, res=s.res, opts=opts)
        torch.cuda.synchronize()

    s.restore()
    enq()
    s.restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        X.rx_step_dev(s.umem, s.rx, s.fq, s.tx, s.pl, n, ws, stats=s.stats, res=s.res, opts=opts)

    def rep():
        graph.replay()
        torch.cuda.synchronize()

    legs = {"host": lambda: host_leg(s, n, bufs), "enq": enq, "graph": rep}
    per_run = {k: [] for k in legs}
    for _ in range(runs):
        t = {k: [] for k in legs}
        for _ in range(reps):
            finals = {}
            for k, f in legs.items():  # interleaved
                s.restore()
                t0 = time.perf_counter()
                f()
                t[k].append((time.perf_counter() - t0) * 1e6)
                finals[k] = s.final()
            for k in ("enq", "graph"):
                assert all(torch.equal(a, b) for a, b in zip(finals["host"], finals[k])), f"{k} differs from the host leg"
        for k in legs:
            per_run[k].append(statistics.median(t[k]))
    line = dict(row="a", frames=n, opts=opts, ring=s.size, runs=runs, reps=reps, build_id=X.build_id(),
                **{k: summary(v) for k, v in per_run.items()})
    out.write(json.dumps(line) + "\n")
    print(json.dumps(line))


def row_b(n, opts, runs, reps, out, calls=20):
    s = State(calls * n, pow2_at_least(calls * n), opts)
    ws = torch.zeros(X.rx_step_dev_workspace_size(n), dtype=torch.uint8, device=DEV)
    verd = torch.zeros(n, dtype=torch.uint8, device=DEV)
    d_tx, d_free = torch.zeros(n * 16, dtype=torch.uint8, device=DEV), torch.zeros(n * 8, dtype=torch.uint8, device=DEV)
    counts, cnt = torch.zeros(16, dtype=torch.uint8, device=DEV), words(n)
    ews = torch.zeros(max(X.egress_workspace_size(n), 4), dtype=torch.uint8, device=DEV)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def glue():
        for _ in range(calls):
            X.rx_step_dev(s.umem, s.rx, s.fq, s.tx, s.pl, n, ws, stats=s.stats, res=s.res, opts=opts)

    def plain():
        for k in range(calls):
            d = s.rx_ent[k * n * 16:(k + 1) * n * 16]
            X.echo_dev_indirect(s.umem, d, cnt, n, verd, None, s.stats, opts=opts)
            X.egress_dev(d, verd, n, d_tx, d_free, counts, count=cnt, stats=s.stats, workspace=ews)

    legs = {"plain": plain, "glue": glue}
    per_run = {k: [] for k in legs}
    for _ in range(runs):
        t = {k: [] for k in legs}
        for _ in range(reps):
            for k, f in legs.items():
                s.restore()
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                t[k].append(e0.elapsed_time(e1) * 1e3 / calls)
            assert int(s.rx_w.cpu().numpy().view(np.uint32)[1]) == calls * n  # every call had a full batch
        for k in legs:
            per_run[k].append(statistics.median(t[k]))
    line = dict(row="b", frames=n, opts=opts, calls=calls, runs=runs, reps=reps, build_id=X.build_id(),
                **{k: summary(v) for k, v in per_run.items()})
    out.write(json.dumps(line) + "\n")
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024,65536")
    ap.add_argument("--opts", type=lambda v: int(v, 0), default=0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="profiles/rx_step_dev")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    sizes = [int(x) for x in a.sizes.split(",")]
    with open(os.path.join(a.out, "step.jsonl"), "w") as f:
        for n in sizes:
            row_a(n, a.opts, a.runs, a.reps, f)
    with open(os.path.join(a.out, "glue.jsonl"), "w") as f:
        for n in sizes:
            row_b(n, a.opts, a.runs, a.reps, f)


if __name__ == "__main__":
    main()
