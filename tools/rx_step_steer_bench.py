#!/usr/bin/env python3
"""Measurement of xsk_gpu_rx_step_steer_dev: recorded, no gate.

(a) One steered RX loop step with rings, pool and UMEM in device memory, host clock from the first call until the rings
    are final (a synchronisation), three legs interleaved:
      host    what the library offered before: synchronise, D2H of the index words and RX entries, host linearisation
              and refill (numpy), H2D, ingress_steer_dev + egress_ports_dev with the host-known count, synchronise, D2H
              of the offsets, counts, actions and lists, the ring and pool writes from the host (every port's span, the
              pool's list), H2D;
      enq     rx_step_steer_dev enqueued;
      graph   rx_step_steer_dev as a graph replay.
    Every repetition starts from the same state (restored outside the clock) and the tool asserts that the three legs
    leave identical rings, words, pool, counters and UMEM.  -> step.jsonl
(b) The price of prepare + end: device events around back-to-back rx_step_steer_dev calls over a ring holding that many
    batches, against ingress_steer_dev + egress_ports_dev alone over the same frames.  -> glue.jsonl
(c) The price of the pad: one step at a bound of n frames over a ring that holds n / 4, against one step at a bound of
    n / 4 over the same ring (what an indirect-count form of the steer kernels could at most save).  -> pad.jsonl
Traffic: a 4096-frame tests/v6_frames.mixed_batch6 batch tiled at a 2048-B stride, opts 0x17, tables of
tests/steer_spec.sample_table (1 port: no table; 8 ports: 64 entries; 64 ports: 1024 entries), default port 0, every
port bound, every TX ring empty and large enough for its port's replies.  Five runs of ten repetitions, the legs of a
repetition in alternating order (with a fixed order whichever leg ran second measured 15 to 20 us faster in row (c));
the lines carry the build id.
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
from tests import steer_spec as SS  # noqa: E402
from tests.classify_wire import tile_batch  # noqa: E402
from tests.v6_frames import mixed_batch6  # noqa: E402

STRIDE, OPTS = 2048, 0x17
DEV = torch.device("cuda:0")
ENTRIES = {1: 0, 8: 64, 64: 1024}
REDIRECT = 4


def pow2_at_least(n):
    p = 1
    while p < n:
        p *= 2
    return p


def words(*v):
    return torch.tensor(np.array(v, np.uint32).view(np.int32), dtype=torch.int32, device=DEV)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


_BASE = {}


def base_batch():
    if not _BASE:
        h_umem, h_descs = mixed_batch6(4096, STRIDE, seed=7)
        h_descs = np.ascontiguousarray(h_descs, X.DESC_DTYPE)
        _BASE.update(umem=h_umem, descs=h_descs, keys=SS.destinations(h_umem, h_descs, OPTS))
    return _BASE


class State:
    """n_frames mixed frames on an RX ring of `size` entries, n_ports empty TX rings of tx_size entries, a fill ring
    holding fill_used entries (half full by default), a pool of `size` // 2 frames in a stack of 2 * size."""

    def __init__(self, n_frames, size, tx_size, n_ports, fill_used=None):
        b = base_batch()
        h_umem, h_descs, _ = tile_batch(b["umem"], b["descs"], np.zeros(len(b["descs"]), np.uint8), n_frames, STRIDE)
        self.size, self.tx_size, self.n_ports = size, tx_size, n_ports
        self.umem = torch.from_numpy(h_umem).to(DEV)
        self.rx_ent = torch.zeros(size * 16, dtype=torch.uint8, device=DEV)
        self.rx_ent[:n_frames * 16] = to_dev(h_descs)
        table = SS.sample_table(b["keys"], ENTRIES[n_ports], n_ports, seed=n_ports) if ENTRIES[n_ports] else {}
        e = X.steer_table_prepare(SS.entries_of(table))
        self.table, self.n_entries = (to_dev(e), len(e)) if len(e) else (None, 0)
        self.rx_w, self.pool_w = words(n_frames, 0), words(size // 2)
        self.fq_w = words(size // 2 if fill_used is None else fill_used, 0)
        self.tx_w = torch.zeros(2 * n_ports, dtype=torch.int32, device=DEV)
        self.fq_ent = torch.zeros(size * 8, dtype=torch.uint8, device=DEV)
        self.tx_ent = torch.zeros(n_ports * tx_size * 16, dtype=torch.uint8, device=DEV)
        self.pool = (torch.arange(2 * size, dtype=torch.int64, device=DEV) + (1 << 20)) * 4096
        self.stats = torch.zeros(40, dtype=torch.uint8, device=DEV)
        self.port_stats = torch.zeros(40 * n_ports, dtype=torch.uint8, device=DEV)
        self.res = torch.zeros(32, dtype=torch.uint8, device=DEV)
        self.mutable = [self.umem, self.rx_w, self.fq_w, self.tx_w, self.fq_ent, self.tx_ent, self.pool, self.pool_w]
        torch.cuda.synchronize()
        self.saved = [t.clone() for t in self.mutable]
        self.rx = X.RingDev.of(self.rx_w[0:1], self.rx_w[1:2], self.rx_ent, size)
        self.fq = X.RingDev.of(self.fq_w[0:1], self.fq_w[1:2], self.fq_ent, size)
        self.tx = [X.RingDev.of(self.tx_w[2 * p:2 * p + 1], self.tx_w[2 * p + 1:2 * p + 2],
                                self.tx_ent[p * tx_size * 16:(p + 1) * tx_size * 16], tx_size) for p in range(n_ports)]
        self.pl = X.PoolDev.of(self.pool, self.pool_w, 2 * size)

    def restore(self):
        for t, s in zip(self.mutable, self.saved):
            t.copy_(s)
        self.stats.zero_()
        self.port_stats.zero_()
        torch.cuda.synchronize()

    def final(self):
        """Everything a step leaves, as device copies (the pool below its count)."""
        n = int(self.pool_w.cpu().numpy().view(np.uint32)[0])
        return [t.clone() for t in (self.rx_w, self.fq_w, self.tx_w, self.fq_ent, self.tx_ent, self.pool_w, self.umem,
                                    self.stats, self.port_stats)] + [self.pool[:n].clone()]

    def step(self, max_batch, ws):
        X.rx_step_steer_dev(self.umem, self.rx, self.fq, self.tx, self.pl, max_batch, self.table, self.n_entries, 0, ws,
                            stats=self.stats, port_stats=self.port_stats, res=self.res, opts=OPTS)


class Bufs:
    """The intermediate arrays of the two existing calls for a bound of n frames."""

    def __init__(self, n, n_ports):
        z = lambda k: torch.zeros(max(k, 4), dtype=torch.uint8, device=DEV)  # noqa: E731
        self.descs, self.out, self.tx, self.free = z(n * 16), z(n * 16), z(n * 16), z(n * 8)
        self.verd, self.act, self.ports = z(n), z(n), z(n)
        self.off, self.counts, self.room = z(4 * (n_ports + 1)), z(16 * n_ports), z(4 * n_ports)
        self.sws, self.ews = z(X.steer_workspace_size(n, n_ports)), z(X.egress_ports_workspace_size(n, n_ports))

    def calls(self, s: State, descs, n):
        X.ingress_steer_dev(s.umem, descs, n, s.table, s.n_entries, 0, s.n_ports, None, self.act, self.ports, self.out,
                            self.off, self.verd, None, s.stats, self.sws, opts=OPTS)
        X.egress_ports_dev(self.out, self.verd, self.off, s.n_ports, n, self.tx, self.free, self.counts,
                           tx_room=self.room, stats=s.stats, port_stats=s.port_stats, workspace=self.ews)


def put_words(t, *v):
    t.copy_(torch.from_numpy(np.array(v, np.uint32).view(np.int32)))


def host_leg(s: State, n, b: Bufs):
    """The step as a caller of the earlier API had to do it."""
    size, mask, tmask, P = s.size, s.size - 1, s.tx_size - 1, s.n_ports
    torch.cuda.synchronize()
    rxw, fqw, txw = (t.cpu().numpy().view(np.uint32).astype(np.int64) for t in (s.rx_w, s.fq_w, s.tx_w))
    pool_n = int(s.pool_w.cpu().numpy().view(np.uint32)[0])
    rcvd = min(int((rxw[0] - rxw[1]) & 0xFFFFFFFF), n)
    if rcvd == 0:
        return
    descs = s.rx_ent.cpu().numpy().view(X.DESC_DTYPE)[(rxw[1] + np.arange(rcvd)) & mask]  # linearise
    stock = min(size - int((fqw[0] - fqw[1]) & 0xFFFFFFFF), pool_n)
    room = s.tx_size - np.minimum((txw[0::2] - txw[1::2]) & 0xFFFFFFFF, s.tx_size)
    b.descs[:rcvd * 16].copy_(torch.from_numpy(descs.view(np.uint8).reshape(-1)))
    b.room.copy_(torch.from_numpy(room.astype(np.uint32).view(np.uint8)))
    b.calls(s, b.descs, rcvd)
    torch.cuda.synchronize()
    off = b.off.cpu().numpy().view(np.uint32).astype(np.int64)
    c = b.counts.cpu().numpy().view(X.EGRESS_COUNTS_DTYPE)
    act = b.act[:rcvd].cpu().numpy()
    tx_list = b.tx[:int(off[P]) * 16].cpu().numpy().view(X.DESC_DTYPE)
    free_list = b.free[:int(off[P]) * 8].cpu().numpy().view(np.uint64)
    pool = s.pool.cpu().numpy().view(np.uint64).copy()
    fq = s.fq_ent.cpu().numpy().view(np.uint64).copy()
    fq[(fqw[0] + np.arange(stock)) & mask] = pool[pool_n - 1 - np.arange(stock)]
    pool_n -= stock
    push = [free_list[off[p]:off[p] + int(c[p]["n_free"])] for p in range(P)] + [descs["addr"][act != REDIRECT]]
    push = np.concatenate(push)
    pushed = min(len(push), len(pool) - pool_n)
    pool[pool_n:pool_n + pushed] = push[:pushed]
    for p in range(P):  # every port's span onto its ring (the rings start empty at index 0: one contiguous copy each)
        t = int(c[p]["n_tx"])
        if t:
            assert (txw[2 * p] & tmask) + t <= s.tx_size
            lo = (p * s.tx_size + int(txw[2 * p] & tmask)) * 16
            s.tx_ent[lo:lo + t * 16].copy_(torch.from_numpy(tx_list[off[p]:off[p] + t].view(np.uint8).reshape(-1)))
        txw[2 * p] += t
    s.fq_ent.copy_(torch.from_numpy(fq.view(np.uint8)))
    s.pool[pool_n:pool_n + pushed].copy_(torch.from_numpy(pool[pool_n:pool_n + pushed].view(np.int64)))
    put_words(s.pool_w, pool_n + pushed)
    put_words(s.fq_w, fqw[0] + stock, fqw[1])
    put_words(s.tx_w, *txw)
    put_words(s.rx_w, rxw[0], rxw[1] + rcvd)
    torch.cuda.synchronize()


def in_turn(legs, i):
    """The legs interleaved, in alternating order: whatever precedes a leg precedes every leg equally often."""
    order = list(legs.items())
    return order[::-1] if i % 2 else order


def summary(v):
    return dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))


def emit(out, **line):
    line["build_id"] = X.build_id()
    out.write(json.dumps(line) + "\n")
    out.flush()
    print(json.dumps(line), flush=True)


def row_a(n, n_ports, runs, reps, out):
    s = State(n, pow2_at_least(2 * n), pow2_at_least(n), n_ports)
    ws = torch.zeros(X.rx_step_steer_dev_workspace_size(n, n_ports), dtype=torch.uint8, device=DEV)
    b = Bufs(n, n_ports)

    def enq():
        s.step(n, ws)
        torch.cuda.synchronize()

    s.restore()
    enq()
    s.restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.step(n, ws)

    def rep():
        graph.replay()
        torch.cuda.synchronize()

    legs = {"host": lambda: host_leg(s, n, b), "enq": enq, "graph": rep}
    per_run = {k: [] for k in legs}
    for _ in range(runs):
        t = {k: [] for k in legs}
        for i in range(reps):
            finals = {}
            for k, f in in_turn(legs, i):
                s.restore()
                t0 = time.perf_counter()
                f()
                t[k].append((time.perf_counter() - t0) * 1e6)
                finals[k] = s.final()
            for k in ("enq", "graph"):
                assert all(torch.equal(x, y) for x, y in zip(finals["host"], finals[k])), f"{k} differs from the host leg"
        for k in legs:
            per_run[k].append(statistics.median(t[k]))
    r = s.res.cpu().numpy().view(np.uint32)
    emit(out, row="a", frames=n, ports=n_ports, entries=s.n_entries, opts=OPTS, ring=s.size, runs=runs, reps=reps,
         redirected=int(r[1]), replied=int(r[2]), freed=int(r[5]), **{k: summary(v) for k, v in per_run.items()})


def timed(fn, e0, e1):
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def row_b(n, n_ports, runs, reps, out, calls):
    size = pow2_at_least(calls * n)
    s = State(calls * n, size, size, n_ports, fill_used=size)  # a full fill ring: no refill inside the window
    ws = torch.zeros(X.rx_step_steer_dev_workspace_size(n, n_ports), dtype=torch.uint8, device=DEV)
    b = Bufs(n, n_ports)
    b.room.copy_(to_dev(np.full(n_ports, 0xFFFFFFFF, np.uint32)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def glue():
        for _ in range(calls):
            s.step(n, ws)

    def plain():
        for k in range(calls):
            b.calls(s, s.rx_ent[k * n * 16:(k + 1) * n * 16], n)

    legs = {"plain": plain, "glue": glue}
    per_run = {k: [] for k in legs}
    for _ in range(runs):
        t = {k: [] for k in legs}
        for i in range(reps):
            for k, f in in_turn(legs, i):
                s.restore()
                t[k].append(timed(f, e0, e1) / calls)
                if k == "glue":
                    assert int(s.rx_w.cpu().numpy().view(np.uint32)[1]) == calls * n  # every call had a full batch
        for k in legs:
            per_run[k].append(statistics.median(t[k]))
    emit(out, row="b", frames=n, ports=n_ports, entries=s.n_entries, opts=OPTS, calls=calls, runs=runs, reps=reps,
         **{k: summary(v) for k, v in per_run.items()})


def row_c(n, n_ports, runs, reps, out):
    q = n // 4
    s = State(q, pow2_at_least(2 * n), pow2_at_least(n), n_ports)
    ws = torch.zeros(X.rx_step_steer_dev_workspace_size(n, n_ports), dtype=torch.uint8, device=DEV)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    legs = {"bound_quarter": lambda: s.step(q, ws), "bound_full": lambda: s.step(n, ws)}
    per_run = {k: [] for k in legs}
    for _ in range(runs):
        t = {k: [] for k in legs}
        for i in range(reps):
            finals = {}
            for k, f in in_turn(legs, i):
                s.restore()
                t[k].append(timed(f, e0, e1))
                finals[k] = s.final()
            assert all(torch.equal(x, y) for x, y in zip(*finals.values())), "the bound changed what the step leaves"
        for k in legs:
            per_run[k].append(statistics.median(t[k]))
    emit(out, row="c", bound=n, arrived=q, ports=n_ports, entries=s.n_entries, opts=OPTS, runs=runs, reps=reps,
         **{k: summary(v) for k, v in per_run.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024,65536")
    ap.add_argument("--ports", default="1,8,64")
    ap.add_argument("--rows", default="a,b,c")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="profiles/rx_step_steer")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    sizes, ports, rows = [int(x) for x in a.sizes.split(",")], [int(x) for x in a.ports.split(",")], a.rows.split(",")
    if "a" in rows:
        with open(os.path.join(a.out, "step.jsonl"), "w") as f:
            for n in sizes:
                for p in ports:
                    row_a(n, p, a.runs, a.reps, f)
    if "b" in rows:
        with open(os.path.join(a.out, "glue.jsonl"), "w") as f:
            for n in sizes:
                for p in ports:
                    if n * p <= 65536 * 8:  # (64 ports at 65 536 frames: rings for all the calls' replies are not held)
                        row_b(n, p, a.runs, a.reps, f, calls=10 if n <= 1024 else 4)
    if "c" in rows:
        with open(os.path.join(a.out, "pad.jsonl"), "w") as f:
            for n in sizes:
                for p in ports:
                    row_c(n, p, a.runs, a.reps, f)


if __name__ == "__main__":
    main()
