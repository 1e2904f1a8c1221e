#!/usr/bin/env python3
"""Measurement of xsk_gpu_unreach_serve_dev: recorded, no gate.

(a) The serve call against the host round trip it replaces, at 64 `up` entries (half IPv4 and half IPv6 UDP probes of a
    closed port, 32 bytes of data each, 8 ports, a table of 16 entries, every probe answered), legs interleaved:
      host    D2H of the index words, the up ring's entries and the frames' chunks (pinned host memory, one copy
              each); the rule on the CPU (xsk_unreach.h compiled for the host: tools/unreach_host.cpp, built here with
              g++ -O2); H2D of the rewritten frames, the TX and rest rings' entries and the index words; synchronise.
              Host clock.
      enq     unreach_serve_dev enqueued, synchronise.  Host clock.
      graph   unreach_serve_dev as a graph replay: device events around the replay (graph_dev), and the host clock
              around replay and synchronise (graph), which is what compares with the host leg's clock.
(b) The same legs over 64 IPv6 probes of 1193 payload bytes: every quote is 1232 bytes, the rewrite at its longest.
Every repetition starts from the same state (restored outside the clock) and the tool asserts that the legs leave
identical rings, index words and UMEM.  Five runs of ten repetitions, the median of the runs' medians with min .. max.
-> serve_vs_host.jsonl
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rx_step_steer_bench import DEV, X, in_turn, pow2_at_least, summary, timed  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_unreach_golden",
                                               os.path.join(ROOT, "tests", "golden", "make_unreach_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

OPTS, STRIDE = 0x17, 2048


def host_lib(td):
    so = os.path.join(td, "libunreach_host.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "unreach_host.cpp")],
                   check=True)
    L = C.CDLL(so)
    P = C.c_void_p
    L.unreach_host_serve.argtypes = [P, C.c_uint64, P, C.c_uint32, P, P, C.c_uint32, P, C.c_uint32, P, C.c_uint32, P,
                                     C.c_uint32, C.c_uint32, P, C.c_uint32, C.c_uint64, P, C.c_uint32, P]
    L.unreach_host_serve.restype = C.c_uint32
    return L


def pinned(t):
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t)
    return h


class State:
    """n up entries over n frames, n_ports TX rings and the rest ring in device memory; host mirrors in pinned memory."""

    def __init__(self, n, n_ports, ring_size, kind):
        own = []
        for p in range(n_ports):
            own.append((4, bytes([10, 1, p, 1]), p, bytes([2, 0, 0, 4, 0, p])))
            own.append((6, bytes.fromhex("20010db80001000000000000000000") + bytes([p + 1]), p, bytes([2, 0, 0, 6, 0, p])))
        umem = np.zeros(n * STRIDE, np.uint8)
        descs = np.zeros(ring_size, X.DESC_DTYPE)
        self.quoted = 0
        for i in range(n):
            e = own[2 * ((i // 2) % n_ports) + (1 if kind == "long6" else i & 1)]
            case = G.udp6_case(entry=e, data=1185 if kind == "long6" else 32) if e[0] == 6 else G.udp4_case(entry=e, data=32)
            f = case[0](())
            self.quoted += len(case[1](())[0]) - 14 - (48 if e[0] == 6 else 28)
            umem[i * STRIDE:i * STRIDE + len(f)] = np.frombuffer(f, np.uint8)
            descs[i] = (i * STRIDE, len(f), 0)
        arr = np.zeros(len(own), X.NEIGH_ENTRY_DTYPE)
        for k, (fam, addr, port, mac) in enumerate(own):
            arr[k]["addr"][:len(addr)] = np.frombuffer(addr, np.uint8)
            arr[k]["family"], arr[k]["port"] = fam, port
            arr[k]["mac"] = np.frombuffer(mac, np.uint8)
        self.h_table = X.neigh_table_prepare(arr)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)  # noqa: E731
        self.n, self.n_ports, self.size = n, n_ports, ring_size
        self.umem, self.table = dev(umem), dev(self.h_table)
        self.h_open = np.zeros(X.UNREACH_OPEN_BYTES, np.uint8)
        self.h_open[53 >> 3] |= 1 << (53 & 7)
        self.open = dev(self.h_open)
        w = np.zeros(2 + 2 * n_ports + 2, np.uint32)  # { producer, consumer }: up, tx[0 .. P), rest
        w[0] = n
        self.w = torch.from_numpy(w.view(np.int32).copy()).to(DEV)
        self.up_ent = dev(descs)
        self.tx_ent = torch.zeros(n_ports * ring_size * 16, dtype=torch.uint8, device=DEV)
        self.rest_ent = torch.zeros(ring_size * 16, dtype=torch.uint8, device=DEV)
        self.res = torch.zeros(32, dtype=torch.uint8, device=DEV)
        self.mutable = [self.umem, self.w, self.up_ent, self.tx_ent, self.rest_ent]
        torch.cuda.synchronize()
        self.saved = [t.clone() for t in self.mutable]
        self.up = X.RingDev.of(self.w[0:1], self.w[1:2], self.up_ent, ring_size)
        self.tx = [X.RingDev.of(self.w[2 + 2 * p:3 + 2 * p], self.w[3 + 2 * p:4 + 2 * p],
                                self.tx_ent[p * ring_size * 16:(p + 1) * ring_size * 16], ring_size) for p in range(n_ports)]
        self.rest = X.RingDev.of(self.w[-2:-1], self.w[-1:], self.rest_ent, ring_size)
        self.h = [pinned(t) for t in self.mutable]  # host mirrors of umem, w, up_ent, tx_ent, rest_ent

    def restore(self):
        for t, s in zip(self.mutable, self.saved):
            t.copy_(s)
        torch.cuda.synchronize()

    def final(self):
        return [t.clone() for t in self.mutable]

    def serve(self):
        X.unreach_serve_dev(self.umem, self.up, self.tx, self.rest, self.n, self.table, len(self.h_table), STRIDE,
                            open_ports=self.open, res=self.res, opts=OPTS)


def host_leg(s: State, L):
    h_umem, h_w, h_up, h_tx, h_rest = s.h
    h_w.copy_(s.w)
    h_up.copy_(s.up_ent)
    h_umem.copy_(s.umem)
    w = h_w.numpy().view(np.uint32)
    P = s.n_ports
    L.unreach_host_serve(h_umem.numpy().ctypes.data, h_umem.numel(), h_up.numpy().ctypes.data, s.size,
                         w[0:2].ctypes.data, h_tx.numpy().ctypes.data, s.size, w[2:2 + 2 * P].ctypes.data, P,
                         h_rest.numpy().ctypes.data, s.size, w[2 + 2 * P:].ctypes.data, s.n, OPTS, s.h_table.ctypes.data,
                         len(s.h_table), (1 << 64) - 1, s.h_open.ctypes.data, STRIDE, None)
    s.umem.copy_(h_umem, non_blocking=True)
    s.tx_ent.copy_(h_tx, non_blocking=True)
    s.rest_ent.copy_(h_rest, non_blocking=True)
    s.w.copy_(h_w, non_blocking=True)
    torch.cuda.synchronize()


def emit(out, **line):
    line["build_id"] = X.build_id()
    out.write(json.dumps(line) + "\n")
    out.flush()
    print(json.dumps(line), flush=True)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def row(name, kind, n, n_ports, runs, reps, out, L):
    s = State(n, n_ports, pow2_at_least(max(n, 64)), kind)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_us = []

    def enq():
        s.serve()
        torch.cuda.synchronize()

    s.restore()
    enq()
    s.restore()
    host_leg(s, L)  # (the mirrors of the TX and rest rings now hold what every repetition writes)
    s.restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.serve()

    def rep():
        dev_us.append(timed(graph.replay, e0, e1))

    legs = {"host": lambda: host_leg(s, L), "enq": enq, "graph": rep}
    per_run = {k: [] for k in list(legs) + ["graph_dev"]}
    for _ in range(runs):
        t = {k: [] for k in legs}
        dev_us.clear()
        for i in range(reps):
            final = {}
            for k, f in in_turn(legs, i):
                s.restore()
                t0 = time.perf_counter()
                f()
                t[k].append((time.perf_counter() - t0) * 1e6)
                final[k] = s.final()
            for k in ("enq", "graph"):
                assert same(final["host"], final[k]), f"{k} differs from the host leg"
        for k in legs:
            per_run[k].append(statistics.median(t[k]))
        per_run["graph_dev"].append(statistics.median(dev_us))
    r = s.res.cpu().numpy().view(X.UNREACH_RESULT_DTYPE)[0]
    assert int(r["consumed"]) == n and int(r["unreach4"]) + int(r["unreach6"]) == n
    emit(out, row=name, entries=n, ports=n_ports, table=len(s.h_table), opts=OPTS, runs=runs, reps=reps,
         unreach4=int(r["unreach4"]), unreach6=int(r["unreach6"]), quoted_bytes=s.quoted,
         d2h_bytes=s.umem.numel() + s.size * 16, **{k: summary(v) for k, v in per_run.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=64)
    ap.add_argument("--ports", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="profiles/unreach")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    with tempfile.TemporaryDirectory() as td:
        L = host_lib(td)
        with open(os.path.join(a.out, "serve_vs_host.jsonl"), "w") as f:
            row("a", "mixed", a.entries, a.ports, a.runs, a.reps, f, L)
            row("b", "long6", a.entries, a.ports, a.runs, a.reps, f, L)


if __name__ == "__main__":
    main()
