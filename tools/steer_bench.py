#!/usr/bin/env python3
"""Time xsk_gpu_steer_dev against the filter it extends, and xsk_gpu_ingress_steer_dev against xsk_gpu_ingress_dev_opts
(GPU box; profiles/steer/).  One session, legs interleaved, five runs a leg; every file ends in summary
lines: medians, spread (max - min of a leg's five runs), ratio of the medians against the first leg.

  (a) steer_alone.jsonl: 1 M dual-stack frames (the traffic of profiles/classify_wire/: a 4096-frame
      tests/v6_frames.mixed_batch6 batch tiled at a 2048-B stride), opts 0x17, device events around 20 calls enqueued
      back to back.  Leg `classify`: xsk_gpu_classify_dev_opts.  Legs `steer_p1_e0`, `steer_p8_e64`, `steer_p64_e1024`:
      xsk_gpu_steer_dev at that many ports and table entries; the tables hold every second destination of the base
      batch (tests/steer_spec.sample_table), default port 0, every port bound.
  (b) ingress.jsonl: the synthetic 1 M slab of tools/classify_bench.py --ingress (mode 1, 20-1500 B, stride 2048, opts
      0) with every frame's destination overwritten by one of 64 addresses.  Leg `ingress`: ingress_dev.  Leg
      `ingress_steer`: ingress_steer_dev, 8 ports, a 64-entry table that holds all 64 addresses, so both legs redirect
      the same frames.  Host clock from before the enqueue to the return of the synchronisation; frames re-armed after
      every repetition, untimed.

--trace runs every leg of (a) five times behind a warm-up and nothing else: the workload of a `rocprofv3 --kernel-trace
--stats` run of its own.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import xsknet_amd as X  # noqa: E402
from tests import steer_spec as SS  # noqa: E402
from tests.classify_wire import tile_batch  # noqa: E402
from tests.v6_frames import mixed_batch6  # noqa: E402

N, STRIDE, NRUNS = 1 << 20, 2048, 5


def summarise(path, what, legs, runs, extra):
    """The runs, then one summary line per leg behind the first (the baseline)."""
    with open(path, "a") as f:
        for i in range(NRUNS):
            for leg in legs:
                f.write(json.dumps({"cmp": what, "leg": leg, "run": i, "us": round(runs[leg][i], 2), **extra}) + "\n")
        base = legs[0]
        mb = statistics.median(runs[base])
        for leg in legs[1:]:
            m = statistics.median(runs[leg])
            line = {"cmp": what, "summary": True, **extra, "baseline": base, "leg": leg,
                    f"{base}_us_median": round(mb, 2), f"{base}_us_min": round(min(runs[base]), 2),
                    f"{base}_us_max": round(max(runs[base]), 2), f"{leg}_us_median": round(m, 2),
                    f"{leg}_us_min": round(min(runs[leg]), 2), f"{leg}_us_max": round(max(runs[leg]), 2),
                    "ratio": round(m / mb, 4), "delta_us": round(m - mb, 2),
                    "baseline_spread_us": round(max(runs[base]) - min(runs[base]), 2)}
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")


def alone(args):
    dev = torch.device("cuda:0")
    opts, inner, reps = 0x17, 20, 10
    h_umem, h_descs = mixed_batch6(4096, STRIDE, seed=7)
    keys = SS.destinations(h_umem, h_descs, opts)
    h_umem, h_descs, _ = tile_batch(h_umem, h_descs, np.zeros(len(h_descs), np.uint8), N, STRIDE)
    umem, descs = torch.from_numpy(h_umem).to(dev), to_dev(h_descs)
    del h_umem
    act = torch.empty(N, dtype=torch.uint8, device=dev)
    ports = torch.empty(N, dtype=torch.uint8, device=dev)
    red = torch.empty(N * 16, dtype=torch.uint8, device=dev)
    nred = torch.zeros(1, dtype=torch.int32, device=dev)
    off = torch.zeros(65, dtype=torch.int32, device=dev)
    cws = torch.empty(int(X.lib().xsk_gpu_classify_workspace_size(N)), dtype=torch.uint8, device=dev)
    sws = torch.empty(X.steer_workspace_size(N, 64), dtype=torch.uint8, device=dev)
    cur = torch.cuda.current_stream().cuda_stream  # (looked up once: calls back to back time the device, not Python)
    legs = {"classify": lambda: X.classify_dev(umem, descs, N, True, act, red, nred, cws, stream=cur, opts=opts)}
    totals = {}
    for n_ports, n_entries in ((1, 0), (8, 64), (64, 1024)):
        table = SS.sample_table(keys, n_entries, n_ports, seed=n_entries)
        d_table = to_dev(X.steer_table_prepare(SS.entries_of(table))) if n_entries else None

        def leg(n_ports=n_ports, n_entries=n_entries, d_table=d_table):
            X.steer_dev(umem, descs, N, d_table, n_entries, 0, n_ports, None, act, ports, red, off, sws, stream=cur,
                        opts=opts)
        legs[f"steer_p{n_ports}_e{n_entries}"] = leg
        leg()
        torch.cuda.synchronize()
        o = off.cpu().numpy().view(np.uint32)[:n_ports + 1]
        totals[f"steer_p{n_ports}_e{n_entries}"] = int(o[n_ports])
        assert (np.diff(o.astype(np.int64)) >= 0).all()
    legs["classify"]()
    torch.cuda.synchronize()
    k = int(nred.cpu().numpy().view(np.uint32)[0])
    assert all(t == k for t in totals.values()), (k, totals)  # default port 0, all bound: the same REDIRECT set
    if args.trace:
        for _ in range(5):
            for leg in legs.values():
                leg()
                torch.cuda.synchronize()
        return

    def timed(fn):
        tot = 0.0
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            tot += e0.elapsed_time(e1) / inner
        return tot / reps * 1e3

    for leg in legs.values():
        timed(leg)
    runs = {name: [] for name in legs}
    for _ in range(NRUNS):
        for name, leg in legs.items():
            runs[name].append(timed(leg))
    summarise(os.path.join(args.out, "steer_alone.jsonl"), "steer_alone", list(legs), runs,
              {"frames": N, "redirected": k, "opts": opts, "traffic": "dual",
               "clock": f"device events around {inner} calls back to back", "reps_per_run": reps})


def ingress(args):
    dev = torch.device("cuda:0")
    reps, n_ports = 10, 8
    umem = torch.zeros(N * STRIDE, dtype=torch.uint8, device=dev)
    descs = torch.zeros(N * 16, dtype=torch.uint8, device=dev)
    X.synth_dev(umem, descs, N, 0, STRIDE, 0x5EED0E0E, 0, 1, 1, 20, 1500)  # mixed traffic
    # every frame's destination (bytes 30-33; every frame starts at i * STRIDE) becomes one of 64 addresses
    addrs = np.array([[10, 9, 0, a] for a in range(64)], np.uint8)
    pick = torch.from_numpy(((np.arange(N, dtype=np.uint64) * 2654435761 >> 7) % 64).astype(np.int64)).to(dev)
    umem.view(N, STRIDE)[:, 30:34] = torch.from_numpy(addrs).to(dev)[pick]
    table = {SS.GS.key(bytes(addrs[a])): a % n_ports for a in range(64)}
    d_table = to_dev(X.steer_table_prepare(SS.entries_of(table)))
    act = torch.empty(N, dtype=torch.uint8, device=dev)
    ports = torch.empty(N, dtype=torch.uint8, device=dev)
    red = torch.empty(N * 16, dtype=torch.uint8, device=dev)
    nred = torch.zeros(1, dtype=torch.int32, device=dev)
    off = torch.zeros(n_ports + 1, dtype=torch.int32, device=dev)
    verd = torch.empty(N, dtype=torch.uint8, device=dev)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    cws = torch.empty(int(X.lib().xsk_gpu_classify_workspace_size(N)), dtype=torch.uint8, device=dev)
    sws = torch.empty(X.steer_workspace_size(N, n_ports), dtype=torch.uint8, device=dev)
    redirected = []

    def plain():
        X.ingress_dev(umem, descs, N, True, act, red, nred, verd, None, stats, cws, opts=0)
        return lambda: int(nred.cpu().numpy().view(np.uint32)[0])

    def steered():
        X.ingress_steer_dev(umem, descs, N, d_table, 64, SS.PASS, n_ports, None, act, ports, red, off, verd, None, stats,
                            sws, opts=0)
        return lambda: int(off.cpu().numpy().view(np.uint32)[n_ports])

    def run(leg):
        tot = 0.0
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            count = leg()
            torch.cuda.synchronize()
            tot += time.perf_counter() - t0
            k = count()
            redirected.append(k)
            X.rearm_dev(umem, red, verd, k)
        return tot / reps * 1e6

    legs = {"ingress": plain, "ingress_steer": steered}
    for leg in legs.values():
        run(leg)
    o = off.cpu().numpy().view(np.uint32).astype(np.int64)
    assert (np.diff(o) > 0).all(), o  # every port serves frames
    runs = {name: [] for name in legs}
    for _ in range(NRUNS):
        for name, leg in legs.items():
            runs[name].append(run(leg))
    assert len(set(redirected)) == 1, set(redirected)  # re-armed, and both legs redirect the same frames
    summarise(os.path.join(args.out, "ingress.jsonl"), "ingress_steer", list(legs), runs,
              {"frames": N, "redirected": redirected[0], "opts": 0, "n_ports": n_ports, "n_entries": 64,
               "clock": "host, ends in a synchronise", "reps_per_run": reps})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "steer"))
    ap.add_argument("--trace", action="store_true", help="run the legs of (a) a few times and exit (for rocprofv3)")
    ap.add_argument("--only", choices=["alone", "ingress"], default="")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.only != "ingress":
        alone(args)
    if args.only != "alone" and not args.trace:
        torch.cuda.empty_cache()
        ingress(args)


if __name__ == "__main__":
    main()
