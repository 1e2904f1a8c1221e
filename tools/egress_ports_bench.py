#!/usr/bin/env python3
"""Time xsk_gpu_egress_ports_dev: behind the steered ingress against what the library offered before it (one
xsk_gpu_egress_dev call per port behind a synchronisation), and alone against xsk_gpu_egress_dev over the same list
(GPU box; profiles/egress_ports/).  One session, legs interleaved, five runs a leg, ten repetitions a
run; every file ends in summary lines: medians, min .. max of a leg's five runs, ratio of the medians.

Traffic of rows 1, 2 and 4: 1 M dual-stack frames (a 4096-frame tests/v6_frames.mixed_batch6 batch tiled at a 2048-B
stride, as tools/steer_bench.py), opts 0x17, tables of tests/steer_spec.sample_table, default port 0, every port bound.

  1 pipeline_tail.jsonl: 8 ports / 64 entries and 64 ports / 1024 entries.  Leg `per_port_calls`: ingress_steer_dev,
    synchronise, D2H of d_off, n_ports calls of egress_dev on pointer offsets computed on the host, synchronise.  Leg
    `egress_ports`: ingress_steer_dev + egress_ports_dev, one synchronisation, D2H of d_off.  Both legs then copy the
    counts and every port's two lists into pinned host memory.  Host clock from before the first enqueue until the lists
    lie in host memory; the frames are restored from a pristine device copy after every repetition, untimed.  Every run
    asserts that both legs yield identical lists and counts.
  2 alone_1m.jsonl: the lists the steered ingress leaves at 1, 8 and 64 ports; legs `egress_pN` (egress_dev over the
    whole list, count = d_off[N]) and `ports_pN` (egress_ports_dev); no counter block, unlimited room.  Device events
    around 20 calls enqueued back to back, so the window holds the gaps between a call's launches too.
  3 alone_small.jsonl: the same clock at n_max = 64, 1024 (one launch) and 1025 (three launches), 8 even ports over
    random verdicts.
  4 price_1m.jsonl: 1 M frames, 1 port -- every workgroup's counter sums belong to one block: `plain` (no counter
    block), `stats_uncut` (d_stats given, nothing cut: no atomic), `port_stats` (a fourth launch sums the workgroups'
    records), `cut` (rooms R // 2, no block), `cut_stats`, `cut_both`; and `egress_cut_stats`, egress_dev with the same
    room, for scale.

--trace runs every leg of rows 2 to 4 six times (the first is the warm-up), a synchronise between calls, and nothing
else: the workload of a `rocprofv3 --kernel-trace --stats` run of its own.
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
from tests import egress_ports_spec as EP  # noqa: E402
from tests import egress_spec as ES  # noqa: E402
from tests import steer_spec as SS  # noqa: E402
from tests.classify_wire import tile_batch  # noqa: E402
from tests.v6_frames import mixed_batch6  # noqa: E402

N, STRIDE, NRUNS, REPS, INNER, OPTS = 1 << 20, 2048, 5, 10, 20, 0x17
CONFIGS = ((1, 0), (8, 64), (64, 1024))  # (ports, table entries)


def summarise(path, what, pairs, runs, extra):
    """The runs, then one summary line per (baseline, leg) pair."""
    with open(path, "a") as f:
        for i in range(NRUNS):
            for leg in runs:
                f.write(json.dumps({"cmp": what, "leg": leg, "run": i, "us": round(runs[leg][i], 2), **extra}) + "\n")
        for base, leg in pairs:
            mb, m = statistics.median(runs[base]), statistics.median(runs[leg])
            lo, hi = min(runs[base]), max(runs[base])
            line = {"cmp": what, "summary": True, **extra, "baseline": base, "leg": leg,
                    "baseline_us_median": round(mb, 2), "baseline_us_min": round(lo, 2), "baseline_us_max": round(hi, 2),
                    "leg_us_median": round(m, 2), "leg_us_min": round(min(runs[leg]), 2),
                    "leg_us_max": round(max(runs[leg]), 2), "ratio": round(m / mb, 4), "delta_us": round(m - mb, 2),
                    "leg_median_outside_baseline_min_max": not lo <= m <= hi}
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line))


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")


def timed_events(fn):
    tot = 0.0
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        tot += e0.elapsed_time(e1) / INNER
    return tot / REPS * 1e3


def interleaved(legs):
    for leg in legs.values():
        timed_events(leg)
    runs = {name: [] for name in legs}
    for _ in range(NRUNS):
        for name, leg in legs.items():
            runs[name].append(timed_events(leg))
    return runs


class Traffic:
    """The 1 M-frame slab on the device with a pristine copy, and the steering state per (ports, entries)."""

    def __init__(self):
        dev = torch.device("cuda:0")
        h_umem, h_descs = mixed_batch6(4096, STRIDE, seed=7)
        self.keys = SS.destinations(h_umem, h_descs, OPTS)
        h_umem, h_descs, _ = tile_batch(h_umem, h_descs, np.zeros(len(h_descs), np.uint8), N, STRIDE)
        self.pristine = torch.from_numpy(h_umem).to(dev)
        self.umem = self.pristine.clone()
        self.descs = to_dev(h_descs)
        self.act = torch.empty(N, dtype=torch.uint8, device=dev)
        self.ports = torch.empty(N, dtype=torch.uint8, device=dev)
        self.sws = torch.empty(X.steer_workspace_size(N, 64), dtype=torch.uint8, device=dev)
        self.stats = torch.zeros(40, dtype=torch.uint8, device=dev)

    def table(self, n_ports, n_entries):
        if not n_entries:
            return None
        return to_dev(X.steer_table_prepare(SS.entries_of(SS.sample_table(self.keys, n_entries, n_ports, seed=n_entries))))

    def steer(self, d_table, n_entries, n_ports, out, off, verd):
        X.ingress_steer_dev(self.umem, self.descs, N, d_table, n_entries, 0, n_ports, None, self.act, self.ports, out,
                            off, verd, None, self.stats, self.sws, opts=OPTS)

    def restore(self):
        self.umem.copy_(self.pristine)


def tail(args, tr):
    dev = torch.device("cuda:0")
    tx = torch.empty(N * 16, dtype=torch.uint8, device=dev)
    free = torch.empty(N * 8, dtype=torch.uint8, device=dev)
    out = torch.empty(N * 16, dtype=torch.uint8, device=dev)
    verd = torch.empty(N, dtype=torch.uint8, device=dev)
    ews = torch.empty(X.egress_workspace_size(N), dtype=torch.uint8, device=dev)
    host = {leg: (torch.empty(N * 16, dtype=torch.uint8, pin_memory=True),
                  torch.empty(N * 8, dtype=torch.uint8, pin_memory=True)) for leg in ("per_port_calls", "egress_ports")}
    for n_ports, n_entries in CONFIGS[1:]:
        d_table = tr.table(n_ports, n_entries)
        off = torch.zeros(n_ports + 1, dtype=torch.int32, device=dev)
        counts = torch.zeros(n_ports * 16, dtype=torch.uint8, device=dev)
        epws = torch.empty(X.egress_ports_workspace_size(N, n_ports), dtype=torch.uint8, device=dev)
        h_off = torch.empty(n_ports + 1, dtype=torch.int32, pin_memory=True)
        h_counts = {leg: torch.empty(n_ports * 16, dtype=torch.uint8, pin_memory=True) for leg in host}

        def fetch(leg, o):
            """Counts, then every port's lists, into pinned memory."""
            h_counts[leg].copy_(counts)
            c = h_counts[leg].numpy().view(X.EGRESS_COUNTS_DTYPE)
            h_tx, h_free = host[leg]
            for p in range(n_ports):
                a, n_tx, n_free = int(o[p]), int(c["n_tx"][p]), int(c["n_free"][p])
                if n_tx:
                    h_tx[a * 16:(a + n_tx) * 16].copy_(tx[a * 16:(a + n_tx) * 16], non_blocking=True)
                if n_free:
                    h_free[a * 8:(a + n_free) * 8].copy_(free[a * 8:(a + n_free) * 8], non_blocking=True)
            torch.cuda.synchronize()

        def per_port_calls():
            tr.steer(d_table, n_entries, n_ports, out, off, verd)
            torch.cuda.synchronize()
            h_off.copy_(off)
            o = h_off.numpy().view(np.uint32)
            for p in range(n_ports):
                a, n_p = int(o[p]), int(o[p + 1]) - int(o[p])
                X.egress_dev(out[a * 16:], verd[a:], n_p, tx[a * 16:], free[a * 8:], counts[p * 16:p * 16 + 16],
                             stats=tr.stats, workspace=ews)
            torch.cuda.synchronize()
            fetch("per_port_calls", o)

        def egress_ports():
            tr.steer(d_table, n_entries, n_ports, out, off, verd)
            X.egress_ports_dev(out, verd, off, n_ports, N, tx, free, counts, stats=tr.stats, workspace=epws)
            torch.cuda.synchronize()
            h_off.copy_(off)
            fetch("egress_ports", h_off.numpy().view(np.uint32))

        legs = {"per_port_calls": per_port_calls, "egress_ports": egress_ports}

        def run(name):
            tot = 0.0
            for _ in range(REPS):
                tx.fill_(0xEE)
                free.fill_(0xEE)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                legs[name]()
                tot += time.perf_counter() - t0
                tr.restore()
            return tot / REPS * 1e6

        def same_lists():
            o = h_off.numpy().view(np.uint32)
            ca, cb = (h_counts[leg].numpy().view(X.EGRESS_COUNTS_DTYPE) for leg in host)
            assert (ca == cb).all() and int(ca["n"].sum()) == int(o[n_ports]) - int(o[0])
            (tx_a, free_a), (tx_b, free_b) = host.values()
            for p in range(n_ports):
                a, n_tx, n_free = int(o[p]), int(ca["n_tx"][p]), int(ca["n_free"][p])
                assert torch.equal(tx_a[a * 16:(a + n_tx) * 16], tx_b[a * 16:(a + n_tx) * 16]), p
                assert torch.equal(free_a[a * 8:(a + n_free) * 8], free_b[a * 8:(a + n_free) * 8]), p
            return int(o[n_ports]), int(ca["n_tx"].sum())

        for name in legs:
            run(name)
        runs = {name: [] for name in legs}
        for _ in range(NRUNS):
            for name in legs:
                runs[name].append(run(name))
            k, n_tx = same_lists()
        summarise(os.path.join(args.out, "pipeline_tail.jsonl"), "pipeline_tail", [("per_port_calls", "egress_ports")],
                  runs, {"frames": N, "redirected": k, "replies": n_tx, "opts": OPTS, "n_ports": n_ports,
                         "n_entries": n_entries, "clock": "host, until the lists lie in pinned memory",
                         "reps_per_run": REPS})


def steered_lists(tr):
    """{ports: (out, verd, off, k)}: what the steered ingress leaves at each port count, the frames restored."""
    dev = torch.device("cuda:0")
    lists = {}
    for n_ports, n_entries in CONFIGS:
        out = torch.empty(N * 16, dtype=torch.uint8, device=dev)
        verd = torch.empty(N, dtype=torch.uint8, device=dev)
        off = torch.zeros(n_ports + 1, dtype=torch.int32, device=dev)
        tr.steer(tr.table(n_ports, n_entries), n_entries, n_ports, out, off, verd)
        torch.cuda.synchronize()
        tr.restore()
        o = off.cpu().numpy().view(np.uint32).astype(np.int64)
        assert o[0] == 0 and (np.diff(o) >= 0).all()
        lists[n_ports] = (out, verd, off, int(o[n_ports]))
    assert len({v[3] for v in lists.values()}) == 1  # default port 0, all bound: the same REDIRECT set
    return lists


def alone_legs(lists, dev):
    cur = torch.cuda.current_stream().cuda_stream  # (looked up once: calls back to back time the device, not Python)
    tx = torch.empty(N * 16, dtype=torch.uint8, device=dev)
    free = torch.empty(N * 8, dtype=torch.uint8, device=dev)
    counts = torch.zeros(64 * 16, dtype=torch.uint8, device=dev)
    ews = torch.empty(X.egress_workspace_size(N), dtype=torch.uint8, device=dev)
    epws = torch.empty(X.egress_ports_workspace_size(N, 64), dtype=torch.uint8, device=dev)
    legs, pairs = {}, []
    for P, (out, verd, off, _) in lists.items():
        def one(out=out, verd=verd, off=off, P=P):
            X.egress_dev(out, verd, N, tx, free, counts, count=off[P:P + 1], workspace=ews, stream=cur)

        def ports(out=out, verd=verd, off=off, P=P):
            X.egress_ports_dev(out, verd, off, P, N, tx, free, counts, workspace=epws, stream=cur)
        legs[f"egress_p{P}"], legs[f"ports_p{P}"] = one, ports
        pairs.append((f"egress_p{P}", f"ports_p{P}"))
    return legs, pairs, (tx, free, counts, ews, epws, cur)


def small_legs(dev):
    cur = torch.cuda.current_stream().cuda_stream
    legs, pairs, keep = {}, [], []
    for n in (64, 1024, 1025):
        descs, verd = to_dev(ES.random_descs(n, seed=n)), to_dev(ES.verdict_pattern("random", n, seed=n))
        off = to_dev(np.array(EP.layout("even", 8, n), np.uint32)).view(torch.int32)
        tx = torch.empty(n * 16, dtype=torch.uint8, device=dev)
        free = torch.empty(n * 8, dtype=torch.uint8, device=dev)
        counts = torch.zeros(8 * 16, dtype=torch.uint8, device=dev)
        ws = torch.empty(max(X.egress_ports_workspace_size(n, 8), 4), dtype=torch.uint8, device=dev)
        keep.append((descs, verd, off, tx, free, counts, ws))

        def one(n=n, b=keep[-1]):
            X.egress_dev(b[0], b[1], n, b[3], b[4], b[5], count=b[2][8:9], workspace=b[6], stream=cur)

        def ports(n=n, b=keep[-1]):
            X.egress_ports_dev(b[0], b[1], b[2], 8, n, b[3], b[4], b[5], workspace=b[6], stream=cur)
        legs[f"egress_n{n}"], legs[f"ports_n{n}"] = one, ports
        pairs.append((f"egress_n{n}", f"ports_n{n}"))
    return legs, pairs, keep


def price_legs(lists, bufs, dev):
    tx, free, counts, ews, epws, cur = bufs
    out, verd, off, k = lists[1]
    R = int((verd[:k] == 0).sum())
    room = torch.full((1,), R // 2, dtype=torch.int32, device=dev)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    pstats = torch.zeros(40, dtype=torch.uint8, device=dev)

    def leg(rooms, st, ps):
        return lambda: X.egress_ports_dev(out, verd, off, 1, N, tx, free, counts, tx_room=rooms, stats=st,
                                          port_stats=ps, workspace=epws, stream=cur)
    legs = {"plain": leg(None, None, None), "stats_uncut": leg(None, stats, None), "port_stats": leg(None, None, pstats),
            "cut": leg(room, None, None), "cut_stats": leg(room, stats, None), "cut_both": leg(room, stats, pstats),
            "egress_cut_stats": lambda: X.egress_dev(out, verd, N, tx, free, counts, count=off[1:2], tx_room=room,
                                                     stats=stats, workspace=ews, stream=cur)}
    pairs = [("plain", name) for name in legs if name != "plain"]
    return legs, pairs, {"replies": R, "room": R // 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "egress_ports"))
    ap.add_argument("--trace", action="store_true", help="run the legs of rows 2 to 4 a few times and exit")
    ap.add_argument("--only", choices=["tail", "alone"], default="")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    dev = torch.device("cuda:0")
    tr = Traffic()
    if args.only != "alone" and not args.trace:
        tail(args, tr)
        torch.cuda.empty_cache()
    if args.only == "tail":
        return
    lists = steered_lists(tr)
    k = lists[1][3]
    a_legs, a_pairs, bufs = alone_legs(lists, dev)
    s_legs, s_pairs, _keep = small_legs(dev)
    p_legs, p_pairs, p_extra = price_legs(lists, bufs, dev)
    if args.trace:
        for legs in (a_legs, s_legs, p_legs):
            for leg in legs.values():
                for _ in range(6):
                    leg()
                    torch.cuda.synchronize()
        return
    clock = {"clock": f"device events around {INNER} calls back to back", "reps_per_run": REPS}
    summarise(os.path.join(args.out, "alone_1m.jsonl"), "alone_1m", a_pairs, interleaved(a_legs),
              {"frames": N, "listed": k, **clock})
    summarise(os.path.join(args.out, "alone_small.jsonl"), "alone_small", s_pairs, interleaved(s_legs),
              {"n_ports": 8, **clock})
    summarise(os.path.join(args.out, "price_1m.jsonl"), "price_1m", p_pairs, interleaved(p_legs),
              {"frames": N, "listed": k, "n_ports": 1, **p_extra, **clock})


if __name__ == "__main__":
    main()
