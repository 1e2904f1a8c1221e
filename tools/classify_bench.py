#!/usr/bin/env python3
"""Time the device XDP ingress filter (xsk_gpu_classify_dev, inner_xdp.c:26-61) and the filter ->
echo pipeline on a 1 M mixed-traffic batch (GPU box).  Prints one JSON line.

--lib PATH times the xsk_gpu_classify_dev of another build of xsk_classify.hip (same C signature; e.g. round 1's
three-launch filter, `git show <rev>:xsknet_amd/csrc/xsk_classify.hip` built with hipcc -shared -I xsknet_amd/csrc)
against the same batch, for A/B; its workspace is the larger of the two builds'.

Algorithmic bytes per frame of the filter: 16-B descriptor read, the frame bytes the eBPF program
reads (12-13 and 23: one 64-B sector per frame in practice), 1-B action written, 16-B descriptor
written per redirected frame.

--opts N times xsk_gpu_classify_dev_opts (classify_dev(opts=N)) and hands the echo leg the same option word;
--traffic dual replaces the synthetic IPv4 slab by dual-stack traffic: a 4096-frame tests/v6_frames.mixed_batch6 batch
(VLAN stacks, IPv4 and IPv6, truncations) tiled to 1 M frames at the same 2048-B stride.  The echo leg is not re-armed
then (xsk_gpu_rearm_dev restores IPv4 replies only): after the first repetition most echo requests have become
replies, so with --traffic dual only the classify figures are comparable between runs.

--ingress runs two interleaved A/B comparisons instead, five runs a leg, and appends their JSON lines to
--out DIR/pipeline.jsonl and DIR/indirect.jsonl (profiles/ingress/):
  (a) filter -> transform on the synthetic 1 M slab: classify_dev, the count copied to the host behind a
      synchronisation, echo_dev with that count (leg "roundtrip") against one ingress_dev call (leg "ingress").  Host
      clock from before the first enqueue to the return of the final synchronisation, which both legs end in;
  (b) the transform alone on c3's shape (1 M x 1500 B at a 4 KiB stride): echo_dev(n) (leg "direct") against
      echo_dev_indirect with *d_n == n_max == n (leg "indirect"), device events.
Frames are re-armed between repetitions, untimed.  The last line of each file gives the medians, the spread (max - min)
of each leg's five runs and the ratio of the medians; the baseline is the first leg.

--egress does the same for xsk_gpu_egress_dev (egress_compare below; --out DIR/pipeline_tail.jsonl,
egress_alone_1m.jsonl and egress_alone_small.jsonl, profiles/egress/).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import xsknet_amd as X  # noqa: E402


def _summarise(path, what, legs, runs, extra):
    """Append the runs of an A/B (legs[0] is the baseline) and their summary line to `path`."""
    med = {leg: statistics.median(runs[leg]) for leg in legs}
    line = {"cmp": what, "summary": True, **extra}
    for leg in legs:
        line[f"{leg}_us_median"] = round(med[leg], 2)
        line[f"{leg}_us_spread"] = round(max(runs[leg]) - min(runs[leg]), 2)
    line["ratio"] = round(med[legs[1]] / med[legs[0]], 4)
    line["delta_us"] = round(med[legs[1]] - med[legs[0]], 2)
    line["within_baseline_spread"] = bool(med[legs[1]] - med[legs[0]] <= max(runs[legs[0]]) - min(runs[legs[0]]))
    with open(path, "a") as f:
        for i in range(len(runs[legs[0]])):
            for leg in legs:
                f.write(json.dumps({"cmp": what, "leg": leg, "run": i, "us": round(runs[leg][i], 2), **extra}) + "\n")
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


def ingress_compare(args):
    n, reps, nruns = 1 << 20, 10, 5
    dev = torch.device("cuda:0")
    os.makedirs(args.out, exist_ok=True)
    # ---- (a) filter -> transform, with and without the host round trip ----
    stride = 2048
    umem = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    descs = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    X.synth_dev(umem, descs, n, 0, stride, 0x5EED0E0E, 0, 1, 1, 20, 1500)  # mixed traffic
    act = torch.empty(n, dtype=torch.uint8, device=dev)
    red = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    nred = torch.zeros(1, dtype=torch.int32, device=dev)
    verd = torch.empty(n, dtype=torch.uint8, device=dev)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    ws = torch.empty(int(X.lib().xsk_gpu_classify_workspace_size(n)), dtype=torch.uint8, device=dev)
    ews = torch.zeros(X.workspace_size(0, n), dtype=torch.uint8, device=dev)
    redirected = []

    def roundtrip():
        X.classify_dev(umem, descs, n, True, act, red, nred, ws, opts=args.opts)
        torch.cuda.synchronize()
        k = int(nred.cpu()[0])
        X.echo_dev(umem, red, k, verd, None, stats, ews, opts=args.opts)
        return k

    def ingress():
        X.ingress_dev(umem, descs, n, True, act, red, nred, verd, None, stats, ws, opts=args.opts)
        return None

    def run_a(leg):
        tot = 0.0
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = leg()
            torch.cuda.synchronize()
            tot += time.perf_counter() - t0
            k = int(nred.cpu()[0]) if k is None else k
            redirected.append(k)
            X.rearm_dev(umem, red, verd, k)
        return tot / reps * 1e6

    legs = {"roundtrip": roundtrip, "ingress": ingress}
    for leg in legs.values():  # warm-up of every kernel either leg launches
        run_a(leg)
    runs = {name: [] for name in legs}
    for _ in range(nruns):
        for name, leg in legs.items():
            runs[name].append(run_a(leg))
    assert len(set(redirected)) == 1, set(redirected)  # re-armed: every repetition filters the same traffic
    _summarise(os.path.join(args.out, "pipeline.jsonl"), "filter_then_transform", list(legs), runs,
               {"frames": n, "redirected": redirected[0], "opts": args.opts, "clock": "host, ends in a synchronise",
                "reps_per_run": reps})
    del umem, descs, act, red, verd
    torch.cuda.empty_cache()
    # ---- (b) the transform alone on c3's shape: host count against device count ----
    stride = 4096
    umem = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    descs = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    X.synth_dev(umem, descs, n, 0, stride, 0x5EED0003, 0, 1, 0, 1500, 1500)
    verd = torch.empty(n, dtype=torch.uint8, device=dev)
    cnt = torch.full((1,), n, dtype=torch.int32, device=dev)

    def direct():
        X.echo_dev(umem, descs, n, verd, None, stats, ews)

    def indirect():
        X.echo_dev_indirect(umem, descs, cnt, n, verd, None, stats)

    def run_b(leg):
        tot = 0.0
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            leg()
            e1.record()
            X.rearm_dev(umem, descs, verd, n)
            torch.cuda.synchronize()
            tot += e0.elapsed_time(e1)
        return tot / reps * 1e3

    legs = {"direct": direct, "indirect": indirect}
    for leg in legs.values():
        run_b(leg)
    runs = {name: [] for name in legs}
    for _ in range(nruns):
        for name, leg in legs.items():
            runs[name].append(run_b(leg))
    _summarise(os.path.join(args.out, "indirect.jsonl"), "transform_c3", list(legs), runs,
               {"frames": n, "frame_len": 1500, "stride": stride, "opts": 0, "clock": "device events",
                "reps_per_run": reps})


def egress_compare(args):
    """--egress (profiles/egress/), legs interleaved, five runs of ten repetitions each:
      (a) the pipeline's tail on the synthetic 1 M slab, host clock from the first enqueue to both lists lying in
          (pinned) host memory: ingress_dev, synchronise, D2H of nout, of d_out[:nout] and of d_verdicts[:nout], a
          vectorised numpy pass that builds both lists (leg "hostpass") against ingress_dev + egress_dev, synchronise,
          D2H of the counts, of d_tx[:n_tx] and of d_free[:n_free] (leg "egress").  The two ways must yield identical
          lists (asserted on every repetition).  Unlimited room;
      (b) egress_dev alone, device events around 20 calls back to back: at 1 M frames next to a device-to-device copy
          of the same 16 n bytes (the floor), and at n_max = 1024, 1025 and 64 (the first pair: what the one-launch
          path saves)."""
    n, reps, nruns, inner = 1 << 20, 10, 5, 20
    dev = torch.device("cuda:0")
    out_dir = args.out
    os.makedirs(out_dir, exist_ok=True)
    stride = 2048
    umem = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    descs = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    X.synth_dev(umem, descs, n, 0, stride, 0x5EED0E0E, 0, 1, 1, 20, 1500)  # mixed traffic
    act = torch.empty(n, dtype=torch.uint8, device=dev)
    red = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    nred = torch.zeros(1, dtype=torch.int32, device=dev)
    verd = torch.empty(n, dtype=torch.uint8, device=dev)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    ws = torch.empty(int(X.lib().xsk_gpu_classify_workspace_size(n)), dtype=torch.uint8, device=dev)
    d_tx = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    d_free = torch.empty(n * 8, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(16, dtype=torch.uint8, device=dev)
    ews = torch.empty(X.egress_workspace_size(n), dtype=torch.uint8, device=dev)
    h_nout = torch.zeros(1, dtype=torch.int32).pin_memory()
    h_counts = torch.zeros(16, dtype=torch.uint8).pin_memory()
    h_a = torch.empty(n * 16, dtype=torch.uint8).pin_memory()  # d_out, or d_tx
    h_b = torch.empty(n * 8, dtype=torch.uint8).pin_memory()   # d_verdicts, or d_free
    lists, seen = {}, []

    def hostpass():
        X.ingress_dev(umem, descs, n, True, act, red, nred, verd, None, stats, ws, opts=args.opts)
        h_nout.copy_(nred)  # (a copy to pinned memory on the current stream, then the synchronisation)
        torch.cuda.synchronize()
        k = int(h_nout[0])
        h_a[:k * 16].copy_(red[:k * 16], non_blocking=True)
        h_b[:k].copy_(verd[:k], non_blocking=True)
        torch.cuda.synchronize()
        out = h_a[:k * 16].numpy().view(X.DESC_DTYPE)
        reply = h_b[:k].numpy() == X.TX_REPLY
        tx = out[reply]  # (a copy)
        tx["options"] = 0
        free = out["addr"][~reply]
        t1 = time.perf_counter()
        lists["hostpass"] = (tx, free)
        return k, t1

    def egress():
        X.ingress_dev(umem, descs, n, True, act, red, nred, verd, None, stats, ws, opts=args.opts)
        X.egress_dev(red, verd, n, d_tx, d_free, d_counts, count=nred, stats=stats, workspace=ews)
        h_counts.copy_(d_counts)
        torch.cuda.synchronize()
        c = h_counts.numpy().view(X.EGRESS_COUNTS_DTYPE)[0]
        n_tx, n_free = int(c["n_tx"]), int(c["n_free"])
        h_a[:n_tx * 16].copy_(d_tx[:n_tx * 16], non_blocking=True)
        h_b[:n_free * 8].copy_(d_free[:n_free * 8], non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()  # both lists lie in host memory; the copies below only keep them for the comparison
        lists["egress"] = (h_a[:n_tx * 16].numpy().view(X.DESC_DTYPE).copy(), h_b[:n_free * 8].numpy().view("<u8").copy())
        return int(c["n"]), t1

    def run_a(name, leg):
        tot = 0.0
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k, t1 = leg()
            tot += t1 - t0
            seen.append((k, len(lists[name][0]), len(lists[name][1])))
            X.rearm_dev(umem, red, verd, k)
        torch.cuda.synchronize()
        return tot / reps * 1e6

    legs = {"hostpass": hostpass, "egress": egress}
    for name, leg in legs.items():  # warm-up, and the two ways yield identical lists
        run_a(name, leg)
    assert (lists["hostpass"][0] == lists["egress"][0]).all() and (lists["hostpass"][1] == lists["egress"][1]).all()
    runs = {name: [] for name in legs}
    for _ in range(nruns):
        for name, leg in legs.items():
            runs[name].append(run_a(name, leg))
        assert (lists["hostpass"][0] == lists["egress"][0]).all() and (lists["hostpass"][1] == lists["egress"][1]).all()
    assert len(set(seen)) == 1, set(seen)  # re-armed: every repetition sees the same traffic and builds the same lists
    k, n_tx, n_free = seen[0]
    _summarise(os.path.join(out_dir, "pipeline_tail.jsonl"), "pipeline_tail", list(legs), runs,
               {"frames": n, "redirected": k, "n_tx": n_tx, "n_free": n_free, "opts": args.opts,
                "clock": "host, first enqueue to both lists in pinned host memory", "reps_per_run": reps})
    # ---- (b) egress_dev alone, device events ----
    # verdicts for all 1 M descriptors: the transform over the whole slab, re-armed afterwards
    ews_echo = torch.zeros(X.workspace_size(0, n), dtype=torch.uint8, device=dev)
    X.echo_dev(umem, descs, n, verd, None, stats, ews_echo, opts=args.opts)
    X.rearm_dev(umem, descs, verd, n)
    cnt = torch.full((1,), n, dtype=torch.int32, device=dev)
    src, dst = descs, torch.empty_like(descs)

    def timed(fn):
        def run():
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
        return run

    cur = torch.cuda.current_stream().cuda_stream  # (looked up once: 20 calls back to back time the device, not Python)

    def eg(n_max, workspace):
        return lambda: X.egress_dev(descs, verd, n_max, d_tx, d_free, d_counts, count=cnt, workspace=workspace,
                                    stream=cur)

    big = {"d2d_copy": timed(lambda: dst.copy_(src)), "egress": timed(eg(n, ews))}
    small_ws = torch.empty(X.egress_workspace_size(1025), dtype=torch.uint8, device=dev)
    small = {"n1024": timed(eg(1024, None)), "n1025": timed(eg(1025, small_ws)), "n64": timed(eg(64, None))}
    for what, legs, extra in (("egress_alone_1m", big, {"frames": n, "copy_bytes": 16 * n}),
                              ("egress_alone_small", small, {"frames": "64 / 1024 / 1025"})):
        for leg in legs.values():
            leg()
        runs = {name: [] for name in legs}
        for _ in range(nruns):
            for name, leg in legs.items():
                runs[name].append(leg())
        _summarise(os.path.join(out_dir, f"{what}.jsonl"), what, list(legs), runs,
                   {**extra, "clock": f"device events around {inner} calls back to back", "reps_per_run": reps})
    c = d_counts.cpu().numpy().view(X.EGRESS_COUNTS_DTYPE)[0]
    assert int(c["n"]) == 64 and int(c["n_tx"]) + int(c["n_free"]) == 64, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--egress", action="store_true", help="the comparisons of DESIGN.md 9.3 instead (profiles/egress/)")
    ap.add_argument("--ingress", action="store_true", help="the two A/B comparisons of DESIGN.md 9.2 instead")
    ap.add_argument("--out", default="", help="--ingress / --egress: where the lines go (profiles/ingress, "
                                              "profiles/egress)")
    ap.add_argument("--lib", default="")
    ap.add_argument("--opts", type=lambda x: int(x, 0), default=0, help="XSK_GPU_OPT_* word for the filter and the echo")
    ap.add_argument("--traffic", choices=["synth", "dual"], default="synth")
    args = ap.parse_args()
    if args.lib and args.opts:
        ap.error("--lib times xsk_gpu_classify_dev of another build: it takes no option word")
    if args.ingress or args.egress:
        if args.lib or args.traffic != "synth" or (args.ingress and args.egress):
            ap.error("--ingress and --egress each compare this build's entry points on the synthetic slab")
        args.out = args.out or os.path.join(ROOT, "profiles", "egress" if args.egress else "ingress")
        return egress_compare(args) if args.egress else ingress_compare(args)
    n, stride, reps = 1 << 20, 2048, 20
    dev = torch.device("cuda:0")

    def classify(umem, descs, n, bound, act, out, nout, ws):
        X.classify_dev(umem, descs, n, bound, act, out, nout, ws, opts=args.opts)

    if args.lib:
        L = C.CDLL(os.path.abspath(args.lib))
        L.xsk_gpu_classify_dev.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.xsk_gpu_classify_dev.restype = C.c_int
        L.xsk_gpu_classify_workspace_size.argtypes = [C.c_uint32]
        L.xsk_gpu_classify_workspace_size.restype = C.c_size_t

        def classify(umem, descs, n, bound, act, out, nout, ws):
            rc = L.xsk_gpu_classify_dev(umem.data_ptr(), umem.numel(), descs.data_ptr(), n, 1 if bound else 0,
                                        act.data_ptr(), out.data_ptr(), nout.data_ptr(), ws.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc
    if args.traffic == "dual":
        import numpy as np

        from tests.classify_wire import tile_batch
        from tests.v6_frames import mixed_batch6
        h_umem, h_descs = mixed_batch6(4096, stride, seed=7)
        h_umem, h_descs, _ = tile_batch(h_umem, h_descs, np.zeros(len(h_descs), np.uint8), n, stride)
        umem = torch.from_numpy(h_umem).to(dev)
        descs = torch.from_numpy(h_descs.view(np.uint8).reshape(-1)).to(dev)
    else:
        umem = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
        descs = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        X.synth_dev(umem, descs, n, 0, stride, 0x5EED0E0E, 0, 1, 1, 20, 1500)  # mixed traffic
    act = torch.empty(n, dtype=torch.uint8, device=dev)
    red = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    nred = torch.zeros(1, dtype=torch.int64, device=dev)
    wsz = int(X.lib().xsk_gpu_classify_workspace_size(n))
    if args.lib:
        wsz = max(wsz, int(L.xsk_gpu_classify_workspace_size(n)))
    ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
    for _ in range(3):
        classify(umem, descs, n, True, act, red, nred, ws)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        classify(umem, descs, n, True, act, red, nred, ws)
    e1.record()
    torch.cuda.synchronize()
    t_cls = e0.elapsed_time(e1) / reps / 1e3
    k = int(nred.cpu().view(torch.int32)[0].item())
    # filter -> echo on the redirected frames (echo re-armed between reps, untimed)
    verd = torch.empty(max(k, 1), dtype=torch.uint8, device=dev)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    ews = torch.zeros(X.workspace_size(0, k), dtype=torch.uint8, device=dev)
    t_pipe = 0.0
    for _ in range(reps):
        a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        classify(umem, descs, n, True, act, red, nred, ws)
        X.echo_dev(umem, red, k, verd, None, stats, ews, opts=args.opts)
        a1.record()
        if args.traffic == "synth":
            X.rearm_dev(umem, red, verd, k)
        torch.cuda.synchronize()
        t_pipe += a0.elapsed_time(a1) / 1e3
    t_pipe /= reps
    algo = n * (16 + 64 + 1) + k * 16
    extra = {"opts": args.opts, "traffic": args.traffic} if args.opts or args.traffic != "synth" else {}
    print(json.dumps({"lib": args.lib or "libxsknet_amd.so", **extra, "frames": n, "redirected": k, "classify_us": round(t_cls * 1e6, 2),
                      "classify_mframes_s": round(n / t_cls / 1e6, 1),
                      "classify_gbs_algorithmic": round(algo / t_cls / 1e9, 1),
                      "filter_plus_echo_us": round(t_pipe * 1e6, 2),
                      "filter_plus_echo_mframes_s": round(n / t_pipe / 1e6, 1)}))


if __name__ == "__main__":
    main()
