#!/usr/bin/env python3
"""xsk_gpu_rearm_dev alone (GPU box): 1 M frames at the bench's layouts, cold, several implementations in one session.

Per layout a pool of batches larger than the 256 MiB Infinity Cache.  A run of one implementation: a real
xsk_gpu_echo_dev pass over every batch (untimed: its verdicts drive the re-arm), 1 GiB of other traffic so that nothing
of the pool is cached, then one pair of HIP events around the pool's back-to-back re-arm calls on one stream, a fresh
batch per call; the figure is microseconds per call.  The implementations alternate run by run inside every round.
Round 0 is a warm-up and is not counted; in it every batch is compared with the generator's output after the re-arm,
the whole slab, and every difference is reported, so an implementation that skips or misplaces a store cannot pass
as fast.

    python tools/rearm_bench.py [--layouts c5,c3,c4,c2] [--rounds 5] [--impls new,floor3,v4,...]
                                [--parent PATH/libxsknet_amd.so] [--out FILE.jsonl]

Implementations: `new` the library of this tree, `parent` another build of it (--parent), `floor3` tools/c2floor.hip
mode 3 (four lanes per frame: descriptor and 64 B read, 64 B, a record and a verdict written; it leaves the frames as
they are), `vN` instance N of tools/rearm_variants.hip (N = nt | bcast << 1 | fpl_index << 2 | stride << 4).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import xsknet_amd as X  # noqa: E402
from bench import CONFIGS  # noqa: E402

_P = C.c_void_p


def tool_lib(name):
    """tools/lib<name>.so, rebuilt when it is missing or older than its source or the re-arm header it may include."""
    so, src = os.path.join(HERE, f"lib{name}.so"), os.path.join(HERE, f"{name}.hip")
    deps = [src, os.path.join(os.path.dirname(HERE), "xsknet_amd", "csrc", "xsk_rearm_device.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in deps):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so,
                        src], check=True)
    return C.CDLL(so)


def variant_name(v):
    return f"fpl{(1, 2, 4)[(v >> 2) & 3]}{'_nt' if v & 1 else ''}{'_bcast' if v & 2 else ''}{'_stride' if v & 16 else ''}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layouts", default="c5,c3,c4,c2")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pool", type=int, default=8)
    ap.add_argument("--impls", default="new,floor3")
    ap.add_argument("--parent", default=None, help="another build of libxsknet_amd.so, timed as `parent`")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    impls = ([] if args.parent is None else ["parent"]) + args.impls.split(",")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    n = 1 << 20

    calls = {}
    if args.parent is not None:
        par = C.CDLL(os.path.abspath(args.parent))
        par.xsk_gpu_rearm_dev.argtypes = [_P, _P, _P, C.c_uint32, _P]
        calls["parent"] = lambda u, d, v, fv, fr: par.xsk_gpu_rearm_dev(u.data_ptr(), d.data_ptr(), v.data_ptr(), n, sp)
    calls["new"] = lambda u, d, v, fv, fr: X.lib().xsk_gpu_rearm_dev(u.data_ptr(), d.data_ptr(), v.data_ptr(), n, sp)
    if "floor3" in impls:
        fl = tool_lib("c2floor")
        fl.c2floor_run.argtypes = [C.c_int, _P, _P, _P, _P, C.c_uint32, _P]
        calls["floor3"] = lambda u, d, v, fv, fr: fl.c2floor_run(3, u.data_ptr(), d.data_ptr(), fv.data_ptr(),
                                                                 fr.data_ptr(), n, sp)
    if any(i[0] == "v" for i in impls):
        va = tool_lib("rearm_variants")
        va.rearm_variant_run.argtypes = [C.c_int, _P, _P, _P, C.c_uint32, _P]
        for i in impls:
            if i[0] == "v":
                calls[i] = (lambda k: lambda u, d, v, fv, fr: va.rearm_variant_run(k, u.data_ptr(), d.data_ptr(),
                                                                                   v.data_ptr(), n, sp))(int(i[1:]))

    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    flush = torch.zeros(1 << 30, dtype=torch.uint8, device=dev)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    ws = torch.zeros(max(1 << 20, X.workspace_size(0, n)), dtype=torch.uint8, device=dev)
    recs = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    fverd = torch.zeros(n, dtype=torch.uint8, device=dev)
    frecs = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    for layout in args.layouts.split(","):
        _, lo, hi, stride, seed, _ = CONFIGS[layout]
        sets = []
        for b in range(args.pool):
            u = torch.zeros(n * stride, dtype=torch.uint8, device=dev)  # zeros: the gaps between frames are compared too
            d = torch.empty(n * 16, dtype=torch.uint8, device=dev)
            X.synth_dev(u, d, n, 0, stride, seed + b, 0, 1, 0, lo, hi)
            sets.append((u, d, torch.zeros(n, dtype=torch.uint8, device=dev)))
        want = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
        wdesc = torch.empty(n * 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        times = {i: [] for i in impls}
        wrong = {i: [] for i in impls}  # batches whose slab differs from the generator's after the re-arm
        for r in range(args.rounds + 1):
            for i in impls[r % len(impls):] + impls[:r % len(impls)]:  # the order rotates round by round
                for (u, d, v) in sets:
                    X.echo_dev(u, d, n, v, recs, stats, ws, stream)
                flush.add_(1)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for (u, d, v) in sets:
                    rc = calls[i](u, d, v, fverd, frecs)
                    assert rc == 0, (i, rc)
                e1.record(stream)
                torch.cuda.synchronize()
                if i == "floor3":  # the frames are still replies: restore them for the next run
                    for (u, d, v) in sets:
                        X.rearm_dev(u, d, v, n, stream)
                if r == 0:
                    for b, (u, d, v) in enumerate(sets):
                        assert bool((v == 0).all().item()), (layout, i, b, "verdicts")
                        want.zero_()  # ragged frames: the last batch's longer ones must not stay behind
                        X.synth_dev(want, wdesc, n, 0, stride, seed + b, 0, 1, 0, lo, hi)
                        if not torch.equal(u, want):
                            fr = torch.nonzero((u != want).view(n, stride).any(dim=1)).view(-1)
                            first = []
                            for f in fr[:4].tolist():
                                g, w = u[f * stride:(f + 1) * stride], want[f * stride:(f + 1) * stride]
                                at = torch.nonzero(g != w).view(-1)[:6]
                                first.append({"frame": f, "len": int(d.view(torch.int32).view(-1, 4)[f, 2].item()),
                                              "at": at.tolist(), "got": g[at].tolist(), "want": w[at].tolist()})
                            wrong[i].append({"batch": b, "frames": int(fr.numel()), "first": first})
                            u.copy_(want)
                else:
                    times[i].append(e0.elapsed_time(e1) * 1e3 / len(sets))
        base = float(np.median(times["parent"])) if "parent" in times else None
        floor = float(np.median(times["floor3"])) if "floor3" in times else None
        for i in impls:
            t = times[i]
            med = float(np.median(t))
            emit({"layout": layout, "frame_len": [lo, hi], "stride": stride, "frames": n, "impl": i,
                  **({"variant": variant_name(int(i[1:]))} if i[0] == "v" else {}),
                  "us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                  "spread": round((max(t) - min(t)) / med, 4), "runs_us": [round(x, 2) for x in t],
                  "tbs": round(n * (161 if i == "floor3" else 145) / (med * 1e-6) / 1e12, 3),
                  "ratio_to_parent": round(med / base, 4) if base else None,
                  "ratio_to_floor3": round(med / floor, 4) if floor else None,
                  "pool": len(sets), "slab_vs_generator_after_rearm": wrong[i] or "equal, every batch (round 0)"})
        del sets, want, wdesc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
