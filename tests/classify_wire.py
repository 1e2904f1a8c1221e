"""The spec of xsk_gpu_classify_dev_opts over a batch, and batches large enough for the scan at no Python cost.

spec_classify_batch() adds the descriptor rule to tests/golden/make_classify_wire_golden.classify(); tile_batch()
replicates a base batch (frames, descriptors, expected actions) at a fixed stride, so a batch of a quarter of a million
frames costs one spec run over a few thousand.
"""
import importlib.util
import json
import os

import numpy as np

from tests.wire_frames import G_DESC

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_classify_wire_golden",
                                               os.path.join(_HERE, "golden", "make_classify_wire_golden.py"))
GC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GC)

XDP_DROP, XDP_PASS, XDP_REDIRECT = GC.XDP_DROP, GC.XDP_PASS, GC.XDP_REDIRECT
MAX_LEN = 1 << 30  # XSK_GPU_MAX_LEN


def golden():
    with open(os.path.join(_HERE, "golden", "classify_wire.json")) as f:
        return json.load(f)


def spec_classify_batch(umem: np.ndarray, descs: np.ndarray, opts: int, bound: bool = True):
    """(actions, redirected descriptors in batch order) of the header's spec for nonzero opts.  Rule 1: a descriptor
    with len > 2^30 or whose [addr, addr + len) leaves the UMEM is DROP."""
    n = len(descs)
    act = np.zeros(n, np.uint8)
    for i in range(n):
        a, L = int(descs[i]["addr"]), int(descs[i]["len"])
        if L > MAX_LEN or a > umem.size or L > umem.size - a:
            act[i] = XDP_DROP
            continue
        act[i] = GC.classify(umem[a:a + min(L, 128)].tobytes(), L, opts, bound)  # the spec reads below byte 70
    return act, np.ascontiguousarray(descs[act == XDP_REDIRECT])


def tile_batch(umem: np.ndarray, descs: np.ndarray, actions: np.ndarray, n: int, stride: int):
    """(umem, descs, actions) of n frames: the base batch -- len(descs) frames, frame i inside
    [i * stride, (i + 1) * stride) -- repeated back to back and cut at n frames."""
    nb = len(descs)
    span = nb * stride
    assert (descs["addr"] // stride == np.arange(nb)).all() and ((descs["addr"] % stride) + descs["len"] <= stride).all()
    reps = (n + nb - 1) // nb
    big = np.tile(umem[:span], reps)
    d = np.tile(descs, reps)
    d["addr"] += np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(span), nb)
    return big[:n * stride].copy(), np.ascontiguousarray(d[:n]), np.tile(actions, reps)[:n].copy()


def family(umem: np.ndarray, desc, opts: int) -> int:
    """4 / 6 / 0: the family rule 3 of the spec arrives at (inner ethertype 0x0800 / 0x86DD / anything else, a frame
    too short to say included).  Classes of a batch, not part of the spec."""
    a, L = int(desc["addr"]), int(desc["len"])
    if L < 14 or a + L > umem.size:
        return 0
    f = umem[a:a + min(L, 24)].tobytes()
    l3, et, tags = 14, (f[12] << 8) | f[13], 0
    if opts & GC.OPT_VLAN:
        while tags < 2 and et in (0x8100, 0x88A8):
            if L < l3 + 4:
                return 0
            et = (f[l3 + 2] << 8) | f[l3 + 3]
            l3 += 4
            tags += 1
    return {0x0800: 4, 0x86DD: 6}.get(et, 0)
