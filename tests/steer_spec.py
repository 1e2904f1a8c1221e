"""The spec of xsk_gpu_steer_dev and xsk_gpu_ingress_steer_dev over a batch: tests/golden/make_steer_golden.steer() per
frame plus the descriptor rule, then the stable partition of the REDIRECT descriptors by port.

A table here is a dict {(family, 16 address bytes): port}; entries_of() turns it into the host array
xsk_gpu_steer_table_prepare() takes, sample_table() draws one from the destinations that occur in a batch, so that no
frame needs rewriting.
"""
import importlib.util
import json
import os

import numpy as np

from tests import classify_wire as CW

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_steer_golden", os.path.join(_HERE, "golden", "make_steer_golden.py"))
GS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GS)

XDP_DROP, XDP_PASS, XDP_REDIRECT = GS.XDP_DROP, GS.XDP_PASS, GS.XDP_REDIRECT
PASS, MAX_PORTS, MAX_ENTRIES = GS.PASS, GS.MAX_PORTS, 1024
ALL_BOUND = (1 << 64) - 1
MAX_LEN = 1 << 30
ENTRY_DTYPE = np.dtype([("addr", "u1", (16,)), ("family", "u1"), ("port", "u1"), ("pad", "u1", (6,))])


def golden():
    with open(os.path.join(_HERE, "golden", "steer.json")) as f:
        return json.load(f)


def golden_maps():
    """[(table dict, default_port, n_ports, bound mask)] in the order of steer.json's result lists."""
    return [(GS.TABLES[t][1], d, GS.TABLES[t][0], m) for _, t, d, m in GS.combos()]


def entries_of(table: dict) -> np.ndarray:
    """The table as an unsorted host array of struct xsk_gpu_steer_entry (insertion order)."""
    e = np.zeros(len(table), ENTRY_DTYPE)
    for i, ((fam, addr), port) in enumerate(table.items()):
        e[i]["addr"] = np.frombuffer(addr, np.uint8)
        e[i]["family"] = fam
        e[i]["port"] = port
    return e


def descriptor_ok(umem: np.ndarray, a: int, L: int, opts: int) -> bool:
    """The descriptor rule: for nonzero opts [addr, addr + len) lies inside the UMEM (rule 1); for opts == 0, as
    xsk_gpu_classify_dev(), the bytes the reference's program reads do (the first 14, or 34 from len 34 on)."""
    if L > MAX_LEN or a > umem.size:
        return False
    need = L if opts else (34 if L >= 34 else 14 if L >= 14 else 0)
    return need <= umem.size - a


def spec_steer_batch(umem: np.ndarray, descs: np.ndarray, opts: int, table: dict, default_port: int, n_ports: int,
                     bound: int = ALL_BOUND):
    """dict of actions, ports, out (the REDIRECT descriptors grouped by ascending port, batch order within a port) and
    off (n_ports + 1 offsets into out)."""
    n = len(descs)
    act = np.zeros(n, np.uint8)
    ports = np.full(n, PASS, np.uint8)
    for i in range(n):
        a, L = int(descs[i]["addr"]), int(descs[i]["len"])
        if not descriptor_ok(umem, a, L, opts):
            act[i] = XDP_DROP
            continue
        act[i], ports[i] = GS.steer(umem[a:a + min(L, 128)].tobytes(), L, opts, table, default_port, n_ports, bound)
    return partition(descs, act, ports, n_ports)


def partition(descs: np.ndarray, act: np.ndarray, ports: np.ndarray, n_ports: int):
    """The grouped list and its offsets from per-frame actions and ports, by the definition: for every port in
    ascending order, its REDIRECT frames in batch order."""
    groups = [np.nonzero((act == XDP_REDIRECT) & (ports == p))[0] for p in range(n_ports)]
    off = np.zeros(n_ports + 1, np.uint32)
    off[1:] = np.cumsum([len(g) for g in groups])
    order = np.concatenate(groups) if n_ports else np.zeros(0, np.int64)
    return dict(actions=act, ports=ports, out=np.ascontiguousarray(descs[order]), off=off, order=order)


def destinations(umem: np.ndarray, descs: np.ndarray, opts: int):
    """The keys (family, 16 bytes) of the frames the filter's rules redirect, in batch order (None for the others)."""
    keys = []
    for i in range(len(descs)):
        a, L = int(descs[i]["addr"]), int(descs[i]["len"])
        k = None
        if descriptor_ok(umem, a, L, opts):
            f = umem[a:a + min(L, 128)].tobytes()
            base = GS.GC.classify(f, L, opts, True) if opts else GS.ref_classify(f, L)
            if base == XDP_REDIRECT:
                l3, fam = GS.ip_header(f, opts)
                lo, hi = (l3 + 16, l3 + 20) if fam == 4 else (l3 + 24, l3 + 40)
                k = GS.key(f[lo:hi])
        keys.append(k)
    return keys


def sample_table(keys, n_entries: int, n_ports: int, seed: int, unicast_only: bool = False) -> dict:
    """A table of exactly n_entries keys: as many as it can take of the distinct destinations in `keys` (every second
    one, so that some frames miss), the rest addresses that do not occur; ports drawn from [0, n_ports)."""
    rng = np.random.default_rng(seed)
    seen = []
    for k in keys:
        if k is not None and k not in seen and not (unicast_only and not is_unicast(k)):
            seen.append(k)
    table = {}
    for k in seen[::2][:n_entries]:
        table[k] = int(rng.integers(0, n_ports))
    fill = 0
    while len(table) < n_entries:  # 198.18.0.0/15 and 2001:db8:ffff::/48 do not occur in the generators' traffic
        fam = 4 if fill % 2 else 6
        k = GS.key(bytes([198, 18, fill >> 8 & 0xFF, fill & 0xFF]) if fam == 4 else
                   bytes.fromhex("20010db8ffff") + fill.to_bytes(10, "big"))
        fill += 1
        if k not in table and k not in seen:
            table[k] = int(rng.integers(0, n_ports))
    return table


def is_unicast(k) -> bool:
    fam, addr = k
    if fam == 4:
        return addr[0] < 224 and addr[:4] != b"\xff\xff\xff\xff"
    return addr[0] != 0xFF


def spec_ingress_steer(umem: np.ndarray, descs: np.ndarray, opts: int, table: dict, default_port: int, n_ports: int,
                       bound: int = ALL_BOUND):
    """xsk_gpu_ingress_steer_dev over the batch, UMEM in place: spec_steer_batch, then the transform's spec
    (tests/ingress_spec.spec_transform) over the grouped list; verdicts and recs by position in out."""
    from tests import ingress_spec as IS
    ref = spec_steer_batch(umem, descs, opts, table, default_port, n_ports, bound)
    if len(ref["out"]):
        v, r, st = IS.spec_transform(umem, ref["out"], opts)
    else:
        v, r, st = np.zeros(0, np.uint8), np.zeros((0, 16), np.uint8), dict.fromkeys(IS.KEYS, 0)
    ref.update(verdicts=v, recs=r, stats=st)
    return ref


__all__ = ["CW", "GS"]
