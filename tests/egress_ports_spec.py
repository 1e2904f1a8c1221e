"""The spec of xsk_gpu_egress_ports_dev (include/xsk_gpu.h) in plain Python: the sequential rule, frame by frame.

    o_p = min(max(off[0..p]), n_max);  port p owns [o_p, o_{p+1})
    reply(i) = verdicts[i] == TX_REPLY;  R_p(i) = replies in [o_p, i)
    a reply with R_p(i) < room_p is submitted: tx[o_p + R_p(i)] = (addr, len, 0)
    every other frame of the segment is freed: free[o_p + (i - o_p) - min(R_p(i), room_p)] = addr

`spec_egress_ports` walks the positions 0 .. n_max - 1 once, keeping one open port; tests/test_egress_ports_spec.py
compares it with egress_spec.spec_egress applied to each segment, which is written independently of this batch form.
"""
import numpy as np

import oracle
from tests.egress_spec import TX_REPLY, UNLIMITED

STATS_KEYS = ("rx_packets", "rx_bytes", "tx_packets", "tx_bytes")


def offsets(off, n_ports: int, n_max: int):
    """The n_ports + 1 segment offsets of any words: the clamped running maximum."""
    o, run = [], 0
    for p in range(n_ports + 1):
        run = max(run, int(off[p]))
        o.append(min(run, n_max))
    return o


def spec_egress_ports(descs, verdicts, off, n_ports: int, n_max: int, rooms=None):
    """A dict: `o` (the offsets), `tx` / `free` (per-port lists: DESC_DTYPE with options 0, uint64 addresses), `counts`
    (per-port dicts n / n_tx / n_tx_full / n_free), `d_tx_packets` / `d_tx_bytes` (the non-positive deltas of the
    shared block) and `port_stats` (per-port dicts of the four counter deltas).  `rooms`: n_ports values or None."""
    d = np.ascontiguousarray(descs, oracle.DESC_DTYPE)
    assert 1 <= n_ports <= 64 and len(off) >= n_ports + 1 and n_max <= len(d) and n_max <= len(verdicts)
    rooms = [UNLIMITED] * n_ports if rooms is None else [int(r) for r in rooms]
    assert len(rooms) == n_ports and all(0 <= r <= UNLIMITED for r in rooms)
    o = offsets(off, n_ports, n_max)
    addrs, lens, verd = d["addr"][:n_max].tolist(), d["len"][:n_max].tolist(), np.asarray(verdicts[:n_max]).tolist()
    tx, free = [[] for _ in range(n_ports)], [[] for _ in range(n_ports)]
    below = [0] * n_ports
    ps = [dict.fromkeys(STATS_KEYS, 0) for _ in range(n_ports)]
    lost_packets = lost_bytes = 0
    p = 0
    for i in range(o[0], o[n_ports]):
        while o[p + 1] <= i:  # the port that owns i: empty segments are stepped over
            p += 1
        addr, length = addrs[i], lens[i]
        ps[p]["rx_packets"] += 1
        ps[p]["rx_bytes"] += length
        if verd[i] == TX_REPLY:
            if below[p] < rooms[p]:
                tx[p].append((addr, length, 0))
                ps[p]["tx_packets"] += 1
                ps[p]["tx_bytes"] += length
            else:
                free[p].append(addr)
                lost_packets += 1
                lost_bytes += length
            below[p] += 1
        else:
            free[p].append(addr)
    counts = []
    for q in range(n_ports):
        n_p, n_tx = o[q + 1] - o[q], min(below[q], rooms[q])
        counts.append(dict(n=n_p, n_tx=n_tx, n_tx_full=below[q] - n_tx, n_free=n_p - n_tx))
        assert len(tx[q]) == n_tx and len(free[q]) == n_p - n_tx
    return dict(o=o,
                tx=[np.array(t, oracle.DESC_DTYPE).reshape(-1) for t in tx],
                free=[np.array(f, np.uint64).reshape(-1) for f in free],
                counts=counts, d_tx_packets=-lost_packets, d_tx_bytes=-lost_bytes, port_stats=ps)


def expected_arrays(spec, n_max: int, sentinel: int = 0xEE, tail: int = 4):
    """What d_tx ((n_max + tail) * 16 bytes) and d_free ((n_max + tail) * 8 bytes) hold after a call into arrays
    pre-filled with `sentinel`: every port's lists at its offset, the sentinel everywhere else."""
    tx = np.full((n_max + tail) * 16, sentinel, np.uint8)
    free = np.full((n_max + tail) * 8, sentinel, np.uint8)
    for p, o_p in enumerate(spec["o"][:-1]):
        t, f = spec["tx"][p], spec["free"][p]
        tx[o_p * 16:(o_p + len(t)) * 16] = t.view(np.uint8)
        free[o_p * 8:(o_p + len(f)) * 8] = f.view(np.uint8)
    return tx, free


def layout(name: str, n_ports: int, n_max: int, seed: int = 0):
    """n_ports + 1 offset words with the named layout over [0, n_max]."""
    rng = np.random.default_rng(0x0FF5 + seed)
    if name == "one":         # port 0 owns everything
        off = [0] + [n_max] * n_ports
    elif name == "last":      # ... the last port does
        off = [0] * n_ports + [n_max]
    elif name == "empty":     # all segments empty
        off = [n_max // 2] * (n_ports + 1)
    elif name == "even":
        off = [(n_max * p) // n_ports for p in range(n_ports + 1)]
    elif name == "random":    # with repeats: empty segments anywhere
        off = [0] + sorted(rng.integers(0, n_max + 1, n_ports - 1).tolist()) + [n_max]
    elif name == "inner":     # off[0] > 0 and off[n_ports] < n_max: frames on no list at both ends
        a, b = n_max // 5, n_max - n_max // 7
        off = [a] + sorted(rng.integers(a, b + 1, n_ports - 1).tolist()) + [b]
    elif name == "wild":      # not ascending, above the bound
        off = rng.integers(0, n_max + n_max // 2 + 2, n_ports + 1).tolist()
        off[0] = min(off[0], n_max // 3)
        off[rng.integers(1, n_ports + 1)] = 0xFFFFFFFF if seed % 2 else n_max + 5
    else:
        raise ValueError(name)
    return [int(x) for x in off]


LAYOUTS = ("one", "last", "empty", "even", "random", "inner", "wild")
