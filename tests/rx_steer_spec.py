"""The spec of xsk_gpu_rx_prepare_ports_dev, xsk_gpu_rx_ports_end_dev and xsk_gpu_rx_step_steer_dev (include/xsk_gpu.h)
in numpy: a composition of rx_dev_spec.spec_begin, steer_spec.spec_ingress_steer and egress_ports_spec.spec_egress_ports
with the prepare and end rules written sequentially, one entry at a time, over rx_dev_spec's RingState / PoolState.

    r = min(plan.received, n_max);  o_p = the clamped running maximum of off;  n_p = o_{p+1} - o_p
    prepare: room[p] = free(tx[p]);  descs[r:n_max] = the pad descriptor (0, 0, 0)
    end:     per port t_p = min(counts[p].n_tx, n_p, free(tx[p])) entries of d_tx[o_p:] onto tx[p];
             the pool's list = for ascending p d_free[o_p : o_p + min(counts[p].n_free, n_p)], then descs[i].addr for
             i < r with actions[i] != REDIRECT; the first min(len, capacity - pool_n) are pushed;  rx.cons += r
"""
import numpy as np

import oracle
from tests import egress_ports_spec as EP
from tests import ingress_spec as IS
from tests import rx_dev_spec as RS
from tests import steer_spec as SS

RESULT_DTYPE = np.dtype([("received", "<u4"), ("redirected", "<u4"), ("replied", "<u4"), ("tx_full", "<u4"),
                         ("refilled", "<u4"), ("freed", "<u4"), ("reserved", "<u4", (2,))])
assert RESULT_DTYPE.itemsize == 32
RESULT_KEYS = RESULT_DTYPE.names[:6]
PAD = np.zeros(1, oracle.DESC_DTYPE)[0]


def spec_prepare(txs, plan: dict, descs: np.ndarray, n_max: int):
    """The rooms (a list, one per port); descs[r:n_max] padded in place."""
    r = min(plan["received"], n_max)
    for i in range(r, n_max):
        descs[i] = PAD
    return [t.free() for t in txs]


def spec_end_ports(rx: RS.RingState, txs, pool: RS.PoolState, plan: dict, descs: np.ndarray, actions: np.ndarray, off,
                   d_tx: np.ndarray, d_free: np.ndarray, counts, n_max: int):
    """The ring half.  `counts`: per-port dicts with n_tx / n_tx_full / n_free.  Returns the result as a dict."""
    n_ports = len(txs)
    o = EP.offsets(off, n_ports, n_max)
    r = min(plan["received"], n_max)
    replied = tx_full = 0
    push = []
    for p, tx in enumerate(txs):
        n_p = o[p + 1] - o[p]
        t_p = min(counts[p]["n_tx"], n_p, tx.free())
        for k in range(t_p):
            tx.entries[tx.slot(tx.prod + k)] = d_tx[o[p] + k]
        tx.prod = (tx.prod + t_p) & RS.M32
        replied += t_p
        tx_full = (tx_full + counts[p]["n_tx_full"]) & RS.M32
        push += [int(a) for a in d_free[o[p]:o[p] + min(counts[p]["n_free"], n_p)]]
    push += [int(descs[i]["addr"]) for i in range(r) if actions[i] != SS.XDP_REDIRECT]
    n = pool.n()
    pushed = min(len(push), pool.capacity - n)
    for j in range(pushed):
        pool.addr[n + j] = push[j]
    pool.n_free = n + pushed
    rx.cons = (rx.cons + r) & RS.M32
    return dict(received=r, redirected=o[n_ports], replied=replied, tx_full=tx_full, refilled=plan["refilled"],
                freed=pushed)


def flat_lists(ep: dict, n_max: int, fill: int = 0):
    """d_tx and d_free (n_max entries each) as xsk_gpu_egress_ports_dev leaves them in arrays pre-filled with the byte
    `fill`: port p's lists at o_p."""
    d_tx = np.full(n_max * 16, fill, np.uint8).view(oracle.DESC_DTYPE)
    d_free = np.full(n_max * 8, fill, np.uint8).view(np.uint64)
    for p, o_p in enumerate(ep["o"][:-1]):
        d_tx[o_p:o_p + len(ep["tx"][p])] = ep["tx"][p]
        d_free[o_p:o_p + len(ep["free"][p])] = ep["free"][p]
    return d_tx, d_free


def spec_step_steer(umem: np.ndarray, rx: RS.RingState, fill: RS.RingState, txs, pool: RS.PoolState, max_batch: int,
                    opts: int, table: dict, default_port: int, bound: int = SS.ALL_BOUND, stats: dict = None,
                    port_stats: list = None):
    """begin (against port 0's ring), prepare, the steered ingress over all max_batch descriptors, the per-port egress
    against the rooms prepare read, end.  UMEM, rings and pool change in place; `stats` (a dict of the four counters)
    and `port_stats` (a list of such dicts, one per port) are accumulated.  Returns a dict: result, plan, rooms, actions,
    ports (max_batch each), off, counts (per-port dicts), verdicts (by position in the steered list)."""
    n_ports = len(txs)
    descs = np.zeros(max_batch, oracle.DESC_DTYPE)
    plan = RS.spec_begin(rx, fill, txs[0], pool, max_batch, descs)
    rooms = spec_prepare(txs, plan, descs, max_batch)
    ing = SS.spec_ingress_steer(umem, descs, opts, table, default_port, n_ports, bound)
    total = int(ing["off"][n_ports])
    out = np.zeros(max_batch, oracle.DESC_DTYPE)
    out[:total] = ing["out"]
    verd = np.full(max_batch, 0xFF, np.uint8)
    verd[:total] = ing["verdicts"]
    ep = EP.spec_egress_ports(out, verd, ing["off"], n_ports, max_batch, rooms)
    d_tx, d_free = flat_lists(ep, max_batch)
    res = spec_end_ports(rx, txs, pool, plan, descs, ing["actions"], ing["off"], d_tx, d_free, ep["counts"], max_batch)
    if stats is not None:
        for k in IS.KEYS:
            stats[k] += ing["stats"][k]
        stats["tx_packets"] += ep["d_tx_packets"]
        stats["tx_bytes"] += ep["d_tx_bytes"]
    if port_stats is not None:
        for p in range(n_ports):
            for k in EP.STATS_KEYS:
                port_stats[p][k] += ep["port_stats"][p][k]
    return dict(result=res, plan=plan, rooms=rooms, actions=ing["actions"], ports=ing["ports"], off=ing["off"],
                counts=ep["counts"], verdicts=ing["verdicts"], descs=descs)
