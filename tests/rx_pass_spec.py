"""The spec of xsk_gpu_rx_pass_end_dev and xsk_gpu_rx_pass_step_dev (include/xsk_gpu.h) in numpy: the end rule written
sequentially, one plain loop over the received frames, and the step composed from rx_steer_spec's pieces.

    r = min(plan.received, n_max);  o_p, n_p, t_p, f_p as in rx_steer_spec.spec_end_ports
    room_s = free(stack), 0 without a stack ring;  Q = the PASS frames below r;  s = min(Q, room_s)
    for i < r in batch order:  REDIRECT: on some port's list;
                               PASS and fewer than s taken so far: descs[i], all 16 bytes, onto the stack ring;
                               otherwise (DROP, PASS beyond s, any other byte): descs[i].addr into the rest
    the pool's list = the ports' free lists as before, then the rest;  stack.prod += s;  rx.cons += r
"""
import numpy as np

import oracle
from tests import egress_ports_spec as EP
from tests import ingress_spec as IS
from tests import rx_dev_spec as RS
from tests import rx_steer_spec as RP
from tests import steer_spec as SS

RESULT_DTYPE = np.dtype([("received", "<u4"), ("redirected", "<u4"), ("replied", "<u4"), ("tx_full", "<u4"),
                         ("refilled", "<u4"), ("freed", "<u4"), ("passed", "<u4"), ("pass_full", "<u4")])
assert RESULT_DTYPE.itemsize == 32
RESULT_KEYS = RESULT_DTYPE.names


def spec_end_pass(rx: RS.RingState, txs, stack, pool: RS.PoolState, plan: dict, descs: np.ndarray, actions: np.ndarray,
                  off, d_tx: np.ndarray, d_free: np.ndarray, counts, n_max: int):
    """The ring half with a stack ring (`stack`: a RingState of descriptors, or None).  Returns the result as a dict."""
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
    room_s = stack.free() if stack is not None else 0
    taken = n_pass = 0
    for i in range(r):
        a = int(actions[i])
        if a == SS.XDP_REDIRECT:
            continue
        if a == SS.XDP_PASS:
            n_pass += 1
            if taken < room_s:
                stack.entries[stack.slot(stack.prod + taken)] = descs[i]
                taken += 1
                continue
        push.append(int(descs[i]["addr"]))
    if stack is not None:
        stack.prod = (stack.prod + taken) & RS.M32
    n = pool.n()
    pushed = min(len(push), pool.capacity - n)
    for j in range(pushed):
        pool.addr[n + j] = push[j]
    pool.n_free = n + pushed
    rx.cons = (rx.cons + r) & RS.M32
    return dict(received=r, redirected=o[n_ports], replied=replied, tx_full=tx_full, refilled=plan["refilled"],
                freed=pushed, passed=taken, pass_full=n_pass - taken)


def spec_step_pass(umem: np.ndarray, rx: RS.RingState, fill: RS.RingState, txs, stack, pool: RS.PoolState,
                   max_batch: int, opts: int, table: dict, default_port: int, bound: int = SS.ALL_BOUND,
                   stats: dict = None, port_stats: list = None):
    """rx_steer_spec.spec_step_steer with spec_end_pass as its last piece: the same arguments, `stack` behind `txs`,
    and the same dict, the result with `passed` and `pass_full`."""
    n_ports = len(txs)
    descs = np.zeros(max_batch, oracle.DESC_DTYPE)
    plan = RS.spec_begin(rx, fill, txs[0], pool, max_batch, descs)
    rooms = RP.spec_prepare(txs, plan, descs, max_batch)
    ing = SS.spec_ingress_steer(umem, descs, opts, table, default_port, n_ports, bound)
    total = int(ing["off"][n_ports])
    out = np.zeros(max_batch, oracle.DESC_DTYPE)
    out[:total] = ing["out"]
    verd = np.full(max_batch, 0xFF, np.uint8)
    verd[:total] = ing["verdicts"]
    ep = EP.spec_egress_ports(out, verd, ing["off"], n_ports, max_batch, rooms)
    d_tx, d_free = RP.flat_lists(ep, max_batch)
    res = spec_end_pass(rx, txs, stack, pool, plan, descs, ing["actions"], ing["off"], d_tx, d_free, ep["counts"],
                        max_batch)
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
