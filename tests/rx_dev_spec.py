"""The spec of xsk_gpu_rx_begin_dev, xsk_gpu_rx_end_dev, xsk_gpu_rx_step_dev and xsk_gpu_tx_complete_dev
(include/xsk_gpu.h) in numpy: the sequential rule over (index words, entry arrays, pool) as plain arrays.

    used(r) = min((producer - consumer) mod 2^32, size),  free(r) = size - used(r),  pool_n = min(n_free, capacity)

Every function changes the state it is given in place, one entry at a time, as the host's xsk_gpu_rx_step() walks its
rings; tests/test_rx_dev_spec.py compares it with the host functions themselves.
"""
import numpy as np

import oracle
from tests import egress_spec as ES
from tests import ingress_spec as IS

M32 = 0xFFFFFFFF
PLAN_DTYPE = np.dtype([("received", "<u4"), ("tx_room", "<u4"), ("refilled", "<u4"), ("rx_cons", "<u4"),
                       ("fq_prod", "<u4"), ("pool_n", "<u4"), ("reserved", "<u4", (2,))])
RESULT_DTYPE = np.dtype([("received", "<u4"), ("replied", "<u4"), ("tx_full", "<u4"), ("refilled", "<u4")])
assert PLAN_DTYPE.itemsize == 32 and RESULT_DTYPE.itemsize == 16


class RingState:
    """A ring: two free-running 32-bit words and `size` entries (oracle.DESC_DTYPE for RX / TX, uint64 for fill /
    completion)."""

    def __init__(self, entries: np.ndarray, prod: int = 0, cons: int = 0):
        size = len(entries)
        assert size >= 1 and size & (size - 1) == 0 and entries.dtype in (oracle.DESC_DTYPE, np.dtype(np.uint64))
        self.entries, self.size, self.prod, self.cons = entries, size, prod & M32, cons & M32

    def copy(self):
        return RingState(self.entries.copy(), self.prod, self.cons)

    def used(self) -> int:
        return min((self.prod - self.cons) & M32, self.size)

    def free(self) -> int:
        return self.size - self.used()

    def slot(self, idx: int) -> int:
        return idx & (self.size - 1)

    def produce(self, items) -> None:
        """A peer's producer: the items behind the producer word (the caller keeps within free())."""
        for it in items:
            self.entries[self.slot(self.prod)] = it
            self.prod = (self.prod + 1) & M32

    def same(self, other) -> bool:
        return (self.prod, self.cons) == (other.prod, other.cons) and (self.entries == other.entries).all()


class PoolState:
    """The free-frame stack: `capacity` addresses and the count word."""

    def __init__(self, addr: np.ndarray, n_free: int):
        assert addr.dtype == np.uint64 and len(addr) >= 1
        self.addr, self.capacity, self.n_free = addr, len(addr), n_free & M32

    def copy(self):
        return PoolState(self.addr.copy(), self.n_free)

    def n(self) -> int:
        return min(self.n_free, self.capacity)

    def same(self, other) -> bool:
        """The count and the stack below it (what lies above the count is not part of the pool)."""
        return self.n_free == other.n_free and (self.addr[:self.n()] == other.addr[:other.n()]).all()


def spec_begin(rx: RingState, fill: RingState, tx: RingState, pool: PoolState, max_batch: int, descs: np.ndarray):
    """Steps 1 and 2.  `descs` (max_batch entries of DESC_DTYPE) receives the batch; returns the plan as a dict."""
    assert 1 <= max_batch <= len(descs)
    rcvd = min(rx.used(), max_batch)
    plan = dict(received=rcvd, tx_room=tx.free(), refilled=0, rx_cons=rx.cons, fq_prod=fill.prod, pool_n=pool.n())
    if rcvd == 0:
        return plan
    stock = min(fill.free(), pool.n())
    n = pool.n()
    for i in range(stock):
        n -= 1
        fill.entries[fill.slot(fill.prod + i)] = pool.addr[n]  # the LIFO pop
    fill.prod = (fill.prod + stock) & M32
    pool.n_free = n  # (a count word above the capacity ends clamped)
    for i in range(rcvd):
        descs[i] = rx.entries[rx.slot(rx.cons + i)]
    plan["refilled"] = stock
    return plan


def spec_end(rx: RingState, tx: RingState, pool: PoolState, plan: dict, d_tx: np.ndarray, d_free: np.ndarray,
             counts: dict, n_max: int):
    """The ring half of step 4, and step 5.  Returns the result as a dict."""
    n_tx = min(counts["n_tx"], n_max, tx.free())
    for k in range(n_tx):
        tx.entries[tx.slot(tx.prod + k)] = d_tx[k]
    tx.prod = (tx.prod + n_tx) & M32
    n = pool.n()
    pushed = min(min(counts["n_free"], n_max), pool.capacity - n)
    for j in range(pushed):
        pool.addr[n + j] = d_free[j]
    pool.n_free = n + pushed
    release = min(plan["received"], n_max)
    rx.cons = (rx.cons + release) & M32
    return dict(received=release, replied=n_tx, tx_full=counts["n_tx_full"], refilled=plan["refilled"])


def spec_step(umem: np.ndarray, rx: RingState, fill: RingState, tx: RingState, pool: PoolState, max_batch: int,
              opts: int, stats: dict = None, verdicts_out: list = None):
    """begin, the transform (tests/ingress_spec.spec_transform: the C oracle, or the dual-stack spec) over the batch in
    `umem`, egress_spec.spec_egress, end.  `stats` (a dict of the four counters) is accumulated."""
    descs = np.zeros(max_batch, oracle.DESC_DTYPE)
    plan = spec_begin(rx, fill, tx, pool, max_batch, descs)
    n = plan["received"]
    if n:
        verd, _, st = IS.spec_transform(umem, descs[:n], opts)
    else:
        verd, st = np.zeros(0, np.uint8), dict.fromkeys(IS.KEYS, 0)
    d_tx, d_free, counts, dp, db = ES.spec_egress(descs, verd, n, plan["tx_room"])
    if stats is not None:
        for k in IS.KEYS:
            stats[k] += st[k]
        stats["tx_packets"] += dp
        stats["tx_bytes"] += db
    if verdicts_out is not None:
        verdicts_out.append(verd)
    return spec_end(rx, tx, pool, plan, d_tx, d_free, counts, max_batch)


def spec_complete(comp: RingState, pool: PoolState, max_entries: int) -> int:
    """xsk_gpu_tx_complete(): returns the count moved off the ring."""
    n = min(comp.used(), max_entries)
    cnt = pool.n()
    pushed = min(n, pool.capacity - cnt)
    for j in range(pushed):
        pool.addr[cnt + j] = comp.entries[comp.slot(comp.cons + j)]
    pool.n_free = cnt + pushed
    comp.cons = (comp.cons + n) & M32
    return n
