"""The spec of xsk_gpu_tx_complete_rings_dev (include/xsk_gpu.h) in numpy, stated twice:

    spec_complete_rings         the literal loop: rx_dev_spec.spec_complete over ring 0, 1, ... in turn;
    spec_complete_rings_prefix  the prefix formulation of the header: pool_n, room, n_q, A_q, p_q.

Both change the state they are given in place and return (moved, pushed): the list of n_q and A_{n_rings}.
tests/test_tx_complete_rings_spec.py holds them against each other and against the host's xsk_gpu_tx_complete().
"""
from tests import rx_dev_spec as RS

M32 = RS.M32
MAX_RINGS = 65


def spec_complete_rings(comps, pool: RS.PoolState, max_entries: int):
    if max_entries == 0:  # the call launches nothing: no word is stored, a count word above the capacity stays
        return [0] * len(comps), 0
    before = pool.n()
    moved = [RS.spec_complete(c, pool, max_entries) for c in comps]
    return moved, pool.n() - before


def spec_complete_rings_prefix(comps, pool: RS.PoolState, max_entries: int):
    if max_entries == 0:
        return [0] * len(comps), 0
    pool_n = min(pool.n_free, pool.capacity)
    room = pool.capacity - pool_n
    n = [min(c.used(), max_entries) for c in comps]
    A = [0]
    for q in range(len(comps)):
        A.append(A[q] + min(n[q], room - A[q]))
    assert all(a <= room for a in A)
    for q, c in enumerate(comps):
        for j in range(A[q + 1] - A[q]):
            pool.addr[pool_n + A[q] + j] = c.entries[(c.cons + j) & (c.size - 1)]
    for q, c in enumerate(comps):
        c.cons = (c.cons + n[q]) & M32
    pool.n_free = pool_n + A[-1]
    return n, A[-1]
