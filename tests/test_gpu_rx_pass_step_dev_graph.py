"""xsk_gpu_tx_complete_dev over the stack's completion ring and xsk_gpu_rx_pass_step_dev behind it, captured once and
replayed: the chunks the stack's consumer has finished with return to the pool, then a whole steered RX loop iteration
runs with the frames the filter passes put on the stack ring.  Nothing is frozen into the capture but pointers, sizes
and the bound; every index, count and the bound mask is device memory that the replay reads when it executes.  Between
replays the test plays the peers on the device: the stack's consumer moves the stack ring's entries to the completion
ring (a device gather and scatter) and advances both rings' words, new RX entries arrive, the TX and fill rings are
consumed, *d_bound is rewritten.  One replay meets a full stack ring, one an empty RX ring.  One linear chain on the
capture stream: no parallel branches."""
from collections import Counter

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import egress_ports_spec as EP  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests import rx_dev_spec as RS  # noqa: E402
from tests import rx_pass_spec as PS  # noqa: E402
from tests import steer_spec as SS  # noqa: E402
from tests.test_gpu_ingress import _dev, stats_of, to_dev  # noqa: E402
from tests.test_gpu_rx_pass_step_dev import PassState, make_stack  # noqa: E402
from tests.test_gpu_rx_step_dev import WRAP, DevRing, Guarded  # noqa: E402
from tests.test_gpu_rx_step_steer_dev import _table, _traffic, make_state, port_stats_of  # noqa: E402

SIZE, MAX_BATCH, OPTS, N_PORTS, STACK_SIZE = 64, 48, 0x17, 3, 16
EMPTY, FULL = 2, 4  # the replay that meets an empty RX ring, and the one that meets a full stack ring
OFFERS = [40, 48, 0, 55, 33, 41]  # frames the peer puts on the RX ring before each replay (55 > max_batch: 7 stay)
BOUNDS = [SS.ALL_BOUND, SS.ALL_BOUND & ~2, SS.ALL_BOUND, SS.ALL_BOUND & ~4, SS.ALL_BOUND, 1]


def census(rx, fill, txs, stack, comp, pool) -> Counter:
    """The multiset of chunk addresses the six containers hold: every ring's unconsumed entries, the pool below its
    count."""
    c = Counter()
    for r in (rx, fill, *txs, stack, comp):
        for j in range(r.used()):
            e = r.entries[r.slot(r.cons + j)]
            c[int(e["addr"]) if r.entries.dtype.names else int(e)] += 1
    c.update(int(a) for a in pool.addr[:pool.n()])
    return c


def test_one_capture_of_tx_complete_and_the_pass_step_replayed_six_times():
    dev = _dev()
    umem, descs = _traffic(sum(OFFERS))
    table = _table(sum(OFFERS), OPTS, N_PORTS, entries=94)
    rx, fill, txs, pool = make_state(N_PORTS, SIZE, WRAP - 20, descs[:0], SIZE // 2, SIZE, 8 * SIZE, [4096] * N_PORTS)
    stack = make_stack(STACK_SIZE, 0xFFFFFFF5, STACK_SIZE)
    comp = RS.RingState(np.arange(SIZE, dtype=np.uint64) + np.uint64(1 << 50), 0xFFFFFFE0, 0xFFFFFFE0)
    d = PassState(rx, fill, txs, stack, pool, MAX_BATCH, table, SS.ALL_BOUND)
    d_comp, d_moved = DevRing(comp), Guarded(4)
    d_umem = to_dev(umem)

    def both():
        X.tx_complete_dev(d_comp.view, d.pool.view, SIZE, moved=d_moved.data)
        d.step(d_umem, OPTS, SS.PASS)

    # outside the capture first: the library's kernels are loaded, the device is known (empty rings: nothing changes)
    both()
    torch.cuda.synchronize()
    d.check(rx, fill, txs, pool, stack)
    d.stats.zero_()
    d.port_stats.data.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    s_rx, s_fill, s_txs, s_pool, s_stack, s_comp = rx.copy(), fill.copy(), [t.copy() for t in txs], pool.copy(), \
        stack.copy(), comp.copy()
    u = umem.copy()
    st = dict.fromkeys(IS.KEYS, 0)
    pst = [dict.fromkeys(EP.STATS_KEYS, 0) for _ in txs]
    taken = passed = completed = 0
    for k, offer in enumerate(OFFERS):
        # the peers.  The stack's consumer: every entry of the stack ring onto the completion ring, on the device
        n_move = 0 if k == FULL else s_stack.used()
        if n_move:
            src = [s_stack.slot(s_stack.cons + j) for j in range(n_move)]
            dst = [s_comp.slot(s_comp.prod + j) for j in range(n_move)]
            assert s_comp.free() >= n_move
            d_comp.ent.data.view(torch.int64)[torch.tensor(dst, device=dev)] = \
                d.stack.ent.data.view(torch.int64).view(-1, 2)[torch.tensor(src, device=dev), 0]
            s_comp.entries[dst] = s_stack.entries["addr"][src]
            s_comp.prod = (s_comp.prod + n_move) & RS.M32
            s_stack.cons = (s_stack.cons + n_move) & RS.M32
            d_comp.words.put(np.array([s_comp.prod, s_comp.cons], np.uint32))
            d.stack.words.put(np.array([s_stack.prod, s_stack.cons], np.uint32))
        if k == FULL:
            assert s_stack.free() == 0  # the replay before it left the ring full
        # the wire: new RX entries, the TX rings transmitted, fill entries taken
        s_rx.produce(descs[taken:taken + offer])
        taken += offer
        assert s_rx.used() <= SIZE
        for t in s_txs:
            t.cons = t.prod
        s_fill.cons = (s_fill.cons + min(s_fill.used(), 30)) & RS.M32
        d.rx.write(s_rx)
        d.fill.write(s_fill)
        for t, dt in zip(s_txs, d.txs):
            dt.write(t)
        d.bound.copy_(torch.from_numpy(np.array([BOUNDS[k]], np.uint64).view(np.int64)))
        torch.cuda.synchronize()
        before = census(d.rx.read(), d.fill.read(), [t.read() for t in d.txs], d.stack.read(), d_comp.read(), d.pool.read())
        assert before == census(s_rx, s_fill, s_txs, s_stack, s_comp, s_pool)
        avail, q_room, comp_used = s_rx.used(), s_stack.free(), s_comp.used()
        # the spec: tx_complete, then the step
        moved = RS.spec_complete(s_comp, s_pool, SIZE)
        got = PS.spec_step_pass(u, s_rx, s_fill, s_txs, s_stack, s_pool, MAX_BATCH, OPTS, table, SS.PASS, BOUNDS[k], st, pst)
        res = got["result"]
        graph.replay()
        torch.cuda.synchronize()
        d.check(s_rx, s_fill, s_txs, s_pool, s_stack)
        g = d_comp.read()
        assert (g.prod, g.cons) == (s_comp.prod, s_comp.cons) and (g.entries == s_comp.entries).all()
        assert d_comp.words.intact() and d_comp.ent.intact() and d_moved.intact()
        assert int(d_moved.get(np.uint32)[0]) == moved == comp_used
        d.check_outputs(got)
        assert d.result() == res and stats_of(d.stats) == st and port_stats_of(d.port_stats, N_PORTS) == pst, k
        # conservation: the replay only moves chunks among the six containers
        after = census(d.rx.read(), d.fill.read(), [t.read() for t in d.txs], d.stack.read(), d_comp.read(), d.pool.read())
        assert after == before and sum(after.values()) == sum(before.values()), k
        q = int((got["actions"][:res["received"]] == SS.XDP_PASS).sum())
        assert res["received"] == min(avail, MAX_BATCH) and res["passed"] == min(q, q_room)
        assert res["pass_full"] == q - res["passed"]
        if k == EMPTY:
            assert res == dict.fromkeys(PS.RESULT_KEYS, 0) and moved >= 1  # the completion ring is served all the same
        elif k == FULL:
            assert q >= 4 and res["passed"] == 0 and res["pass_full"] == q
        else:
            assert res["passed"] >= 4
        passed += res["passed"]
        completed += moved
    assert passed > 2 * STACK_SIZE and completed >= STACK_SIZE and s_stack.prod < 0x1000  # around the ring, past 2^32
    assert s_pool.n() < s_pool.capacity and s_comp.prod < 0x1000  # nothing was dropped for want of room in the pool
    assert (d_umem.cpu().numpy() == u).all()
