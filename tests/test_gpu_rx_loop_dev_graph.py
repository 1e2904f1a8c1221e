"""xsk_gpu_rx_loop_dev captured once and replayed: a whole RX loop iteration over all sockets -- receive, refill, steer,
reply, per-port TX, stack ring, and every completion ring back into the pool -- with the loop closed on the device.
Nothing is frozen into the capture but pointers, sizes and the bounds; every index, count and the bound mask is device
memory that the replay reads when it executes.  Between replays the test plays the peers on the device: every TX ring's
entries are "transmitted" onto that port's completion ring and the stack ring's entries onto the fourth (device gathers
and scatters of the addresses, then the words), new RX entries arrive, fill entries are taken, *d_bound is rewritten.
One replay meets an empty RX ring (the completion rings are served all the same), one a full stack ring.  After every
replay the state is the spec's, and the multiset of chunk addresses over the RX, fill, TX, stack and completion rings
and the pool is what it was before it; the pool has room for every chunk, so none is dropped.  One linear chain on the
capture stream: no parallel branches."""
from collections import Counter

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import egress_ports_spec as EP  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests import rx_dev_spec as RS  # noqa: E402
from tests import rx_pass_spec as PS  # noqa: E402
from tests import steer_spec as SS  # noqa: E402
from tests import tx_complete_rings_spec as CS  # noqa: E402
from tests.test_gpu_ingress import _dev, stats_of, to_dev  # noqa: E402
from tests.test_gpu_rx_pass_step_dev import make_stack  # noqa: E402
from tests.test_gpu_rx_step_dev import WRAP  # noqa: E402
from tests.test_gpu_rx_step_steer_dev import _table, _traffic, make_state, port_stats_of  # noqa: E402
from tests.test_gpu_tx_complete_rings import LoopState  # noqa: E402

SIZE, MAX_BATCH, OPTS, N_PORTS, STACK_SIZE = 64, 48, 0x17, 3, 16
EMPTY, FULL = 2, 4  # the replay that meets an empty RX ring, and the one that meets a full stack ring
OFFERS = [40, 48, 0, 55, 33, 41]  # frames the peer puts on the RX ring before each replay (55 > max_batch: 7 stay)
BOUNDS = [SS.ALL_BOUND, SS.ALL_BOUND & ~2, SS.ALL_BOUND, SS.ALL_BOUND & ~4, SS.ALL_BOUND, 1]


def census(rx, fill, txs, stack, comps, pool) -> Counter:
    """The multiset of chunk addresses the containers hold: every ring's unconsumed entries, the pool below its count."""
    c = Counter()
    for r in (rx, fill, *txs, stack, *comps):
        for j in range(r.used()):
            e = r.entries[r.slot(r.cons + j)]
            c[int(e["addr"]) if r.entries.dtype.names else int(e)] += 1
    c.update(int(a) for a in pool.addr[:pool.n()])
    return c


def transmit(dev, d_src, s_src, d_comp, s_comp):
    """A peer on the device: every entry of a descriptor ring onto a completion ring (the addresses), both rings' words
    advanced; the mirrors follow.  Returns the count."""
    n = s_src.used()
    if n == 0:
        return 0
    src = [s_src.slot(s_src.cons + j) for j in range(n)]
    dst = [s_comp.slot(s_comp.prod + j) for j in range(n)]
    assert s_comp.free() >= n
    d_comp.ent.data.view(torch.int64)[torch.tensor(dst, device=dev)] = \
        d_src.ent.data.view(torch.int64).view(-1, 2)[torch.tensor(src, device=dev), 0]
    s_comp.entries[dst] = s_src.entries["addr"][src]
    s_comp.prod = (s_comp.prod + n) & RS.M32
    s_src.cons = (s_src.cons + n) & RS.M32
    d_comp.words.put(np.array([s_comp.prod, s_comp.cons], np.uint32))
    d_src.words.put(np.array([s_src.prod, s_src.cons], np.uint32))
    return n


def test_one_capture_of_the_loop_call_replayed_six_times_with_the_loop_closed():
    dev = _dev()
    umem, descs = _traffic(sum(OFFERS))
    table = _table(sum(OFFERS), OPTS, N_PORTS, entries=94)
    rx, fill, txs, pool = make_state(N_PORTS, SIZE, WRAP - 20, descs[:0], SIZE // 2, SIZE, 8 * SIZE, [4096] * N_PORTS)
    stack = make_stack(STACK_SIZE, 0xFFFFFFF5, STACK_SIZE)
    # (a port's socket completes a handful of replies over the run, the stack's consumer three rings full: the words
    # start that far below 2^32)
    comps = [RS.RingState(np.arange(SIZE, dtype=np.uint64) + np.uint64((q + 1) << 50), start, start)
             for q, start in enumerate([WRAP] * N_PORTS + [0xFFFFFFE0])]
    d = LoopState(rx, fill, txs, stack, pool, MAX_BATCH, comps, table, SS.ALL_BOUND)
    d_umem = to_dev(umem)

    def body():
        d.loop(d_umem, OPTS, SS.PASS, SIZE)

    # outside the capture first: the library's kernels are loaded, the device is known (empty rings: nothing changes)
    body()
    torch.cuda.synchronize()
    d.check(rx, fill, txs, pool, stack)
    d.check_comps(comps)
    d.stats.zero_()
    d.port_stats.data.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    s_rx, s_fill, s_txs, s_pool, s_stack = rx.copy(), fill.copy(), [t.copy() for t in txs], pool.copy(), stack.copy()
    s_comps = [c.copy() for c in comps]
    u = umem.copy()
    st = dict.fromkeys(IS.KEYS, 0)
    pst = [dict.fromkeys(EP.STATS_KEYS, 0) for _ in txs]
    taken = passed = completed = sent = 0
    for k, offer in enumerate(OFFERS):
        # the peers.  Every port's socket transmits its TX ring; the stack's consumer finishes with the stack ring's
        # frames (not before the replay that is to meet the ring full)
        for p in range(N_PORTS):
            sent += transmit(dev, d.txs[p], s_txs[p], d.comps[p], s_comps[p])
        if k == FULL:
            assert s_stack.free() == 0  # the replay before it left the ring full
        else:
            transmit(dev, d.stack, s_stack, d.comps[N_PORTS], s_comps[N_PORTS])
        # the wire: new RX entries, fill entries taken
        s_rx.produce(descs[taken:taken + offer])
        taken += offer
        assert s_rx.used() <= SIZE
        s_fill.cons = (s_fill.cons + min(s_fill.used(), 30)) & RS.M32
        d.rx.write(s_rx)
        d.fill.write(s_fill)
        d.bound.copy_(torch.from_numpy(np.array([BOUNDS[k]], np.uint64).view(np.int64)))
        torch.cuda.synchronize()
        before = census(d.rx.read(), d.fill.read(), [t.read() for t in d.txs], d.stack.read(),
                        [c.read() for c in d.comps], d.pool.read())
        assert before == census(s_rx, s_fill, s_txs, s_stack, s_comps, s_pool)
        avail, q_room, comp_used = s_rx.used(), s_stack.free(), [c.used() for c in s_comps]
        # the spec: the step, then every completion ring
        got = PS.spec_step_pass(u, s_rx, s_fill, s_txs, s_stack, s_pool, MAX_BATCH, OPTS, table, SS.PASS, BOUNDS[k], st, pst)
        moved, pushed = CS.spec_complete_rings(s_comps, s_pool, SIZE)
        res = got["result"]
        graph.replay()
        torch.cuda.synchronize()
        d.check(s_rx, s_fill, s_txs, s_pool, s_stack)
        d.check_comps(s_comps)
        d.check_outputs(got)
        assert [int(x) for x in d.moved.get(np.uint32)] == moved == comp_used, k
        assert int(d.pushed.get(np.uint32)[0]) == pushed == sum(moved), k  # the pool had room: nothing was dropped
        assert d.result() == res and stats_of(d.stats) == st and port_stats_of(d.port_stats, N_PORTS) == pst, k
        # conservation: the replay only moves chunks among the containers
        after = census(d.rx.read(), d.fill.read(), [t.read() for t in d.txs], d.stack.read(),
                       [c.read() for c in d.comps], d.pool.read())
        assert after == before and sum(after.values()) == sum(before.values()), k
        assert all(c.used() == 0 for c in s_comps)
        q = int((got["actions"][:res["received"]] == SS.XDP_PASS).sum())
        assert res["received"] == min(avail, MAX_BATCH) and res["passed"] == min(q, q_room)
        assert res["pass_full"] == q - res["passed"]
        if k == EMPTY:
            assert res == dict.fromkeys(PS.RESULT_KEYS, 0) and sum(moved) >= 4  # completion is served all the same
        elif k == FULL:
            assert q >= 4 and res["passed"] == 0 and res["pass_full"] == q
        else:
            assert res["passed"] >= 4
        passed += res["passed"]
        completed += sum(moved)
    assert passed > 2 * STACK_SIZE and s_stack.prod < 0x1000  # around the stack ring, past 2^32
    assert sent >= 3 * N_PORTS and completed >= sent + STACK_SIZE  # every port's TX chunks and the stack's came back
    assert all(c.prod < 0x1000 for c in s_comps) and s_pool.n() < s_pool.capacity
    assert (d_umem.cpu().numpy() == u).all()
