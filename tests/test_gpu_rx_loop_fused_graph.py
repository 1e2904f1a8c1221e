"""xsk_gpu_rx_fused_loop_dev captured once and replayed: the scenario of tests/test_gpu_rx_loop_dev_graph.py with the
fused call in the loop call's place.  A whole RX loop iteration over all sockets -- receive, refill, steer, reply,
per-port TX, stack ring, and every completion ring back into the pool -- is ONE kernel node; nothing is frozen into the
capture but pointers, sizes and the bounds, and every index, count and the bound mask is device memory that the replay
reads when it executes.  Between replays the test plays the peers on the device (that file's census() and transmit()).
One replay meets an empty RX ring (the completion rings are served all the same), one a full stack ring.  After every
replay the state is the spec's, and the multiset of chunk addresses over the RX, fill, TX, stack and completion rings and
the pool is what it was before it.  The capture holds one kernel node per replay: a linear chain, no parallel
branches."""
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
from tests.test_gpu_rx_loop_dev_graph import BOUNDS, EMPTY, FULL, MAX_BATCH, N_PORTS, OFFERS, OPTS, SIZE, STACK_SIZE  # noqa: E402
from tests.test_gpu_rx_loop_dev_graph import census, transmit  # noqa: E402
from tests.test_gpu_rx_loop_fused import FusedState  # noqa: E402


def test_one_capture_of_the_fused_call_replayed_six_times_with_the_loop_closed():
    dev = _dev()
    umem, descs = _traffic(sum(OFFERS))
    table = _table(sum(OFFERS), OPTS, N_PORTS, entries=94)
    rx, fill, txs, pool = make_state(N_PORTS, SIZE, WRAP - 20, descs[:0], SIZE // 2, SIZE, 8 * SIZE, [4096] * N_PORTS)
    stack = make_stack(STACK_SIZE, 0xFFFFFFF5, STACK_SIZE)
    # (a port's socket completes a handful of replies over the run, the stack's consumer three rings full: the words
    # start that far below 2^32)
    comps = [RS.RingState(np.arange(SIZE, dtype=np.uint64) + np.uint64((q + 1) << 50), start, start)
             for q, start in enumerate([WRAP] * N_PORTS + [0xFFFFFFE0])]
    d = FusedState(rx, fill, txs, stack, pool, MAX_BATCH, comps, table, SS.ALL_BOUND)
    d_umem = to_dev(umem)

    def body():
        d.run(True, d_umem, OPTS, SS.PASS, SIZE)

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


def test_the_capture_holds_one_kernel_node():
    """The fused call captured through the HIP runtime itself: the graph has exactly one node and it is a kernel node,
    for each of the three instances and with completion rings or without -- a linear chain with no parallel branches,
    no memset and no copy node (complete_max == 0 included: the kernel stores the zeros itself)."""
    import ctypes as C
    dev = _dev()
    # the HIP runtime this process already runs on (the one torch and the library loaded), not a second copy
    loaded = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert len(loaded) == 1, loaded
    hip = C.CDLL(loaded[0])
    umem, descs = _traffic(40)
    d_umem = to_dev(umem)
    for opts, complete_max, with_comps in ((0, 64, True), (0x7, 0, True), (0x17, 64, True), (0x17, 64, False)):
        table = _table(40, opts, N_PORTS, entries=22)
        rx, fill, txs, pool = make_state(N_PORTS, SIZE, WRAP, descs[:0], SIZE // 2, SIZE, 8 * SIZE, [4096] * N_PORTS)
        stack = make_stack(STACK_SIZE, 0xFFFFFFF5, STACK_SIZE)
        comps = [RS.RingState(np.arange(SIZE, dtype=np.uint64) + np.uint64((q + 1) << 50), WRAP, WRAP)
                 for q in range(N_PORTS + 1)]
        d = FusedState(rx, fill, txs, stack, pool, MAX_BATCH, comps, table, SS.ALL_BOUND)
        d.run(True, d_umem, opts, SS.PASS, complete_max, comps=with_comps)  # the kernel is loaded outside the capture
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device=dev)
        graph = C.c_void_p()
        with torch.cuda.stream(stream):
            assert hip.hipStreamBeginCapture(C.c_void_p(stream.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
            try:
                d.run(True, d_umem, opts, SS.PASS, complete_max, comps=with_comps)
            finally:
                rc = hip.hipStreamEndCapture(C.c_void_p(stream.cuda_stream), C.byref(graph))
        assert rc == 0 and graph.value
        n = C.c_size_t(0)
        assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value == 1, (opts, n.value)
        node, kind = (C.c_void_p * 1)(), C.c_int(-1)
        assert hip.hipGraphGetNodes(graph, node, C.byref(n)) == 0
        assert hip.hipGraphNodeGetType(C.c_void_p(node[0]), C.byref(kind)) == 0 and kind.value == 0  # hipGraphNodeTypeKernel
        assert hip.hipGraphDestroy(graph) == 0
        torch.cuda.synchronize()
        d.check(rx, fill, txs, pool, stack)  # empty rings: nothing changed, in or out of the capture
