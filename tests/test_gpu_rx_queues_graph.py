"""xsk_gpu_rx_queues_dev captured once and replayed: the scenario of tests/test_gpu_rx_loop_fused_graph.py with three
queues in one call.  A whole RX loop iteration over all sockets of all three queues is ONE kernel node; nothing is
frozen into the capture but the block's address, the queue count and the options, and the block holds nothing but
pointers, sizes and bounds: every index, count and bound mask is device memory that the replay reads when it executes.
Between replays the test plays every queue's peers on the device (census() and transmit() of
tests/test_gpu_rx_loop_dev_graph.py), with offers that differ from queue to queue.  After every replay every queue's
state is the spec's stepped the same number of times, and its multiset of chunk addresses is what it was before."""
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
from tests import tx_complete_rings_spec as CS  # noqa: E402
from tests.test_gpu_ingress import _dev, stats_of, to_dev  # noqa: E402
from tests.test_gpu_rx_loop_dev_graph import BOUNDS, MAX_BATCH, N_PORTS, OFFERS, OPTS, SIZE, STACK_SIZE  # noqa: E402
from tests.test_gpu_rx_loop_dev_graph import census, transmit  # noqa: E402
from tests.test_gpu_rx_loop_fused import FusedState  # noqa: E402
from tests.test_gpu_rx_pass_step_dev import make_stack  # noqa: E402
from tests.test_gpu_rx_queues import Queue  # noqa: E402
from tests.test_gpu_rx_step_dev import WRAP  # noqa: E402
from tests.test_gpu_rx_step_steer_dev import _table, _traffic, make_state, port_stats_of  # noqa: E402

N_QUEUES = 3


def _offers(k):
    """Queue k's offers: the scenario's, rotated, so that the empty RX ring meets another replay in every queue."""
    return OFFERS[k:] + OFFERS[:k]


class Mirror:
    """One queue: the device state, the host mirrors the spec steps, and the traffic it is fed from."""

    def __init__(self, k):
        self.k, self.offers = k, _offers(k)
        total = sum(OFFERS)
        self.umem, self.descs = _traffic(total, seed=k)
        self.table = _table(total, OPTS, N_PORTS, seed=k, entries=94)
        self.rx, self.fill, self.txs, self.pool = make_state(N_PORTS, SIZE, WRAP - 20 - k, self.descs[:0], SIZE // 2, SIZE,
                                                             8 * SIZE, [4096] * N_PORTS)
        self.stack = make_stack(STACK_SIZE, 0xFFFFFFF5, STACK_SIZE, seed=k)
        self.comps = [RS.RingState(np.arange(SIZE, dtype=np.uint64) + np.uint64((q + 1) << 50), start, start)
                      for q, start in enumerate([WRAP] * N_PORTS + [0xFFFFFFE0])]
        self.d = FusedState(self.rx, self.fill, self.txs, self.stack, self.pool, MAX_BATCH, self.comps, self.table,
                            SS.ALL_BOUND)
        self.d_umem = to_dev(self.umem)
        self.q = Queue(self.umem, self.table, self.rx, self.fill, self.txs, self.pool, self.stack, self.comps, MAX_BATCH,
                       SS.PASS, SS.ALL_BOUND, SIZE)
        self.s = (self.rx.copy(), self.fill.copy(), [t.copy() for t in self.txs], self.pool.copy(), self.stack.copy(),
                  [c.copy() for c in self.comps])
        self.u = self.umem.copy()
        self.st = dict.fromkeys(IS.KEYS, 0)
        self.pst = [dict.fromkeys(EP.STATS_KEYS, 0) for _ in self.txs]
        self.taken = 0

    def census(self, host):
        if host:
            s_rx, s_fill, s_txs, s_pool, s_stack, s_comps = self.s
            return census(s_rx, s_fill, s_txs, s_stack, s_comps, s_pool)
        d = self.d
        return census(d.rx.read(), d.fill.read(), [t.read() for t in d.txs], d.stack.read(), [c.read() for c in d.comps],
                      d.pool.read())

    def peers(self, dev, k):
        """Before replay k: every port's socket transmits, the stack's consumer drains the stack ring, new RX entries
        arrive, fill entries are taken, the bound mask is rewritten."""
        s_rx, s_fill, s_txs, s_pool, s_stack, s_comps = self.s
        d = self.d
        for p in range(N_PORTS):
            transmit(dev, d.txs[p], s_txs[p], d.comps[p], s_comps[p])
        transmit(dev, d.stack, s_stack, d.comps[N_PORTS], s_comps[N_PORTS])
        offer = self.offers[k]
        s_rx.produce(self.descs[self.taken:self.taken + offer])
        self.taken += offer
        assert s_rx.used() <= SIZE
        s_fill.cons = (s_fill.cons + min(s_fill.used(), 30)) & RS.M32
        d.rx.write(s_rx)
        d.fill.write(s_fill)
        self.bound = BOUNDS[(k + self.k) % len(BOUNDS)]
        d.bound.copy_(torch.from_numpy(np.array([self.bound], np.uint64).view(np.int64)))

    def step_spec(self):
        s_rx, s_fill, s_txs, s_pool, s_stack, s_comps = self.s
        avail = s_rx.used()
        got = PS.spec_step_pass(self.u, s_rx, s_fill, s_txs, s_stack, s_pool, MAX_BATCH, OPTS, self.table, SS.PASS,
                                self.bound, self.st, self.pst)
        moved, pushed = CS.spec_complete_rings(s_comps, s_pool, SIZE)
        assert got["result"]["received"] == min(avail, MAX_BATCH)
        return got, moved, pushed

    def check(self, got, moved, pushed):
        s_rx, s_fill, s_txs, s_pool, s_stack, s_comps = self.s
        d = self.d
        d.check(s_rx, s_fill, s_txs, s_pool, s_stack)
        d.check_comps(s_comps)
        d.check_outputs(got)
        assert [int(x) for x in d.moved.get(np.uint32)] == moved and int(d.pushed.get(np.uint32)[0]) == pushed
        assert d.result() == got["result"] and stats_of(d.stats) == self.st
        assert port_stats_of(d.port_stats, N_PORTS) == self.pst


def _block(mirrors):
    host = X.rx_queues_prepare([m.q.record(m.d, m.d_umem) for m in mirrors], OPTS)
    return to_dev(host)


def test_one_capture_of_three_queues_replayed_six_times_with_the_loop_closed():
    dev = _dev()
    mirrors = [Mirror(k) for k in range(N_QUEUES)]
    d_block = _block(mirrors)

    def body():
        X.rx_queues_dev(d_block, N_QUEUES, OPTS)

    # outside the capture first: the library's kernels are loaded, the device is known (empty rings: nothing changes)
    body()
    torch.cuda.synchronize()
    for m in mirrors:
        m.d.check(m.rx, m.fill, m.txs, m.pool, m.stack)
        m.d.check_comps(m.comps)
        m.d.stats.zero_()
        m.d.port_stats.data.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    empties = 0
    for k in range(len(OFFERS)):
        for m in mirrors:
            m.peers(dev, k)
        torch.cuda.synchronize()
        before = [m.census(False) for m in mirrors]
        assert before == [m.census(True) for m in mirrors]
        want = [m.step_spec() for m in mirrors]
        graph.replay()
        torch.cuda.synchronize()
        for m, w, was in zip(mirrors, want, before):
            m.check(*w)
            after = m.census(False)  # conservation: the replay only moves chunks among the queue's containers
            assert after == was and sum(after.values()) == sum(was.values()), (k, m.k)
            if w[0]["result"]["received"] == 0:  # the completion rings are served all the same
                assert w[0]["result"] == dict.fromkeys(PS.RESULT_KEYS, 0) and k == (2 - m.k) % len(OFFERS)
                empties += 1
    assert empties == N_QUEUES  # every queue met its empty RX ring, each at another replay
    for m in mirrors:
        assert (m.d_umem.cpu().numpy() == m.u).all() and m.taken == sum(OFFERS)
        assert m.st["rx_packets"] > 0 and m.st["tx_packets"] > 0
    assert len({tuple(sorted(m.st.items())) for m in mirrors}) == N_QUEUES  # three different histories


def test_the_capture_holds_one_kernel_node():
    """The call captured through the HIP runtime itself: the graph has exactly one node and it is a kernel node, for each
    of the three instances -- no memset, no copy, no parallel branches."""
    import ctypes as C
    dev = _dev()
    loaded = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert len(loaded) == 1, loaded
    hip = C.CDLL(loaded[0])
    mirrors = [Mirror(k) for k in range(N_QUEUES)]
    for opts in (0, 0x7, 0x17):
        host = X.rx_queues_prepare([m.q.record(m.d, m.d_umem) for m in mirrors], opts)
        d_block = to_dev(host)
        X.rx_queues_dev(d_block, N_QUEUES, opts)  # the kernel is loaded outside the capture
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device=dev)
        graph = C.c_void_p()
        with torch.cuda.stream(stream):
            assert hip.hipStreamBeginCapture(C.c_void_p(stream.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
            try:
                X.rx_queues_dev(d_block, N_QUEUES, opts)
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
        for m in mirrors:
            m.d.check(m.rx, m.fill, m.txs, m.pool, m.stack)  # empty rings: nothing changed, in or out of the capture
