"""xsk_gpu_rx_pass_step_dev, xsk_gpu_neigh_serve_dev and xsk_gpu_unreach_serve_dev captured once in one graph on one stream
and replayed four times: the chain of consumers on the device.  The step puts what the filter passes on the stack ring,
the neighbour responder answers the requests among it and hands the rest to `up`, the port-unreachable responder answers
the UDP probes among that and hands the rest to `rest`.  Nothing is frozen into the capture but pointers and sizes: every
index word and the budget word are device memory that the replay reads when it executes.  The budget is never refilled,
so the fourth replay runs with it spent and its probes go on as LIMITED.  After each replay the spec's composition
(tests/rx_pass_spec.py, tests/neigh_spec.py, tests/unreach_spec.py) is held against every ring, every index word, the
budget, the results, the counters and the whole UMEM.  One linear chain: no parallel branches."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import egress_ports_spec as EP  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests import neigh_frames as NF  # noqa: E402
from tests import neigh_spec as NS  # noqa: E402
from tests import rx_dev_spec as RS  # noqa: E402
from tests import rx_pass_spec as PS  # noqa: E402
from tests import steer_spec as SS  # noqa: E402
from tests import unreach_frames as UF  # noqa: E402
from tests import unreach_spec as US  # noqa: E402
from tests.test_gpu_ingress import _dev, stats_of  # noqa: E402
from tests.test_gpu_neigh import dev_table, dev_word  # noqa: E402
from tests.test_gpu_neigh_graph import (MAX_BATCH, N_PORTS, OPTS, OWN4, OWN6, SIZE, STACK_SIZE, STEER, UP_SIZE, echo4, echo6,  # noqa: E402
                                        hip_runtime, node_kinds, place)
from tests.test_gpu_neigh_serve import ring  # noqa: E402
from tests.test_gpu_rx_pass_step_dev import PassState, make_stack  # noqa: E402
from tests.test_gpu_rx_step_dev import WRAP, DevRing, Guarded  # noqa: E402
from tests.test_gpu_rx_step_steer_dev import make_state, port_stats_of  # noqa: E402
from tests.test_gpu_unreach import dev_open  # noqa: E402

G, GN = UF.G, NF.G
REST_SIZE, BUDGET, CHUNK = 32, 7, 2048


def offers():
    """Four RX offers: requests for the neighbour responder, probes for the port-unreachable responder (closed and open
    ports, a stranger, one behind a tag), echo requests for the step, TCP for nobody."""
    arp, ns, tcp = GN.arp_case(tpa_entry=OWN4)[0](()), GN.ns_case(target_entry=OWN6)[0](()), GN.tcp4(())
    p4, p6 = G.udp4_case(entry=OWN4)[0](()), G.udp6_case(entry=OWN6, data=33)[0](())
    p4_opts, p6_long = G.udp4_case(entry=OWN4, ihl=15, data=1)[0](()), G.udp6_case(entry=OWN6, data=1185)[0](())
    tagged = G.udp6_case(entry=OWN6, data=0)[0](G.TAGS[1])
    listened, stranger = G.udp4_case(entry=OWN4, dport=53)[0](()), G.udp4_case(dst=G.STRANGER4)[0](())
    return [[arp, p4, ns, tcp, p6],
            [echo4(1), p6_long, listened, arp, p4_opts, stranger, echo6(1)],
            [tagged, ns, p4, tcp, p6, echo4(2)],
            [p4, arp, p6_long, listened, p6, echo6(2), tagged]]


def test_one_capture_of_the_three_calls_replayed_four_times_the_last_with_the_budget_spent():
    dev = _dev()
    batches = offers()
    umem, descs = place([f for b in batches for f in b])
    table = NF.table([OWN4, OWN6])
    rx, fill, txs, pool = make_state(N_PORTS, SIZE, WRAP - 9, descs[:0], SIZE // 2, SIZE, 8 * SIZE, [4096] * N_PORTS)
    stack = make_stack(STACK_SIZE, 0xFFFFFFFA, STACK_SIZE)
    up, rest = ring(UP_SIZE, 0xFFFFFFFA, 0, seed=3), ring(REST_SIZE, 0xFFFFFFF9, 0, seed=4)
    d = PassState(rx, fill, txs, stack, pool, MAX_BATCH, STEER, SS.ALL_BOUND)
    d_up, d_rest, d_tab = DevRing(up), DevRing(rest), dev_table(table)
    d_nres, d_nstats = Guarded(32), Guarded(32, np.zeros(32, np.uint8))
    d_ures, d_ustats = Guarded(32), Guarded(64, np.zeros(64, np.uint8))
    d_open, d_budget = dev_open(UF.OPEN), dev_word(BUDGET, np.uint32)
    d_umem = Guarded(umem.nbytes, umem)

    def step():
        d.step(d_umem.data, OPTS, SS.PASS)

    def neigh():
        X.neigh_serve_dev(d_umem.data, d.stack.view, d.views, d_up.view, STACK_SIZE, d_tab[0].data, d_tab[1],
                          bound=d.bound, nstats=d_nstats.data, res=d_nres.data, opts=OPTS)

    def unreach():
        X.unreach_serve_dev(d_umem.data, d_up.view, d.views, d_rest.view, UP_SIZE, d_tab[0].data, d_tab[1], CHUNK,
                            bound=d.bound, open_ports=d_open.data, budget=d_budget.data, ustats=d_ustats.data,
                            res=d_ures.data, opts=OPTS)

    def two():
        step()
        neigh()

    def three():
        two()
        unreach()

    # outside the capture first: the library's kernels are loaded (empty rings: nothing changes)
    three()
    torch.cuda.synchronize()
    d.check(rx, fill, txs, pool, stack)
    assert int(d_budget.get(np.uint32)[0]) == BUDGET
    d.stats.zero_()
    d.port_stats.data.zero_()
    # the third call adds exactly one node to the capture, a kernel node
    hip, side = hip_runtime(), torch.cuda.Stream(device=dev)
    pair, triple = node_kinds(hip, side, two), node_kinds(hip, side, three)
    assert len(triple) == len(pair) + 1 and triple.count(0) == pair.count(0) + 1  # 0: hipGraphNodeTypeKernel
    torch.cuda.synchronize()
    d.check(rx, fill, txs, pool, stack)  # a capture executes nothing

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        three()
    s_rx, s_fill, s_txs, s_pool, s_stack, s_up, s_rest = rx.copy(), fill.copy(), [t.copy() for t in txs], pool.copy(), \
        stack.copy(), up.copy(), rest.copy()
    u = umem.copy()
    st = dict.fromkeys(IS.KEYS, 0)
    pst = [dict.fromkeys(EP.STATS_KEYS, 0) for _ in txs]
    nst, ust = dict.fromkeys(NS.STATS_KEYS, 0), dict.fromkeys(US.STATS_KEYS, 0)
    taken, left = 0, BUDGET
    seen = set()
    for k, offer in enumerate(batches):
        # the peers: new RX entries; the TX rings transmitted, the rest ring and some fill entries taken
        s_rx.produce(descs[taken:taken + len(offer)])
        taken += len(offer)
        for t in s_txs:
            t.cons = t.prod
        s_rest.cons = s_rest.prod
        s_fill.cons = (s_fill.cons + min(s_fill.used(), 30)) & RS.M32
        d.rx.write(s_rx)
        d.fill.write(s_fill)
        d_rest.write(s_rest)
        for t, dt in zip(s_txs, d.txs):
            dt.write(t)
        torch.cuda.synchronize()
        # the spec's composition
        got = PS.spec_step_pass(u, s_rx, s_fill, s_txs, s_stack, s_pool, MAX_BATCH, OPTS, STEER, SS.PASS, SS.ALL_BOUND, st,
                                pst)
        nres = NS.spec_serve(u, s_stack, s_txs, s_up, STACK_SIZE, OPTS, table, NS.ALL_BOUND, nst)
        verdicts = []
        ures, left = US.spec_serve(u, s_up, s_txs, s_rest, UP_SIZE, OPTS, table, US.ALL_BOUND, UF.OPEN, CHUNK, left, ust,
                                   verdicts)
        graph.replay()
        torch.cuda.synchronize()
        d.check(s_rx, s_fill, s_txs, s_pool, s_stack)
        for dr, want in ((d_up, s_up), (d_rest, s_rest)):
            g = dr.read()
            assert (g.prod, g.cons) == (want.prod, want.cons) and (g.entries == want.entries).all(), k
            assert dr.words.intact() and dr.ent.intact()
        for g in (d_nres, d_nstats, d_ures, d_ustats, d_open, d_budget, d_umem):
            assert g.intact()
        d.check_outputs(got)
        assert d.result() == got["result"] and stats_of(d.stats) == st and port_stats_of(d.port_stats, N_PORTS) == pst, k
        r = d_nres.get(X.NEIGH_RESULT_DTYPE)[0]
        assert {key: int(r[key]) for key in NS.RESULT_KEYS} == nres, k
        s = d_nstats.get(X.NEIGH_STATS_DTYPE)[0]
        assert {key: int(s[key]) for key in NS.STATS_KEYS} == nst, k
        r = d_ures.get(X.UNREACH_RESULT_DTYPE)[0]
        assert {key: int(r[key]) for key in US.RESULT_KEYS} == ures and not r["reserved"].any(), k
        s = d_ustats.get(X.UNREACH_STATS_DTYPE)[0]
        assert {key: int(s[key]) for key in US.STATS_KEYS} == ust, k
        assert int(d_budget.get(np.uint32)[0]) == left, k
        assert (d_umem.get() == u).all(), k
        # what this replay was about: everything the neighbour responder passed on was served in the same replay
        assert ures["consumed"] == nres["up"] and ures["backlog"] == 0 and s_up.used() == 0 and s_stack.used() == 0
        if k < 3:
            assert ures["unreach4"] >= 1 and ures["unreach6"] >= 1 and ures["limited"] == 0 and left == (5, 3, 0)[k]
        else:  # the budget is spent: nothing is rewritten, every probe that was due goes on
            assert ures["unreach4"] + ures["unreach6"] == 0 and ures["limited"] == 4 and ures["rest"] == ures["consumed"]
        seen |= set(verdicts)
    assert seen >= {US.NONE, US.UNREACH4, US.UNREACH6, US.UNKNOWN, US.LEFT, US.LIMITED}
    assert s_up.prod < 0x100 and s_rest.prod < 0x100  # around 2^32
    assert ust["limited"] == 4 and ust["unreach4"] + ust["unreach6"] == BUDGET
