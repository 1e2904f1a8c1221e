"""xsk_gpu_rx_pass_step_dev followed by xsk_gpu_neigh_serve_dev, captured once in one graph on one stream and replayed
four times: "steer + echo + neighbour", the self-standing ping responder on the device.  A peer first asks who owns an
address (an ARP request, a neighbour solicitation), the responder's reply leaves on the owning port's TX ring, then the
peer's echo requests to the address just resolved are answered by the step; TCP and an ARP request for a stranger go up.
Nothing is frozen into the capture but pointers and sizes; every index word is device memory that the replay reads when
it executes.  After each replay the spec's composition (tests/rx_pass_spec.py, then tests/neigh_spec.py) is held against
every ring, every index word, the results, the counters and the whole UMEM.  One linear chain: no parallel branches."""
import ctypes as C

import numpy as np
import pytest

import oracle

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
from tests.test_gpu_ingress import _dev, stats_of, to_dev  # noqa: E402
from tests.test_gpu_neigh import dev_table  # noqa: E402
from tests.test_gpu_neigh_serve import ring  # noqa: E402
from tests.test_gpu_rx_pass_step_dev import PassState, make_stack  # noqa: E402
from tests.test_gpu_rx_step_dev import WRAP, DevRing, Guarded  # noqa: E402
from tests.test_gpu_rx_step_steer_dev import make_state, port_stats_of  # noqa: E402
from tests.v6_frames import G6  # noqa: E402

G = NF.G
SIZE, MAX_BATCH, OPTS, N_PORTS, STACK_SIZE, UP_SIZE, STRIDE = 64, 48, 0x17, 3, 16, 32, 2048
OWN4, OWN6 = (4, bytes([192, 0, 2, 1]), 1, bytes.fromhex("020000000a01")), \
    (6, bytes.fromhex("20010db80000000000000000000000fe"), 2, bytes.fromhex("0200000006fe"))
STEER = {(4, OWN4[1] + bytes(12)): 1, (6, OWN6[1]): 2}


def echo4(seq):
    return G6.W.build(saddr=G.PEER4, daddr=OWN4[1], src_mac=G.PEER_MAC, dst_mac=OWN4[3], seq=seq, payload=b"ping" * 5)


def echo6(seq):
    return G6.build6(saddr=G.PEER6, daddr=OWN6[1], src_mac=G.PEER_MAC, dst_mac=OWN6[3], seq=seq, payload=b"pong" * 3,
                     hlim=64)


def offers():
    """Four RX offers that differ: who-has and solicitation first, the echo requests to the resolved addresses behind
    them, TCP and a stranger's ARP request among them."""
    arp, ns = G.arp_case(tpa_entry=OWN4)[0](()), G.ns_case(target_entry=OWN6)[0](())
    stranger, tcp, dad = G.arp_case(tpa=G.STRANGER4)[0](()), G.tcp4(()), G.ns_case(src=bytes(16))[0](())
    tagged = G.ns_case(target_entry=OWN6, pad=6)[0](G.TAGS[1])
    return [[arp, ns, tcp, stranger],
            [echo4(1), echo6(1), arp, echo4(2), tcp, ns, stranger, echo6(2)],
            [tagged, dad, echo6(3), stranger, arp, arp, echo4(3), ns, tcp, tcp, ns],
            [ns, echo4(4), arp, echo6(4), stranger, tcp]]


def place(frames):
    """Frame i inside chunk i, at a small odd offset; sentinel bytes everywhere else."""
    umem = np.full(len(frames) * STRIDE, NF.SENTINEL, np.uint8)
    descs = np.zeros(len(frames), oracle.DESC_DTYPE)
    for i, f in enumerate(frames):
        a = i * STRIDE + 2 * (i % 7) + 1
        umem[a:a + len(f)] = np.frombuffer(f, np.uint8)
        descs[i] = (a, len(f), 0x3000 + i)
    return umem, descs


def hip_runtime():
    loaded = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert len(loaded) == 1, loaded
    return C.CDLL(loaded[0])


def node_kinds(hip, stream, fn):
    """The node types of what `fn` enqueues, captured through the HIP runtime itself."""
    graph = C.c_void_p()
    with torch.cuda.stream(stream):
        assert hip.hipStreamBeginCapture(C.c_void_p(stream.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
        try:
            fn()
        finally:
            rc = hip.hipStreamEndCapture(C.c_void_p(stream.cuda_stream), C.byref(graph))
    assert rc == 0 and graph.value
    n = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0
    nodes = (C.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(graph, nodes, C.byref(n)) == 0
    kinds = []
    for node in nodes:
        kind = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(kind)) == 0
        kinds.append(kind.value)
    assert hip.hipGraphDestroy(graph) == 0
    return kinds


def test_one_capture_of_the_pass_step_and_the_responder_replayed_four_times():
    dev = _dev()
    batches = offers()
    umem, descs = place([f for b in batches for f in b])
    neigh = NF.table([OWN4, OWN6])
    rx, fill, txs, pool = make_state(N_PORTS, SIZE, WRAP - 9, descs[:0], SIZE // 2, SIZE, 8 * SIZE, [4096] * N_PORTS)
    stack = make_stack(STACK_SIZE, 0xFFFFFFFA, STACK_SIZE)
    up = ring(UP_SIZE, 0xFFFFFFFA, 0, seed=3)
    d = PassState(rx, fill, txs, stack, pool, MAX_BATCH, STEER, SS.ALL_BOUND)
    d_up, d_tab = DevRing(up), dev_table(neigh)
    d_nres, d_nstats = Guarded(32), Guarded(32, np.zeros(32, np.uint8))
    d_umem = Guarded(umem.nbytes, umem)

    def step():
        d.step(d_umem.data, OPTS, SS.PASS)

    def serve():
        X.neigh_serve_dev(d_umem.data, d.stack.view, d.views, d_up.view, STACK_SIZE, d_tab[0].data, d_tab[1],
                          bound=d.bound, nstats=d_nstats.data, res=d_nres.data, opts=OPTS)

    def both():
        step()
        serve()

    # outside the capture first: the library's kernels are loaded (empty rings: nothing changes)
    both()
    torch.cuda.synchronize()
    d.check(rx, fill, txs, pool, stack)
    d.stats.zero_()
    d.port_stats.data.zero_()
    # the second call adds exactly one node to the capture, a kernel node
    hip, side = hip_runtime(), torch.cuda.Stream(device=dev)
    alone, pair = node_kinds(hip, side, step), node_kinds(hip, side, both)
    assert len(pair) == len(alone) + 1 and pair.count(0) == alone.count(0) + 1  # 0: hipGraphNodeTypeKernel
    torch.cuda.synchronize()
    d.check(rx, fill, txs, pool, stack)  # a capture executes nothing

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    s_rx, s_fill, s_txs, s_pool, s_stack, s_up = rx.copy(), fill.copy(), [t.copy() for t in txs], pool.copy(), \
        stack.copy(), up.copy()
    u = umem.copy()
    st = dict.fromkeys(IS.KEYS, 0)
    pst = [dict.fromkeys(EP.STATS_KEYS, 0) for _ in txs]
    nst = dict.fromkeys(NS.STATS_KEYS, 0)
    taken = 0
    seen = set()
    for k, offer in enumerate(batches):
        # the peers: new RX entries; the TX rings transmitted, the up ring and some fill entries taken
        s_rx.produce(descs[taken:taken + len(offer)])
        taken += len(offer)
        for t in s_txs:
            t.cons = t.prod
        s_up.cons = s_up.prod
        s_fill.cons = (s_fill.cons + min(s_fill.used(), 30)) & RS.M32
        d.rx.write(s_rx)
        d.fill.write(s_fill)
        d_up.write(s_up)
        for t, dt in zip(s_txs, d.txs):
            dt.write(t)
        torch.cuda.synchronize()
        # the spec's composition
        got = PS.spec_step_pass(u, s_rx, s_fill, s_txs, s_stack, s_pool, MAX_BATCH, OPTS, STEER, SS.PASS, SS.ALL_BOUND, st,
                                pst)
        passed = got["result"]["passed"]
        verdicts = []
        nres = NS.spec_serve(u, s_stack, s_txs, s_up, STACK_SIZE, OPTS, neigh, NS.ALL_BOUND, nst, verdicts)
        graph.replay()
        torch.cuda.synchronize()
        d.check(s_rx, s_fill, s_txs, s_pool, s_stack)
        g = d_up.read()
        assert (g.prod, g.cons) == (s_up.prod, s_up.cons) and (g.entries == s_up.entries).all()
        assert d_up.words.intact() and d_up.ent.intact() and d_nres.intact() and d_nstats.intact() and d_umem.intact()
        d.check_outputs(got)
        assert d.result() == got["result"] and stats_of(d.stats) == st and port_stats_of(d.port_stats, N_PORTS) == pst, k
        r = d_nres.get(X.NEIGH_RESULT_DTYPE)[0]
        assert {key: int(r[key]) for key in NS.RESULT_KEYS} == nres and not r["reserved"].any(), k
        s = d_nstats.get(X.NEIGH_STATS_DTYPE)[0]
        assert {key: int(s[key]) for key in NS.STATS_KEYS} == nst, k
        assert (d_umem.get() == u).all(), k
        # what this replay was about: everything the filter passed was served, the requests for our addresses answered
        assert nres["consumed"] == passed and nres["backlog"] == 0 and s_stack.used() == 0
        assert nres["arp_replies"] >= 1 and nres["na_replies"] >= 1 and nres["up"] >= 2
        assert got["result"]["replied"] == sum(f in (echo4(i), echo6(i)) for f in offer for i in range(1, 5))
        seen |= set(verdicts)
    assert seen >= {NS.NONE, NS.ARP_REPLY, NS.NA_REPLY, NS.UNKNOWN, NS.LEFT}
    assert s_stack.prod < 0x100 and s_up.prod < 0x100  # around 2^32
    assert nst["seen"] == sum(len(b) for b in batches) - 8  # every frame but the eight echo requests went through the ring
