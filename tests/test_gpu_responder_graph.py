"""xsk_gpu_responder_dev and xsk_gpu_responder_queues_dev under graph capture: each call is ONE kernel
node, and one capture is replayed four times with the host rewriting the RX ring in between -- replay 1 offers a who-has
and a solicitation, and both replies are on the TX rings after that same replay; replays 2 and 3 offer echo requests to
the resolved addresses; replay 4 offers nothing.  Nothing is frozen into the capture but pointers, sizes and bounds:
every index word is device memory read when the replay executes.  Every replay is compared with the spec
(loop_world.spec_round through Leg.hold), exactly."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import loop_world as LW  # noqa: E402
from tests.responder_dev import RLeg, echo4, hand_world, problems, responder_block, solicit, who_has  # noqa: E402
from tests.test_gpu_ingress import _dev  # noqa: E402

OPTS = 0x17


def scenario(port):
    """(the world, the offers of the four replays as slices of w.later)."""
    later = [who_has(port), solicit(port)] + [echo4(port, s) for s in range(1, 6)] + [echo4(port, 9), echo4((port + 1) % 8, 10)]
    w = hand_world([], later=later, n_comp=4)
    return w, [w.later[0:2], w.later[2:7], w.later[7:9], w.later[0:0]]


def replays(worlds, offers, legs, body):
    """Round 0 outside the capture (the kernels are loaded; empty rings), the capture, then the four replays."""
    def run(k, launch):
        rounds = [LW.spec_round(w) for w in worlds]
        launch()
        torch.cuda.synchronize()
        wrong = []
        for q, (leg, r) in enumerate(zip(legs, rounds)):
            wrong += problems(f"queue {q}", leg.hold, r)
        assert not wrong, f"replay {k}: " + " | ".join(wrong)
        return rounds

    run(0, body)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    torch.cuda.synchronize()
    tx_before = [[t.copy() for t in w.txs] for w in worlds]
    out = []
    for k in range(4):
        for w, leg, offer in zip(worlds, legs, offers):
            w.rx.produce(offer[k])
            leg.follow([w.rx])
        out.append(run(k + 1, graph.replay))
    return out, tx_before


def check_story(w, rounds, tx_before, port):
    first, second, third, last = rounds
    assert first["got"]["result"]["received"] == 2 and first["got"]["result"]["passed"] == 2
    assert first["nres"] == dict(consumed=2, arp_replies=1, na_replies=1, up=0, backlog=0)  # in that same replay
    assert second["got"]["result"]["replied"] == 5 and third["got"]["result"]["replied"] == 2
    assert last["got"]["result"]["received"] == 0 and last["nres"]["consumed"] == 0
    assert ((w.txs[port].prod - tx_before[port].prod) & 0xFFFFFFFF) == 2 + 5 + 1


def test_one_capture_of_the_one_queue_call_replayed_four_times():
    _dev()
    w, offers = scenario(2)
    leg = RLeg(w)
    rec = leg.responder_record()
    rounds, tx_before = replays([w], [offers], [leg], lambda: X.responder_dev(rec, OPTS))
    check_story(w, [r[0] for r in rounds], tx_before[0], 2)


def test_one_capture_of_the_queues_call_replayed_four_times():
    _dev()
    (wa, oa), (wb, ob) = scenario(1), scenario(6)
    ob = [ob[3], ob[0], ob[1], ob[2]]  # the second queue's story starts a replay later: its idle replay is the first
    legs = [RLeg(wa), RLeg(wb)]
    d_block = responder_block(legs, OPTS)
    rounds, tx_before = replays([wa, wb], [oa, ob], legs, lambda: X.responder_queues_dev(d_block, 2, OPTS))
    check_story(wa, [r[0] for r in rounds], tx_before[0], 1)
    b = [r[1] for r in rounds]
    check_story(wb, [b[1], b[2], b[3], b[0]], tx_before[1], 6)


def test_each_call_is_one_kernel_node():
    """Captured through the HIP runtime itself: the graph has exactly one node and it is a kernel node, for each of the
    three instances of both kernels -- no memset, no copy, no second kernel.  (Empty rings: a launch changes nothing the
    spec's round does not change too.)"""
    dev = _dev()
    loaded = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert len(loaded) == 1, loaded
    hip = C.CDLL(loaded[0])
    for opts in (0, 0x7, 0x17):
        worlds = [hand_world([], opts=opts, n_comp=4), hand_world([], opts=opts)]
        legs = [RLeg(w) for w in worlds]
        rec = legs[0].responder_record()
        q_legs = [RLeg(w) for w in worlds]
        d_block = responder_block(q_legs, opts)
        calls = {"one queue": lambda: X.responder_dev(rec, opts),
                 "queues": lambda: X.responder_queues_dev(d_block, 2, opts)}
        for name, call in calls.items():
            call()  # the kernel is loaded outside the capture
            torch.cuda.synchronize()
            stream = torch.cuda.Stream(device=dev)
            graph = C.c_void_p()
            with torch.cuda.stream(stream):
                assert hip.hipStreamBeginCapture(C.c_void_p(stream.cuda_stream), 2) == 0  # hipStreamCaptureModeRelaxed
                try:
                    call()  # (on the current stream: the capturing one)
                finally:
                    rc = hip.hipStreamEndCapture(C.c_void_p(stream.cuda_stream), C.byref(graph))
            assert rc == 0 and graph.value
            n = C.c_size_t(0)
            assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0 and n.value == 1, (name, opts, n.value)
            node, kind = (C.c_void_p * 1)(), C.c_int(-1)
            assert hip.hipGraphGetNodes(graph, node, C.byref(n)) == 0
            assert hip.hipGraphNodeGetType(C.c_void_p(node[0]), C.byref(kind)) == 0 and kind.value == 0  # a kernel node
            assert hip.hipGraphDestroy(graph) == 0
            torch.cuda.synchronize()
