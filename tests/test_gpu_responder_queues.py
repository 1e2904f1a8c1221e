"""GPU parity of xsk_gpu_responder_queues_dev: Q = 1, 2 and 5 queues in one launch against
xsk_gpu_responder_dev called queue after queue, both held against the spec (loop_world.spec_round) and against each
other byte for byte.  Two of the queues are worlds over one UMEM (loop_world.shared_pair), with rings, pools and tables
of their own; the loads are unequal -- one queue has nothing to do at all, one has 1024 frames.  A block that does not
match the call -- prepared for other options, for another queue count, or by xsk_gpu_rx_queues_prepare -- leaves every
byte of every buffer as it was, and so does this call's block handed to xsk_gpu_rx_queues_dev.  All comparisons exact."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import loop_world as LW  # noqa: E402
from tests import responder_seeds as SEEDS  # noqa: E402
from tests.responder_dev import (RLeg, echo4, hand_world, problems, responder_block, same_bytes, snapshot,  # noqa: E402
                                 solicit, stranger, who_has)
from tests.test_gpu_ingress import _dev, to_dev  # noqa: E402
from tests.test_gpu_rx_queues import block_of  # noqa: E402
from tests.test_gpu_rx_step_dev import Guarded  # noqa: E402

OPTS = 0x17


def mixed(n, shift=0):
    return [who_has((i + shift) % 8) if i % 8 == 3 else solicit((i + shift) % 8) if i % 8 == 6 else
            stranger() if i % 16 == 9 else echo4((i + shift) % 8, i) for i in range(n)]


def worlds_of(n_queues):
    """(worlds, which of them share the first one's UMEM).  Five: the shared pair after its first offer, a queue with
    nothing on any ring, a queue with 1024 frames, a queue with a backlog and a port without room."""
    pair = list(LW.shared_pair(*SEEDS.seeds(OPTS), OPTS))
    for w in pair:
        LW.peers(w, 0)
    rooms = [64] * 8
    rooms[3] = 6  # its five echo replies and one more entry
    rest = [hand_world([], n_comp=4),
            hand_world(mixed(1024), max_batch=1024, serve_max=1024, tx_size=256, stack_size=512, up_size=128, n_comp=4,
                       complete_max=1024),
            hand_world(mixed(40, 3), [who_has(3), stranger(), who_has(3)], rooms=rooms, serve_max=16)]
    if n_queues == 1:
        return rest[2:], 0
    if n_queues == 2:
        return pair, 2
    return pair + rest, 2


def upload(worlds, n_shared):
    shared = Guarded(worlds[0].umem.nbytes, worlds[0].umem) if n_shared else None
    return [RLeg(w, shared if q < n_shared else None) for q, w in enumerate(worlds)]


@pytest.mark.parametrize("n_queues", [1, 2, 5])
def test_queues_against_the_one_queue_call(n_queues):
    _dev()
    worlds, n_shared = worlds_of(n_queues)
    assert len(worlds) == n_queues and all(w.in_fused_bounds() for w in worlds)
    p_legs, q_legs = upload(worlds, n_shared), upload(worlds, n_shared)
    d_block = responder_block(q_legs, OPTS)
    rounds = [LW.spec_round(w) for w in worlds]  # (a shared UMEM takes both sharers' rounds before it is compared)
    for leg in p_legs:
        leg.responder()
    X.responder_queues_dev(d_block, n_queues, OPTS)
    torch.cuda.synchronize()
    wrong = []
    for q, r in enumerate(rounds):
        wrong += problems(f"queue {q} leg one-queue", p_legs[q].hold, r)
        wrong += problems(f"queue {q} leg queues", q_legs[q].hold, r)
        wrong += problems(f"queue {q} leg queues against leg one-queue", same_bytes, p_legs[q], q_legs[q])
    assert not wrong, " | ".join(wrong)
    if n_queues == 5:  # the loads were unequal, and the responder had work
        assert rounds[2]["got"]["result"]["received"] == 0 and rounds[2]["nres"]["consumed"] == 0
        assert rounds[3]["got"]["result"]["received"] == 1024 and rounds[3]["nres"]["consumed"] == 320
        assert rounds[4]["nres"]["backlog"] > 0 and rounds[4]["nres"]["arp_replies"] > 0


def test_a_block_that_does_not_match_the_call_is_a_no_op():
    _dev()
    worlds, n_shared = worlds_of(2)
    legs = upload(worlds, n_shared)
    before = [snapshot(leg) for leg in legs]

    def untouched(what):
        torch.cuda.synchronize()
        for leg, was in zip(legs, before):
            assert all(torch.equal(x, y) for x, y in zip(was, snapshot(leg))), f"{what}: a buffer changed"

    X.responder_queues_dev(responder_block(legs, 0x7), 2, OPTS)
    untouched("a block prepared for other options")
    X.responder_queues_dev(responder_block(legs, OPTS), 1, OPTS)
    untouched("a block of two queues in a call over one")
    X.responder_queues_dev(responder_block(legs[:1], OPTS), 2, OPTS)
    untouched("a block of one queue in a call over two")
    rq_block = block_of(legs, legs, [leg.umem.data for leg in legs], OPTS)
    assert rq_block.numel() >= 64
    X.responder_queues_dev(rq_block, 2, OPTS)
    untouched("an xsk_gpu_rx_queues_prepare block")
    X.rx_queues_dev(responder_block(legs, OPTS), 2, OPTS)
    untouched("this call's block handed to xsk_gpu_rx_queues_dev")
    zeros = to_dev(np.zeros(64, np.uint8))
    X.responder_queues_dev(zeros, 1, 0)
    untouched("64 zero bytes")
    # and the matching block is not a no-op: the same legs, the same call
    rounds = [LW.spec_round(w) for w in worlds]
    X.responder_queues_dev(responder_block(legs, OPTS), 2, OPTS)
    torch.cuda.synchronize()
    wrong = []
    for q, r in enumerate(rounds):
        wrong += problems(f"queue {q}", legs[q].hold, r)
    assert not wrong, " | ".join(wrong)
