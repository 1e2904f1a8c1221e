"""GPU parity of xsk_gpu_responder_dev: hand-written cases, each run three ways from one initial state --
the one call; xsk_gpu_rx_fused_loop_dev followed by xsk_gpu_neigh_serve_dev; the Python spec (loop_world.spec_round:
rx_pass_spec, neigh_spec, tx_complete_rings_spec) -- and compared as tests/test_gpu_loop_fuzz.py's hold compares: every
ring entry and index word (`up` and the stack ring's consumer word among them), the pool, the whole UMEM, every output of
the fused call, the responder's result and counters, sentinels around every buffer; the two device legs byte for byte.
The base shape: 64 frames offered, 8 ports, 16 entries in the steering table and 16 in the neighbour table, 2048-B
chunks.  What a case is about is asserted from the spec's record on top of the comparison.  All comparisons are exact."""
import errno

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import neigh_frames as NF  # noqa: E402
from tests import rx_dev_spec as RS  # noqa: E402
from tests.responder_dev import (CHUNK, RLeg, echo4, hand_world, snapshot, solicit, stranger, three_ways,  # noqa: E402
                                 who_has)
from tests.test_gpu_ingress import _dev  # noqa: E402

TAG1 = NF.G.TAGS[1]


def added(before: RS.RingState, after: RS.RingState):
    """The frame numbers (chunk numbers) of the entries a ring received, in ring order."""
    n = (after.prod - before.prod) & RS.M32
    return [int(after.entries[after.slot(before.prod + k)]["addr"]) // CHUNK for k in range(n)]


def mixed_offer(n=64):
    """Echo requests with an ARP request at i % 8 == 3 and a solicitation at i % 8 == 6, the ports interleaved: of 64
    frames every port gets six echo requests, one ARP request and one solicitation."""
    kinds, frames = [], []
    for i in range(n):
        p = (i // 8 + i) % 8
        kind = "arp" if i % 8 == 3 else "ns" if i % 8 == 6 else "echo"
        frames.append(who_has(p) if kind == "arp" else solicit(p) if kind == "ns" else echo4(p, i))
        kinds.append((kind, p))
    return frames, kinds


@pytest.mark.parametrize("n_comp,complete_max", [(0, 64), (4, 0), (4, 64)], ids=["no-comp", "complete-max-0", "comp"])
def test_mixed_traffic_and_the_three_exits_of_the_loop_body(n_comp, complete_max):
    """opts 0x17, 48 echo requests, 8 ARP requests and 8 solicitations in one RX offer: every request comes back on its
    port's TX ring, behind that port's echo replies, in this one call -- behind each exit of the loop body (no completion
    rings; completion rings with a bound of zero; its end)."""
    _dev()
    frames, kinds = mixed_offer()
    w = hand_world(frames, n_comp=n_comp, complete_max=complete_max)
    tx_before = [t.copy() for t in w.txs]
    r, _, _ = three_ways(w, tag=f"mixed, n_comp {n_comp}, complete_max {complete_max}")
    assert r["got"]["result"]["received"] == 64 and r["got"]["result"]["replied"] == 48
    assert r["got"]["result"]["passed"] == 16 and r["got"]["result"]["pass_full"] == 0
    assert r["nres"] == dict(consumed=16, arp_replies=8, na_replies=8, up=0, backlog=0)
    for p in range(8):
        got = [kinds[i][0] for i in added(tx_before[p], w.txs[p])]
        assert all(kinds[i][1] == p for i in added(tx_before[p], w.txs[p]))
        n_echo = got.count("echo")
        assert n_echo == 6 and got[:n_echo] == ["echo"] * n_echo and sorted(got[n_echo:]) == ["arp", "ns"], (p, got)


@pytest.mark.parametrize("opts", [0, 0x2])
def test_reference_mode_and_tagged_arp(opts):
    """opts 0: ARP only, a solicitation goes up, and so does a tagged ARP request.  opts 0x2: tagged ARP is answered."""
    _dev()
    frames = [echo4(1, 1), who_has(1), solicit(2), who_has(3, TAG1), echo4(3, 2), who_has(4), stranger(), echo4(4, 3),
              who_has(5, TAG1), solicit(6, TAG1)]
    r, _, _ = three_ways(hand_world(frames, opts=opts), tag=f"opts {opts:#x}")
    assert r["nres"]["na_replies"] == 0 and r["nres"]["backlog"] == 0
    assert r["nres"]["arp_replies"] == (2 if opts == 0 else 4)
    assert r["nres"]["up"] == r["nres"]["consumed"] - r["nres"]["arp_replies"] >= 3


def test_a_backlog_is_served_in_front_of_what_this_call_passes():
    _dev()
    backlog = [who_has(1), stranger(), solicit(2), who_has(3), stranger()]
    frames = [echo4(1, 1), who_has(1), stranger(), solicit(2), echo4(3, 2), who_has(3)]
    w = hand_world(frames, backlog)
    tx_before, up_before = [t.copy() for t in w.txs], w.up.copy()
    r, _, _ = three_ways(w, tag="backlog")
    assert r["nres"] == dict(consumed=9, arp_replies=4, na_replies=2, up=3, backlog=0)
    n = len(frames)
    assert added(tx_before[1], w.txs[1]) == [0, n + 0, 1]          # the echo reply, the old request, the new one
    assert added(tx_before[2], w.txs[2]) == [n + 2, 3]
    assert added(tx_before[3], w.txs[3]) == [4, n + 3, 5]
    assert added(up_before, w.up) == [n + 1, n + 4, 2]


def test_room_is_what_the_step_left_not_what_it_found():
    """Port 2's TX ring has room for its three echo replies and exactly one more entry; two ARP requests for port 2 are
    offered.  The first is answered; the second stays on the stack ring, untouched, with a backlog of 1.  (A room read
    before the step's publish would answer both, onto entries the ring does not have.)"""
    _dev()
    frames = [echo4(2, 1), who_has(0), echo4(2, 2), who_has(2), echo4(2, 3), solicit(5), who_has(2)]
    rooms = [64] * 8
    rooms[2] = 4
    w = hand_world(frames, rooms=rooms)
    tx_before, stack_before = w.txs[2].copy(), w.stack.copy()
    second = w.umem[6 * CHUNK:7 * CHUNK].copy()
    r, _, _ = three_ways(w, tag="stale room")
    assert r["got"]["result"]["replied"] == 3 and r["got"]["result"]["tx_full"] == 0
    assert r["nres"] == dict(consumed=3, arp_replies=2, na_replies=1, up=0, backlog=1)
    assert added(tx_before, w.txs[2]) == [0, 2, 4, 3] and w.txs[2].free() == 0
    assert added(stack_before, w.stack) == [1, 3, 5, 6] and w.stack.used() == 1
    assert (w.umem[6 * CHUNK:7 * CHUNK] == second).all()


@pytest.mark.parametrize("up_room,want", [(0, dict(consumed=1, arp_replies=1, na_replies=0, up=0, backlog=4)),
                                          (1, dict(consumed=3, arp_replies=2, na_replies=0, up=1, backlog=2))])
def test_up_full_and_up_with_room_for_one(up_room, want):
    _dev()
    frames = [who_has(0), stranger(), who_has(1), stranger(), who_has(2)]
    r, _, _ = three_ways(hand_world(frames, up_size=8, up_used=8 - up_room), tag=f"up room {up_room}")
    assert r["nres"] == want


def test_serve_max_1_with_several_entries_waiting():
    _dev()
    r, _, _ = three_ways(hand_world([who_has(0), echo4(0, 1), solicit(1)], [who_has(2), stranger()], serve_max=1),
                         tag="serve_max 1")
    assert r["nres"] == dict(consumed=1, arp_replies=1, na_replies=0, up=0, backlog=3)


def test_serve_max_1024_with_1024_entries_waiting_on_a_stack_ring_of_1024():
    _dev()
    backlog = [(who_has, solicit, lambda p: stranger())[i % 3](i % 8) for i in range(1024)]
    w = hand_world([echo4(0, 1), who_has(1), echo4(2, 2)], backlog, stack_size=1024, serve_max=1024, tx_size=256,
                   up_size=1024, n_comp=4)
    assert w.stack.used() == w.stack.size == 1024
    r, _, _ = three_ways(w, tag="serve_max 1024")
    assert r["got"]["result"]["pass_full"] == 1
    assert r["nres"]["consumed"] == 1024 and r["nres"]["backlog"] == 0 and r["nres"]["up"] == 341
    assert r["nres"]["arp_replies"] == 342 and r["nres"]["na_replies"] == 341


def test_nothing_received_and_a_backlog():
    _dev()
    w = hand_world([], [who_has(0), solicit(1), stranger()], n_comp=4)
    assert w.rx.used() == 0
    r, _, _ = three_ways(w, tag="nothing received")
    assert r["got"]["result"]["received"] == 0
    assert r["nres"] == dict(consumed=3, arp_replies=1, na_replies=1, up=1, backlog=0)


def test_a_full_stack_ring_shows_the_responder_only_what_fitted():
    _dev()
    frames = [who_has(0), who_has(1), solicit(2), who_has(3), solicit(4)]
    w = hand_world(frames, [stranger()] * 6, stack_size=8, up_size=8, up_used=8)  # (up full: the backlog stays)
    r, _, _ = three_ways(w, tag="stack ring full")
    assert r["got"]["result"]["passed"] == 2 and r["got"]["result"]["pass_full"] == 3
    assert r["nres"] == dict(consumed=0, arp_replies=0, na_replies=0, up=0, backlog=8)
    w = hand_world(frames, [stranger()] * 6, stack_size=8)
    r, _, _ = three_ways(w, tag="stack ring full, up with room")
    assert r["got"]["result"]["pass_full"] == 3
    assert r["nres"] == dict(consumed=8, arp_replies=2, na_replies=0, up=6, backlog=0)


def test_max_batch_1():
    _dev()
    r, _, _ = three_ways(hand_world([who_has(3), echo4(1, 1), solicit(2)], max_batch=1), tag="max_batch 1")
    assert r["got"]["result"]["received"] == 1
    assert r["nres"] == dict(consumed=1, arp_replies=1, na_replies=0, up=0, backlog=0)


def test_max_batch_1024_with_1024_offered_of_which_100_are_requests():
    _dev()
    frames = [(who_has((i // 10) % 8) if i % 20 else solicit((i // 10) % 8)) if i % 10 == 0 and i < 1000 else
              echo4(i % 8, i) for i in range(1024)]
    w = hand_world(frames, max_batch=1024, tx_size=256, stack_size=128, serve_max=1024, n_comp=4, complete_max=1024)
    r, _, _ = three_ways(w, tag="max_batch 1024")
    assert r["got"]["result"]["received"] == 1024 and r["got"]["result"]["replied"] == 924
    assert r["nres"] == dict(consumed=100, arp_replies=50, na_replies=50, up=0, backlog=0)


def test_index_words_within_8_of_2_to_the_32():
    """On the stack ring, `up` and a TX ring: each word crosses 2^32 in this call."""
    _dev()
    tx_prod = [0x1000 + 3 * p for p in range(8)]
    tx_prod[1] = 0xFFFFFFFE
    frames = [echo4(1, 1), who_has(1), stranger(), echo4(1, 2), solicit(1), stranger(), who_has(2), stranger()]
    w = hand_world(frames, [stranger(), who_has(1)], stack_prod=0xFFFFFFFD, up_prod=0xFFFFFFFF, tx_prod=tx_prod)
    r, _, _ = three_ways(w, tag="index words near 2^32")
    assert r["crossed"] and r["nres"]["consumed"] == 8 and r["nres"]["backlog"] == 0
    assert w.stack.prod < 8 and w.stack.cons < 8 and w.up.prod < 8 and w.txs[1].prod < 8


def test_optional_outputs_null():
    """d_nres and d_nstats NULL; the fused call's optional outputs NULL.  Nothing is written where NULL was passed."""
    _dev()
    frames, _ = mixed_offer(24)
    three_ways(hand_world(frames, n_comp=4), nres=False, nstats=False, tag="d_nres and d_nstats NULL")
    three_ways(hand_world(frames, n_comp=4, outputs=False), tag="the fused call's outputs NULL")
    three_ways(hand_world(frames, outputs=False), nres=False, nstats=False, tag="every optional output NULL")


@pytest.mark.parametrize("what", ["max_batch 1025", "serve_max 0"])
def test_refusals_have_written_nothing(what):
    _dev()
    frames, _ = mixed_offer(16)
    w = hand_world(frames, [who_has(0)], max_batch=1025 if what == "max_batch 1025" else 64,
                   serve_max=0 if what == "serve_max 0" else 64, n_comp=4)
    leg = RLeg(w)
    before = snapshot(leg)
    with pytest.raises(X.XskGpuError) as e:
        leg.responder()
    torch.cuda.synchronize()
    assert e.value.rc == -errno.EINVAL
    assert all(torch.equal(x, y) for x, y in zip(before, snapshot(leg))), "the refused call wrote"
