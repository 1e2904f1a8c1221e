"""GPU parity of xsk_gpu_rx_pass_step_dev / xsk_gpu_rx_pass_end_dev: the steered RX step with a stack ring.  One RX
ring, one fill ring and one pool in device memory, a TX ring per steered port and a descriptor ring for the frames the
filter passes to the kernel stack; after a step they hold what tests/rx_pass_spec.py (the end rule written as one plain
loop behind rx_steer_spec's pieces) leaves from the same state, and without a stack ring, or with a full one, what
xsk_gpu_rx_step_steer_dev() itself leaves.

Common to every case (as in tests/test_gpu_rx_step_steer_dev.py, whose helpers these are): every ring, index-word pair,
pool stack, count word, output array, result and workspace sits between two runs of the sentinel byte SENT, which must
survive; the traffic is dual stack with VLAN tags, every drop verdict and nonzero `options` on the RX entries; the free
part of every ring holds stale bytes that must stay where the step stores nothing."""
import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import egress_ports_spec as EP  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests import rx_dev_spec as RS  # noqa: E402
from tests import rx_pass_spec as PS  # noqa: E402
from tests import rx_steer_spec as RP  # noqa: E402
from tests import steer_spec as SS  # noqa: E402
from tests.test_gpu_egress import SENT  # noqa: E402
from tests.test_gpu_ingress import _dev, stats_of, to_dev  # noqa: E402
from tests.test_gpu_rx_step_dev import WRAP, DevRing, Guarded  # noqa: E402
from tests.test_gpu_rx_step_steer_dev import (SteerState, _port_replies, _table, _traffic, make_state,  # noqa: E402
                                               port_stats_of, pow2_at_least)


def make_stack(size, prod, room, seed=0):
    """A stack ring of `size` descriptors with `room` free entries and its producer word at `prod`; every entry, free
    or not, holds stale nonzero bytes."""
    rng = np.random.default_rng(size + seed)
    s = RS.RingState(np.zeros(size, oracle.DESC_DTYPE), prod, (prod - (size - room)) & RS.M32)
    s.entries["addr"] = rng.integers(1, 1 << 40, size, dtype=np.uint64)
    s.entries["len"], s.entries["options"] = 0x5A5A, 0xFACE
    assert s.free() == room
    return s


class PassState(SteerState):
    """SteerState with a stack ring (a RingState, or None), the pass step's workspace and its result."""

    def __init__(self, rx, fill, txs, stack, pool, max_batch, table=None, bound=None):
        super().__init__(rx, fill, txs, pool, max_batch, table, bound)
        self.ws = Guarded(X.rx_pass_step_dev_workspace_size(max_batch, self.n_ports))
        self.stack = DevRing(stack) if stack is not None else None
        self.stack_view = self.stack.view if self.stack is not None else None

    def step(self, d_umem, opts, default_port, outputs=True):
        X.rx_pass_step_dev(d_umem, self.rx.view, self.fill.view, self.views, self.stack_view, self.pool.view,
                           self.max_batch, self.table, self.n_entries, default_port, self.ws.data, bound=self.bound,
                           actions=self.actions.data if outputs else None, ports=self.ports.data if outputs else None,
                           port_counts=self.counts.data if outputs else None, stats=self.stats,
                           port_stats=self.port_stats.data if outputs else None, res=self.res.data, opts=opts)

    def guards(self):
        return super().guards() + ([self.stack.words, self.stack.ent] if self.stack is not None else [])

    def result(self) -> dict:
        r = self.res.get(PS.RESULT_DTYPE)[0]
        return {k: int(r[k]) for k in PS.RESULT_KEYS}

    def check(self, rx, fill, txs, pool, stack=None):
        super().check(rx, fill, txs, pool)
        assert (stack is None) == (self.stack is None)
        if stack is not None:
            g = self.stack.read()
            assert (g.prod, g.cons) == (stack.prod, stack.cons), ("stack", g.prod, g.cons, stack.prod, stack.cons)
            bad = np.nonzero(g.entries != stack.entries)[0]
            assert len(bad) == 0, ("stack", bad[:5], g.entries[bad[:5]], stack.entries[bad[:5]])


def spec_after(umem, rx, fill, txs, stack, pool, max_batch, opts, table, default_port, bound):
    """tests/rx_pass_spec.spec_step_pass on copies: (UMEM after, states after, stats, port stats, the spec's dict)."""
    s = (rx.copy(), fill.copy(), [t.copy() for t in txs], pool.copy(), None if stack is None else stack.copy())
    u = umem.copy()
    st = dict.fromkeys(IS.KEYS, 0)
    pst = [dict.fromkeys(EP.STATS_KEYS, 0) for _ in txs]
    got = PS.spec_step_pass(u, s[0], s[1], s[2], s[4], s[3], max_batch, opts, table, default_port,
                            SS.ALL_BOUND if bound is None else bound, st, pst)
    return u, s, st, pst, got


def n_pass(got, n):
    return int((got["actions"][:n] == SS.XDP_PASS).sum())


# ---- the matrix ------------------------------------------------------------------------------------------------------

CASES = [(n, p, o) for n in (1, 64, 65, 256, 257, 1024, 1025, 1300) for p in (1, 3, 64) for o in (0, 0x17)]


@pytest.mark.parametrize("n,n_ports,opts", CASES)
def test_against_the_spec(n, n_ports, opts):
    """Up to 1024 frames the one-workgroup path, above it the launched one.  A table mixing IPv4 and IPv6 keys; the
    default port alternates between port 0 and PASS; the ring of the port with the most replies is cut below them and,
    with several ports, the next port's ring is full; the stack ring's producer word starts three below 2^32; in half
    the cases the stack ring has room for Q // 2 descriptors only, in the other half for all."""
    _dev()
    case = CASES.index((n, n_ports, opts))
    default_port = SS.PASS if (case // 2) % 2 else 0
    cut = (case % 2 + (case // 2) % 3 + case // 6) % 2 == 1  # over the option words, the port counts and the sizes
    bound = SS.ALL_BOUND & ~2 if n_ports > 1 else None
    max_batch = n + (5 if n in (65, 257, 1300) else 0)
    umem, descs = _traffic(n)
    table = _table(n, opts, n_ports)
    size = pow2_at_least(n)
    R = _port_replies(n, n, max_batch, opts, n_ports, default_port, bound if bound is not None else SS.ALL_BOUND)
    rooms = [4096] * n_ports
    by_replies = sorted(range(n_ports), key=lambda p: -R[p])
    rooms[by_replies[0]] = max(R[by_replies[0]] - 1, 0)  # cut below its replies
    if n_ports > 1:
        rooms[by_replies[1]] = 0                         # a full ring
    start = (WRAP, 0x12345 + size // 2, 0)[case % 3]
    rx, fill, txs, pool = make_state(n_ports, size, start, descs, size // 2, size // 2 + 2, 2 * size + 3, rooms)
    # Q from the spec without a stack ring (pass_full == Q there), then the ring that is cut or roomy
    Q = spec_after(umem, rx, fill, txs, None, pool, max_batch, opts, table, default_port, bound)[4]["result"]["pass_full"]
    stack = make_stack(2 * size, WRAP, Q // 2 if cut else min(Q + 3, 2 * size), seed=case)
    after, want, st, pst, got = spec_after(umem, rx, fill, txs, stack, pool, max_batch, opts, table, default_port, bound)
    res = got["result"]
    assert n_pass(got, n) == Q == res["passed"] + res["pass_full"]
    if n >= 64:  # conditions of the input: a case cannot pass empty-handed
        assert Q >= 4
        if cut:
            assert 0 < res["passed"] < Q and res["pass_full"] >= 1
        else:
            assert res["passed"] == Q and want[4].prod < 0x1000  # the producer word wrapped past 2^32
    d = PassState(rx, fill, txs, stack, pool, max_batch, table, bound)
    d_umem = to_dev(umem)
    d.step(d_umem, opts, default_port)
    torch.cuda.synchronize()
    d.check(want[0], want[1], want[2], want[3], want[4])
    d.check_outputs(got)
    assert d.result() == res and res["received"] == n
    assert stats_of(d.stats) == st and port_stats_of(d.port_stats, n_ports) == pst
    assert (d_umem.cpu().numpy() == after).all(), "UMEM differs from the spec's"


# ---- the identity with the steered step itself ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [64, 1300])
@pytest.mark.parametrize("full_ring", [False, True])
def test_without_room_on_a_stack_ring_the_step_is_rx_step_steer_dev(n, full_ring):
    """stack == NULL, or a stack ring with no free entry: every ring, index word, pool entry, counter and UMEM byte ends
    where xsk_gpu_rx_step_steer_dev() leaves it from the same state; the first six result words are equal, passed == 0
    and pass_full == Q."""
    _dev()
    opts, n_ports = 0x17, 3
    umem, descs = _traffic(n)
    table = _table(n, opts, n_ports)
    size = pow2_at_least(n)
    rx, fill, txs, pool = make_state(n_ports, size, WRAP, descs, size // 2, size // 2, 2 * size, [4096, 3, 4096])
    stack = make_stack(16, WRAP, 0) if full_ring else None
    a = SteerState(rx, fill, txs, pool, n, table)
    b = PassState(rx, fill, txs, stack, pool, n, table)
    ua, ub = to_dev(umem), to_dev(umem)
    a.step(ua, opts, SS.PASS)
    b.step(ub, opts, SS.PASS)
    torch.cuda.synchronize()
    b.check(a.rx.read(), a.fill.read(), [t.read() for t in a.txs], a.pool.read(), stack)
    ra, rb = a.result(), b.result()
    Q = int((b.actions.get()[:n] == SS.XDP_PASS).sum())
    assert {k: rb[k] for k in ra} == ra and rb["passed"] == 0 and rb["pass_full"] == Q and Q >= 4 and ra["received"] == n
    assert stats_of(a.stats) == stats_of(b.stats) and torch.equal(ua, ub)
    assert port_stats_of(a.port_stats, n_ports) == port_stats_of(b.port_stats, n_ports)
    assert (a.actions.get() == b.actions.get()).all() and (a.ports.get() == b.ports.get()).all()
    assert (a.counts.get() == b.counts.get()).all()


# ---- consecutive steps -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_batch,size,stack_size", [(48, 64, 16), (1100, 2048, 256)])
def test_three_consecutive_steps_cross_the_stack_rings_end(max_batch, size, stack_size):
    """Three steps on one device state, the RX ring refilled and the TX and stack rings drained by device copies in
    between; the stack ring's slots wrap past its end and its index words past 2^32, and it is too small for some
    step's PASS frames."""
    _dev()
    per, n_ports, opts = max_batch - 5, 3, 0x17
    umem, descs = _traffic(3 * per)
    table = _table(3 * per, opts, n_ports)
    rx, fill, txs, pool = make_state(n_ports, size, WRAP - per, descs[:per], size // 2, size, 3 * size, [4096] * 3)
    stack = make_stack(stack_size, 0xFFFFFFF8, stack_size)
    d = PassState(rx, fill, txs, stack, pool, max_batch, table)
    d_umem = to_dev(umem)
    s = [rx.copy(), fill.copy(), [t.copy() for t in txs], pool.copy(), stack.copy()]
    u = umem.copy()
    st = dict.fromkeys(IS.KEYS, 0)
    pst = [dict.fromkeys(EP.STATS_KEYS, 0) for _ in txs]
    passed = pass_full = 0
    for k in range(3):
        if k:  # the peers: new RX entries, the TX rings, the stack ring and part of the fill ring consumed
            s[0].produce(descs[k * per:(k + 1) * per])
            s[1].cons = (s[1].cons + min(s[1].used(), per)) & RS.M32
            d.rx.write(s[0])
            d.fill.write(s[1])
            for t, dt in zip(s[2], d.txs):
                t.cons = t.prod
                dt.write(t)
            s[4].cons = s[4].prod
            d.stack.write(s[4])
        got = PS.spec_step_pass(u, s[0], s[1], s[2], s[4], s[3], max_batch, opts, table, SS.PASS, SS.ALL_BOUND, st, pst)
        assert got["result"]["received"] == per
        d.step(d_umem, opts, SS.PASS)
        torch.cuda.synchronize()
        d.check(s[0], s[1], s[2], s[3], s[4])
        d.check_outputs(got)
        assert d.result() == got["result"] and stats_of(d.stats) == st
        assert port_stats_of(d.port_stats, n_ports) == pst
        passed += got["result"]["passed"]
        pass_full += got["result"]["pass_full"]
    assert passed > stack_size and pass_full >= 1 and s[4].prod < 0x10000  # around the ring, past 2^32, once too small
    assert (d_umem.cpu().numpy() == u).all()


# ---- the empty RX ring ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_batch", [64, 1300])
def test_an_empty_rx_ring_leaves_every_byte_untouched(max_batch):
    _dev()
    umem, descs = _traffic(64)
    rx, fill, txs, pool = make_state(3, 64, WRAP, descs[:0], 64, 67, 80, [8, 0, 100])
    d = PassState(rx, fill, txs, make_stack(32, WRAP, 20), pool, max_batch, _table(64, 0x17, 3))
    d_umem = to_dev(umem)
    d.stats.fill_(SENT)
    d.port_stats.data.fill_(SENT)
    torch.cuda.synchronize()
    outputs = (d.ws, d.res, d.actions, d.ports, d.counts)
    before = [g.buf.clone() for g in d.guards() if g not in outputs]
    d.step(d_umem, 0x17, SS.PASS)
    torch.cuda.synchronize()
    after = [g.buf for g in d.guards() if g not in outputs]
    assert any(g is d.stack.ent for g in d.guards()) and all(torch.equal(a, b) for a, b in zip(before, after))
    assert bool((d.stats == SENT).all()) and torch.equal(d_umem, to_dev(umem))
    assert d.result() == dict.fromkeys(PS.RESULT_KEYS, 0) and all(g.intact() for g in outputs)
    assert (d.actions.get() == SS.XDP_DROP).all() and (d.ports.get() == SS.PASS).all()  # what the pad gets


# ---- garbage words -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_max", [64, 1300])
def test_garbage_words_in_front_of_end(n_max):
    """Action bytes that are none of 1, 2, 4, offsets that are not ascending and lie above the bound, counts above their
    segment, a received word above the bound, used > size on a TX ring and on the stack ring, a pool count above the
    capacity: the result is the spec's, nothing lands outside."""
    _dev()
    n_ports = 3
    rng = np.random.default_rng(n_max)
    descs = np.zeros(n_max, oracle.DESC_DTYPE)
    descs["addr"] = (np.arange(n_max, dtype=np.uint64) + np.uint64(1)) * np.uint64(2048)
    descs["len"], descs["options"] = np.arange(n_max) + 100, np.arange(n_max) + 0x300
    d_tx = descs.copy()
    d_tx["addr"] += 7
    d_tx["len"] = np.arange(n_max) + 60
    d_free = (np.arange(n_max, dtype=np.uint64) + np.uint64(5000)) * np.uint64(4096)
    actions = rng.choice([0, 1, 2, 2, 3, 4, 0xFF], n_max).astype(np.uint8)
    for off, n_free_word, received, stack_words in (
            ([n_max // 8, 0xFFFFFFFF, 3, n_max // 2], 0xFFFFFF00, 1 << 31, (0xFFFFFFFE, 0xFFFFFFFE)),
            ([0, n_max // 3, n_max // 4, n_max + 9], 2, n_max + 1, (5, 0x80000000)),
            ([5, 5, n_max - 1, 0], 0, 3, (0x10, 0x0C)),
            ([0, 0, 0, 0], 1, 0xFFFFFFFF, (3, 0xFFFFFFFF))):
        rx, fill, txs, pool = make_state(n_ports, 64, 7, descs[:0], 0, 0, n_max // 2 + 3, [8, 30, 2048])
        pool.n_free = n_free_word
        txs[1].prod = (txs[1].cons + 0x80000005) & RS.M32  # used > size: no room
        stack = make_stack(8, 0, 8)
        stack.prod, stack.cons = stack_words
        counts = np.zeros(n_ports, X.EGRESS_COUNTS_DTYPE)
        counts["n_tx"], counts["n_free"], counts["n_tx_full"] = (0xFFFFFFFF, 11, n_max // 4), 0xFFFFFFF0, (1, 2, 3)
        plan = np.zeros(1, RS.PLAN_DTYPE)
        plan["received"], plan["refilled"] = received, 9
        w = [rx.copy(), [t.copy() for t in txs], pool.copy(), stack.copy()]
        res = PS.spec_end_pass(w[0], w[1], w[3], w[2], dict(received=received, refilled=9), descs, actions, off, d_tx,
                               d_free, [{k: int(c[k]) for k in c.dtype.names} for c in counts], n_max)
        d = PassState(rx, fill, txs, stack, pool, n_max)
        g = [Guarded(a.nbytes, a) for a in (plan, descs, actions, np.array(off, np.uint32), d_tx, d_free, counts)]
        X.rx_pass_end_dev(d.rx.view, d.views, d.stack_view, d.pool.view, g[0].data, g[1].data, g[2].data, g[3].data,
                          g[4].data, g[5].data, g[6].data, n_max, d.ws.data, d.res.data)
        torch.cuda.synchronize()
        d.check(w[0], fill, w[1], w[2], w[3])
        assert d.result() == res and all(x.intact() for x in g), (off, res)
        assert res["passed"] == min(res["passed"] + res["pass_full"], stack.free())


# ---- begin, prepare, the two existing calls and end by hand --------------------------------------------------------------

@pytest.mark.parametrize("n,max_batch", [(65, 100), (1300, 1310)])
def test_composed_by_hand_equals_the_wrapper(n, max_batch):
    _dev()
    dev = _dev()
    opts, n_ports = 0x17, 3
    umem, descs = _traffic(n)
    table = _table(n, opts, n_ports)
    size = pow2_at_least(n)
    R = _port_replies(n, n, max_batch, opts, n_ports, SS.PASS, SS.ALL_BOUND)
    rooms = [4096, max(R[1] - 1, 0), 0]
    rx, fill, txs, pool = make_state(n_ports, size, WRAP, descs, size // 3, size // 2, 2 * size, rooms)
    stack = make_stack(size, 0xFFFFFFFE, 6)
    a = PassState(rx, fill, txs, stack, pool, max_batch, table)
    b = PassState(rx, fill, txs, stack, pool, max_batch, table)
    ua, ub = to_dev(umem), to_dev(umem)
    a.step(ua, opts, SS.PASS)
    g_descs, g_plan, g_verd = Guarded(max_batch * 16), Guarded(32), Guarded(max_batch)
    g_out, g_off, g_room = Guarded(max_batch * 16), Guarded(4 * (n_ports + 1)), Guarded(4 * n_ports)
    g_tx, g_free = Guarded(max_batch * 16), Guarded(max_batch * 8)
    sws = torch.empty(max(X.steer_workspace_size(max_batch, n_ports), 4), dtype=torch.uint8, device=dev)
    ews = torch.empty(max(X.egress_ports_workspace_size(max_batch, n_ports), 4), dtype=torch.uint8, device=dev)
    X.rx_begin_dev(b.rx.view, b.fill.view, b.views[0], b.pool.view, max_batch, g_descs.data, g_plan.data)
    X.rx_prepare_ports_dev(b.views, g_plan.data, g_descs.data, max_batch, g_room.data)
    X.ingress_steer_dev(ub, g_descs.data, max_batch, b.table, b.n_entries, SS.PASS, n_ports, None, b.actions.data,
                        b.ports.data, g_out.data, g_off.data, g_verd.data, None, b.stats, sws, opts=opts)
    X.egress_ports_dev(g_out.data, g_verd.data, g_off.data, n_ports, max_batch, g_tx.data, g_free.data, b.counts.data,
                       tx_room=g_room.data, stats=b.stats, port_stats=b.port_stats.data, workspace=ews)
    X.rx_pass_end_dev(b.rx.view, b.views, b.stack_view, b.pool.view, g_plan.data, g_descs.data, b.actions.data,
                      g_off.data, g_tx.data, g_free.data, b.counts.data, max_batch, b.ws.data, b.res.data)
    torch.cuda.synchronize()
    b.check(a.rx.read(), a.fill.read(), [t.read() for t in a.txs], a.pool.read(), a.stack.read())
    after, spec, st, pst, got = spec_after(umem, rx, fill, txs, stack, pool, max_batch, opts, table, SS.PASS, None)
    a.check(spec[0], spec[1], spec[2], spec[3], spec[4])
    a.check_outputs(got)
    b.check_outputs(got)
    assert a.result() == b.result() == got["result"] and got["result"]["passed"] == 6 and got["result"]["pass_full"] >= 1
    assert stats_of(a.stats) == stats_of(b.stats) == st and torch.equal(ua, ub)
    assert port_stats_of(a.port_stats, n_ports) == port_stats_of(b.port_stats, n_ports) == pst
    assert all(g.intact() for g in (g_descs, g_plan, g_verd, g_out, g_off, g_room, g_tx, g_free))
