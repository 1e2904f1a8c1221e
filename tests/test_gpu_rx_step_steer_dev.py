"""GPU parity of xsk_gpu_rx_step_steer_dev / xsk_gpu_rx_prepare_ports_dev / xsk_gpu_rx_ports_end_dev: one RX ring, one
fill ring and one pool in device memory, a TX ring per steered port; after a step they hold what tests/rx_steer_spec.py
(the numpy composition of the begin, steering, transform, per-port egress and end rules, with the oracle's verdicts)
leaves from the same state, and with one port what xsk_gpu_rx_step_dev() itself leaves.

Common to every case: every ring, index-word pair, pool stack, count word, output array, result and workspace sits
between two runs of the sentinel byte tests.test_gpu_egress.SENT, which must survive; the traffic is
tests.v6_frames.mixed_batch6 (dual stack, VLAN tags, every drop verdict) with nonzero `options` on the RX entries; the
free part of every ring holds stale bytes that must stay where the step stores nothing."""
import functools

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import egress_ports_spec as EP  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests import rx_dev_spec as RS  # noqa: E402
from tests import rx_steer_spec as RP  # noqa: E402
from tests import steer_spec as SS  # noqa: E402
from tests.test_gpu_egress import SENT  # noqa: E402
from tests.test_gpu_ingress import _dev, stats_of, to_dev  # noqa: E402
from tests.test_gpu_rx_step_dev import WRAP, DevPool, DevRing, DevState, Guarded  # noqa: E402
from tests.test_gpu_steer import dev_bound, dev_table  # noqa: E402
from tests.v6_frames import mixed_batch6  # noqa: E402

STRIDE = 2048
STARTS = (0, 0x12345, WRAP)
TX_SIZES = (8, 64, 2048, 256, 16)


def pow2_at_least(n):
    return 1 << max(3, (max(n, 1) - 1).bit_length())


class SteerState:
    """(rx, fill, txs, pool) on the device, with the steered step's workspace, outputs, counters and result."""

    def __init__(self, rx, fill, txs, pool, max_batch, table=None, bound=None):
        self.rx, self.fill, self.pool = DevRing(rx), DevRing(fill), DevPool(pool)
        self.txs = [DevRing(t) for t in txs]
        self.n_ports, self.max_batch = len(txs), max_batch
        self.views = [t.view for t in self.txs]
        self.ws = Guarded(X.rx_step_steer_dev_workspace_size(max_batch, self.n_ports))
        self.res = Guarded(32)
        self.actions, self.ports = Guarded(max_batch), Guarded(max_batch)
        self.counts = Guarded(16 * self.n_ports)
        self.port_stats = Guarded(40 * self.n_ports, np.zeros(40 * self.n_ports, np.uint8))
        self.stats = torch.zeros(40, dtype=torch.uint8, device=_dev())
        self.table, self.n_entries = dev_table(table or {})
        self.bound = dev_bound(bound)

    def step(self, d_umem, opts, default_port, outputs=True):
        X.rx_step_steer_dev(d_umem, self.rx.view, self.fill.view, self.views, self.pool.view, self.max_batch, self.table,
                            self.n_entries, default_port, self.ws.data, bound=self.bound,
                            actions=self.actions.data if outputs else None, ports=self.ports.data if outputs else None,
                            port_counts=self.counts.data if outputs else None, stats=self.stats,
                            port_stats=self.port_stats.data if outputs else None, res=self.res.data, opts=opts)

    def guards(self):
        gs = [self.ws, self.res, self.actions, self.ports, self.counts, self.port_stats, self.pool.addr, self.pool.word]
        for r in (self.rx, self.fill, *self.txs):
            gs += [r.words, r.ent]
        return gs

    def result(self) -> dict:
        r = self.res.get(RP.RESULT_DTYPE)[0]
        assert (r["reserved"] == 0).all()
        return {k: int(r[k]) for k in RP.RESULT_KEYS}

    def check(self, rx, fill, txs, pool):
        """After a synchronisation: every ring's whole entry array, the index words, the pool's stack below its count
        and the count against the expected states; every sentinel."""
        rings = [("rx", self.rx, rx), ("fill", self.fill, fill)] + [(f"tx{p}", g, w) for p, (g, w) in
                                                                     enumerate(zip(self.txs, txs))]
        for name, got, want in rings:
            g = got.read()
            assert (g.prod, g.cons) == (want.prod, want.cons), (name, g.prod, g.cons, want.prod, want.cons)
            bad = np.nonzero(g.entries != want.entries)[0]
            assert len(bad) == 0, (name, bad[:5], g.entries[bad[:5]], want.entries[bad[:5]])
        p = self.pool.read()
        assert p.n_free == pool.n_free and (p.addr[:p.n()] == pool.addr[:pool.n()]).all(), (p.n_free, pool.n_free)
        assert all(g.intact() for g in self.guards()), "a sentinel was overwritten"

    def check_outputs(self, got):
        """actions, ports, the per-port counts and counter blocks against a spec_step_steer result."""
        assert (self.actions.get() == got["actions"]).all() and (self.ports.get() == got["ports"]).all()
        c = self.counts.get(X.EGRESS_COUNTS_DTYPE)
        assert [{k: int(c[p][k]) for k in c.dtype.names} for p in range(self.n_ports)] == got["counts"]


def port_stats_of(g: Guarded, n_ports):
    s = g.get(X.STATS_DTYPE)
    assert (s["timestamp"] == 0).all()
    return [{k: int(s[p][k]) for k in EP.STATS_KEYS} for p in range(n_ports)]


@functools.lru_cache(maxsize=None)
def _traffic(n, seed=0):
    """(UMEM, descriptors) of n mixed dual-stack frames, frame i inside chunk i; nonzero options.  Read-only."""
    umem, descs = mixed_batch6(max(n, 1), STRIDE, seed=0x57EE0000 + n + seed)
    descs = np.ascontiguousarray(descs, oracle.DESC_DTYPE)[:n].copy()
    descs["options"] = np.arange(n, dtype=np.uint32) + 0x1000
    umem.setflags(write=False)
    descs.setflags(write=False)
    return umem, descs


@functools.lru_cache(maxsize=None)
def _table(n, opts, n_ports, seed=0, entries=22):
    """Every second destination of the batch (at most `entries`), and one key of each family that does not occur: the
    table mixes IPv4 and IPv6 keys under every option word (the reference filter, opts == 0, redirects IPv4 only)."""
    umem, descs = _traffic(n, seed)
    table = SS.sample_table(SS.destinations(umem, descs, opts), entries, n_ports, seed=n + opts)
    table[SS.GS.key(bytes([198, 19, 255, 1]))] = 0
    table[SS.GS.key(bytes.fromhex("20010db8fffe") + bytes(9) + b"\x01")] = n_ports - 1
    assert {k[0] for k in table} == {4, 6} and len(table) == entries + 2
    return table


@functools.lru_cache(maxsize=None)
def _port_replies(n, k, max_batch, opts, n_ports, default_port, bound):
    """Replies per port of the first k frames: what a cut room has to lie below.  From the steered ingress alone."""
    umem, descs = _traffic(n)
    d = np.zeros(max_batch, oracle.DESC_DTYPE)
    d[:k] = descs[:k]
    ing = SS.spec_ingress_steer(umem.copy(), d, opts, _table(n, opts, n_ports), default_port, n_ports, bound)
    off = [int(x) for x in ing["off"]]
    return tuple(int((ing["verdicts"][off[p]:off[p + 1]] == 0).sum()) for p in range(n_ports))


def make_state(n_ports, size, start, descs, fill_free, pool_n, cap, rooms):
    """RingStates: `descs` on an RX ring of `size` entries, the fill ring with fill_free free slots, TX rings of sizes
    that differ per port (8 to 2048) with rooms[p] free slots (clamped to the size), a pool of pool_n frames.  Index
    words start near `start`; free slots hold stale nonzero bytes."""
    rng = np.random.default_rng(size * 31 + len(descs))
    rx = RS.RingState(np.zeros(size, oracle.DESC_DTYPE), start, start)
    rx.entries["addr"], rx.entries["len"], rx.entries["options"] = 0xA5A5A5A5, 0xA5A5, 0xDEAD
    rx.produce(descs)
    fill = RS.RingState(rng.integers(1, 1 << 40, size, dtype=np.uint64), start + 1 + size - fill_free, start + 1)
    txs = []
    for p in range(n_ports):
        ts = TX_SIZES[p % len(TX_SIZES)]
        room = min(rooms[p], ts)
        t = RS.RingState(np.zeros(ts, oracle.DESC_DTYPE), start + 2 + 3 * p + ts - room, start + 2 + 3 * p)
        t.entries["addr"] = rng.integers(1, 1 << 40, ts, dtype=np.uint64)
        t.entries["options"] = 0xBEEF
        txs.append(t)
    pool = RS.PoolState((np.arange(cap, dtype=np.uint64) + np.uint64(1 << 20)) * np.uint64(4096), pool_n)
    return rx, fill, txs, pool


def spec_after(umem, rx, fill, txs, pool, max_batch, opts, table, default_port, bound):
    """tests/rx_steer_spec.spec_step_steer on copies: (UMEM after, states after, stats, port stats, the spec's dict)."""
    s = (rx.copy(), fill.copy(), [t.copy() for t in txs], pool.copy())
    u = umem.copy()
    st = dict.fromkeys(IS.KEYS, 0)
    pst = [dict.fromkeys(EP.STATS_KEYS, 0) for _ in txs]
    got = RP.spec_step_steer(u, *s, max_batch, opts, table, default_port,
                             SS.ALL_BOUND if bound is None else bound, st, pst)
    return u, s, st, pst, got


# ---- the identity with the unsteered step itself -------------------------------------------------------------------

@pytest.mark.parametrize("opts", [0, 0x17])
def test_one_port_equals_rx_step_dev(opts):
    """n_ports == 1, no table, default port 0, d_bound NULL, 64 valid echo requests (all REDIRECT): rings, every index
    word, the pool, d_stats and the UMEM end where xsk_gpu_rx_step_dev() leaves them from the same state."""
    _dev()
    n, size = 64, 64
    umem = np.zeros(n * STRIDE, np.uint8)
    descs = np.ascontiguousarray(oracle.synth_batch(umem, n, 0, STRIDE, seed=0x1DE7, mode=0, len_lo=64, len_hi=1500),
                                 oracle.DESC_DTYPE)
    descs["options"] = 0x77
    assert (SS.spec_steer_batch(umem, descs, opts, {}, 0, 1)["actions"] == SS.XDP_REDIRECT).all()
    for tx_room in (64, 20):
        rx, fill, _, pool = make_state(1, size, WRAP, descs, size // 2, size // 2 + 2, size + 3, [0])
        tx = RS.RingState(np.zeros(size, oracle.DESC_DTYPE), WRAP + 2 + size - tx_room, WRAP + 2)
        tx.entries["addr"], tx.entries["options"] = np.arange(size, dtype=np.uint64) + np.uint64(1 << 41), 0xBEEF
        a = DevState(rx, fill, tx, pool, n)
        b = SteerState(rx, fill, [tx], pool, n)
        ua, ub = to_dev(umem), to_dev(umem)
        a.step(ua, opts)
        b.step(ub, opts, 0)
        torch.cuda.synchronize()
        want = [x.read() for x in (a.rx, a.fill, a.tx)] + [a.pool.read()]
        b.check(want[0], want[1], [want[2]], want[3])
        ra, rb = a.result(), b.result()
        assert {k: rb[k] for k in ra} == ra and ra["received"] == n and ra["replied"] == tx_room
        assert rb["redirected"] == n and rb["freed"] == n - tx_room
        assert stats_of(a.stats) == stats_of(b.stats) and torch.equal(ua, ub)
        assert not torch.equal(ua, to_dev(umem))  # the frames were answered


# ---- the matrix ------------------------------------------------------------------------------------------------------

CASES = [(n, p, o) for n in (1, 64, 65, 1024, 1025, 1300) for p in (1, 3, 64) for o in (0, 0x17)]


@pytest.mark.parametrize("n,n_ports,opts", CASES)
def test_against_the_spec(n, n_ports, opts):
    """Up to 1024 frames the one-workgroup path, above it the launched one.  A table mixing IPv4 and IPv6 keys; the
    default port alternates between port 0 and PASS; with several ports port 1 is unbound through *d_bound; the ring
    of the port with the most replies is cut below them and, with several ports, the next port's ring is full; three
    RX start indices over the cases."""
    _dev()
    case = CASES.index((n, n_ports, opts))
    start = STARTS[case % 3]
    # (behind the reference filter a PASS default leaves a small batch only its few table hits: from 1024 frames on)
    default_port = SS.PASS if (case // 2) % 2 and (opts or n >= 1024) else 0
    bound = SS.ALL_BOUND & ~2 if n_ports > 1 else None
    max_batch = n + (5 if n in (65, 1300) else 0)
    umem, descs = _traffic(n)
    table = _table(n, opts, n_ports)
    size = pow2_at_least(n)
    R = _port_replies(n, n, max_batch, opts, n_ports, default_port, bound if bound is not None else SS.ALL_BOUND)
    rooms = [4096] * n_ports
    by_replies = sorted(range(n_ports), key=lambda p: -R[p])
    rooms[by_replies[0]] = max(R[by_replies[0]] - 1, 0)  # cut below its replies
    if n_ports > 1:
        rooms[by_replies[1]] = 0                         # a full ring
    mid = start + size // 2 if start == 0x12345 else start
    rx, fill, txs, pool = make_state(n_ports, size, mid, descs, size // 2, size // 2 + 2, 2 * size + 3, rooms)
    after, want, st, pst, got = spec_after(umem, rx, fill, txs, pool, max_batch, opts, table, default_port, bound)
    res = got["result"]
    acts = got["actions"]
    if n >= 64:  # conditions of the input: mixed traffic (the reference filter passes what the wire filter drops)
        kinds = set(acts[:n].tolist())
        assert {SS.XDP_PASS, SS.XDP_REDIRECT} <= kinds and (SS.XDP_DROP in kinds or not opts)
        assert res["tx_full"] >= 1 and (res["replied"] >= 1 or max(R) < 2) and (sum(R) >= 8 or not opts)
        assert len(set(got["verdicts"].tolist())) >= (3 if opts else 2)
        assert n_ports == 1 or (got["ports"] != 1).all()  # the unbound port gets nothing
    d = SteerState(rx, fill, txs, pool, max_batch, table, bound)
    d_umem = to_dev(umem)
    d.step(d_umem, opts, default_port)
    torch.cuda.synchronize()
    d.check(*want)
    d.check_outputs(got)
    assert d.result() == res and res["received"] == n
    assert stats_of(d.stats) == st and port_stats_of(d.port_stats, n_ports) == pst
    assert (d_umem.cpu().numpy() == after).all(), "UMEM differs from the spec's"


# ---- consecutive steps -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_batch,size", [(48, 64), (1100, 2048)])
def test_three_consecutive_steps_cross_the_rings_ends(max_batch, size):
    """Three steps on one device state, the RX ring refilled and the TX rings drained by device copies in between; the
    slots wrap past every ring's end and the index words past 2^32.  Each step receives fewer frames than the bound:
    the pads are steered too."""
    _dev()
    per, n_ports, opts = max_batch - 5, 3, 0x17
    umem, descs = _traffic(3 * per)
    table = _table(3 * per, opts, n_ports)
    rx, fill, txs, pool = make_state(n_ports, size, WRAP - per, descs[:per], size // 2, size, 3 * size, [4096] * 3)
    d = SteerState(rx, fill, txs, pool, max_batch, table)
    d_umem = to_dev(umem)
    s = [rx.copy(), fill.copy(), [t.copy() for t in txs], pool.copy()]
    u = umem.copy()
    st = dict.fromkeys(IS.KEYS, 0)
    pst = [dict.fromkeys(EP.STATS_KEYS, 0) for _ in txs]
    for k in range(3):
        if k:  # the peer: new RX entries, the TX rings consumed, the fill ring consumed
            s[0].produce(descs[k * per:(k + 1) * per])
            s[1].cons = (s[1].cons + min(s[1].used(), per)) & RS.M32
            d.rx.write(s[0])
            d.fill.write(s[1])
            for t, dt in zip(s[2], d.txs):
                t.cons = t.prod
                dt.write(t)
        got = RP.spec_step_steer(u, s[0], s[1], s[2], s[3], max_batch, opts, table, 0, SS.ALL_BOUND, st, pst)
        assert got["result"]["received"] == per
        d.step(d_umem, opts, 0)
        torch.cuda.synchronize()
        d.check(*s)
        d.check_outputs(got)
        assert d.result() == got["result"] and stats_of(d.stats) == st
        assert port_stats_of(d.port_stats, n_ports) == pst
    assert s[0].cons < per * 3 and (d_umem.cpu().numpy() == u).all()  # the words wrapped


# ---- the pool's limit ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,max_batch", [(64, 64), (1300, 1300)])
def test_pool_limit_drops_the_tail(n, max_batch):
    """A pool with room for none, for a few and for all but one of the list: the first `pushed` addresses land, in list
    order (the ports' free lists, then the rest), the tail is dropped as pool_push() drops it."""
    _dev()
    n_ports, opts = 3, 0
    umem, descs = _traffic(n)
    table = _table(n, opts, n_ports)
    size = pow2_at_least(n)
    probe = spec_after(umem, *make_state(n_ports, size, 7, descs, 0, 0, 4 * size, [2, 4096, 1]), max_batch, opts, table,
                       SS.PASS, None)[4]["result"]["freed"]
    assert probe >= 10
    d_umem0 = to_dev(umem)
    cap = probe + 10
    for room in (0, 5, probe - 1, probe):
        rx, fill, txs, pool = make_state(n_ports, size, 7, descs, 0, cap - room, cap, [2, 4096, 1])
        after, want, st, pst, got = spec_after(umem, rx, fill, txs, pool, max_batch, opts, table, SS.PASS, None)
        assert got["result"]["freed"] == room and want[3].n_free == want[3].capacity
        d = SteerState(rx, fill, txs, pool, max_batch, table)
        d_umem = d_umem0.clone()
        d.step(d_umem, opts, SS.PASS)
        torch.cuda.synchronize()
        d.check(*want)
        assert d.result() == got["result"] and stats_of(d.stats) == st


# ---- garbage words -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_max", [64, 1300])
def test_garbage_words_in_front_of_end(n_max):
    """Offsets that are not ascending and lie above the bound, counts above their segment, a received word above the
    bound, used > size on a ring, a pool count above the capacity: the result is the spec's, nothing lands outside."""
    _dev()
    n_ports = 3
    rng = np.random.default_rng(n_max)
    descs = np.zeros(n_max, oracle.DESC_DTYPE)
    descs["addr"] = (np.arange(n_max, dtype=np.uint64) + np.uint64(1)) * np.uint64(2048)
    d_tx = descs.copy()
    d_tx["addr"] += 7
    d_tx["len"] = np.arange(n_max) + 60
    d_free = (np.arange(n_max, dtype=np.uint64) + np.uint64(5000)) * np.uint64(4096)
    actions = rng.choice([1, 2, 4], n_max).astype(np.uint8)
    for off, n_free_word, received in (([n_max // 8, 0xFFFFFFFF, 3, n_max // 2], 0xFFFFFF00, 1 << 31),
                                       ([0, n_max // 3, n_max // 4, n_max + 9], 2, n_max + 1),
                                       ([5, 5, n_max - 1, 0], 0, 3)):
        rx, fill, txs, pool = make_state(n_ports, 64, 7, descs[:0], 0, 0, n_max // 2 + 3, [8, 30, 2048])
        pool.n_free = n_free_word
        txs[1].prod = (txs[1].cons + 0x80000005) & RS.M32  # used > size: no room
        counts = np.zeros(n_ports, X.EGRESS_COUNTS_DTYPE)
        counts["n_tx"], counts["n_free"], counts["n_tx_full"] = (0xFFFFFFFF, 11, n_max // 4), 0xFFFFFFF0, (1, 2, 3)
        plan = np.zeros(1, RS.PLAN_DTYPE)
        plan["received"], plan["refilled"] = received, 9
        w = [rx.copy(), [t.copy() for t in txs], pool.copy()]
        res = RP.spec_end_ports(w[0], w[1], w[2], dict(received=received, refilled=9), descs, actions, off, d_tx, d_free,
                                [{k: int(c[k]) for k in c.dtype.names} for c in counts], n_max)
        d = SteerState(rx, fill, txs, pool, n_max)
        g = [Guarded(a.nbytes, a) for a in (plan, descs, actions, np.array(off, np.uint32), d_tx, d_free, counts)]
        X.rx_end_ports_dev(d.rx.view, d.views, d.pool.view, g[0].data, g[1].data, g[2].data, g[3].data, g[4].data,
                           g[5].data, g[6].data, n_max, d.ws.data, d.res.data)
        torch.cuda.synchronize()
        d.check(w[0], fill, w[1], w[2])
        assert d.result() == res and all(x.intact() for x in g), (off, res)


# ---- the empty RX ring ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_batch", [64, 1300])
def test_an_empty_rx_ring_leaves_every_byte_untouched(max_batch):
    _dev()
    umem, descs = _traffic(64)
    rx, fill, txs, pool = make_state(3, 64, WRAP, descs[:0], 64, 67, 80, [8, 0, 100])
    d = SteerState(rx, fill, txs, pool, max_batch, _table(64, 0x17, 3))
    d_umem = to_dev(umem)
    d.stats.fill_(SENT)
    d.port_stats.data.fill_(SENT)
    torch.cuda.synchronize()
    outputs = (d.ws, d.res, d.actions, d.ports, d.counts)
    before = [g.buf.clone() for g in d.guards() if g not in outputs]
    d.step(d_umem, 0x17, 0)
    torch.cuda.synchronize()
    after = [g.buf for g in d.guards() if g not in outputs]
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert bool((d.stats == SENT).all()) and torch.equal(d_umem, to_dev(umem))
    assert d.result() == dict.fromkeys(RP.RESULT_KEYS, 0) and all(g.intact() for g in outputs)
    assert (d.actions.get() == SS.XDP_DROP).all() and (d.ports.get() == SS.PASS).all()  # what the pad gets
    assert not d.counts.get().any()


# ---- begin, prepare, the two existing calls and end by hand --------------------------------------------------------------

@pytest.mark.parametrize("n,max_batch", [(65, 100), (1300, 1310)])
def test_composed_by_hand_equals_the_wrapper(n, max_batch):
    _dev()
    dev = _dev()
    opts, n_ports = 0x17, 3
    umem, descs = _traffic(n)
    table = _table(n, opts, n_ports)
    size = pow2_at_least(n)
    R = _port_replies(n, n, max_batch, opts, n_ports, 0, SS.ALL_BOUND)
    rooms = [4096, max(R[1] - 1, 0), 0]
    rx, fill, txs, pool = make_state(n_ports, size, WRAP, descs, size // 3, size // 2, 2 * size, rooms)
    a, b = SteerState(rx, fill, txs, pool, max_batch, table), SteerState(rx, fill, txs, pool, max_batch, table)
    ua, ub = to_dev(umem), to_dev(umem)
    a.step(ua, opts, 0)
    g_descs, g_plan, g_verd = Guarded(max_batch * 16), Guarded(32), Guarded(max_batch)
    g_out, g_off, g_room = Guarded(max_batch * 16), Guarded(4 * (n_ports + 1)), Guarded(4 * n_ports)
    g_tx, g_free = Guarded(max_batch * 16), Guarded(max_batch * 8)
    sws = torch.empty(max(X.steer_workspace_size(max_batch, n_ports), 4), dtype=torch.uint8, device=dev)
    ews = torch.empty(max(X.egress_ports_workspace_size(max_batch, n_ports), 4), dtype=torch.uint8, device=dev)
    X.rx_begin_dev(b.rx.view, b.fill.view, b.views[0], b.pool.view, max_batch, g_descs.data, g_plan.data)
    X.rx_prepare_ports_dev(b.views, g_plan.data, g_descs.data, max_batch, g_room.data)
    X.ingress_steer_dev(ub, g_descs.data, max_batch, b.table, b.n_entries, 0, n_ports, None, b.actions.data,
                        b.ports.data, g_out.data, g_off.data, g_verd.data, None, b.stats, sws, opts=opts)
    X.egress_ports_dev(g_out.data, g_verd.data, g_off.data, n_ports, max_batch, g_tx.data, g_free.data, b.counts.data,
                       tx_room=g_room.data, stats=b.stats, port_stats=b.port_stats.data, workspace=ews)
    X.rx_end_ports_dev(b.rx.view, b.views, b.pool.view, g_plan.data, g_descs.data, b.actions.data, g_off.data,
                       g_tx.data, g_free.data, b.counts.data, max_batch, b.ws.data, b.res.data)
    torch.cuda.synchronize()
    want = [a.rx.read(), a.fill.read(), [t.read() for t in a.txs], a.pool.read()]
    b.check(*want)
    after, spec, st, pst, got = spec_after(umem, rx, fill, txs, pool, max_batch, opts, table, 0, None)
    a.check(*spec)
    a.check_outputs(got)
    b.check_outputs(got)
    assert a.result() == b.result() == got["result"] and got["result"]["tx_full"] >= 1
    assert stats_of(a.stats) == stats_of(b.stats) == st and torch.equal(ua, ub)
    assert port_stats_of(a.port_stats, n_ports) == port_stats_of(b.port_stats, n_ports) == pst
    # what prepare leaves: the rooms; the received entries whole, `options` included; the pad behind them
    assert list(g_room.get(np.uint32)) == [t.free() for t in txs]
    d = g_descs.get(oracle.DESC_DTYPE)
    assert (d[:n] == descs[:n]).all() and (descs["options"][:n] != 0).all() and not g_descs.get()[n * 16:].any()
    assert list(g_off.get(np.uint32)) == [int(x) for x in got["off"]]
    assert all(g.intact() for g in (g_descs, g_plan, g_verd, g_out, g_off, g_room, g_tx, g_free))


# ---- the optional outputs ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [64, 1100])
def test_optional_outputs_as_null_and_as_given(n):
    """d_actions, d_ports, d_port_counts and d_port_stats as NULL (carved from the workspace, or left out): the rings,
    the pool, the shared counters, the result and the UMEM are those of the call that was given them."""
    _dev()
    opts, n_ports = 0x17, 3
    umem, descs = _traffic(n)
    table = _table(n, opts, n_ports)
    size = pow2_at_least(n)
    rx, fill, txs, pool = make_state(n_ports, size, 0x12345, descs, size // 2, size // 2, 2 * size, [4096, 3, 4096])
    a, b = SteerState(rx, fill, txs, pool, n, table), SteerState(rx, fill, txs, pool, n, table)
    ua, ub = to_dev(umem), to_dev(umem)
    a.step(ua, opts, SS.PASS, outputs=True)
    b.step(ub, opts, SS.PASS, outputs=False)
    torch.cuda.synchronize()
    b.check(a.rx.read(), a.fill.read(), [t.read() for t in a.txs], a.pool.read())
    assert a.result() == b.result() and a.result()["received"] == n and a.result()["tx_full"] >= 1
    assert stats_of(a.stats) == stats_of(b.stats) and torch.equal(ua, ub)
    for g in (b.actions, b.ports, b.counts):
        assert (g.get() == SENT).all()  # not given: not written
    assert not b.port_stats.get().any() and any(any(s.values()) for s in port_stats_of(a.port_stats, n_ports))
