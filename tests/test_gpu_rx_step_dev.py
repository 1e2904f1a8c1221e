"""GPU parity of xsk_gpu_rx_step_dev / xsk_gpu_rx_begin_dev / xsk_gpu_rx_end_dev / xsk_gpu_tx_complete_dev: rings, frame
pool and UMEM in device memory end where the host's xsk_gpu_rx_step() / xsk_gpu_tx_complete() leave host rings from the
same starting state (up to 1024 frames, the host step's bound), and where tests/rx_dev_spec.py plus the oracle put them
(above it).

Common to every case: every ring, index-word pair, pool stack, count word, result and workspace sits between two runs of
the sentinel byte tests.test_gpu_egress.SENT, which must survive; the traffic is oracle.synth_batch(mode=1); the RX
entries carry nonzero `options` (a TX entry must carry 0); the free part of every ring holds stale bytes that must stay
where the step stores nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import egress_spec as ES  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests import rx_dev_spec as RS  # noqa: E402
from tests.test_gpu_egress import SENT  # noqa: E402
from tests.test_gpu_ingress import _dev, stats_of, to_dev  # noqa: E402

STRIDE = 2048
PAD = 64  # sentinel bytes in front of and behind every array (keeps its 16-B alignment)
WRAP = 0xFFFFFFFD


class Guarded:
    """`nbytes` of device memory between two runs of SENT."""

    def __init__(self, nbytes, init=None):
        self.buf = torch.full((PAD + nbytes + PAD,), SENT, dtype=torch.uint8, device=_dev())
        self.data = self.buf[PAD:PAD + nbytes]
        if init is not None:
            self.put(init)

    def put(self, a: np.ndarray):
        self.data.copy_(to_dev(a))  # a device copy on the current stream

    def get(self, dtype=np.uint8) -> np.ndarray:
        return self.data.cpu().numpy().view(dtype)

    def intact(self) -> bool:
        return bool((self.buf[:PAD] == SENT).all()) and bool((self.buf[PAD + self.data.numel():] == SENT).all())


class DevRing:
    """A RingState in device memory: [producer, consumer] and the entries, each guarded."""

    def __init__(self, ring: RS.RingState):
        self.size, self.dtype = ring.size, ring.entries.dtype
        self.words = Guarded(8, np.array([ring.prod, ring.cons], np.uint32))
        self.ent = Guarded(ring.entries.nbytes, ring.entries)
        self.view = X.RingDev.of(self.words.data[0:4], self.words.data[4:8], self.ent.data, ring.size)

    def write(self, ring: RS.RingState):
        self.words.put(np.array([ring.prod, ring.cons], np.uint32))
        self.ent.put(ring.entries)

    def read(self) -> RS.RingState:
        w = self.words.get(np.uint32)
        return RS.RingState(self.ent.get(self.dtype).copy(), int(w[0]), int(w[1]))


class DevPool:
    def __init__(self, pool: RS.PoolState):
        self.addr = Guarded(pool.addr.nbytes, pool.addr)
        self.word = Guarded(4, np.array([pool.n_free], np.uint32))
        self.view = X.PoolDev.of(self.addr.data, self.word.data, pool.capacity)

    def read(self) -> RS.PoolState:
        return RS.PoolState(self.addr.get(np.uint64).copy(), int(self.word.get(np.uint32)[0]))


class DevState:
    """(rx, fill, tx, pool) [+ comp] on the device, with the step's workspace, counters and result."""

    def __init__(self, rx, fill, tx, pool, max_batch, comp=None):
        self.rx, self.fill, self.tx, self.pool = DevRing(rx), DevRing(fill), DevRing(tx), DevPool(pool)
        self.comp = DevRing(comp) if comp is not None else None
        self.max_batch = max_batch
        self.ws = Guarded(X.rx_step_dev_workspace_size(max_batch))
        self.res = Guarded(16)
        self.stats = torch.zeros(40, dtype=torch.uint8, device=_dev())

    def step(self, d_umem, opts, stats=True, res=True):
        X.rx_step_dev(d_umem, self.rx.view, self.fill.view, self.tx.view, self.pool.view, self.max_batch, self.ws.data,
                      stats=self.stats if stats else None, res=self.res.data if res else None, opts=opts)

    def guards(self):
        gs = [self.ws, self.res, self.pool.addr, self.pool.word]
        for r in (self.rx, self.fill, self.tx, self.comp):
            if r is not None:
                gs += [r.words, r.ent]
        return gs

    def result(self) -> dict:
        r = self.res.get(RS.RESULT_DTYPE)[0]
        return {k: int(r[k]) for k in RS.RESULT_DTYPE.names}

    def check(self, rx, fill, tx, pool, comp=None):
        """After a synchronisation: every ring's whole entry array, the index words, the pool's stack below its count
        and the count against the expected states; every sentinel."""
        for name, got, want in (("rx", self.rx, rx), ("fill", self.fill, fill), ("tx", self.tx, tx),
                                ("comp", self.comp, comp)):
            if want is None:
                continue
            g = got.read()
            assert (g.prod, g.cons) == (want.prod, want.cons), (name, g.prod, g.cons, want.prod, want.cons)
            bad = np.nonzero(g.entries != want.entries)[0]
            assert len(bad) == 0, (name, bad[:5], g.entries[bad[:5]], want.entries[bad[:5]])
        p = self.pool.read()
        assert p.n_free == pool.n_free and (p.addr[:p.n()] == pool.addr[:pool.n()]).all(), (p.n_free, pool.n_free)
        assert all(g.intact() for g in self.guards()), "a sentinel was overwritten"


@functools.lru_cache(maxsize=None)
def _traffic(n, seed=0):
    """(UMEM, descriptors) of n mixed frames, frame i inside [i * STRIDE, (i + 1) * STRIDE); nonzero options.  Read-only."""
    umem = np.zeros(max(n, 1) * STRIDE, np.uint8)
    descs = np.ascontiguousarray(
        oracle.synth_batch(umem, n, 0, STRIDE, seed=0x5EED0000 + n + seed, mode=1, len_lo=20, len_hi=1500),
        oracle.DESC_DTYPE)
    descs["options"] = np.arange(n, dtype=np.uint32) + 0x1000
    umem.setflags(write=False)
    descs.setflags(write=False)
    return umem, descs


@functools.lru_cache(maxsize=None)
def _verdicts(n, opts, seed=0):
    umem, descs = _traffic(n, seed)
    v, _, _ = IS.spec_transform(umem.copy(), descs, opts)
    v.setflags(write=False)
    return v


def make_state(size, start, descs, fill_free, pool_n, tx_room, cap=None, comp_used=0):
    """RingStates of `size` entries: `descs` on the RX ring, the fill ring with fill_free free slots, the TX ring with
    tx_room, a completion ring holding comp_used addresses, a pool of pool_n frames (capacity size + 3 by default).
    Index words start near `start`; free slots hold stale nonzero bytes."""
    cap = cap or size + 3
    rng = np.random.default_rng(size * 31 + len(descs))
    rx = RS.RingState(np.zeros(size, oracle.DESC_DTYPE), start, start)
    rx.entries["addr"], rx.entries["len"], rx.entries["options"] = 0xA5A5A5A5, 0xA5A5, 0xDEAD
    rx.produce(descs)
    fill = RS.RingState(rng.integers(1, 1 << 40, size, dtype=np.uint64), start + 1 + size - fill_free, start + 1)
    tx = RS.RingState(np.zeros(size, oracle.DESC_DTYPE), start + 2 + size - tx_room, start + 2)
    tx.entries["addr"] = rng.integers(1, 1 << 40, size, dtype=np.uint64)
    tx.entries["options"] = 0xBEEF
    comp = RS.RingState(rng.integers(1, 1 << 40, size, dtype=np.uint64), start + 3 + comp_used, start + 3)
    pool = RS.PoolState((np.arange(cap, dtype=np.uint64) + np.uint64(1 << 20)) * np.uint64(4096), pool_n)
    return rx, fill, tx, pool, comp


class HostRing:
    """struct xsk_gpu_ring over copies of a RingState's words and entries; the caches refresh on first use."""

    def __init__(self, ring: RS.RingState, consumer: bool):
        self.ctr = np.array([ring.prod, ring.cons], np.uint32)
        self.slots = ring.entries.copy()
        c = ring.cons if consumer else ring.prod
        self.view = X.Ring(c, c, ring.size - 1, ring.size, self.ctr.ctypes.data, self.ctr.ctypes.data + 4,
                           self.slots.ctypes.data, None)

    def state(self) -> RS.RingState:
        return RS.RingState(self.slots.copy(), int(self.ctr[0]), int(self.ctr[1]))


def host_step(umem: np.ndarray, rx, fill, tx, pool, comp, max_batch, opts, complete_max):
    """xsk_gpu_rx_step() on a ZEROCOPY context over an xsk_gpu_umem_alloc UMEM holding `umem`, then
    xsk_gpu_tx_complete(): (UMEM after, the five states after, stats dict, result dict, completed)."""
    hr, hf, ht, hc = HostRing(rx, True), HostRing(fill, False), HostRing(tx, False), HostRing(comp, True)
    stack = pool.addr.copy()
    hp = X.FramePool(stack.ctypes.data, pool.n_free, pool.capacity)
    st = np.zeros(1, X.STATS_DTYPE)
    with X.HugeUmem(umem.nbytes) as hu:
        hu.array[:] = umem
        with X.EchoContext(hu.array, 0, max_batch=1024, mode=X.MODE_ZEROCOPY, opts=opts) as ctx:
            rc, res = ctx.rx_step(hr.view, hf.view, ht.view, hp, max_batch, st)
        after = hu.array.copy()
    moved = int(X.lib().xsk_gpu_tx_complete(C.byref(hc.view), C.byref(hp), complete_max)) if complete_max else 0
    assert rc == res.received
    return (after, (hr.state(), hf.state(), ht.state(), RS.PoolState(stack, hp.n_free), hc.state()),
            {k: int(st[0][k]) for k in IS.KEYS},
            dict(received=res.received, replied=res.replied, tx_full=res.tx_full, refilled=res.refilled), moved)


# ---- parity with the host step -----------------------------------------------------------------------------------

@pytest.mark.parametrize("opts", [0, 0x17])
@pytest.mark.parametrize("start", [0, 0x12345, WRAP])
@pytest.mark.parametrize("n,size", [(1, 8), (64, 64), (65, 128), (1024, 2048)])
def test_parity_with_the_host_step(n, size, start, opts):
    """The same UMEM, rings and pool on both sides; after the step (and a tx_complete over a completion ring of a few
    entries): every ring's entries, all eight index words, the pool, the counters, the result, every UMEM byte.  Once
    with room for every reply and once with the TX ring cut below R."""
    _dev()
    umem, descs = _traffic(n)
    v = _verdicts(n, opts)
    R = int((v == 0).sum())
    if n >= 64:
        assert R >= 3 and n - R >= 3  # a condition of the input: a mixed batch
    mid = start + size // 2 if start == 0x12345 else start
    for tx_room in (size, max(R - 2, 0)):
        if tx_room < size and n >= 64:
            assert 0 < tx_room < R  # the cut room really lies below R
        rx, fill, tx, pool, comp = make_state(size, mid, descs, fill_free=size // 2, pool_n=size // 2 + 2,
                                              tx_room=tx_room, comp_used=min(5, size))
        after, want, st, res, moved = host_step(umem, rx, fill, tx, pool, comp, 1024, opts, 4)
        assert res["received"] == n and res["replied"] == min(R, tx_room) and res["tx_full"] == R - res["replied"]
        d = DevState(rx, fill, tx, pool, min(max(n, 1), 1024), comp)
        d_umem = to_dev(umem)
        d_moved = Guarded(4)
        d.step(d_umem, opts)
        X.tx_complete_dev(d.comp.view, d.pool.view, 4, d_moved.data)
        torch.cuda.synchronize()
        d.check(*want[:4], comp=want[4])
        assert stats_of(d.stats) == st
        assert d.result() == res
        assert int(d_moved.get(np.uint32)[0]) == moved == 4 and d_moved.intact()
        assert (d_umem.cpu().numpy() == after).all(), "UMEM differs from the host step's"


# ---- above the host step's bound: the spec and the oracle ----------------------------------------------------------

def spec_after(umem, rx, fill, tx, pool, max_batch, opts):
    """tests/rx_dev_spec.spec_step on copies: (UMEM after, states after, stats, result)."""
    s = tuple(x.copy() for x in (rx, fill, tx, pool))
    u = umem.copy()
    st = dict.fromkeys(IS.KEYS, 0)
    res = RS.spec_step(u, *s, max_batch, opts, st)
    return u, s, st, res


@pytest.mark.parametrize("opts", [0, 0x17])
@pytest.mark.parametrize("n,max_batch", [(1025, 1025), (1300, 1300), (1300, 1100)])
def test_above_1024_frames_against_the_spec(n, max_batch, opts):
    """The path of kernel boundaries (ring 2048, wrap start): all frames taken, and a bound below what the ring holds."""
    _dev()
    umem, descs = _traffic(n)
    k = min(n, max_batch)
    R = int((_verdicts(n, opts)[:k] == 0).sum())
    for tx_room, fill_free, pool_n in ((2048, 2048, 2051), (R - 1, 700, 2000), (R + 1, 1, 0)):
        rx, fill, tx, pool, _ = make_state(2048, WRAP - 1000, descs, fill_free, pool_n, tx_room)
        after, want, st, res = spec_after(umem, rx, fill, tx, pool, max_batch, opts)
        assert res["received"] == k and res["replied"] == min(R, tx_room)
        d = DevState(rx, fill, tx, pool, max_batch)
        d_umem = to_dev(umem)
        d.step(d_umem, opts)
        torch.cuda.synchronize()
        d.check(*want)
        assert stats_of(d.stats) == st and d.result() == res
        assert (d_umem.cpu().numpy() == after).all()


# ---- consecutive steps -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_batch,size", [(48, 64), (1100, 2048)])
def test_three_consecutive_steps_cross_the_rings_end(max_batch, size):
    """Three steps on one device state, the RX ring refilled and the TX ring drained by device copies in between; the
    slots wrap past the ring's end and the index words past 2^32."""
    _dev()
    per = max_batch - 5
    umem, descs = _traffic(3 * per)
    rx, fill, tx, pool, _ = make_state(size, WRAP - per, descs[:per], size // 2, size, size)
    d = DevState(rx, fill, tx, pool, max_batch)
    d_umem = to_dev(umem)
    s = [x.copy() for x in (rx, fill, tx, pool)]
    u = umem.copy()
    st = dict.fromkeys(IS.KEYS, 0)
    for k in range(3):
        if k:  # the peer: new RX entries, the TX ring consumed, the fill ring consumed
            s[0].produce(descs[k * per:(k + 1) * per])
            s[2].cons = s[2].prod
            s[1].cons = (s[1].cons + per) & RS.M32
            d.rx.write(s[0])
            d.tx.write(s[2])
            d.fill.write(s[1])
        res = RS.spec_step(u, *s, max_batch, 0x17, st)
        assert res["received"] == per
        d.step(d_umem, 0x17)
        torch.cuda.synchronize()
        d.check(*s)
        assert d.result() == res and stats_of(d.stats) == st
    assert s[0].cons < per * 3 and (d_umem.cpu().numpy() == u).all()  # the words wrapped


# ---- rooms and pool limits ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,size,max_batch", [(64, 64, 64), (1300, 2048, 1300)])
def test_rooms_and_pool_limits(n, size, max_batch):
    """Fill ring full / one free / all free; pool empty / one / full / capacity - 1; TX room 0 / R - 1 / R / R + 1 /
    unlimited.  The UMEM does not depend on any of them: compared once."""
    _dev()
    umem, descs = _traffic(n)
    R = int((_verdicts(n, 0) == 0).sum())
    cap = size + 3
    d_umem0 = to_dev(umem)
    combos = [(ff, pn, room) for ff in (0, 1, size) for pn in (0, 1, cap, cap - 1)
              for room in (0, R - 1, R, R + 1, size)]
    if n > 1024:
        combos = combos[::7]
    first = True
    for ff, pn, room in combos:
        rx, fill, tx, pool, _ = make_state(size, WRAP, descs, ff, pn, room)
        after, want, st, res = spec_after(umem, rx, fill, tx, pool, max_batch, 0)
        d = DevState(rx, fill, tx, pool, max_batch)
        d_umem = d_umem0.clone()
        d.step(d_umem, 0)
        torch.cuda.synchronize()
        d.check(*want)
        assert stats_of(d.stats) == st and d.result() == res, (ff, pn, room)
        assert res["refilled"] == min(ff, pn) and res["replied"] == min(R, room)
        if first:
            assert (d_umem.cpu().numpy() == after).all()
            first = False


@pytest.mark.parametrize("max_batch", [64, 1300])
def test_garbage_words(max_batch):
    """used > size on every ring and a pool count above the capacity: the result is the spec's, nothing lands outside."""
    _dev()
    umem, descs = _traffic(64)
    rx, fill, tx, pool, comp = make_state(64, 7, descs, 10, 20, 30, comp_used=9)
    rx.prod = (rx.cons + 0x70000000) & RS.M32      # reads as a full ring: 64 entries, the frames above
    fill.cons = (fill.prod + 12345) & RS.M32       # used > size: no room
    tx.prod = (tx.cons + 0x80000005) & RS.M32      # used > size: no room
    comp.prod = (comp.cons - 1) & RS.M32           # used = 2^32 - 1: a full ring
    pool.n_free = 0xFFFFFFF0                       # a full pool
    after, want, st, res = spec_after(umem, rx, fill, tx, pool, max_batch, 0)
    assert res == dict(received=64, replied=0, tx_full=int((_verdicts(64, 0) == 0).sum()), refilled=0)
    assert want[3].n_free == pool.capacity
    cw, pw = comp.copy(), want[3].copy()
    assert RS.spec_complete(cw, pw, max_batch) == 64
    d = DevState(rx, fill, tx, pool, max_batch, comp)
    d_umem = to_dev(umem)
    d_moved = Guarded(4)
    d.step(d_umem, 0)
    X.tx_complete_dev(d.comp.view, d.pool.view, max_batch, d_moved.data)
    torch.cuda.synchronize()
    d.check(want[0], want[1], want[2], pw, comp=cw)
    assert d.result() == res and stats_of(d.stats) == st and int(d_moved.get(np.uint32)[0]) == 64


# ---- the empty RX ring -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_batch", [64, 1300])
def test_an_empty_rx_ring_leaves_every_byte_untouched(max_batch):
    _dev()
    umem, descs = _traffic(64)
    rx, fill, tx, pool, comp = make_state(64, WRAP, descs[:0], 64, 67, 64)
    d = DevState(rx, fill, tx, pool, max_batch)
    d_umem = to_dev(umem)
    d.stats.fill_(SENT)
    torch.cuda.synchronize()
    before = [g.buf.clone() for g in d.guards() if g not in (d.ws, d.res)]
    d.step(d_umem, 0x17)
    torch.cuda.synchronize()
    after = [g.buf for g in d.guards() if g not in (d.ws, d.res)]
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert bool((d.stats == SENT).all()) and torch.equal(d_umem, to_dev(umem))
    assert d.result() == dict(received=0, replied=0, tx_full=0, refilled=0) and d.res.intact() and d.ws.intact()
    plan = d.ws.get()[:32].view(RS.PLAN_DTYPE)[0]
    assert (int(plan["received"]), int(plan["refilled"]), int(plan["tx_room"]), int(plan["pool_n"])) == (0, 0, 64, 67)
    assert (int(plan["rx_cons"]), int(plan["fq_prod"])) == (rx.cons, fill.prod)


# ---- begin, the existing calls and end by hand -------------------------------------------------------------------

@pytest.mark.parametrize("n,size,max_batch", [(65, 128, 100), (1300, 2048, 1300)])
def test_composed_by_hand_equals_the_wrapper(n, size, max_batch):
    _dev()
    dev = _dev()
    opts = 0x17
    umem, descs = _traffic(n)
    R = int((_verdicts(n, opts)[:min(n, max_batch)] == 0).sum())
    rx, fill, tx, pool, _ = make_state(size, WRAP, descs, size // 3, size // 2, R - 1)
    a, b = DevState(rx, fill, tx, pool, max_batch), DevState(rx, fill, tx, pool, max_batch)
    ua, ub = to_dev(umem), to_dev(umem)
    a.step(ua, opts)
    g_descs, g_plan, g_verd = Guarded(max_batch * 16), Guarded(32), Guarded(max_batch)
    g_tx, g_free, g_counts = Guarded(max_batch * 16), Guarded(max_batch * 8), Guarded(16)
    ews = torch.empty(max(X.egress_workspace_size(max_batch), 4), dtype=torch.uint8, device=dev)
    X.rx_begin_dev(b.rx.view, b.fill.view, b.tx.view, b.pool.view, max_batch, g_descs.data, g_plan.data)
    received, tx_room = g_plan.data[0:4], g_plan.data[4:8]
    X.echo_dev_indirect(ub, g_descs.data, received, max_batch, g_verd.data, None, b.stats, opts=opts)
    X.egress_dev(g_descs.data, g_verd.data, max_batch, g_tx.data, g_free.data, g_counts.data, count=received,
                 tx_room=tx_room, stats=b.stats, workspace=ews)
    X.rx_end_dev(b.rx.view, b.tx.view, b.pool.view, g_plan.data, g_tx.data, g_free.data, g_counts.data, max_batch,
                 b.res.data)
    torch.cuda.synchronize()
    want = [x.read() for x in (a.rx, a.fill, a.tx)] + [a.pool.read()]
    b.check(*want)
    after, spec, st, res = spec_after(umem, rx, fill, tx, pool, max_batch, opts)
    a.check(*spec)
    assert a.result() == b.result() == res and res["tx_full"] == 1
    assert stats_of(a.stats) == stats_of(b.stats) == st and torch.equal(ua, ub)
    # what begin leaves: the whole RX entries, `options` included; the plan; nothing behind the count
    k = min(n, max_batch)
    got = g_descs.get(oracle.DESC_DTYPE)
    assert (got[:k] == descs[:k]).all() and (descs["options"][:k] != 0).all()
    assert (g_descs.get()[k * 16:] == SENT).all() and (g_verd.get()[k:] == SENT).all()
    plan = g_plan.get(RS.PLAN_DTYPE)[0]
    assert int(plan["received"]) == k and int(plan["tx_room"]) == R - 1 and int(plan["refilled"]) == size // 3
    assert (int(plan["rx_cons"]), int(plan["fq_prod"]), int(plan["pool_n"])) == (rx.cons, fill.prod, size // 2)
    assert (plan["reserved"] == 0).all()
    assert ES.counts_of(g_counts.get()) == dict(n=k, n_tx=R - 1, n_tx_full=1, n_free=k - R + 1)
    assert all(g.intact() for g in (g_descs, g_plan, g_verd, g_tx, g_free, g_counts))


# ---- tx_complete_dev ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("start", [0, WRAP])
@pytest.mark.parametrize("size,used,pool_n,mx", [(8, 0, 3, 4), (8, 8, 0, 8), (64, 40, 60, 64), (2048, 2048, 100, 1024),
                                                 (2048, 1500, 700, 1025), (2048, 2048, 2051, 5000), (64, 30, 5, 0)])
def test_tx_complete_dev_against_the_host_function(size, used, pool_n, mx, start):
    """Both paths (max up to 1024: one launch; above: copy grid and publish), a pool that takes all, some and none of
    the entries, max == 0 (a memset of *d_moved and no launch)."""
    _dev()
    rx, fill, tx, pool, comp = make_state(size, start, np.zeros(0, oracle.DESC_DTYPE), 0, pool_n, size, comp_used=used)
    hc = HostRing(comp, True)
    stack = pool.addr.copy()
    hp = X.FramePool(stack.ctypes.data, pool.n_free, pool.capacity)
    moved = int(X.lib().xsk_gpu_tx_complete(C.byref(hc.view), C.byref(hp), mx))
    assert moved == min(used, mx)
    dc, dp, d_moved = DevRing(comp), DevPool(pool), Guarded(4)
    X.tx_complete_dev(dc.view, dp.view, mx, d_moved.data)
    X.tx_complete_dev(dc.view, dp.view, 0, None)  # nothing at all
    torch.cuda.synchronize()
    g, w = dc.read(), hc.state()
    assert (g.prod, g.cons) == (w.prod, w.cons) and (g.entries == w.entries).all()
    p = dp.read()
    assert p.n_free == hp.n_free and (p.addr[:p.n()] == stack[:hp.n_free]).all()
    assert int(d_moved.get(np.uint32)[0]) == moved
    assert all(x.intact() for x in (dc.words, dc.ent, dp.addr, dp.word, d_moved))
