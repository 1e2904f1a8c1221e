"""GPU parity of xsk_gpu_tx_complete_rings_dev / xsk_gpu_rx_loop_dev: up to 65 completion rings and one pool in device
memory; after the call they hold what tests/tx_complete_rings_spec.py leaves from the same state, and what a second copy
of the state holds after xsk_gpu_tx_complete_dev() was called for ring 0, 1, ... in turn on the device (the identity of
include/xsk_gpu.h).  The loop call against xsk_gpu_rx_pass_step_dev() followed by the completion call by hand, and with
no completion ring against the step alone.

Common to every case (the helpers are tests/test_gpu_rx_step_dev.py's): every ring, index-word pair, pool stack, count
word and output sits between two runs of the sentinel byte SENT, which must survive; the part of every ring that holds
no completion carries stale nonzero addresses, and the pool above its count stale entries that must stay where the call
stores nothing."""
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
from tests.test_gpu_egress import SENT  # noqa: E402
from tests.test_gpu_ingress import _dev, stats_of, to_dev  # noqa: E402
from tests.test_gpu_rx_pass_step_dev import PassState, make_stack  # noqa: E402
from tests.test_gpu_rx_step_dev import WRAP, DevPool, DevRing, Guarded  # noqa: E402
from tests.test_gpu_rx_step_steer_dev import _table, _traffic, make_state, port_stats_of, pow2_at_least  # noqa: E402


def make_comps(n_rings, sizes, useds, wrap_all=False):
    """Completion rings with sizes and fill levels cycled (a level above the size is a full ring); the consumer word of
    every second ring (of every ring with wrap_all) is three below 2^32.  Every entry is a distinct nonzero address."""
    comps = []
    for q in range(n_rings):
        size = sizes[q % len(sizes)]
        used = min(useds[q % len(useds)], size)
        cons = WRAP if wrap_all or q % 2 == 0 else 0x12345 + 11 * q
        comps.append(RS.RingState((np.arange(size, dtype=np.uint64) + np.uint64(1 + (q << 12))) * np.uint64(2048),
                                  cons + used, cons))
    return comps


def make_pool(room, below=5):
    """A pool with `below` frames on it and `room` free entries holding stale addresses."""
    cap = max(below + room, 1)
    return RS.PoolState((np.arange(cap, dtype=np.uint64) + np.uint64(1 << 30)) * np.uint64(4096), min(below, cap))


class CompState:
    """Completion rings and a pool on the device, with the two outputs (SENT where nothing was written)."""

    def __init__(self, comps, pool):
        self.comps, self.pool = [DevRing(c) for c in comps], DevPool(pool)
        self.views = [c.view for c in self.comps]
        self.moved, self.pushed = Guarded(4 * len(comps)), Guarded(4)

    def call(self, mx, moved=True, pushed=True):
        X.tx_complete_rings_dev(self.views, self.pool.view, mx, moved=self.moved.data if moved else None,
                                pushed=self.pushed.data if pushed else None)

    def singles(self, mx, moved=True):
        for q, v in enumerate(self.views):
            X.tx_complete_dev(v, self.pool.view, mx, moved=self.moved.data[4 * q:4 * q + 4] if moved else None)

    def guards(self):
        gs = [self.moved, self.pushed, self.pool.addr, self.pool.word]
        for c in self.comps:
            gs += [c.words, c.ent]
        return gs

    def check(self, comps, pool):
        """After a synchronisation: every ring's whole entry array and words, the pool's whole array (what lies above the
        count included: the expected state carries the stale entries the call must leave) and count; every sentinel."""
        for q, (got, want) in enumerate(zip(self.comps, comps)):
            g = got.read()
            assert (g.prod, g.cons) == (want.prod, want.cons), (q, g.prod, g.cons, want.prod, want.cons)
            assert (g.entries == want.entries).all(), q
        p = self.pool.read()
        assert p.n_free == pool.n_free, (p.n_free, pool.n_free)
        bad = np.nonzero(p.addr != pool.addr)[0]
        assert len(bad) == 0, (bad[:5], p.addr[bad[:5]], pool.addr[bad[:5]])
        assert all(g.intact() for g in self.guards()), "a sentinel was overwritten"

    def moved_words(self):
        return [int(x) for x in self.moved.get(np.uint32)]

    def pushed_word(self):
        return int(self.pushed.get(np.uint32)[0])


def cut_room(n, cut):
    """The pool's room for a list of n_q: all, none, a cut strictly inside a ring in the list's second half, or exactly
    on a ring boundary there."""
    total, half = sum(n), len(n) // 2
    if cut == "all":
        return total + 7
    if cut == "none":
        return 0
    if cut == "inside":
        q = next(q for q in list(range(half, len(n))) + list(range(half)) if n[q] >= 2)
        return sum(n[:q]) + max(n[q] // 2, 1)
    q = next(q for q in list(range(half, len(n) - 1)) + list(range(half)) if n[q] and sum(n[q + 1:]))
    return sum(n[:q + 1])


# sizes and fill levels (cycled over the rings; a level above the size: full) per max: empty, one, partial and full rings
# in one call; for the larger path rings of 2048 entries with 1300 and more used
SHAPES = {4: ([8, 16, 1, 64, 4], [3, 0, 1, 64, 2, 9]),
          1024: ([2048, 16, 1, 64, 1024], [1300, 0, 1, 64, 1024, 5]),
          1300: ([2048, 8, 1, 2048], [1300, 0, 1, 2048, 1299])}
CASES = [(r, m, c) for r in (1, 3, 64, 65) for m in (4, 1024, 1300) for c in ("all", "inside", "boundary", "none")
         if not (r == 1 and c == "boundary")]  # (one ring has no boundary with anything behind it)


@pytest.mark.parametrize("n_rings,mx,cut", CASES)
def test_against_the_spec_and_against_the_single_ring_calls(n_rings, mx, cut):
    """max 4 and 1024 the one-workgroup path, 1300 the copy grid and the publish launch."""
    _dev()
    sizes, useds = SHAPES[mx]
    comps = make_comps(n_rings, sizes, useds)
    n = [min(c.used(), mx) for c in comps]
    pool = make_pool(cut_room(n, cut))
    want, wp = [c.copy() for c in comps], pool.copy()
    moved, pushed = CS.spec_complete_rings_prefix(want, wp, mx)
    # conditions of the input: a case cannot pass empty-handed
    assert moved == n and sum(n) >= 2 and (mx != 1300 or max(n) == 1300)
    if n_rings > 1:
        assert 0 in n and 1 in n and any(c.used() == c.size for c in comps) and any(1 < c.used() < c.size for c in comps)
    if cut in ("inside", "boundary"):
        A = np.cumsum([0] + n)
        assert 0 < pushed < sum(n) and (pushed in A) == (cut == "boundary")
    else:
        assert pushed == (sum(n) if cut == "all" else 0)
    a, b = CompState(comps, pool), CompState(comps, pool)
    a.call(mx)
    b.singles(mx)
    torch.cuda.synchronize()
    a.check(want, wp)
    b.check(want, wp)  # the identity: ring after ring on the device
    assert a.moved_words() == b.moved_words() == moved and a.pushed_word() == pushed
    assert any(c.cons < 0x1000 for c in want)  # a consumer word wrapped past 2^32


@pytest.mark.parametrize("mx", [4, 1300])
@pytest.mark.parametrize("moved,pushed", [(True, False), (False, True), (False, False)])
def test_the_outputs_may_be_null(mx, moved, pushed):
    _dev()
    comps = make_comps(3, *SHAPES[mx], wrap_all=True)
    n = [min(c.used(), mx) for c in comps]
    pool = make_pool(cut_room(n, "inside"))
    want, wp = [c.copy() for c in comps], pool.copy()
    w_moved, w_pushed = CS.spec_complete_rings(want, wp, mx)
    a, b = CompState(comps, pool), CompState(comps, pool)
    a.call(mx, moved, pushed)
    b.singles(mx, moved)
    torch.cuda.synchronize()
    a.check(want, wp)
    b.check(want, wp)
    assert a.moved_words() == b.moved_words() == (w_moved if moved else [SENT * 0x01010101] * 3)
    assert a.pushed_word() == (w_pushed if pushed else SENT * 0x01010101) and 0 < w_pushed < sum(n)


@pytest.mark.parametrize("n_rings", [1, 65])
def test_max_zero_launches_nothing_and_zeroes_the_outputs(n_rings):
    _dev()
    comps = make_comps(n_rings, [8, 64], [3, 64, 0])
    pool = make_pool(100)
    pool.n_free = pool.capacity + 9  # stays: no word is stored
    for moved, pushed in ((True, True), (False, False)):
        a = CompState(comps, pool)
        a.call(0, moved, pushed)
        torch.cuda.synchronize()
        a.check(comps, pool)
        assert a.moved_words() == [0 if moved else SENT * 0x01010101] * n_rings
        assert a.pushed_word() == (0 if pushed else SENT * 0x01010101)


@pytest.mark.parametrize("mx", [1024, 1300])
def test_garbage_words(mx):
    """prod - cons above the size reads as a full ring, a count word above the capacity as a full pool that ends
    clamped; then random words in every ring against a pool with room for part."""
    _dev()
    rng = np.random.default_rng(mx)
    for it in range(3):
        comps = make_comps(65, [1, 2, 32, 2048, 128], [0, 1, 7, 2048])
        for c in comps:
            if it == 0:
                c.prod = (c.cons + 0x80000005) & RS.M32
            elif it == 2:
                c.prod, c.cons = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
        pool = make_pool(0 if it == 0 else 3000, below=4)
        if it != 1:
            pool.n_free = int(rng.integers(pool.capacity + 1, 1 << 32))
        want, wp = [c.copy() for c in comps], pool.copy()
        moved, pushed = CS.spec_complete_rings_prefix(want, wp, mx)
        a, b = CompState(comps, pool), CompState(comps, pool)
        a.call(mx)
        b.singles(mx)
        torch.cuda.synchronize()
        a.check(want, wp)
        b.check(want, wp)
        assert a.moved_words() == b.moved_words() == moved and a.pushed_word() == pushed
        assert wp.n_free <= wp.capacity and (it == 1 or pushed == 0) and (it != 1 or 0 < pushed < sum(moved))


# ---- the loop call ---------------------------------------------------------------------------------------------------

class LoopState(PassState):
    """PassState with completion rings (one per port and the stack consumer's) and the completion call's outputs."""

    def __init__(self, rx, fill, txs, stack, pool, max_batch, comps, table=None, bound=None):
        super().__init__(rx, fill, txs, stack, pool, max_batch, table, bound)
        self.comps = [DevRing(c) for c in comps]
        self.comp_views = [c.view for c in self.comps]
        self.moved, self.pushed = Guarded(4 * max(len(comps), 1)), Guarded(4)

    def loop(self, d_umem, opts, default_port, complete_max, comps=True):
        X.rx_loop_dev(d_umem, self.rx.view, self.fill.view, self.views, self.stack_view, self.pool.view, self.max_batch,
                      self.table, self.n_entries, default_port, self.comp_views if comps else [], complete_max,
                      self.ws.data, bound=self.bound, actions=self.actions.data, ports=self.ports.data,
                      port_counts=self.counts.data, stats=self.stats, port_stats=self.port_stats.data, res=self.res.data,
                      moved=self.moved.data, pushed=self.pushed.data, opts=opts)

    def complete(self, complete_max):
        X.tx_complete_rings_dev(self.comp_views, self.pool.view, complete_max, moved=self.moved.data,
                                pushed=self.pushed.data)

    def guards(self):
        gs = super().guards() + [self.moved, self.pushed]
        for c in self.comps:
            gs += [c.words, c.ent]
        return gs

    def check_comps(self, comps):
        for q, (got, want) in enumerate(zip(self.comps, comps)):
            g = got.read()
            assert (g.prod, g.cons) == (want.prod, want.cons) and (g.entries == want.entries).all(), q


def _loop_case(n, max_batch, comp_used):
    opts, n_ports = 0x17, 3
    umem, descs = _traffic(n)
    table = _table(n, opts, n_ports)
    size = pow2_at_least(n)
    rx, fill, txs, pool = make_state(n_ports, size, WRAP, descs, size // 3, size // 2, 4 * size, [4096, 4096, 0])
    stack = make_stack(size, 0xFFFFFFFE, 6)
    comps = make_comps(n_ports + 1, [pow2_at_least(max(comp_used))], comp_used, wrap_all=True)
    return opts, n_ports, umem, table, rx, fill, txs, pool, stack, comps


@pytest.mark.parametrize("n,max_batch,complete_max,comp_used", [(65, 100, 64, [9, 0, 64, 70]), (1300, 1310, 1300, [1300, 5, 0, 2048])])
def test_the_two_calls_by_hand_equal_the_loop_call(n, max_batch, complete_max, comp_used):
    _dev()
    opts, n_ports, umem, table, rx, fill, txs, pool, stack, comps = _loop_case(n, max_batch, comp_used)
    a = LoopState(rx, fill, txs, stack, pool, max_batch, comps, table)
    b = LoopState(rx, fill, txs, stack, pool, max_batch, comps, table)
    ua, ub = to_dev(umem), to_dev(umem)
    a.loop(ua, opts, SS.PASS, complete_max)
    b.step(ub, opts, SS.PASS)
    b.complete(complete_max)
    torch.cuda.synchronize()
    # the spec: the step, then the completion rings
    s = (rx.copy(), fill.copy(), [t.copy() for t in txs], pool.copy(), stack.copy(), [c.copy() for c in comps])
    u, st = umem.copy(), dict.fromkeys(IS.KEYS, 0)
    pst = [dict.fromkeys(EP.STATS_KEYS, 0) for _ in txs]
    got = PS.spec_step_pass(u, s[0], s[1], s[2], s[4], s[3], max_batch, opts, table, SS.PASS, SS.ALL_BOUND, st, pst)
    moved, pushed = CS.spec_complete_rings(s[5], s[3], complete_max)
    assert moved == [min(x, complete_max) for x in (c.used() for c in comps)] and pushed == sum(moved)
    for d, du in ((a, ua), (b, ub)):
        d.check(s[0], s[1], s[2], s[3], s[4])
        d.check_comps(s[5])
        d.check_outputs(got)
        assert d.result() == got["result"] and got["result"]["received"] == n and got["result"]["freed"] >= 1
        assert stats_of(d.stats) == st and port_stats_of(d.port_stats, n_ports) == pst
        assert [int(x) for x in d.moved.get(np.uint32)] == moved and int(d.pushed.get(np.uint32)[0]) == pushed
        assert (du.cpu().numpy() == u).all()


@pytest.mark.parametrize("n,max_batch", [(65, 100), (1300, 1310)])
def test_the_loop_call_without_completion_rings_is_the_step(n, max_batch):
    """n_comp == 0: comp, complete_max and the outputs are ignored (the outputs keep their bytes)."""
    _dev()
    opts, n_ports, umem, table, rx, fill, txs, pool, stack, comps = _loop_case(n, max_batch, [9, 0, 64, 70])
    a = LoopState(rx, fill, txs, stack, pool, max_batch, comps, table)
    b = PassState(rx, fill, txs, stack, pool, max_batch, table)
    ua, ub = to_dev(umem), to_dev(umem)
    a.loop(ua, opts, SS.PASS, 0xFFFFFFFF, comps=False)
    b.step(ub, opts, SS.PASS)
    torch.cuda.synchronize()
    a.check(b.rx.read(), b.fill.read(), [t.read() for t in b.txs], b.pool.read(), b.stack.read())
    a.check_comps(comps)
    assert a.result() == b.result() and a.result()["received"] == n
    assert stats_of(a.stats) == stats_of(b.stats) and torch.equal(ua, ub)
    assert port_stats_of(a.port_stats, n_ports) == port_stats_of(b.port_stats, n_ports)
    for x, y in ((a.actions, b.actions), (a.ports, b.ports), (a.counts, b.counts)):
        assert (x.get() == y.get()).all()
    assert bool((a.moved.data == SENT).all()) and bool((a.pushed.data == SENT).all())
