"""GPU parity of xsk_gpu_rx_fused_loop_dev with xsk_gpu_rx_loop_dev: every case builds one host state and uploads it
twice, runs the loop call on one copy and the fused call on the other, and holds both against the Python spec
(tests/rx_pass_spec.py, then tests/tx_complete_rings_spec.py) and against each other: every ring entry and index word,
the pool's whole array and its count word, every UMEM byte, d_actions and d_ports over all max_batch entries,
d_port_counts, d_stats, d_port_stats, *d_res, d_moved and *d_pushed.  The workspace is the one thing not compared.

The helpers are those of the loop call's own tests (make_state, _traffic, make_stack, LoopState); every array sits
between two runs of the sentinel byte, which must survive.  A list of cases, not a cross product: each names what it is
there for."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
import xsknet_amd as X  # noqa: E402
from tests import egress_ports_spec as EP  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests import rx_dev_spec as RS  # noqa: E402
from tests import rx_pass_spec as PS  # noqa: E402
from tests import steer_spec as SS  # noqa: E402
from tests import stream_paths as S  # noqa: E402
from tests import tx_complete_rings_spec as CS  # noqa: E402
from tests.test_gpu_egress import SENT  # noqa: E402
from tests.test_gpu_ingress import _dev, stats_of, to_dev  # noqa: E402
from tests.test_gpu_rx_pass_step_dev import make_stack  # noqa: E402
from tests.test_gpu_rx_step_dev import WRAP  # noqa: E402
from tests.test_gpu_rx_step_steer_dev import _traffic, make_state, port_stats_of, pow2_at_least  # noqa: E402
from tests.test_gpu_tx_complete_rings import LoopState, make_comps  # noqa: E402


class FusedState(LoopState):
    """LoopState whose loop() is the fused call when `fused` is set; `outputs` False passes every optional output as
    NULL at once."""

    def run(self, fused, d_umem, opts, default_port, complete_max, comps=True, outputs=True):
        fn = X.rx_loop_fused_dev if fused else X.rx_loop_dev
        o = outputs
        fn(d_umem, self.rx.view, self.fill.view, self.views, self.stack_view, self.pool.view, self.max_batch, self.table,
           self.n_entries, default_port, self.comp_views if comps else [], complete_max, self.ws.data, bound=self.bound,
           actions=self.actions.data if o else None, ports=self.ports.data if o else None,
           port_counts=self.counts.data if o else None, stats=self.stats if o else None,
           port_stats=self.port_stats.data if o else None, res=self.res.data if o else None,
           moved=self.moved.data if o else None, pushed=self.pushed.data if o else None, opts=opts)


def _table_of(umem, descs, opts, n_ports, entries, seed):
    return SS.sample_table(SS.destinations(umem, descs, opts), entries, n_ports, seed=seed) if entries else {}


def _long_traffic(n, at, length):
    """n IPv4 echo requests of 64 to 200 B with one of `length` bytes at index `at`; every frame in a slot of its own."""
    frames, addrs, a = [], [], 0
    for i in range(n):
        ln = length if i == at else 64 + (i * 37) % 137
        frames.append(S.frame(False, ln, "random", ln & 0xFFFF, i))
        addrs.append(a + (i % 16))
        a += (16 + ln + 255 + 256) & ~255
    umem, descs = S.place_at(frames, addrs, a + 256, 1)
    return umem, np.ascontiguousarray(descs, oracle.DESC_DTYPE)


# name: n frames on the RX ring, max_batch, ports, table entries, default port, bound mask, opts, index-word start,
# TX rooms (cycled), fill ring's free slots, pool count, pool capacity, stack (size, room) or None, completion rings,
# their fill levels (cycled), complete_max, outputs
ALL = SS.ALL_BOUND
CASES = {
    "empty_rx":        (0, 64, 3, 94, SS.PASS, ALL, 0x17, WRAP, [4096], 20, 30, 400, (16, 16), 4, [3, 0, 9, 16], 4, True),
    "one_frame_mb1":   (1, 1, 1, 1, 0, ALL, 0, 0, [4096], 5, 9, 64, None, 1, [5], 1024, True),
    "three_mb48":      (3, 48, 3, 0, 0, ALL, 0x7, 0x12345, [4096], 20, 30, 400, (8, 8), 4, [1, 2, 3, 4], 1024, True),
    "n63_unbound":     (63, 64, 3, 94, SS.PASS, ALL & ~2, 0x17, WRAP, [4096], 40, 64, 600, (64, 64), 4, [9, 0, 64, 70], 64, True),
    "n64_bound_null":  (64, 64, 64, 94, 5, None, 0x17, WRAP, [4096], 64, 64, 900, (64, 5), 65, [3, 0, 1, 64, 2, 9], 4, True),
    "n65_over_bound":  (65, 64, 3, 1, SS.PASS, ALL, 0x17, 5, [4096], 64, 64, 900, (16, 3), 4, [9, 0, 64, 70], 1024, True),
    "n65_mb48_ref":    (65, 48, 3, 94, 0, ALL, 0, WRAP, [4096], 64, 64, 900, None, 0, [0], 0, True),
    "tx_full_and_cut": (64, 64, 3, 94, 1, ALL, 0x17, WRAP, [0, 2, 4096], 64, 64, 900, (64, 64), 4, [9, 0, 64, 70], 1024, True),
    "pool_dry":        (64, 64, 3, 94, SS.PASS, ALL, 0x17, WRAP, [4096], 40, 0, 900, (64, 64), 4, [9, 0, 64, 70], 1024, True),
    "pool_part":       (64, 64, 3, 94, SS.PASS, ALL, 0x17, WRAP, [0, 0, 0], 0, 120, 128, (64, 0), 4, [9, 3, 64, 70], 1024, True),
    "comp_half":       (48, 48, 3, 94, SS.PASS, ALL, 0x17, WRAP, [4096], 10, 40, 90, (64, 64), 4, [30, 30, 30, 30], 1024, True),
    "stack_absent":    (64, 64, 3, 94, SS.PASS, ALL, 0x17, WRAP, [4096], 64, 64, 900, None, 4, [9, 0, 64, 70], 1024, True),
    "stack_full":      (64, 64, 3, 94, SS.PASS, ALL, 0x7, WRAP, [4096], 64, 64, 900, (16, 0), 1, [7], 4, True),
    "complete_max0":   (64, 64, 3, 94, SS.PASS, ALL, 0x17, WRAP, [4096], 64, 64, 900, (64, 64), 4, [9, 0, 64, 70], 0, True),
    "outputs_null":    (64, 64, 3, 94, SS.PASS, ALL, 0x17, WRAP, [4096, 3], 64, 64, 900, (16, 4), 4, [9, 0, 64, 70], 64, False),
    "n1023_p3":        (1023, 1024, 3, 1024, SS.PASS, ALL, 0x17, WRAP, [4096, 100, 7], 1024, 1024, 6000, (1024, 200), 4, [1300, 5, 0, 1024], 1024, True),
    "n1024_p64":       (1024, 1024, 64, 1024, 7, ALL & ~(1 << 9), 0x17, WRAP, [4096, 3, 0, 64], 600, 700, 9000, (512, 512), 65, [40, 0, 1, 64, 1024, 5], 1024, True),
    "n1024_p1_ref":    (1024, 1024, 1, 94, 0, ALL, 0, 0x12345, [4096], 1024, 1024, 6000, (2048, 2048), 1, [2048], 1024, True),
}


def _build(case):
    (n, max_batch, n_ports, entries, default_port, bound, opts, start, rooms, fill_free, pool_n, cap, stack, n_comp,
     comp_used, complete_max, outputs) = CASES[case]
    umem, descs = _traffic(n)
    table = _table_of(umem, descs, opts, n_ports, entries, seed=n + opts)
    size = pow2_at_least(n)
    rx, fill, txs, pool = make_state(n_ports, size, start, descs, min(fill_free, size), pool_n, cap,
                                     [rooms[p % len(rooms)] for p in range(n_ports)])
    stk = make_stack(stack[0], 0xFFFFFFFE, stack[1]) if stack else None
    comps = make_comps(n_comp, [pow2_at_least(max(comp_used))], comp_used, wrap_all=True) if n_comp else []
    return umem, table, rx, fill, txs, pool, stk, comps


def _run_both(umem, table, rx, fill, txs, pool, stk, comps, max_batch, opts, default_port, bound, complete_max, outputs=True):
    """The loop call on one upload, the fused call on another, the spec on host copies; returns (states, UMEMs, spec)."""
    _dev()
    a = FusedState(rx, fill, txs, stk, pool, max_batch, comps, table, bound)
    b = FusedState(rx, fill, txs, stk, pool, max_batch, comps, table, bound)
    ua, ub = to_dev(umem), to_dev(umem)
    a.run(False, ua, opts, default_port, complete_max, comps=bool(comps), outputs=outputs)
    b.run(True, ub, opts, default_port, complete_max, comps=bool(comps), outputs=outputs)
    torch.cuda.synchronize()
    s = (rx.copy(), fill.copy(), [t.copy() for t in txs], pool.copy(), None if stk is None else stk.copy(),
         [c.copy() for c in comps])
    u, st = umem.copy(), dict.fromkeys(IS.KEYS, 0)
    pst = [dict.fromkeys(EP.STATS_KEYS, 0) for _ in txs]
    got = PS.spec_step_pass(u, s[0], s[1], s[2], s[4], s[3], max_batch, opts, table, default_port,
                            SS.ALL_BOUND if bound is None else bound, st, pst)
    moved, pushed = CS.spec_complete_rings(s[5], s[3], complete_max) if comps else ([], 0)
    return a, b, ua, ub, s, u, st, pst, got, moved, pushed


def _compare(a, b, ua, ub, s, u, st, pst, got, moved, pushed, n_ports, n_comp, outputs=True):
    for d, du in ((a, ua), (b, ub)):
        d.check(s[0], s[1], s[2], s[3], s[4])
        d.check_comps(s[5])
        assert (du.cpu().numpy() == u).all()
        if outputs:
            d.check_outputs(got)
            assert d.result() == got["result"]
            assert stats_of(d.stats) == st and port_stats_of(d.port_stats, n_ports) == pst
            if n_comp:
                assert [int(x) for x in d.moved.get(np.uint32)][:n_comp] == moved
                assert int(d.pushed.get(np.uint32)[0]) == pushed
        assert all(g.intact() for g in d.guards()), "a sentinel was overwritten"
    # the two calls against each other, byte for byte: what the spec's comparison leaves out (the pool above its count,
    # stale ring entries, outputs where nothing is written)
    assert (a.pool.read().addr == b.pool.read().addr).all() and a.pool.read().n_free == b.pool.read().n_free
    for x, y in zip([a.rx, a.fill, *a.txs, *a.comps] + ([a.stack] if a.stack else []),
                    [b.rx, b.fill, *b.txs, *b.comps] + ([b.stack] if b.stack else [])):
        assert torch.equal(x.ent.data, y.ent.data) and torch.equal(x.words.data, y.words.data)
    for x, y in ((a.actions, b.actions), (a.ports, b.ports), (a.counts, b.counts), (a.port_stats, b.port_stats),
                 (a.res, b.res), (a.moved, b.moved), (a.pushed, b.pushed)):
        assert torch.equal(x.data, y.data)
    assert torch.equal(a.stats, b.stats) and torch.equal(ua, ub)


@pytest.mark.parametrize("case", list(CASES))
def test_the_fused_call_leaves_what_the_loop_call_leaves(case):
    (n, max_batch, n_ports, entries, default_port, bound, opts, start, rooms, fill_free, pool_n, cap, stack, n_comp,
     comp_used, complete_max, outputs) = CASES[case]
    umem, table, rx, fill, txs, pool, stk, comps = _build(case)
    r = _run_both(umem, table, rx, fill, txs, pool, stk, comps, max_batch, opts, default_port, bound, complete_max, outputs)
    _compare(*r, n_ports, n_comp, outputs)
    a, b, got = r[0], r[1], r[8]
    res = got["result"]
    assert res["received"] == min(n, max_batch)
    if not outputs:  # nothing was written where nothing was given
        for g in (b.actions, b.ports, b.counts, b.res, b.moved, b.pushed):
            assert bool((g.data == SENT).all())
    if case == "tx_full_and_cut":
        c = got["counts"]
        assert c[0]["n_tx"] == 0 and c[0]["n_tx_full"] >= 1 and c[1]["n_tx"] == 2 and c[1]["n_tx_full"] >= 1
    if case == "pool_dry":
        assert res["refilled"] == 0 and n > 0
    if case == "pool_part":
        assert 0 < res["freed"] == 8 and s_pool_full(r[4][3])
    if case == "comp_half":
        assert 0 < r[10] < sum(r[9])  # the pool took part of what the completion rings held
    if case == "stack_full":
        assert res["passed"] == 0 and res["pass_full"] >= 1
    if case == "complete_max0":
        assert r[9] == [0] * n_comp and r[10] == 0
    if case == "n65_over_bound":
        assert res["received"] == 64 and r[4][0].used() == 1 and res["pass_full"] >= 1
    if n >= 63 and opts == 0x17:  # IPv4 and IPv6 echo requests and PASS traffic in the mix
        acts = got["actions"][:res["received"]]
        assert (acts == SS.XDP_PASS).any() and (acts == SS.XDP_REDIRECT).any()


def s_pool_full(pool):
    return pool.n() == pool.capacity


def test_garbage_in_every_index_word_and_count_word():
    """The totality claim: whatever the words hold, both calls clamp alike and leave what the spec leaves."""
    rng = np.random.default_rng(11)
    for it in range(3):
        n, max_batch, n_ports, opts = 64, 64, 3, 0x17
        umem, descs = _traffic(n)
        table = _table_of(umem, descs, opts, n_ports, 94, seed=it)
        rx, fill, txs, pool = make_state(n_ports, 64, WRAP, descs, 30, 40, 300, [4096, 5, 0])
        stk = make_stack(16, 0xFFFFFFFE, 7)
        comps = make_comps(4, [64], [9, 0, 64, 70], wrap_all=True)
        for r in (rx, fill, *txs, stk, *comps):
            r.prod, r.cons = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
        if it != 1:
            pool.n_free = int(rng.integers(300, 1 << 32))  # above the capacity: a full pool that ends clamped
        r = _run_both(umem, table, rx, fill, txs, pool, stk, comps, max_batch, opts, SS.PASS, SS.ALL_BOUND, 1024)
        _compare(*r, n_ports, 4)
        assert r[4][3].n_free <= r[4][3].capacity


@pytest.mark.parametrize("opts", [0, 0x17])
def test_a_frame_of_70000_bytes_among_short_ones(opts):
    """The long-frame branch of the transform's body inside the fused kernel (a tile that is neither short nor mid)."""
    n, max_batch, n_ports = 20, 64, 3
    umem, descs = _long_traffic(n, 5, 70_000)
    table = {}  # every frame to the default port, whose TX ring holds 2048 entries
    rx, fill, txs, pool = make_state(n_ports, 32, WRAP, descs, 20, 30, 200, [4096] * n_ports)
    stk = make_stack(16, 0xFFFFFFFE, 16)
    comps = make_comps(4, [16], [3, 0, 16, 5], wrap_all=True)
    r = _run_both(umem, table, rx, fill, txs, pool, stk, comps, max_batch, opts, 2, SS.ALL_BOUND, 64)
    _compare(*r, n_ports, 4)
    got, st = r[8], r[6]
    assert got["result"]["received"] == n and got["result"]["redirected"] == n and int(st["rx_bytes"]) >= 70_000
    if opts == 0:  # the reference answers the long frame too (wire mode's rules refuse its IPv4 length field)
        assert got["result"]["replied"] == n and int(st["tx_bytes"]) >= 70_000
