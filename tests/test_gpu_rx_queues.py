"""GPU identity of xsk_gpu_rx_queues_dev with xsk_gpu_rx_fused_loop_dev called once per queue: every test builds Q host
states and uploads each twice; leg A makes Q fused calls in ascending order, leg B prepares one block over its copies,
uploads it and makes ONE rx_queues_dev call.  Per queue both legs are then held against the Python spec
(tests/rx_pass_spec.py, then tests/tx_complete_rings_spec.py) and against each other byte for byte, as
tests/test_gpu_rx_loop_fused.py's _compare does: every ring entry and index word, the pool's whole array and its count
word, every UMEM byte, d_actions and d_ports over all max_batch entries, d_port_counts, d_stats, d_port_stats, *d_res,
d_moved and *d_pushed, and every sentinel around every array.  The workspaces are the one thing not compared.  Nothing
here has a tolerance.

The states, cases and helpers are those of the fused call's own tests."""
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
from tests.test_gpu_ingress import _dev, to_dev  # noqa: E402
from tests.test_gpu_rx_loop_fused import CASES, FusedState, _build, _compare, _table_of  # noqa: E402
from tests.test_gpu_rx_pass_step_dev import make_stack  # noqa: E402
from tests.test_gpu_rx_step_dev import WRAP  # noqa: E402
from tests.test_gpu_rx_step_steer_dev import _traffic, make_state  # noqa: E402
from tests.test_gpu_tx_complete_rings import make_comps  # noqa: E402


class Queue:
    """One queue's host state and the arguments that are not state.  Queues given the same `share` key name ONE UMEM
    (one device copy a leg, one array for the spec); every other queue has copies of its own."""

    def __init__(self, umem, table, rx, fill, txs, pool, stk, comps, max_batch, default_port, bound, complete_max,
                 outputs=True, share=None):
        self.key = ("own", id(self)) if share is None else ("shared", share)
        self.umem, self.table, self.rx, self.fill, self.txs, self.pool, self.stk, self.comps = (
            umem, table, rx, fill, txs, pool, stk, comps)
        self.max_batch, self.default_port, self.bound, self.complete_max, self.outputs = (
            max_batch, default_port, bound, complete_max, outputs)

    def state(self):
        return FusedState(self.rx, self.fill, self.txs, self.stk, self.pool, self.max_batch, self.comps, self.table,
                          self.bound)

    def fused(self, d, d_umem, opts):
        d.run(True, d_umem, opts, self.default_port, self.complete_max, comps=bool(self.comps), outputs=self.outputs)

    def record(self, d, d_umem):
        """The struct xsk_gpu_rx_queue of the arguments fused() passes."""
        o = self.outputs
        return X.rx_queue(d_umem, d.rx.view, d.fill.view, d.views, d.stack_view, d.pool.view, d.max_batch, d.table,
                          d.n_entries, self.default_port, d.comp_views if self.comps else [], self.complete_max, d.ws.data,
                          bound=d.bound, actions=d.actions.data if o else None, ports=d.ports.data if o else None,
                          port_counts=d.counts.data if o else None, stats=d.stats if o else None,
                          port_stats=d.port_stats.data if o else None, res=d.res.data if o else None,
                          moved=d.moved.data if o else None, pushed=d.pushed.data if o else None)

    def spec(self, u, opts):
        """The spec on copies of the state and on `u` (this queue's UMEM copy, or the one it shares), in place."""
        s = (self.rx.copy(), self.fill.copy(), [t.copy() for t in self.txs], self.pool.copy(),
             None if self.stk is None else self.stk.copy(), [c.copy() for c in self.comps])
        st = dict.fromkeys(IS.KEYS, 0)
        pst = [dict.fromkeys(EP.STATS_KEYS, 0) for _ in self.txs]
        got = PS.spec_step_pass(u, s[0], s[1], s[2], s[4], s[3], self.max_batch, opts, self.table, self.default_port,
                                SS.ALL_BOUND if self.bound is None else self.bound, st, pst)
        moved, pushed = CS.spec_complete_rings(s[5], s[3], self.complete_max) if self.comps else ([], 0)
        return s, st, pst, got, moved, pushed


def upload(queues):
    """Device states of every queue and their UMEM copies; queues that share a UMEM share the device copy."""
    _dev()
    umems = {}
    for q in queues:
        if q.key not in umems:
            umems[q.key] = to_dev(q.umem)
    return [q.state() for q in queues], [umems[q.key] for q in queues]


def block_of(queues, states, umems, opts):
    """The block of one call over `states`, in device memory; the RxQueue structs are kept alive on the tensor."""
    recs = [q.record(d, du) for q, d, du in zip(queues, states, umems)]
    host = X.rx_queues_prepare(recs, opts)
    assert host.nbytes == X.rx_queues_block_size(len(queues))
    d_block = to_dev(host)
    assert d_block.data_ptr() % 64 == 0
    return d_block


def run_and_compare(queues, opts):
    """Leg A, leg B, the spec, and _compare for every queue.  Returns per queue what _compare took."""
    a, ua = upload(queues)
    b, ub = upload(queues)
    for q, d, du in zip(queues, a, ua):
        q.fused(d, du, opts)
    d_block = block_of(queues, b, ub, opts)
    X.rx_queues_dev(d_block, len(queues), opts)
    torch.cuda.synchronize()
    us = {}
    out = []
    for q in queues:  # (a shared UMEM takes every sharer's step before anything is compared with it)
        if q.key not in us:
            us[q.key] = q.umem.copy()
        u = us[q.key]
        out.append((u, *q.spec(u, opts)))
    for k, (q, (u, s, st, pst, got, moved, pushed)) in enumerate(zip(queues, out)):
        try:
            _compare(a[k], b[k], ua[k], ub[k], s, u, st, pst, got, moved, pushed, len(q.txs), len(q.comps), q.outputs)
        except AssertionError as e:
            raise AssertionError(f"queue {k} of {len(queues)}: {e}") from e
    return a, b, out


def case_queue(case):
    (n, max_batch, n_ports, entries, default_port, bound, opts, start, rooms, fill_free, pool_n, cap, stack, n_comp,
     comp_used, complete_max, outputs) = CASES[case]
    umem, table, rx, fill, txs, pool, stk, comps = _build(case)
    return Queue(umem, table, rx, fill, txs, pool, stk, comps, max_batch, default_port, bound, complete_max, outputs)


GROUPS = {opts: [c for c in CASES if CASES[c][6] == opts] for opts in (0x17, 0, 0x7)}
assert sum(len(g) for g in GROUPS.values()) == len(CASES) == 18 and all(GROUPS.values())


@pytest.mark.parametrize("opts", list(GROUPS))
def test_the_fused_calls_cases_as_the_queues_of_one_call(opts):
    """The 18 cases of the fused call's own test, grouped by their options, each group as the queues of one call: an
    empty RX ring, max_batch 1, 64 ports with 65 completion rings, 1024 frames, absent and full stack rings and NULL
    outputs side by side in one grid, every queue with its own n_ports and max_batch."""
    queues = [case_queue(c) for c in GROUPS[opts]]
    a, b, out = run_and_compare(queues, opts)
    for case, (u, s, st, pst, got, moved, pushed) in zip(GROUPS[opts], out):
        assert got["result"]["received"] == min(CASES[case][0], CASES[case][1]), case
    if opts == 0x17:  # the group is what the docstring says it is
        names = GROUPS[opts]
        assert {"empty_rx", "n64_bound_null", "n1024_p64", "stack_absent", "outputs_null", "complete_max0"} <= set(names)
        assert len({(CASES[c][1], CASES[c][2]) for c in names}) >= 5


@pytest.mark.parametrize("case", ["one_frame_mb1", "three_mb48", "n63_unbound"])
def test_one_queue_is_the_fused_call_to_the_byte(case):
    """Q = 1 for each instance: reference mode, wire mode, dual stack."""
    assert [CASES[c][6] for c in ("one_frame_mb1", "three_mb48", "n63_unbound")] == [0, 0x7, 0x17]
    run_and_compare([case_queue(case)], CASES[case][6])


def small_queue(q, opts):
    """1 to 3 frames, one port, one completion ring on the smallest rings make_state allows; the frame count, where the
    index words start, the fill ring's free slots, the pool's count and the completion ring's level all depend on q."""
    n = 1 + q % 3
    umem, descs = _traffic(n, seed=q % 5)
    table = _table_of(umem, descs, opts, 1, 2 if q % 2 else 0, seed=q)
    start = (WRAP, 0, 0x12345 + 977 * q, 0xFFFFFFFF - q)[q % 4]
    rx, fill, txs, pool = make_state(1, 8, start, descs, 1 + q % 8, q % 7, 16 + q % 9, [4096 if q % 11 else 1])
    stk = make_stack(8, 0xFFFFFFFE, q % 4) if q % 3 else None
    comps = make_comps(1, [8], [q % 10], wrap_all=bool(q % 2))
    return Queue(umem, table, rx, fill, txs, pool, stk, comps, 4, 0 if q % 4 else SS.PASS, SS.ALL_BOUND, 1 + q % 8)


def test_more_queues_than_the_device_has_compute_units():
    """Q = 272 on a device of 256 CUs: the last workgroups wait for a CU, no workgroup waits for another.  Every queue is
    checked."""
    q_n, opts = 272, 0x17
    assert q_n > torch.cuda.get_device_properties(_dev()).multi_processor_count
    queues = [small_queue(q, opts) for q in range(q_n)]
    a, b, out = run_and_compare(queues, opts)
    received = [o[4]["result"]["received"] for o in out]
    assert received == [1 + q % 3 for q in range(q_n)]
    assert len({(q.rx.prod, q.rx.cons) for q in queues}) > q_n // 2  # the index words differ from queue to queue


def test_two_queues_over_one_umem():
    """The traffic's descriptors dealt alternately onto two RX rings with pools of their own; both queues name the same
    UMEM (frames of different queues are different chunks).  Leg A is two fused calls on its one UMEM copy, leg B one
    call; the UMEMs are equal afterwards and equal the spec's after both steps."""
    n, n_ports, opts = 64, 3, 0x17
    umem, descs = _traffic(n)
    table = _table_of(umem, descs, opts, n_ports, 94, seed=3)
    queues = []
    for k in range(2):
        rx, fill, txs, pool = make_state(n_ports, 32, WRAP + k, descs[k::2], 20, 30, 200, [4096, 5, 4096])
        pool.addr += np.uint64(k * 200 * 4096)  # the pools hold chunks of their own
        queues.append(Queue(umem, table, rx, fill, txs, pool, make_stack(16, 0xFFFFFFFE, 9 + k),
                            make_comps(4, [16], [3 + k, 0, 16, 5], wrap_all=True), 64, SS.PASS, SS.ALL_BOUND, 64,
                            share="one"))
    a, b, out = run_and_compare(queues, opts)
    assert out[0][0] is out[1][0] and (out[0][0] != umem).any()  # one spec UMEM, and replies were written into it
    assert [o[4]["result"]["received"] for o in out] == [32, 32]
    assert all(o[4]["result"]["replied"] > 0 for o in out)


def test_garbage_in_every_index_word_and_count_word_of_the_middle_queue():
    """The totality claim inside a grid: queue 1 of 3 holds garbage in every index word and in the pool's count word
    (the patterns of the fused call's garbage test); it leaves what the fused call leaves from the same garbage, and
    queues 0 and 2 leave exactly what they leave alone."""
    rng = np.random.default_rng(11)
    for it in range(3):
        n, max_batch, n_ports, opts = 64, 64, 3, 0x17
        queues = []
        for k in range(3):
            umem, descs = _traffic(n, seed=k)
            table = _table_of(umem, descs, opts, n_ports, 94, seed=it)
            rx, fill, txs, pool = make_state(n_ports, 64, WRAP, descs, 30, 40, 300, [4096, 5, 0])
            stk = make_stack(16, 0xFFFFFFFE, 7)
            comps = make_comps(4, [64], [9, 0, 64, 70], wrap_all=True)
            if k == 1:
                for r in (rx, fill, *txs, stk, *comps):
                    r.prod, r.cons = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
                if it != 1:
                    pool.n_free = int(rng.integers(300, 1 << 32))  # above the capacity: a full pool that ends clamped
            queues.append(Queue(umem, table, rx, fill, txs, pool, stk, comps, max_batch, SS.PASS, SS.ALL_BOUND, 1024))
        a, b, out = run_and_compare(queues, opts)
        assert out[1][1][3].n_free <= out[1][1][3].capacity
        assert out[0][4]["result"]["received"] == out[2][4]["result"]["received"] == n


def _snapshot(states, umems):
    """Every byte a call could reach, sentinels and workspaces included."""
    snap = []
    for d, du in zip(states, umems):
        snap.append([g.buf.clone() for g in d.guards()] + [d.stats.clone(), du.clone()])
    return snap


def test_a_block_that_does_not_match_the_call_is_a_no_op():
    """A valid 2-queue block prepared for opts 0x17, called with opts 0x7 and, separately, with n_queues 1: every
    workgroup returns before its first store.  After a synchronisation every ring, word, pool, UMEM byte, output and
    workspace byte of both queues is what was uploaded.  The matching call then does the work, as the fused calls do."""
    opts = 0x17
    queues = [case_queue("n63_unbound"), case_queue("tx_full_and_cut")]
    a, ua = upload(queues)
    b, ub = upload(queues)
    d_block = block_of(queues, b, ub, opts)
    before = _snapshot(b, ub)
    torch.cuda.synchronize()
    X.rx_queues_dev(d_block, 2, 0x7)   # the wire-mode instance meets a dual-stack block
    X.rx_queues_dev(d_block, 2, 0)     # the reference-mode instance too
    X.rx_queues_dev(d_block, 1, opts)  # the right instance, the wrong count
    torch.cuda.synchronize()
    for k, (was, now) in enumerate(zip(before, _snapshot(b, ub))):
        for j, (x, y) in enumerate(zip(was, now)):
            assert torch.equal(x, y), (k, j)
    for q, d, du in zip(queues, a, ua):
        q.fused(d, du, opts)
    X.rx_queues_dev(d_block, 2, opts)
    torch.cuda.synchronize()
    for k, q in enumerate(queues):
        u = q.umem.copy()
        s, st, pst, got, moved, pushed = q.spec(u, opts)
        _compare(a[k], b[k], ua[k], ub[k], s, u, st, pst, got, moved, pushed, len(q.txs), len(q.comps), q.outputs)
        assert got["result"]["received"] >= 63 and got["result"]["replied"] > 0
