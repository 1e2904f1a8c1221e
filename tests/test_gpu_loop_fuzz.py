"""Randomised parity for the device RX-loop family under every option word: tests/loop_world.py draws a world from a
seed, and every equivalent device call is driven from it for three rounds, the peers (loop_world.peers) acting on every
leg and on the spec in between.

    leg A   xsk_gpu_rx_pass_step_dev, xsk_gpu_neigh_serve_dev where a responder is attached, xsk_gpu_tx_complete_rings_dev
    leg B   xsk_gpu_rx_loop_dev, the responder behind it
    leg C   xsk_gpu_rx_fused_loop_dev, the responder behind it; outside the fused call's bounds the call returns
            -EINVAL and has written nothing
    queues  five fused worlds of one option word as the queues of one xsk_gpu_rx_queues_dev call a round, two of them
            over one UMEM, against five fused calls

After each round every leg is held against the spec (loop_world.spec_round) as tests/test_gpu_rx_loop_fused.py's
_compare does -- every ring entry and index word, the pool below its count and the count, every UMEM byte, d_actions and
d_ports over all max_batch entries, d_port_counts, d_stats, d_port_stats, *d_res, d_moved, *d_pushed, the responder's
result and counters, every sentinel -- and the legs against each other byte for byte (the pool above its count and the
sentinels included; the workspace is the one thing left out).  An output passed as NULL has a stand-in buffer that must
still be all sentinel.  Every comparison is exact.  One synchronisation a leg a round; no graphs.  A failure names
seed, option word, round and leg; a seed is never retried."""
import errno

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import loop_world as LW  # noqa: E402
from tests import neigh_spec as NS  # noqa: E402
from tests.test_gpu_egress import SENT  # noqa: E402
from tests.test_gpu_ingress import _dev, stats_of  # noqa: E402
from tests.test_gpu_neigh import dev_table as dev_neigh_table  # noqa: E402
from tests.test_gpu_rx_loop_fused import FusedState  # noqa: E402
from tests.test_gpu_rx_queues import block_of  # noqa: E402
from tests.test_gpu_rx_step_dev import DevRing, Guarded  # noqa: E402
from tests.test_gpu_rx_step_steer_dev import port_stats_of  # noqa: E402


class Leg(FusedState):
    """One upload of a world's state: FusedState's rings, pool, workspace and outputs, and with them the UMEM, the
    responder's up ring, table, result and counters.  An output the world passes as NULL keeps its buffer, filled with
    the sentinel."""

    def __init__(self, w, umem=None):
        _dev()
        super().__init__(w.rx, w.fill, w.txs, w.stack, w.pool, w.max_batch, w.comps, w.table, w.bound)
        self.w = w
        self.umem = umem if umem is not None else Guarded(w.umem.nbytes, w.umem)
        self.g_stats = Guarded(40, np.zeros(40, np.uint8))
        self.stats = self.g_stats.data
        self.up = DevRing(w.up) if w.up is not None else None
        self.neigh, self.n_neigh = dev_neigh_table(w.neigh) if w.up is not None else (None, 0)
        self.nres, self.nstats = Guarded(32), Guarded(32, np.zeros(32, np.uint8))
        self.out = dict(actions=self.actions, ports=self.ports, port_counts=self.counts, stats=self.g_stats,
                        port_stats=self.port_stats, res=self.res, moved=self.moved, pushed=self.pushed)
        for name, g in self.out.items():
            if not w.outputs[name]:
                g.data.fill_(SENT)

    def arg(self, name):
        return self.out[name].data if self.w.outputs[name] else None

    def step_args(self):
        return dict(bound=self.bound, actions=self.arg("actions"), ports=self.arg("ports"),
                    port_counts=self.arg("port_counts"), stats=self.arg("stats"), port_stats=self.arg("port_stats"),
                    res=self.arg("res"), opts=self.w.opts)

    def serve(self):
        w = self.w
        if self.up is not None:
            X.neigh_serve_dev(self.umem.data, self.stack.view, self.views, self.up.view, w.serve_max, self.neigh.data,
                              self.n_neigh, bound=self.bound, nstats=self.nstats.data, res=self.nres.data, opts=w.opts)

    def by_hand(self):
        w = self.w
        X.rx_pass_step_dev(self.umem.data, self.rx.view, self.fill.view, self.views, self.stack_view, self.pool.view,
                           w.max_batch, self.table, self.n_entries, w.default_port, self.ws.data, **self.step_args())
        self.serve()
        if w.comps:
            X.tx_complete_rings_dev(self.comp_views, self.pool.view, w.complete_max, moved=self.arg("moved"),
                                    pushed=self.arg("pushed"))

    def loop_call(self, fn):
        w = self.w
        fn(self.umem.data, self.rx.view, self.fill.view, self.views, self.stack_view, self.pool.view, w.max_batch,
           self.table, self.n_entries, w.default_port, self.comp_views, w.complete_max, self.ws.data,
           moved=self.arg("moved"), pushed=self.arg("pushed"), **self.step_args())

    def loop(self):
        self.loop_call(X.rx_loop_dev)
        self.serve()

    def fused(self):
        self.loop_call(X.rx_loop_fused_dev)
        self.serve()

    def record(self, d=None, du=None):
        """The struct xsk_gpu_rx_queue of the arguments fused() passes (the signature tests/test_gpu_rx_queues.block_of
        calls)."""
        w, a = self.w, self.step_args()
        a.pop("opts")
        return X.rx_queue(self.umem.data, self.rx.view, self.fill.view, self.views, self.stack_view, self.pool.view,
                          w.max_batch, self.table, self.n_entries, w.default_port, self.comp_views, w.complete_max,
                          self.ws.data, moved=self.arg("moved"), pushed=self.arg("pushed"), **a)

    def guards(self):
        gs = super().guards() + [self.umem, self.g_stats, self.nres, self.nstats]
        if self.up is not None:
            gs += [self.up.words, self.up.ent] + ([self.neigh] if self.neigh is not None else [])
        return gs

    def follow(self, touched):
        """The peers' moves, from the spec's state: the words and entries of the rings they touched."""
        w = self.w
        mine = dict(zip(map(id, w.rings()), [self.rx, self.fill, *self.txs] +
                        [d for d in (self.stack, self.up) if d is not None] + list(self.comps)))
        for r in touched:
            mine[id(r)].write(r)

    def hold(self, r):
        """Against the spec's state after a round and what the round produced (loop_world.spec_round's record): every
        comparison is made, and all that differ are reported together."""
        w, got, o, n_comp = self.w, r["got"], self.w.outputs, len(self.w.comps)
        wrong = []

        def ring(name, d, want):
            g = d.read()
            if (g.prod, g.cons) != (want.prod, want.cons):
                wrong.append(f"{name}: words {g.prod:#x}, {g.cons:#x}, the spec's {want.prod:#x}, {want.cons:#x}")
            bad = np.nonzero(g.entries != want.entries)[0]
            if len(bad):
                wrong.append(f"{name}: {len(bad)} entries differ, first {bad[:4]}: {g.entries[bad[:4]]}, the spec's "
                             f"{want.entries[bad[:4]]}")

        def same(name, have, want):
            if not np.array_equal(have, want):
                bad = np.nonzero(np.asarray(have) != np.asarray(want))[0]
                wrong.append(f"{name}: {len(bad)} differ, first {bad[:6]}: {np.asarray(have)[bad[:6]]}, the spec's "
                             f"{np.asarray(want)[bad[:6]]}")

        def equal(name, have, want):
            if have != want:
                wrong.append(f"{name}: {have}, the spec's {want}")

        names = ["rx", "fill"] + [f"tx{p}" for p in range(self.n_ports)] + \
            [n for n, x in (("stack", self.stack), ("up", self.up)) if x is not None] + [f"comp{q}" for q in range(n_comp)]
        mine = [self.rx, self.fill, *self.txs] + [d for d in (self.stack, self.up) if d is not None] + list(self.comps)
        for name, d, want in zip(names, mine, w.rings()):
            ring(name, d, want)
        p = self.pool.read()
        equal("pool count", p.n_free, w.pool.n_free)
        same("pool below its count", p.addr[:min(p.n(), w.pool.n())], w.pool.addr[:min(p.n(), w.pool.n())])
        same("UMEM", self.umem.get(), w.umem)
        if self.up is not None:
            res = self.nres.get(X.NEIGH_RESULT_DTYPE)[0]
            equal("responder result", {k: int(res[k]) for k in NS.RESULT_KEYS}, r["nres"])
            equal("responder result's reserved words", bool(res["reserved"].any()), False)
            s = self.nstats.get(X.NEIGH_STATS_DTYPE)[0]
            equal("responder counters", {k: int(s[k]) for k in NS.STATS_KEYS}, w.nstats)
        if o["actions"]:
            same("actions", self.actions.get(), got["actions"])
        if o["ports"]:
            same("ports", self.ports.get(), got["ports"])
        if o["port_counts"]:
            c = self.counts.get(X.EGRESS_COUNTS_DTYPE)
            equal("port_counts", [{k: int(c[q][k]) for k in c.dtype.names} for q in range(self.n_ports)], got["counts"])
        if o["stats"]:
            equal("stats", stats_of(self.stats), w.stats)
        if o["port_stats"]:
            equal("port_stats", port_stats_of(self.port_stats, self.n_ports), w.port_stats)
        if o["res"]:
            equal("res", self.result(), got["result"])
        if o["moved"] and n_comp:
            equal("moved", [int(x) for x in self.moved.get(np.uint32)][:n_comp], r["moved"])
        if o["pushed"] and n_comp:
            equal("pushed", int(self.pushed.get(np.uint32)[0]), r["pushed"])
        for name, g in self.out.items():  # NULL, or (without completion rings) ignored: the buffer keeps its bytes
            if (not o[name] or (name in ("moved", "pushed") and not n_comp)) and not bool((g.data == SENT).all()):
                wrong.append(f"{name} was passed as NULL and written")
        if not all(g.intact() for g in self.guards()):
            wrong.append("a sentinel was overwritten")
        assert not wrong, "; ".join(wrong)[:4000]


def same_bytes(a: Leg, b: Leg):
    """Two legs byte for byte: every guarded array with its sentinels but the workspace."""
    ga, gb = a.guards(), b.guards()
    assert len(ga) == len(gb)
    for k, (x, y) in enumerate(zip(ga, gb)):
        if x is a.ws or x is a.umem:
            continue
        assert torch.equal(x.buf, y.buf), f"guarded array {k} of {len(ga)} differs"
    assert torch.equal(a.umem.buf, b.umem.buf), "the UMEMs differ"


def snapshot(leg: Leg):
    return [g.buf.clone() for g in leg.guards()]


def problems(what, fn, *args):
    """[] where the comparison holds, else what differs, named."""
    try:
        fn(*args)
        return []
    except AssertionError as e:
        return [f"{what}: {e}"]


WORLDS = [(o, s) for o in LW.OPTS_ALL for s in LW.SEEDS[o]]


@pytest.mark.parametrize("opts,seed", WORLDS, ids=[f"{o:#x}-{s}" for o, s in WORLDS])
def test_world(opts, seed):
    _dev()
    w = LW.make_world(seed, opts)
    legs = {"A": Leg(w), "B": Leg(w), "C": Leg(w)}
    run = {"A": Leg.by_hand, "B": Leg.loop, "C": Leg.fused}
    tag = f"seed {seed} opts {opts:#x}"
    if not w.in_fused_bounds():  # the one-workgroup form refuses the bound; nothing is written
        c = legs.pop("C")
        before = snapshot(c)
        with pytest.raises(X.XskGpuError) as e:
            c.loop_call(X.rx_loop_fused_dev)
        torch.cuda.synchronize()
        assert e.value.rc == -errno.EINVAL, f"{tag} leg C: {e.value}"
        assert all(torch.equal(x, y) for x, y in zip(before, snapshot(c))), f"{tag} leg C: the refused call wrote"
    for k in range(LW.ROUNDS):
        touched = LW.peers(w, k)
        for leg in legs.values():  # (before the spec's round changes the rings it is copied from)
            leg.follow(touched)
        r = LW.spec_round(w)
        for name, leg in legs.items():
            run[name](leg)
            torch.cuda.synchronize()
        wrong = []
        for name, leg in legs.items():
            wrong += problems(f"leg {name}", leg.hold, r)
        for name in list(legs)[1:]:
            wrong += problems(f"leg {name} against leg A", same_bytes, legs["A"], legs[name])
        assert not wrong, f"{tag} round {k}: " + " | ".join(wrong)


@pytest.mark.parametrize("opts", LW.OPTS_ALL, ids=[f"{o:#x}" for o in LW.OPTS_ALL])
def test_queues(opts):
    """Five fused worlds of one option word: leg F makes five fused calls a round, leg Q one xsk_gpu_rx_queues_dev call
    over a block prepared once (only device words change between rounds).  The first two worlds share one UMEM and have
    rings and pools of their own."""
    _dev()
    seeds = LW.QUEUE_SEEDS[opts]
    worlds = list(LW.shared_pair(seeds[0], seeds[1], opts)) + [LW.make_world(s, opts, fused=True) for s in seeds[2:]]
    assert all(w.in_fused_bounds() for w in worlds)
    tag = f"seeds {seeds} opts {opts:#x}"

    def upload():
        shared = Guarded(worlds[0].umem.nbytes, worlds[0].umem)
        return [Leg(w, shared if q < 2 else None) for q, w in enumerate(worlds)]

    f_legs, q_legs = upload(), upload()
    d_block = block_of(q_legs, q_legs, [leg.umem.data for leg in q_legs], opts)
    for k in range(LW.ROUNDS):
        touched = [LW.peers(w, k) for w in worlds]
        for legs in (f_legs, q_legs):  # (before the spec's round changes the rings they are copied from)
            for leg, t in zip(legs, touched):
                leg.follow(t)
        rounds = [LW.spec_round(w) for w in worlds]  # (the shared UMEM takes both sharers' rounds before it is compared)
        for leg in f_legs:
            leg.loop_call(X.rx_loop_fused_dev)
        for leg in f_legs:
            leg.serve()
        torch.cuda.synchronize()
        X.rx_queues_dev(d_block, len(worlds), opts)
        for leg in q_legs:
            leg.serve()
        torch.cuda.synchronize()
        wrong = []
        for q, (w, r) in enumerate(zip(worlds, rounds)):
            wrong += problems(f"queue {q} (seed {w.seed}) leg fused", f_legs[q].hold, r)
            wrong += problems(f"queue {q} (seed {w.seed}) leg queues", q_legs[q].hold, r)
            wrong += problems(f"queue {q} (seed {w.seed}) leg queues against leg fused", same_bytes, f_legs[q], q_legs[q])
        assert not wrong, f"{tag} round {k}: " + " | ".join(wrong)
