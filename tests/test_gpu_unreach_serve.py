"""GPU parity of xsk_gpu_unreach_serve_dev: the consumer of the `up` ring.  Byte-exact against
tests/unreach_spec.spec_serve (the sequential rule) over every ring's entries -- the stale ones the call must leave too --
every index word, the budget word, the result, the counters and the whole UMEM, each between two runs of the sentinel
byte SENT.

The traffic: UDP probes over IPv4 and IPv6 for the addresses of up to 64 ports, interleaved, with quotes from 28 to 1232
bytes, and among them probes of strangers, of open ports, of unbound ports, malformed ones, multicast, TCP and probes
whose chunk is one byte short (built by tests/golden/make_unreach_golden.py's builders); at least a quarter answered and
every verdict present, asserted from the spec's output."""
import functools

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import rx_dev_spec as RS  # noqa: E402
from tests import unreach_frames as UF  # noqa: E402
from tests import unreach_spec as US  # noqa: E402
from tests.test_gpu_ingress import _dev  # noqa: E402
from tests.test_gpu_neigh import dev_table, dev_word  # noqa: E402
from tests.test_gpu_neigh_serve import owners, ring  # noqa: E402
from tests.test_gpu_rx_step_dev import WRAP, DevRing, Guarded  # noqa: E402
from tests.test_gpu_unreach import dev_open  # noqa: E402

G = UF.G
OPTS = 0x17
UNBOUND_PORT = 5
NULL = "null"  # no budget word at all


@functools.lru_cache(maxsize=None)
def traffic(n, n_ports, seed=0):
    """(UMEM, descriptors, table): n frames, port of frame i walking the ports with a stride that interleaves them."""
    rng = np.random.default_rng(1000 * n + n_ports + seed)
    own = owners(n_ports)
    others = [(G.udp4_case(dst=G.STRANGER4), None), (G.udp6_case(dst=G.STRANGER6), None), (G.udp4_case(spoil=True), None),
              (G.udp6_case(udp_zero=True), None), (G.udp4_case(entry=own[0], dport=53), None), (G.other(G.tcp4), None),
              (G.udp6_case(entry=own[1], dst_mac=G.MCAST_MAC6), None), (G.udp4_case(entry=own[0], data=3), -1),
              (G.udp6_case(entry=own[1], data=9), -1)]
    frames, rooms = [], []
    for i in range(n):
        tags = G.TAGS[int(rng.integers(0, 3))]
        if rng.integers(0, 8) < 5:
            e = own[2 * ((i * 7) % n_ports) + int(rng.integers(0, 2))]
            case = (G.udp4_case(entry=e, ihl=int(rng.integers(5, 16)), data=int(rng.integers(0, 60)), pad=int(rng.integers(0, 19)))
                    if e[0] == 4 else
                    G.udp6_case(entry=e, data=int(rng.choice([0, 1, 33, 500, 1183, 1184, 1185, 1300])), pad=int(rng.integers(0, 9))))
            room = None
        else:
            case, room = others[int(rng.integers(0, len(others)))]
        frames.append(case[0](tags))
        rooms.append(G.room_of(case[1], room, tags))
    umem, descs = UF.layout(frames, rooms)
    descs["options"] = np.arange(n, dtype=np.uint32) + 0x700
    umem.setflags(write=False)
    descs.setflags(write=False)
    return umem, descs, UF.table(own)


def bound_of(n_ports):
    return US.ALL_BOUND & ~(1 << UNBOUND_PORT) if n_ports > UNBOUND_PORT else US.ALL_BOUND


class ServeDev:
    """(UMEM, up, tx rings, rest) on the device with the table, the bound word, the map, the budget, the counters and
    the result."""

    def __init__(self, umem, up, txs, rest, table, bound, budget):
        _dev()
        self.umem = Guarded(umem.nbytes, umem)
        self.up, self.rest, self.txs = DevRing(up), DevRing(rest), [DevRing(t) for t in txs]
        self.table, self.n_entries = dev_table(table)
        self.bound = dev_word(None if bound == US.ALL_BOUND else bound, np.uint64)
        self.open = dev_open(UF.OPEN)
        self.budget = dev_word(None if budget == NULL else budget, np.uint32)
        self.stats = Guarded(64, np.zeros(64, np.uint8))
        self.res = Guarded(32)

    def serve(self, max_entries, opts=OPTS, stats=True, res=True):
        X.unreach_serve_dev(self.umem.data, self.up.view, [t.view for t in self.txs], self.rest.view, max_entries,
                            self.table.data if self.table else None, self.n_entries, UF.CHUNK,
                            bound=self.bound.data if self.bound else None, open_ports=self.open.data,
                            budget=self.budget.data if self.budget else None, ustats=self.stats.data if stats else None,
                            res=self.res.data if res else None, opts=opts)

    def check(self, umem, up, txs, rest, res=None, stats=None, left=None):
        torch.cuda.synchronize()
        assert (self.umem.get() == umem).all(), np.nonzero(self.umem.get() != umem)[0][:8]
        for name, d, want in [("up", self.up, up), ("rest", self.rest, rest)] + \
                [(f"tx{p}", d, t) for p, (d, t) in enumerate(zip(self.txs, txs))]:
            g = d.read()
            assert (g.prod, g.cons) == (want.prod, want.cons), (name, g.prod, g.cons, want.prod, want.cons)
            bad = np.nonzero(g.entries != want.entries)[0]
            assert len(bad) == 0, (name, bad[:5], g.entries[bad[:5]], want.entries[bad[:5]])
            assert d.words.intact() and d.ent.intact(), name
        if res is not None:
            r = self.res.get(X.UNREACH_RESULT_DTYPE)[0]
            assert {k: int(r[k]) for k in US.RESULT_KEYS} == res and not r["reserved"].any()
        if stats is not None:
            s = self.stats.get(X.UNREACH_STATS_DTYPE)[0]
            assert {k: int(s[k]) for k in US.STATS_KEYS} == stats and not s["reserved"].any()
        if self.budget:
            assert int(self.budget.get(np.uint32)[0]) == left
        for g in (self.umem, self.table, self.bound, self.open, self.budget, self.stats, self.res):
            assert g is None or g.intact()


def both(umem, up, txs, rest, table, bound, max_entries, opts=OPTS, budget=NULL):
    """The call and the spec from the same state; everything compared.  Returns (result, verdicts, UMEM after, rings,
    the budget left)."""
    d = ServeDev(umem, up, txs, rest, table, bound, budget)
    d.serve(max_entries, opts)
    u, s, t, w = umem.copy(), up.copy(), [x.copy() for x in txs], rest.copy()
    st = dict.fromkeys(US.STATS_KEYS, 0)
    verdicts = []
    res, left = US.spec_serve(u, s, t, w, max_entries, opts, table, bound, UF.OPEN, UF.CHUNK,
                              None if budget == NULL else budget, st, verdicts)
    d.check(u, s, t, w, res, st, left)
    return res, verdicts, u, (s, t, w), left


def state(n, n_ports, up_size, tx_sizes, tx_used, rest_size, rest_used, start=WRAP, n_on_ring=None):
    umem, descs, table = traffic(n, n_ports)
    k = n if n_on_ring is None else n_on_ring
    up = ring(up_size, start + k, k, items=descs[:k])
    txs = [ring(tx_sizes[p % len(tx_sizes)], start + 3 * p + 1, min(tx_used[p % len(tx_used)], tx_sizes[p % len(tx_sizes)]),
                seed=p) for p in range(n_ports)]
    rest = ring(rest_size, start - 2, rest_used, seed=99)
    return umem, up, txs, rest, table


def eligible_of(umem, up, table, n_ports, bound, m):
    return [j for j in range(m) if US.decide_desc(umem, up.entries[up.slot(up.cons + j)], OPTS, table, n_ports, bound,
                                                  UF.OPEN, UF.CHUNK)[0] in US.REPLIES]


def test_the_used_ring_binds_and_everything_has_room():
    umem, up, txs, rest, table = state(40, 3, 64, [64], [5], 64, 3)
    res, v, _, _, _ = both(umem, up, txs, rest, table, US.ALL_BOUND, 64)
    assert res["consumed"] == 40 and res["backlog"] == 0 and res["unreach4"] + res["unreach6"] + res["rest"] == 40
    assert 4 * (res["unreach4"] + res["unreach6"]) >= 40 and res["unreach4"] and res["unreach6"] and not res["limited"]


def test_max_binds():
    umem, up, txs, rest, table = state(60, 3, 64, [64], [0], 64, 0)
    for mx in (1, 17, 59):
        res, _, _, _, _ = both(umem, up, txs, rest, table, US.ALL_BOUND, mx)
        assert res["consumed"] == mx and res["backlog"] == 60 - mx


@pytest.mark.parametrize("rest_room", [0, 1, 6])
def test_a_full_rest_ring_stops_the_call(rest_room):
    umem, up, txs, rest, table = state(60, 3, 64, [64], [0], 16, 16 - rest_room)
    res, v, _, _, _ = both(umem, up, txs, rest, table, US.ALL_BOUND, 64)
    c = res["consumed"]
    assert res["rest"] == rest_room and c < 60 and res["backlog"] == 60 - c
    assert c >= rest_room  # errors in front of the stopping entry went out all the same


@pytest.mark.parametrize("full_port,room", [(0, 0), (1, 2), (2, 5)])
def test_a_full_tx_ring_stops_the_call_in_the_middle_and_the_frames_behind_stay(full_port, room):
    umem, up, txs, rest, table = state(60, 3, 64, [32], [0], 64, 0)
    txs[full_port] = ring(8, 0xFFFFFFFE, 8 - room, seed=7)
    res, v, after, _, _ = both(umem, up, txs, rest, table, US.ALL_BOUND, 64)
    c = res["consumed"]
    assert c < 60 and res["backlog"] == 60 - c
    first_behind = int(up.entries[up.slot(up.cons + c)]["addr"])
    assert (after[first_behind:] == umem[first_behind:]).all()  # (held against the device's UMEM in both())
    verdict, port, _, _ = US.decide_desc(umem, up.entries[up.slot(up.cons + c)], OPTS, table, 3, US.ALL_BOUND, UF.OPEN,
                                         UF.CHUNK)
    assert verdict in US.REPLIES and port == full_port  # the entry it stopped at is a probe of the full port


@pytest.mark.parametrize("budget", [0, 1, "eligible", "eligible-3", "eligible+2", 0xFFFFFFFF, NULL])
def test_the_budget(budget):
    umem, up, txs, rest, table = state(300, 64, 512, [64], [0], 512, 0)
    bound = bound_of(64)
    n = len(eligible_of(umem, up, table, 64, bound, 300))
    assert n >= 75
    b = {"eligible": n, "eligible-3": n - 3, "eligible+2": n + 2}.get(budget, budget)
    res, v, after, _, left = both(umem, up, txs, rest, table, bound, 1024, budget=b)
    sent = res["unreach4"] + res["unreach6"]
    assert res["consumed"] == 300 and sent == (n if b == NULL else min(n, b)) and res["limited"] == n - sent
    assert left == (None if b == NULL else b - sent)
    if b == 0:
        assert (after == umem).all() and res["rest"] == 300  # nothing is rewritten, everything goes on
    if b == n - 3:
        UF.check_condition(v, limited=True)


def test_the_budget_binds_in_front_of_a_full_ring_and_behind_it():
    """A LIMITED entry goes to rest, so a budget changes where a full ring stops the call."""
    umem, up, txs, rest, table = state(60, 3, 64, [4], [0], 64, 0)
    res_free, _, _, _, _ = both(umem, up, txs, rest, table, US.ALL_BOUND, 64)
    res_two, _, _, _, left = both(umem, up, txs, rest, table, US.ALL_BOUND, 64, budget=2)
    assert res_free["consumed"] < 60 and res_two["consumed"] == 60 and left == 0 and res_two["limited"] >= 10
    res, _, _, _, left = both(umem, up, txs, rest, table, US.ALL_BOUND, 64, budget=50)  # the ring stops it first
    assert res == res_free and left == 50 - res["unreach4"] - res["unreach6"] > 0


@pytest.mark.parametrize("start", [0xFFFFFFFF, 0xFFFFFFF0, 0xFFFFFFC4])
def test_index_words_that_wrap(start):
    umem, up, txs, rest, table = state(60, 3, 64, [32, 64], [3], 64, 10, start=start)
    res, _, _, (s, t, w), _ = both(umem, up, txs, rest, table, US.ALL_BOUND, 64, budget=0xFFFFFFF0)
    assert s.cons < 0x100 and res["consumed"] == 60
    if start == 0xFFFFFFFF:
        assert w.prod < 0x100 and any(x.prod < 0x100 for x in t)


def test_garbage_index_words_are_clamped():
    """producer - consumer above the size: an up ring read as full, a TX ring and a rest ring read as without room."""
    umem, up, txs, rest, table = state(64, 3, 64, [64], [2], 64, 0)
    up.prod = (up.cons + 0x80000007) & RS.M32
    res, _, _, _, _ = both(umem, up, txs, rest, table, US.ALL_BOUND, 1024)
    assert res["consumed"] + res["backlog"] == 64
    txs[1].prod = (txs[1].cons + 0x90000000) & RS.M32
    res, v, _, _, _ = both(umem, up, txs, rest, table, US.ALL_BOUND, 1024)
    assert res["consumed"] < 64
    rest.prod = (rest.cons + 65) & RS.M32
    res, _, _, _, _ = both(umem, up, txs, rest, table, US.ALL_BOUND, 1024)
    assert res["rest"] == 0


def test_an_empty_ring_stores_nothing():
    umem, up, txs, rest, table = state(10, 3, 16, [16], [2], 16, 1, n_on_ring=0)
    d = ServeDev(umem, up, txs, rest, table, US.ALL_BOUND, 9)
    d.res.data.fill_(0x77)
    d.serve(64, stats=True, res=False)  # without a result nothing at all is stored
    d.check(umem, up, txs, rest, None, dict.fromkeys(US.STATS_KEYS, 0), 9)
    assert (d.res.get() == 0x77).all()
    res, v, _, _, left = both(umem, up, txs, rest, table, US.ALL_BOUND, 64, budget=9)
    assert res == dict.fromkeys(US.RESULT_KEYS, 0) and v == [] and left == 9


def test_sixty_four_ports_interleaved_keep_their_order_within_a_port():
    umem, up, txs, rest, table = state(300, 64, 512, [8, 16], [1], 256, 9)
    res, v, after, (s, t, w), _ = both(umem, up, txs, rest, table, bound_of(64), 1024)
    UF.check_condition(v)
    assert res["consumed"] == 300
    seen = 0
    for p, tx in enumerate(t):
        got = [int(tx.entries[tx.slot(txs[p].prod + k)]["addr"]) for k in range((tx.prod - txs[p].prod) & RS.M32)]
        assert got == sorted(got)  # the frames lie in the UMEM in ring order
        seen += len(got)
    assert seen == res["unreach4"] + res["unreach6"]
    assert sum(((x.prod - y.prod) & RS.M32) > 0 for x, y in zip(t, txs)) >= 50  # most ports answered


def test_max_1024_with_a_full_ring_of_1024_entries():
    umem, up, txs, rest, table = state(1024, 64, 1024, [64], [0], 1024, 0, start=0xFFFFFE00)
    assert up.used() == up.size == 1024
    res, v, _, _, left = both(umem, up, txs, rest, table, bound_of(64), 1024, budget=400)
    assert res["consumed"] == 1024 and res["backlog"] == 0 and left == 0 and res["limited"] > 0
    UF.check_condition(v, limited=True)


def test_without_counters_and_result_and_with_other_option_words():
    umem, up, txs, rest, table = state(60, 3, 64, [64], [0], 64, 0)
    for opts in (0, 0x2, 0x10, 0x12):
        both(umem, up, txs, rest, table, US.ALL_BOUND, 64, opts)
    d = ServeDev(umem, up, txs, rest, table, US.ALL_BOUND, NULL)
    d.stats.data.fill_(0x11)
    d.res.data.fill_(0x22)
    d.serve(64, stats=False, res=False)
    u, s, t, w = umem.copy(), up.copy(), [x.copy() for x in txs], rest.copy()
    US.spec_serve(u, s, t, w, 64, OPTS, table, US.ALL_BOUND, UF.OPEN, UF.CHUNK)
    d.check(u, s, t, w)
    assert (d.stats.get() == 0x11).all() and (d.res.get() == 0x22).all()


def test_the_serve_call_is_the_list_call_over_the_same_entries():
    """With room for everything and no budget: verdicts, frames and reply lengths equal those of xsk_gpu_unreach_dev over
    the ring's entries as a list."""
    umem, up, txs, rest, table = state(300, 64, 512, [64], [0], 512, 0)
    bound = bound_of(64)
    res, v, after, (s, t, w), _ = both(umem, up, txs, rest, table, bound, 1024)
    descs = np.array([up.entries[up.slot(up.cons + j)] for j in range(300)], oracle.DESC_DTYPE)
    d_umem, d_descs = Guarded(umem.nbytes, umem), Guarded(300 * 16, descs)
    d_tab, n_entries = dev_table(table)
    d_bound, d_open = dev_word(bound, np.uint64), dev_open(UF.OPEN)
    d_v, d_p, d_r = Guarded(300), Guarded(300), Guarded(1200, np.zeros(1200, np.uint8))
    X.unreach_dev(d_umem.data, d_descs.data, 300, d_tab.data, n_entries, 64, UF.CHUNK, d_v.data, d_p.data,
                  bound=d_bound.data, open_ports=d_open.data, reply_len=d_r.data, opts=OPTS)
    torch.cuda.synchronize()
    assert (d_umem.get() == after).all() and list(d_v.get()) == v
    rl, ports = d_r.get(np.uint32), d_p.get()
    for p in range(64):
        mine = [i for i in range(300) if ports[i] == p]
        got = [t[p].entries[t[p].slot(txs[p].prod + k)] for k in range(len(mine))]
        assert [(int(e["addr"]), int(e["len"]), int(e["options"])) for e in got] == \
            [(int(descs[i]["addr"]), int(rl[i]), 0) for i in mine]
    passed = [w.entries[w.slot(rest.prod + k)] for k in range(res["rest"])]
    assert [e.tobytes() for e in passed] == [descs[i].tobytes() for i in range(300) if ports[i] == 0xFF]
