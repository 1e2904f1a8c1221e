"""GPU parity of xsk_gpu_neigh_serve_dev: the consumer of the stack ring.  Byte-exact against tests/neigh_spec.spec_serve
(the sequential rule) over every ring's entries -- the stale ones the call must leave too -- every index word, the
result, the counters and the whole UMEM, each between two runs of the sentinel byte SENT.

The traffic: ARP requests and neighbour solicitations for the addresses of up to 64 ports, interleaved, with strangers,
malformed requests, duplicate address detection, TCP and requests for unbound ports among them (built by
tests/golden/make_neigh_golden.py's builders); at least a quarter answered and every verdict present, asserted from the
spec's output."""
import functools

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import neigh_frames as NF  # noqa: E402
from tests import neigh_spec as NS  # noqa: E402
from tests import rx_dev_spec as RS  # noqa: E402
from tests.test_gpu_ingress import _dev  # noqa: E402
from tests.test_gpu_neigh import dev_table, dev_word  # noqa: E402
from tests.test_gpu_rx_step_dev import WRAP, DevRing, Guarded  # noqa: E402

G = NF.G
OPTS = 0x17
UNBOUND_PORT = 5


def owners(n_ports):
    """An IPv4 and an IPv6 address per port: (family, addr, port, mac)."""
    out = []
    for p in range(n_ports):
        out.append((4, bytes([10, 1, p, 1]), p, bytes([2, 0, 0, 4, 0, p])))
        out.append((6, bytes.fromhex("20010db8000100000000000000000000")[:15] + bytes([p + 1]), p, bytes([2, 0, 0, 6, 0, p])))
    return out


@functools.lru_cache(maxsize=None)
def traffic(n, n_ports, seed=0):
    """(UMEM, descriptors, table): n frames, port of frame i walking the ports with a stride that interleaves them."""
    rng = np.random.default_rng(1000 * n + n_ports + seed)
    own = owners(n_ports)
    others = [G.arp_case(tpa=G.STRANGER4), G.ns_case(target=G.STRANGER6), G.ns_case(spoil=True), G.arp_case(hlen=8),
              G.ns_case(src=bytes(16)), G.other_case(G.tcp4), G.arp_case(op=2), G.ns_case(options=G.long_options(264))]
    frames = []
    for i in range(n):
        tags = G.TAGS[int(rng.integers(0, 3))]
        if rng.integers(0, 8) < 5:
            e = own[2 * ((i * 7) % n_ports) + int(rng.integers(0, 2))]
            frame = (G.arp_case(tpa_entry=e, pad=int(rng.integers(0, 19))) if e[0] == 4 else
                     G.ns_case(target_entry=e, pad=int(rng.integers(0, 9))))[0]
        else:
            frame = others[int(rng.integers(0, len(others)))][0]
        frames.append(frame(tags))
    umem, descs = NF.layout(frames)
    descs["options"] = np.arange(n, dtype=np.uint32) + 0x700
    umem.setflags(write=False)
    descs.setflags(write=False)
    return umem, descs, NF.table(own)


def bound_of(n_ports):
    return NS.ALL_BOUND & ~(1 << UNBOUND_PORT) if n_ports > UNBOUND_PORT else NS.ALL_BOUND


def ring(size, prod, used, seed=0, items=None):
    """A descriptor ring of `size` entries, `used` of them in front of the producer word `prod` (garbage words: used may
    exceed the size); every entry holds stale nonzero bytes unless `items` are produced into it."""
    rng = np.random.default_rng(size + seed)
    r = RS.RingState(np.zeros(size, oracle.DESC_DTYPE), prod - used, prod - used)
    r.entries["addr"] = rng.integers(1, 1 << 40, size, dtype=np.uint64)
    r.entries["len"], r.entries["options"] = 0x5A5A, 0xFACE
    if items is not None:
        r.produce(items)
    else:
        r.prod = prod & RS.M32
    return r


class ServeDev:
    """(UMEM, stack, tx rings, up) on the device with the table, the bound word, the counters and the result."""

    def __init__(self, umem, stack, txs, up, table, bound):
        _dev()
        self.umem = Guarded(umem.nbytes, umem)
        self.stack, self.up, self.txs = DevRing(stack), DevRing(up), [DevRing(t) for t in txs]
        self.table, self.n_entries = dev_table(table)
        self.bound = dev_word(None if bound == NS.ALL_BOUND else bound, np.uint64)
        self.stats = Guarded(32, np.zeros(32, np.uint8))
        self.res = Guarded(32)

    def serve(self, max_entries, opts=OPTS, stats=True, res=True):
        X.neigh_serve_dev(self.umem.data, self.stack.view, [t.view for t in self.txs], self.up.view, max_entries,
                          self.table.data if self.table else None, self.n_entries,
                          bound=self.bound.data if self.bound else None, nstats=self.stats.data if stats else None,
                          res=self.res.data if res else None, opts=opts)

    def check(self, umem, stack, txs, up, res=None, stats=None):
        torch.cuda.synchronize()
        assert (self.umem.get() == umem).all(), np.nonzero(self.umem.get() != umem)[0][:8]
        for name, d, want in [("stack", self.stack, stack), ("up", self.up, up)] + \
                [(f"tx{p}", d, t) for p, (d, t) in enumerate(zip(self.txs, txs))]:
            g = d.read()
            assert (g.prod, g.cons) == (want.prod, want.cons), (name, g.prod, g.cons, want.prod, want.cons)
            bad = np.nonzero(g.entries != want.entries)[0]
            assert len(bad) == 0, (name, bad[:5], g.entries[bad[:5]], want.entries[bad[:5]])
            assert d.words.intact() and d.ent.intact(), name
        if res is not None:
            r = self.res.get(X.NEIGH_RESULT_DTYPE)[0]
            assert {k: int(r[k]) for k in NS.RESULT_KEYS} == res and not r["reserved"].any()
        if stats is not None:
            s = self.stats.get(X.NEIGH_STATS_DTYPE)[0]
            assert {k: int(s[k]) for k in NS.STATS_KEYS} == stats
        for g in (self.umem, self.table, self.bound, self.stats, self.res):
            assert g is None or g.intact()


def both(umem, stack, txs, up, table, bound, max_entries, opts=OPTS):
    """The call and the spec from the same state; everything compared.  Returns (result, verdicts, UMEM after)."""
    d = ServeDev(umem, stack, txs, up, table, bound)
    d.serve(max_entries, opts)
    u, s, t, w = umem.copy(), stack.copy(), [x.copy() for x in txs], up.copy()
    st = dict.fromkeys(NS.STATS_KEYS, 0)
    verdicts = []
    res = NS.spec_serve(u, s, t, w, max_entries, opts, table, bound, st, verdicts)
    d.check(u, s, t, w, res, st)
    return res, verdicts, u, (s, t, w)


def state(n, n_ports, stack_size, tx_sizes, tx_used, up_size, up_used, start=WRAP, n_on_stack=None):
    umem, descs, table = traffic(n, n_ports)
    k = n if n_on_stack is None else n_on_stack
    stack = ring(stack_size, start + k, k, items=descs[:k])
    txs = [ring(tx_sizes[p % len(tx_sizes)], start + 3 * p + 1, min(tx_used[p % len(tx_used)], tx_sizes[p % len(tx_sizes)]),
                seed=p) for p in range(n_ports)]
    up = ring(up_size, start - 2, up_used, seed=99)
    return umem, stack, txs, up, table


def test_used_stack_binds_and_everything_has_room():
    umem, stack, txs, up, table = state(40, 3, 64, [64], [5], 64, 3)
    res, v, _, _ = both(umem, stack, txs, up, table, NS.ALL_BOUND, 64)
    assert res["consumed"] == 40 and res["backlog"] == 0 and res["arp_replies"] + res["na_replies"] + res["up"] == 40
    assert 4 * (res["arp_replies"] + res["na_replies"]) >= 40 and res["arp_replies"] and res["na_replies"]


def test_max_binds():
    umem, stack, txs, up, table = state(60, 3, 64, [64], [0], 64, 0)
    for mx in (1, 17, 59):
        res, _, _, _ = both(umem, stack, txs, up, table, NS.ALL_BOUND, mx)
        assert res["consumed"] == mx and res["backlog"] == 60 - mx


@pytest.mark.parametrize("up_room", [0, 1, 6])
def test_a_full_up_ring_stops_the_call(up_room):
    umem, stack, txs, up, table = state(60, 3, 64, [64], [0], 16, 16 - up_room)
    res, v, _, _ = both(umem, stack, txs, up, table, NS.ALL_BOUND, 64)
    c = res["consumed"]
    assert res["up"] == up_room and c < 60 and v == v[:c] and res["backlog"] == 60 - c
    assert c >= up_room  # replies in front of the stopping entry went out all the same


@pytest.mark.parametrize("full_port,room", [(0, 0), (1, 2), (2, 5)])
def test_a_full_tx_ring_stops_the_call_in_the_middle_and_the_frames_behind_stay(full_port, room):
    umem, stack, txs, up, table = state(60, 3, 64, [32], [0], 64, 0)
    txs[full_port] = ring(8, 0xFFFFFFFE, 8 - room, seed=7)
    res, v, after, _ = both(umem, stack, txs, up, table, NS.ALL_BOUND, 64)
    c = res["consumed"]
    assert c < 60 and res["backlog"] == 60 - c
    first_behind = int(stack.entries[stack.slot(stack.cons + c)]["addr"])
    assert (after[first_behind:] == umem[first_behind:]).all()  # (held against the device's UMEM in both())
    # the entry it stopped at is a request of the full port
    verdict, port, _, _ = NS.decide_desc(umem, stack.entries[stack.slot(stack.cons + c)], OPTS, table, 3, NS.ALL_BOUND)
    assert verdict in (NS.ARP_REPLY, NS.NA_REPLY) and port == full_port


@pytest.mark.parametrize("start", [0xFFFFFFFF, 0xFFFFFFF0, 0xFFFFFFC4])
def test_index_words_that_wrap(start):
    umem, stack, txs, up, table = state(60, 3, 64, [16, 32], [3], 64, 10, start=start)
    res, _, _, (s, t, w) = both(umem, stack, txs, up, table, NS.ALL_BOUND, 64)
    assert s.cons < 0x100 and res["consumed"] == 60
    if start == 0xFFFFFFFF:
        assert w.prod < 0x100 and any(x.prod < 0x100 for x in t)


def test_garbage_index_words_are_clamped():
    """producer - consumer above the size: a stack ring read as full, a TX ring and an up ring read as without room."""
    umem, stack, txs, up, table = state(64, 3, 64, [16], [2], 64, 0)
    stack.prod = (stack.cons + 0x80000007) & RS.M32
    res, _, _, _ = both(umem, stack, txs, up, table, NS.ALL_BOUND, 1024)
    assert res["consumed"] + res["backlog"] == 64
    txs[1].prod = (txs[1].cons + 0x90000000) & RS.M32
    res, v, _, _ = both(umem, stack, txs, up, table, NS.ALL_BOUND, 1024)
    assert res["consumed"] < 64
    up.prod = (up.cons + 65) & RS.M32
    res, _, _, _ = both(umem, stack, txs, up, table, NS.ALL_BOUND, 1024)
    assert res["up"] == 0


def test_an_empty_stack_ring_stores_nothing():
    umem, stack, txs, up, table = state(10, 3, 16, [16], [2], 16, 1, n_on_stack=0)
    d = ServeDev(umem, stack, txs, up, table, NS.ALL_BOUND)
    d.res.data.fill_(0x77)
    d.serve(64, stats=True, res=False)  # without a result nothing at all is stored
    d.check(umem, stack, txs, up, None, dict.fromkeys(NS.STATS_KEYS, 0))
    assert (d.res.get() == 0x77).all()
    res, v, _, _ = both(umem, stack, txs, up, table, NS.ALL_BOUND, 64)
    assert res == dict.fromkeys(NS.RESULT_KEYS, 0) and v == []


def test_sixty_four_ports_interleaved_keep_their_order_within_a_port():
    umem, stack, txs, up, table = state(300, 64, 512, [8, 16], [1], 256, 9)
    res, v, after, (s, t, w) = both(umem, stack, txs, up, table, bound_of(64), 1024)
    NF.check_condition(v)
    assert res["consumed"] == 300
    seen = 0
    for p, tx in enumerate(t):
        got = [int(tx.entries[tx.slot(txs[p].prod + k)]["addr"]) for k in range((tx.prod - txs[p].prod) & RS.M32)]
        assert got == sorted(got)  # the frames lie in the UMEM in stack order
        seen += len(got)
    assert seen == res["arp_replies"] + res["na_replies"]
    assert sum(((x.prod - y.prod) & RS.M32) > 0 for x, y in zip(t, txs)) >= 50  # most ports answered


def test_max_1024_with_a_full_ring_of_1024_entries():
    umem, stack, txs, up, table = state(1024, 64, 1024, [64], [0], 1024, 0, start=0xFFFFFE00)
    assert stack.used() == stack.size == 1024
    res, v, _, _ = both(umem, stack, txs, up, table, bound_of(64), 1024)
    assert res["consumed"] == 1024 and res["backlog"] == 0
    NF.check_condition(v)


def test_without_counters_and_result_and_with_other_option_words():
    umem, stack, txs, up, table = state(60, 3, 64, [64], [0], 64, 0)
    for opts in (0, 0x2, 0x10, 0x12):
        both(umem, stack, txs, up, table, NS.ALL_BOUND, 64, opts)
    d = ServeDev(umem, stack, txs, up, table, NS.ALL_BOUND)
    d.stats.data.fill_(0x11)
    d.res.data.fill_(0x22)
    d.serve(64, stats=False, res=False)
    u, s, t, w = umem.copy(), stack.copy(), [x.copy() for x in txs], up.copy()
    NS.spec_serve(u, s, t, w, 64, OPTS, table, NS.ALL_BOUND)
    d.check(u, s, t, w)
    assert (d.stats.get() == 0x11).all() and (d.res.get() == 0x22).all()


def test_the_serve_call_is_the_list_call_over_the_same_entries():
    """With room for everything: verdict counts, frames and reply lengths equal those of xsk_gpu_neigh_dev over the stack
    ring's entries as a list."""
    umem, stack, txs, up, table = state(300, 64, 512, [64], [0], 512, 0)
    bound = bound_of(64)
    res, v, after, (s, t, w) = both(umem, stack, txs, up, table, bound, 1024)
    descs = np.array([stack.entries[stack.slot(stack.cons + j)] for j in range(300)], oracle.DESC_DTYPE)
    d_umem, d_descs = Guarded(umem.nbytes, umem), Guarded(300 * 16, descs)
    d_tab, n_entries = dev_table(table)
    d_bound = dev_word(bound, np.uint64)
    d_v, d_p, d_r = Guarded(300), Guarded(300), Guarded(1200, np.zeros(1200, np.uint8))
    X.neigh_dev(d_umem.data, d_descs.data, 300, d_tab.data, n_entries, 64, d_v.data, d_p.data, bound=d_bound.data,
                reply_len=d_r.data, opts=OPTS)
    torch.cuda.synchronize()
    assert (d_umem.get() == after).all() and list(d_v.get()) == v
    rl, ports = d_r.get(np.uint32), d_p.get()
    for p in range(64):
        mine = [i for i in range(300) if ports[i] == p]
        got = [t[p].entries[t[p].slot(txs[p].prod + k)] for k in range(len(mine))]
        assert [(int(e["addr"]), int(e["len"]), int(e["options"])) for e in got] == \
            [(int(descs[i]["addr"]), int(rl[i]), 0) for i in mine]
    passed = [w.entries[w.slot(up.prod + k)] for k in range(res["up"])]
    assert [e.tobytes() for e in passed] == [descs[i].tobytes() for i in range(300) if ports[i] == 0xFF]
