"""A seeded world for the device RX-loop family: everything one RX loop needs -- option word, traffic, UMEM, three RX
offers, the steering and neighbour tables, the call's parameters, every ring, the pool and the choice of optional
outputs -- drawn from np.random.default_rng(seed), and the spec's composition over it.  Plain Python: nothing here
touches a GPU.  tests/test_loop_world.py holds the generator and the spec against the coverage the seed set must reach,
tests/test_gpu_loop_fuzz.py drives every equivalent device call from the same worlds.

    make_world(seed, opts=None, fused=None)   the world before its first round
    peers(world, k)                           what the other side does before round k; returns the rings it touched
    spec_round(world)                         rx_pass_spec, then neigh_spec where a responder is attached, then
                                              tx_complete_rings_spec, on the world's own state, in place

The world's rings are the spec's state: a device leg is uploaded from them before the first peers() call and follows by
writing the touched rings after every later one.

The draw spaces (the weights are this file's):
  option word   all sixteen valid words, or the argument
  traffic       wire_frames.random_frame and v6_frames.random_frame6 half and half (echo requests and every negative);
                in a third of the worlds three frames in ten are neigh_frames ARP requests and neighbour solicitations
                for the responder's own addresses and for strangers, and a responder is attached behind the stack ring
  placement     frame i in a 2048-B chunk of its own at a headroom from {0, 1, i % 16, 256}; the chunks in a random
                permutation of ring order; the frame in the last chunk ends on the last byte of the world's UMEM
  offers        three rounds of {0, 1, 2, 63, 64, 65, 255, 256, 257} frames, at most one of {1023, 1024, 1025, 1300}
  bad entries   in a quarter of the worlds 1-3 descriptors a round do not fit the UMEM (BAD_ROWS)
  parameters    MAX_BATCH, N_PORTS, ENTRIES, COMPLETE_MAX; default port PASS, bound or unbound; bound NULL, all, holes, 0
  state         index words at 0, WRAP, a random word or within 8 of 2^32; TX rooms from the first round's reply counts;
                fill, pool, stack and completion rings at every level; one world in eight with garbage in every word
  outputs       each of OUTPUTS present or NULL on its own (no entry point refuses a combination: every one is optional)
"""
import functools
import time
from collections import Counter

import numpy as np

import oracle
from tests import egress_ports_spec as EP
from tests import ingress_spec as IS
from tests import neigh_frames as NF
from tests import neigh_spec as NS
from tests import rx_dev_spec as RS
from tests import rx_pass_spec as PS
from tests import steer_spec as SS
from tests import tx_complete_rings_spec as CS
from tests.test_gpu_neigh_serve import owners, ring
from tests.test_gpu_rx_pass_step_dev import make_stack
from tests.test_gpu_rx_step_dev import WRAP
from tests.test_gpu_rx_step_steer_dev import make_state, pow2_at_least
from tests.test_gpu_tx_complete_rings import make_comps
from tests.v6_frames import random_frame6
from tests.wire_frames import random_frame

G = NF.G
CHUNK = 2048
OPTS_ALL = tuple(range(8)) + tuple(range(0x10, 0x18))
SMALL_OFFERS = (0, 1, 2, 63, 64, 65, 255, 256, 257)
LARGE_OFFERS = (1023, 1024, 1025, 1300)
MAX_BATCH = (1, 4, 48, 64, 256, 1024, 1025, 2048)
N_PORTS = (1, 2, 3, 8, 63, 64)
ENTRIES = (0, 1, 22, 1023, 1024)
COMPLETE_MAX = (0, 1, 64, 1024, 2048)
N_COMP = (0, 1, 4, 65)
SERVE_MAX = (1, 16, 64, 1024)
FUSED_MAX = 1024  # the bounds of xsk_gpu_rx_fused_loop_dev(): max_batch and, with completion rings, complete_max
OUTPUTS = ("actions", "ports", "port_counts", "stats", "port_stats", "res", "moved", "pushed")
ROUNDS = 3

# The seed set: three worlds an option word for test_world, five fused worlds an option word for test_queues (the first
# two of them share one UMEM).  A seed that found a difference stays.
SEEDS = {o: tuple(1000 * o + k for k in range(3)) for o in OPTS_ALL}
SEEDS[0x12] += (18003, 18004)  # (the first three: max_batch 1, garbage words, one port -- no IPv6 reply among them)
QUEUE_SEEDS = {o: tuple(500_000 + 1000 * o + k for k in range(5)) for o in OPTS_ALL}


def bad_rows(size):
    """Descriptors that do not fit a UMEM of `size` bytes, and the empty one at its end."""
    return [(size + 5, 60), (size - 10, 60), (0, (1 << 30) + 1), (size, 0), (0xFFFFFFFFFFFFFFF0, 64)]


class World:
    """One world.  The rings, the pool, the UMEM and the counters are the spec's state and change with every peers() and
    spec_round(); everything else is fixed by make_world()."""

    def bound_word(self):
        return SS.ALL_BOUND if self.bound is None else self.bound

    def rings(self):
        return [self.rx, self.fill, *self.txs] + [r for r in (self.stack, self.up) if r is not None] + list(self.comps)

    def in_fused_bounds(self):
        return self.max_batch <= FUSED_MAX and (not self.comps or self.complete_max <= FUSED_MAX)

    def census(self) -> Counter:
        """The multiset of chunk addresses the containers hold: every ring's unconsumed entries, the pool below its
        count (tests/test_gpu_rx_loop_dev_graph.census, with the up ring)."""
        c = Counter()
        for r in self.rings():
            for j in range(r.used()):
                e = r.entries[r.slot(r.cons + j)]
                c[int(e["addr"]) if r.entries.dtype.names else int(e)] += 1
        c.update(int(a) for a in self.pool.addr[:self.pool.n()])
        return c


def _word(rng):
    kind = int(rng.integers(0, 4))
    return (0, WRAP, int(rng.integers(0, 1 << 32)), (1 << 32) - int(rng.integers(1, 9)))[kind]


def rebase(r: RS.RingState, cons: int):
    """The same ring with its consumer word at `cons`: the entries turn with the words."""
    shift = (cons - r.cons) & RS.M32
    r.entries[:] = np.roll(r.entries, shift % r.size)
    r.prod, r.cons = (r.prod + shift) & RS.M32, cons & RS.M32


def _neigh_frame(rng, own, others):
    tags = G.TAGS[int(rng.integers(0, 3))]
    if rng.integers(0, 8) < 5:
        e = own[int(rng.integers(0, len(own)))]
        case = (G.arp_case(tpa_entry=e, pad=int(rng.integers(0, 19))) if e[0] == 4 else
                G.ns_case(target_entry=e, pad=int(rng.integers(0, 9))))
    else:
        case = others[int(rng.integers(0, len(others)))]
    f = case[0](tags)
    return f, len(f)


def _traffic(rng, n, own, before, after):
    """(UMEM, descriptors in ring order): n frames, each in a chunk of its own behind `before` reserved bytes."""
    others = [G.arp_case(tpa=G.STRANGER4), G.ns_case(target=G.STRANGER6), G.ns_case(spoil=True), G.arp_case(hlen=8),
              G.ns_case(src=bytes(16)), G.other_case(G.tcp4), G.arp_case(op=2)]
    own_size = max(n, 1) * CHUNK
    umem = np.zeros(before + own_size + after, np.uint8)
    umem[before:before + own_size] = rng.integers(0, 256, own_size, dtype=np.uint8)  # garbage around the frames
    descs = np.zeros(n, oracle.DESC_DTYPE)
    chunk_of = rng.permutation(n)
    for i in range(n):
        r = rng.random()
        if own and r < 0.3:
            f, L = _neigh_frame(rng, own, others)
        elif r < 0.65:
            f, L = random_frame(rng, int(rng.choice([40, 200, 1400])))
        else:
            f, L = random_frame6(rng, int(rng.choice([40, 200, 1400])))
        head = (0, 1, i % 16, 256)[int(rng.integers(0, 4))]
        c = int(chunk_of[i])
        if c == n - 1:  # the last chunk's frame ends on the last byte of the world's own UMEM
            if len(f) == 0:
                f = b"\0"
            head, L = CHUNK - len(f), len(f)
        assert head + len(f) <= CHUNK
        a = before + c * CHUNK + head
        umem[a:a + len(f)] = np.frombuffer(f, np.uint8)
        descs[i] = (a, L, 0x1000 + i)
    return umem, descs


def _pick_level(rng, levels):
    return levels[int(rng.integers(0, len(levels)))]


def make_world(seed, opts=None, fused=None, before=0, after=0) -> World:
    """`before` and `after` reserve bytes of the UMEM in front of and behind the world's own chunks (for a second world
    over the same UMEM); they change no draw."""
    rng = np.random.default_rng(seed)
    w = World()
    w.seed, w.fused = seed, fused
    drawn = int(OPTS_ALL[int(rng.integers(0, len(OPTS_ALL)))])
    w.opts = drawn if opts is None else int(opts)
    assert w.opts in OPTS_ALL
    # ---- parameters ----
    mb = [m for m in MAX_BATCH if not fused or m <= FUSED_MAX]
    cm = [m for m in COMPLETE_MAX if not fused or m <= FUSED_MAX]
    w.max_batch = int(mb[int(rng.integers(0, len(mb)))])
    w.complete_max = int(cm[int(rng.integers(0, len(cm)))])
    w.n_ports = int(N_PORTS[int(rng.integers(0, len(N_PORTS)))])
    entries = int(rng.choice(ENTRIES, p=[0.1, 0.15, 0.45, 0.15, 0.15]))
    kind = int(rng.choice(4, p=[0.3, 0.3, 0.35, 0.05]))  # NULL, all, holes, 0
    holes = int(rng.integers(0, 1 << 63)) | int(rng.integers(0, 2)) << 63 | 1 << int(rng.integers(0, w.n_ports))
    w.bound = (None, SS.ALL_BOUND, holes, 0)[kind]  # (a mask with holes keeps at least one port bound)
    bound_ports = [p for p in range(w.n_ports) if (w.bound_word() >> p) & 1]
    unbound_ports = [p for p in range(w.n_ports) if not (w.bound_word() >> p) & 1]
    kind = int(rng.choice(3, p=[0.5, 0.4, 0.1]))  # PASS, a bound port, an unbound port
    pick = lambda ps: ps[int(rng.integers(0, len(ps)))] if ps else SS.PASS  # noqa: E731
    w.default_port = int((SS.PASS, pick(bound_ports), pick(unbound_ports))[kind])
    w.garbage = bool(rng.integers(0, 8) == 0)
    with_neigh = bool(rng.integers(0, 3) == 0)
    bad = bool(rng.integers(0, 4) == 0)
    # ---- offers ----
    counts = [int(SMALL_OFFERS[int(rng.integers(0, len(SMALL_OFFERS)))]) for _ in range(ROUNDS)]
    if rng.random() < 0.3:
        counts[int(rng.integers(0, ROUNDS))] = int(LARGE_OFFERS[int(rng.integers(0, len(LARGE_OFFERS)))])
    total = sum(counts)
    own = owners(w.n_ports) if with_neigh else []
    w.umem, descs = _traffic(rng, total, own, before, after)
    w.own_bytes = len(w.umem) - before - after
    w.neigh = NF.table(own) if with_neigh else None
    w.offers, at = [], 0
    rows = bad_rows(len(w.umem))
    for n in counts:
        d = descs[at:at + n].copy()
        at += n
        if bad and n:
            for _ in range(int(rng.integers(1, 4))):
                a, ln = rows[int(rng.integers(0, len(rows)))]
                d[int(rng.integers(0, n))] = (a, ln, int(rng.integers(0, 1 << 32)))
        w.offers.append(d)
    every = np.concatenate(w.offers) if total else descs
    w.table = (SS.sample_table(SS.destinations(w.umem, every, w.opts), entries, w.n_ports, seed=seed & 0xFFFF)
               if entries else {})
    # ---- the first round's steered ingress: the replies per port and the PASS count the rooms are drawn around ----
    first = min(counts[0], w.max_batch)
    d0 = np.zeros(max(first, 1), oracle.DESC_DTYPE)
    d0[:first] = w.offers[0][:first]
    if first:
        ing = SS.spec_ingress_steer(w.umem.copy(), d0[:first], w.opts, w.table, w.default_port, w.n_ports, w.bound_word())
        off = [int(x) for x in ing["off"]]
        replies = [int((ing["verdicts"][off[p]:off[p + 1]] == 0).sum()) for p in range(w.n_ports)]
        n_pass = int((ing["actions"] == SS.XDP_PASS).sum())
    else:
        replies, n_pass = [0] * w.n_ports, 0
    # ---- state ----
    size = pow2_at_least(total) * int(rng.choice([1, 2], p=[0.7, 0.3]))
    rooms = []
    for p in range(w.n_ports):
        k = int(rng.choice(5, p=[0.1, 0.1, 0.25, 0.15, 0.4]))
        rooms.append((0, 1, max(replies[p] - 1, 0), replies[p], 4096)[k])
    cap = int(rng.choice([max(size // 2, 8), 2 * size + 3, 8 * size], p=[0.2, 0.3, 0.5]))
    few = int(rng.integers(1, 6))
    pool_n = int(rng.choice([0, few, cap - few, cap], p=[0.15, 0.35, 0.35, 0.15]))
    w.rx, w.fill, w.txs, w.pool = make_state(w.n_ports, size, _word(rng), descs[:0], int(rng.integers(0, size + 1)),
                                             pool_n, cap, rooms)
    w.pool.addr += np.uint64((seed & 0xFFF) << 44)  # pools of different worlds hold chunks of their own
    w.up, w.serve_max = None, 0
    if with_neigh:  # a responder consumes the stack ring: the ring is there, with room for part or plenty
        part = bool(rng.integers(0, 3) == 0)
        room = max(n_pass // 2, 1) if part else n_pass + int(rng.integers(3, 40))
        s_size = pow2_at_least(room) * int(rng.choice([1, 2]))
        w.stack = make_stack(s_size, _word(rng), min(room, s_size), seed=seed & 0xFF)
        u_size = int(rng.choice([8, 64, 2048]))
        w.up = ring(u_size, _word(rng), int(_pick_level(rng, (0, u_size // 2, u_size - 1, u_size))), seed=seed & 0xFF)
        w.serve_max = int(rng.choice(SERVE_MAX, p=[0.1, 0.25, 0.25, 0.4]))
    else:
        k = int(rng.choice(4, p=[0.2, 0.15, 0.3, 0.35]))  # absent, room 0, room for part, plenty
        room = (0, 0, max(n_pass // 2, 1), n_pass + int(rng.integers(3, 40)))[k]
        s_size = pow2_at_least(room) * int(rng.choice([1, 2]))
        w.stack = None if k == 0 else make_stack(s_size, _word(rng), min(room, s_size), seed=seed & 0xFF)
    n_comp = int(rng.choice(N_COMP, p=[0.15, 0.2, 0.4, 0.25]))
    if n_comp:
        sizes = [int(x) for x in rng.choice([8, 64, 256, 2048], 5)]
        useds = [int(_pick_level(rng, (0, 3, 40, 5000))) for _ in range(6)]  # empty, part, full (a level above the size)
        w.comps = make_comps(n_comp, sizes, useds)
        for c in w.comps:
            rebase(c, _word(rng))
    else:
        w.comps = []
    if w.garbage:  # the totality claim: whatever the words hold
        for r in w.rings():
            r.prod, r.cons = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
        w.pool.n_free = int(rng.integers(0, 1 << 32))
    w.outputs = {name: bool(rng.random() < 0.7) for name in OUTPUTS}
    # ---- the spec's running state ----
    w.stats = dict.fromkeys(IS.KEYS, 0)
    w.port_stats = [dict.fromkeys(EP.STATS_KEYS, 0) for _ in w.txs]
    w.nstats = dict.fromkeys(NS.STATS_KEYS, 0)
    w.round = 0
    w.peer_rng = np.random.default_rng([seed, 0x9EE5])
    return w


def shared_pair(seed_a, seed_b, opts, fused=True):
    """Two worlds over one UMEM: a's chunks in front, b's behind; each has rings and a pool of its own, and descriptors
    that do not fit are measured against the whole UMEM.  Both worlds' `umem` is the one array."""
    size_b = make_world(seed_b, opts, fused).own_bytes
    a = make_world(seed_a, opts, fused, after=size_b)
    b = make_world(seed_b, opts, fused, before=a.own_bytes)
    assert len(a.umem) == len(b.umem) and b.own_bytes == size_b
    a.umem[a.own_bytes:] = b.umem[a.own_bytes:]
    b.umem = a.umem
    return a, b


def _some(rng, n):
    """A random number in [0, n]: none, all, or anything between."""
    k = int(rng.integers(0, 4))
    return 0 if k == 0 else n if k == 1 else int(rng.integers(0, n + 1))


def peers(w: World, k: int):
    """The other side before round k: the round's RX offer (as much as the ring has room for), some entries of every TX
    ring "transmitted" onto that port's completion ring where it has one with room (without one they leave), some fill
    entries taken, some stack entries taken (the up ring's where a responder is attached).  Returns the rings touched."""
    rng = w.peer_rng
    touched = [w.rx, w.fill]
    offer = w.offers[k]
    assert w.garbage or w.rx.free() >= len(offer)
    w.rx.produce(offer[:w.rx.free()])
    for p, tx in enumerate(w.txs):
        comp = w.comps[p] if p < len(w.comps) else None
        n = _some(rng, tx.used() if comp is None else min(tx.used(), comp.free()))
        if n == 0:
            continue
        if comp is not None:
            comp.produce([tx.entries[tx.slot(tx.cons + j)]["addr"] for j in range(n)])
            touched.append(comp)
        tx.cons = (tx.cons + n) & RS.M32
        touched.append(tx)
    w.fill.cons = (w.fill.cons + _some(rng, w.fill.used())) & RS.M32
    taker = w.up if w.up is not None else w.stack
    if taker is not None:
        taker.cons = (taker.cons + _some(rng, taker.used())) & RS.M32
        touched.append(taker)
    return touched


def spec_round(w: World) -> dict:
    """One round of the spec on the world's state: the pass step, the responder where attached, the completion rings.
    Returns what each produced, and what the coverage conditions are read from."""
    words = [(r.prod, r.cons) for r in w.rings()]
    out = dict(round=w.round, offered=w.rx.used(), fill_free=w.fill.free(), pool_room=w.pool.capacity - w.pool.n(),
               stack_room=None if w.stack is None else w.stack.free(), comp_used=[c.used() for c in w.comps],
               census=None if w.garbage else w.census())
    t0 = time.perf_counter()
    out["got"] = PS.spec_step_pass(w.umem, w.rx, w.fill, w.txs, w.stack, w.pool, w.max_batch, w.opts, w.table,
                                   w.default_port, w.bound_word(), w.stats, w.port_stats)
    out["nres"], out["nverdicts"] = None, []
    if w.up is not None:
        out["nres"] = NS.spec_serve(w.umem, w.stack, w.txs, w.up, w.serve_max, w.opts, w.neigh, w.bound_word(), w.nstats,
                                    out["nverdicts"])
    out["moved"], out["pushed"] = CS.spec_complete_rings(w.comps, w.pool, w.complete_max) if w.comps else ([], 0)
    out["seconds"] = time.perf_counter() - t0
    # an index word crossed 2^32: it advanced (by less than 2^31) and is smaller than it was
    out["crossed"] = (not w.garbage) and any(
        (a != b and ((a - b) & RS.M32) < (1 << 31) and a < b) for r, (p0, c0) in zip(w.rings(), words)
        for a, b in ((r.prod, p0), (r.cons, c0)))
    out["census_after"] = None if w.garbage else w.census()
    w.round += 1
    return out


def reply_families(w: World, got) -> Counter:
    """The IP family of every frame the round answered (TX_REPLY in the transform's verdicts), from the UMEM."""
    fams = Counter()
    total = int(got["off"][len(w.txs)])
    order = SS.partition(got["descs"], got["actions"], got["ports"], len(w.txs))["out"]
    for i in range(total):
        if got["verdicts"][i] == IS.TX_REPLY:
            a, ln = int(order[i]["addr"]), int(order[i]["len"])
            fams[SS.GS.ip_header(w.umem[a:a + min(ln, 128)].tobytes(), w.opts)[1]] += 1
    return fams


@functools.lru_cache(maxsize=None)
def run_spec(seed, opts, fused=None):
    """A world run through its three rounds by the spec alone: (world after, the rounds' records, build seconds)."""
    t0 = time.perf_counter()
    w = make_world(seed, opts, fused)
    built = time.perf_counter() - t0
    rounds = []
    for k in range(ROUNDS):
        peers(w, k)
        r = spec_round(w)
        r["families"] = reply_families(w, r["got"])
        rounds.append(r)
    return w, rounds, built
