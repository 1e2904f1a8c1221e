"""CPU tests of tests/loop_world.py: the generator is deterministic, the spec's composition conserves chunk addresses,
and the committed seed set (loop_world.SEEDS, the one tests/test_gpu_loop_fuzz.py runs on the device) reaches every
situation the randomised GPU tests are there for.  Coverage is read from the spec's output alone; the conditions do not
relax: a seed set that misses one gets more seeds (up to six an option word) or other weights."""
from collections import Counter

import numpy as np

from tests import loop_world as LW
from tests import steer_spec as SS


def _worlds():
    """(opts, seed, world after its rounds, the rounds' records, build seconds) of every world of the seed set."""
    return [(o, s, *LW.run_spec(s, o)) for o in LW.OPTS_ALL for s in LW.SEEDS[o]]


def _same(a, b):
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def _fingerprint(w):
    fp = [w.opts, w.max_batch, w.n_ports, w.default_port, w.bound, w.complete_max, w.garbage, w.serve_max, w.table,
          w.neigh, w.outputs, w.umem, w.pool.addr, w.pool.n_free, *w.offers]
    for r in w.rings():
        fp += [r.prod, r.cons, r.entries]
    return fp


def test_make_world_is_deterministic_in_its_seed():
    for o, s in ((None, 7), (0x11, 17000), (0x6, 6002)):
        a, b = LW.make_world(s, o), LW.make_world(s, o)
        fa, fb = _fingerprint(a), _fingerprint(b)
        assert len(fa) == len(fb) and all(_same(x, y) for x, y in zip(fa, fb))
        for k in range(LW.ROUNDS):  # the peers and the spec too
            ta, tb = LW.peers(a, k), LW.peers(b, k)
            assert [a.rings().index(r) for r in ta] == [b.rings().index(r) for r in tb]
            ra, rb = LW.spec_round(a), LW.spec_round(b)
            assert ra["got"]["result"] == rb["got"]["result"] and ra["moved"] == rb["moved"] and ra["nres"] == rb["nres"]
        assert all(_same(x, y) for x, y in zip(_fingerprint(a), _fingerprint(b)))
    assert LW.make_world(7).opts == LW.make_world(7, None).opts and LW.make_world(7, 0x12).opts == 0x12
    c = LW.make_world(8)
    assert not all(_same(x, y) for x, y in zip(_fingerprint(LW.make_world(7)), _fingerprint(c)))


def test_fused_worlds_lie_inside_the_fused_calls_bounds():
    for o in LW.OPTS_ALL:
        for s in LW.QUEUE_SEEDS[o]:
            w = LW.make_world(s, o, fused=True)
            assert w.in_fused_bounds() and w.max_batch <= LW.FUSED_MAX and w.complete_max <= LW.FUSED_MAX and w.opts == o
    assert any(not w.in_fused_bounds() for _, _, w, _, _ in _worlds())  # and the others do not all: leg C's refusal


def test_a_shared_pair_keeps_each_worlds_frames_and_measures_against_the_whole_umem():
    a, b = LW.shared_pair(*LW.QUEUE_SEEDS[0x17][:2], 0x17)
    alone = LW.make_world(LW.QUEUE_SEEDS[0x17][1], 0x17, fused=True)
    assert a.umem is b.umem and len(a.umem) == a.own_bytes + b.own_bytes
    assert (b.umem[a.own_bytes:] == alone.umem).all()
    for d, x in zip(b.offers, alone.offers):  # b's descriptors lie behind a's chunks; those that do not fit stay outside
        fits = np.array([SS.descriptor_ok(alone.umem, int(e["addr"]), int(e["len"]), 0x17) for e in x], bool)
        assert (d["addr"][fits] == x["addr"][fits] + np.uint64(a.own_bytes)).all()
        assert not any(SS.descriptor_ok(b.umem, int(e["addr"]), int(e["len"]), 0x17) for e in d[~fits])
    for w, lo, hi in ((a, 0, a.own_bytes), (b, a.own_bytes, len(a.umem))):
        for d in w.offers:
            for e in d:
                if SS.descriptor_ok(w.umem, int(e["addr"]), int(e["len"]), 0x17) and e["len"]:
                    assert lo <= int(e["addr"]) and int(e["addr"]) + int(e["len"]) <= hi
    assert not set(a.pool.addr.tolist()) & set(b.pool.addr.tolist())


def test_a_round_of_the_spec_only_moves_chunk_addresses():
    """Non-garbage worlds: where the pool has room for whatever a round can push (what it receives and what the
    completion rings hold, up to complete_max each), the multiset of chunk addresses over every ring's unconsumed
    entries and the pool below its count is the same after the round; elsewhere nothing appears that was not there."""
    held = 0
    for o, s, w, rounds, _ in _worlds():
        if w.garbage:
            continue
        for r in rounds:
            res = r["got"]["result"]
            want = res["received"] + (sum(min(u, w.complete_max) for u in r["comp_used"]) if w.comps else 0)
            before, after = r["census"], r["census_after"]
            if r["pool_room"] >= want:
                assert after == before, (hex(o), s, r["round"])
                held += 1
            else:
                assert not after - before, (hex(o), s, r["round"])
    assert held >= 40


def coverage():
    """The coverage table of the seed set: {condition: count}, from the spec's output alone."""
    c = Counter()
    per_word = {o: Counter() for o in LW.OPTS_ALL}
    for o, s, w, rounds, _ in _worlds():
        pw = per_word[o]
        pw["worlds"] += 1
        c[f"max_batch {w.max_batch}"] += 1
        c[f"n_ports {w.n_ports}"] += 1
        for name in LW.OUTPUTS:
            c[f"{name} {'present' if w.outputs[name] else 'NULL'}"] += 1
        acts, replies, v6, tx_full, arp, na, backlog = set(), 0, 0, 0, 0, 0, 0
        for r in rounds:
            got, res = r["got"], r["got"]["result"]
            n = res["received"]
            a = got["actions"][:n]
            acts |= set(int(x) for x in a)
            replies += res["replied"]
            v6 += r["families"][6]
            pw["v4 replies"] += r["families"][4]
            tx_full += sum(x["n_tx_full"] for x in got["counts"])
            q = int((a == SS.XDP_PASS).sum())
            assert q == res["passed"] + res["pass_full"]
            if w.garbage:
                continue
            if q:
                c["stack takes none" if res["passed"] == 0 else "stack takes all" if res["passed"] == q else
                  "stack takes some"] += 1
            wants = n - res["replied"] - res["passed"]  # every received frame is on a TX ring, the stack ring or pushed
            assert res["freed"] <= wants
            c["pool drops a tail"] += res["freed"] < wants
            if n and r["fill_free"]:
                c["fill refills none" if res["refilled"] == 0 else "fill refills all" if res["refilled"] == r["fill_free"]
                  else "fill refills part"] += 1
            c["completion drained in part"] += 0 < r["pushed"] < sum(r["moved"])
            below = set(int(x) for x in w.pool.addr[:w.pool.n()])  # (of the world's last round: enough for a count)
            for e, act in zip(got["descs"][:n], a):
                if not SS.descriptor_ok(w.umem, int(e["addr"]), int(e["len"]), 0x17):
                    assert act == SS.XDP_DROP
                    c["bad descriptor dropped"] += 1
                    c["bad descriptor's address on the pool"] += r is rounds[-1] and int(e["addr"]) in below
            c["an index word crosses 2^32"] += r["crossed"]
            c["received == max_batch < offered"] += n == w.max_batch < r["offered"]
            if r["nres"] is not None:
                arp += r["nres"]["arp_replies"]
                na += r["nres"]["na_replies"]
                backlog += r["nres"]["backlog"] > 0
        pw["v6 replies"] += v6
        pw["pass, redirect and a reply"] += (SS.XDP_PASS in acts and SS.XDP_REDIRECT in acts and replies > 0)
        c["worlds where a TX ring cuts a reply"] += tx_full > 0
        c["responder worlds"] += w.up is not None
        c["responder answers ARP and NS"] += arp > 0 and na > 0
        c["responder leaves a backlog"] += backlog > 0
        c["garbage worlds"] += w.garbage
    return c, per_word


def test_the_seed_set_reaches_every_situation():
    c, per_word = coverage()
    print("\ncoverage of the seed set:")
    for k in sorted(c):
        print(f"  {k}: {c[k]}")
    for o in LW.OPTS_ALL:
        print(f"  opts {o:#x}: {dict(per_word[o])}")
    for o, pw in per_word.items():
        assert 3 <= pw["worlds"] <= 6, hex(o)
        assert pw["pass, redirect and a reply"] >= 1, hex(o)
        assert (pw["v6 replies"] >= 1) if o & 0x10 else (pw["v6 replies"] == 0), hex(o)
        assert pw["v4 replies"] >= 1, hex(o)
    assert c["worlds where a TX ring cuts a reply"] >= 6
    for k in ("stack takes none", "stack takes some", "stack takes all", "pool drops a tail", "fill refills none",
              "fill refills part", "fill refills all", "completion drained in part", "bad descriptor dropped",
              "bad descriptor's address on the pool", "an index word crosses 2^32", "received == max_batch < offered",
              "responder answers ARP and NS", "responder leaves a backlog", "garbage worlds"):
        assert c[k] >= 1, k
    for m in LW.MAX_BATCH:
        assert c[f"max_batch {m}"] >= 1, m
    for p in LW.N_PORTS:
        assert c[f"n_ports {p}"] >= 1, p
    for name in LW.OUTPUTS:
        assert c[f"{name} NULL"] >= 2 and c[f"{name} present"] >= 2, name


def test_the_specs_wall_time():
    """Printed, not bounded: what a GPU test id spends in the Python spec (the peers and the three rounds of a world,
    and building the world)."""
    rows = [(sum(r["seconds"] for r in rounds), built, o, s) for o, s, w, rounds, built in _worlds()]
    spec, built, o, s = max(rows)
    print(f"\nslowest world of {len(rows)}: opts {o:#x} seed {s}: spec {spec:.3f} s over {LW.ROUNDS} rounds, "
          f"built in {built:.3f} s; all worlds: spec {sum(r[0] for r in rows):.2f} s, built in "
          f"{sum(r[1] for r in rows):.2f} s")
    assert spec > 0

