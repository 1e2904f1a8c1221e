"""Frames, tables and UMEM layouts for the neighbour responder's tests, CPU and GPU.  The frames and what the responder
must make of them come from tests/golden/make_neigh_golden.py (the restatement that builds field by field and parses
nothing), drawn at random for the seeded batches; tests/neigh_spec.py is what they are held against."""
import importlib.util
import json
import os

import numpy as np

import oracle
from tests import neigh_spec as NS
from tests.conftest import ROOT

_spec = importlib.util.spec_from_file_location("make_neigh_golden",
                                               os.path.join(ROOT, "tests", "golden", "make_neigh_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

OPTS = G.OPTS
SENTINEL = 0xC3
N_PORTS, BOUND = G.N_PORTS, G.BOUND
_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with open(os.path.join(ROOT, "tests", "golden", "neigh.json")) as f:
            _GOLDEN = json.load(f)
    return _GOLDEN


def table(entries=G.TABLE) -> dict:
    """The golden table as neigh_spec's dict."""
    return {(fam, addr + bytes(16 - len(addr))): (port, mac) for fam, addr, port, mac in entries}


def big_table(n: int, seed: int = 1) -> dict:
    """A table of exactly n entries: the golden table's (as many as fit), then seeded strangers around them."""
    rng = np.random.default_rng(seed)
    t = dict(list(table().items())[:n])
    while len(t) < n:
        fam = 4 if rng.integers(0, 2) else 6
        addr = bytes(rng.integers(1, 255, 4 if fam == 4 else 16, dtype=np.uint8))
        if fam == 6 and addr[0] == 0xFF:
            continue
        key = (fam, addr + bytes(16 - len(addr)))
        if key[1][:4] in (G.STRANGER4,) or key[1] == G.STRANGER6:
            continue
        t.setdefault(key, (int(rng.integers(0, 64)), bytes([2]) + bytes(rng.integers(0, 256, 5, dtype=np.uint8))))
    return t


def golden_frames(opts: int):
    """[(frame, expectation)] of every golden case under one option word."""
    return [(bytes.fromhex(c["frame"]), c["expect"]["0x%x" % opts]) for c in golden()["cases"]]


def random_frames(n: int, opts: int, seed: int):
    """n frames drawn from the generator's cases and tag counts: about half of them from those it says are answered
    under `opts`.  Returns [(frame, expectation)]."""
    rng = np.random.default_rng(seed)
    every = [(case, tags) for case in G.CASES for tags in G.TAGS]
    answered = [(case, tags) for case, tags in every
                if "reply" in G.expect(case[1], case[3], case[2][1], tags, opts, case[2][0](tags))]
    out = []
    for _ in range(n):
        pool = answered if answered and rng.integers(0, 2) else every
        (name, family, (frame, reply), verdict), tags = pool[int(rng.integers(0, len(pool)))]
        f = frame(tags)
        out.append((f, G.expect(family, verdict, reply, tags, opts, f)))
    return out


def layout(frames, gap: int = 7, odd: bool = True, tail: int = 0):
    """A UMEM of sentinel bytes with the frames in it, `gap` sentinel bytes apart and (odd) at odd addresses; the last
    frame ends `tail` bytes before the UMEM's end, padded in front so that the size stays a multiple of 16.  Returns
    (umem, descs)."""
    addrs, a = [], 1 if odd else 0
    for f in frames:
        if odd and a % 2 == 0:
            a += 1
        addrs.append(a)
        a += len(f) + gap
    end = addrs[-1] + len(frames[-1]) + tail if frames else 16
    size = max((end + 15) // 16 * 16, 16)
    if frames and tail == 0:
        addrs[-1] = size - len(frames[-1])  # the last frame ends at the UMEM's last byte
    umem = np.full(size, SENTINEL, np.uint8)
    descs = np.zeros(len(frames), oracle.DESC_DTYPE)
    for i, (f, at) in enumerate(zip(frames, addrs)):
        umem[at:at + len(f)] = np.frombuffer(f, np.uint8)
        descs[i] = (at, len(f), i & 3)
    return umem, descs


def check_condition(verdicts):
    """The condition on a random batch, from the spec's output: at least a quarter answered, every verdict present."""
    v = list(verdicts)
    answered = sum(x in (NS.ARP_REPLY, NS.NA_REPLY) for x in v)
    assert 4 * answered >= len(v), (answered, len(v))
    assert set(v) == set(range(7)), sorted(set(v))
