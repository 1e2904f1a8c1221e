"""Frames, tables and UMEM layouts for the port-unreachable responder's tests, CPU and GPU.  The frames and what the
responder must make of them come from tests/golden/make_unreach_golden.py (the restatement that builds field by field
and parses nothing), drawn at random for the seeded batches; tests/unreach_spec.py is what they are held against."""
import importlib.util
import json
import os

import numpy as np

import oracle
from tests import unreach_spec as US
from tests.conftest import ROOT

_spec = importlib.util.spec_from_file_location("make_unreach_golden",
                                               os.path.join(ROOT, "tests", "golden", "make_unreach_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

OPTS = G.OPTS
SENTINEL = 0xC3
CHUNK = 2048
N_PORTS, BOUND = G.N_PORTS, G.BOUND
OPEN = frozenset(G.OPEN_PORTS)
_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with open(os.path.join(ROOT, "tests", "golden", "unreach.json")) as f:
            _GOLDEN = json.load(f)
    return _GOLDEN


def table(entries=G.TABLE) -> dict:
    """The golden table as the spec's dict."""
    return {(fam, addr + bytes(16 - len(addr))): (port, mac) for fam, addr, port, mac in entries}


def golden_frames(opts: int):
    """[(frame, room, expectation)] of every golden case under one option word."""
    return [(bytes.fromhex(c["frame"]), c["room"], c["expect"]["0x%x" % opts]) for c in golden()["cases"]]


def random_frames(n: int, opts: int, seed: int):
    """n frames drawn from the generator's cases and tag counts: about half of them from those it says are answered
    under `opts`.  Returns [(frame, room, expectation)]."""
    rng = np.random.default_rng(seed)
    every = [(case, tags) for case in G.CASES for tags in G.TAGS]

    def judged(case, tags):
        name, family, (frame, reply), verdict, room = case
        f = frame(tags)
        r = G.room_of(reply, room, tags)
        return f, r, G.expect(family, verdict, reply, tags, opts, f, r)

    answered = [ct for ct in every if "reply" in judged(*ct)[2]]
    out = []
    for _ in range(n):
        pool = answered if answered and rng.integers(0, 2) else every
        out.append(judged(*pool[int(rng.integers(0, len(pool)))]))
    return out


def layout(frames, rooms=None, chunk: int = CHUNK, short: int = 0):
    """A UMEM of sentinel bytes, a chunk per frame: frame i lies `rooms[i]` bytes in front of its chunk's end, or, with
    None, 1, 2, 0 or 7 bytes behind its beginning (odd and even addresses).  `short` bytes are cut off the UMEM's end (a
    multiple of 16).  Returns (umem, descs)."""
    n = len(frames)
    umem = np.full(max(n * chunk - short, 16), SENTINEL, np.uint8)
    descs = np.zeros(n, oracle.DESC_DTYPE)
    for i, f in enumerate(frames):
        room = None if rooms is None else rooms[i]
        at = i * chunk + ((1, 2, 0, 7)[i & 3] if room is None else chunk - room)
        umem[at:at + len(f)] = np.frombuffer(f, np.uint8)
        descs[i] = (at, len(f), i & 3)
    return umem, descs


def check_condition(verdicts, limited: bool = False):
    """The condition on a random batch, from the spec's output: at least a quarter answered, every verdict present
    (LIMITED too where a budget binds)."""
    v = list(verdicts)
    answered = sum(x in US.REPLIES for x in v)
    assert 4 * answered >= len(v), (answered, len(v))
    assert set(v) == set(range(9 if limited else 8)), sorted(set(v))
