"""Randomised parity of xsk_gpu_responder_dev and xsk_gpu_responder_queues_dev under every option word:
the 32 worlds of tests/responder_seeds.py (two an option word, every one with a responder attached), three rounds each,
the peers (loop_world.peers) acting on every leg and on the spec in between.

    leg R   xsk_gpu_responder_dev
    leg C   tests/test_gpu_loop_fuzz.py's own: xsk_gpu_rx_fused_loop_dev, then xsk_gpu_neigh_serve_dev
    leg Q   the two worlds of the option word as the two queues of one xsk_gpu_responder_queues_dev call a round, over a
            block prepared once

After every round each leg is held against the spec (Leg.hold: every ring entry and index word, the pool, every UMEM
byte, every output, the responder's result and counters, every sentinel) and against leg C byte for byte.  Every
comparison is exact; a failure names seed, option word, round and leg; a seed is never retried.
tests/test_responder_spec.py asserts from the spec alone what this seed set reaches."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import loop_world as LW  # noqa: E402
from tests import responder_seeds as SEEDS  # noqa: E402
from tests.responder_dev import RLeg, problems, responder_block, same_bytes  # noqa: E402
from tests.test_gpu_ingress import _dev  # noqa: E402
from tests.test_gpu_loop_fuzz import Leg  # noqa: E402


@pytest.mark.parametrize("opts", LW.OPTS_ALL, ids=[f"{o:#x}" for o in LW.OPTS_ALL])
def test_two_worlds_an_option_word(opts):
    _dev()
    seeds = SEEDS.seeds(opts)
    worlds = [LW.make_world(s, opts, fused=True) for s in seeds]
    assert all(w.up is not None and w.in_fused_bounds() for w in worlds)
    legs = [{"R": RLeg(w), "C": Leg(w), "Q": RLeg(w)} for w in worlds]
    d_block = responder_block([x["Q"] for x in legs], opts)
    for k in range(LW.ROUNDS):
        rounds = []
        for w, x in zip(worlds, legs):
            touched = LW.peers(w, k)
            for leg in x.values():  # (before the spec's round changes the rings it is copied from)
                leg.follow(touched)
            rounds.append(LW.spec_round(w))
        for x in legs:
            x["R"].responder()
            x["C"].fused()
        X.responder_queues_dev(d_block, len(worlds), opts)
        torch.cuda.synchronize()
        wrong = []
        for w, x, r in zip(worlds, legs, rounds):
            for name, leg in x.items():
                wrong += problems(f"seed {w.seed} leg {name}", leg.hold, r)
            for name in ("R", "Q"):
                wrong += problems(f"seed {w.seed} leg {name} against leg C", same_bytes, x["C"], x[name])
        assert not wrong, f"opts {opts:#x} round {k}: " + " | ".join(wrong)
