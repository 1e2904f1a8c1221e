"""The seed set of the responder's randomised tests: for each option word o of loop_world.OPTS_ALL the
first two seeds 700000 + 1000 * o + k, k = 0, 1, 2, ..., whose fused world has a responder attached (make_world(s, o,
fused=True).up is not None) -- 32 worlds.  Plain Python: nothing here touches a GPU.  tests/test_responder_spec.py holds
the set against what it must reach; tests/test_gpu_responder_fuzz.py drives the device calls from it."""
import functools

from tests import loop_world as LW

BASE = 700000
PER_WORD = 2


@functools.lru_cache(maxsize=None)
def seeds(opts):
    found, k = [], 0
    while len(found) < PER_WORD:
        s = BASE + 1000 * opts + k
        if LW.make_world(s, opts, fused=True).up is not None:
            found.append(s)
        k += 1
        assert k < 1000, "the draw attaches a responder to one world in three"
    return tuple(found)


def seed_set():
    return {o: seeds(o) for o in LW.OPTS_ALL}
