"""xsk_gpu_tx_complete_rings_dev / xsk_gpu_rx_loop_dev without a GPU: the ABI surface and the export-name rule, the
argument checks (fabricated pointers, no device call reached; the aliasing rules among the completion rings and, in the
loop call, with the step's rings), the numpy spec (tests/tx_complete_rings_spec.py) stated twice and held against itself
and against the real host xsk_gpu_tx_complete() called ring after ring on host rings, and the ring arithmetic of both
kernel paths compiled for the host under AddressSanitizer (tests/c/test_ring_complete.cpp)."""
import ctypes as C
import errno
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import rx_dev_spec as RS
from tests import tx_complete_rings_spec as CS
from tests.conftest import ROOT
from tests.test_rx_dev_spec import MAX_BATCH, _bad_pools, _bad_rings, _decl, _header, _host_ring, _pool, _ref, _ring
from tests.test_rx_steer_spec import _ports

EINVAL = -errno.EINVAL
NAMES = ("xsk_gpu_tx_complete_rings_dev", "xsk_gpu_rx_loop_dev")
# substrings that existing tests reserve for existing exports
RESERVED = ("ring_dev", "rx_begin", "rx_end", "rx_step_dev", "tx_complete_dev", "rd_", "ring_ports", "rx_prepare", "rx_ports",
            "rx_step_steer", "rp_", "pass", "egress")
SRC = os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_ring_complete.hip")


def _params(ret, name):
    return _decl(ret, name).replace(" ,", ",")


def _exports():
    import xsknet_amd as X
    out = subprocess.run(["nm", "-D", "--defined-only", X.LIB_PATH], capture_output=True, text=True, check=True)
    return re.findall(r"\bT (\w+)", out.stdout)


def test_header_declares_and_library_exports_the_entry_points():
    import xsknet_amd as X
    R, P = "const struct xsk_gpu_ring_dev*", "const struct xsk_gpu_pool_dev*"
    assert _params("int", "xsk_gpu_tx_complete_rings_dev") == (
        f"{R} comp, uint32_t n_rings, {P} pool, uint32_t max, uint32_t* d_moved, uint32_t* d_pushed, void* stream")
    step = _params("int", "xsk_gpu_rx_pass_step_dev")
    head, tail = step.split(", void* d_workspace, ")
    assert _params("int", "xsk_gpu_rx_loop_dev") == (
        f"{head}, {R} comp, uint32_t n_comp, uint32_t complete_max, uint32_t* d_moved, uint32_t* d_pushed, "
        f"void* d_workspace, {tail}")
    assert re.search(r"#define\s+XSK_GPU_COMPLETE_MAX_RINGS\s+65u\b", _header())
    assert X.COMPLETE_MAX_RINGS == 65 == X.STEER_MAX_PORTS + 1 == CS.MAX_RINGS
    exported = _exports()
    for name in NAMES:
        assert name in exported and hasattr(X.lib(), name) and name in X._SIGS, name
    for f in ("COMPLETE_MAX_RINGS", "tx_complete_rings_dev", "rx_loop_dev"):
        assert f in X.__all__
    assert callable(X.tx_complete_rings_dev) and callable(X.rx_loop_dev)
    assert [len(X._SIGS[n][0]) for n in NAMES] == [7, 27]
    # struct-free ABI: the calls take the structs that exist, the header gained none
    assert X._SIGS[NAMES[1]][0][:20] == X._SIGS["xsk_gpu_rx_pass_step_dev"][0][:20]
    assert X._SIGS[NAMES[1]][0][25:] == X._SIGS["xsk_gpu_rx_pass_step_dev"][0][20:]
    assert X.lib().xsk_gpu_abi_version() == 1
    assert not re.search(r"struct\s+xsk_gpu_\w*(complete|loop)\w*\s*\{", _header())


def test_the_new_exports_keep_clear_of_the_reserved_names():
    """No new exported symbol contains a substring that an existing test reserves; everything else of the feature is
    static or in an anonymous namespace, so the two entry points are all the library gained."""
    for name in NAMES:
        assert not [s for s in RESERVED if s in name], name
    src = open(SRC).read()
    pub = src[src.index('extern "C" {'):]
    assert sorted(re.findall(r"^(?:int|size_t) (\w+)\(", pub, re.M)) == sorted(NAMES)
    assert sorted(s for s in _exports() if "complete_rings" in s or "rx_loop" in s) == sorted(NAMES)
    for obj in ("xsk_ring_complete.o", "xsk_ring_complete.h"):
        assert obj in open(os.path.join(ROOT, "Makefile")).read()


# ---- the argument rules ------------------------------------------------------------------------------------------

def _comps(X, n, base=0x2000000):
    return _ports(X, n, base)


def test_argument_validation_needs_no_gpu():
    import xsknet_amd as X
    L = X.lib()
    pool = _pool(X)
    mv, pu = 0x580000, 0x5F0000

    def complete(comp=None, n=3, pool=pool, mx=64, mv=mv, pu=pu):
        comp = _comps(X, max(min(n, 65), 1)) if comp is None else comp
        return L.xsk_gpu_tx_complete_rings_dev(comp if comp != 0 else None, n, _ref(pool), mx, mv, pu, None)

    assert complete(comp=0) == EINVAL
    for n in (0, 66, 0xFFFFFFFF):
        assert complete(n=n) == EINVAL
    for b in _bad_rings(X, 0x2000000, 8):
        if b is None:
            continue
        for n, at in ((1, 0), (3, 2), (65, 64), (65, 31)):
            comp = _comps(X, n)
            comp[at] = b
            assert complete(comp=comp, n=n) == EINVAL
    for n, a, b in ((2, 0, 1), (65, 5, 64), (65, 63, 64)):
        for f in ("d_ring", "d_consumer"):
            comp = _comps(X, n)
            setattr(comp[b], f, getattr(comp[a], f))
            assert complete(comp=comp, n=n) == EINVAL, f
    for b in _bad_pools(X):
        assert complete(pool=b) == EINVAL
    for mx in (MAX_BATCH + 1, 0xFFFFFFFF):
        assert complete(mx=mx) == EINVAL
    for mx in (0, 64, 1024, 1025, 70000):  # both paths and the empty call refuse alike
        for mis in (1, 2, 3):
            assert complete(mx=mx, mv=mv + mis) == EINVAL and complete(mx=mx, pu=pu + mis) == EINVAL
        assert complete(mx=mx, comp=0) == EINVAL and complete(mx=mx, pool=None) == EINVAL and complete(mx=mx, n=66) == EINVAL


def test_the_loop_call_checks_both_calls_rules_and_the_aliasing_with_the_steps_rings():
    import xsknet_amd as X
    L = X.lib()
    rx, fill, stack = _ring(X, 0x100000), _ring(X, 0x200000), _ring(X, 0x300000)
    pool = _pool(X)
    res, st, ws, um, mv, pu = 0x550000, 0x560000, 0x570000, 0x600000, 0x580000, 0x5F0000

    def loop(rx=rx, fill=fill, tx=None, stack=stack, pool=pool, mb=64, opts=0, np_=3, ws=ws, um=um, comp=None, nc=4, cm=64,
             mv=mv, pu=pu):
        tx = _ports(X, max(min(np_, 64), 1)) if tx is None else tx
        comp = _comps(X, max(min(nc, 65), 1)) if comp is None else comp
        return L.xsk_gpu_rx_loop_dev(um, 1 << 20, _ref(rx), _ref(fill), tx if tx != 0 else None, _ref(stack), _ref(pool),
                                     mb, opts, None, 0, 0, np_, None, None, None, None, st, None, res,
                                     comp if comp != 0 else None, nc, cm, mv, pu, ws, None)

    # the completion call's rules
    assert loop(comp=0) == EINVAL and loop(nc=66) == EINVAL and loop(nc=0xFFFFFFFF) == EINVAL
    for b in _bad_rings(X, 0x2000000, 8):
        if b is not None:
            comp = _comps(X, 65)
            comp[64] = b
            assert loop(comp=comp, nc=65) == EINVAL
    for f in ("d_ring", "d_consumer"):
        comp = _comps(X, 4)
        setattr(comp[3], f, getattr(comp[1], f))
        assert loop(comp=comp) == EINVAL
    for cm in (MAX_BATCH + 1, 0xFFFFFFFF):
        assert loop(cm=cm) == EINVAL
    for cm in (0, 64, 1300):
        for mis in (1, 2, 3):
            assert loop(cm=cm, mv=mv + mis) == EINVAL and loop(cm=cm, pu=pu + mis) == EINVAL
    # a completion ring that shares d_ring or d_consumer with rx, fill, the stack ring or a port's ring
    tx = _ports(X, 64)
    for other in (rx, fill, stack, tx[0], tx[17], tx[63]):
        for f in ("d_ring", "d_consumer"):
            for n, at in ((1, 0), (65, 64), (65, 9)):
                comp = _comps(X, n)
                setattr(comp[at], f, getattr(other, f))
                assert loop(tx=tx, np_=64, comp=comp, nc=n) == EINVAL, f
    # the step's rules, with completion rings and without (n_comp == 0: comp and the outputs are ignored)
    for nc, comp in ((4, None), (0, 0)):
        for b in _bad_rings(X, 0x100000, 16):
            assert loop(rx=b, comp=comp, nc=nc) == EINVAL
            if b is not None:
                assert loop(stack=b, comp=comp, nc=nc) == EINVAL
                t = _ports(X, 3)
                t[2] = b
                assert loop(tx=t, comp=comp, nc=nc) == EINVAL
        for b in _bad_rings(X, 0x200000, 8):
            assert loop(fill=b, comp=comp, nc=nc) == EINVAL
        for b in _bad_pools(X):
            assert loop(pool=b, comp=comp, nc=nc) == EINVAL
        assert loop(tx=0, comp=comp, nc=nc) == EINVAL
        for n in (0, 65, 0xFFFFFFFF):
            assert loop(np_=n, comp=comp, nc=nc) == EINVAL
        for mb in (0, MAX_BATCH + 1):
            assert loop(mb=mb, comp=comp, nc=nc) == EINVAL
        for opts in (0x8, 0x20, 0xFFFFFFFF):
            assert loop(opts=opts, comp=comp, nc=nc) == EINVAL
        assert loop(ws=None, comp=comp, nc=nc) == EINVAL and loop(ws=ws + 8, comp=comp, nc=nc) == EINVAL
        assert loop(um=None, comp=comp, nc=nc) == EINVAL
    # n_comp == 0 ignores comp, complete_max and the two outputs: only the step's rules are left
    assert loop(comp=0, nc=0, cm=0xFFFFFFFF, mv=mv + 1, pu=pu + 2, ws=None) == EINVAL


def test_every_rule_stands_in_front_of_the_first_device_call():
    """The host functions' own text: each public call returns -EINVAL from one block of checks before anything that
    launches -- in the loop call before the step, which launches -- and the file stores through no inline assembly,
    hands out no slot by an atomic and reads its index words through load_word."""
    src = open(SRC).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "asm" not in code and "atomicAdd" not in code and "atomic_fetch" not in code and "__restrict__" not in code
    pub = code[code.index('extern "C" {'):]
    for name in NAMES:
        body = pub[pub.index("int " + name + "("):]
        body = body[:body.index("\n}\n")]
        first = min(body.index(t) for t in ("_launch(", "<<<", "hipMemsetAsync", "xsk_gpu_rx_pass_step_dev(") if t in body)
        assert body.count("return -EINVAL") == 1 and body.index("return -EINVAL") < first, name
    loop = pub[pub.index("int xsk_gpu_rx_loop_dev("):]
    assert loop.index("complete_ok(") < loop.index("xsk_gpu_rx_pass_step_dev(d_umem") < loop.index("complete_launch(")
    assert "<<<" not in pub and "hipMemsetAsync" not in pub  # the launches live behind the checks, in complete_launch()
    for word in ("ring.cons", "ring.prod", "pool.n_free"):
        assert f"load_word({word})" in code
    hdr = open(os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_ring_complete.h")).read()
    assert re.search(r"kRcMaxRings\s*=\s*kEpMaxPorts \+ 1u", hdr) and re.search(r"kRcPublish\s*=\s*128\b", hdr)


# ---- the spec ----------------------------------------------------------------------------------------------------

def _state(n_rings, sizes, useds, start, room, below=3, seed=0):
    """n_rings completion rings (sizes and fill levels cycled), consumer words near `start`, and a pool with `below`
    frames on it and `room` free entries."""
    rng = np.random.default_rng(seed + n_rings)
    comps = []
    for q in range(n_rings):
        size = sizes[q % len(sizes)]
        used = min(useds[q % len(useds)], size)
        comps.append(RS.RingState((np.arange(size, dtype=np.uint64) + np.uint64(1 + (q << 16))) * np.uint64(4096),
                                  start + 3 * q + used, start + 3 * q))
    cap = max(below + room, 1)
    pool = RS.PoolState(rng.integers(1, 1 << 40, cap, dtype=np.uint64), min(below, cap))
    return comps, pool


def _both(comps, pool, mx):
    """Both formulations from copies of the state; asserts they agree and returns what they leave."""
    a, pa = [c.copy() for c in comps], pool.copy()
    b, pb = [c.copy() for c in comps], pool.copy()
    ra = CS.spec_complete_rings(a, pa, mx)
    rb = CS.spec_complete_rings_prefix(b, pb, mx)
    assert ra == rb and pa.same(pb) and all(x.same(y) for x, y in zip(a, b))
    return a, pa, ra


@pytest.mark.parametrize("start", [0, 5, 0xFFFFFFFD])
@pytest.mark.parametrize("n_rings", [1, 2, 3, 64, 65])
def test_both_formulations_agree_with_each_other_and_with_the_host_function_ring_after_ring(n_rings, start):
    """used 0 / 1 / partial / full mixed in one call; max below, at and above what a ring holds; a pool with room for
    nothing, one, a cut strictly inside a ring, a cut on a ring boundary and all."""
    import xsknet_amd as X
    sizes, useds = [8, 1, 64, 16, 4], [0, 1, 5, 64, 3, 16]
    for mx in (1, 4, 7, 64, 1024):
        probe, _ = _state(n_rings, sizes, useds, start, 0)
        n = [min(c.used(), mx) for c in probe]
        total = sum(n)
        inside = next((sum(n[:q]) + n[q] // 2 for q in range(n_rings) if n[q] >= 2), total)
        boundary = next((sum(n[:q + 1]) for q in range(n_rings - 1) if n[q] and sum(n[:q + 1]) < total), total)
        for room in sorted({0, 1, inside, boundary, total, total + 9}):
            comps, pool = _state(n_rings, sizes, useds, start, room)
            got, gp, (moved, pushed) = _both(comps, pool, mx)
            assert moved == n and pushed == min(total, room) and gp.n_free == pool.n_free + pushed
            # the host function, ring after ring, over one host pool
            stack = pool.addr.copy()
            hp = X.FramePool(stack.ctypes.data, pool.n_free, pool.capacity)
            for q, c in enumerate(comps):
                view, ctr, slots = _host_ring(c, True)
                assert X.lib().xsk_gpu_tx_complete(C.byref(view), C.byref(hp), mx) == moved[q]
                assert (int(ctr[0]), int(ctr[1])) == (got[q].prod, got[q].cons) and (slots == got[q].entries).all()
            assert hp.n_free == gp.n_free and (stack[:hp.n_free] == gp.addr[:gp.n_free]).all()
            # order: ring order, inside a ring the ring's own
            want = [int(c.entries[c.slot(c.cons + j)]) for q, c in enumerate(comps) for j in range(n[q])][:pushed]
            assert [int(a) for a in gp.addr[pool.n_free:gp.n_free]] == want


def test_one_ring_is_the_single_ring_rule():
    for used, room, mx in ((0, 5, 4), (5, 2, 9), (8, 100, 3), (8, 0, 8)):
        comps, pool = _state(1, [8], [used], 0xFFFFFFFD, room)
        one, p1 = comps[0].copy(), pool.copy()
        n = RS.spec_complete(one, p1, mx)
        got, gp, (moved, pushed) = _both(comps, pool, mx)
        assert moved == [n] and got[0].same(one) and gp.same(p1) and pushed == p1.n_free - pool.n_free


def test_max_zero_changes_nothing():
    comps, pool = _state(3, [8, 16], [3, 16], 0xFFFFFFFD, 10)
    pool.n_free = pool.capacity + 7  # no word is stored: the count is not even clamped
    got, gp, (moved, pushed) = _both(comps, pool, 0)
    assert moved == [0, 0, 0] and pushed == 0 and gp.n_free == pool.n_free
    assert all(x.same(y) for x, y in zip(got, comps))


def test_garbage_words_are_clamped():
    """prod - cons > size reads as a full ring, a count word above the capacity as a full pool that ends clamped; with
    room, 65 rings whose words hold anything."""
    comps, pool = _state(3, [8], [8], 5, 0, below=4)
    comps[1].prod = (comps[1].cons + 0x80000005) & RS.M32
    pool.n_free = 77
    got, gp, (moved, pushed) = _both(comps, pool, 100)
    assert moved == [8, 8, 8] and pushed == 0 and gp.n_free == 4
    assert [c.cons for c in got] == [(c.cons + 8) & RS.M32 for c in comps]
    rng = np.random.default_rng(5)
    for _ in range(30):
        comps, pool = _state(65, [1, 2, 32, 128], [0], 0, int(rng.integers(0, 3000)))
        for c in comps:
            c.prod, c.cons = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
        if rng.integers(0, 2):
            pool.n_free = int(rng.integers(0, 1 << 32))
        _, gp, (moved, pushed) = _both(comps, pool, int(rng.choice([1, 50, 1024, 1300, MAX_BATCH])))
        assert gp.n_free <= gp.capacity and pushed <= sum(moved)


def test_consumer_words_three_below_the_wrap():
    comps, pool = _state(3, [16], [9, 16, 2], 0xFFFFFFFD, 100)
    for q, c in enumerate(comps):
        c.prod, c.cons = (0xFFFFFFFD + min([9, 16, 2][q], 16)) & RS.M32, 0xFFFFFFFD
    got, gp, (moved, pushed) = _both(comps, pool, 1024)
    assert moved == [9, 16, 2] and pushed == 27 and [c.cons for c in got] == [6, 13, 0xFFFFFFFF]
    want = [int(c.entries[(0xFFFFFFFD + j) & 15]) for q, c in enumerate(comps) for j in range(moved[q])]
    assert [int(a) for a in gp.addr[pool.n_free:gp.n_free]] == want


def test_ring_arithmetic_on_the_host_under_address_sanitizer():
    """tests/c/test_ring_complete.cpp: xsk_ring_complete.h's shares, prefix, owners, slots and grids, both paths replayed
    lane by lane into heap arrays of exactly the rings' and the pool's sizes, against the rule stated sequentially; the
    case matrix of its header comment.  A stand-alone program: nothing loaded into Python runs under a sanitizer."""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "t")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "c", "test_ring_complete.cpp")], check=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    assert "ring complete ok" in res.stdout
