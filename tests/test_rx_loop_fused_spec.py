"""xsk_gpu_rx_fused_loop_dev (Python: rx_loop_fused_dev) without a GPU: the ABI surface and the export-name rules, every
-EINVAL of xsk_gpu_rx_loop_dev reached through the fused call with fabricated pointers (no device call is reached), the
two bounds of the one-workgroup form, the host function's own text (one block of checks, through the function the loop
call checks through, in front of the one launch), and the one-workgroup steering partition and the packed ring form
compiled for the host under AddressSanitizer (tests/c/test_loop_fused.cpp)."""
import errno
import os
import re
import subprocess
import tempfile

from tests.conftest import ROOT
from tests.test_rx_dev_spec import MAX_BATCH, _bad_pools, _bad_rings, _decl, _header, _pool, _ref, _ring
from tests.test_rx_steer_spec import _ports
from tests.test_tx_complete_rings_spec import RESERVED, _comps, _exports, _params

EINVAL = -errno.EINVAL
NAME = "xsk_gpu_rx_fused_loop_dev"
CSRC = os.path.join(ROOT, "xsknet_amd", "csrc")
LOWLAT_MAX = 1024


def test_header_declares_and_library_exports_the_entry_point():
    import xsknet_amd as X
    assert _params("int", NAME) == _params("int", "xsk_gpu_rx_loop_dev")  # the 27 parameters, same order, same names
    assert _decl("int", NAME).count(",") == 26
    assert NAME in _exports() and hasattr(X.lib(), NAME) and NAME in X._SIGS
    assert len(X._SIGS[NAME][0]) == 27 and X._SIGS[NAME] == X._SIGS["xsk_gpu_rx_loop_dev"]
    assert "rx_loop_fused_dev" in X.__all__ and callable(X.rx_loop_fused_dev)
    import inspect
    assert inspect.signature(X.rx_loop_fused_dev) == inspect.signature(X.rx_loop_dev)
    assert X.lib().xsk_gpu_abi_version() == 1 and X.LOWLAT_MAX == LOWLAT_MAX
    assert not re.search(r"struct\s+xsk_gpu_\w*fused\w*\s*\{", _header())  # struct-free: the header gained no struct


def test_the_new_export_keeps_clear_of_the_reserved_names():
    """The one new exported symbol contains no substring an existing test reserves for the existing exports -- "rx_loop"
    among them, which tests/test_tx_complete_rings_spec.py keeps for xsk_gpu_rx_loop_dev -- and is all the library
    gained: everything else of the feature is hidden, static or in an anonymous namespace."""
    assert not [s for s in RESERVED + ("rx_loop", "complete_rings") if s in NAME]
    exported = _exports()
    assert sorted(s for s in exported if "fused" in s) == [NAME]
    src = open(os.path.join(CSRC, "xsk_loop_fused.hip")).read()
    pub = src[src.index('extern "C" {'):]
    assert re.findall(r"^(?:int|size_t) (\w+)\(", pub, re.M) == [NAME]
    mk = open(os.path.join(ROOT, "Makefile")).read()
    for f in ("xsk_loop_fused.o", "xsk_loop_fused_ds.o", "xsk_loop_fused_body.h", "xsk_ring_pack.h"):
        assert f in mk
    assert re.search(r"xsk_loop_fused_ds\.o:.*\n\t.*-pragma-unroll-threshold=32768", mk)


def _loop_fn(X, which):
    L = X.lib()
    rx, fill, stack = _ring(X, 0x100000), _ring(X, 0x200000), _ring(X, 0x300000)
    pool = _pool(X)
    res, st, ws, um, mv, pu = 0x550000, 0x560000, 0x570000, 0x600000, 0x580000, 0x5F0000
    fn = getattr(L, which)

    def loop(rx=rx, fill=fill, tx=None, stack=stack, pool=pool, mb=64, opts=0, np_=3, ws=ws, um=um, size=1 << 20,
             comp=None, nc=4, cm=64, mv=mv, pu=pu, tab=None, ne=0, dp=0, bnd=None, co=None, st=st, pst=None, res=res):
        tx = _ports(X, max(min(np_, 64), 1)) if tx is None else tx
        comp = _comps(X, max(min(nc, 65), 1)) if comp is None else comp
        return fn(um, size, _ref(rx), _ref(fill), tx if tx != 0 else None, _ref(stack), _ref(pool), mb, opts, tab, ne, dp,
                  np_, bnd, None, None, co, st, pst, res, comp if comp != 0 else None, nc, cm, mv, pu, ws, None)

    return loop, (rx, fill, stack, pool, res, st, ws, um, mv, pu)


def test_every_einval_of_the_loop_call_through_the_fused_call():
    """The lists of tests/test_tx_complete_rings_spec.py (the completion call's rules, the aliasing with the step's
    rings) and tests/test_rx_pass_spec.py (the step's rules), each reached through the fused call."""
    import xsknet_amd as X
    loop, (rx, fill, stack, pool, res, st, ws, um, mv, pu) = _loop_fn(X, NAME)
    co, pst, tab, bnd = 0x540000, 0x5E0000, 0x5B0000, 0x5C0000
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
    for cm in (0, 64, 1024):
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
                for n, at in ((1, 0), (3, 2), (64, 63)):
                    t = _ports(X, n)
                    t[at] = b
                    assert loop(tx=t, np_=n, comp=comp, nc=nc) == EINVAL
        for b in _bad_rings(X, 0x200000, 8):
            assert loop(fill=b, comp=comp, nc=nc) == EINVAL
        for b in _bad_pools(X):
            assert loop(pool=b, comp=comp, nc=nc) == EINVAL
        assert loop(tx=0, comp=comp, nc=nc) == EINVAL
        for n in (0, 65, 0xFFFFFFFF):
            assert loop(np_=n, comp=comp, nc=nc) == EINVAL
        for n, a, b in ((2, 0, 1), (64, 5, 63)):  # two ports that share an entry array or a producer word
            for f in ("d_ring", "d_producer"):
                t = _ports(X, n)
                setattr(t[b], f, getattr(t[a], f))
                assert loop(tx=t, np_=n, comp=comp, nc=nc) == EINVAL
        for other in (rx, *_ports(X, 3)):  # the stack ring's aliasing rules
            for f in ("d_ring", "d_producer"):
                s = _ring(X, 0x300000)
                setattr(s, f, getattr(other, f))
                assert loop(stack=s, comp=comp, nc=nc) == EINVAL, f
        for mb in (0, MAX_BATCH + 1, 0xFFFFFFFF):
            assert loop(mb=mb, comp=comp, nc=nc) == EINVAL
        for opts in (0x8, 0x20, 0x18, 0xFFFFFFFF):
            assert loop(opts=opts, comp=comp, nc=nc) == EINVAL
        for mis in (1, 2, 4, 8):
            assert loop(ws=ws + mis, comp=comp, nc=nc) == EINVAL and loop(um=um + mis, comp=comp, nc=nc) == EINVAL
            assert loop(size=(1 << 20) + mis, comp=comp, nc=nc) == EINVAL
        for mis in (1, 2, 4):
            assert loop(st=st + mis, comp=comp, nc=nc) == EINVAL and loop(pst=pst + mis, comp=comp, nc=nc) == EINVAL
            assert loop(bnd=bnd + mis, comp=comp, nc=nc) == EINVAL and loop(tab=tab + mis, ne=4, comp=comp, nc=nc) == EINVAL
        for mis in (1, 2, 3):
            assert loop(res=res + mis, comp=comp, nc=nc) == EINVAL and loop(co=co + mis, comp=comp, nc=nc) == EINVAL
        assert loop(ws=None, comp=comp, nc=nc) == EINVAL and loop(um=None, comp=comp, nc=nc) == EINVAL
        assert loop(size=1 << 48, comp=comp, nc=nc) == EINVAL
        for dp in (3, 64, 0xFE, 0x100):
            assert loop(dp=dp, comp=comp, nc=nc) == EINVAL
        assert loop(ne=1025, tab=tab, comp=comp, nc=nc) == EINVAL and loop(ne=1, tab=None, comp=comp, nc=nc) == EINVAL
    # n_comp == 0 ignores comp, complete_max and the two outputs: only the step's rules are left
    assert loop(comp=0, nc=0, cm=0xFFFFFFFF, mv=mv + 1, pu=pu + 2, ws=None) == EINVAL


def test_the_loop_call_still_refuses_what_it_refused():
    """The loop call checks through the shared function now: a sample of each group of its rules, as before."""
    import xsknet_amd as X
    loop, (rx, fill, stack, pool, res, st, ws, um, mv, pu) = _loop_fn(X, "xsk_gpu_rx_loop_dev")
    assert loop(comp=0) == EINVAL and loop(cm=MAX_BATCH + 1) == EINVAL and loop(mv=mv + 2) == EINVAL
    comp = _comps(X, 4)
    comp[2].d_ring = rx.d_ring
    assert loop(comp=comp) == EINVAL
    for nc, comp in ((4, None), (0, 0)):
        assert loop(rx=None, comp=comp, nc=nc) == EINVAL and loop(mb=0, comp=comp, nc=nc) == EINVAL
        assert loop(opts=0x8, comp=comp, nc=nc) == EINVAL and loop(ws=ws + 8, comp=comp, nc=nc) == EINVAL
        assert loop(dp=3, comp=comp, nc=nc) == EINVAL and loop(np_=65, comp=comp, nc=nc) == EINVAL


def test_the_bounds_of_the_one_workgroup_form():
    import xsknet_amd as X
    loop, (rx, fill, stack, pool, res, st, ws, um, mv, pu) = _loop_fn(X, NAME)
    for mb in (LOWLAT_MAX + 1, 1300, 70000, MAX_BATCH):
        assert loop(mb=mb) == EINVAL and loop(mb=mb, comp=0, nc=0) == EINVAL
    for cm in (LOWLAT_MAX + 1, 1300, MAX_BATCH):
        assert loop(cm=cm, nc=1) == EINVAL and loop(cm=cm, nc=65) == EINVAL
    # a ring the packed kernel arguments cannot carry (an entry array at or above 2^56) is refused with the rules
    assert loop(rx=_ring(X, 0x100000, d_ring=1 << 56)) == EINVAL
    t = _ports(X, 3)
    t[2].d_ring = (1 << 60) + 0x1000
    assert loop(tx=t) == EINVAL
    comp = _comps(X, 4)
    comp[3].d_ring = 0xFF00000000001000
    assert loop(comp=comp) == EINVAL


def test_every_rule_stands_in_front_of_the_one_launch():
    """The host function's own text, as the existing spec tests read theirs: one -EINVAL, from one block of checks, before
    anything that launches; the checks are the loop call's own function and the two bounds, of which complete_max's
    holds only with completion rings (complete_max 1025 with n_comp 0 passes the argument check); one kernel launch
    and nothing else is enqueued -- no memset, no copy, no allocation, no synchronisation; no inline assembly, no
    atomic that hands out a slot, no __restrict__ in the fused kernel's own files."""
    src = open(os.path.join(CSRC, "xsk_loop_fused.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    pub = code[code.index('extern "C" {'):]
    body = pub[pub.index("int " + NAME + "("):]
    body = body[:body.index("\n}\n")]
    assert body.count("return -EINVAL") == 1 and body.index("return -EINVAL") < body.index("_launch(")
    assert body.index("fused_ok(") < body.index("return -EINVAL")
    ok = code[code.index("bool fused_ok("):code.index("int fused_launch(")]
    assert ok.index("loop_complete_ok(") < ok.index("max_batch > kLfMax")
    assert re.search(r"max_batch > kLfMax \|\| \(n_comp && complete_max > kLfMax\)", ok)
    launch = code[code.index("int fused_launch("):code.index('extern "C" {')]
    assert launch.count("<<<") == 2 and launch.count("xsk_gpu__loop_fused_ds_launch(") == 1
    for f in ("xsk_loop_fused.hip", "xsk_loop_fused_ds.hip", "xsk_loop_fused_body.h"):
        c = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())
        for word in ("hipMemsetAsync", "hipMemcpy", "hipMalloc", "Synchronize", "asm", "atomicAdd", "__restrict__"):
            assert word not in c, (f, word)
    # the loop call checks through the same function
    ring = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "xsk_ring_complete.hip")).read())
    assert "loop_complete_ok(" in ring[ring.index("int xsk_gpu_rx_loop_dev("):]
    hdr = open(os.path.join(CSRC, "xsk_loop_fused_body.h")).read()
    assert re.search(r"static_assert\(sizeof\(LoopFusedArgs\) \+ 256 <= 4096", hdr)
    assert re.search(r"static_assert\(sizeof\(LoopFusedLds\) <= 160u \* 1024u", hdr)
    assert "__launch_bounds__(kLfThreads, 1)" in src and re.search(r"kLfThreads\s*=\s*1024\b", hdr)


def test_steering_slots_and_packed_rings_on_the_host_under_address_sanitizer():
    """tests/c/test_loop_fused.cpp: the one-workgroup steering partition of xsk_steer.h replayed lane by lane into heap
    arrays of exactly the REDIRECT count and n_ports + 1 offsets, against std::stable_sort; the packed ring form
    round-tripped for sizes 1, 2, ... 2^31 and pointers with bit 47 set.  A stand-alone program: nothing loaded into
    Python runs under a sanitizer."""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "t")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "c", "test_loop_fused.cpp")], check=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    assert "loop fused ok" in res.stdout
