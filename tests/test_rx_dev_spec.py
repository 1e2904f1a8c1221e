"""xsk_gpu_rx_begin_dev / xsk_gpu_rx_end_dev / xsk_gpu_rx_step_dev / xsk_gpu_tx_complete_dev without a GPU: the ABI
surface, the argument checks (fabricated pointers, no device call reached), the Python spec (tests/rx_dev_spec.py)
against the real host xsk_gpu_tx_complete() and against its own identities, and the ring arithmetic of both kernel paths
compiled for the host under AddressSanitizer (tests/c/test_ring_dev.cpp)."""
import ctypes as C
import errno
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from tests import egress_spec as ES
from tests import ingress_spec as IS
from tests import rx_dev_spec as RS
from tests.conftest import ROOT

EINVAL = -errno.EINVAL
MAX_BATCH = 0xFFFFFF00
NAMES = ("xsk_gpu_rx_begin_dev", "xsk_gpu_rx_end_dev", "xsk_gpu_rx_step_dev", "xsk_gpu_tx_complete_dev",
         "xsk_gpu_rx_step_dev_workspace_size")


def _header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xsk_gpu.h")).read(), flags=re.S)
    assert re.search(r"#define\s+XSK_GPU_ABI_VERSION\s+1\b", src)
    assert re.search(r"#define\s+XSK_GPU_OPT_MASK\s+0x17u\b", src)  # additive: no new version, no new option bits
    return src


def _decl(ret, name):
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)", _header())
    assert m, f"{name} is not declared"
    return re.sub(r"\s+", " ", m.group(1)).strip()


def _struct(name):
    m = re.search(r"struct\s+" + name + r"\s*\{([^}]*)\}", _header())
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_header_declares_and_library_exports_the_entry_points():
    import xsknet_amd as X
    R, P = "const struct xsk_gpu_ring_dev*", "const struct xsk_gpu_pool_dev*"
    assert _decl("int", "xsk_gpu_rx_begin_dev") == (
        f"{R} rx, {R} fill, {R} tx, {P} pool, uint32_t max_batch, struct xsk_gpu_desc* d_descs, "
        "struct xsk_gpu_rx_plan* d_plan, void* stream")
    assert _decl("int", "xsk_gpu_rx_end_dev") == (
        f"{R} rx, {R} tx, {P} pool, const struct xsk_gpu_rx_plan* d_plan, const struct xsk_gpu_desc* d_tx, "
        "const uint64_t* d_free, const struct xsk_gpu_egress_counts* d_counts, uint32_t n_max, "
        "struct xsk_gpu_rx_result* d_res, void* stream")
    assert _decl("int", "xsk_gpu_rx_step_dev") == (
        f"void* d_umem, uint64_t umem_size, {R} rx, {R} fill, {R} tx, {P} pool, uint32_t max_batch, uint32_t opts, "
        "struct xsk_gpu_stats* d_stats, struct xsk_gpu_rx_result* d_res, void* d_workspace, void* stream")
    assert _decl("int", "xsk_gpu_tx_complete_dev") == f"{R} comp, {P} pool, uint32_t max, uint32_t* d_moved, void* stream"
    assert _decl("size_t", "xsk_gpu_rx_step_dev_workspace_size") == "uint32_t max_batch"
    assert _struct("xsk_gpu_ring_dev") == \
        "uint32_t* d_producer; uint32_t* d_consumer; void* d_ring; uint32_t size; uint32_t reserved;"
    assert _struct("xsk_gpu_pool_dev") == "uint64_t* d_addr; uint32_t* d_n_free; uint32_t capacity; uint32_t reserved;"
    assert _struct("xsk_gpu_rx_plan") == ("uint32_t received; uint32_t tx_room; uint32_t refilled; "
                                          "uint32_t rx_cons, fq_prod, pool_n; uint32_t reserved[2];")
    out = subprocess.run(["nm", "-D", "--defined-only", X.LIB_PATH], capture_output=True, text=True, check=True)
    for name in NAMES:
        assert re.search(r"\bT " + name + r"\b", out.stdout), name
        assert hasattr(X.lib(), name) and name in X._SIGS
    # no new hook: everything else of the feature is static or in an anonymous namespace
    exported = re.findall(r"\bT (\w+)", out.stdout)
    assert not [s for s in exported if re.search(r"ring_dev|rx_begin|rx_end|rx_step_dev|tx_complete_dev|rd_", s)
                and s not in NAMES]
    for f in (X.rx_begin_dev, X.rx_end_dev, X.rx_step_dev, X.rx_step_dev_workspace_size, X.tx_complete_dev):
        assert callable(f)
    assert [len(X._SIGS[n][0]) for n in NAMES] == [8, 10, 12, 5, 1]


def test_struct_layouts():
    import xsknet_amd as X
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "xsk_gpu.h"
#define O(s, f) printf(#s "." #f " %zu\n", offsetof(struct s, f))
int main(void){
 printf("sizes %zu %zu %zu\n", sizeof(struct xsk_gpu_ring_dev), sizeof(struct xsk_gpu_pool_dev), sizeof(struct xsk_gpu_rx_plan));
 O(xsk_gpu_ring_dev, d_producer); O(xsk_gpu_ring_dev, d_consumer); O(xsk_gpu_ring_dev, d_ring); O(xsk_gpu_ring_dev, size);
 O(xsk_gpu_ring_dev, reserved); O(xsk_gpu_pool_dev, d_addr); O(xsk_gpu_pool_dev, d_n_free); O(xsk_gpu_pool_dev, capacity);
 O(xsk_gpu_pool_dev, reserved); O(xsk_gpu_rx_plan, received); O(xsk_gpu_rx_plan, tx_room); O(xsk_gpu_rx_plan, refilled);
 O(xsk_gpu_rx_plan, rx_cons); O(xsk_gpu_rx_plan, fq_prod); O(xsk_gpu_rx_plan, pool_n); O(xsk_gpu_rx_plan, reserved);
 return 0; }
'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "p.c")
        open(c, "w").write(probe)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(td, "p"), c],
                       check=True)
        out = subprocess.run([os.path.join(td, "p")], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "sizes 32 24 32"
    assert (C.sizeof(X.RingDev), C.sizeof(X.PoolDev), C.sizeof(X.RxPlan)) == (32, 24, 32)
    offs = dict(line.split() for line in out[1:] if line)
    for cls, name in ((X.RingDev, "xsk_gpu_ring_dev"), (X.PoolDev, "xsk_gpu_pool_dev"), (X.RxPlan, "xsk_gpu_rx_plan")):
        for f, _ in cls._fields_:
            assert int(offs[f"{name}.{f}"]) == getattr(cls, f).offset, (name, f)
    for f in RS.PLAN_DTYPE.names:
        assert RS.PLAN_DTYPE.fields[f][1] == getattr(X.RxPlan, f).offset
    assert [n for n, _ in X.RxResult._fields_] == list(RS.RESULT_DTYPE.names)


def test_workspace_size():
    import xsknet_amd as X
    ws = X.rx_step_dev_workspace_size
    for n in (1, 63, 64, 1024, 1025, 1300, 65536, MAX_BATCH):
        want = 48 + n * (16 + 16 + 8 + 1)
        want = (want + 3) // 4 * 4 + X.egress_workspace_size(n)
        assert ws(n) == (want + 15) // 16 * 16, n


# ---- the argument rules ------------------------------------------------------------------------------------------

def _ring(X, base, size=64, **kw):
    r = X.RingDev(base, base + 0x100, base + 0x1000, size, 0)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _pool(X, **kw):
    p = X.PoolDev(0x900000, 0x910000, 128, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _bad_rings(X, base, entry_align):
    """Every way a ring struct is refused."""
    bad = [None]
    for f in ("d_producer", "d_consumer", "d_ring"):
        bad.append(_ring(X, base, **{f: None}))
    for mis in (1, 2, 3):
        bad.append(_ring(X, base, d_producer=base + mis))
        bad.append(_ring(X, base, d_consumer=base + 0x100 + mis))
    mis = 1
    while mis < entry_align:
        bad.append(_ring(X, base, d_ring=base + 0x1000 + mis))
        mis *= 2
    for size in (0, 3, 6, 100, 0x80000001, 0xC0000000, 0xFFFFFFFF):
        bad.append(_ring(X, base, size=size))
    bad.append(_ring(X, base, reserved=1))
    return bad


def _bad_pools(X):
    bad = [None, _pool(X, d_addr=None), _pool(X, d_n_free=None), _pool(X, capacity=0), _pool(X, reserved=7)]
    bad += [_pool(X, d_addr=0x900000 + m) for m in (1, 2, 4)]
    bad += [_pool(X, d_n_free=0x910000 + m) for m in (1, 2, 3)]
    return bad


def _ref(x):
    return None if x is None else C.byref(x)


def test_argument_validation_needs_no_gpu():
    import xsknet_amd as X
    L = X.lib()
    rx, fill, tx, comp = (_ring(X, b) for b in (0x100000, 0x200000, 0x300000, 0x400000))
    pool = _pool(X)
    de, pl, dtx, dfr, co, res, st, ws, um, mv = (0x500000, 0x510000, 0x520000, 0x530000, 0x540000, 0x550000, 0x560000,
                                                 0x570000, 0x600000, 0x580000)
    ok_sizes = (1, 8, 0x80000000)
    assert all(_ring(X, 0x100000, size=s).size == s for s in ok_sizes)

    def begin(rx=rx, fill=fill, tx=tx, pool=pool, mb=64, de=de, pl=pl):
        return L.xsk_gpu_rx_begin_dev(_ref(rx), _ref(fill), _ref(tx), _ref(pool), mb, de, pl, None)

    def end(rx=rx, tx=tx, pool=pool, pl=pl, dtx=dtx, dfr=dfr, co=co, n_max=64, res=res):
        return L.xsk_gpu_rx_end_dev(_ref(rx), _ref(tx), _ref(pool), pl, dtx, dfr, co, n_max, res, None)

    def step(um=um, size=1 << 20, rx=rx, fill=fill, tx=tx, pool=pool, mb=64, opts=0, st=st, res=res, ws=ws):
        return L.xsk_gpu_rx_step_dev(um, size, _ref(rx), _ref(fill), _ref(tx), _ref(pool), mb, opts, st, res, ws, None)

    def complete(comp=comp, pool=pool, mx=64, mv=mv):
        return L.xsk_gpu_tx_complete_dev(_ref(comp), _ref(pool), mx, mv, None)

    for b in _bad_rings(X, 0x100000, 16):  # descriptor rings
        assert begin(rx=b) == EINVAL and begin(tx=b) == EINVAL
        assert end(rx=b) == EINVAL and end(tx=b) == EINVAL
        assert step(rx=b) == EINVAL and step(tx=b) == EINVAL
    for b in _bad_rings(X, 0x200000, 8):   # address rings
        assert begin(fill=b) == EINVAL and step(fill=b) == EINVAL and complete(comp=b) == EINVAL
    for b in _bad_pools(X):
        assert begin(pool=b) == EINVAL and end(pool=b) == EINVAL and step(pool=b) == EINVAL
        assert complete(pool=b) == EINVAL
    for mb in (0, MAX_BATCH + 1, 0xFFFFFFFF):
        assert begin(mb=mb) == EINVAL and end(n_max=mb) == EINVAL and step(mb=mb) == EINVAL
    for mb in (MAX_BATCH + 1, 0xFFFFFFFF):
        assert complete(mx=mb) == EINVAL
    for mb in (64, 1024, 1025, 70000):  # both paths refuse alike
        assert begin(mb=mb, de=None) == EINVAL and begin(mb=mb, pl=None) == EINVAL
        for mis in (1, 2, 4, 8):
            assert begin(mb=mb, de=de + mis) == EINVAL
            assert end(n_max=mb, dtx=dtx + mis) == EINVAL
            assert step(mb=mb, ws=ws + mis) == EINVAL and step(mb=mb, um=um + mis) == EINVAL
            assert step(mb=mb, size=(1 << 20) + mis) == EINVAL
        for mis in (1, 2, 4):
            assert end(n_max=mb, dfr=dfr + mis) == EINVAL
            assert step(mb=mb, st=st + mis) == EINVAL
        for mis in (1, 2, 3):
            assert begin(mb=mb, pl=pl + mis) == EINVAL
            assert end(n_max=mb, pl=pl + mis) == EINVAL and end(n_max=mb, co=co + mis) == EINVAL
            assert end(n_max=mb, res=res + mis) == EINVAL and step(mb=mb, res=res + mis) == EINVAL
            assert complete(mx=mb, mv=mv + mis) == EINVAL
        for miss in ("pl", "dtx", "dfr", "co"):
            assert end(n_max=mb, **{miss: None}) == EINVAL
        assert step(mb=mb, ws=None) == EINVAL and step(mb=mb, um=None) == EINVAL
        assert step(mb=mb, size=1 << 48) == EINVAL
        for opts in (0x8, 0x20, 0x18, 0xFFFFFFFF):
            assert step(mb=mb, opts=opts) == EINVAL
    # the rules hold for max == 0 too (nothing is issued before them)
    assert complete(comp=None, mx=0) == EINVAL and complete(pool=None, mx=0) == EINVAL
    assert complete(mx=0, mv=mv + 2) == EINVAL


def test_every_rule_stands_in_front_of_the_first_device_call():
    """The host functions' own text: each public call returns -EINVAL from one block of checks before anything that
    launches, and the file stores through no inline assembly."""
    src = open(os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_ring_dev.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "asm" not in code and "__restrict__" not in code.split("load_word")[1].split("}")[0]
    pub = code[code.index('extern "C" {'):]
    for name in NAMES[:4]:
        body = pub[pub.index("int " + name + "("):]
        body = body[:body.index("\n}\n")]
        first = min(body.index(t) for t in ("_launch(", "<<<", "hipMemsetAsync", "xsk_gpu_echo_dev_indirect(")
                    if t in body)
        assert body.rindex("return -EINVAL") < first, name
    hdr = open(os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_ring_dev.h")).read()
    assert re.search(r"kRdSmallMax\s*=\s*1024\b", hdr) and re.search(r"kRdCopy\s*=\s*256\b", hdr)


# ---- the spec ----------------------------------------------------------------------------------------------------

STARTS = (0, 5, 0xFFFFFFFD)


def _host_ring(ring: RS.RingState, consumer: bool):
    """An X.Ring over copies of a RingState's words and entries, caches set so that the first use refreshes."""
    import xsknet_amd as X
    ctr = np.array([ring.prod, ring.cons], np.uint32)
    slots = ring.entries.copy()
    c = ring.cons if consumer else ring.prod
    view = X.Ring(c, c, ring.size - 1, ring.size, ctr.ctypes.data, ctr.ctypes.data + 4, slots.ctypes.data, None)
    return view, ctr, slots


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("size", [1, 8, 64])
def test_complete_against_the_host_function(size, start):
    """spec_complete over (ring, pool) == xsk_gpu_tx_complete() over the same state: ring used 0 / 1 / half / full, pool
    empty / one / room for some / full, max below, at and above what the ring holds."""
    import xsknet_amd as X
    cap = size + 3
    rng = np.random.default_rng(size * 7 + (start & 0xFF))
    for used in sorted({0, 1, size // 2, size}):
        for pool_n in sorted({0, 1, max(cap - max(used // 2, 1), 0), cap - 1, cap}):
            for mx in sorted({1, max(used - 1, 1), used + 1, size + 5, 4096}):
                comp = RS.RingState(rng.integers(1, 1 << 40, size, dtype=np.uint64), start + used, start)
                pool = RS.PoolState(rng.integers(1, 1 << 40, cap, dtype=np.uint64), pool_n)
                view, ctr, slots = _host_ring(comp, True)
                stack = pool.addr.copy()
                hp = X.FramePool(stack.ctypes.data, pool_n, cap)
                n_host = X.lib().xsk_gpu_tx_complete(C.byref(view), C.byref(hp), mx)
                n_spec = RS.spec_complete(comp, pool, mx)
                assert n_host == n_spec == min(used, mx)
                assert (int(ctr[0]), int(ctr[1])) == (comp.prod, comp.cons) and (slots == comp.entries).all()
                assert hp.n_free == pool.n_free and (stack[:hp.n_free] == pool.addr[:pool.n_free]).all()


def _traffic(n, seed, stride=2048):
    umem = np.zeros(max(n, 1) * stride, np.uint8)
    descs = oracle.synth_batch(umem, n, 0, stride, seed=seed, mode=1, len_lo=20, len_hi=1500)
    return umem, np.ascontiguousarray(descs, oracle.DESC_DTYPE)


def _state(size, start, descs, fill_free, pool_n, tx_room, cap=None):
    """Rings of `size` entries holding `descs` on the RX ring, the fill ring with fill_free free slots, the TX ring with
    tx_room, a pool of pool_n frames; every index word starts near `start`."""
    cap = cap or size + 3
    rng = np.random.default_rng(size + len(descs))
    rx = RS.RingState(np.zeros(size, oracle.DESC_DTYPE), start, start)
    rx.entries["options"] = 0xDEAD
    rx.produce(descs)
    fill = RS.RingState(rng.integers(1, 1 << 40, size, dtype=np.uint64), start + 1 + size - fill_free, start + 1)
    tx = RS.RingState(np.zeros(size, oracle.DESC_DTYPE), start + 2 + size - tx_room, start + 2)
    tx.entries["addr"] = rng.integers(1, 1 << 40, size, dtype=np.uint64)
    pool = RS.PoolState((np.arange(cap, dtype=np.uint64) + np.uint64(1 << 20)) * np.uint64(4096), pool_n)
    return rx, fill, tx, pool


@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("n,size,max_batch", [(1, 8, 4), (7, 8, 8), (64, 64, 64), (65, 128, 100), (300, 512, 1300)])
def test_step_is_begin_egress_end(n, size, max_batch, start):
    umem, descs = _traffic(n, seed=0x5EED0000 + n)
    for fill_free, pool_n, tx_room in ((size, size + 3, size), (1, 2, 3), (0, 0, 0), (size // 2, 1, size // 4)):
        a = _state(size, start, descs, fill_free, pool_n, tx_room)
        b = tuple(s.copy() for s in a)
        ua, ub = umem.copy(), umem.copy()
        st = dict.fromkeys(IS.KEYS, 0)
        res = RS.spec_step(ua, *a, max_batch, 0, st)
        # by hand
        rx, fill, tx, pool = b
        d = np.zeros(max_batch, oracle.DESC_DTYPE)
        plan = RS.spec_begin(rx, fill, tx, pool, max_batch, d)
        k = plan["received"]
        assert k == min(n, max_batch) and (d[:k] == descs[:k]).all() and rx.cons == start  # not released yet
        assert plan["refilled"] == min(fill_free, pool_n) and plan["tx_room"] == tx_room
        v, _, s2 = IS.spec_transform(ub, d[:k], 0)
        txl, frl, counts, dp, db = ES.spec_egress(d, v, k, plan["tx_room"])
        res2 = RS.spec_end(rx, tx, pool, plan, txl, frl, counts, max_batch)
        assert res == res2 and (ua == ub).all()
        for x, y in zip(a, b):
            assert x.same(y)
        assert res["received"] == k and res["replied"] == min(int((v == 0).sum()), tx_room)
        assert res["replied"] + res["tx_full"] == int((v == 0).sum())
        assert st["rx_packets"] == k and st["tx_packets"] == res["replied"] == s2["tx_packets"] + dp
        assert st["tx_bytes"] == s2["tx_bytes"] + db
        # every frame is somewhere: pool + fill ring + TX ring hold what they held, plus the batch
        assert pool.n() <= pool.capacity and rx.cons == (start + k) & RS.M32


@pytest.mark.parametrize("start", STARTS)
def test_an_empty_rx_ring_changes_nothing(start):
    a = _state(8, start, np.zeros(0, oracle.DESC_DTYPE), 8, 11, 8)
    b = tuple(s.copy() for s in a)
    d = np.full(4, 0xEE, np.uint8).repeat(16).view(oracle.DESC_DTYPE).copy()
    d0 = d.copy()
    plan = RS.spec_begin(*a, 4, d)
    assert plan == dict(received=0, tx_room=8, refilled=0, rx_cons=start, fq_prod=(start + 1) & RS.M32, pool_n=11)
    assert (d == d0).all() and all(x.same(y) for x, y in zip(a, b))
    res = RS.spec_step(np.zeros(16, np.uint8), *a, 4, 0x17)
    assert res == dict(received=0, replied=0, tx_full=0, refilled=0) and all(x.same(y) for x, y in zip(a, b))


def test_garbage_words_are_clamped():
    """used > size reads as a full ring, *d_n_free > capacity as a full pool: nothing indexes outside."""
    r = RS.RingState(np.zeros(8, np.uint64), 5, 100)
    assert r.used() == 8 and r.free() == 0
    p = RS.PoolState(np.zeros(4, np.uint64), 77)
    assert p.n() == 4
    comp = RS.RingState(np.arange(8, dtype=np.uint64), 1000, 3)
    assert RS.spec_complete(comp, p, 100) == 8 and p.n_free == 4 and comp.cons == 11


def test_ring_arithmetic_on_the_host_under_address_sanitizer():
    """tests/c/test_ring_dev.cpp: xsk_ring_dev.h's plans, slots, grid and workspace layout, both paths replayed thread
    by thread into heap arrays of exactly the rings' sizes, against xr_*() driven as xsk_gpu_rx.c drives it; the case
    matrix of its header comment."""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "t")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "c", "test_ring_dev.cpp")], check=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    assert "ring dev ok" in res.stdout
