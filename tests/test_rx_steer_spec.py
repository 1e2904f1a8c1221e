"""xsk_gpu_rx_prepare_ports_dev / xsk_gpu_rx_ports_end_dev / xsk_gpu_rx_step_steer_dev without a GPU: the ABI surface,
the argument checks (fabricated pointers, no device call reached), the numpy spec (tests/rx_steer_spec.py) against its
own identities -- the pad descriptor, the one-port identity with rx_dev_spec.spec_step, conservation, the empty RX ring
-- and the ring arithmetic of both kernel paths compiled for the host under AddressSanitizer
(tests/c/test_ring_ports.cpp)."""
import ctypes as C
import errno
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from tests import ingress_spec as IS
from tests import rx_dev_spec as RS
from tests import rx_steer_spec as RP
from tests import steer_spec as SS
from tests.conftest import ROOT
from tests.test_rx_dev_spec import MAX_BATCH, _bad_pools, _bad_rings, _decl, _pool, _ref, _ring, _struct
from tests.v6_frames import mixed_batch6

EINVAL = -errno.EINVAL
NAMES = ("xsk_gpu_rx_prepare_ports_dev", "xsk_gpu_rx_ports_end_dev", "xsk_gpu_rx_step_steer_dev",
         "xsk_gpu_rx_step_steer_dev_workspace_size")


def _params(ret, name):
    return _decl(ret, name).replace(" ,", ",")


def test_header_declares_and_library_exports_the_entry_points():
    import xsknet_amd as X
    R, P = "const struct xsk_gpu_ring_dev*", "const struct xsk_gpu_pool_dev*"
    assert _params("int", "xsk_gpu_rx_prepare_ports_dev") == (
        f"{R} tx, uint32_t n_ports, const struct xsk_gpu_rx_plan* d_plan, struct xsk_gpu_desc* d_descs, "
        "uint32_t n_max, uint32_t* d_tx_room, void* stream")
    assert _params("int", "xsk_gpu_rx_ports_end_dev") == (
        f"{R} rx, {R} tx, uint32_t n_ports, {P} pool, const struct xsk_gpu_rx_plan* d_plan, "
        "const struct xsk_gpu_desc* d_descs, const uint8_t* d_actions, const uint32_t* d_off, "
        "const struct xsk_gpu_desc* d_tx, const uint64_t* d_free, const struct xsk_gpu_egress_counts* d_counts, "
        "uint32_t n_max, struct xsk_gpu_rx_steer_result* d_res, void* d_workspace, void* stream")
    assert _params("int", "xsk_gpu_rx_step_steer_dev") == (
        f"void* d_umem, uint64_t umem_size, {R} rx, {R} fill, {R} tx, {P} pool, uint32_t max_batch, uint32_t opts, "
        "const struct xsk_gpu_steer_entry* d_table, uint32_t n_entries, uint32_t default_port, uint32_t n_ports, "
        "const uint64_t* d_bound, uint8_t* d_actions, uint8_t* d_ports, struct xsk_gpu_egress_counts* d_port_counts, "
        "struct xsk_gpu_stats* d_stats, struct xsk_gpu_stats* d_port_stats, struct xsk_gpu_rx_steer_result* d_res, "
        "void* d_workspace, void* stream")
    assert _params("size_t", "xsk_gpu_rx_step_steer_dev_workspace_size") == "uint32_t max_batch, uint32_t n_ports"
    assert _struct("xsk_gpu_rx_steer_result") == (
        "uint32_t received; uint32_t redirected; uint32_t replied; uint32_t tx_full; uint32_t refilled; "
        "uint32_t freed; uint32_t reserved[2];")
    out = subprocess.run(["nm", "-D", "--defined-only", X.LIB_PATH], capture_output=True, text=True, check=True)
    for name in NAMES:
        assert re.search(r"\bT " + name + r"\b", out.stdout), name
        assert hasattr(X.lib(), name) and name in X._SIGS
    # no new hook: everything else of the feature is static or in an anonymous namespace
    exported = re.findall(r"\bT (\w+)", out.stdout)
    assert not [s for s in exported if re.search(r"ring_ports|rx_prepare|rx_ports|rx_step_steer|rp_", s) and s not in NAMES]
    for f in (X.rx_prepare_ports_dev, X.rx_end_ports_dev, X.rx_step_steer_dev, X.rx_step_steer_dev_workspace_size):
        assert callable(f)
    assert [len(X._SIGS[n][0]) for n in NAMES] == [7, 15, 21, 2]


def test_struct_layout():
    import xsknet_amd as X
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "xsk_gpu.h"
#define O(s, f) printf(#s "." #f " %zu\n", offsetof(struct s, f))
int main(void){
 printf("size %zu abi %d\n", sizeof(struct xsk_gpu_rx_steer_result), XSK_GPU_ABI_VERSION);
 O(xsk_gpu_rx_steer_result, received); O(xsk_gpu_rx_steer_result, redirected); O(xsk_gpu_rx_steer_result, replied);
 O(xsk_gpu_rx_steer_result, tx_full); O(xsk_gpu_rx_steer_result, refilled); O(xsk_gpu_rx_steer_result, freed);
 O(xsk_gpu_rx_steer_result, reserved);
 return 0; }
'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "p.c")
        open(c, "w").write(probe)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(td, "p"), c],
                       check=True)
        out = subprocess.run([os.path.join(td, "p")], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "size 32 abi 1" and C.sizeof(X.RxSteerResult) == 32
    offs = dict(line.split() for line in out[1:] if line)
    for f, _ in X.RxSteerResult._fields_:
        assert int(offs[f"xsk_gpu_rx_steer_result.{f}"]) == getattr(X.RxSteerResult, f).offset == \
            RP.RESULT_DTYPE.fields[f][1], f
    assert [n for n, _ in X.RxSteerResult._fields_] == list(RP.RESULT_DTYPE.names)


def test_workspace_size():
    import xsknet_amd as X

    def up(x, a):
        return (x + a - 1) // a * a

    for n in (1, 63, 64, 1024, 1025, 1300, 65536, MAX_BATCH):
        for p in (1, 3, 64):
            want = up(32 + p * 4 + (p + 1) * 4 + p * 16, 16) + n * (16 + 16 + 16 + 8 + 1 + 1 + 1)
            want = up(up(want, 4) + X.steer_workspace_size(n, p), 4) + X.egress_ports_workspace_size(n, p)
            end = 0 if n <= 1024 else up(n * 8 + (n + 255) // 256 * 4 + 4, 16)
            assert X.rx_step_steer_dev_workspace_size(n, p) == up(up(want, 16) + end, 16), (n, p)


# ---- the argument rules ------------------------------------------------------------------------------------------

def _ports(X, n, base=0x1000000):
    return (X.RingDev * n)(*[_ring(X, base + p * 0x10000) for p in range(n)])


def test_argument_validation_needs_no_gpu():
    import xsknet_amd as X
    L = X.lib()
    rx, fill = _ring(X, 0x100000), _ring(X, 0x200000)
    pool = _pool(X)
    de, pl, dtx, dfr, co, res, st, ws, um, room, act, off, tab, bnd, prt, pst = (
        0x500000, 0x510000, 0x520000, 0x530000, 0x540000, 0x550000, 0x560000, 0x570000, 0x600000, 0x580000, 0x590000,
        0x5A0000, 0x5B0000, 0x5C0000, 0x5D0000, 0x5E0000)

    def prepare(tx=None, np_=3, pl=pl, de=de, n_max=64, room=room):
        tx = _ports(X, max(min(np_, 64), 1)) if tx is None else tx
        return L.xsk_gpu_rx_prepare_ports_dev(tx if tx != 0 else None, np_, pl, de, n_max, room, None)

    def end(rx=rx, tx=None, np_=3, pool=pool, pl=pl, de=de, act=act, off=off, dtx=dtx, dfr=dfr, co=co, n_max=64, res=res,
            ws=ws):
        tx = _ports(X, max(min(np_, 64), 1)) if tx is None else tx
        return L.xsk_gpu_rx_ports_end_dev(_ref(rx), tx if tx != 0 else None, np_, _ref(pool), pl, de, act, off, dtx, dfr,
                                          co, n_max, res, ws, None)

    def step(um=um, size=1 << 20, rx=rx, fill=fill, tx=None, pool=pool, mb=64, opts=0, tab=None, ne=0, dp=0, np_=3, bnd=None,
             act=None, prt=None, co=None, st=st, pst=None, res=res, ws=ws):
        tx = _ports(X, max(min(np_, 64), 1)) if tx is None else tx
        return L.xsk_gpu_rx_step_steer_dev(um, size, _ref(rx), _ref(fill), tx if tx != 0 else None, _ref(pool), mb, opts,
                                           tab, ne, dp, np_, bnd, act, prt, co, st, pst, res, ws, None)

    # rings: rx / fill / pool as in the unsteered step; every port's ring, whichever port it is
    for b in _bad_rings(X, 0x100000, 16):
        assert end(rx=b) == EINVAL and step(rx=b) == EINVAL
        if b is not None:
            for n, at in ((1, 0), (3, 0), (3, 2), (64, 63)):
                tx = _ports(X, n)
                tx[at] = b
                assert prepare(tx=tx, np_=n) == EINVAL and end(tx=tx, np_=n) == EINVAL and step(tx=tx, np_=n) == EINVAL
    for b in _bad_rings(X, 0x200000, 8):
        assert step(fill=b) == EINVAL
    for b in _bad_pools(X):
        assert end(pool=b) == EINVAL and step(pool=b) == EINVAL
    assert prepare(tx=0) == EINVAL and end(tx=0) == EINVAL and step(tx=0) == EINVAL
    for n in (0, 65, 0xFFFFFFFF):
        assert prepare(np_=n) == EINVAL and end(np_=n) == EINVAL and step(np_=n) == EINVAL
    # two ports on one entry array or one producer word
    for n, a, b in ((2, 0, 1), (64, 5, 63)):
        for f in ("d_ring", "d_producer"):
            tx = _ports(X, n)
            setattr(tx[b], f, getattr(tx[a], f))
            assert prepare(tx=tx, np_=n) == EINVAL and end(tx=tx, np_=n) == EINVAL and step(tx=tx, np_=n) == EINVAL
    for mb in (0, MAX_BATCH + 1, 0xFFFFFFFF):
        assert prepare(n_max=mb) == EINVAL and end(n_max=mb) == EINVAL and step(mb=mb) == EINVAL
    for mb in (64, 1024, 1025, 70000):  # both paths refuse alike
        assert prepare(n_max=mb, de=None) == EINVAL and prepare(n_max=mb, pl=None) == EINVAL
        assert prepare(n_max=mb, room=None) == EINVAL
        for mis in (1, 2, 4, 8):
            assert prepare(n_max=mb, de=de + mis) == EINVAL
            assert end(n_max=mb, de=de + mis) == EINVAL and end(n_max=mb, dtx=dtx + mis) == EINVAL
            assert end(n_max=mb, ws=ws + mis) == EINVAL
            assert step(mb=mb, ws=ws + mis) == EINVAL and step(mb=mb, um=um + mis) == EINVAL
            assert step(mb=mb, size=(1 << 20) + mis) == EINVAL
        for mis in (1, 2, 4):
            assert end(n_max=mb, dfr=dfr + mis) == EINVAL
            assert step(mb=mb, st=st + mis) == EINVAL and step(mb=mb, pst=pst + mis) == EINVAL
            assert step(mb=mb, bnd=bnd + mis) == EINVAL and step(mb=mb, tab=tab + mis, ne=4) == EINVAL
        for mis in (1, 2, 3):
            assert prepare(n_max=mb, pl=pl + mis) == EINVAL and prepare(n_max=mb, room=room + mis) == EINVAL
            assert end(n_max=mb, pl=pl + mis) == EINVAL and end(n_max=mb, co=co + mis) == EINVAL
            assert end(n_max=mb, off=off + mis) == EINVAL and end(n_max=mb, res=res + mis) == EINVAL
            assert step(mb=mb, res=res + mis) == EINVAL and step(mb=mb, co=co + mis) == EINVAL
        for miss in ("pl", "de", "act", "off", "dtx", "dfr", "co", "ws"):
            assert end(n_max=mb, **{miss: None}) == EINVAL, miss
        assert step(mb=mb, ws=None) == EINVAL and step(mb=mb, um=None) == EINVAL
        assert step(mb=mb, size=1 << 48) == EINVAL
        for opts in (0x8, 0x20, 0x18, 0xFFFFFFFF):
            assert step(mb=mb, opts=opts) == EINVAL
        # the steering call's rules: the default port, the table
        for dp in (3, 64, 0xFE, 0x100):
            assert step(mb=mb, dp=dp) == EINVAL
        assert step(mb=mb, ne=1025, tab=tab) == EINVAL and step(mb=mb, ne=1, tab=None) == EINVAL


def test_every_rule_stands_in_front_of_the_first_device_call():
    """The host functions' own text: each public call returns -EINVAL from one block of checks before anything that
    launches, and the file stores through no inline assembly."""
    src = open(os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_ring_ports.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "asm" not in code and "atomicAdd" not in code and "__restrict__" not in code.split("load_word")[1].split("}")[0]
    pub = code[code.index('extern "C" {'):]
    for name in NAMES[:3]:
        body = pub[pub.index("int " + name + "("):]
        body = body[:body.index("\n}\n")]
        first = min(body.index(t) for t in ("_launch(", "<<<", "hipMemsetAsync", "xsk_gpu_rx_begin_dev(") if t in body)
        assert body.rindex("return -EINVAL") < first, name


# ---- the spec ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("opts", [0, 0x2, 0x10, 0x17])
def test_the_pad_descriptor_is_dropped_under_every_option_word(opts):
    umem = np.random.default_rng(opts).integers(0, 256, 4096, dtype=np.uint8)
    umem[12:14] = (0x08, 0x00)  # whatever lies at offset 0 of the UMEM, an IPv4 ethertype included
    pads = np.zeros(5, oracle.DESC_DTYPE)
    table = {SS.GS.key(bytes(umem[30:34])): 1}
    for default_port in (0, SS.PASS):
        ref = SS.spec_steer_batch(umem, pads, opts, table, default_port, 3)
        assert (ref["actions"] == SS.XDP_DROP).all() and (ref["ports"] == SS.PASS).all()
        assert list(ref["off"]) == [0, 0, 0, 0] and len(ref["out"]) == 0


def _rings(n_ports, sizes, start, rooms, seed=0):
    rng = np.random.default_rng(seed)
    txs = []
    for p in range(n_ports):
        size = sizes[p % len(sizes)]
        room = min(rooms[p % len(rooms)], size)
        t = RS.RingState(np.zeros(size, oracle.DESC_DTYPE), start + 2 * p + size - room, start + 2 * p)
        t.entries["addr"] = rng.integers(1, 1 << 40, size, dtype=np.uint64)
        t.entries["options"] = 0xBEEF
        txs.append(t)
    return txs


def _rx_state(size, start, descs, fill_free, pool_n, cap):
    rng = np.random.default_rng(size + len(descs))
    rx = RS.RingState(np.zeros(size, oracle.DESC_DTYPE), start, start)
    rx.entries["options"] = 0xDEAD
    rx.produce(descs)
    fill = RS.RingState(rng.integers(1, 1 << 40, size, dtype=np.uint64), start + 1 + size - fill_free, start + 1)
    pool = RS.PoolState((np.arange(cap, dtype=np.uint64) + np.uint64(1 << 20)) * np.uint64(4096), pool_n)
    return rx, fill, pool


@pytest.mark.parametrize("start", [0, 5, 0xFFFFFFFD])
@pytest.mark.parametrize("n,size,max_batch,opts", [(1, 8, 4, 0), (64, 64, 64, 0), (65, 128, 100, 0), (64, 64, 80, 0x17)])
def test_identity_with_the_unsteered_step_at_one_port(n, size, max_batch, opts, start):
    """n_ports == 1, no table, default port 0, everything bound, a batch the filter redirects whole: rings, words, pool,
    counters and UMEM end where rx_dev_spec.spec_step leaves them."""
    umem = np.zeros(n * 2048, np.uint8)
    descs = np.ascontiguousarray(oracle.synth_batch(umem, n, 0, 2048, seed=0x1D + n, mode=0, len_lo=64, len_hi=1500),
                                 oracle.DESC_DTYPE)
    assert (SS.spec_steer_batch(umem, descs, opts, {}, 0, 1)["actions"] == SS.XDP_REDIRECT).all()
    for fill_free, pool_n, tx_room in ((size, size + 3, size), (1, 2, 3), (0, 0, 0), (size // 2, 1, size // 4)):
        rx, fill, pool = _rx_state(size, start, descs, fill_free, pool_n, size + 3)
        tx = _rings(1, [size], start, [tx_room])[0]
        a = (rx.copy(), fill.copy(), tx.copy(), pool.copy())
        ua, ub = umem.copy(), umem.copy()
        sa, sb = dict.fromkeys(IS.KEYS, 0), dict.fromkeys(IS.KEYS, 0)
        ra = RS.spec_step(ua, *a, max_batch, opts, sa)
        got = RP.spec_step_steer(ub, rx, fill, [tx], pool, max_batch, opts, {}, 0, stats=sb)
        rb = got["result"]
        assert all(x.same(y) for x, y in zip(a, (rx, fill, tx, pool)))
        assert (ua == ub).all() and sa == sb
        assert {k: rb[k] for k in ra} == ra and rb["redirected"] == rb["received"] == min(n, max_batch)
        assert rb["freed"] == min(rb["received"] - rb["replied"], pool.capacity - (pool.n() - rb["freed"]))


@pytest.mark.parametrize("opts", [0, 0x17])
@pytest.mark.parametrize("n,n_ports,max_batch", [(40, 1, 64), (64, 3, 64), (300, 64, 300), (130, 2, 200)])
def test_conservation_with_a_pool_that_has_room(n, n_ports, max_batch, opts):
    """Every received address appears exactly once: among some TX ring's new entries or among the pool's new entries;
    DROP and PASS frames are among the latter."""
    umem, descs = mixed_batch6(n, 2048, seed=0xC0 + n)
    descs = np.ascontiguousarray(descs, oracle.DESC_DTYPE)
    table = SS.sample_table(SS.destinations(umem, descs, opts), 24, n_ports, seed=n)
    for default_port in (0, SS.PASS):
        rx, fill, pool = _rx_state(512, 0xFFFFFFFD, descs, 0, 7, 600)
        txs = _rings(n_ports, [8, 64, 512, 16], 0xFFFFFFF0, [512, 0, 3, 512])
        before = [t.copy() for t in txs]
        got = RP.spec_step_steer(umem.copy(), rx, fill, txs, pool, max_batch, opts, table, default_port,
                                 bound=SS.ALL_BOUND & ~2)
        res = got["result"]
        k = min(n, max_batch)
        new = [int(a) for a in pool.addr[7:pool.n()]]
        for t, b in zip(txs, before):
            cnt = (t.prod - b.prod) & RS.M32
            new += [int(t.entries[t.slot(b.prod + j)]["addr"]) for j in range(cnt)]
            assert t.cons == b.cons and cnt <= b.free()
        assert sorted(new) == sorted(int(a) for a in descs["addr"][:k]) and len(set(new)) == k
        assert res["received"] == k and res["freed"] == pool.n() - 7 and res["freed"] + res["replied"] == k
        acts = got["actions"]
        assert (acts[k:] == SS.XDP_DROP).all() and (got["ports"][k:] == SS.PASS).all()
        assert res["redirected"] == int((acts == SS.XDP_REDIRECT).sum()) == int(got["off"][n_ports])
        if n >= 64:
            assert 0 < res["redirected"] < k and (acts[:k] == SS.XDP_DROP).any()
        if default_port == SS.PASS and n >= 64:
            assert (acts[:k] == SS.XDP_PASS).any()
        assert rx.cons == (0xFFFFFFFD + k) & RS.M32


@pytest.mark.parametrize("start", [0, 0xFFFFFFFD])
def test_an_empty_rx_ring_changes_nothing(start):
    rx, fill, pool = _rx_state(8, start, np.zeros(0, oracle.DESC_DTYPE), 8, 11, 16)
    txs = _rings(3, [8, 4, 16], start, [8, 0, 5])
    before = [x.copy() for x in (rx, fill, pool, *txs)]
    umem = np.arange(4096, dtype=np.uint8)
    st = dict.fromkeys(IS.KEYS, 0)
    got = RP.spec_step_steer(umem, rx, fill, txs, pool, 4, 0x17, {}, 0, stats=st)
    assert got["result"] == dict.fromkeys(RP.RESULT_KEYS, 0) and not any(st.values())
    assert all(x.same(y) for x, y in zip(before, (rx, fill, pool, *txs)))
    assert (umem == np.arange(4096, dtype=np.uint8)).all() and got["rooms"] == [8, 0, 5]
    assert (got["actions"] == SS.XDP_DROP).all() and (got["descs"] == RP.PAD).all()


def test_end_is_total_for_garbage_words():
    """Offsets that are not ascending or lie above the bound, counts above a segment's length, a received word above
    the bound, used > size, a pool count above the capacity: the clamps keep every index inside its array."""
    rng = np.random.default_rng(7)
    n_max = 40
    descs = np.zeros(n_max, oracle.DESC_DTYPE)
    descs["addr"] = np.arange(n_max) * 2048 + 2048
    d_tx, d_free = descs.copy(), (np.arange(n_max, dtype=np.uint64) + np.uint64(1000)) * np.uint64(4096)
    actions = rng.choice([1, 2, 4], n_max).astype(np.uint8)
    rx, _, pool = _rx_state(64, 3, descs[:0], 0, 0, 50)
    pool.n_free = 0xFFFFFF00
    txs = _rings(3, [8, 16, 4], 9, [8, 16, 4])
    txs[1].prod = (txs[1].cons + 0x80000000) & RS.M32
    counts = [dict(n_tx=0xFFFFFFFF, n_tx_full=1, n_free=0xFFFFFFFF) for _ in range(3)]
    res = RP.spec_end_ports(rx, txs, pool, dict(received=1 << 31, refilled=9), descs, actions, [7, 0xFFFFFFFF, 3, 20],
                            d_tx, d_free, counts, n_max)
    # o = [7, 40, 40, 40]: port 0 owns 33 frames and its ring takes 8 of them; the pool is full
    assert res == dict(received=40, redirected=40, replied=8, tx_full=3, refilled=9, freed=0)
    assert pool.n_free == 50 and rx.cons == 43 and txs[0].prod == (9 + 8) & RS.M32
    assert (txs[0].entries[[(9 + k) & 7 for k in range(8)]] == d_tx[7:15]).all()


def test_ring_arithmetic_on_the_host_under_address_sanitizer():
    """tests/c/test_ring_ports.cpp: xsk_ring_ports.h's shares, sources, grids and workspace layouts, both paths replayed
    thread by thread into heap arrays of exactly the rings' and the pool's sizes, against the rule stated sequentially;
    the case matrix of its header comment."""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "t")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "c", "test_ring_ports.cpp")], check=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    assert "ring ports ok" in res.stdout
