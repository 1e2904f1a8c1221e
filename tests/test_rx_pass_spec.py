"""xsk_gpu_rx_pass_end_dev / xsk_gpu_rx_pass_step_dev without a GPU: the ABI surface and the export-name rule, the
argument checks (fabricated pointers, no device call reached; the stack ring's aliasing rules among them), the numpy
spec (tests/rx_pass_spec.py) against its own identities -- no stack ring or a full one is rx_steer_spec's end and step,
conservation, batch order on the stack ring and in the rest, a stack ring that takes none, some and all of the PASS
frames, the empty RX ring, garbage -- and the ring arithmetic of both kernel paths compiled for the host under
AddressSanitizer (tests/c/test_ring_pass.cpp)."""
import ctypes as C
import errno
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from tests import egress_ports_spec as EP
from tests import ingress_spec as IS
from tests import rx_dev_spec as RS
from tests import rx_pass_spec as PS
from tests import rx_steer_spec as RP
from tests import steer_spec as SS
from tests.conftest import ROOT
from tests.test_rx_dev_spec import MAX_BATCH, _bad_pools, _bad_rings, _decl, _pool, _ref, _ring, _struct
from tests.test_rx_steer_spec import _ports, _rings, _rx_state
from tests.v6_frames import mixed_batch6

EINVAL = -errno.EINVAL
NAMES = ("xsk_gpu_rx_pass_end_dev", "xsk_gpu_rx_pass_step_dev", "xsk_gpu_rx_pass_step_dev_workspace_size")
# substrings that existing tests reserve for existing exports
RESERVED = ("ring_dev", "rx_begin", "rx_end", "rx_step_dev", "tx_complete_dev", "rd_", "ring_ports", "rx_prepare", "rx_ports",
            "rx_step_steer", "rp_")


def _params(ret, name):
    return _decl(ret, name).replace(" ,", ",")


def _exports():
    import xsknet_amd as X
    out = subprocess.run(["nm", "-D", "--defined-only", X.LIB_PATH], capture_output=True, text=True, check=True)
    return re.findall(r"\bT (\w+)", out.stdout)


def test_header_declares_and_library_exports_the_entry_points():
    import xsknet_amd as X
    R, P = "const struct xsk_gpu_ring_dev*", "const struct xsk_gpu_pool_dev*"
    assert _params("int", "xsk_gpu_rx_pass_end_dev") == (
        f"{R} rx, {R} tx, uint32_t n_ports, {R} stack, {P} pool, const struct xsk_gpu_rx_plan* d_plan, "
        "const struct xsk_gpu_desc* d_descs, const uint8_t* d_actions, const uint32_t* d_off, "
        "const struct xsk_gpu_desc* d_tx, const uint64_t* d_free, const struct xsk_gpu_egress_counts* d_counts, "
        "uint32_t n_max, struct xsk_gpu_rx_pass_result* d_res, void* d_workspace, void* stream")
    assert _params("int", "xsk_gpu_rx_pass_step_dev") == (
        f"void* d_umem, uint64_t umem_size, {R} rx, {R} fill, {R} tx, {R} stack, {P} pool, uint32_t max_batch, "
        "uint32_t opts, const struct xsk_gpu_steer_entry* d_table, uint32_t n_entries, uint32_t default_port, "
        "uint32_t n_ports, const uint64_t* d_bound, uint8_t* d_actions, uint8_t* d_ports, "
        "struct xsk_gpu_egress_counts* d_port_counts, struct xsk_gpu_stats* d_stats, struct xsk_gpu_stats* d_port_stats, "
        "struct xsk_gpu_rx_pass_result* d_res, void* d_workspace, void* stream")
    assert _params("size_t", "xsk_gpu_rx_pass_step_dev_workspace_size") == "uint32_t max_batch, uint32_t n_ports"
    assert _struct("xsk_gpu_rx_pass_result") == (
        "uint32_t received; uint32_t redirected; uint32_t replied; uint32_t tx_full; uint32_t refilled; "
        "uint32_t freed; uint32_t passed; uint32_t pass_full;")
    exported = _exports()
    for name in NAMES:
        assert name in exported and hasattr(X.lib(), name) and name in X._SIGS, name
    for f in (X.rx_pass_end_dev, X.rx_pass_step_dev, X.rx_pass_step_dev_workspace_size):
        assert callable(f)
    assert [len(X._SIGS[n][0]) for n in NAMES] == [16, 22, 2]
    assert X.lib().xsk_gpu_abi_version() == 1


def test_the_new_exports_keep_clear_of_the_reserved_names():
    """No new exported symbol contains a substring that an existing test reserves for the existing exports (`egress`
    outside the prefix xsk_gpu_egress_ included); everything else of the feature is static or in an anonymous
    namespace, so the three entry points are all the library gained."""
    for name in NAMES:
        assert not [s for s in RESERVED if s in name], name
        assert "egress" not in name
    src = open(os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_ring_pass.hip")).read()
    pub = src[src.index('extern "C" {'):]
    assert sorted(re.findall(r"^(?:int|size_t) (\w+)\(", pub, re.M)) == sorted(NAMES)
    assert sorted(s for s in _exports() if "pass" in s) == sorted(NAMES)


def test_struct_layout():
    import xsknet_amd as X
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "xsk_gpu.h"
#define O(s, f) printf(#s "." #f " %zu\n", offsetof(struct s, f))
int main(void){
 printf("size %zu abi %d\n", sizeof(struct xsk_gpu_rx_pass_result), XSK_GPU_ABI_VERSION);
 O(xsk_gpu_rx_pass_result, received); O(xsk_gpu_rx_pass_result, redirected); O(xsk_gpu_rx_pass_result, replied);
 O(xsk_gpu_rx_pass_result, tx_full); O(xsk_gpu_rx_pass_result, refilled); O(xsk_gpu_rx_pass_result, freed);
 O(xsk_gpu_rx_pass_result, passed); O(xsk_gpu_rx_pass_result, pass_full);
 return 0; }
'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "p.c")
        open(c, "w").write(probe)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(td, "p"), c],
                       check=True)
        out = subprocess.run([os.path.join(td, "p")], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "size 32 abi 1" and C.sizeof(X.RxPassResult) == 32
    offs = dict(line.split() for line in out[1:] if line)
    for f, _ in X.RxPassResult._fields_:
        assert int(offs[f"xsk_gpu_rx_pass_result.{f}"]) == getattr(X.RxPassResult, f).offset == \
            PS.RESULT_DTYPE.fields[f][1], f
    assert [n for n, _ in X.RxPassResult._fields_] == list(PS.RESULT_DTYPE.names)
    # the first six words are struct xsk_gpu_rx_steer_result's
    for f in RP.RESULT_KEYS:
        assert PS.RESULT_DTYPE.fields[f][1] == RP.RESULT_DTYPE.fields[f][1]


def test_workspace_size():
    """The steered step's layout with end's part grown by the second count row and its total (the formula of
    include/xsk_gpu.h, restated)."""
    import xsknet_amd as X

    def up(x, a):
        return (x + a - 1) // a * a

    for n in (1, 63, 64, 1024, 1025, 1300, 65536, MAX_BATCH):
        for p in (1, 3, 64):
            want = up(32 + p * 4 + (p + 1) * 4 + p * 16, 16) + n * (16 + 16 + 16 + 8 + 1 + 1 + 1)
            want = up(up(want, 4) + X.steer_workspace_size(n, p), 4) + X.egress_ports_workspace_size(n, p)
            nwg = (n + 255) // 256
            end = 0 if n <= 1024 else up(n * 8 + 2 * nwg * 4 + 2 * 4, 16)
            assert X.rx_pass_step_dev_workspace_size(n, p) == up(up(want, 16) + end, 16), (n, p)
            steer_end = 0 if n <= 1024 else up(n * 8 + nwg * 4 + 4, 16)
            assert X.rx_pass_step_dev_workspace_size(n, p) - X.rx_step_steer_dev_workspace_size(n, p) == end - steer_end
    assert X.rx_pass_step_dev_workspace_size(64, 65) == X.rx_pass_step_dev_workspace_size(64, 64)


# ---- the argument rules ------------------------------------------------------------------------------------------

def test_argument_validation_needs_no_gpu():
    import xsknet_amd as X
    L = X.lib()
    rx, fill, stack = _ring(X, 0x100000), _ring(X, 0x200000), _ring(X, 0x300000)
    pool = _pool(X)
    de, pl, dtx, dfr, co, res, st, ws, um, act, off, tab, bnd, pst = (
        0x500000, 0x510000, 0x520000, 0x530000, 0x540000, 0x550000, 0x560000, 0x570000, 0x600000, 0x590000, 0x5A0000,
        0x5B0000, 0x5C0000, 0x5E0000)

    def end(rx=rx, tx=None, np_=3, stack=stack, pool=pool, pl=pl, de=de, act=act, off=off, dtx=dtx, dfr=dfr, co=co,
            n_max=64, res=res, ws=ws):
        tx = _ports(X, max(min(np_, 64), 1)) if tx is None else tx
        return L.xsk_gpu_rx_pass_end_dev(_ref(rx), tx if tx != 0 else None, np_, _ref(stack), _ref(pool), pl, de, act, off,
                                         dtx, dfr, co, n_max, res, ws, None)

    def step(um=um, size=1 << 20, rx=rx, fill=fill, tx=None, stack=stack, pool=pool, mb=64, opts=0, tab=None, ne=0, dp=0,
             np_=3, bnd=None, act=None, prt=None, co=None, st=st, pst=None, res=res, ws=ws):
        tx = _ports(X, max(min(np_, 64), 1)) if tx is None else tx
        return L.xsk_gpu_rx_pass_step_dev(um, size, _ref(rx), _ref(fill), tx if tx != 0 else None, _ref(stack), _ref(pool),
                                          mb, opts, tab, ne, dp, np_, bnd, act, prt, co, st, pst, res, ws, None)

    # the stack ring: NULL is allowed (no refusal that a valid ring would not get too); a ring that is given is checked
    # by a TX ring's rules, and may share neither its entry array nor its producer word with rx or a port's ring
    for b in _bad_rings(X, 0x300000, 16):
        if b is not None:
            assert end(stack=b) == EINVAL and step(stack=b) == EINVAL
    for other in (rx, *_ports(X, 3)):
        for f in ("d_ring", "d_producer"):
            s = _ring(X, 0x300000)
            setattr(s, f, getattr(other, f))
            assert end(stack=s) == EINVAL and step(stack=s) == EINVAL, f
    for n, at in ((1, 0), (64, 63), (64, 17)):
        tx = _ports(X, n)
        for f in ("d_ring", "d_producer"):
            s = _ring(X, 0x300000)
            setattr(s, f, getattr(tx[at], f))
            assert end(tx=tx, np_=n, stack=s) == EINVAL and step(tx=tx, np_=n, stack=s) == EINVAL
    # every rule of xsk_gpu_rx_ports_end_dev() / xsk_gpu_rx_step_steer_dev(), with a stack ring and without
    for stk in (stack, None):
        for b in _bad_rings(X, 0x100000, 16):
            assert end(rx=b, stack=stk) == EINVAL and step(rx=b, stack=stk) == EINVAL
            if b is not None:
                for n, at in ((1, 0), (3, 2), (64, 63)):
                    tx = _ports(X, n)
                    tx[at] = b
                    assert end(tx=tx, np_=n, stack=stk) == EINVAL and step(tx=tx, np_=n, stack=stk) == EINVAL
        for b in _bad_rings(X, 0x200000, 8):
            assert step(fill=b, stack=stk) == EINVAL
        for b in _bad_pools(X):
            assert end(pool=b, stack=stk) == EINVAL and step(pool=b, stack=stk) == EINVAL
        assert end(tx=0, stack=stk) == EINVAL and step(tx=0, stack=stk) == EINVAL
        for n in (0, 65, 0xFFFFFFFF):
            assert end(np_=n, stack=stk) == EINVAL and step(np_=n, stack=stk) == EINVAL
        for n, a, b in ((2, 0, 1), (64, 5, 63)):
            for f in ("d_ring", "d_producer"):
                tx = _ports(X, n)
                setattr(tx[b], f, getattr(tx[a], f))
                assert end(tx=tx, np_=n, stack=stk) == EINVAL and step(tx=tx, np_=n, stack=stk) == EINVAL
        for mb in (0, MAX_BATCH + 1, 0xFFFFFFFF):
            assert end(n_max=mb, stack=stk) == EINVAL and step(mb=mb, stack=stk) == EINVAL
    for mb in (64, 1024, 1025, 70000):  # both paths refuse alike
        for mis in (1, 2, 4, 8):
            assert end(n_max=mb, de=de + mis) == EINVAL and end(n_max=mb, dtx=dtx + mis) == EINVAL
            assert end(n_max=mb, ws=ws + mis) == EINVAL
            assert step(mb=mb, ws=ws + mis) == EINVAL and step(mb=mb, um=um + mis) == EINVAL
            assert step(mb=mb, size=(1 << 20) + mis) == EINVAL
        for mis in (1, 2, 4):
            assert end(n_max=mb, dfr=dfr + mis) == EINVAL
            assert step(mb=mb, st=st + mis) == EINVAL and step(mb=mb, pst=pst + mis) == EINVAL
            assert step(mb=mb, bnd=bnd + mis) == EINVAL and step(mb=mb, tab=tab + mis, ne=4) == EINVAL
        for mis in (1, 2, 3):
            assert end(n_max=mb, pl=pl + mis) == EINVAL and end(n_max=mb, co=co + mis) == EINVAL
            assert end(n_max=mb, off=off + mis) == EINVAL and end(n_max=mb, res=res + mis) == EINVAL
            assert step(mb=mb, res=res + mis) == EINVAL and step(mb=mb, co=co + mis) == EINVAL
        for miss in ("pl", "de", "act", "off", "dtx", "dfr", "co", "ws"):
            assert end(n_max=mb, **{miss: None}) == EINVAL, miss
        assert step(mb=mb, ws=None) == EINVAL and step(mb=mb, um=None) == EINVAL
        assert step(mb=mb, size=1 << 48) == EINVAL
        for opts in (0x8, 0x20, 0x18, 0xFFFFFFFF):
            assert step(mb=mb, opts=opts) == EINVAL
        for dp in (3, 64, 0xFE, 0x100):
            assert step(mb=mb, dp=dp) == EINVAL
        assert step(mb=mb, ne=1025, tab=tab) == EINVAL and step(mb=mb, ne=1, tab=None) == EINVAL


def test_every_rule_stands_in_front_of_the_first_device_call():
    """The host functions' own text: each public call returns -EINVAL from one block of checks before anything that
    launches; the file stores through no inline assembly and hands out no slot by an atomic."""
    src = open(os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_ring_pass.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "asm" not in code and "atomicAdd" not in code and "atomic_fetch" not in code
    pub = code[code.index('extern "C" {'):]
    for name in NAMES[:2]:
        body = pub[pub.index("int " + name + "("):]
        body = body[:body.index("\n}\n")]
        first = min(body.index(t) for t in ("_launch(", "<<<", "hipMemsetAsync", "xsk_gpu_rx_begin_dev(") if t in body)
        assert body.count("return -EINVAL") == 1 and body.index("return -EINVAL") < first, name


# ---- the spec ----------------------------------------------------------------------------------------------------

def _stack(size, start, room, seed=3):
    """A stack ring of `size` descriptors with `room` free entries, its producer word at `start`; stale entries."""
    rng = np.random.default_rng(seed + size)
    s = RS.RingState(np.zeros(size, oracle.DESC_DTYPE), start, (start - (size - room)) & RS.M32)
    s.entries["addr"] = rng.integers(1, 1 << 40, size, dtype=np.uint64)
    s.entries["len"], s.entries["options"] = 0x5A5A, 0xFACE
    assert s.free() == room
    return s


def _case(n, n_ports, opts, seed=0):
    umem, descs = mixed_batch6(n, 2048, seed=0xC0 + n + seed)
    descs = np.ascontiguousarray(descs, oracle.DESC_DTYPE)
    descs["options"] = np.arange(n, dtype=np.uint32) + 0x2000
    table = SS.sample_table(SS.destinations(umem, descs, opts), 24, n_ports, seed=n)
    return umem, descs, table


def _copies(*xs):
    return [[t.copy() for t in x] if isinstance(x, list) else (None if x is None else x.copy()) for x in xs]


@pytest.mark.parametrize("opts", [0, 0x17])
@pytest.mark.parametrize("n,n_ports,max_batch", [(40, 1, 64), (64, 3, 64), (300, 64, 300), (130, 2, 200)])
def test_without_a_stack_ring_or_with_a_full_one_the_step_is_the_steered_step(n, n_ports, max_batch, opts):
    """Rings, words, pool, counters and UMEM end where rx_steer_spec.spec_step_steer leaves them; the first six result
    words are equal, passed == 0 and pass_full == Q."""
    umem, descs, table = _case(n, n_ports, opts)
    for default_port in (0, SS.PASS):
        for stack in (None, _stack(16, 0xFFFFFFF9, 0), _stack(1, 5, 0)):
            rx, fill, pool = _rx_state(512, 0xFFFFFFFD, descs, 100, 150, 600)
            txs = _rings(n_ports, [8, 64, 512, 16], 0xFFFFFFF0, [512, 0, 3, 512])
            a = _copies(rx, fill, txs, pool)
            ua, ub = umem.copy(), umem.copy()
            sa, sb = dict.fromkeys(IS.KEYS, 0), dict.fromkeys(IS.KEYS, 0)
            pa, pb = ([dict.fromkeys(EP.STATS_KEYS, 0) for _ in txs] for _ in range(2))
            want = RP.spec_step_steer(ua, a[0], a[1], a[2], a[3], max_batch, opts, table, default_port, SS.ALL_BOUND & ~2,
                                      sa, pa)
            before = None if stack is None else stack.copy()
            got = PS.spec_step_pass(ub, rx, fill, txs, stack, pool, max_batch, opts, table, default_port,
                                    SS.ALL_BOUND & ~2, sb, pb)
            assert rx.same(a[0]) and fill.same(a[1]) and pool.same(a[3]) and all(x.same(y) for x, y in zip(txs, a[2]))
            assert stack is None or stack.same(before)
            assert (ua == ub).all() and sa == sb and pa == pb
            res, k = got["result"], min(n, max_batch)
            q = int((got["actions"][:k] == SS.XDP_PASS).sum())
            assert {f: res[f] for f in RP.RESULT_KEYS} == want["result"] and res["passed"] == 0 and res["pass_full"] == q
            assert (got["actions"] == want["actions"]).all() and (got["ports"] == want["ports"]).all()
            if n >= 64 and (opts == 0 or default_port == SS.PASS):
                assert q >= 1


def test_end_without_a_stack_ring_is_the_steered_end_for_garbage_words_too():
    rng = np.random.default_rng(11)
    n_max = 40
    descs = np.zeros(n_max, oracle.DESC_DTYPE)
    descs["addr"] = np.arange(n_max) * 2048 + 2048
    d_tx, d_free = descs.copy(), (np.arange(n_max, dtype=np.uint64) + np.uint64(1000)) * np.uint64(4096)
    for k in range(20):
        actions = rng.integers(0, 7, n_max).astype(np.uint8)
        off = [int(x) for x in rng.integers(0, n_max + 10, 4)]
        counts = [dict(n_tx=int(rng.integers(0, 50)), n_tx_full=k, n_free=int(rng.integers(0, 50))) for _ in range(3)]
        plan = dict(received=int(rng.integers(0, n_max + 5)), refilled=k)
        for stack in (None, _stack(8, k, 0)):
            rx, _, pool = _rx_state(64, 3, descs[:0], 0, k, 50)
            txs = _rings(3, [8, 16, 4], 9, [8, 3, 4])
            a = _copies(rx, txs, pool)
            want = RP.spec_end_ports(a[0], a[1], a[2], plan, descs, actions, off, d_tx, d_free, counts, n_max)
            res = PS.spec_end_pass(rx, txs, stack, pool, plan, descs, actions, off, d_tx, d_free, counts, n_max)
            assert rx.same(a[0]) and pool.same(a[2]) and all(x.same(y) for x, y in zip(txs, a[1]))
            r = min(plan["received"], n_max)
            assert {f: res[f] for f in RP.RESULT_KEYS} == want and res["passed"] == 0
            assert res["pass_full"] == int((actions[:r] == SS.XDP_PASS).sum())


@pytest.mark.parametrize("opts", [0, 0x17])
@pytest.mark.parametrize("n,n_ports,max_batch", [(64, 1, 64), (64, 3, 64), (300, 64, 300), (130, 2, 200)])
def test_conservation_order_and_a_stack_ring_that_takes_none_some_and_all(n, n_ports, max_batch, opts):
    """With a pool that has room every received address ends exactly once: on some TX ring, on the stack ring or on the
    pool.  The stack ring's new entries are the first s PASS descriptors in batch order, whole, `options` included; the
    pool's new entries behind the ports' free lists are the other frames that were not redirected, in batch order."""
    umem, descs, table = _case(n, n_ports, opts, seed=1)
    k = min(n, max_batch)
    probe = SS.spec_ingress_steer(umem.copy(), np.concatenate([descs[:k], np.zeros(max_batch - k, oracle.DESC_DTYPE)]),
                                  opts, table, SS.PASS, n_ports, SS.ALL_BOUND & ~2)["actions"][:k]
    q = int((probe == SS.XDP_PASS).sum())
    assert q >= 4, "the traffic passes too little for this test"
    for room, size, start in ((0, 8, 3), (1, 1, 0), (q // 2, 512, 0xFFFFFFFD), (q - 1, 512, 7), (q, 512, 0xFFFFFF00),
                              (q + 5, 1024, 0x80000000)):
        rx, fill, pool = _rx_state(512, 0xFFFFFFFD, descs, 0, 7, 600)
        txs = _rings(n_ports, [8, 64, 512, 16], 0xFFFFFFF0, [512, 0, 3, 512])
        stack = _stack(size, start, room)
        before, sb = [t.copy() for t in txs], stack.copy()
        got = PS.spec_step_pass(umem.copy(), rx, fill, txs, stack, pool, max_batch, opts, table, SS.PASS,
                                bound=SS.ALL_BOUND & ~2)
        res, acts = got["result"], got["actions"]
        assert (acts[:k] == probe).all()
        s = min(q, room)
        assert res["passed"] == s and res["pass_full"] == q - s and res["received"] == k
        assert stack.prod == (sb.prod + s) & RS.M32 and stack.cons == sb.cons
        on_stack = [stack.entries[stack.slot(sb.prod + j)] for j in range(s)]
        passes = [i for i in range(k) if acts[i] == SS.XDP_PASS]
        assert all(e == descs[i] for e, i in zip(on_stack, passes[:s])) and (descs["options"][passes] != 0).all()
        untouched = np.ones(stack.size, bool)
        untouched[[stack.slot(sb.prod + j) for j in range(s)]] = False
        assert (stack.entries[untouched] == sb.entries[untouched]).all()
        new_pool = [int(a) for a in pool.addr[7:pool.n()]]
        rest = [int(descs[i]["addr"]) for i in range(k) if acts[i] != SS.XDP_REDIRECT and i not in passes[:s]]
        assert new_pool[len(new_pool) - len(rest):] == rest and res["freed"] == len(new_pool)
        new = new_pool + [int(e["addr"]) for e in on_stack]
        for t, b in zip(txs, before):
            cnt = (t.prod - b.prod) & RS.M32
            new += [int(t.entries[t.slot(b.prod + j)]["addr"]) for j in range(cnt)]
        assert sorted(new) == sorted(int(a) for a in descs["addr"][:k]) and len(set(new)) == k
        assert res["freed"] + res["replied"] + res["passed"] == k


@pytest.mark.parametrize("start", [0, 0xFFFFFFFD])
def test_an_empty_rx_ring_changes_nothing(start):
    rx, fill, pool = _rx_state(8, start, np.zeros(0, oracle.DESC_DTYPE), 8, 11, 16)
    txs = _rings(3, [8, 4, 16], start, [8, 0, 5])
    stack = _stack(8, start, 5)
    before = [x.copy() for x in (rx, fill, pool, stack, *txs)]
    umem = np.arange(4096, dtype=np.uint8)
    st = dict.fromkeys(IS.KEYS, 0)
    got = PS.spec_step_pass(umem, rx, fill, txs, stack, pool, 4, 0x17, {}, 0, stats=st)
    assert got["result"] == dict.fromkeys(PS.RESULT_KEYS, 0) and not any(st.values())
    assert all(x.same(y) for x, y in zip(before, (rx, fill, pool, stack, *txs)))
    assert (umem == np.arange(4096, dtype=np.uint8)).all()


def test_end_is_total_for_garbage_words():
    """Action bytes that are none of 1, 2, 4 (freed, never passed), offsets above the bound, a received word above the
    bound, a stack ring with used > size (no room) and one whose words are far apart modulo 2^32."""
    n_max = 40
    descs = np.zeros(n_max, oracle.DESC_DTYPE)
    descs["addr"] = np.arange(n_max) * 2048 + 2048
    descs["options"] = 9
    d_tx, d_free = descs.copy(), (np.arange(n_max, dtype=np.uint64) + np.uint64(1000)) * np.uint64(4096)
    actions = np.array([2, 0, 3, 2, 4, 1, 0xFF, 2] * 5, np.uint8)
    counts = [dict(n_tx=0, n_tx_full=1, n_free=0) for _ in range(3)]
    plan = dict(received=1 << 31, refilled=9)

    def run(stack):
        rx, _, pool = _rx_state(64, 3, descs[:0], 0, 0, 50)
        txs = _rings(3, [8, 16, 4], 9, [8, 16, 4])
        return PS.spec_end_pass(rx, txs, stack, pool, plan, descs, actions, [0, 0, 0, 0], d_tx, d_free, counts, n_max), pool

    s = _stack(8, 0xFFFFFFFE, 8)
    res, pool = run(s)  # 15 PASS frames among 40, 5 REDIRECT: the ring takes 8, 27 are freed
    assert res == dict(received=40, redirected=0, replied=0, tx_full=3, refilled=9, freed=27, passed=8, pass_full=7)
    assert s.prod == 6 and [int(e["addr"]) for e in s.entries[[(0xFFFFFFFE + j) & 7 for j in range(8)]]] == \
        [int(descs[i]["addr"]) for i in range(40) if actions[i] == 2][:8]
    assert int(pool.addr[0]) == int(descs[1]["addr"])  # the byte 0 is a rest frame
    s = _stack(8, 5, 8)
    s.prod = (s.cons + 0x80000005) & RS.M32  # used > size
    res, _ = run(s)
    assert res["passed"] == 0 and res["pass_full"] == 15 and res["freed"] == 35


def test_ring_arithmetic_on_the_host_under_address_sanitizer():
    """tests/c/test_ring_pass.cpp: xsk_ring_pass.h's shares, slots, rest positions and workspace layouts, both paths
    replayed thread by thread into heap arrays of exactly the rings' and the pool's sizes, against the rule stated
    sequentially; the case matrix of its header comment."""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "t")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "c", "test_ring_pass.cpp")], check=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    assert "ring pass ok" in res.stdout
