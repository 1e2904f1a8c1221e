"""xsk_gpu_rx_queues_dev (Python: rx_queues_dev) and its two host calls without a GPU: the ABI surface and the export-name
rules; the block's size; every -EINVAL of xsk_gpu_rx_fused_loop_dev reached through xsk_gpu_rx_queues_prepare with
fabricated pointers (no device call is reached), with the offending queue first and last of three, the fused call
refusing the same queue and the block left untouched to the byte; the sharing rules between queues; the bytes of a valid
block; what the launching call refuses before any device call; the new files' own text; and the block's layout, writer
and header check compiled for the host under AddressSanitizer (tests/c/test_rx_queues.cpp)."""
import ctypes as C
import errno
import os
import re
import subprocess
import tempfile

import numpy as np

from tests.conftest import ROOT
from tests.test_rx_dev_spec import MAX_BATCH, _bad_pools, _bad_rings, _decl, _header, _pool, _ring, _struct
from tests.test_rx_loop_fused_spec import _loop_fn
from tests.test_rx_steer_spec import _ports
from tests.test_tx_complete_rings_spec import RESERVED, _comps, _exports

EINVAL = -errno.EINVAL
NAMES = ["xsk_gpu_rx_queues_block_size", "xsk_gpu_rx_queues_dev", "xsk_gpu_rx_queues_prepare"]
FUSED = "xsk_gpu_rx_fused_loop_dev"
CSRC = os.path.join(ROOT, "xsknet_amd", "csrc")
NEW_FILES = ("xsk_rx_queues.hip", "xsk_rx_queues_ds.hip", "xsk_rx_queues.h")
LOWLAT_MAX, MAX_QUEUES = 1024, 1024
MAGIC = 0x51525358
SHIFT = 0x100000000  # queue k's fabricated pointers lie k * SHIFT above queue 0's
SENTINEL = 0xEE


def _ptr_of(x):
    return None if x is None else C.pointer(x)


def _queue(X, um=0x600000, size=1 << 20, rx=None, fill=None, tx=None, stack=None, pool=None, mb=64, np_=3, tab=None, ne=0,
           dp=0, bnd=None, act=None, por=None, co=None, st=None, pst=None, res=None, comp=None, nc=4, cm=64, mv=None,
           pu=None, ws=None):
    """A struct xsk_gpu_rx_queue from ring structs, arrays (or None) and integers; what it points to is kept on it."""
    q = X.RxQueue(um, size, _ptr_of(rx), _ptr_of(fill), tx, _ptr_of(stack), _ptr_of(pool), tab, bnd, act, por, co, st, pst,
                  res, comp, mv, pu, ws, mb, np_, ne, dp, nc, cm)
    q._keep = (rx, fill, tx, stack, pool, comp)
    return q


def _good(X, k, **kw):
    """A valid queue whose every pointer lies k * SHIFT above _loop_fn's fabricated ones: no two of them share any."""
    b = k * SHIFT
    a = dict(um=0x600000 + b, rx=_ring(X, 0x100000 + b), fill=_ring(X, 0x200000 + b), stack=_ring(X, 0x300000 + b),
             tx=_ports(X, 3, 0x1000000 + b), comp=_comps(X, 4, 0x2000000 + b),
             pool=_pool(X, d_addr=0x900000 + b, d_n_free=0x910000 + b), res=0x550000 + b, st=0x560000 + b,
             ws=0x570000 + b, mv=0x580000 + b, pu=0x5F0000 + b)
    a.update(kw)
    return _queue(X, **a)


def _prepare(X, queues, opts=0, fill=SENTINEL):
    """(return value, the block as written) of xsk_gpu_rx_queues_prepare over a block filled with `fill` first."""
    n = len(queues)
    block = np.full(max(X.rx_queues_block_size(n), 64), fill, np.uint8)
    arr = (X.RxQueue * max(n, 1))(*queues)
    return X.lib().xsk_gpu_rx_queues_prepare(arr, n, opts, block.ctypes.data), block


def _words(block, at, n):
    return [int(x) for x in block[at:at + 4 * n].view("<u4")]


def test_header_declares_and_library_exports_the_entry_points():
    import xsknet_amd as X
    assert _decl("size_t", NAMES[0]) == "uint32_t n_queues"
    assert _decl("int", NAMES[2]) == "const struct xsk_gpu_rx_queue* queues, uint32_t n_queues, uint32_t opts, void* h_block"
    assert _decl("int", NAMES[1]) == "const void* d_block, uint32_t n_queues, uint32_t opts, void* stream"
    assert re.search(r"#define\s+XSK_GPU_RX_MAX_QUEUES\s+1024u\b", _header()) and X.RX_MAX_QUEUES == MAX_QUEUES
    # the struct: the fused call's parameters but opts and stream, every one under its own name; ctypes in the same order
    fields = re.findall(r"(\w+)\s*[;,]", _struct("xsk_gpu_rx_queue"))
    fused = re.findall(r"(\w+)\s*(?:,|$)", _decl("int", FUSED))
    assert sorted(fields) == sorted(set(fused) - {"opts", "stream"}) and len(fields) == 25
    assert [f[0] for f in X.RxQueue._fields_] == fields and C.sizeof(X.RxQueue) == 176
    exported = _exports()
    assert sorted(s for s in exported if "queues" in s and s.startswith("xsk_gpu_rx")) == NAMES
    assert sorted(s for s in exported if "rx_queue" in s) == NAMES  # all the library gained: the rest is hidden or static
    for name in NAMES:
        assert hasattr(X.lib(), name) and name in X._SIGS
        assert not [s for s in RESERVED + ("rx_loop", "complete_rings", "fused") if s in name], name
    for py in ("RxQueue", "RX_MAX_QUEUES", "rx_queue", "rx_queues_block_size", "rx_queues_prepare", "rx_queues_dev"):
        assert py in X.__all__ and hasattr(X, py)
    assert X.lib().xsk_gpu_abi_version() == 1
    assert not re.search(r"struct\s+xsk_gpu_\w*(complete|loop|fused)\w*\s*\{", _header())
    mk = open(os.path.join(ROOT, "Makefile")).read()
    for f in ("xsk_rx_queues.o", "xsk_rx_queues_ds.o", "xsk_rx_queues.h"):
        assert f in mk
    assert re.search(r"xsk_rx_queues_ds\.o:.*\n\t.*-pragma-unroll-threshold=32768", mk)


def test_block_size():
    import xsknet_amd as X
    size = X.lib().xsk_gpu_rx_queues_block_size
    assert size(0) == 0 and size(MAX_QUEUES + 1) == 0 and size(0xFFFFFFFF) == 0
    stride = size(2) - size(1)
    # a record is the fused kernel's explicit arguments: with 256 B of hidden ones, at most an argument segment
    hdr = open(os.path.join(CSRC, "xsk_rx_queues.h")).read()
    record = int(re.search(r"kRqRecordBytes = (\d+);", hdr).group(1))
    src = open(os.path.join(CSRC, "xsk_rx_queues.hip")).read()
    assert re.search(r"static_assert\(sizeof\(LoopFusedArgs\) == kRqRecordBytes", src)
    assert stride >= record and record + 256 <= 4096 and stride % 64 == 0 and stride - record < 64
    for n in (1, 2, 3, 64, 272, MAX_QUEUES):
        assert size(n) == 64 + n * stride == X.rx_queues_block_size(n)


def _both(X):
    """loop(**kw) with the keywords and defaults of _loop_fn's: EINVAL when the fused call refuses the queue AND prepare
    refuses it first of three and last of three with the block untouched; anything else fails the test at once."""
    fused, (rx, fill, stack, pool, res, st, ws, um, mv, pu) = _loop_fn(X, FUSED)
    good = [_good(X, 1), _good(X, 2)]
    assert _prepare(X, good)[0] == 0

    def loop(rx=rx, fill=fill, tx=None, stack=stack, pool=pool, mb=64, opts=0, np_=3, ws=ws, um=um, size=1 << 20,
             comp=None, nc=4, cm=64, mv=mv, pu=pu, tab=None, ne=0, dp=0, bnd=None, co=None, st=st, pst=None, res=res):
        tx = _ports(X, max(min(np_, 64), 1)) if tx is None else tx
        comp = _comps(X, max(min(nc, 65), 1)) if comp is None else comp
        assert fused(rx=rx, fill=fill, tx=tx, stack=stack, pool=pool, mb=mb, opts=opts, np_=np_, ws=ws, um=um, size=size,
                     comp=comp, nc=nc, cm=cm, mv=mv, pu=pu, tab=tab, ne=ne, dp=dp, bnd=bnd, co=co, st=st, pst=pst,
                     res=res) == EINVAL
        bad = _queue(X, um=um, size=size, rx=rx, fill=fill, tx=tx if tx != 0 else None, stack=stack, pool=pool, mb=mb,
                     np_=np_, tab=tab, ne=ne, dp=dp, bnd=bnd, co=co, st=st, pst=pst, res=res,
                     comp=comp if comp != 0 else None, nc=nc, cm=cm, mv=mv, pu=pu, ws=ws)
        for queues in ([bad] + good, good + [bad]):
            rc, block = _prepare(X, queues, opts)
            assert rc == EINVAL and (block == SENTINEL).all(), "refused, and the block untouched"
        return EINVAL

    return loop, (rx, fill, stack, pool, res, st, ws, um, mv, pu)


def test_every_einval_of_the_fused_call_through_prepare():
    """The lists of tests/test_rx_loop_fused_spec.py -- the completion call's rules, the aliasing with the step's rings,
    the step's rules, the two bounds of the one-workgroup form, a ring the packed form cannot carry -- each through the
    fused call and through prepare, where the offending queue stands first and last among two valid ones."""
    import xsknet_amd as X
    loop, (rx, fill, stack, pool, res, st, ws, um, mv, pu) = _both(X)
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
    assert loop(comp=0, nc=0, cm=0xFFFFFFFF, mv=mv + 1, pu=pu + 2, ws=None) == EINVAL
    # the bounds of the one-workgroup form, and a ring the packed form cannot carry
    for mb in (LOWLAT_MAX + 1, 1300, 70000, MAX_BATCH):
        assert loop(mb=mb) == EINVAL and loop(mb=mb, comp=0, nc=0) == EINVAL
    for cm in (LOWLAT_MAX + 1, 1300, MAX_BATCH):
        assert loop(cm=cm, nc=1) == EINVAL and loop(cm=cm, nc=65) == EINVAL
    assert loop(rx=_ring(X, 0x100000, d_ring=1 << 56)) == EINVAL
    t = _ports(X, 3)
    t[2].d_ring = (1 << 60) + 0x1000
    assert loop(tx=t) == EINVAL
    comp = _comps(X, 4)
    comp[3].d_ring = 0xFF00000000001000
    assert loop(comp=comp) == EINVAL


def test_the_two_statements_of_the_fused_rules_are_one():
    """fused_ok() stays in xsk_loop_fused.hip (a test reads it there); prepare's queue_ok() states its three extra rules
    again.  Held together here: the same three statements over the same loop_complete_ok(), in the same order, and the
    values on either side of each bound accepted and refused alike (complete_max 1025 with n_comp 0 passes both)."""
    import xsknet_amd as X

    def rules(path, start, end):
        code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, path)).read())
        body = code[code.index(start):]
        body = body[:body.index(end)]
        body = re.sub(r"\bq\.", "", body)
        at = body.index("return false;") + len("return false;")  # behind the call of loop_complete_ok
        assert "loop_complete_ok(" in body[:at]
        return re.sub(r"\s+", " ", re.sub(r"\b(q|c)\b", "i", body[at:])).strip()

    assert rules("xsk_loop_fused.hip", "bool fused_ok(", "\n}\n") == rules("xsk_rx_queues.hip", "bool queue_ok(", "\n}\n")
    fused = _loop_fn(X, FUSED)[0]
    for kw, ok in ((dict(mb=1024), True), (dict(mb=1025), False), (dict(cm=1024), True), (dict(cm=1025), False),
                   (dict(cm=1025, nc=0, comp=0), True), (dict(cm=0), True)):
        q = _good(X, 0, **{k: (None if k == "comp" else v) for k, v in kw.items()})
        assert (_prepare(X, [q])[0] == 0) == ok, kw
        if not ok:
            assert fused(**kw) == EINVAL


def test_count_and_null_rules_of_prepare():
    import xsknet_amd as X
    L = X.lib()
    q = (X.RxQueue * 3)(_good(X, 0), _good(X, 1), _good(X, 2))
    block = np.full(X.rx_queues_block_size(3), SENTINEL, np.uint8)
    assert L.xsk_gpu_rx_queues_prepare(None, 3, 0, block.ctypes.data) == EINVAL
    assert L.xsk_gpu_rx_queues_prepare(q, 3, 0, None) == EINVAL
    assert L.xsk_gpu_rx_queues_prepare(q, 0, 0, block.ctypes.data) == EINVAL
    assert L.xsk_gpu_rx_queues_prepare(q, MAX_QUEUES + 1, 0, block.ctypes.data) == EINVAL
    assert L.xsk_gpu_rx_queues_prepare(q, 0xFFFFFFFF, 0, block.ctypes.data) == EINVAL
    for opts in (0x8, 0x20, 0x18):
        assert L.xsk_gpu_rx_queues_prepare(q, 3, opts, block.ctypes.data) == EINVAL
    assert (block == SENTINEL).all()
    assert L.xsk_gpu_rx_queues_prepare(q, 3, 0x17, block.ctypes.data) == 0 and not (block == SENTINEL).all()
    try:
        X.rx_queues_prepare([_good(X, 0), _good(X, 0)])
        raise AssertionError("two identical queues were accepted")
    except X.XskGpuError as e:
        assert e.rc == EINVAL
    assert X.rx_queues_prepare([_good(X, 0), _good(X, 1)], 0x7).nbytes == X.rx_queues_block_size(2)


def test_two_queues_may_not_share_a_pointer_the_kernel_writes_through():
    import xsknet_amd as X
    a = _good(X, 0)
    k = a._keep  # (rx, fill, tx, stack, pool, comp)

    def other(**kw):
        return _good(X, 1, **kw)

    def ring_with(base, **kw):
        return _ring(X, base + SHIFT, **kw)

    shared = {
        "rx d_producer": other(rx=ring_with(0x100000, d_producer=k[0].d_producer)),
        "rx d_consumer": other(rx=ring_with(0x100000, d_consumer=k[0].d_consumer)),
        "rx d_ring": other(rx=ring_with(0x100000, d_ring=k[0].d_ring)),
        "fill d_ring": other(fill=ring_with(0x200000, d_ring=k[1].d_ring)),
        "stack d_producer": other(stack=ring_with(0x300000, d_producer=k[3].d_producer)),
        "rx of one, fill of the other": other(rx=ring_with(0x100000, d_consumer=k[1].d_consumer)),
        "pool d_n_free": other(pool=_pool(X, d_addr=0x900000 + SHIFT, d_n_free=k[4].d_n_free)),
        "pool d_addr": other(pool=_pool(X, d_addr=k[4].d_addr, d_n_free=0x910000 + SHIFT)),
        "workspace": other(ws=a.d_workspace),
        "d_stats": other(st=a.d_stats),
        "d_res": other(res=a.d_res),
        "d_moved": other(mv=a.d_moved),
        "d_pushed": other(pu=a.d_pushed),
        "d_actions": (_good(X, 0, act=0x5A0000), other(act=0x5A0000)),
        "d_ports": (_good(X, 0, por=0x5A8000), other(por=0x5A8000)),
        "d_port_counts": (_good(X, 0, co=0x540000), other(co=0x540000)),
        "d_port_stats": (_good(X, 0, pst=0x5E0000), other(pst=0x5E0000)),
        "one queue's d_res, the other's d_stats": other(st=a.d_res),
    }
    tx = _ports(X, 3, 0x1000000 + SHIFT)
    tx[2].d_producer = k[2][1].d_producer
    shared["a port's d_producer"] = other(tx=tx)
    comp = _comps(X, 4, 0x2000000 + SHIFT)
    comp[3].d_ring = k[5][0].d_ring
    shared["a completion ring's d_ring"] = other(comp=comp)
    comp = _comps(X, 4, 0x2000000 + SHIFT)
    comp[0].d_consumer = k[5][2].d_consumer
    shared["a completion ring's d_consumer"] = other(comp=comp)
    for name, b in shared.items():
        first, b = b if isinstance(b, tuple) else (a, b)
        for queues in ([first, b], [b, first], [first, _good(X, 2), b], [b, _good(X, 3), _good(X, 2), first]):
            rc, block = _prepare(X, queues)
            assert rc == EINVAL and (block == SENTINEL).all(), name
    # d_moved and d_pushed are ignored without completion rings, as the fused call ignores them
    assert _prepare(X, [_good(X, 0, nc=0, comp=None), other(nc=0, comp=None, mv=a.d_moved, pu=a.d_pushed)])[0] == 0
    # what may be shared: the table, the bound word, the UMEM
    tab, bnd = 0x5B0000, 0x5C0000
    assert _prepare(X, [_good(X, 0, tab=tab, ne=4), other(tab=tab, ne=4)])[0] == 0
    assert _prepare(X, [_good(X, 0, bnd=bnd), other(bnd=bnd)])[0] == 0
    assert _prepare(X, [a, other(um=a.d_umem)])[0] == 0
    assert _prepare(X, [_good(X, 0, tab=tab, ne=9, bnd=bnd), other(tab=tab, ne=9, bnd=bnd, um=a.d_umem),
                        _good(X, 2, tab=tab, ne=9, bnd=bnd, um=a.d_umem)], 0x17)[0] == 0
    assert open(os.path.join(CSRC, "xsk_rx_queues.hip")).read().count("std::sort(") == 1  # sorted, not a quadratic loop


def test_the_bytes_of_a_valid_block():
    import xsknet_amd as X
    queues = [_good(X, 0, np_=3, nc=4), _good(X, 1, tx=_ports(X, 64, 0x1000000 + SHIFT), np_=64, mb=1024, cm=0,
                                              comp=_comps(X, 65, 0x2000000 + SHIFT), nc=65, tab=0x5B0000, ne=7, dp=5),
              _good(X, 2, stack=None, nc=0, comp=None, mb=1, np_=1, tx=_ports(X, 1, 0x1000000 + 2 * SHIFT), bnd=0x5C0000)]
    rc, block = _prepare(X, queues, 0x17, fill=0xEE)
    rc2, again = _prepare(X, queues, 0x17, fill=0x11)
    assert rc == 0 and rc2 == 0 and (block == again).all(), "deterministic, padding zeroed"
    stride = X.rx_queues_block_size(2) - X.rx_queues_block_size(1)
    record = int(re.search(r"kRqRecordBytes = (\d+);", open(os.path.join(CSRC, "xsk_rx_queues.h")).read()).group(1))
    assert block.nbytes == 64 + 3 * stride
    assert _words(block, 0, 6) == [MAGIC, X.lib().xsk_gpu_abi_version(), 3, 0x17, stride, record]
    assert not block[24:64].any()
    for q, queue in enumerate(queues):
        rc, alone = _prepare(X, [queue], 0x17)
        assert rc == 0 and _words(alone, 0, 4) == [MAGIC, 1, 1, 0x17]
        assert (block[64 + q * stride:64 + (q + 1) * stride] == alone[64:64 + stride]).all(), q
        assert not block[64 + q * stride + record:64 + (q + 1) * stride].any()
    # a record's rings, unpacked as xsk_ring_pack.h packs them: tx[64], comp[65], rx, fill, stack
    def ring(q, k):
        w = _words(block, 64 + q * stride + 24 * k, 6)
        return w[0] | w[1] << 32, w[2] | w[3] << 32, w[4] | (w[5] & 0xFFFFFF) << 32, 1 << (w[5] >> 24)

    absent = (0, 0, 0, 1)
    for q, queue in enumerate(queues):
        rx, fill, tx, stack, pool, comp = queue._keep
        for p in range(64):
            assert ring(q, p) == ((tx[p].d_producer, tx[p].d_consumer, tx[p].d_ring, tx[p].size) if p < queue.n_ports else absent)
        for c in range(65):
            assert ring(q, 64 + c) == ((comp[c].d_producer, comp[c].d_consumer, comp[c].d_ring, comp[c].size)
                                       if c < queue.n_comp else absent)
        for k, r in ((129, rx), (130, fill), (131, stack)):
            assert ring(q, k) == (absent if r is None else (r.d_producer, r.d_consumer, r.d_ring, r.size))
    # other options, other bytes: the header's word and every record's
    rc, other = _prepare(X, queues, 0x7)
    assert rc == 0 and _words(other, 0, 4) == [MAGIC, 1, 3, 0x7] and (other[64:64 + stride] != block[64:64 + stride]).any()


def test_the_launching_call_refuses_before_any_device_call():
    """On a machine with no GPU these return -EINVAL, not an error of the runtime: nothing was asked of a device."""
    import xsknet_amd as X
    dev = X.lib().xsk_gpu_rx_queues_dev
    ok = 0x7F0000001000
    assert dev(None, 1, 0, None) == EINVAL
    for mis in (1, 2, 4, 8, 16, 32, 48):
        assert dev(ok + mis, 1, 0, None) == EINVAL
    for n in (0, MAX_QUEUES + 1, 0xFFFFFFFF):
        assert dev(ok, n, 0, None) == EINVAL
    for opts in (0x8, 0x20, 0x18, 0xFFFFFFFF):
        assert dev(ok, 1, opts, None) == EINVAL
    try:
        X.rx_queues_dev(None, 1, 0, stream=0)
        raise AssertionError("a NULL block was accepted")
    except X.XskGpuError as e:
        assert e.rc == EINVAL


def test_every_rule_stands_in_front_of_the_one_launch():
    """The new files' own text, as the fused call's spec test reads its files."""
    src = open(os.path.join(CSRC, "xsk_rx_queues.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    pub = code[code.index('extern "C" {'):]
    assert re.findall(r"^(?:int|size_t) (\w+)\(", pub, re.M) == [NAMES[0], NAMES[2], NAMES[1]]
    body = pub[pub.index("int " + NAMES[1] + "("):]
    body = body[:body.index("\n}\n")]
    assert body.count("return -EINVAL") == 1 and body.index("return -EINVAL") < body.index("_launch(")
    for rule in ("!d_block", "(uintptr_t)d_block & (kRqAlign - 1u)", "!rq_count_ok(n_queues)", "opts & ~XSK_GPU_OPT_MASK"):
        assert rule in body[:body.index("return -EINVAL")], rule
    launch = code[code.index("int queues_launch("):code.index('extern "C" {')]
    assert launch.count("<<<") == 2 and launch.count("xsk_gpu__rx_queues_ds_launch(") == 1
    assert launch.count("dim3(n_queues), dim3(kLfThreads)") == 2
    prep = pub[pub.index("int " + NAMES[2] + "("):pub.index("int " + NAMES[1] + "(")]
    assert prep.index("queue_ok(") < prep.index("queues_disjoint(") < prep.index("rq_write_block<")  # checks, then writes
    for word in ("hip", "<<<"):
        assert word not in prep, "prepare is host only: no device call"
    for f in NEW_FILES:
        c = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())
        for word in ("hipMemsetAsync", "hipMemcpy", "hipMalloc", "Synchronize", "asm", "atomicAdd", "__restrict__"):
            assert word not in c, (f, word)
    ds = open(os.path.join(CSRC, "xsk_rx_queues_ds.hip")).read()
    for text in (src, ds):
        assert re.search(r"static_assert\(sizeof\(QueuesLds\) <= 160u \* 1024u", text)
        assert "__launch_bounds__(kLfThreads, 1)" in text
        assert "rq_stage(block, n_queues, opts, M.S)) return;" in text
        assert text.index("rq_stage(") < text.index("loop_fused_body<")
    assert "loop_fused_body<RoundCfg<WIRE, true>>(M.S.a, M.L)" in src and "loop_fused_body<RoundCfg<true, true, true>>(M.S.a, M.L)" in ds
    assert ds.count("<<<") == 1 and "dim3(n_queues), dim3(kLfThreads)" in ds
    # the header check stands in front of the first store of the staging function, and the stride is a constant
    hdr = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "xsk_rx_queues.h")).read())
    stage = hdr[hdr.index("bool rq_stage("):]
    assert stage.index("rq_header_ok(") < stage.index("return false;") < stage.index("S.v[k] =")
    assert "h1.x" not in stage[stage.index("return false;"):], "no word of the block is an offset"


def test_the_block_on_the_host_under_address_sanitizer():
    """tests/c/test_rx_queues.cpp: blocks of 1, 2 and 1024 queues written into heap arrays of exactly block_size bytes,
    every ring of every record unpacked and compared, no byte outside the block touched, the header check against each
    mismatch.  A stand-alone program: nothing loaded into Python runs under a sanitizer."""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "t")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "c", "test_rx_queues.cpp")], check=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    assert "rx queues ok" in res.stdout
