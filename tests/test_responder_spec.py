"""xsk_gpu_responder_dev, xsk_gpu_responder_queues_dev and their two host calls without a GPU: the ABI
surface and the export-name rules; every -EINVAL with fabricated pointers (no device call is made before the checks, and
no accepted call is made here: acceptance is read from xsk_gpu_responder_prepare, which is host only); the sharing rule
between queues; the block's size, header and bytes; the new files' own text, the two statements of the serve body held
against each other; the block's layout compiled for the host under AddressSanitizer (tests/c/test_responder.cpp); and
what the seed set of the randomised GPU tests reaches, from the spec alone."""
import ctypes as C
import errno
import os
import re
import subprocess
import tempfile

import numpy as np

from tests import loop_world as LW
from tests import responder_seeds as SEEDS
from tests.conftest import ROOT
from tests.test_rx_dev_spec import _bad_rings, _decl, _header, _pool, _ring, _struct
from tests.test_rx_queues_spec import MAGIC as RQ_MAGIC
from tests.test_rx_queues_spec import SHIFT, _good, _words
from tests.test_rx_steer_spec import _ports
from tests.test_tx_complete_rings_spec import _comps, _exports

EINVAL = -errno.EINVAL
NAMES = ["xsk_gpu_responder_block_size", "xsk_gpu_responder_dev", "xsk_gpu_responder_prepare", "xsk_gpu_responder_queues_dev"]
RESERVED = ("fused", "rx_loop", "complete_rings", "rx_queue", "neigh", "ng_", "pass", "egress", "rd_", "rp_", "ring_dev",
            "ring_ports")
CSRC = os.path.join(ROOT, "xsknet_amd", "csrc")
SENTINEL = 0xEE
MAGIC = 0x50525358
NTABLE = 0x5D0000  # read only: every queue may use the one table


def _rq(X, q, up=None, nt=NTABLE, nn=16, ns=None, nr=None, smax=64):
    r = X.ResponderQueue(q, None if up is None else C.pointer(up), nt, ns, nr, nn, smax)
    r._keep = (q, up)
    return r


def _rgood(X, k, q=None, **kw):
    """A valid queue whose every pointer lies k * SHIFT above queue 0's."""
    b = k * SHIFT
    a = dict(up=_ring(X, 0x400000 + b), ns=0x5D8000 + b, nr=0x5DC000 + b)
    a.update(kw)
    return _rq(X, _good(X, k) if q is None else q, **a)


def _prepare(X, queues, opts=0, fill=SENTINEL):
    n = len(queues)
    block = np.full(max(X.responder_block_size(n), 64), fill, np.uint8)
    arr = (X.ResponderQueue * max(n, 1))(*queues)
    return X.lib().xsk_gpu_responder_prepare(arr, n, opts, block.ctypes.data), block


def _refused(X, r, opts=0):
    """The one-queue call refuses `r`, and prepare refuses it first and last of three with the block untouched.  Prepare,
    which is host only, is asked first: the device call is made only with what prepare has refused on its own."""
    if _prepare(X, [r], opts)[0] != EINVAL or X.lib().xsk_gpu_responder_dev(C.byref(r), opts, None) != EINVAL:
        return False
    for queues in ([r, _rgood(X, 1), _rgood(X, 2)], [_rgood(X, 1), _rgood(X, 2), r]):
        rc, block = _prepare(X, queues, opts)
        if rc != EINVAL or not (block == SENTINEL).all():
            return False
    return True


def test_header_declares_and_library_exports_the_entry_points():
    import xsknet_amd as X
    assert _decl("int", NAMES[1]) == "const struct xsk_gpu_responder_queue* r, uint32_t opts, void* stream"
    assert _decl("size_t", NAMES[0]) == "uint32_t n_queues"
    assert _decl("int", NAMES[2]) == ("const struct xsk_gpu_responder_queue* queues, uint32_t n_queues, uint32_t opts, "
                                      "void* h_block")
    assert _decl("int", NAMES[3]) == "const void* d_block, uint32_t n_queues, uint32_t opts, void* stream"
    fields = re.findall(r"(\w+)\s*[;,]", _struct("xsk_gpu_responder_queue"))
    assert fields == ["q", "up", "d_ntable", "d_nstats", "d_nres", "n_nentries", "serve_max"]
    assert [f[0] for f in X.ResponderQueue._fields_] == fields
    assert C.sizeof(X.ResponderQueue) == C.sizeof(X.RxQueue) + 3 * 8 + 8 + 2 * 4 == 216
    assert X.ResponderQueue.q.offset == 0 and X.ResponderQueue.up.offset == 176 and X.ResponderQueue.serve_max.offset == 212
    exported = _exports()
    assert sorted(s for s in exported if "responder" in s) == NAMES
    for name in NAMES:
        assert hasattr(X.lib(), name) and name in X._SIGS
        assert not [s for s in RESERVED if s in name], name
        assert not (name.startswith("xsk_gpu_rx") and "queues" in name)
    for py in ("ResponderQueue", "responder_queue", "responder_dev", "responder_block_size", "responder_prepare",
               "responder_queues_dev"):
        assert py in X.__all__ and hasattr(X, py)
    assert X.lib().xsk_gpu_abi_version() == 1
    assert not re.search(r"struct\s+xsk_gpu_\w*(complete|loop|fused)\w*\s*\{", _header())
    mk = open(os.path.join(ROOT, "Makefile")).read()
    for f in ("xsk_responder.o", "xsk_responder_ds.o", "xsk_responder_body.h", "xsk_responder_block.h", "xsk_neigh_device.h"):
        assert f in mk
    assert re.search(r"xsk_responder_ds\.o:.*\n\t.*-pragma-unroll-threshold=32768", mk)


def test_every_rule_of_either_half_and_the_new_rules():
    import xsknet_amd as X
    assert _prepare(X, [_rgood(X, 0), _rgood(X, 1), _rgood(X, 2)])[0] == 0
    assert X.lib().xsk_gpu_responder_dev(None, 0, None) == EINVAL
    try:
        X.responder_dev(None, stream=0)
        raise AssertionError("a NULL struct was accepted")
    except X.XskGpuError as e:
        assert e.rc == EINVAL

    def bad(opts=0, **kw):  # a queue of _good() with these fields changed
        return _refused(X, _rgood(X, 0, q=_good(X, 0, **kw)), opts)

    # ---- the fused call's rules, each once ----
    for b in _bad_rings(X, 0x100000, 16):
        assert bad(rx=b)
    for b in _bad_rings(X, 0x200000, 8)[1:]:
        assert bad(fill=b)
    assert bad(pool=None) and bad(pool=_pool(X, capacity=0)) and bad(pool=_pool(X, d_n_free=0x910001))
    assert bad(tx=None) and bad(np_=0) and bad(np_=65)
    t = _ports(X, 3)
    t[2] = _ring(X, 0x1020000, size=100)
    assert bad(tx=t)
    t = _ports(X, 3)
    t[2].d_producer = t[0].d_producer
    assert bad(tx=t)
    assert bad(mb=0) and bad(mb=1025) and bad(opts=0x8) and bad(opts=0x20) and bad(opts=0xFFFFFFFF)
    assert bad(ws=None) and bad(ws=0x570008) and bad(um=None) and bad(um=0x600004) and bad(size=(1 << 20) + 8)
    assert bad(st=0x560004) and bad(pst=0x5E0004) and bad(bnd=0x5C0004) and bad(res=0x550002) and bad(co=0x540002)
    assert bad(tab=None, ne=1) and bad(tab=0x5B0004, ne=4) and bad(tab=0x5B0000, ne=1025) and bad(dp=3) and bad(dp=0x100)
    assert bad(comp=None) and bad(nc=66) and bad(cm=1025) and bad(mv=0x580002) and bad(pu=0x5F0001)
    c = _comps(X, 4)
    c[3].d_ring = c[1].d_ring
    assert bad(comp=c)
    c = _comps(X, 4)
    c[2].d_consumer = 0x100000 + 0x100  # the RX ring's
    assert bad(comp=c)
    assert bad(rx=_ring(X, 0x100000, d_ring=1 << 56))  # a ring the packed form cannot carry
    s = _ring(X, 0x300000, d_producer=0x100000)        # the stack ring's producer word is the RX ring's
    assert bad(stack=s)
    # ---- the serve call's rules, each once ----
    for b in _bad_rings(X, 0x400000, 16)[1:]:
        assert _refused(X, _rgood(X, 0, up=b))
    assert _refused(X, _rgood(X, 0, up=_ring(X, 0x400000, d_ring=(1 << 56) + 0x1000)))
    for smax in (0, 1025, 0xFFFFFFFF):
        assert _refused(X, _rgood(X, 0, smax=smax))
    assert _prepare(X, [_rgood(X, 0, smax=1024)])[0] == 0 and _prepare(X, [_rgood(X, 0, smax=1)])[0] == 0
    assert _refused(X, _rgood(X, 0, nn=1025)) and _refused(X, _rgood(X, 0, nt=None, nn=1))
    assert _prepare(X, [_rgood(X, 0, nt=None, nn=0)])[0] == 0
    for mis in (1, 2, 4):
        assert _refused(X, _rgood(X, 0, nt=NTABLE + mis)) and _refused(X, _rgood(X, 0, ns=0x5D8000 + mis))
    for mis in (1, 2, 3):
        assert _refused(X, _rgood(X, 0, nr=0x5DC000 + mis))
    assert _prepare(X, [_rgood(X, 0, ns=None, nr=None)])[0] == 0
    # what the serve call refuses and the fused call accepts: a consumer word shared between two ports, or between the
    # stack ring and a port
    t = _ports(X, 3)
    t[2].d_consumer = t[0].d_consumer
    assert bad(tx=t)
    s = _ring(X, 0x300000)
    s.d_consumer = _ports(X, 3)[1].d_consumer
    assert bad(stack=s)
    # ---- the new rules ----
    assert bad(stack=None)
    assert _refused(X, _rq(X, _good(X, 0), up=None, ns=0x5D8000, nr=0x5DC000))
    q = _good(X, 0, tx=_ports(X, 64), np_=64, comp=_comps(X, 65), nc=65)
    rx, fill, tx, stack, pool, comp = q._keep
    assert _prepare(X, [_rgood(X, 0, q=q)])[0] == 0
    for name, other in (("rx", rx), ("fill", fill), ("tx[0]", tx[0]), ("tx[17]", tx[17]), ("tx[63]", tx[63]),
                        ("stack", stack), ("comp[0]", comp[0]), ("comp[9]", comp[9]), ("comp[64]", comp[64])):
        for f in ("d_ring", "d_producer", "d_consumer"):
            up = _ring(X, 0x400000)
            setattr(up, f, getattr(other, f))
            assert _refused(X, _rgood(X, 0, q=q, up=up)), (name, f)
    # (a completion ring the call does not use may share with up: n_comp == 0 ignores comp)
    up = _ring(X, 0x400000, d_ring=comp[0].d_ring)
    assert _prepare(X, [_rgood(X, 0, q=_good(X, 0, nc=0, comp=None), up=up)])[0] == 0


def test_two_queues_may_not_share_a_pointer_the_kernel_writes_through():
    import xsknet_amd as X
    a = _rgood(X, 0)
    up = a._keep[1]
    shared = {
        "up d_ring": _rgood(X, 1, up=_ring(X, 0x400000 + SHIFT, d_ring=up.d_ring)),
        "up d_producer": _rgood(X, 1, up=_ring(X, 0x400000 + SHIFT, d_producer=up.d_producer)),
        "up d_consumer": _rgood(X, 1, up=_ring(X, 0x400000 + SHIFT, d_consumer=up.d_consumer)),
        "d_nstats": _rgood(X, 1, ns=a.d_nstats),
        "d_nres": _rgood(X, 1, nr=a.d_nres),
        "one queue's up, the other's stack": _rgood(X, 1, up=_ring(X, 0x400000 + SHIFT, d_ring=a.q.stack.contents.d_ring)),
        "one queue's d_nres, the other's d_res": _rgood(X, 1, nr=a.q.d_res),
        "the list of the rx-queues call still holds: d_workspace": _rgood(X, 1, q=_good(X, 1, ws=a.q.d_workspace)),
        "and a port's d_producer": _rgood(X, 1, q=_good(X, 1, st=a.q.d_stats)),
    }
    for name, b in shared.items():
        for queues in ([a, b], [b, a], [a, _rgood(X, 2), b], [b, _rgood(X, 3), _rgood(X, 2), a]):
            rc, block = _prepare(X, queues)
            assert rc == EINVAL and (block == SENTINEL).all(), name
    # d_ntable is read only and may be shared, as the steering table, the bound word and the UMEM may
    assert a.d_ntable == _rgood(X, 1).d_ntable == NTABLE and _prepare(X, [a, _rgood(X, 1), _rgood(X, 2)], 0x17)[0] == 0
    assert _prepare(X, [a, _rgood(X, 1, q=_good(X, 1, um=a.q.d_umem, tab=0x5B0000, ne=4, bnd=0x5C0000))])[0] == 0
    try:
        X.responder_prepare([_rgood(X, 0), _rgood(X, 0)])
        raise AssertionError("two identical queues were accepted")
    except X.XskGpuError as e:
        assert e.rc == EINVAL
    assert open(os.path.join(CSRC, "xsk_responder.hip")).read().count("std::sort(") == 1


def test_block_size_header_and_bytes():
    import xsknet_amd as X
    L = X.lib()
    size = L.xsk_gpu_responder_block_size
    assert size(0) == 0 and size(1025) == 0 and size(0xFFFFFFFF) == 0
    stride = size(2) - size(1)
    hdr = open(os.path.join(CSRC, "xsk_responder_block.h")).read()
    rq = open(os.path.join(CSRC, "xsk_rx_queues.h")).read()
    record = int(re.search(r"kRqRecordBytes = (\d+);", rq).group(1)) + 24 + 3 * 8 + 2 * 4
    assert re.search(r"static_assert\(sizeof\(ResponderArgs\) == kRsRecordBytes", open(os.path.join(CSRC, "xsk_responder.hip")).read())
    assert record == 3504 and record + 256 <= 4096 and stride >= record and stride % 64 == 0 and stride - record < 64
    assert size(1) == 64 + stride and size(1024) == 64 + 1024 * stride == X.responder_block_size(1024)
    assert f"kRsMagic = {MAGIC:#x}u" in hdr.replace("0X", "0x") and MAGIC != RQ_MAGIC
    # count and NULL rules of prepare
    q = (X.ResponderQueue * 3)(_rgood(X, 0), _rgood(X, 1), _rgood(X, 2))
    block = np.full(size(3), SENTINEL, np.uint8)
    assert L.xsk_gpu_responder_prepare(None, 3, 0, block.ctypes.data) == EINVAL
    assert L.xsk_gpu_responder_prepare(q, 3, 0, None) == EINVAL
    for n in (0, 1025, 0xFFFFFFFF):
        assert L.xsk_gpu_responder_prepare(q, n, 0, block.ctypes.data) == EINVAL
    for opts in (0x8, 0x20, 0x18):
        assert L.xsk_gpu_responder_prepare(q, 3, opts, block.ctypes.data) == EINVAL
    assert (block == SENTINEL).all()
    # the bytes
    queues = [_rgood(X, 0), _rgood(X, 1, smax=1024, nt=None, nn=0, ns=None), _rgood(X, 2, smax=1, nr=None)]
    rc, block = _prepare(X, queues, 0x17, fill=0xEE)
    rc2, again = _prepare(X, queues, 0x17, fill=0x11)
    assert rc == 0 and rc2 == 0 and (block == again).all(), "the same input gives the same bytes, padding zeroed"
    assert block.nbytes == 64 + 3 * stride
    assert _words(block, 0, 6) == [MAGIC, L.xsk_gpu_abi_version(), 3, 0x17, stride, record]
    assert not block[24:64].any()
    rq_stride = X.rx_queues_block_size(2) - X.rx_queues_block_size(1)
    rq_block = X.rx_queues_prepare([r._keep[0] for r in queues], 0x17)
    for k, r in enumerate(queues):
        at = 64 + k * stride
        rc, alone = _prepare(X, [r], 0x17)
        assert rc == 0 and (block[at:at + stride] == alone[64:64 + stride]).all(), k
        assert not block[at + record:at + stride].any()
        # the record begins with the rx-queues call's record of the same queue, byte for byte
        assert (block[at:at + 3448] == rq_block[64 + k * rq_stride:64 + k * rq_stride + 3448]).all()
        w = _words(block, at + 3448, 6)
        up = r._keep[1]
        assert (w[0] | w[1] << 32, w[2] | w[3] << 32, w[4] | (w[5] & 0xFFFFFF) << 32, 1 << (w[5] >> 24)) == \
            (up.d_producer, up.d_consumer, up.d_ring, up.size)
        tail = block[at + 3472:at + 3504]
        assert [int(x) for x in tail[:24].view("<u8")] == [r.d_ntable or 0, r.d_nstats or 0, r.d_nres or 0]
        assert [int(x) for x in tail[24:].view("<u4")] == [r.n_nentries, r.serve_max]
    rc, other = _prepare(X, queues, 0x7)
    assert rc == 0 and _words(other, 0, 4) == [MAGIC, 1, 3, 0x7] and (other[64:64 + stride] != block[64:64 + stride]).any()
    assert _words(rq_block, 0, 1) == [RQ_MAGIC] and _words(rq_block, 0, 6)[1:4] == _words(block, 0, 6)[1:4]


def test_the_launching_call_refuses_before_any_device_call():
    import xsknet_amd as X
    dev = X.lib().xsk_gpu_responder_queues_dev
    ok = 0x7F0000001000
    assert dev(None, 1, 0, None) == EINVAL
    for mis in (1, 2, 4, 8, 16, 32, 48):
        assert dev(ok + mis, 1, 0, None) == EINVAL
    for n in (0, 1025, 0xFFFFFFFF):
        assert dev(ok, n, 0, None) == EINVAL
    for opts in (0x8, 0x20, 0x18, 0xFFFFFFFF):
        assert dev(ok, 1, opts, None) == EINVAL


def _code(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def test_the_new_files_own_text():
    """Every rule stands in front of the one launch; both halves are checked by the functions their own calls check
    with; the serve stage stands behind a fence behind the loop body and reads no room of stage 2; no inline assembly."""
    src = _code("xsk_responder.hip")
    pub = src[src.index('extern "C" {'):]
    assert re.findall(r"^(?:int|size_t) (\w+)\(", pub, re.M) == [NAMES[1], NAMES[0], NAMES[2], NAMES[3]]
    for name in (NAMES[1], NAMES[3]):
        body = pub[pub.index("int " + name + "("):]
        body = body[:body.index("\n}\n")]
        assert body.count("return -EINVAL") == 1 and body.index("return -EINVAL") < body.index("_launch("), name
    prep = pub[pub.index("int " + NAMES[2] + "("):pub.index("int " + NAMES[3] + "(")]
    assert prep.index("responder_ok(") < prep.index("responders_disjoint(") < prep.index("rs_write_block<")
    for word in ("hip", "<<<"):
        assert word not in prep, "prepare is host only: no device call"
    ok = src[src.index("bool responder_ok("):]
    ok = ok[:ok.index("\n}\n")]
    assert "xsk_gpu__rxq_ok(" in ok and "xsk_gpu__serve_ok(" in ok and "ring_ok(" not in ok.replace("xsk_gpu__", "")
    assert "return queue_ok(*q, opts)" in _code("xsk_rx_queues.hip") and "return serve_ok(d_umem, stack, tx" in _code("xsk_neigh.hip")
    assert src.count("<<<") == 4 and _code("xsk_responder_ds.hip").count("<<<") == 2
    body = _code("xsk_responder_body.h")
    fn = body[body.index("void responder_body("):]
    assert fn.index("loop_fused_body<C>(A.f, L);") < fn.index("lf_stage_fence();") < fn.index("ng_serve_body(")
    assert "room" not in fn.replace("S.room", "") and "L.tx.r[k]" in fn and "L.stack" in fn and "lf_ring_dev(A.up)" in fn
    assert "static_assert(sizeof(ResponderArgs) + 256 <= 4096" in body
    serve = _code("xsk_neigh_device.h")
    fn = serve[serve.index("void ng_serve_body("):]
    assert fn.index("ng_stage_entry(") < fn.index("load_word(r.cons)") < fn.index("__syncthreads();")
    for f in ("xsk_responder.hip", "xsk_responder_ds.hip", "xsk_responder_body.h", "xsk_responder_block.h", "xsk_neigh_device.h"):
        c = _code(f)
        assert "asm" not in c and "hipMalloc" not in c and "hipMemcpy" not in c and "atomic_fetch" not in c, f
    stage = _code("xsk_responder_block.h")
    stage = stage[stage.index("bool rs_stage("):]
    assert stage.index("rs_header_ok(") < stage.index("return false;") < stage.index("S.v[k] =")
    assert "h1.x" not in stage[stage.index("return false;"):], "no word of the block is an offset"
    for f, kernels in (("xsk_responder.hip", 2), ("xsk_responder_ds.hip", 2)):
        c = _code(f)
        assert c.count("__global__") == kernels and c.count("rs_stage(block, n_queues, opts, M.S)) return;") == 1


def _statements(text):
    return re.sub(r"\s+", " ", text).strip()


def test_the_two_statements_of_the_serve_body_are_one():
    """neigh_serve_kernel keeps its own text (xsk_neigh.hip says why); ng_serve_body() states it again for the responder
    kernels.  Held together here: from the first statement to the last they are the same statements, but for where a
    ring comes from and the ng_ prefix of the three helpers."""
    k = _code("xsk_neigh.hip")
    k = k[k.index("void neigh_serve_kernel(ServeArgs A) {"):]
    k = k[k.index("const uint32_t t = threadIdx.x;"):k.index("\n}\n")]
    b = _code("xsk_neigh_device.h")
    b = b[b.index("void ng_serve_body("):]
    b = b[b.index("const uint32_t t = threadIdx.x;"):b.index("\n}\n")]
    b = b.replace("ring_at(t)", "ring_dev(A.ring[t])")
    for name in ("wave_counters", "add_counters", "desc_of"):
        b = b.replace("ng_" + name, name)
    assert _statements(k) == _statements(b)

    def helpers(c, pre):
        out = []
        for n in ("wave_counters", "add_counters", "desc_of"):
            text = c[c.index(f" {pre}{n}("):]
            out.append(_statements(text[:text.index("\n}\n")].replace(pre + n, n)))
        return out

    assert helpers(_code("xsk_neigh.hip"), "") == helpers(_code("xsk_neigh_device.h"), "ng_")


def test_the_kernel_listings_show_every_parent_kernel_unchanged():
    """profiles/responder/: the parent's listing and the new build's (tools/isa_manifest.py): every kernel of the parent
    keeps its hash, and the new build adds the six responder kernels and nothing else; the resource usage of the six
    shows no spill and no scratch."""
    d = os.path.join(ROOT, "profiles", "responder")
    rows = lambda f: dict((ln.split(" ", 2)[2], ln.split(" ", 2)[0]) for ln in open(os.path.join(d, f)).read().splitlines())  # noqa: E731
    parent, new = rows("isa_parent.txt"), rows("isa_new.txt")
    assert all(new.get(k) == v for k, v in parent.items()) and len(parent) >= 60
    added = sorted(set(new) - set(parent))
    assert len(added) == 6 and all("responder" in k for k in added)
    ru = open(os.path.join(d, "resource_usage.txt")).read()
    assert ru.count("Function Name:") == 6 and ru.count("ScratchSize [bytes/lane]: 0") == 6
    assert ru.count("SGPRs Spill: 0") == 6 and ru.count("VGPRs Spill: 0") == 6
    assert all(int(v) <= 128 for v in re.findall(r"\bVGPRs: (\d+)", ru))


def test_the_block_on_the_host_under_address_sanitizer():
    """tests/c/test_responder.cpp: blocks of 1, 2 and 1024 records written into heap arrays of exactly block_size bytes,
    every ring of every record (up included) unpacked and compared, no byte outside the block touched, the header check
    against each mismatch and against an rx-queues header.  A stand-alone program: nothing loaded into Python runs
    under a sanitizer."""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "t")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "c", "test_responder.cpp")], check=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    assert "responder ok" in res.stdout


def test_what_the_seed_set_reaches():
    """The 32 worlds of tests/responder_seeds.py through the spec alone: each condition the randomised GPU tests rest on
    holds at least once.  (Replies are rare in these worlds: the hand-written cases carry them.)"""
    seeds = SEEDS.seed_set()
    assert sorted(seeds) == sorted(LW.OPTS_ALL) and sum(len(s) for s in seeds.values()) == 32
    n = dict.fromkeys(("arp", "na", "no_comp", "complete_max_0", "stopped_for_room", "idle_rx"), 0)
    for o, ss in seeds.items():
        assert all(700000 + 1000 * o <= s < 701000 + 1000 * o for s in ss) and len(set(ss)) == 2
        for s in ss:
            w, rounds, _ = LW.run_spec(s, o, True)
            assert w.up is not None and w.in_fused_bounds()
            n["arp"] += any(r["nres"]["arp_replies"] for r in rounds)
            n["na"] += any(r["nres"]["na_replies"] for r in rounds)
            n["no_comp"] += not w.comps
            n["complete_max_0"] += bool(w.comps) and w.complete_max == 0
            n["stopped_for_room"] += sum(r["nres"]["backlog"] > 0 and r["nres"]["consumed"] < w.serve_max for r in rounds)
            n["idle_rx"] += sum(r["got"]["result"]["received"] == 0 and r["nres"]["consumed"] > 0 for r in rounds)
    print(n)
    assert all(v >= 1 for v in n.values()), n
