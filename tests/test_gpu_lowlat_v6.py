"""XSK_GPU_OPT_IPV6 through the doorbell: a LOWLAT context, a multi object and a pipe with the bit set serve batches of
<= 1024 frames from the resident dual-stack kernel (resident_ds_kernel, xsk_lowlat.hip), bit for bit the Python spec of
tests/golden/make_v6_golden.py -- every UMEM byte, verdict, record and counter -- and lowlat_served() (a counter, not a
timing) shows which path served them."""
import functools
import json
import os
import re

import numpy as np
import pytest

import oracle
from tests.conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests.test_gpu_v6 import KEYS, _dev, _host_run, _mixed, same  # noqa: E402
from tests.v6_frames import G6, spec_batch  # noqa: E402

W = G6.W
STRIDE = 2048
Q1, Q2 = [(0x8100, 0x0064)], [(0x88A8, 0x0005), (0x8100, 0x0064)]
# Four tiles of 4 frames, each with both families.  a6: aligned untagged ICMPv6 request (patched in LDS, leaves as a
# whole sector); t1: aligned behind one tag (l4 + 4 = 62); q2u: unaligned behind two tags (the ICMPv6 header past the
# 64-B window: per-lane UMEM reads and writes); odd: an odd-length message; pad: Ethernet padding (under STRICT plen is
# shorter than len - l4); ns: type 135; bad: a bad checksum; v4: IPv4 echo requests.
PATTERN = ("a6", "v4", "t1", "v4", "q2u", "v4", "odd", "pad", "v4", "ns", "bad", "a6", "v4", "q2u", "v4", "t1")
# (name, frames, frame length or None for short messages, payload bound of the short ones)
CASES = (("1", 1, None, 300), ("63", 63, None, 300), ("64", 64, None, 300), ("65", 65, None, 300),
         ("128_small", 128, None, 40), ("128x1500", 128, 1500, 0), ("1024", 1024, None, 300))
LL_WG = int(re.search(r"#define XSK_GPU__LL_WG (\d+)u",
                      open(os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_lowlat_proto.h")).read()).group(1))


def _frame(kind, i, rng, flen, pmax):
    """(frame, start offset within its 16-B line) of pattern kind `kind`; flen: the frame's length, None: short."""
    def pay(hdr, odd=False):
        n = flen - hdr if flen else int(rng.integers(0, pmax + 1))
        if odd and not flen:
            n |= 1
        return bytes(rng.integers(0, 256, n, dtype=np.uint8))
    a16 = lambda: bytes(rng.integers(0, 255, 16, dtype=np.uint8))  # noqa: E731  (never multicast)
    kw = dict(saddr=a16(), daddr=a16(), ident=int(rng.integers(0, 65536)), seq=i & 0xFFFF)
    if kind == "v4":
        return W.build(payload=pay(42), ident=kw["ident"], seq=kw["seq"]), i % 16
    if kind == "a6":
        return G6.build6(payload=pay(62), **kw), 0
    if kind == "t1":
        return G6.build6(vlan=Q1, payload=pay(66), **kw), 0
    if kind == "q2u":
        return G6.build6(vlan=Q2, payload=pay(70), **kw), 1 + i % 15
    if kind == "odd":
        return G6.build6(payload=pay(62, odd=True), **kw), i % 16
    if kind == "pad":
        return G6.build6(payload=pay(62 + 9), pad=9, **kw), i % 16
    if kind == "ns":
        return G6.build6(itype=135, payload=pay(62), **kw), i % 16
    assert kind == "bad"
    return G6.build6(bad_icmp=True, payload=pay(62), **kw), i % 16


@functools.lru_cache(maxsize=None)
def _traffic():
    """One UMEM of random bytes holding every case's frames (case k's after case k - 1's): (umem, {name: descs})."""
    rng = np.random.default_rng(0x116)
    total = sum(c[1] for c in CASES)
    umem = rng.integers(0, 256, total * STRIDE, dtype=np.uint8)
    out, base = {}, 0
    for name, n, flen, pmax in CASES:
        descs = np.zeros(n, X.DESC_DTYPE)
        for i in range(n):
            f, off = _frame(PATTERN[i % 16], i, rng, flen, pmax)
            a = (base + i) * STRIDE + off
            assert off + len(f) <= STRIDE and (flen is None or len(f) == flen)
            umem[a:a + len(f)] = np.frombuffer(f, np.uint8)
            descs[i] = (a, len(f), 0)
        out[name] = descs
        base += n
    # what the host's choice of serving workgroups looks at (xsk_gpu__ll_groups): leader alone / every workgroup
    assert int(out["128_small"]["len"].sum()) <= 16 << 10 < int(out["128x1500"]["len"].sum())
    umem.setflags(write=False)
    return umem, out


@functools.lru_cache(maxsize=None)
def _traffic_spec(opts):
    """The spec over every case under `opts`: (umem after, {name: (verdicts, records, counters)})."""
    umem, cases = _traffic()
    ref = umem.copy()
    res = {name: spec_batch(ref, descs, opts) for name, descs in cases.items()}
    ref.setflags(write=False)
    return ref, res


def _served_step(ctx, before, batches=1):
    """The doorbell path, from the counters: `batches` more completed by the resident kernel, none launched."""
    now = ctx.lowlat_served()
    assert now == (before[0] + batches, before[1]), (before, now)
    return now


@pytest.mark.parametrize("opts", [0x10, 0x12, 0x17])
def test_doorbell_parity(opts):
    """Batches of 1, 63, 64 (descriptors taken from the poll), 65 (from memory), 128 small frames (leader alone),
    128 x 1500 B (every workgroup) and 1024 frames (16 tiles per slice set) on one LOWLAT context per option word."""
    _dev()
    umem, cases = _traffic()
    ref, spec = _traffic_spec(opts)
    if opts == 0x17:  # the mix reaches the reply paths and the gates (the spec alone)
        v = spec["1024"][0]
        assert {G6.TX_REPLY, G6.DROP_NOT_ECHO, G6.DROP_BAD_CSUM} <= set(v.tolist()), np.unique(v)
    work = X.umem_copy(umem)
    with X.EchoContext(work, 0, max_batch=1024, mode=X.MODE_LOWLAT, opts=opts) as ctx:
        assert ctx.mode == X.MODE_LOWLAT
        served = ctx.lowlat_served()
        assert served == (0, 0)
        for name, descs in cases.items():
            v, r, s = ctx.process(descs)
            served = _served_step(ctx, served)
            v_ref, r_ref, s_ref = spec[name]
            bad = np.nonzero(v != v_ref)[0]
            assert len(bad) == 0, (name, bad[:5], v[bad[:5]], v_ref[bad[:5]], descs[bad[:5]])
            rb, rb_ref = r.view(np.uint8).reshape(-1, 16), r_ref.view(np.uint8).reshape(-1, 16)
            bad = np.nonzero((rb != rb_ref).any(axis=1))[0]
            assert len(bad) == 0, (name, bad[:3], r[bad[:3]], r_ref[bad[:3]], descs[bad[:3]])
            for k in KEYS:
                assert int(s[k]) == int(s_ref[k]), (name, k)
    diff = np.nonzero(work != ref)[0]
    assert len(diff) == 0, f"{len(diff)} bytes differ, first at {diff[:8]} (frames {diff[:8] // STRIDE})"


@pytest.mark.parametrize("opts", range(0x10, 0x18))
def test_golden_frames_through_the_doorbell(opts):
    """The 44 golden frames at all 16 start offsets in 64-frame steps, against the committed expected outputs."""
    _dev()
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "v6.json")))
    n = len(cases) * 16
    umem = X.umem_zeros(n * STRIDE)
    descs = np.zeros(n, X.DESC_DTYPE)
    for i in range(n):
        c = cases[i // 16]
        fr = np.frombuffer(bytes.fromhex(c["frame"]), np.uint8)
        a = i * STRIDE + (i % 16)
        umem[a:a + len(fr)] = fr
        descs[i] = (a, c["len"], 0)
    with X.EchoContext(umem, 0, max_batch=64, mode=X.MODE_LOWLAT, opts=opts) as ctx:
        v, r, _ = _host_run(ctx, descs, 64)
        assert ctx.lowlat_served() == ((n + 63) // 64, 0)
    for i in range(n):
        c = cases[i // 16]
        exp = c["results"][str(opts)]
        assert v[i] == exp["verdict"], (c["name"], c["len"], i % 16)
        assert {k: int(r[i][k]) for k in r.dtype.names} == exp["rec"], (c["name"], c["len"], i % 16)
        a, L = int(descs[i]["addr"]), int(descs[i]["len"])
        assert umem[a:a + max(L, 1)].tobytes().hex() == exp["out"], (c["name"], L, i % 16)


def test_switching_instances_on_one_context():
    """0 -> 7 -> 0x17 -> 7 -> 0x17 -> 0 with a 64-frame batch after each switch: the reference, wire and dual-stack
    instances take turns on one channel; never more than one grid's workgroups run for it, none after fini."""
    _dev()
    words = (0, 7, 0x17, 7, 0x17, 0)
    umem, descs = _mixed(3000)
    ref = umem.copy()
    want = []
    for k, opts in enumerate(words):  # batch k: frames [64 k, 64 k + 64), under words[k]
        d = descs[64 * k:64 * k + 64]
        if opts & X.OPT_IPV6:
            want.append(spec_batch(ref, d, opts))
        else:
            v_ref, r_ref, s_ref = oracle.echo_batch_opts(ref, d, opts) if opts else oracle.echo_batch(ref, d)
            want.append((v_ref, r_ref.view(X.REC_DTYPE), s_ref))
    work = X.umem_copy(umem)
    assert X.lowlat_live(0) == 0
    with X.EchoContext(work, 0, max_batch=64, mode=X.MODE_LOWLAT) as ctx:
        served = ctx.lowlat_served()
        for k, opts in enumerate(words):
            ctx.set_options(opts)
            assert X.lowlat_live(0) <= LL_WG
            d = descs[64 * k:64 * k + 64]
            v, r, s = ctx.process(d)
            assert X.lowlat_live(0) <= LL_WG, (k, hex(opts))
            served = _served_step(ctx, served)
            v_ref, r_ref, s_ref = want[k]
            assert (v == v_ref).all(), (k, hex(opts), np.nonzero(v != v_ref)[0][:5])
            assert (r.view(np.uint8) == r_ref.view(np.uint8)).all(), (k, hex(opts))
            for key in KEYS:
                assert int(s[key]) == int(s_ref[key]), (k, hex(opts), key)
    assert X.lowlat_live(0) == 0
    diff = np.nonzero(work != ref)[0]
    assert len(diff) == 0, f"{len(diff)} bytes differ, first at {diff[:8]}"


def test_bounds_through_the_doorbell():
    """A 64-B aligned request flush with the UMEM's end, a descriptor leaving the UMEM, one starting past it, and a
    30-byte 0x86DD frame 32 bytes before the end (its window clipped): TX_REPLY / BAD_DESC / BAD_DESC / DROP_SHORT."""
    _dev()
    frames = [(G6.build6(vlan=Q2, payload=b"fifteen"), 15), (G6.build6(vlan=Q1), 0), (G6.build6(), 9),
              (G6.build6(payload=b"\x11\x22"), 0)]  # the last: 64 B, aligned, ends the UMEM
    stride = 256
    rng = np.random.default_rng(8)
    size = (len(frames) - 1) * stride + 64
    umem = rng.integers(0, 256, size, dtype=np.uint8)
    d = np.zeros(len(frames) + 2, X.DESC_DTYPE)
    for i, (f, off) in enumerate(frames):
        a = i * stride + off
        umem[a:a + len(f)] = np.frombuffer(f, np.uint8)
        d[i] = (a, len(f), 0)
    assert int(d[3]["addr"]) % 64 == 0 and int(d[3]["addr"]) + int(d[3]["len"]) == size
    d[-2] = (size - 8, 62, 0)   # leaves the UMEM
    d[-1] = (size + 64, 62, 0)  # starts past it
    # the short frame: a UMEM that ends 32 bytes after its start
    umem_s = umem[:2 * stride + 32].copy()
    umem_s[-32:-2] = np.frombuffer(frames[2][0][:30], np.uint8)
    d_s = d[:3].copy()
    d_s[2] = (umem_s.size - 32, 30, 0)
    for um, dd, expect in ((umem, d, {3: G6.TX_REPLY, 4: X.DROP_BAD_DESC, 5: X.DROP_BAD_DESC}),
                           (umem_s, d_s, {2: G6.DROP_SHORT})):
        ref = um.copy()
        v_ref, r_ref, s_ref = spec_batch(ref, dd, 0x17)
        for i, verdict in expect.items():
            assert v_ref[i] == verdict, (i, v_ref)
        work = X.umem_copy(um)
        with X.EchoContext(work, 0, max_batch=64, mode=X.MODE_LOWLAT, opts=0x17) as ctx:
            v, r, s = ctx.process(dd)
            assert ctx.lowlat_served() == (1, 0)
        same((work, v, r, s), (ref, v_ref, r_ref, s_ref), dd)


def test_multi_context_shares_on_the_doorbells():
    """Two LOWLAT contexts on one device under 0x17, 1000 frames in shares of 250: every share on its doorbell."""
    _dev()
    umem, descs = _mixed(3000)
    descs = descs[:1000]
    ref = umem.copy()
    v_ref, r_ref, s_ref = spec_batch(ref, descs, 0x17)
    work = X.umem_copy(umem)
    with X.MultiContext(work, [0, 0], max_batch=500, mode=X.MODE_LOWLAT, opts=0x17) as m:
        members = [X.ContextView(m.context(g)) for g in range(2)]
        assert [c.mode for c in members] == [X.MODE_LOWLAT] * 2
        v, r, tot = _host_run(m, descs, 500)
        assert m.status() == [0, 0]
        assert [c.lowlat_served() for c in members] == [(2, 0), (2, 0)]
        assert m.lowlat_served() == (4, 0)
    same((work, v, r, tot), (ref, v_ref, r_ref, s_ref), descs)


def test_rx_pipe_on_the_doorbells():
    """A depth-2 LOWLAT pipe under 0x17 over 4 x 64 frames: replies on the TX ring and frames handed back, byte for
    byte the spec's (as tests/test_gpu_v6.py::test_v6_rx_pipe), every batch served by a doorbell."""
    import ctypes as C
    from tests.test_gpu_rxloop import FRAME_SIZE, HEADROOM, NUM_FRAMES, RING, KRing
    _dev()
    umem = X.umem_zeros(NUM_FRAMES * FRAME_SIZE)
    rx, fq = KRing(X.DESC_DTYPE, False), KRing(np.uint64, True)
    tx, cq = KRing(X.DESC_DTYPE, True), KRing(np.uint64, False)
    stack = np.zeros(NUM_FRAMES, np.uint64)
    fq.slots[:] = np.arange(RING, dtype=np.uint64) * FRAME_SIZE
    fq.ctr[0] = RING
    fq.view.cached_prod = RING
    stack[:NUM_FRAMES - RING] = np.arange(RING, NUM_FRAMES, dtype=np.uint64) * FRAME_SIZE
    pool = X.FramePool(stack.ctypes.data, NUM_FRAMES - RING, NUM_FRAMES)
    src_umem, src_descs = _mixed(3000)
    totals = np.zeros(1, X.STATS_DTYPE)
    want = {k: 0 for k in KEYS}
    expect, replies = {}, 0

    def collect():
        nonlocal replies
        txd = tx.k_pop(tx.k_avail())
        for t in txd:
            a = int(t["addr"])
            exp, verdict = expect.pop(a)
            assert verdict == G6.TX_REPLY and bytes(umem[a:a + len(exp)]) == bytes(exp), a
            replies += 1
        cq.k_push(np.array([int(t["addr"]) for t in txd], np.uint64))
        X.lib().xsk_gpu_tx_complete(C.byref(cq.view), C.byref(pool), RING)

    with X.RxPipe(umem, 0, depth=2, mode=X.MODE_LOWLAT, opts=0x17) as p:
        assert all(p.context(i).mode == X.MODE_LOWLAT for i in range(p.depth))
        for b in range(4):
            batch = []
            for j, addr in enumerate(fq.k_pop(64)):
                a = (int(addr) & ~(FRAME_SIZE - 1)) + HEADROOM
                sa, L = int(src_descs[b * 64 + j]["addr"]), int(src_descs[b * 64 + j]["len"])
                umem[a:a + 1600] = src_umem[sa:sa + 1600]
                ref = umem[a:a + 1600].copy()
                d1 = np.zeros(1, X.DESC_DTYPE)
                d1[0] = (0, L, 0)
                v, _, st = spec_batch(ref, d1, 0x17)
                for k in KEYS:
                    want[k] += st[k]
                expect[a] = (ref[:max(L, 64)], int(v[0]))
                batch.append((a, L, 0))
            rx.k_push(np.array(batch, X.DESC_DTYPE))
            got, res = p.step(rx.view, fq.view, tx.view, pool, 64, totals)
            assert res.tx_full == 0 and p.inflight <= 2
            collect()
        p.flush(tx.view, pool, totals)
        assert p.inflight == 0
        collect()
        assert p.lowlat_served() == (4, 0)
    for a, (exp, verdict) in expect.items():  # what was not sent was not a reply, and is untouched
        assert verdict != G6.TX_REPLY and bytes(umem[a:a + len(exp)]) == bytes(exp), a
    assert replies == want["tx_packets"] and replies >= 64
    for k in KEYS:
        assert int(totals[0][k]) == want[k], k
