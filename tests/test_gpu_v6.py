"""GPU parity of the ICMPv6 echo widening (XSK_GPU_OPT_IPV6: the dual-stack kernel of xsk_echo_ds.hip) against the
Python spec of tests/golden/make_v6_golden.py: verdicts, records, counters and every byte of the UMEM, bit for bit.
The C oracle does not know the option bit; it checks only the IPv4 equivalence test."""
import functools
import json
import os

import numpy as np
import pytest

import oracle
from tests.conftest import ROOT

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests.v6_frames import G6, mixed_batch6, spec_batch  # noqa: E402
from tests.wire_frames import mixed_batch  # noqa: E402

KEYS = ("rx_packets", "rx_bytes", "tx_packets", "tx_bytes")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def gpu_v6(umem, descs, opts, grid=0):
    dev = _dev()
    n = len(descs)
    to_dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_umem = to_dev(umem)
    d_descs = to_dev(np.ascontiguousarray(descs, X.DESC_DTYPE))
    d_verd = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device=dev)
    d_recs = torch.full((max(n, 1) * 16,), 0xEE, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    ws = torch.zeros(max(X.workspace_size(0, n), 16), dtype=torch.uint8, device=dev)
    X.echo_dev(d_umem, d_descs, n, d_verd, d_recs, d_stats, ws, opts=opts, grid=grid)
    torch.cuda.synchronize()
    return (d_umem.cpu().numpy(), d_verd.cpu().numpy()[:n], d_recs.cpu().numpy()[:n * 16].view(X.REC_DTYPE),
            d_stats.cpu().numpy().view(X.STATS_DTYPE)[0])


def same(got, ref, descs):
    """(umem, verdicts, records, counters) of a run against the spec's."""
    out, v, r, s = got
    ref_umem, v_ref, r_ref, s_ref = ref
    bad = np.nonzero(v != v_ref)[0]
    assert len(bad) == 0, (bad[:5], v[bad[:5]], v_ref[bad[:5]], descs[bad[:5]])
    rb, rb_ref = r.view(np.uint8).reshape(-1, 16), r_ref.view(np.uint8).reshape(-1, 16)
    bad = np.nonzero((rb != rb_ref).any(axis=1))[0]
    assert len(bad) == 0, (bad[:3], r[bad[:3]], r_ref[bad[:3]], descs[bad[:3]])
    for k in KEYS:
        assert int(s[k]) == int(s_ref[k]), k
    diff = np.nonzero(out != ref_umem)[0]
    assert len(diff) == 0, f"{len(diff)} bytes differ, first at {diff[:8]}"


def check(umem, descs, opts, grid=0):
    ref = umem.copy()
    v_ref, r_ref, s_ref = spec_batch(ref, descs, opts)
    same(gpu_v6(umem, descs, opts, grid), (ref, v_ref, r_ref, s_ref), descs)
    return v_ref


@functools.lru_cache(maxsize=None)
def _mixed(n, seed=0):
    umem, descs = mixed_batch6(n, 2048, seed=6000 + n + seed, offsets=True)
    umem.setflags(write=False)
    return umem, descs


@pytest.mark.parametrize("opts", range(0x10, 0x18))
def test_v6_golden_all_offsets(opts):
    """Every golden frame at all 16 start offsets, against the committed expected outputs and the live spec."""
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "v6.json")))
    stride = 2048
    n = len(cases) * 16
    umem = np.zeros(n * stride, np.uint8)
    descs = np.zeros(n, X.DESC_DTYPE)
    for i in range(n):
        c = cases[i // 16]
        fr = np.frombuffer(bytes.fromhex(c["frame"]), np.uint8)
        a = i * stride + (i % 16)
        umem[a:a + len(fr)] = fr
        descs[i] = (a, c["len"], 0)
    out, v, r, s = gpu_v6(umem, descs, opts)
    for i in range(n):
        c = cases[i // 16]
        exp = c["results"][str(opts)]
        assert v[i] == exp["verdict"], (c["name"], c["len"], i % 16)
        assert {k: int(r[i][k]) for k in r.dtype.names} == exp["rec"], (c["name"], c["len"], i % 16)
        a, L = int(descs[i]["addr"]), int(descs[i]["len"])
        assert out[a:a + max(L, 1)].tobytes().hex() == exp["out"], (c["name"], L, i % 16)
    check(umem, descs, opts)


@pytest.mark.parametrize("opts", [0x10, 0x12, 0x15, 0x17])
@pytest.mark.parametrize("n", [1, 64, 65, 3000])
def test_v6_mixed_batches(opts, n):
    umem, descs = _mixed(n)
    if n == 3000 and opts == 0x17:  # the mix really exercises the gates (the spec alone, before the GPU is asked)
        v = spec_batch(umem.copy(), descs, opts)[0]
        assert len(np.unique(v)) >= 6, np.unique(v)
    check(umem.copy(), descs, opts)


@pytest.mark.parametrize("n,grid", [(3000, 1), (3000, 2), (5000, 1)])
def test_v6_multi_round_and_multi_tile_shares(n, grid):
    """Shares of several tiles and rounds per workgroup through grid= (n = 5000, grid 1: 79 tiles, 3 rounds)."""
    umem, descs = _mixed(n, seed=grid)
    check(umem.copy(), descs, 0x17, grid=grid)


def test_v6_paired_short_tiles():
    """5000 aligned 62-byte echoes at a 64-B stride in one workgroup: both tiles of a wave's round read together
    (read_round_short2), every frame's own addresses, identifier and checksum."""
    rng = np.random.default_rng(62)
    n = 5000
    umem = rng.integers(0, 256, n * 64, dtype=np.uint8)
    descs = np.zeros(n, X.DESC_DTYPE)
    for i in range(n):
        f = G6.build6(saddr=bytes(rng.integers(0, 255, 16, dtype=np.uint8)), daddr=bytes(rng.integers(0, 255, 16, dtype=np.uint8)),
                      ident=int(rng.integers(0, 65536)), seq=i & 0xFFFF, bad_icmp=i % 97 == 0)
        assert len(f) == 62
        umem[i * 64:i * 64 + 62] = np.frombuffer(f, np.uint8)
        descs[i] = (i * 64, 62, 0)
    v = check(umem, descs, 0x17, grid=1)
    assert (v == G6.TX_REPLY).sum() == n - len(range(0, n, 97)) and (v == G6.DROP_BAD_CSUM).sum() == len(range(0, n, 97))


def test_v6_window_edges():
    """Aligned replies at a 1536-B stride (whole-sector stores), a two-tag aligned echo (l4 + 4 = 66: byte-exact), two
    tags at off = 15 (the ICMPv6 header past the window), the last frame flush with the UMEM end, a short frame whose
    window the UMEM end clips, descriptors leaving the UMEM."""
    umem, descs = mixed_batch6(1000, 1536, seed=77, offsets=False, max_payload=1300)
    check(umem, descs, 0x17)
    q2 = [(0x88A8, 5), (0x8100, 100)]
    frames = [(G6.build6(vlan=q2, payload=b"two tags"), 0), (G6.build6(vlan=q2, payload=b"fifteen"), 15),
              (G6.build6(vlan=q2[:1]), 0), (G6.build6(vlan=q2[:1], payload=b"x"), 3), (G6.build6(), 9),
              (G6.build6(payload=b"\x11\x22"), 0)]  # the last: 64 B, aligned, ends the UMEM
    stride = 256
    rng = np.random.default_rng(8)
    size = (len(frames) - 1) * stride + 64
    umem2 = rng.integers(0, 256, size, dtype=np.uint8)
    d2 = np.zeros(len(frames) + 3, X.DESC_DTYPE)
    for i, (f, off) in enumerate(frames):
        a = i * stride + off
        umem2[a:a + len(f)] = np.frombuffer(f, np.uint8)
        d2[i] = (a, len(f), 0)
    d2[-3] = (size - 8, 62, 0)    # leaves the UMEM
    d2[-2] = (size + 64, 62, 0)   # starts past it
    d2[-1] = (3 * stride + 128, 20, 0)  # garbage, DROP_SHORT or DROP_NOT_IPV4 (its own bytes, no frame's)
    for opts in (0x10, 0x17):
        v = check(umem2.copy(), d2, opts)
        assert v[-3] == X.DROP_BAD_DESC and v[-2] == X.DROP_BAD_DESC
        assert (v[:6] == G6.TX_REPLY).all() if opts == 0x17 else (v[:4] == G6.DROP_NOT_IPV4).all(), v
    # a short 0x86DD frame 32 bytes before the UMEM end: the window is clipped
    umem3 = umem2[:5 * stride + 32].copy()
    umem3[-32:-2] = np.frombuffer(frames[4][0][:30], np.uint8)
    d3 = d2[:6].copy()
    d3[5] = (umem3.size - 32, 30, 0)
    v = check(umem3, d3, 0x17)
    assert v[5] == G6.DROP_SHORT


def test_v6_ipv4_traffic_equals_the_oracle():
    """IPv4-only traffic under 0x17 is wire mode's under 7: a wire-mode batch with every frame that would parse as
    IPv6 emptied (len 0) against the C oracle."""
    umem, descs = mixed_batch(3000, 2048, seed=4242, offsets=True)
    for i in range(len(descs)):
        a, L = int(descs[i]["addr"]), int(descs[i]["len"])
        if G6.v6_l3(umem[a:a + max(L, 14)].tobytes(), L, 0x17) is not None:
            descs[i]["len"] = 0
    ref = umem.copy()
    v_ref, r_ref, s_ref = oracle.echo_batch_opts(ref, descs, 7)
    same(gpu_v6(umem, descs, 0x17), (ref, v_ref, r_ref.view(X.REC_DTYPE), s_ref), descs)
    assert len(np.unique(v_ref)) >= 6


def _host_run(ctx, descs, step):
    vs, rs, tot = [], [], {k: 0 for k in KEYS}
    for i in range(0, len(descs), step):
        v, r, s = ctx.process(descs[i:i + step])
        vs.append(v)
        rs.append(r)
        for k in KEYS:
            tot[k] += int(s[k])
    return np.concatenate(vs), np.concatenate(rs), tot


@pytest.mark.parametrize("mode,step", [(X.MODE_ZEROCOPY, 1024), (X.MODE_STAGED, 1024), (X.MODE_LOWLAT, 1024),
                                       (X.MODE_LOWLAT, 64)])
def test_v6_host_umem_modes(mode, step):
    """A LOWLAT context with the IPv6 bit serves every batch, 64-frame ones too, through the launch path (the resident
    kernel has no IPv6 instance) and still reports the mode it runs in."""
    _dev()
    umem, descs = _mixed(3000)
    ref = umem.copy()
    v_ref, r_ref, s_ref = spec_batch(ref, descs, 0x17)
    work = X.umem_copy(umem)
    with X.EchoContext(work, 0, max_batch=1024, mode=mode) as ctx:
        m0 = ctx.mode
        ctx.set_options(0x17)
        v, r, tot = _host_run(ctx, descs, step)
        assert ctx.mode == m0 and m0 == mode
    same((work, v, r, tot), (ref, v_ref, r_ref, s_ref), descs)


def test_v6_multi_context():
    """Two LOWLAT contexts on one device, shares of 250 frames: with the IPv6 bit every share is launched."""
    _dev()
    umem, descs = _mixed(3000)
    descs = descs[:1000]
    ref = umem.copy()
    v_ref, r_ref, s_ref = spec_batch(ref, descs, 0x17)
    work = X.umem_copy(umem)
    with X.MultiContext(work, [0, 0], max_batch=500, mode=X.MODE_LOWLAT, opts=0x17) as m:
        v, r, tot = _host_run(m, descs, 500)
        assert m.status() == [0, 0]
    same((work, v, r, tot), (ref, v_ref, r_ref, s_ref), descs)


def test_v6_rx_pipe():
    """A depth-2 pipe over 256 frames in 64-frame steps: replies on the TX ring and frames handed back, in RX order,
    byte for byte the spec's."""
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
            a, L = int(t["addr"]), int(t["len"])
            exp, verdict = expect.pop(a)
            assert verdict == G6.TX_REPLY and bytes(umem[a:a + len(exp)]) == bytes(exp), a
            replies += 1
        cq.k_push(np.array([int(t["addr"]) for t in txd], np.uint64))
        X.lib().xsk_gpu_tx_complete(C.byref(cq.view), C.byref(pool), RING)

    with X.RxPipe(umem, 0, depth=2, mode=X.MODE_LOWLAT, opts=0x17) as p:
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
    for a, (exp, verdict) in expect.items():  # what was not sent was not a reply, and is untouched
        assert verdict != G6.TX_REPLY and bytes(umem[a:a + len(exp)]) == bytes(exp), a
    assert replies == want["tx_packets"] and replies >= 64
    for k in KEYS:
        assert int(totals[0][k]) == want[k], k


def test_v6_option_validation():
    dev = _dev()
    d = torch.zeros(4096, dtype=torch.uint8, device=dev)
    work = X.umem_zeros(1 << 16)
    with X.EchoContext(work, 0, max_batch=64) as ctx, X.MultiContext(work, [0, 0], max_batch=64) as m, \
            X.RxPipe(work, 0, depth=2, mode=X.MODE_ZEROCOPY) as p:
        for bad in (0x8, 0x18, 0x20):
            with pytest.raises(X.XskGpuError):
                X.echo_dev(d, d, 1, opts=bad)
            with pytest.raises(X.XskGpuError):
                ctx.set_options(bad)
            with pytest.raises(X.XskGpuError):
                X._check("xsk_gpu_multi_set_options", X.lib().xsk_gpu_multi_set_options(m._ctx, bad))
            with pytest.raises(X.XskGpuError):
                p.set_options(bad)
        for good in (0x10, 0x17, 0):
            ctx.set_options(good)
            X._check("xsk_gpu_multi_set_options", X.lib().xsk_gpu_multi_set_options(m._ctx, good))
            p.set_options(good)
