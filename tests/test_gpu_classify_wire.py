"""GPU parity of xsk_gpu_classify_dev_opts (classify_wire_kernel of xsk_classify.hip, then the shared scan and scatter)
against the Python spec of tests/golden/make_classify_wire_golden.py: every action, the count and the in-order
REDIRECT list; and the filter -> transform pipeline against tests/v6_frames.spec_batch over the whole batch."""
import functools

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import classify_wire as CW  # noqa: E402
from tests.v6_frames import G6, mixed_batch6, spec_batch  # noqa: E402

D, P, R = X.XDP_DROP, X.XDP_PASS, X.XDP_REDIRECT
KEYS = ("rx_packets", "rx_bytes", "tx_packets", "tx_bytes")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def to_dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(_dev())


def gpu_classify(umem, descs, opts, bound=True, want_out=True):
    """(actions, redirected descriptors or None) of classify_dev(opts=...) on copies of the host arrays; canaries
    behind the action and descriptor arrays must survive."""
    dev = _dev()
    n = len(descs)
    d_umem = umem if isinstance(umem, torch.Tensor) else to_dev(umem)
    d_descs = to_dev(np.ascontiguousarray(descs, X.DESC_DTYPE))
    act = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device=dev)
    out = torch.full(((n + 4) * 16,), 0xEE, dtype=torch.uint8, device=dev) if want_out else None
    nout = torch.full((1,), -1, dtype=torch.int64, device=dev) if want_out else None
    X.classify_dev(d_umem, d_descs, n, bound, act, out, nout, opts=opts)
    torch.cuda.synchronize()
    a = act.cpu().numpy()
    assert (a[n:] == 0xEE).all()
    if not want_out:
        return a[:n], None
    k = int(nout.cpu().numpy().view(np.uint32)[0])
    assert int(nout.cpu().numpy().view(np.uint32)[1]) == 0xFFFFFFFF  # d_nout is one uint32
    assert k <= n
    o = out.cpu().numpy()
    assert (o[k * 16:] == 0xEE).all()
    return a[:n], o[:k * 16].view(X.DESC_DTYPE)


def same(got, ref, descs):
    a, r = got
    a_ref, r_ref = ref
    bad = np.nonzero(a != a_ref)[0]
    assert len(bad) == 0, (len(bad), bad[:5], a[bad[:5]], a_ref[bad[:5]], descs[bad[:5]])
    if r is not None:
        assert len(r) == len(r_ref), (len(r), len(r_ref))
        assert (r.view(CW.G_DESC) == r_ref).all()


@pytest.mark.parametrize("bound", [True, False])
@pytest.mark.parametrize("opts", CW.GC.OPTION_WORDS)
def test_golden_all_offsets(opts, bound):
    """Every crafted frame at all 16 start offsets, garbage around it, against the committed actions and the spec."""
    cases = CW.golden()
    stride = 256
    n = len(cases) * 16
    umem = np.random.default_rng(opts).integers(0, 256, n * stride, dtype=np.uint8)
    descs = np.zeros(n, CW.G_DESC)
    for i in range(n):
        c = cases[i // 16]
        fr = np.frombuffer(bytes.fromhex(c["frame"]), np.uint8)
        a = i * stride + (i % 16)
        umem[a:a + len(fr)] = fr
        descs[i] = (a, c["len"], 0)
    a, r = gpu_classify(umem, descs, opts, bound)
    key = "bound" if bound else "unbound"
    for i in range(n):
        c = cases[i // 16]
        assert a[i] == c["results"][str(opts)][key], (c["name"], i % 16)
    same((a, r), CW.spec_classify_batch(umem, descs, opts, bound), descs)


@functools.lru_cache(maxsize=None)
def _mixed(n):
    umem, descs = mixed_batch6(n, 2048, seed=9100 + n, offsets=True)
    umem.setflags(write=False)
    return umem, descs


@pytest.mark.parametrize("opts", [0x2, 0x10, 0x12, 0x17])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_mixed_batches(n, opts):
    """Random dual-stack traffic at offsets i % 16 around the wave (64) and workgroup (256) sizes: actions, nout and
    the in-order list; actions alone without d_out; and nothing redirected without a bound socket."""
    umem, descs = _mixed(n)
    ref = CW.spec_classify_batch(umem, descs, opts, True)
    d_umem = to_dev(umem)
    same(gpu_classify(d_umem, descs, opts, True), ref, descs)
    same(gpu_classify(d_umem, descs, opts, True, want_out=False), ref, descs)
    ref0 = CW.spec_classify_batch(umem, descs, opts, False)
    assert len(ref0[1]) == 0
    got0 = gpu_classify(d_umem, descs, opts, False)
    assert len(got0[1]) == 0
    same(got0, ref0, descs)


def test_more_workgroups_than_scan_threads():
    """262 147 frames = 1025 workgroups: the smallest batch at which a thread of the scan owns more than one count.
    A 4099-frame base batch tiled at stride 256.  Payloads up to 108 B: the longest frame the source draws (three tags,
    IHL 15, 39 B of padding, offset 15) then ends exactly at its 256-B stride -- with 150 B the generator's own
    assertion fails."""
    nb, n, stride, opts = 4099, 262147, 256, 0x17
    umem, descs = mixed_batch6(nb, stride, seed=4099, offsets=True, max_payload=108)
    act, _ = CW.spec_classify_batch(umem, descs, opts, True)
    assert len(set(act)) == 3
    big, d, a_ref = CW.tile_batch(umem, descs, act, n, stride)
    assert len(d) == n and (n + 255) // 256 == 1025
    same(gpu_classify(big, d, opts, True), (a_ref, d[a_ref == R]), d)


def test_descriptor_edges():
    """Rule 1 and the frames that end flush with the UMEM, under every option bit."""
    opts = 0x17
    size = 4096
    umem = np.random.default_rng(17).integers(0, 256, size, dtype=np.uint8)
    echo6 = np.frombuffer(G6.build6(), np.uint8)
    echo4 = np.frombuffer(G6.W.build(payload=b""), np.uint8)[:34]
    assert len(echo6) == 62 and len(echo4) == 34
    umem[0:62] = echo6                       # a frame at address 0
    umem[size - 62:] = echo6                 # the minimal ICMPv6 echo request flush with the end
    umem[1024:1024 + 62] = echo6
    umem[2048 - 34:2048] = echo4
    descs = np.zeros(10, CW.G_DESC)
    descs[0] = (0, 62, 0)
    descs[1] = (size - 62, 62, 0)
    descs[2] = (size - 62, 63, 0)            # crosses the end by one byte
    descs[3] = (size + 1, 14, 0)             # addr > umem_size
    descs[4] = (1024, (1 << 30) + 1, 0)      # len > XSK_GPU_MAX_LEN
    descs[5] = (size - 13, 13, 0)            # 13 bytes in the last 13 bytes
    descs[6] = (size, 0, 0)                  # empty, at the very end
    descs[7] = (1024, 62, 0)
    descs[8] = (size - 61, 61, 0)            # last 61 bytes: whatever they hold, the spec decides
    descs[9] = (1 << 40, 62, 0)
    want = [R, R, D, D, D, D, D, R]
    ref = CW.spec_classify_batch(umem, descs, opts, True)
    assert list(ref[0][:8]) == want and ref[0][9] == D
    same(gpu_classify(umem, descs, opts, True), ref, descs)
    # a 34-byte IPv4 ICMP frame flush with the end of a UMEM of its own
    um2 = umem[:2048].copy()
    d2 = np.zeros(2, CW.G_DESC)
    d2[0] = (2048 - 34, 34, 0)
    d2[1] = (2048 - 33, 33, 0)               # the last 33 bytes: not that frame any more, the spec decides
    ref2 = CW.spec_classify_batch(um2, d2, opts, True)
    assert ref2[0][0] == R
    same(gpu_classify(um2, d2, opts, True), ref2, d2)


def test_opts_zero_is_the_reference_filter():
    """opts == 0 through the new entry point: xsk_gpu_classify_dev and the oracle, on mixed synthetic traffic."""
    dev = _dev()
    n, stride = 5000, 256
    umem = np.zeros(n * stride, np.uint8)
    descs = oracle.synth_batch(umem, n, 0, stride, seed=0x5EED0C1B, mode=1, len_lo=0, len_hi=200)
    a_ref, r_ref = oracle.xdp_classify_batch(umem, descs, True)
    a_old, r_old = gpu_classify(umem, descs, 0, True)  # classify_dev(opts=0): xsk_gpu_classify_dev
    d_umem, d_descs = to_dev(umem), to_dev(descs)
    act = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    nout = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(int(X.lib().xsk_gpu_classify_workspace_size(n)), dtype=torch.uint8, device=dev)
    rc = X.lib().xsk_gpu_classify_dev_opts(d_umem.data_ptr(), umem.nbytes, d_descs.data_ptr(), n, 0, 1, act.data_ptr(),
                                           out.data_ptr(), nout.data_ptr(), ws.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    k = int(nout.cpu().numpy().view(np.uint32)[0])
    a_new, r_new = act.cpu().numpy(), out.cpu().numpy()[:k * 16].view(X.DESC_DTYPE)
    assert (a_new == a_ref).all() and (a_old == a_ref).all()
    assert k == len(r_ref) and (r_new == r_ref.view(X.DESC_DTYPE)).all() and (r_old == r_ref.view(X.DESC_DTYPE)).all()


@functools.lru_cache(maxsize=None)
def _pipeline_batch():
    umem, descs = mixed_batch6(4096, 2048, seed=9017, offsets=True)
    umem.setflags(write=False)
    return umem, descs


@pytest.mark.parametrize("opts", [0x17, 0x13])
def test_filter_then_transform_pipeline(opts):
    """classify_dev(opts) -> echo_dev(opts) on the redirected list computes what the transform alone computes over the
    whole batch: the same UMEM bytes and tx counters (every frame the transform answers was redirected), rx_packets ==
    nout, and the spec's verdicts at the redirected positions."""
    dev = _dev()
    umem, descs = _pipeline_batch()
    n = len(descs)
    ref = umem.copy()
    v_ref, _, s_ref = spec_batch(ref, descs, opts)
    a_ref, r_ref = CW.spec_classify_batch(umem, descs, opts, True)
    d_umem, d_descs = to_dev(umem), to_dev(np.ascontiguousarray(descs, X.DESC_DTYPE))
    act = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    red = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    nred = torch.zeros(1, dtype=torch.int64, device=dev)
    X.classify_dev(d_umem, d_descs, n, True, act, red, nred, opts=opts)
    torch.cuda.synchronize()
    k = int(nred.cpu().numpy().view(np.uint32)[0])
    a = act.cpu().numpy()
    assert (a == a_ref).all() and k == len(r_ref) and 0 < k < n
    verd = torch.full((k,), 0xEE, dtype=torch.uint8, device=dev)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    ws = torch.zeros(max(X.workspace_size(0, k), 16), dtype=torch.uint8, device=dev)
    X.echo_dev(d_umem, red, k, verd, None, stats, ws, opts=opts)
    torch.cuda.synchronize()
    out = d_umem.cpu().numpy()
    diff = np.nonzero(out != ref)[0]
    assert len(diff) == 0, f"{len(diff)} bytes differ, first at {diff[:8]}"
    st = stats.cpu().numpy().view(X.STATS_DTYPE)[0]
    assert int(st["tx_packets"]) == s_ref["tx_packets"] > 0 and int(st["tx_bytes"]) == s_ref["tx_bytes"]
    assert int(st["rx_packets"]) == k
    assert int(st["rx_bytes"]) == int(descs["len"][a_ref == R].sum())
    assert (verd.cpu().numpy() == v_ref[a_ref == R]).all()
