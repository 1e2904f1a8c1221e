"""GPU parity of xsk_gpu_steer_dev (xsk_steer.hip) against the Python spec of tests/steer_spec.py and the committed
vectors of tests/golden/steer.json: every action and port, the offsets and the grouped list, with canaries behind every
output array."""
import functools

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import classify_wire as CW  # noqa: E402
from tests import steer_spec as SS  # noqa: E402
from tests.test_gpu_classify_wire import _dev, _mixed, gpu_classify, to_dev  # noqa: E402
from tests.v6_frames import G6  # noqa: E402

GS = SS.GS
D, P, R = X.XDP_DROP, X.XDP_PASS, X.XDP_REDIRECT
CANARY = 0xEE


def dev_table(table: dict):
    """(device tensor or None, n_entries) of a table dict, prepared by the library."""
    if not table:
        return None, 0
    e = X.steer_table_prepare(SS.entries_of(table))
    return to_dev(e), len(e)


def dev_bound(mask):
    if mask is None:
        return None
    return torch.from_numpy(np.array([mask], np.uint64).view(np.int64)).to(_dev())


def gpu_steer(umem, descs, opts, table, default_port, n_ports, bound=None, want_out=True):
    """dict(actions, ports, out, off) of steer_dev on copies of the host arrays (`umem` may be a device tensor, `table`
    a dict or a (tensor, n_entries) pair); the canaries behind all four output arrays must survive."""
    dev = _dev()
    n = len(descs)
    d_umem = umem if isinstance(umem, torch.Tensor) else to_dev(umem)
    d_descs = to_dev(np.ascontiguousarray(descs, X.DESC_DTYPE))
    d_table, n_entries = table if isinstance(table, tuple) else dev_table(table)
    act = torch.full((n + 64,), CANARY, dtype=torch.uint8, device=dev)
    ports = torch.full((n + 64,), CANARY, dtype=torch.uint8, device=dev)
    out = torch.full(((n + 4) * 16,), CANARY, dtype=torch.uint8, device=dev) if want_out else None
    off = torch.full((n_ports + 1 + 4,), -1, dtype=torch.int32, device=dev) if want_out else None
    X.steer_dev(d_umem, d_descs, n, d_table, n_entries, default_port, n_ports, dev_bound(bound), act, ports, out, off,
                opts=opts)
    torch.cuda.synchronize()
    a, p = act.cpu().numpy(), ports.cpu().numpy()
    assert (a[n:] == CANARY).all() and (p[n:] == CANARY).all()
    res = dict(actions=a[:n], ports=p[:n], out=None, off=None)
    if want_out:
        o32 = off.cpu().numpy().view(np.uint32)
        assert (o32[n_ports + 1:] == 0xFFFFFFFF).all()
        total = int(o32[n_ports])
        assert total <= n
        o = out.cpu().numpy()
        assert (o[total * 16:] == CANARY).all()
        res.update(out=o[:total * 16].view(X.DESC_DTYPE), off=o32[:n_ports + 1])
    return res


def same(got, ref, descs):
    for k in ("actions", "ports"):
        bad = np.nonzero(got[k] != ref[k])[0]
        assert len(bad) == 0, (k, len(bad), bad[:5], got[k][bad[:5]], ref[k][bad[:5]], descs[bad[:5]])
    if got["off"] is not None:
        assert list(got["off"]) == list(ref["off"])
        assert len(got["out"]) == len(ref["out"])
        assert (got["out"] == np.ascontiguousarray(ref["out"]).view(X.DESC_DTYPE)).all()


# ---- the committed vectors ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("opts", GS.OPTION_WORDS)
def test_golden_all_offsets(opts):
    """Every crafted frame at all 16 start offsets, garbage around it, under the eight maps of steer.json: against the
    committed (action, port) pairs and against the spec over the batch."""
    cases = SS.golden()["frames"]
    stride = 256
    n = len(cases) * 16
    umem = np.random.default_rng(opts + 1).integers(0, 256, n * stride, dtype=np.uint8)
    descs = np.zeros(n, CW.G_DESC)
    for i in range(n):
        c = cases[i // 16]
        fr = np.frombuffer(bytes.fromhex(c["frame"]), np.uint8)
        a = i * stride + (i % 16)
        umem[a:a + len(fr)] = fr
        descs[i] = (a, c["len"], 0)
    d_umem = to_dev(umem)
    for k, (table, default_port, n_ports, bound) in enumerate(SS.golden_maps()):
        got = gpu_steer(d_umem, descs, opts, table, default_port, n_ports, bound)
        want = np.array([c["results"][str(opts)][k] for c in cases], np.uint8).repeat(16, axis=0)
        bad = np.nonzero((got["actions"] != want[:, 0]) | (got["ports"] != want[:, 1]))[0]
        assert len(bad) == 0, (k, [(cases[i // 16]["name"], i % 16, got["actions"][i], got["ports"][i]) for i in bad[:5]])
        same(got, SS.spec_steer_batch(umem, descs, opts, table, default_port, n_ports, bound), descs)


# ---- the degenerate map is the filter ----------------------------------------------------------------------------

@pytest.mark.parametrize("bound", [True, False])
@pytest.mark.parametrize("opts", GS.OPTION_WORDS)
def test_degenerate_map_is_classify_dev(opts, bound):
    """n_entries == 0, default_port == 0, n_ports == 1, *d_bound == target_bound: actions and d_out of
    classify_dev(opts=...) on the same device memory, d_off[1] == *d_nout; opts == 0 on the reference's traffic too."""
    batches = [_mixed(1025)]
    if opts == 0:
        um0 = np.zeros(5000 * 256, np.uint8)
        batches.append((um0, oracle.synth_batch(um0, 5000, 0, 256, seed=0x5EED0C1B, mode=1, len_lo=0, len_hi=200)))
    for umem, descs in batches:
        d_umem = to_dev(umem)
        a_ref, r_ref = gpu_classify(d_umem, descs, opts, bound)
        got = gpu_steer(d_umem, descs, opts, None, 0, 1, int(bound))
        assert (got["actions"] == a_ref).all()
        assert list(got["off"]) == [0, len(r_ref)] and (got["out"] == r_ref).all()
        assert (got["ports"][a_ref == R] == 0).all() and (got["ports"][a_ref != R] == X.STEER_PASS).all()
        assert bound == bool((a_ref == R).any())
        if bound:  # d_bound == NULL binds every port
            got = gpu_steer(d_umem, descs, opts, None, 0, 1, None)
            assert (got["actions"] == a_ref).all() and (got["out"] == r_ref).all()


# ---- mixed batches -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _destinations(n, opts):
    umem, descs = _mixed(n)
    return SS.destinations(umem, descs, opts)


@pytest.mark.parametrize("opts", [0, 0x12, 0x17])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_mixed_batches(n, opts):
    """Random dual-stack traffic at offsets i % 16 around the wave (64) and workgroup (256) sizes, under 1, 2, 3 and 64
    ports and tables of 0, 1, 7 and 1024 entries drawn from the batch's own destinations (padded with addresses that
    do not occur): actions, ports, offsets and the grouped list; actions and ports alone without d_out."""
    umem, descs = _mixed(n)
    d_umem = to_dev(umem)
    keys = _destinations(n, opts)
    k = 0
    for n_ports in (1, 2, 3, 64):
        for n_entries in (0, 1, 7, 1024):
            k += 1
            table = SS.sample_table(keys, n_entries, n_ports, seed=100 * n + k)
            assert len(table) == n_entries
            default_port = (SS.PASS, 0, n_ports - 1)[k % 3]
            bound = (None, SS.ALL_BOUND, 0xAAAAAAAAAAAAAAAB)[k % 3 if n_ports > 1 else 0]
            ref = SS.spec_steer_batch(umem, descs, opts, table, default_port, n_ports,
                                      SS.ALL_BOUND if bound is None else bound)
            d_table = dev_table(table)
            same(gpu_steer(d_umem, descs, opts, d_table, default_port, n_ports, bound), ref, descs)
            same(gpu_steer(d_umem, descs, opts, d_table, default_port, n_ports, bound, want_out=False), ref, descs)


# ---- crafted port patterns ---------------------------------------------------------------------------------------

def _addr(p):
    return bytes([10, 7, 0, p])


PORT_TABLE = {GS.key(_addr(p)): p for p in range(64)}


def port_batch(ports, stride=128, not_ours=()):
    """(umem, descs): frame i is an ICMP echo request to the address PORT_TABLE maps to ports[i]; the frames at the
    indices `not_ours` are UDP."""
    n = len(ports)
    umem = np.random.default_rng(n).integers(0, 256, n * stride, dtype=np.uint8)
    descs = np.zeros(n, CW.G_DESC)
    frames = {}
    for i, p in enumerate(ports):
        key = (int(p), i in not_ours)
        if key not in frames:
            frames[key] = np.frombuffer(GS.W.build(daddr=_addr(int(p)), proto=17 if key[1] else 1), np.uint8)
        f = frames[key]
        a = i * stride + (i % 16)
        umem[a:a + len(f)] = f
        descs[i] = (a, len(f), 0)
    return umem, descs


PATTERNS = {
    "ascending": (lambda n: np.arange(n) % 64, None),          # every lane of a wave a different port
    "descending": (lambda n: 63 - np.arange(n) % 64, None),
    "one_port": (lambda n: np.full(n, 5), None),
    "empty_middle": (lambda n: np.where((np.arange(n) // 3) % 2, 2, 61), None),   # d_off[p] == d_off[p + 1] between them
    "all_on_63": (lambda n: np.full(n, 63), None),
    "unbound_middle": (lambda n: np.arange(n) % 64, SS.ALL_BOUND & ~(1 << 31)),
}


@pytest.mark.parametrize("opts", [0, 0x17])
@pytest.mark.parametrize("n", [256, 257])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_port_patterns(pattern, n, opts):
    make, bound = PATTERNS[pattern]
    ports = make(n)
    umem, descs = port_batch(ports)
    ref = SS.spec_steer_batch(umem, descs, opts, PORT_TABLE, SS.PASS, 64, SS.ALL_BOUND if bound is None else bound)
    redirected = ref["actions"] == R
    if bound is None:
        assert redirected.all() and (ref["ports"] == ports).all()
    else:
        assert (ref["actions"][ports == 31] == D).all() and redirected[ports != 31].all()
        assert ref["off"][31] == ref["off"][32]
    if pattern == "empty_middle":
        assert ref["off"][3] == ref["off"][61] > 0 and ref["off"][64] == n
    if pattern == "all_on_63":
        assert list(ref["off"][:64]) == [0] * 64 and ref["off"][64] == n
    same(gpu_steer(umem, descs, opts, PORT_TABLE, SS.PASS, 64, bound), ref, descs)


@functools.lru_cache(maxsize=None)
def _random_port_base(nb):
    rng = np.random.default_rng(nb)
    ports = rng.integers(0, 64, nb)
    not_ours = set(np.nonzero(rng.random(nb) < 0.2)[0].tolist())
    umem, descs = port_batch(ports, not_ours=not_ours)
    bound = SS.ALL_BOUND & ~(1 << 40)
    ref = SS.spec_steer_batch(umem, descs, 0x17, PORT_TABLE, SS.PASS, 64, bound)
    assert set(ref["actions"].tolist()) == {D, P, R}
    return umem, descs, ref, bound


def test_more_cells_than_one_row_scan_holds_at_64_ports():
    """4097 frames at 64 ports: 17 workgroups of 256 frames, 1088 cells -- more than 1024, the threads of one scan
    workgroup, and more than one workgroup's frames per port."""
    n, n_ports = 4097, 64
    assert X.steer_workspace_size(n, n_ports) // 4 == 1088 > 1024 == X.steer_workspace_size(n - 1, n_ports) // 4
    umem, descs, ref, bound = _random_port_base(n)
    assert (np.diff(ref["off"].astype(np.int64))[:40] > 0).all()
    same(gpu_steer(umem, descs, 0x17, PORT_TABLE, SS.PASS, n_ports, bound), ref, descs)


@pytest.mark.parametrize("n_ports", [64, 3])
def test_a_scan_thread_owns_more_than_one_count(n_ports):
    """The geometry built scans the count matrix a row per workgroup: 256 frames per classify workgroup, one cell per
    workgroup and port, 1024 scan threads over a row.  The smallest batch at which a thread of the scan owns more than
    one count is therefore 1025 workgroups' worth at any port count, 256 * 1024 + 1 = 262 145 frames (262 144: one
    each); with one scan workgroup over the whole matrix it would have been 4097 frames at 64 ports, the test above.
    A 4099-frame base batch tiled at its stride; the spec's actions and ports are tiled with it and partitioned."""
    n, nb, stride = 262145, 4099, 128
    assert X.steer_workspace_size(256, 1) == 4 and X.steer_workspace_size(257, 1) == 8       # 256 frames a workgroup
    assert X.steer_workspace_size(n, n_ports) == 1025 * n_ports * 4                          # one cell each
    assert X.steer_workspace_size(n - 1, n_ports) == 1024 * n_ports * 4                      # 1024: the scan's threads
    umem, descs, ref, bound = _random_port_base(nb)
    if n_ports != 64:  # the same frames under three ports: the rest are "no entry in the map"
        ref = SS.spec_steer_batch(umem, descs, 0x17, PORT_TABLE, SS.PASS, n_ports, bound)
    big, d, a_ref = CW.tile_batch(umem, descs, ref["actions"], n, stride)
    p_ref = np.tile(ref["ports"], (n + nb - 1) // nb)[:n]
    want = SS.partition(d, a_ref, p_ref, n_ports)
    assert int(want["off"][n_ports]) > (8000 if n_ports == 3 else 190000)  # a condition of the input
    same(gpu_steer(big, d, 0x17, PORT_TABLE, SS.PASS, n_ports, bound), want, d)


# ---- descriptors -------------------------------------------------------------------------------------------------

def test_descriptor_edges_with_a_table():
    """The descriptors of test_gpu_classify_wire.test_descriptor_edges, steered: rule 1, and frames that end flush with
    the UMEM whose destination is a table address -- for the 34-byte IPv4 frame the last four bytes of the UMEM."""
    opts = 0x17
    size = 4096
    umem = np.random.default_rng(17).integers(0, 256, size, dtype=np.uint8)
    echo6 = np.frombuffer(G6.build6(), np.uint8)
    echo4 = np.frombuffer(G6.W.build(payload=b""), np.uint8)[:34]
    assert len(echo6) == 62 and len(echo4) == 34
    umem[0:62] = echo6
    umem[size - 62:] = echo6
    umem[1024:1024 + 62] = echo6
    umem[2048 - 34:2048] = echo4
    descs = np.zeros(10, CW.G_DESC)
    descs[0] = (0, 62, 0)
    descs[1] = (size - 62, 62, 0)            # the minimal ICMPv6 echo request flush with the end
    descs[2] = (size - 62, 63, 0)            # crosses the end by one byte
    descs[3] = (size + 1, 14, 0)             # addr > umem_size
    descs[4] = (1024, (1 << 30) + 1, 0)      # len > XSK_GPU_MAX_LEN
    descs[5] = (size - 13, 13, 0)
    descs[6] = (size, 0, 0)
    descs[7] = (1024, 62, 0)
    descs[8] = (size - 61, 61, 0)
    descs[9] = (1 << 40, 62, 0)
    table = {GS.key(GS.V6_LOCAL): 2, GS.key(GS.V4_LOCAL): 1}
    ref = SS.spec_steer_batch(umem, descs, opts, table, SS.PASS, 4)
    assert list(ref["actions"][:8]) == [R, R, D, D, D, D, D, R] and ref["actions"][9] == D
    assert list(ref["ports"][[0, 1, 7]]) == [2, 2, 2] and list(ref["off"]) == [0, 0, 0, 3, 3]
    same(gpu_steer(umem, descs, opts, table, SS.PASS, 4), ref, descs)
    # a 34-byte IPv4 ICMP frame flush with the end of a UMEM of its own, under every option word and 0
    um2 = umem[:2048].copy()
    assert bytes(um2[-4:]) == GS.V4_LOCAL
    d2 = np.zeros(2, CW.G_DESC)
    d2[0] = (2048 - 34, 34, 0)
    d2[1] = (2048 - 33, 33, 0)               # the last 33 bytes: not that frame any more, the spec decides
    for o in GS.OPTION_WORDS:
        ref2 = SS.spec_steer_batch(um2, d2, o, table, SS.PASS, 4)
        assert (ref2["actions"][0], ref2["ports"][0]) == (R, 1)
        same(gpu_steer(um2, d2, o, table, SS.PASS, 4), ref2, d2)


def test_empty_batch_zeroes_the_offsets():
    dev = _dev()
    umem, descs = _mixed(64)
    d_umem, d_descs = to_dev(umem), to_dev(np.ascontiguousarray(descs, X.DESC_DTYPE))
    act = torch.full((64,), CANARY, dtype=torch.uint8, device=dev)
    ports = torch.full((64,), CANARY, dtype=torch.uint8, device=dev)
    out = torch.full((64 * 16,), CANARY, dtype=torch.uint8, device=dev)
    off = torch.full((3 + 1 + 2,), -1, dtype=torch.int32, device=dev)
    X.steer_dev(d_umem, d_descs, 0, None, 0, 0, 3, None, act, ports, out, off, opts=0x17)
    torch.cuda.synchronize()
    assert off.cpu().tolist() == [0, 0, 0, 0, -1, -1]
    for t in (act, ports, out):
        assert bool((t == CANARY).all())
