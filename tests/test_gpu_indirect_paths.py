"""The stream-path matrix of tests/test_gpu_stream_paths.py and the long frames of tests/test_gpu_long_frames.py on the
indirect-count kernels: echo_indirect_kernel<false> (opts 0), echo_indirect_kernel<true> (wire mode) and
echo_ds_indirect_kernel (XSK_GPU_OPT_IPV6) -- echo6_body at RoundCfg<..., false> behind the count prologue of
xsk_echo_indirect.h, instantiations of their own that only xsk_gpu_echo_dev_indirect reaches.

The count is written by a device-side fill, as in tests/test_gpu_ingress.py.  Every case checks the prefix rule of
test_indirect_transform bit for bit: the first `count` frames, verdicts and records are the reference's over
descs[:count] (the C oracle for opts without XSK_GPU_OPT_IPV6, the Python spec with it), every UMEM byte outside them,
every verdict and record at or above `count` keeps its bytes or its sentinel, the counters are the reference's over the
prefix.  tile_paths says on the CPU which path each tile takes, for the full count and for the cut one.
"""
import numpy as np
import pytest

import oracle
from tests import stream_paths as S

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests.test_gpu_long_frames import FAMILIES  # noqa: E402
from tests.test_gpu_parity import FAR_GAP, FAR_N, FAR_SIZE, _dev, far_tile_descs, far_tile_setup  # noqa: E402
from tests.test_gpu_stream_paths import CASES, MODES, N_ROUND, _batch, _spec  # noqa: E402
from tests.test_gpu_v6 import KEYS  # noqa: E402
from tests.v6_frames import G6, spec_batch  # noqa: E402

COUNTS = (N_ROUND, 100)  # every tile but the last whole; tile 1 cut at 36 live frames
CUT = {"uniform": "per_step", "mid_uni": "mid"}  # what a tile of equal frames becomes with dead lanes


def kernel_of(opts):
    return "echo_ds_indirect_kernel" if opts & 0x10 else f"echo_indirect_kernel<{'true' if opts else 'false'}>"


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(_dev())


def reference(umem, descs, opts):
    """(UMEM after, verdicts, records, counters) over `descs`: the C oracle, or the Python spec under OPT_IPV6."""
    ref = umem.copy()
    if opts & 0x10:
        v, r, s = spec_batch(ref, descs, opts)
    elif opts:
        v, r, s = oracle.echo_batch_opts(ref, descs, opts)
    else:
        v, r, s = oracle.echo_batch(ref, descs)
    return ref, v, r, s


def run_indirect(d_orig, d_descs, n_max, count, opts):
    """xsk_gpu_echo_dev_indirect on a clone of d_orig with the count filled on the device: (UMEM tensor, verdicts and
    record bytes with their sentinels, counters)."""
    dev = _dev()
    d_umem = d_orig.clone()
    verd = torch.full((n_max + 64,), 0xEE, dtype=torch.uint8, device=dev)
    recs = torch.full(((n_max + 4) * 16,), 0xEE, dtype=torch.uint8, device=dev)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    cnt.fill_(count)  # a fill kernel on the current stream: the count exists only on the device
    X.echo_dev_indirect(d_umem, d_descs, cnt, n_max, verd, recs, stats, opts=opts)
    torch.cuda.synchronize()
    assert int(cnt.cpu()[0]) == count
    return d_umem, verd.cpu().numpy(), recs.cpu().numpy().reshape(-1, 16), stats.cpu().numpy().view(X.STATS_DTYPE)[0]


def check_prefix(what, got, ref, descs, count):
    """The prefix rule.  ref: the reference over descs[:count] (its UMEM holds every byte outside those frames
    unchanged).  A mismatch names `what` (kernel, batch, count, paths), the first differing frame and the field."""
    d_umem, v, r, s = got
    ref_umem, v_ref, r_ref, s_ref = ref
    assert len(v_ref) == count
    bad = np.nonzero(v[:count] != v_ref)[0]
    assert len(bad) == 0, (what, "verdict", bad[:5], v[bad[:5]], v_ref[bad[:5]], descs[bad[:5]])
    rr = np.ascontiguousarray(r[:count]).view(X.REC_DTYPE).reshape(-1)
    rr_ref = np.ascontiguousarray(r_ref).view(X.REC_DTYPE).reshape(-1)
    for name in rr.dtype.names:
        bad = np.nonzero(rr[name] != rr_ref[name])[0]
        assert len(bad) == 0, (what, "record." + name, bad[:5], rr[bad[:3]], rr_ref[bad[:3]], descs[bad[:3]])
    assert (rr.view(np.uint8) == rr_ref.view(np.uint8)).all(), (what, "record bytes")
    assert (v[count:] == 0xEE).all() and (r[count:] == 0xEE).all(), (what, "sentinels at or above the count")
    for k in KEYS:
        assert int(s[k]) == int(s_ref[k]), (what, "counter " + k, int(s[k]), int(s_ref[k]))
    d_ref = ref_umem if torch.is_tensor(ref_umem) else to_dev(ref_umem)
    if not torch.equal(d_umem, d_ref):
        diff = torch.nonzero(d_umem != d_ref).flatten()[:8].cpu().numpy()
        addr = descs["addr"].astype(np.int64)
        order = np.argsort(addr, kind="stable")
        fr = int(order[max(int(np.searchsorted(addr[order], diff[0], side="right")) - 1, 0)])  # the frame at or below
        raise AssertionError((what, "UMEM", f"first differing bytes at {diff}", "frame", fr,
                              "below the count" if fr < count else "at or above the count", descs[fr],
                              "byte of frame", int(diff[0]) - int(addr[fr])))


# ---- ordinary lengths: every path x mode ------------------------------------------------------------------------
@pytest.mark.parametrize("v6,opts", MODES, ids=[f"{'ipv6' if v else 'ipv4'}-{o:#x}" for v, o in MODES])
@pytest.mark.parametrize("shape,off", CASES)
def test_indirect_path_by_mode(shape, off, v6, opts):
    umem, descs, path = _batch(shape, v6, off)
    n_max = N_ROUND
    assert len(descs) == n_max
    wire = opts != 0
    full = S.tile_paths(descs, umem.nbytes, wire)
    cut = S.tile_paths(descs[:100], umem.nbytes, wire)
    assert full[0] == full[1] == path and cut == [path, CUT.get(path, path)], (shape, off, full[:4], cut)
    _dev()
    d_orig, d_descs = to_dev(umem), to_dev(descs)
    for count, paths in zip(COUNTS, (full, cut)):
        d = descs[:count]
        ref = _spec(shape, v6, off, count, opts) if opts & 0x10 else reference(umem, d, opts)
        if v6 and opts == 0x17:  # answered, but for the bad checksum of tile 2 where the prefix holds it
            v_ref = ref[1]
            if count > 2 * 64 + 21:
                assert (v_ref == G6.TX_REPLY).sum() == count - 1 and v_ref[2 * 64 + 21] == G6.DROP_BAD_CSUM
            else:
                assert (v_ref == G6.TX_REPLY).all()
        what = (kernel_of(opts), hex(opts), shape, off, "count", count, paths[:4])
        check_prefix(what, run_indirect(d_orig, d_descs, n_max, count, opts), ref, descs, count)


# ---- long frames: the 64-bit sums and the kUniMaxNit limit ---------------------------------------------------------
def _long(family, name):
    """The frames of one long batch, built once for all of a family's option sets and counts: (UMEM, descriptors,
    paths), UMEM and descriptors also on the device."""
    v6, strict, _ = FAMILIES[family]
    tiles, n, want = S.INDIRECT_LONG_BATCHES[name]
    umem, descs = S.long_batch(v6, tiles(), n, strict=strict)
    assert umem.nbytes <= 40 << 20 and len(descs) == n
    return umem, descs, want, to_dev(umem), to_dev(descs)


@pytest.mark.parametrize("name", list(S.INDIRECT_LONG_BATCHES))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_indirect_long_frames(family, name):
    """Frames of 131 200 B (two tiles of equal 0xFF frames at offsets 0 and 6, a per-step tile, a ranked one: only
    64-bit sums hold) and of 65 536 B (stream_tile_uniform's longest tile, 256 row-loads, and one row-load more at
    offset 6), with the count at the bound and inside tile 2."""
    opt_sets = FAMILIES[family][2]
    umem, descs, want, d_orig, d_descs = _long(family, name)
    n = len(descs)
    mid = 2 * 64 + 10
    for wire in (False, True):
        if wire or 0 in opt_sets:
            assert S.tile_paths(descs, umem.nbytes, wire) == want
            assert S.tile_paths(descs[:mid], umem.nbytes, wire)[:2] == want[:2]
    for opts in opt_sets:
        # the reference once: over the first `mid` frames, then the rest on top (frames do not overlap)
        ref_mid = reference(umem, descs[:mid], opts)
        rest_umem, v1, r1, s1 = reference(ref_mid[0], descs[mid:], opts)
        ref_all = (rest_umem, np.concatenate([ref_mid[1], v1]), np.concatenate([ref_mid[2], r1]),
                   {k: int(ref_mid[3][k]) + int(s1[k]) for k in KEYS})
        nlong = 64 * (len(want) - 1)
        assert (ref_all[1][:nlong] == X.TX_REPLY).all(), np.unique(ref_all[1][:nlong])  # the long tiles are answered
        for count, ref in ((n, ref_all), (mid, ref_mid)):
            what = (kernel_of(opts), hex(opts), family, name, "count", count, want)
            check_prefix(what, run_indirect(d_orig, d_descs, n, count, opts), ref, descs, count)


# ---- tiles that span more than 2 GiB: the 64-bit-address streams ----------------------------------------------------
@pytest.mark.parametrize("opts", [0, 7, 0x17])
@pytest.mark.parametrize("mode,lo,hi", [(1, 20, 1500), (0, 1500, 1500)], ids=["ragged", "uniform1500"])
def test_indirect_tile_spanning_more_than_2gib(mode, lo, hi, opts):
    """The layout of test_gpu_parity.test_tile_spanning_more_than_2gib (200 frames alternating across a 2 GiB gap)
    through xsk_gpu_echo_dev_indirect with n_max = count = 200: 64-frame tiles, so every tile spans the gap; ragged
    tiles take sorted_far, equal 1500-B frames per_step_far.  The oracle runs on the compact host image."""
    n = FAR_N
    far_descs = far_tile_descs(mode, lo, hi, opts)[1]
    paths = S.tile_paths(far_descs, FAR_SIZE, opts != 0, 64)
    assert len(paths) == 4 and set(paths) == {"sorted_far" if mode else "per_step_far"}, paths
    d_umem, descs, img, hd = far_tile_setup(mode, lo, hi, opts)
    v_ref, r_ref, s_ref = oracle.echo_batch_opts(img, hd, opts & 7)
    got = run_indirect(d_umem, to_dev(descs), n, n, opts)
    del d_umem
    out, v, r, s = got
    what = (kernel_of(opts), hex(opts), paths)
    bad = np.nonzero(v[:n] != v_ref)[0]
    assert len(bad) == 0, (what, "verdict", bad[:5], v[bad[:5]], v_ref[bad[:5]], descs[bad[:5]])
    rr, rr_ref = np.ascontiguousarray(r[:n]).view(X.REC_DTYPE).reshape(-1), r_ref.view(X.REC_DTYPE).reshape(-1)
    bad = np.nonzero(rr != rr_ref)[0]
    assert len(bad) == 0, (what, "record", bad[:5], rr[bad[:3]], rr_ref[bad[:3]], descs[bad[:3]])
    assert (v[n:] == 0xEE).all() and (r[n:] == 0xEE).all()
    for k in KEYS:
        assert int(s[k]) == int(s_ref[k]), (what, "counter " + k)
    span = n * 2048 + 64
    for name, base, want in (("low", 0, img[:span]), ("high", FAR_GAP, img[span:])):
        diff = np.nonzero(out[base:base + span].cpu().numpy() != want)[0]
        assert len(diff) == 0, (what, "UMEM", name, "region: first differing bytes at", diff[:8], "frame",
                                diff[:1] // 2048)
