"""The stream-path matrix of tests/test_gpu_stream_paths.py on the resident (LOWLAT) kernels of xsk_lowlat.hip:
lowlat_kernel<false> (opts 0), lowlat_kernel<true> (wire mode) and resident_ds_kernel (XSK_GPU_OPT_IPV6).  They are
instantiations of echo6_body of their own (ResidentCfg), reached only through a doorbell.

Every case's 1105-frame batch (tests/stream_paths.shape_batch) goes through one LOWLAT context three times, the UMEM
restored in between (S.RESIDENT_GEOMETRIES): its first 1024 frames at the product's geometry (4 workgroups), its first
64 frames (the leader alone, on the descriptors its poll brought: the 64-pings batch of the RX loop), and the 1024
frames again on one workgroup in whole 64-frame tiles, the only geometry in which a resident kernel takes
stream_tile_uniform.  resident_tile_paths asserts on the CPU which paths each call takes (S.resident_table) before the GPU is asked, and
lowlat_served() that the resident kernel served it.  Every UMEM byte, verdict, record and counter is compared with the
C oracle (opts without XSK_GPU_OPT_IPV6) or the Python spec (with it) over exactly the descriptors of the call.
"""
import numpy as np
import pytest

import oracle
from tests import stream_paths as S

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests.test_gpu_parity import _dev  # noqa: E402
from tests.test_gpu_stream_paths import CASES, MODES, _batch, _spec  # noqa: E402
from tests.test_gpu_v6 import KEYS  # noqa: E402
from tests.v6_frames import G6, spec_batch  # noqa: E402


def kernel_of(opts):
    return "resident_ds_kernel" if opts & 0x10 else ("lowlat_kernel<true>" if opts else "lowlat_kernel<false>")


def reference(umem, descs, opts):
    """(UMEM after, verdicts, records, counters) of the C oracle over `descs`."""
    ref = umem.copy()
    v, r, s = oracle.echo_batch_opts(ref, descs, opts) if opts else oracle.echo_batch(ref, descs)
    return ref, v, r, s


def compare(what, got, ref, descs):
    """(UMEM, verdicts, records, counters) of a call against the reference's; a mismatch names `what` (kernel, shape,
    offset, geometry, paths), the first differing frame and the field."""
    out, v, r, s = got
    ref_umem, v_ref, r_ref, s_ref = ref
    bad = np.nonzero(v != v_ref)[0]
    assert len(bad) == 0, (what, "verdict", bad[:5], v[bad[:5]], v_ref[bad[:5]], descs[bad[:5]])
    rr, rr_ref = r.view(X.REC_DTYPE).reshape(-1), np.ascontiguousarray(r_ref).view(X.REC_DTYPE).reshape(-1)
    for name in rr.dtype.names:
        bad = np.nonzero(rr[name] != rr_ref[name])[0]
        assert len(bad) == 0, (what, "record." + name, bad[:5], rr[bad[:3]], rr_ref[bad[:3]], descs[bad[:3]])
    assert (rr.view(np.uint8) == rr_ref.view(np.uint8)).all(), (what, "record bytes")
    for k in KEYS:
        assert int(s[k]) == int(s_ref[k]), (what, "counter " + k, int(s[k]), int(s_ref[k]))
    diff = np.nonzero(np.asarray(out) != ref_umem)[0]
    if len(diff):
        addr = descs["addr"].astype(np.int64)
        order = np.argsort(addr, kind="stable")
        fr = int(order[max(int(np.searchsorted(addr[order], diff[0], side="right")) - 1, 0)])  # the frame at or below
        raise AssertionError((what, "UMEM", f"{len(diff)} bytes differ, first at {diff[:8]}", "frame", fr, descs[fr],
                              "byte of frame", int(diff[0]) - int(addr[fr])))


@pytest.mark.parametrize("v6,opts", MODES, ids=[f"{'ipv6' if v else 'ipv4'}-{o:#x}" for v, o in MODES])
@pytest.mark.parametrize("shape,off", CASES)
def test_resident_path_by_mode(shape, off, v6, opts):
    umem, descs, _ = _batch(shape, v6, off)
    table = S.resident_table(shape, v6)
    _dev()
    work = X.umem_copy(umem)
    with X.EchoContext(work, 0, max_batch=1024, mode=X.MODE_LOWLAT, opts=opts) as ctx:
        assert ctx.mode == X.MODE_LOWLAT
        served = ctx.lowlat_served()
        assert served == (0, 0)
        for name, n, groups, tile in S.RESIDENT_GEOMETRIES:
            d = descs[:n]
            got = S.resident_tile_paths(d, umem.nbytes, opts != 0, groups, tile)
            assert {p: got.count(p) for p in set(got)} == table[name], (shape, off, name, got)
            what = (kernel_of(opts), hex(opts), shape, off, name, table[name])
            if opts & 0x10:
                ref = _spec(shape, v6, off, n, opts)
                if v6 and opts == 0x17:  # answered, but for the bad checksum of tile 2 where the batch holds it
                    v_ref = ref[1]
                    if n > 2 * 64 + 21:
                        assert (v_ref == G6.TX_REPLY).sum() == n - 1 and v_ref[2 * 64 + 21] == G6.DROP_BAD_CSUM
                    else:
                        assert (v_ref == G6.TX_REPLY).all()
            else:
                ref = reference(umem, d, opts)
            if groups or tile:
                ctx.lowlat_tune(tile_frames=tile, groups=groups)
            work[:] = umem
            v, r, s = ctx.process(d)
            now = ctx.lowlat_served()
            assert now == (served[0] + 1, served[1]), (what, served, now)  # the resident kernel, not a launch
            served = now
            compare(what, (work, v, r, s), ref, d)


@pytest.mark.parametrize("v6", [False, True], ids=["ipv4", "ipv6"])
def test_resident_ds_long_uniform_batch(v6):
    """One 64-frame batch of 140 000-B 0xFF frames through the dual-stack resident kernel (opts 0x16): 16 tiles of 4
    frames on the leader, the per-step streams (64-bit sums: a 32-bit row total wraps from 131 110 B of 0xFF on)."""
    opts = 0x16
    umem, descs = S.long_batch(v6, S.uniform_tiles(140_000, "ff", (0,)), 64)
    assert S.resident_tiling(descs) == (4, [(0, 64)])
    assert S.resident_tile_paths(descs, umem.nbytes, True) == ["per_step"] * 16
    ref = umem.copy()
    v_ref, r_ref, s_ref = spec_batch(ref, descs, opts)
    assert (v_ref == X.TX_REPLY).all() and (r_ref["icmp_sum"] == 0xFFFF).all()
    assert (r_ref["flags"] == (0x12 if v6 else 3)).all()
    _dev()
    work = X.umem_copy(umem)
    with X.EchoContext(work, 0, max_batch=64, mode=X.MODE_LOWLAT, opts=opts) as ctx:
        assert ctx.mode == X.MODE_LOWLAT
        v, r, s = ctx.process(descs)
        assert ctx.lowlat_served() == (1, 0)
    compare((kernel_of(opts), hex(opts), "140000 B ff", "ipv6" if v6 else "ipv4"), (work, v, r, s),
            (ref, v_ref, r_ref, s_ref), descs)
