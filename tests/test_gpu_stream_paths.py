"""Every stream path of the read phase at ordinary lengths, in reference, wire and dual-stack mode, with IPv4 and
IPv6 frames, on the round kernel and the sub-tile kernel.

wire_v6_phase takes a plain frame's checksum as the stream's sum of [34, len) plus [22, 34) from registers, so every
path must hand it a sum with exactly that meaning, at aligned and unaligned starts; the IPv4 header phases rely on the
same.  Each batch (tests/stream_paths.shape_batch) has plain tiles of the shape, a tile with one bad checksum, a tile
with a one-tag and a two-tag frame, and a last partial tile; tile_paths asserts on the CPU that the shape takes its
path before the GPU is asked.  Every UMEM byte, verdict, record and counter is compared with the C oracle (opts
without XSK_GPU_OPT_IPV6) or the Python spec (with it).
"""
import functools

import numpy as np
import pytest

from tests import stream_paths as S

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests.test_gpu_parity import _check_grid, _dev  # noqa: E402
from tests.test_gpu_v6 import gpu_v6, same  # noqa: E402
from tests.v6_frames import G6, spec_batch  # noqa: E402

N_ROUND, N_SUB = 1105, 1024  # 17 tiles and a partial one (the round kernel); 16 tiles (the sub-tile kernel)
# IPv4 and IPv6 frames at opts 0 (reference mode: IPv4 only), 7, 0x10, 0x17
MODES = [(False, 0), (False, 7), (False, 0x10), (False, 0x17), (True, 7), (True, 0x10), (True, 0x17)]
CASES = [(shape, off) for shape in S.SHAPES for off in S.SHAPE_OFFS[shape]]


@functools.lru_cache(maxsize=4)
def _batch(shape, v6, off):
    umem, descs, path = S.shape_batch(shape, v6, off, N_ROUND)
    umem.setflags(write=False)
    return umem, descs, path


@functools.lru_cache(maxsize=8)
def _spec(shape, v6, off, n, opts):
    umem, descs, _ = _batch(shape, v6, off)
    ref = umem.copy()
    return (ref,) + tuple(spec_batch(ref, descs[:n], opts))


def _assert_paths(shape, v6, off, wire):
    """The shape's path for at least the plain full tiles 0 and 1, in the round kernel's tiling and in the sub-tile
    kernel's at grid 1 (64-frame tiles)."""
    umem, descs, path = _batch(shape, v6, off)
    for n in (N_ROUND, N_SUB):
        got = S.tile_paths(descs[:n], umem.nbytes, wire, 64)
        assert got[0] == path and got[1] == path, (shape, got[:4], path)
    return path


@pytest.mark.parametrize("shape,off", CASES)
@pytest.mark.parametrize("v6,opts", MODES, ids=[f"{'ipv6' if v else 'ipv4'}-{o:#x}" for v, o in MODES])
@pytest.mark.parametrize("grid", [0, 1])
def test_path_by_mode(grid, v6, opts, shape, off):
    umem, descs, _ = _batch(shape, v6, off)
    _assert_paths(shape, v6, off, opts != 0)
    _dev()
    for n in (N_ROUND, N_SUB):  # the round kernel, the sub-tile kernel (grid 0: 4-frame sub-tiles, 1: 64-frame ones)
        d = descs[:n]
        if opts & 0x10:
            ref, v_ref, r_ref, s_ref = _spec(shape, v6, off, n, opts)
            if v6 and opts == 0x17:  # answered but for the bad checksum of tile 2 (DROP_BAD_CSUM under VERIFY)
                assert (v_ref == G6.TX_REPLY).sum() == n - 1 and v_ref[2 * 64 + 21] == G6.DROP_BAD_CSUM
            same(gpu_v6(umem.copy(), d, opts, grid), (ref, v_ref, r_ref, s_ref), d)
        else:
            _check_grid(umem.copy(), d, grid, opts)
