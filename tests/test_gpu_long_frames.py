"""Frames longer than 64 KiB through every stream path that can carry them, in reference, wire and dual-stack mode.

include/xsk_gpu.h accepts descriptors up to XSK_GPU_MAX_LEN and promises exact records for them; the uniform-tile
stream sums 16-bit halves in 32 bits, which holds only up to 64 KiB frames (0xFF payloads wrap a row total from
len = 131 110 on, random ones from about 256 KiB), so longer uniform tiles must take a path with 64-bit sums.  Every
case compares every UMEM byte, verdict, record and counter with the C oracle (opts without XSK_GPU_OPT_IPV6) or the
Python spec (with it), on the round kernel (n = 1152) and on the sub-tile kernel (the first 1024 frames, one workgroup:
whole 64-frame tiles).  tests/stream_paths.tile_paths says on the CPU which path each batch takes before the GPU runs.
"""
import numpy as np
import pytest

import oracle
from tests import stream_paths as S

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests.test_gpu_parity import _check_grid, _dev  # noqa: E402
from tests.test_gpu_v6 import KEYS, gpu_v6, same  # noqa: E402
from tests.v6_frames import spec_batch  # noqa: E402

N_ROUND, N_SUB = 1152, 1024
MIB = 1 << 20
LENGTHS = [65_535, 65_536, 131_072, 131_200, 140_000, 300_000, MIB]
# (IPv6 frames?, STRICT-shaped frames?) -> the option sets that family runs under
FAMILIES = {
    "v4": (False, False, (0, 6, 0x16)),
    "v4_strict": (False, True, (7, 0x17)),
    "v6": (True, False, (0x16,)),
    "v6_strict": (True, True, (0x17,)),
}


def expected_uniform_path(length, off):
    """stream_tile_uniform up to 256 row-loads (off + len <= 64 KiB), the per-step streams beyond."""
    return "uniform" if (off + length + 255) >> 8 <= S.UNI_MAX_NIT else "per_step"


def run_both_kernels(umem, descs, opts, nlong):
    """The batch on the round kernel and its first N_SUB frames on the sub-tile kernel (grid 1: 64-frame tiles),
    each against the reference of exactly the frames it ran."""
    assert len(descs) > X.LOWLAT_MAX and N_SUB <= X.LOWLAT_MAX and S.sub_tile_live(N_SUB, 1) == 64
    if not opts & 0x10:
        _check_grid(umem, descs, 0, opts)
        _check_grid(umem, descs[:N_SUB], 1, opts)
        return
    # the Python spec once: the first N_SUB frames, then the rest on top (frames do not overlap)
    ref_sub = umem.copy()
    v0, r0, s0 = spec_batch(ref_sub, descs[:N_SUB], opts)
    ref = ref_sub.copy()
    v1, r1, s1 = spec_batch(ref, descs[N_SUB:], opts)
    s_all = {k: s0[k] + s1[k] for k in KEYS}
    assert (v0[:nlong] == X.TX_REPLY).all(), np.unique(v0[:nlong])  # the tiles under test are answered
    same(gpu_v6(umem, descs, opts, 0), (ref, np.concatenate([v0, v1]), np.concatenate([r0, r1]), s_all), descs)
    same(gpu_v6(umem, descs[:N_SUB], opts, 1), (ref_sub, v0, r0, s0), descs[:N_SUB])


def run_family(tiles, want_paths, family):
    v6, strict, opt_sets = FAMILIES[family]
    umem, descs = S.long_batch(v6, tiles, N_ROUND, strict=strict)
    assert umem.nbytes <= 150 * MIB
    for wire in (False, True):
        if not wire and 0 not in opt_sets:
            continue
        for n, tl in ((N_ROUND, 64), (N_SUB, 64)):
            got = S.tile_paths(descs[:n], umem.nbytes, wire, tl)
            assert got[:len(tiles)] == list(want_paths), (got[:len(tiles)], want_paths)
    _dev()
    for opts in opt_sets:
        run_both_kernels(umem, descs, opts, 64 * len(tiles))


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("kind", S.PAYLOADS)
@pytest.mark.parametrize("length", LENGTHS)
def test_uniform_long_tiles(length, kind, family):
    """Two tiles of 64 equal frames, at offsets 0 and 6."""
    run_family(S.uniform_tiles(length, kind, (0, 6)), [expected_uniform_path(length, o) for o in (0, 6)], family)


@pytest.mark.parametrize("off", [0, 6])
def test_uniform_2mib_ff_reference_mode(off):
    """2 MiB + 4096 bytes of 0xFF: past 8192 row-loads a single lane's 32-bit sum of halves would wrap as well."""
    length = 2 * MIB + 4096
    umem, descs = S.long_batch(False, S.uniform_tiles(length, "ff", (off,)), 1088)
    assert umem.nbytes <= 150 * MIB
    assert S.tile_paths(descs, umem.nbytes, False)[0] == "per_step"
    _dev()
    _check_grid(umem, descs, 0, 0)
    _check_grid(umem, descs[:N_SUB], 1, 0)


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("kind", S.PAYLOADS)
@pytest.mark.parametrize("length", [131_200, 140_000, 300_000, MIB])
def test_per_step_long_tiles(length, kind, family):
    """Equal row-load counts at offsets j % 16: the per-step streams (64-bit sums, flushed every four blocks).  At
    1 MiB frame j is j % 16 bytes shorter, so that every frame still ends in row-load 4096."""
    run_family([S.per_step_tile(length, kind)], ["per_step"], family)


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("kind", S.PAYLOADS)
@pytest.mark.parametrize("hi", [131_200, 300_000, MIB])
def test_ragged_long_tiles(hi, kind, family):
    """Lengths spread over 60 000 .. hi: the ranked streams, ranked by the compare loop (row-loads > 7)."""
    tile = S.ragged_tile(kind, 60_000, hi)
    assert min((o + ln + 255) >> 8 for ln, o, _ in tile) > 7
    run_family([tile], ["sorted"], family)


@pytest.mark.parametrize("opts", [0, 6])
@pytest.mark.parametrize("mode", [X.MODE_ZEROCOPY, X.MODE_STAGED, X.MODE_LOWLAT])
def test_host_modes_long_uniform_batch(mode, opts):
    """One 64-frame batch of 140 000-B 0xFF frames through EchoContext.process in every host mode: whatever path the
    mode's kernel takes, the records are the oracle's."""
    umem, descs = S.long_batch(False, S.uniform_tiles(140_000, "ff", (0,)), 64)
    ref = umem.copy()
    v_ref, r_ref, s_ref = oracle.echo_batch_opts(ref, descs, opts) if opts else oracle.echo_batch(ref, descs)
    assert (v_ref == X.TX_REPLY).all() and (r_ref["flags"] == 3).all() and (r_ref["icmp_sum"] == 0xFFFF).all()
    _dev()
    work = X.umem_copy(umem)
    with X.EchoContext(work, 0, max_batch=64, mode=mode) as ctx:
        ctx.set_options(opts)
        v, r, s = ctx.process(descs)
    assert (v == v_ref).all(), np.nonzero(v != v_ref)[0][:10]
    bad = np.nonzero(r != r_ref)[0]
    assert len(bad) == 0, (bad[:5], r[bad[:3]], r_ref[bad[:3]])
    for k in KEYS:
        assert int(s[k]) == int(s_ref[k]), k
    diff = np.nonzero(np.asarray(work) != ref)[0]
    assert len(diff) == 0, f"{len(diff)} bytes differ, first at {diff[:8]}"
