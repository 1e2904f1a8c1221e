"""xsk_gpu_rearm_dev, four lanes per frame: bit for bit oracle.rearm on the CPU, the whole slab compared.

A wave covers 16 frames (lane 4f + k moves 16-B chunk k of frame f), a workgroup 64; a 16-B aligned frame is re-armed as its whole 64-B sector, any other byte by byte by one lane of its quad.  The
cases below put the end of the batch at every place inside a quad group, a wave and a workgroup, mix verdicts and
alignments inside one group of 16 frames, and drive the checksum patch of the chunk-2 lane through its end-around
carries.  Every slab is filled with random bytes first and compared as a whole, so a store that bleeds into a
neighbouring sector or frame shows.
"""
import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402

SIZES = [1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000]
LAYOUTS = {64: (64, 64), 2048: (64, 1500), 4096: (1500, 1500)}  # stride: (len_lo, len_hi)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(_dev())


def _noise(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def gpu_echo(umem, descs):
    """xsk_gpu_echo_dev on a copy of the host slab: (slab of replies, verdicts)."""
    d_umem, d_descs = _up(umem), _up(descs)
    d_verd = torch.full((len(descs),), 0xEE, dtype=torch.uint8, device=_dev())
    X.echo_dev(d_umem, d_descs, len(descs), d_verd)
    torch.cuda.synchronize()
    return d_umem.cpu().numpy(), d_verd.cpu().numpy()


def gpu_rearm(umem, descs, verdicts):
    d_umem = _up(umem)
    X.rearm_dev(d_umem, _up(descs), _up(verdicts), len(descs))
    torch.cuda.synchronize()
    return d_umem.cpu().numpy()


def check_rearm(umem, descs, verdicts):
    """The GPU's re-arm of (umem, descs, verdicts) against the oracle's: every byte of the slab."""
    want = umem.copy()
    oracle.rearm(want, descs, verdicts)
    got = gpu_rearm(umem, descs, verdicts)
    diff = np.nonzero(got != want)[0]
    assert len(diff) == 0, f"{len(diff)} bytes differ from oracle.rearm, first at {diff[:8]}"
    return got


@pytest.mark.parametrize("stride", sorted(LAYOUTS))
@pytest.mark.parametrize("n", SIZES)
def test_roundtrip_sizes(n, stride):
    """synth -> echo_dev -> rearm_dev == the original slab; the slab ends with the last frame's stride, so at 64 B the
    last sector ends exactly at the end of the UMEM and every neighbouring sector belongs to another frame."""
    lo, hi = LAYOUTS[stride]
    umem = _noise(n * stride, 1000 * stride + n)
    descs = oracle.synth_batch(umem, n, 0, stride, 0xA11CE + n, mode=0, len_lo=lo, len_hi=hi)
    replies, verd = gpu_echo(umem, descs)
    assert (verd == X.TX_REPLY).all()
    assert not (replies == umem).all()
    got = check_rearm(replies, descs, verd)
    assert (got == umem).all()


def _replies(n, stride=2048, lo=64, hi=1500, seed=0xBEEF):
    umem = _noise(n * stride, seed)
    descs = oracle.synth_batch(umem, n, 0, stride, seed, mode=0, len_lo=lo, len_hi=hi)
    replies, verd = gpu_echo(umem, descs)
    assert (verd == X.TX_REPLY).all()
    return umem, descs, replies


def _mixes(n):
    i = np.arange(n)
    one_in_wave = np.full(n, 3, np.uint8)
    one_in_wave[[37, 64 + 5]] = 0  # one TX frame in each of the first two waves' groups
    last_quad = np.full(n, 0xEE, np.uint8)
    last_quad[n - 1] = 0
    return {
        "all": np.zeros(n, np.uint8),
        "none": (1 + i % 7).astype(np.uint8),
        "alternating": (i % 2).astype(np.uint8),
        "alternating_odd": ((i + 1) % 2 * 5).astype(np.uint8),
        "one_in_wave": one_in_wave,
        "last_quad_only": last_quad,
        "random": (np.random.default_rng(5).integers(0, 3, n) == 0).astype(np.uint8),
    }


@pytest.mark.parametrize("stride", [64, 2048])
@pytest.mark.parametrize("mix", ["all", "none", "alternating", "alternating_odd", "one_in_wave", "last_quad_only",
                                 "random"])
def test_verdict_mixes(mix, stride):
    """Only TX_REPLY frames change: every byte of any other frame's sector is what it was (n = 197: the last wave and
    the last group of 16 are partial, the last frame sits alone in its group of four)."""
    n = 197
    lo, hi = LAYOUTS[stride]
    orig, descs, replies = _replies(n, stride, lo, hi)
    verd = _mixes(n)[mix]
    got = check_rearm(replies, descs, verd)
    for f in np.nonzero(verd != X.TX_REPLY)[0]:
        a = int(descs["addr"][f])
        assert (got[a:a + 64] == replies[a:a + 64]).all(), f
    for f in np.nonzero(verd == X.TX_REPLY)[0]:
        a = int(descs["addr"][f])
        assert (got[a:a + 64] == orig[a:a + 64]).all(), f


def _placed(offsets, len_lo, len_hi, slot=256, seed=0xF00D, tail=True):
    """Frames of len_lo .. len_hi bytes at addr = slot * i + offsets[i]; with `tail` one more frame follows, aligned
    and of at most 64 B, whose sector ends exactly at the end of the UMEM."""
    m = len(offsets)
    src = np.zeros((m + 1) * 2048, np.uint8)
    sd = oracle.synth_batch(src, m, 0, 2048, seed, mode=0, len_lo=len_lo, len_hi=len_hi)
    if tail:
        st = oracle.synth_batch(src, 1, m * 2048, 2048, seed + 7, mode=0, len_lo=min(len_lo, 64), len_hi=64)
        sd = np.concatenate([sd, st])
    n = len(sd)
    size = n * slot
    umem = _noise(size, seed + 1)
    descs = np.zeros(n, oracle.DESC_DTYPE)
    for i in range(n):
        L, s0 = int(sd["len"][i]), int(sd["addr"][i])
        a = slot * i + int(offsets[i]) if i < m else size - 64
        assert a + max(L, 64) <= slot * (i + 1)
        umem[a:a + L] = src[s0:s0 + L]
        descs[i] = (a, L, 0)
    return umem, descs


@pytest.mark.parametrize("lens", [(42, 63), (64, 64), (42, 200)])
def test_alignment_mixes(lens):
    """Aligned frames and frames at offsets 1, 6, 13 and 15 inside one wave and inside one group of 16 frames (the
    pattern has period 7, so every group of 16 sees each of them), frames shorter than 64 B at unaligned addresses,
    and a last, aligned frame whose sector ends with the UMEM."""
    pat = [0, 1, 0, 6, 13, 0, 15]
    umem, descs = _placed([pat[i % len(pat)] for i in range(149)], *lens)
    work = umem.copy()
    verd, _, _ = oracle.echo_batch(work, descs)  # the transform itself is not under test here
    assert (verd == X.TX_REPLY).all()
    got = check_rearm(work, descs, verd)
    assert (got == umem).all()
    # and with some frames held back, aligned and unaligned ones alike
    verd[::3] = 4
    check_rearm(work, descs, verd)


def test_all_unaligned_wave():
    """Whole waves of unaligned frames: no lane takes the sector path."""
    umem, descs = _placed([1 + i % 15 for i in range(130)], 42, 120, tail=False)
    work = umem.copy()
    verd, _, _ = oracle.echo_batch(work, descs)
    assert (verd == X.TX_REPLY).all()
    assert (check_rearm(work, descs, verd) == umem).all()


CSUMS = [0x0000, 0xFFFF, 0xFFF7, 0x0008, 0xFFF6, 0xFFF8, 0x0007, 0x0009, 0x0800, 0xF7FF, 0xF6FF, 0xF8FF, 0x1234]


@pytest.mark.parametrize("offset", [0, 6])
def test_checksum_edges(offset):
    """Bytes 36-37 of the reply at the values where rearm_csum's two end-around carries fire or just do not, in both
    byte orders, through the chunk-2 lane (aligned) and the byte path (offset 6)."""
    n = 2 * len(CSUMS) + 3
    umem, descs = _placed([offset] * n, 64, 64, tail=False)
    verd, _, _ = oracle.echo_batch(umem, descs)
    assert (verd == X.TX_REPLY).all()
    for i, c in enumerate(CSUMS):
        for j, (b0, b1) in enumerate(((c & 0xFF, c >> 8), (c >> 8, c & 0xFF))):
            a = int(descs["addr"][2 * i + j])
            umem[a + 36], umem[a + 37] = b0, b1
    check_rearm(umem, descs, verd)
