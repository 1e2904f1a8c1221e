"""tests/stream_paths.py without a GPU: the path selector against hand-computed tiles and against the shapes the GPU
tests build, and the references alone on long frames (the C oracle and the Python spec against a big-integer RFC 1071
sum), so that a long-frame mismatch on the GPU is the kernel's."""
import numpy as np
import pytest

import oracle
from tests import stream_paths as S
from tests.v6_frames import G6, spec_batch
from tests.wire_frames import G_DESC

MIB = 1 << 20
SIZE = 1 << 24


def descs_of(pairs):
    d = np.zeros(len(pairs), G_DESC)
    for i, (a, ln) in enumerate(pairs):
        d[i] = (a, ln, 0)
    return d


def tile_at(length, off=0, stride=4096, n=64):
    return [(i * stride + off, length) for i in range(n)]


def one(pairs, wire=False, size=SIZE, tile_live=64):
    return S.tile_paths(descs_of(pairs), size, wire, tile_live)


# ---- selector edges, by hand ----------------------------------------------------------------------------------
def test_lim_64_65_128_129():
    assert one(tile_at(64)) == ["short"]            # lim = 64: every frame inside its window
    assert one(tile_at(63, off=1)) == ["short"]
    assert one(tile_at(65)) == ["mid_uni"]          # lim = 65
    assert one(tile_at(64, off=1)) == ["mid_uni"]   # off + len = 65
    assert one(tile_at(128)) == ["mid_uni"]         # lim = 128
    assert one(tile_at(113, off=15)) == ["mid_uni"]
    assert one(tile_at(129)) == ["sorted"]          # lim = 129: one row-load (< 4): ranked streams
    assert one(tile_at(114, off=15)) == ["sorted"]
    # a short frame's lim is its window (64) while the window lies in the UMEM; the UMEM end clips it
    assert one(tile_at(20)) == ["short"]
    assert one([(SIZE - 48, 20)], size=SIZE) == ["short"]


def test_nit_3_and_4():
    assert one(tile_at(768)) == ["sorted"]          # 3 row-loads: too short to fill a batch of four
    assert one(tile_at(769)) == ["uniform"]         # 4 row-loads
    assert one(tile_at(753, off=15)) == ["sorted"]  # off + len = 768
    assert one(tile_at(754, off=15)) == ["uniform"]
    assert one([(i * 4096 + i % 16, 1000) for i in range(64)]) == ["per_step"]


def test_one_other_end_one_unparsed_and_partial_tiles():
    t = tile_at(1500)
    assert one(t) == ["uniform"]
    u = list(t)
    u[17] = (u[17][0], 1499)                        # same row-load count, another end
    assert one(u) == ["per_step"]
    u[17] = (u[17][0], 1200)                        # another row-load count
    assert one(u) == ["sorted"]
    u[17] = (u[17][0], 10)                          # one frame too short to parse: no loads, the others are equal
    assert one(u) == ["per_step"] and one(u, wire=True) == ["per_step"]
    u[17] = (u[17][0], 14)                          # wire mode parses from 14 bytes on (lim = its window: 1 load)
    assert one(u) == ["per_step"] and one(u, wire=True) == ["sorted"]
    u[17] = (SIZE + 16, 1500)                       # a bad descriptor
    assert one(u) == ["per_step"]
    assert one(t[:63]) == ["per_step"]              # fewer than 64 live frames: the dead lane does not parse
    assert one(tile_at(98)[:63]) == ["mid"] and one(tile_at(98)) == ["mid_uni"]
    assert one(tile_at(60)[:63]) == ["short"]
    assert one(t + t[:5]) == ["uniform", "per_step"]
    assert one([(SIZE + 16, 64)] * 64) == ["none"] and one([(0, 0)] * 3) == ["none"]
    assert one(t, tile_live=4) == ["per_step"] * 16  # 4-frame sub-tiles


def test_reference_and_wire_need():
    # reference mode reads [0, 38) of any frame of 20 bytes or more; wire mode only the frame
    last = [(SIZE - 30, 30)]
    assert one(last, wire=True) == ["short"] and one(last, wire=False) == ["none"]
    assert one([(SIZE - 38, 30)], wire=False) == ["short"]
    assert one([(0, 16)], wire=True) == ["short"] and one([(0, 16)], wire=False) == ["none"]
    assert one([(0, MIB * 1024 + 1)], size=1 << 31) == ["none"]  # len > XSK_GPU_MAX_LEN


def test_uniform_length_bound_and_far_tiles():
    big = 1 << 33
    assert one(tile_at(65536, stride=1 << 17), size=big) == ["uniform"]          # 256 row-loads
    assert one(tile_at(65521, off=15, stride=1 << 17), size=big) == ["uniform"]
    assert one(tile_at(65537, stride=1 << 17), size=big) == ["per_step"]         # 257
    assert one(tile_at(65536, off=1, stride=1 << 17), size=big) == ["per_step"]
    assert one(tile_at(MIB, stride=2 * MIB), size=big) == ["per_step"]
    far = [((2 << 30) + (64 << 20) if i % 2 else 0) + i * 2048 for i in range(64)]
    assert one([(a, 1500) for a in far], size=big) == ["per_step_far"]
    assert one([(a, 300 + 17 * i) for i, a in enumerate(far)], size=big) == ["sorted_far"]
    assert one([(a, 60) for a in far], size=big) == ["short"]
    assert one([(a, 98) for a in far], size=big) == ["mid_uni"]


# ---- the shapes the GPU tests build take their paths ------------------------------------------------------------
@pytest.mark.parametrize("v6", [False, True])
@pytest.mark.parametrize("shape", S.SHAPES)
def test_shape_batches_take_their_paths(shape, v6):
    for off in S.SHAPE_OFFS[shape]:
        umem, descs, path = S.shape_batch(shape, v6, off, 64 * 5 + 17)
        for wire in (False, True):
            got = S.tile_paths(descs, umem.nbytes, wire)
            assert got[0] == path and got[1] == path and got[2] == path and got[4] == path, (shape, off, got)
            assert len(got) == 6 and got[5] != "none"


@pytest.mark.parametrize("v6", [False, True])
def test_long_batches_take_their_paths(v6):
    for length in (65_535, 65_536, 131_072, 131_200):
        umem, descs = S.long_batch(v6, S.uniform_tiles(length, "zero", (0, 6)), 192)
        want = ["uniform" if (o + length + 255) >> 8 <= 256 else "per_step" for o in (0, 6)]
        assert S.tile_paths(descs, umem.nbytes, True) == want + ["short"]
    for length in (131_200, 140_000, 300_000, MIB):
        tile = S.per_step_tile(length, "zero")
        assert len({(o + ln + 255) >> 8 for ln, o, _ in tile}) == 1 and len({o for _, o, _ in tile}) == 16
        if length != MIB:
            umem, descs = S.long_batch(v6, [tile], 128)
            assert S.tile_paths(descs, umem.nbytes, False) == ["per_step", "short"]
    tile = S.ragged_tile("zero", 60_000, 131_200)
    umem, descs = S.long_batch(v6, [tile], 64)
    assert S.tile_paths(descs, umem.nbytes, True) == ["sorted"]
    assert len({(o + ln + 255) >> 8 for ln, o, _ in tile}) > 32 and min((o + ln) >> 8 for ln, o, _ in tile) > 7


# ---- the references alone are right on long frames -----------------------------------------------------------------
def big_csum16(data: bytes) -> int:
    """RFC 1071 by one big integer: the sum of the 16-bit big-endian words is the number's digit sum in base 65536,
    and x mod 65535 keeps it (0 only for all-zero data, else 1 .. 65535 with 65535 for multiples)."""
    if len(data) % 2:
        data += b"\0"
    x = int.from_bytes(data, "big")
    return 0 if x == 0 else (x % 0xFFFF or 0xFFFF)


def test_big_csum16_is_csum16():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 7, 64, 1501):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert big_csum16(d) == G6.csum16(d)
    assert big_csum16(b"\xff" * 40) == 0xFFFF and big_csum16(b"\0" * 9) == 0 and big_csum16(b"\0\x01") == 1


@pytest.mark.parametrize("length", [65_535, 131_072, 140_000, MIB, 2 * MIB + 4096])
@pytest.mark.parametrize("kind", S.PAYLOADS)
def test_references_on_long_frames(kind, length):
    off = 6
    for v6 in (False, True):
        for strict in (False, True):
            f = S.frame(v6, length, kind, 1, 0x1234, strict=strict)
            umem, descs = S.place([f], [off], (length + 512) & ~255)
            l4 = 54 if v6 else 34
            opt_sets = ((7, 0x17) if strict else (0, 6, 0x16)) if not v6 else ((0x17,) if strict else (0x16,))
            for opts in opt_sets:
                ref = umem.copy()
                if opts & 0x10:
                    v, r, _ = spec_batch(ref, descs, opts)
                elif opts:
                    v, r, _ = oracle.echo_batch_opts(ref, descs, opts)
                else:
                    v, r, _ = oracle.echo_batch(ref, descs)
                end = length
                if opts & 1:
                    end = 14 + int.from_bytes(f[16:18], "big") if not v6 else 54 + int.from_bytes(f[18:20], "big")
                    assert end <= length
                msg = f[l4:end]
                if v6:
                    msg = G6.pseudo(f[22:38], f[38:54], end - l4) + msg
                assert int(v[0]) == G6.TX_REPLY, (v6, strict, opts, v)
                assert int(r[0]["icmp_sum"]) == big_csum16(msg) == 0xFFFF, (v6, strict, opts, r[0])
                want_flags = (0x10 | 2) if v6 else 3
                assert int(r[0]["flags"]) == want_flags, (v6, strict, opts, r[0])
                a = off
                assert bytes(ref[a + l4:a + l4 + 1]) == (b"\x81" if v6 else b"\0")  # the reply's type
                assert (ref[:a] == umem[:a]).all() and (ref[a + length:] == umem[a + length:]).all()
            if v6:  # the spec itself, on the frame alone
                vi, rec, _ = G6.expect(f, length, 0x17 if strict else 0x16)
                assert vi == G6.TX_REPLY and rec["icmp_sum"] == 0xFFFF and rec["flags"] == 0x12
