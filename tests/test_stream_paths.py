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


# ---- the resident kernels' tiling, restated ------------------------------------------------------------------------
def test_resident_slices_and_groups():
    """Literal values worked out from xsk_gpu__ll_slice / xsk_gpu__ll_groups (xsk_lowlat_proto.h); the group cases are
    those of tests/c/test_lowlat_proto.c, step 10."""
    assert [S.ll_slice(1024, 4, g) for g in range(4)] == [(0, 256), (256, 512), (512, 768), (768, 1024)]
    assert [S.ll_slice(1023, 4, g) for g in range(4)] == [(0, 256), (256, 512), (512, 768), (768, 1023)]
    assert [S.ll_slice(65, 4, g) for g in range(4)] == [(0, 20), (20, 40), (40, 60), (60, 65)]  # per = 17 -> 20
    assert [S.ll_slice(5, 4, g) for g in range(4)] == [(0, 4), (4, 5), (5, 5), (5, 5)]
    assert S.ll_slice(64, 1, 0) == (0, 64)
    for n in (1, 3, 64, 65, 127, 1000, 1024):  # as step 9 there: contiguous, multiples of 4 but the last, covering
        for w in range(1, S.LL_WG + 1):
            sl = [S.ll_slice(n, w, g) for g in range(w)]
            assert sl[0][0] == 0 and sl[-1][1] == n and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
            assert all((f1 - f0) % 4 == 0 for f0, f1 in sl if f1 < n)
    d = descs_of(tile_at(1500, n=1024))
    assert S.ll_groups(d[:64]) == 1 and S.ll_groups(d[:65]) == 4 and S.ll_groups(d[:100]) == 4 and S.ll_groups(d) == 4
    d = descs_of(tile_at(64, n=1024))
    assert S.ll_groups(d[:128]) == 1 and S.ll_groups(d[:129]) == 4              # 8 KiB; more than 128 frames
    assert S.ll_groups(d[:300]) == 4 and S.ll_groups(d[:256]) == 4
    d[0]["len"] = 1500
    assert S.ll_groups(d[:128]) == 1                                            # 9.5 KiB
    d[:16]["len"] = 1500
    assert S.ll_groups(d[:128]) == 4                                            # 30 KiB
    # the 128-frame / 16 KiB line itself, and a frame counted up to 4096 B only
    d = descs_of(tile_at(128, n=128))
    assert int(d["len"].sum()) == 16 << 10 and S.ll_groups(d) == 1
    d[77]["len"] = 129
    assert S.ll_groups(d) == 4
    d = descs_of(tile_at(64, n=128))
    d[:2]["len"] = 1 << 20                                                      # 2 x 4096 + 126 x 64 = 16 256
    assert S.ll_groups(d) == 1
    d[2]["len"] = 1 << 20                                                       # 20 288
    assert S.ll_groups(d) == 4


def test_resident_tile_size():
    """xsk_gpu__small_tile (xsk_gpu_internal.h) of slice 0, one size for every slice; the tuned values replace it."""
    assert S.resident_tiling(descs_of(tile_at(64, n=64))) == (64, [(0, 64)])      # 4 KiB: one wave, one 64-frame tile
    assert S.resident_tiling(descs_of(tile_at(98, n=64))) == (64, [(0, 64)])      # 6.1 KiB: the RX loop's 64 pings
    assert S.resident_tiling(descs_of(tile_at(1500, n=1024))) == \
        (16, [(0, 256), (256, 512), (512, 768), (768, 1024)])                     # 375 KiB a slice: 16 waves of 16
    assert S.resident_tiling(descs_of(tile_at(1500, n=64))) == (8, [(0, 64)])     # 93.75 KiB: 12 waves, 6 -> 8 frames
    assert S.resident_tiling(descs_of(tile_at(98, n=1024)))[0] == 64              # 24.5 KiB a slice: 4 waves of 64
    assert S.resident_tiling(descs_of(tile_at(128, n=128))) == (64, [(0, 128)])   # 16 KiB on the leader: 2 waves
    assert S.resident_tiling(descs_of(tile_at(1500, n=1))) == (4, [(0, 1)])
    assert S.resident_tiling(descs_of(tile_at(1 << 20, n=64, stride=1 << 21))) == (4, [(0, 64)])  # 4 KiB each
    # slice 0 decides: 256 frames of 64 B (2 waves: 64 a tile) in front of 768 of 1500 B
    d = descs_of(tile_at(1500, n=1024))
    d[:256]["len"] = 64
    assert S.resident_tiling(d)[0] == 64
    # tuned (xsk_gpu__lowlat_tune): min(groups, n) workgroups, tile_frames a tile
    d = descs_of(tile_at(1500, n=1024))
    assert S.resident_tiling(d, groups=1, tile_frames=64) == (64, [(0, 1024)])
    assert S.resident_tiling(d, groups=2) == (32, [(0, 512), (512, 1024)])        # 750 KiB: 16 waves of 32
    assert S.resident_tiling(d[:2], groups=4) == (4, [(0, 2), (2, 2)])            # the second slice empty
    assert S.resident_tiling(d[:64], tile_frames=4) == (4, [(0, 64)])
    # tiles start at their slice's first frame: 65 frames of 1500 B, 4 slices of 20 / 20 / 20 / 5 frames; slice 0 is
    # 29.3 KiB, 4 waves, ceil(20 / 4) = 5 -> 8 frames a tile: tiles of 8, 8, 4 frames per full slice, one of 5
    assert S.resident_tiling(d[:65]) == (8, [(0, 20), (20, 40), (40, 60), (60, 65)])
    assert S.resident_tile_paths(d[:65], SIZE, False) == ["per_step"] * 10
    d2 = d[:65].copy()
    d2[16:20]["len"] = 60  # the third tile of slice 0, and no part of a tile of slice 1
    assert S.resident_tile_paths(d2, SIZE, False) == ["per_step"] * 2 + ["short"] + ["per_step"] * 7
    assert S.resident_tile_paths(d[:64], SIZE, False, tile_frames=64) == ["uniform"]
    assert S.resident_tile_paths(d[:64], SIZE, False) == ["per_step"] * 8


@pytest.mark.parametrize("v6", [False, True])
def test_resident_path_tables(v6):
    """The resident-kernel matrix's three batches of every case take the paths of S.resident_table, in reference and in
    wire mode, and their union is the six ordinary paths."""
    for wire in (False, True):
        reached = {name: set() for name, *_ in S.RESIDENT_GEOMETRIES}
        for shape in S.SHAPES:
            want = S.resident_table(shape, v6)
            for off in S.SHAPE_OFFS[shape]:
                umem, descs, path = S.shape_batch(shape, v6, off, 1105)
                for name, n, groups, tile in S.RESIDENT_GEOMETRIES:
                    got = S.resident_tile_paths(descs[:n], umem.nbytes, wire, groups, tile)
                    assert {p: got.count(p) for p in set(got)} == want[name], (shape, off, wire, name, got)
                    reached[name] |= set(got)
                    if name == "tuned":  # whole 64-frame tiles: the shape's own path on the plain tiles
                        assert got[0] == got[1] == path
        assert reached["full"] == reached["poll"] == {"mid_uni", "mid", "short", "per_step", "sorted"}, reached
        assert reached["tuned"] == {"mid_uni", "mid", "short", "uniform", "per_step", "sorted"}, reached


@pytest.mark.parametrize("v6", [False, True])
def test_indirect_counts_reach_every_ordinary_path(v6):
    """The indirect-kernel matrix (tests/test_gpu_indirect_paths.py: counts 1105 and 100 of every case's 1105-frame
    batch): the full count keeps the shape's path on tiles 0 and 1; count 100 keeps it on tile 0 and cuts tile 1 at
    36 live frames, which turns `uniform` into `per_step` and `mid_uni` into `mid`; every ordinary path is reached in
    both modes."""
    for wire in (False, True):
        reached = set()
        for shape in S.SHAPES:
            for off in S.SHAPE_OFFS[shape]:
                umem, descs, path = S.shape_batch(shape, v6, off, 1105)
                full = S.tile_paths(descs, umem.nbytes, wire)
                cut = S.tile_paths(descs[:100], umem.nbytes, wire)
                assert len(full) == 18 and full[0] == full[1] == path and full[17] != "none"
                assert cut == [path, {"uniform": "per_step", "mid_uni": "mid"}.get(path, path)], (shape, off, cut)
                reached |= set(full) | set(cut)
        assert reached == {"mid_uni", "mid", "short", "uniform", "per_step", "sorted"}, reached


@pytest.mark.parametrize("v6", [False, True])
def test_indirect_long_batches_take_their_paths(v6):
    for name, (tiles, n, want) in S.INDIRECT_LONG_BATCHES.items():
        umem, descs = S.long_batch(v6, tiles(), n)
        assert umem.nbytes <= 40 * MIB
        for wire in (False, True):
            assert S.tile_paths(descs, umem.nbytes, wire) == want, name


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
