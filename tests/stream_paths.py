"""Which stream path the read phase of echo6_body (xsknet_amd/csrc/xsk_echo_device.h) takes for each tile of a batch,
restated in Python, and builders of batches that aim at one path each (no GPU needed).

tile_paths() derives, per tile, the quantities the kernel derives per lane -- need, ok, parse, off, rowhi, wend, lim,
nit, ukey, span -- and walks the same if / else chain, so a GPU test can assert on the CPU that its batch really takes
the path it is about before the GPU is asked.  The frame builders are thin wrappers over make_wire_golden.build and
make_v6_golden.build6: valid echo requests of a given total length with a 0xFF, 0x00 or seeded random payload, placed
at addr = i * stride + off_i in a UMEM of seeded random bytes, so that a stray write shows.

resident_tiling() / resident_tile_paths() restate the tiling of the resident (LOWLAT) kernels -- serving workgroups,
slices and frames per tile as xsk_gpu__lowlat_post posts them and the kernels of xsk_lowlat.hip derive them -- so the
same assertion holds for a doorbell batch.  The users: tests/test_gpu_stream_paths.py and tests/test_gpu_long_frames.py
(the launched round and sub-tile kernels), tests/test_gpu_resident_paths.py (lowlat_kernel<false>, lowlat_kernel<true>,
resident_ds_kernel) and tests/test_gpu_indirect_paths.py (echo_indirect_kernel<false>, <true>, echo_ds_indirect_kernel);
tests/test_stream_paths.py pins the selector, the restated tiling and the tables on the CPU.
"""
import functools

import numpy as np

from tests.v6_frames import G6
from tests.wire_frames import G, G_DESC

TILE = 64            # XSK_GPU_TILE_FRAMES
WIN = 64             # kWin: the header window
MAX_LEN = 1 << 30    # XSK_GPU_MAX_LEN
U = 4                # kU: a tile whose longest frame has fewer row-loads takes the ranked streams
UNI_MAX_NIT = 256    # kUniMaxNit: the longest tile of stream_tile_uniform (32-bit sums of halves)

PATHS = ("short", "mid_uni", "mid", "sorted", "sorted_far", "uniform", "per_step", "per_step_far", "none")
PAYLOADS = ("ff", "zero", "random")


def lane_geometry(addr: int, length: int, live: bool, umem_size: int, wire: bool):
    """One lane's (ok, parse, a16, off, rowhi, lim, nit, ukey) as frame_in() / the round body compute them."""
    need = length if wire else (max(length, 38) if length >= 20 else length)
    ok = live and length <= MAX_LEN and addr <= umem_size and need <= umem_size - addr
    parse = ok and length >= (14 if wire else 20)
    a16, off = addr & ~15, addr & 15
    rowhi = off + length if parse else 0
    wend = min(umem_size - a16, WIN) if ok else 0
    lim = max(rowhi, wend if parse else 0)
    nit = (lim + 255) >> 8
    ukey = ((off << 24) ^ rowhi) & 0xFFFFFFFF
    return ok, parse, a16, off, rowhi, lim, nit, ukey


def tile_path(lanes):
    """The path of one tile from its 64 lanes' lane_geometry() tuples (dead lanes included)."""
    assert len(lanes) == TILE
    lims = [x[5] for x in lanes]
    nits = [x[6] for x in lanes]
    ukeys = [x[7] for x in lanes]
    if not any(nits):
        return "none"
    short_tile = max(lims) <= WIN
    mid_tile = not short_tile and max(lims) <= 128
    one_key = all(k == ukeys[0] for k in ukeys)  # ballot(ukey != readfirstlane(ukey)) == 0, every lane of the wave
    if short_tile:
        return "short"
    if mid_tile:
        return "mid_uni" if one_key else "mid"
    wlo = min(x[2] for x in lanes if x[6])
    span = max(x[2] + x[5] for x in lanes if x[6]) - wlo
    fast = span < 0x80000000
    mx = max(nits)
    if any(n != 0 and n != mx for n in nits) or mx < U:
        return "sorted" if fast else "sorted_far"
    if fast and mx <= UNI_MAX_NIT and all(x[1] for x in lanes) and one_key:
        return "uniform"
    return "per_step" if fast else "per_step_far"


def tile_paths(descs, umem_size: int, wire: bool, tile_live: int = TILE):
    """One path name per tile, in tile order: tile t holds frames [t * tile_live, (t + 1) * tile_live) in lanes
    0 .. tile_live - 1 (tile_live < 64: the sub-tile kernel); the other lanes carry an all-zero descriptor."""
    n = len(descs)
    out = []
    for t in range((n + tile_live - 1) // tile_live):
        lanes = []
        for lane in range(TILE):
            fi = t * tile_live + lane
            live = lane < tile_live and fi < n
            a, ln = (int(descs[fi]["addr"]), int(descs[fi]["len"])) if live else (0, 0)
            lanes.append(lane_geometry(a, ln, live, umem_size, wire))
        out.append(tile_path(lanes))
    return out


def sub_tile_live(n: int, grid: int) -> int:
    """Frames per tile of a small batch (n <= XSK_GPU_LOWLAT_MAX) launched on `grid` workgroups (0: the default 16),
    as echo_launch() picks it."""
    wg = grid if grid else 16
    tl = ((n + 16 * wg - 1) // (16 * wg) + 3) & ~3
    return min(max(tl, 4), TILE)


# ---- the resident (LOWLAT) kernels' tiling --------------------------------------------------------------------------
LL_WG = 4            # XSK_GPU__LL_WG: workgroups of the resident grid
LOWLAT_MAX = 1024    # XSK_GPU_LOWLAT_MAX: the largest doorbell batch
LL_WAVES = 16        # kWaves6: waves of one resident workgroup


def _capped_bytes(descs) -> int:
    return int(np.minimum(np.asarray(descs["len"], np.uint64), 4096).sum())


def ll_groups(descs) -> int:
    """xsk_gpu__ll_groups (xsk_lowlat_proto.h): the leader alone up to 64 frames, and up to 128 frames of at most
    16 KiB (each frame counted up to 4096 B); every workgroup above."""
    n = len(descs)
    if n <= 64 or (n <= 128 and _capped_bytes(descs) <= 16 << 10):
        return 1
    return LL_WG


def ll_slice(n: int, w: int, g: int):
    """xsk_gpu__ll_slice: workgroup g's frames [f0, f1) of an n-frame batch over w workgroups."""
    per = ((n + w - 1) // w + 3) & ~3
    a = min(g * per, n)
    return a, min(a + per, n)


def small_tile(descs, max_waves: int = LL_WAVES) -> int:
    """xsk_gpu__small_tile_w (xsk_gpu_internal.h): frames per wave, 8 KiB of frame bytes (a frame counted up to
    4096 B) per wave, 1 .. max_waves waves, rounded up to a multiple of 4 and clamped to 4 .. 64."""
    n = len(descs)
    waves = min(max((_capped_bytes(descs) + 8191) // 8192, 1), max_waves)
    t = ((n + waves - 1) // waves + 3) & ~3
    return min(max(t, 4), TILE)


def resident_tiling(descs, groups: int = 0, tile_frames: int = 0):
    """(frames per tile, [(f0, f1) per serving workgroup]) of a doorbell batch, as xsk_gpu__lowlat_post (xsk_lowlat.hip)
    posts it and lowlat_kernel / resident_ds_kernel derive it: w = xsk_gpu__ll_groups, or min(groups, n) when tuned;
    one tile size for every slice, xsk_gpu__small_tile of slice 0's descriptors, or tile_frames when tuned
    (xsk_gpu__lowlat_tune); workgroup g serves slice g in tiles that start at the slice's first frame (a slice past
    the batch's end is empty: f0 == f1)."""
    n = len(descs)
    assert 0 < n <= LOWLAT_MAX and 0 <= groups <= LL_WG
    assert tile_frames == 0 or (4 <= tile_frames <= TILE and tile_frames % 4 == 0)
    w = min(groups, n) if groups else ll_groups(descs)
    slices = [ll_slice(n, w, g) for g in range(w)]
    f0, f1 = slices[0]
    tl = tile_frames if tile_frames else 4 * (small_tile(descs[f0:f1]) // 4)
    return tl, slices


def resident_tile_paths(descs, umem_size: int, wire: bool, groups: int = 0, tile_frames: int = 0):
    """tile_paths() of a doorbell batch in the resident kernels' tiling: one path per tile, slice after slice."""
    tl, slices = resident_tiling(descs, groups, tile_frames)
    out = []
    for f0, f1 in slices:
        out += tile_paths(descs[f0:f1], umem_size, wire, tl)
    return out


# ---- frames ---------------------------------------------------------------------------------------------------
def payload_bytes(kind: str, nbytes: int, seed: int = 0) -> bytes:
    if kind == "ff":
        return b"\xff" * nbytes
    if kind == "zero":
        return b"\0" * nbytes
    assert kind == "random"
    return np.random.default_rng(0x5EED0000 + seed).integers(0, 256, nbytes, dtype=np.uint8).tobytes()


def echo4(total: int, kind: str = "random", seed: int = 0, tags: int = 0, bad: bool = False, strict: bool = False,
          ident: int = 0x1234, seq: int = 7) -> bytes:
    """A valid IPv4 echo request of `total` bytes behind `tags` VLAN tags.  strict: a frame longer than tot_len can
    say (65535) carries the longest message that fits and Ethernet padding behind it; otherwise tot_len is the
    message's length modulo 2^16 (what reference mode and non-STRICT wire mode never look at)."""
    l4 = 14 + 4 * tags + 20
    assert total >= l4 + 8
    vlan = [(0x88A8, 5), (0x8100, 100)][2 - tags:] if tags else []
    npay = total - l4 - 8
    pad = 0
    if strict and total - 14 - 4 * tags > 65535:
        npay = 65535 - 20 - 8
        pad = total - l4 - 8 - npay
    f = G.build(vlan=vlan, payload=payload_bytes(kind, npay, seed), pad=pad, bad_icmp=bad, ident=ident, seq=seq)
    assert len(f) == total
    return f


def echo6(total: int, kind: str = "random", seed: int = 0, tags: int = 0, bad: bool = False, strict: bool = False,
          ident: int = 0x1234, seq: int = 7) -> bytes:
    """A valid ICMPv6 echo request of `total` bytes; strict: plen <= 65535 and Ethernet padding, as echo4()."""
    l4 = 14 + 4 * tags + 40
    assert total >= l4 + 8
    vlan = [(0x88A8, 5), (0x8100, 100)][2 - tags:] if tags else []
    npay = total - l4 - 8
    pad = 0
    if strict and npay + 8 > 65535:
        npay = 65535 - 8
        pad = total - l4 - 8 - npay
    f = G6.build6(vlan=vlan, payload=payload_bytes(kind, npay, seed), pad=pad, bad_icmp=bad, ident=ident, seq=seq)
    assert len(f) == total
    return f


@functools.lru_cache(maxsize=None)
def _base_frame(v6: bool, total: int, kind: str, seed: int, tags: int, bad: bool, strict: bool) -> bytes:
    return (echo6 if v6 else echo4)(total, kind, seed, tags, bad, strict, ident=0, seq=0xFFFF)


def frame(v6: bool, total: int, kind: str, seed: int, i: int, tags: int = 0, bad: bool = False,
          strict: bool = False) -> bytes:
    """Frame i of a family: the builder's frame for (total, kind, seed) with identifier i and sequence number ~i --
    the two words sum to 0xFFFF whatever i is, so the builder's checksum holds for every i and a batch of long
    frames costs one builder call per (length, payload), yet no two frames of a tile are the same."""
    f = bytearray(_base_frame(v6, total, kind, seed, tags, bad, strict))
    o = 14 + 4 * tags + (40 if v6 else 20) + 4
    i &= 0xFFFF
    f[o:o + 4] = bytes([i >> 8, i & 0xFF, (~i >> 8) & 0xFF, ~i & 0xFF])
    return bytes(f)


def place(frames, offs, stride: int, seed: int = 1, lens=None):
    """(umem, descs): frame i at addr = i * stride + offs[i] in a UMEM of seeded random bytes (16-B multiple)."""
    n = len(frames)
    rng = np.random.default_rng(0x5EEDCAFE + seed)
    size = (n * stride + 256 + 15) & ~15
    umem = rng.integers(0, 256, size, dtype=np.uint8)
    descs = np.zeros(n, G_DESC)
    for i, f in enumerate(frames):
        a = i * stride + offs[i]
        assert offs[i] + len(f) <= stride
        umem[a:a + len(f)] = np.frombuffer(f, np.uint8)
        descs[i] = (a, len(f) if lens is None else lens[i], 0)
    return umem, descs


def place_at(frames, addrs, size: int, seed: int = 1):
    """(umem, descs) with frame i at addrs[i] (non-overlapping, inside `size`)."""
    rng = np.random.default_rng(0x5EEDCAFE + seed)
    umem = rng.integers(0, 256, (size + 15) & ~15, dtype=np.uint8)
    descs = np.zeros(len(frames), G_DESC)
    for i, (f, a) in enumerate(zip(frames, addrs)):
        umem[a:a + len(f)] = np.frombuffer(f, np.uint8)
        descs[i] = (a, len(f), 0)
    return umem, descs


# ---- batches that aim at one path -----------------------------------------------------------------------------
FILL = 64  # the filler frames of a batch: 64-B echoes (62-B ICMPv6 ones), 64-B slots


def _filler(v6: bool, i: int) -> bytes:
    return frame(v6, 62 if v6 else 64, "random", 99, i)


def long_batch(v6: bool, tiles, n: int, strict: bool = False, seed: int = 1):
    """A batch of n frames whose first tiles have the shapes under test and whose rest are 64-B fillers.

    tiles: one list per leading tile of 64 (length, offset, kind) triples.  Each long frame gets a slot of its own
    (a multiple of 256 B past its end); the fillers follow at 64-B slots.  Returns (umem, descs)."""
    frames, addrs, a = [], [], 0
    for t, tile in enumerate(tiles):
        assert len(tile) == TILE
        for j, (ln, off, kind) in enumerate(tile):
            frames.append(frame(v6, ln, kind, ln & 0xFFFF, t * TILE + j, strict=strict))
            addrs.append(a + off)
            a += (off + ln + 255 + 256) & ~255
    for i in range(len(frames), n):
        frames.append(_filler(v6, i))
        addrs.append(a)
        a += FILL
    return place_at(frames, addrs, a + 256, seed)


def uniform_tiles(length: int, kind: str, offs=(0, 6)):
    return [[(length, off, kind)] * TILE for off in offs]


def per_step_tile(length: int, kind: str):
    """Equal row-load counts, offsets j % 16.  A length whose row-load count 15 more bytes would raise (a multiple of
    256, or up to 15 below one) is shortened by the frame's offset instead, so that every frame ends where the
    aligned one does."""
    if (length + 255) >> 8 == (length + 15 + 255) >> 8:
        return [(length, j % 16, kind) for j in range(TILE)]
    return [(length - j % 16, j % 16, kind) for j in range(TILE)]


def ragged_tile(kind: str, lo: int = 60_000, hi: int = 300_000):
    """Lengths spread over [lo, hi] (row-load counts all different and > 7: the compare-rank branch)."""
    return [(lo + (hi - lo) * ((j * 37) % TILE) // (TILE - 1), j % 16, kind) for j in range(TILE)]


# The long-frame batches of the indirect-kernel matrix: name -> (tiles, frames, tile_paths in reference and wire mode).
# "long": past 128 KiB, where only 64-bit sums hold (two equal-frame tiles, a per-step one, a ranked one, 41 fillers);
# "limit": 64 KiB frames, the longest stream_tile_uniform takes (256 row-loads at offset 0; offset 6 is one too many).
INDIRECT_LONG_BATCHES = {
    "long": (lambda: uniform_tiles(131_200, "ff", (0, 6)) + [per_step_tile(131_200, "random")]
             + [ragged_tile("zero", 60_000, 131_200)], 4 * 64 + 41,
             ["per_step", "per_step", "per_step", "sorted", "short"]),
    "limit": (lambda: uniform_tiles(65_536, "ff", (0, 6)), 2 * 64 + 41, ["uniform", "per_step", "short"]),
}


# ordinary lengths: shape name -> (expected path, per-frame (length, offset) of one tile as a function of j, v6)
def shape_tile(shape: str, v6: bool, off: int = 0):
    """64 (length, offset) pairs of one tile of `shape` and the path it must take."""
    if shape == "mid_uni":
        ln = 118 if v6 else 98
        return "mid_uni", [(ln, min(off, 128 - ln))] * TILE  # (118 B end past 128 from offset 11 on: 13 -> 10)
    if shape == "mid":
        return "mid", [(66 + (j * 7) % 47, j % 16) for j in range(TILE)]
    if shape == "uniform":
        return "uniform", [(1500, off)] * TILE
    if shape == "per_step":
        return "per_step", [(1500, j % 16) for j in range(TILE)]
    if shape == "sorted":
        return "sorted", [(300 + (j * 19) % 1201, j % 16) for j in range(TILE)]
    if shape == "short":
        return "short", [((62 if v6 else 42) + (0 if v6 else j % 7), (off + j) % 2 if off else 0) for j in range(TILE)]
    raise ValueError(shape)


SHAPES = ("mid_uni", "mid", "uniform", "per_step", "sorted", "short")
SHAPE_OFFS = {"mid_uni": (0, 6, 13), "uniform": (0, 6, 15), "short": (0, 1), "mid": (0,), "per_step": (0,),
              "sorted": (0,)}


# The three doorbell batches the resident-kernel matrix (tests/test_gpu_resident_paths.py) cuts from
# shape_batch(shape, v6, off, 1105): (name, frames, lowlat_tune groups, lowlat_tune tile_frames).  "full" and "poll" run
# at the product's own geometry (poll: <= 64 frames, the descriptors the leader's poll brought); "tuned" is one
# workgroup and whole 64-frame tiles, the only geometry in which a resident kernel takes stream_tile_uniform.
RESIDENT_GEOMETRIES = (("full", 1024, 0, 0), ("poll", 64, 0, 0), ("tuned", 1024, 1, 64))


def resident_table(shape: str, v6: bool):
    """{geometry name: {path: tiles}}: what resident_tile_paths must give for the three RESIDENT_GEOMETRIES batches of
    shape_batch(shape, v6, off, 1105), at every offset of SHAPE_OFFS[shape], in reference and in wire mode.  Worked out
    from xsk_gpu__ll_groups / xsk_gpu__ll_slice / xsk_gpu__small_tile: 1024 ping-size frames are 4 slices of 256 frames
    in 64-frame tiles (4 x 4 tiles), 1024 frames of 1500 B 4 slices in 16-frame tiles (4 x 16: a tile with dead lanes is
    never `uniform`), 64 frames of 1500 B one slice in 8-frame tiles (12 waves); two of the `sorted` shape's
    8-frame tiles hold one row-load count each (lengths 19 B apart).  IPv6 `short` frames behind VLAN tags (tile 3)
    are longer than their window: that tile is `mid`."""
    if shape in ("mid_uni", "mid"):
        return {"full": {shape: 16}, "poll": {shape: 1}, "tuned": {shape: 16}}
    if shape == "short":
        full = {"short": 15, "mid": 1} if v6 else {"short": 16}
        return {"full": full, "poll": {"short": 1}, "tuned": full}
    if shape == "uniform":
        return {"full": {"per_step": 64}, "poll": {"per_step": 8}, "tuned": {"uniform": 16}}
    if shape == "per_step":
        return {"full": {"per_step": 64}, "poll": {"per_step": 8}, "tuned": {"per_step": 16}}
    if shape == "sorted":
        return {"full": {"sorted": 64}, "poll": {"sorted": 6, "per_step": 2}, "tuned": {"sorted": 16}}
    raise ValueError(shape)


def shape_batch(shape: str, v6: bool, off: int, n: int, stride: int = 2048, seed: int = 1):
    """n frames at a fixed stride: tiles 0 and 1 are plain tiles of `shape` (valid echoes; tile 1 is the one a test
    asserts the path on), tile 2 the same shape with one frame whose checksum is bad, tile 3 with one one-tag and one
    two-tag frame, the rest the shape again, ending in a partial tile when n % 64 != 0.  Returns
    (umem, descs, expected path)."""
    path, tile = shape_tile(shape, v6, off)
    if shape == "short":
        stride = 128
    frames, offs = [], []
    for i in range(n):
        t, j = divmod(i, TILE)
        ln, o = tile[j]
        tags, bad = 0, False
        if t == 2 and j == 21:
            bad = True
        if t == 3 and j in (9, 40):
            tags = 1 if j == 9 else 2
            if shape in ("mid_uni", "uniform"):
                pass  # same length behind the tags: the tile keeps its one end
            elif shape == "short":
                ln = max(ln, 14 + 4 * tags + (40 if v6 else 20) + 8)
        kind = PAYLOADS[(t + j) % 3] if shape != "short" else "random"
        frames.append(frame(v6, ln, kind, (ln * 3 + t) & 0xFFFF, i, tags=tags, bad=bad))
        offs.append(o)
    umem, descs = place(frames, offs, stride, seed)
    return umem, descs, path
