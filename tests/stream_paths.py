"""Which stream path the read phase of echo6_body (xsknet_amd/csrc/xsk_echo_device.h) takes for each tile of a batch,
restated in Python, and builders of batches that aim at one path each (no GPU needed).

tile_paths() derives, per tile, the quantities the kernel derives per lane -- need, ok, parse, off, rowhi, wend, lim,
nit, ukey, span -- and walks the same if / else chain, so a GPU test can assert on the CPU that its batch really takes
the path it is about before the GPU is asked.  The frame builders are thin wrappers over make_wire_golden.build and
make_v6_golden.build6: valid echo requests of a given total length with a 0xFF, 0x00 or seeded random payload, placed
at addr = i * stride + off_i in a UMEM of seeded random bytes, so that a stray write shows.
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
