// xsk_echo_geometry.h — the launch geometry of the transform, once: how a batch of n frames becomes tiles, workgroup
// shares, consecutive launches and workspace rows, for the direct launch (xsk_echo.hip), the indirect-count launch
// (xsk_echo_indirect.hip) and the tuning library.  Plain host functions: tests/c/test_indirect_geometry.cpp runs them.
#ifndef XSK_ECHO_GEOMETRY_H
#define XSK_ECHO_GEOMETRY_H

#include <stdint.h>

#include "../../include/xsk_gpu.h"

namespace xskgpu {

constexpr int kTile = XSK_GPU_TILE_FRAMES;  // frames per wave tile (= RX_BATCH_SIZE, xsk_utils.h:8)
constexpr int kWaves6 = 16;                 // waves per workgroup (one workgroup per CU)
constexpr int kRefTPW = 2;                  // reference mode: tiles per wave per round (2048 frames per CU)
constexpr uint32_t kRoundTiles = (uint32_t)kWaves6 * kRefTPW;  // tiles of one workgroup's round
constexpr uint32_t kMaxRounds = 4, kPieceRounds = 2;           // echo6_pieces
constexpr uint32_t kSmallWG = 16;       // workgroups a small batch's sub-tiles may spread over
constexpr uint32_t kMaxCuBound = 1024;  // workspace bound for the round kernel's one-workgroup-per-CU grid

// Workgroups a batch can use: one per CU, one per tile for fewer tiles (the indirect-count launch starts them all).
inline uint32_t echo6_max_grid(uint32_t n, uint32_t num_cu) {
    const uint32_t ntiles = (n + kTile - 1) / kTile;
    uint32_t g = num_cu < 1 ? 1 : num_cu;
    if (g > ntiles) g = ntiles < 1 ? 1 : ntiles;
    return g;
}

// Round kernel geometry: one workgroup per CU (fewer for small batches), equal contiguous tile shares.
inline void echo6_geometry(uint32_t n, uint32_t num_cu, uint32_t* grid, uint32_t* tiles_per_wg) {
    const uint32_t ntiles = (n + kTile - 1) / kTile;
    const uint32_t g = echo6_max_grid(n, num_cu);
    const uint32_t per = (ntiles + g - 1) / g;
    *tiles_per_wg = per < 1 ? 1 : per;
    *grid = (ntiles + *tiles_per_wg - 1) / *tiles_per_wg;
    if (*grid < 1) *grid = 1;
}

// A batch of more than kMaxRounds rounds per workgroup runs as consecutive launches of about kPieceRounds rounds
// each, over consecutive slices of its descriptors: every launch's last round scatters its windows while no
// workgroup of that launch still reads, where a long share writes every round's windows into other
// workgroups' reads (tools/split_bench.py, profiles/r04/split/: 8 M x 1500 B at 4 KiB, one launch 300.5 us per
// M frames, launches of 1 M 264.3; c5's 64 M at 2 KiB 19.50 -> 18.66 ms).  Returns the launches; *piece_tiles: the
// 64-frame tiles of each but the last.
inline uint32_t echo6_pieces(uint32_t n, uint32_t num_cu, uint32_t* piece_tiles) {
    const uint32_t ntiles = (n + kTile - 1) / kTile;
    uint32_t grid, per;
    echo6_geometry(n, num_cu, &grid, &per);
    const uint32_t rounds = (per + kRoundTiles - 1) / kRoundTiles;
    const uint32_t pieces = rounds > kMaxRounds ? (rounds + kPieceRounds - 1) / kPieceRounds : 1;
    *piece_tiles = (ntiles + pieces - 1) / pieces;
    return pieces;
}

// A small batch (n <= XSK_GPU_LOWLAT_MAX) runs as sub-tiles of *tl frames (a multiple of 4 in [4, 64]), one per wave, over
// up to kSmallWG workgroups of 16 waves: a device-resident batch (tile == 0) on every one of them (tl = ceil(n / 256),
// >= 4: tools/smallbatch.py measured 1024 x 1500 B in 14.6 us over 16 workgroups against 44.1 us on one); a zerocopy
// batch with the caller's tile (about 8 KiB of PCIe reads per wave, xsk_gpu__small_tile_w).  grid_force: workgroups.
inline void echo6_small_tiling(uint32_t n, uint32_t tile, uint32_t grid_force, uint32_t* tl, uint32_t* tiles_per_wg,
                               uint32_t* grid) {
    const uint32_t waves = kWaves6 * (grid_force ? grid_force : kSmallWG);
    const uint32_t t = tile ? ((tile + 3u) & ~3u) : ((n + waves - 1) / waves + 3u) & ~3u;
    *tl = t < 4u ? 4u : (t > (uint32_t)kTile ? (uint32_t)kTile : t);
    const uint32_t nt = (n + *tl - 1) / *tl;
    *tiles_per_wg = grid_force ? (nt + grid_force - 1) / grid_force : (uint32_t)kWaves6;
    *grid = (nt + *tiles_per_wg - 1) / *tiles_per_wg;
}

// Partial-counter rows of xsk_gpu_workspace_size(): the round kernel's grid, or a small batch's kSmallWG workgroups.
inline uint32_t echo6_workspace_rows(uint32_t n) {
    const uint32_t ntiles = (n + kTile - 1) / kTile;
    const uint32_t g = ntiles < kMaxCuBound ? ntiles : kMaxCuBound;
    return g < kSmallWG ? kSmallWG : g;
}

}  // namespace xskgpu

#endif  // XSK_ECHO_GEOMETRY_H
