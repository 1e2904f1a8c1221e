// xsk_echo_indirect.h — launch geometry of xsk_gpu_echo_dev_indirect() (include/xsk_gpu.h): the
// transform whose frame count is a word in device memory, read when the kernel executes.  The host knows only the bound
// n_max, so it sizes the launches from n_max and every workgroup works out its own share from the count it reads.  A
// header of its own so that the same functions compile for the host: tests/c/test_indirect_geometry.cpp checks on the
// CPU that the shares partition the tiles and equal the direct launch's.
//
// The direct launch (echo_launch, xsk_echo.hip) gives a batch of n frames, ntiles = ceil(n / 64) tiles, to
// g = min(ncu, ntiles) workgroups, each a contiguous share of per = ceil(ntiles / g) tiles (echo6_geometry,
// xsk_echo_device.h); workgroups whose share would start past the last tile are not launched.  The indirect launch
// starts G = min(ncu, ntiles(n_max)) workgroups.  For n <= n_max, min(G, ntiles(n)) = min(ncu, ntiles(n)): workgroup b
// computes the direct launch's `per` and takes the direct launch's share [b * per, b * per + per), or nothing where the
// direct launch has no workgroup b.
//
// Pieces: the direct launch runs a batch of more than 4 rounds (of 32 tiles) per workgroup as consecutive launches of
// about 2 rounds each over consecutive slices of the descriptors.  The indirect launch keeps the rule, derived from
// n_max: piece p owns the descriptors [i0, i0 + len) and serves ind_piece_n(n, i0, len) of them.
#ifndef XSK_ECHO_INDIRECT_H
#define XSK_ECHO_INDIRECT_H

#include <stdint.h>

#include "../../include/xsk_gpu.h"

#ifdef __HIPCC__
#define XSK_IND_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define XSK_IND_FN static inline
#endif

namespace xskgpu {

constexpr uint32_t kIndTile = XSK_GPU_TILE_FRAMES;
constexpr uint32_t kIndRound = 32;      // tiles of one workgroup's round: kWaves6 * kRefTPW (xsk_echo_device.h)
constexpr uint32_t kIndMaxRounds = 4;   // echo_launch's kMaxRounds
constexpr uint32_t kIndPieceRounds = 2; // echo_launch's kPieceRounds

XSK_IND_FN uint32_t ind_ntiles(uint32_t n) { return n / kIndTile + (n % kIndTile ? 1u : 0u); }

// Frames of piece [i0, i0 + len) in a batch of n: clamp(n - i0, 0, len).
XSK_IND_FN uint32_t ind_piece_n(uint32_t n, uint32_t i0, uint32_t len) {
    if (n <= i0) return 0u;
    return n - i0 < len ? n - i0 : len;
}

// The tiles [*t_begin, *t_end) of workgroup `wg` of a launch of `launched` workgroups over n frames; empty for n == 0
// and for a workgroup the direct launch of n would not have.
XSK_IND_FN void ind_share(uint32_t n, uint32_t launched, uint32_t wg, uint32_t* t_begin, uint32_t* t_end) {
    const uint32_t ntiles = ind_ntiles(n);
    uint32_t g = launched < ntiles ? launched : ntiles;
    if (g < 1u) g = 1u;
    const uint32_t per = (ntiles + g - 1u) / g;
    const uint64_t b = (uint64_t)wg * per, e = b + per;
    *t_begin = (uint32_t)(b < ntiles ? b : ntiles);
    *t_end = (uint32_t)(e < ntiles ? e : ntiles);
}

// Workgroups the host launches for a bound of n_max frames on ncu compute units.
XSK_IND_FN uint32_t ind_grid(uint32_t n_max, uint32_t ncu) {
    const uint32_t ntiles = ind_ntiles(n_max);
    uint32_t g = ncu < ntiles ? ncu : ntiles;
    return g < 1u ? 1u : g;
}

// Consecutive launches a bound of n_max frames runs as, and the tiles of each but the last (*piece_tiles).
XSK_IND_FN uint32_t ind_pieces(uint32_t n_max, uint32_t ncu, uint32_t* piece_tiles) {
    const uint32_t ntiles = ind_ntiles(n_max), g = ind_grid(n_max, ncu);
    const uint32_t per = (ntiles + g - 1u) / g;
    const uint32_t rounds = (per + kIndRound - 1u) / kIndRound;
    const uint32_t pieces = rounds > kIndMaxRounds ? (rounds + kIndPieceRounds - 1u) / kIndPieceRounds : 1u;
    *piece_tiles = (ntiles + pieces - 1u) / pieces;
    return pieces;
}

}  // namespace xskgpu

#endif  // XSK_ECHO_INDIRECT_H
