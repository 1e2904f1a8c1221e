// The transform's launch geometry (xsknet_amd/csrc/xsk_echo_geometry.h) and the device prologue of
// xsk_gpu_echo_dev_indirect (xsk_echo_indirect.h) compiled for the host: for launches sized from a bound n_max, and
// every count n <= n_max the kernels may read, the shares the workgroups of all pieces work out for themselves
// partition the tiles of n -- none twice, none missing -- and within one launch each workgroup's share is the one the
// direct launch of that many frames gives it (echo6_geometry, the function the host launches with).  Then the small
// batches' sub-tiling (echo6_small_tiling), for every size the host may give it.  Stand-alone: prints "indirect
// geometry ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../xsknet_amd/csrc/xsk_echo_indirect.h"

using namespace xskgpu;

#define CHECK(c, ...)                     \
    do {                                  \
        if (!(c)) {                       \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            exit(1);                      \
        }                                 \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t bound) {  // xorshift64*, [0, bound]
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return (uint32_t)(((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % ((uint64_t)bound + 1));
}

static uint64_t check_one(uint32_t n_max, uint32_t ncu, uint32_t n, std::vector<uint8_t>& seen) {
    const uint32_t ntiles_max = ind_ntiles(n_max), ntiles = ind_ntiles(n);
    uint32_t piece_tiles = 0;
    const uint32_t pieces = echo6_pieces(n_max, ncu, &piece_tiles);
    CHECK(piece_tiles >= 1 && (uint64_t)pieces * piece_tiles >= ntiles_max, "pieces do not cover n_max %u", n_max);
    seen.assign(ntiles_max + 1, 0);
    uint64_t shares = 0;
    uint32_t launches = 0, sum_len = 0;
    for (uint32_t t0 = 0; t0 < ntiles_max; t0 += piece_tiles, ++launches) {  // the host's loop (xsk_echo_indirect.hip)
        const uint32_t i0 = t0 * 64;
        const uint64_t cap = (uint64_t)piece_tiles * 64;
        const uint32_t len = (uint32_t)(n_max - i0 < cap ? n_max - i0 : cap);
        sum_len += len;
        const uint32_t grid = echo6_max_grid(len, ncu);
        CHECK(grid >= 1 && grid <= ncu && grid <= ind_ntiles(len), "grid %u for len %u ncu %u", grid, len, ncu);
        const uint32_t np = ind_piece_n(n, i0, len);  // the kernel's prologue
        CHECK(np <= len && (n <= i0 ? np == 0 : np == (n - i0 < len ? n - i0 : len)), "piece_n");
        uint32_t dg = 0, dper = 0;
        echo6_geometry(np, ncu, &dg, &dper);
        const uint32_t nt = ind_ntiles(np);
        for (uint32_t wg = 0; wg < grid; ++wg) {
            uint32_t b = 0, e = 0;
            ind_share(np, grid, wg, &b, &e);
            CHECK(b <= e && e <= nt, "share [%u, %u) of %u tiles", b, e, nt);
            // the direct launch of np frames: workgroup wg < dg takes [wg * dper, wg * dper + dper), cut at nt
            uint32_t db = 0, de = 0;
            if (np && wg < dg) {
                db = wg * dper;
                de = db + dper < nt ? db + dper : nt;
            }
            if (b < e || db < de)
                CHECK(b == db && e == de, "n_max %u ncu %u n %u piece %u wg %u: [%u, %u) direct [%u, %u)", n_max, ncu, n,
                      launches, wg, b, e, db, de);
            for (uint32_t t = b; t < e; ++t) {
                CHECK(t0 + t < ntiles, "tile %u past the batch's %u", t0 + t, ntiles);
                CHECK(!seen[t0 + t], "n_max %u ncu %u n %u: tile %u twice", n_max, ncu, n, t0 + t);
                seen[t0 + t] = 1;
            }
            ++shares;
        }
        if (np) CHECK(dg <= grid, "the direct launch has %u workgroups, the indirect one %u", dg, grid);
    }
    CHECK(launches == pieces && sum_len == n_max, "n_max %u: %u launches for %u pieces", n_max, launches, pieces);
    for (uint32_t t = 0; t < ntiles; ++t) CHECK(seen[t], "n_max %u ncu %u n %u: tile %u missing", n_max, ncu, n, t);
    return shares;
}

// A small batch's sub-tiles (echo_launch: n <= XSK_GPU_LOWLAT_MAX; `tile` 0 or the zerocopy context's, grid_force 0 or
// the tests' and tools' workgroup count): live frames per tile a multiple of 4 in [4, 64], the launch covers the batch,
// every workgroup has a tile, and an unforced grid's partial rows fit the workspace the caller was told to bring.
static void check_small_tiling(void) {
    const uint32_t tiles[] = {0, 4, 8, 64}, forces[] = {0, 1, 3, 16};
    for (uint32_t n = 1; n <= 1024; ++n)
        for (uint32_t tile : tiles)
            for (uint32_t gf : forces) {
                uint32_t tl = 0, per = 0, grid = 0;
                echo6_small_tiling(n, tile, gf, &tl, &per, &grid);
                CHECK(tl >= 4 && tl <= 64 && tl % 4 == 0, "n %u tile %u force %u: tl %u", n, tile, gf, tl);
                CHECK((uint64_t)grid * per * tl >= n, "n %u tile %u force %u: %u x %u x %u frames", n, tile, gf, grid,
                      per, tl);
                const uint32_t nt = (n + tl - 1) / tl;
                CHECK(grid >= 1 && per >= 1 && (uint64_t)(grid - 1) * per < nt,
                      "n %u tile %u force %u: workgroup %u of %u x %u tiles has none of %u", n, tile, gf, grid - 1, grid,
                      per, nt);
                if (gf == 0)
                    CHECK(grid <= echo6_workspace_rows(n), "n %u tile %u: %u workgroups, %u workspace rows", n, tile,
                          grid, echo6_workspace_rows(n));
            }
}

int main(void) {
    const uint32_t n_maxes[] = {1, 64, 65, 1024, 1025, 16385, (1u << 21) + 64};
    const uint32_t ncus[] = {1, 16, 256};
    std::vector<uint8_t> seen;
    uint64_t shares = 0, cases = 0;
    for (uint32_t n_max : n_maxes) {
        for (uint32_t ncu : ncus) {
            const uint32_t fixed[] = {0, 1, 63, 64, 65, n_max - 1, n_max};
            for (uint32_t n : fixed) {
                if (n > n_max) continue;
                shares += check_one(n_max, ncu, n, seen);
                ++cases;
            }
            for (int k = 0; k < 1000; ++k) {
                shares += check_one(n_max, ncu, rnd(n_max), seen);
                ++cases;
            }
        }
    }
    // the piece rule by hand: 256 CUs, 128 tiles (4 rounds) per workgroup is one launch, one tile more is
    // 5 rounds -> ceil(5 / 2) = 3 launches
    uint32_t pt = 0;
    CHECK(echo6_pieces(1u << 21, 256, &pt) == 1 && pt == 32768, "2^21 frames on 256 CUs: one launch");
    CHECK(echo6_pieces((1u << 21) + 64, 256, &pt) == 3 && pt == 10923, "2^21 + 64 frames on 256 CUs: three launches");
    CHECK(echo6_max_grid(0xFFFFFF00u, 256) == 256 && ind_ntiles(0xFFFFFF00u) == 0x3FFFFFCu, "XSK_GPU_MAX_BATCH");
    check_small_tiling();
    printf("indirect geometry ok: %llu cases, %llu shares\n", (unsigned long long)cases, (unsigned long long)shares);
    return 0;
}
