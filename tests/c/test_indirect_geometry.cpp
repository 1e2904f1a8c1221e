// The launch geometry of xsk_gpu_echo_dev_indirect (xsknet_amd/csrc/xsk_echo_indirect.h) compiled for the host: for
// launches sized from a bound n_max, and every count n <= n_max the kernels may read, the shares the workgroups of all
// pieces work out for themselves partition the tiles of n -- none twice, none missing -- and within one launch each
// workgroup's share is the one the direct launch of that many frames gives it (echo6_geometry, transcribed below from
// xsknet_amd/csrc/xsk_echo_device.h, which is device code).  Stand-alone: prints "indirect geometry ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../xsknet_amd/csrc/xsk_echo_indirect.h"

using namespace xskgpu;

static void direct_geometry(uint32_t n, uint32_t num_cu, uint32_t* grid, uint32_t* tiles_per_wg) {
    const uint32_t ntiles = (n + 64 - 1) / 64;
    uint32_t g = num_cu < 1 ? 1 : num_cu;
    if (g > ntiles) g = ntiles < 1 ? 1 : ntiles;
    const uint32_t per = (ntiles + g - 1) / g;
    *tiles_per_wg = per < 1 ? 1 : per;
    *grid = (ntiles + *tiles_per_wg - 1) / *tiles_per_wg;
    if (*grid < 1) *grid = 1;
}

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
    const uint32_t pieces = ind_pieces(n_max, ncu, &piece_tiles);
    CHECK(piece_tiles >= 1 && (uint64_t)pieces * piece_tiles >= ntiles_max, "pieces do not cover n_max %u", n_max);
    seen.assign(ntiles_max + 1, 0);
    uint64_t shares = 0;
    uint32_t launches = 0, sum_len = 0;
    for (uint32_t t0 = 0; t0 < ntiles_max; t0 += piece_tiles, ++launches) {  // the host's loop (xsk_echo_indirect.hip)
        const uint32_t i0 = t0 * 64;
        const uint64_t cap = (uint64_t)piece_tiles * 64;
        const uint32_t len = (uint32_t)(n_max - i0 < cap ? n_max - i0 : cap);
        sum_len += len;
        const uint32_t grid = ind_grid(len, ncu);
        CHECK(grid >= 1 && grid <= ncu && grid <= ind_ntiles(len), "grid %u for len %u ncu %u", grid, len, ncu);
        const uint32_t np = ind_piece_n(n, i0, len);  // the kernel's prologue
        CHECK(np <= len && (n <= i0 ? np == 0 : np == (n - i0 < len ? n - i0 : len)), "piece_n");
        uint32_t dg = 0, dper = 0;
        direct_geometry(np, ncu, &dg, &dper);
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
    CHECK(ind_pieces(1u << 21, 256, &pt) == 1 && pt == 32768, "2^21 frames on 256 CUs: one launch");
    CHECK(ind_pieces((1u << 21) + 64, 256, &pt) == 3 && pt == 10923, "2^21 + 64 frames on 256 CUs: three launches");
    CHECK(ind_grid(0xFFFFFF00u, 256) == 256 && ind_ntiles(0xFFFFFF00u) == 0x3FFFFFCu, "XSK_GPU_MAX_BATCH");
    printf("indirect geometry ok: %llu cases, %llu shares\n", (unsigned long long)cases, (unsigned long long)shares);
    return 0;
}
