// The host-side arithmetic of xsk_gpu_rx_fused_loop_dev()'s kernel compiled for the host: the
// one-workgroup steering partition of xsknet_amd/csrc/xsk_steer.h (st1_port_total, st1_lower_waves, st1_slot) replayed
// lane by lane -- 16 waves of 64 lanes, a wave's count row and every lane's rank as wave_ranks()'s ballots leave them
// -- and the packed ring form of xsknet_amd/csrc/xsk_ring_pack.h.  The REDIRECT descriptors go into a heap array of
// exactly `total` entries and the offsets into one of exactly n_ports + 1 words; the test builds this file with
// -fsanitize=address,undefined, so an index one past an array's end is a failure here, not a stray store on a device.
// Asserted: every slot is stored exactly once, no store falls outside, the result equals a stable partition by port
// computed with std::stable_sort, and d_off equals the prefix counts.
//
// n in {0, 1, 63, 64, 65, 1023, 1024}; n_ports in {1, 2, 3, 64}; all frames on one port, round-robin, one frame per
// port, nothing redirected, a fixed-seed random assignment (a third of the frames not redirected).  The packed form:
// sizes 1, 2, 2^31 and every power of two between, pointers with bit 47 set, the absent ring, and what pk_packable()
// refuses.  Stand-alone: prints "loop fused ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/xsk_gpu.h"
#include "../../xsknet_amd/csrc/xsk_ring_pack.h"
#include "../../xsknet_amd/csrc/xsk_steer.h"

#define CHECK(c, ...)                     \
    do {                                  \
        if (!(c)) {                       \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            exit(1);                      \
        }                                 \
    } while (0)

using namespace xskgpu;

static_assert(kSt1Frames == XSK_GPU_LOWLAT_MAX && kSt1Waves == 16 && kStWave == 64, "the header's constants");

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {  // xorshift64*
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}

struct Frame {
    bool redirect;
    uint32_t port;
    uint64_t id;  // stands for the descriptor
};

// The kernel's steering stage over n <= 1024 frames, a lane per frame.  red[i] / port[i] for i >= n: not redirected.
static void replay(const std::vector<Frame>& f, uint32_t n_ports) {
    const uint32_t n = (uint32_t)f.size();
    CHECK(n <= kSt1Frames, "n");
    // wave_ranks(): the wave's count of every port present, and every lane's rank among the lower lanes of its port
    uint32_t(*cnt)[kStMaxPorts] = (uint32_t(*)[kStMaxPorts])calloc(kSt1Waves, sizeof(*cnt));
    std::vector<uint32_t> rank(kSt1Frames, 0);
    for (uint32_t t = 0; t < kSt1Frames; ++t) {
        if (t >= n || !f[t].redirect) continue;
        const uint32_t w = t / kStWave;
        for (uint32_t l = w * kStWave; l < t; ++l)
            if (l < n && f[l].redirect && f[l].port == f[t].port) ++rank[t];
        ++cnt[w][f[t].port];
    }
    // a lane per port: the column sums and their exclusive prefix
    uint32_t* off = (uint32_t*)malloc((n_ports + 1u) * sizeof(uint32_t));  // exactly n_ports + 1 words
    uint32_t base[kStMaxPorts];
    uint32_t run = 0;
    for (uint32_t p = 0; p < kStMaxPorts; ++p) {
        const uint32_t tot = p < n_ports ? st1_port_total(cnt, p) : 0u;
        base[p] = run;
        if (p < n_ports) off[p] = run;
        run += tot;
        if (p == n_ports - 1u) off[n_ports] = run;
    }
    const uint32_t total = off[n_ports];
    uint64_t* out = (uint64_t*)malloc(total * sizeof(uint64_t) + (total ? 0 : 1));  // exactly `total` entries
    std::vector<uint32_t> stored(total, 0);
    for (uint32_t t = 0; t < kSt1Frames; ++t) {
        if (t >= n || !f[t].redirect) continue;
        const uint32_t slot = st1_slot(base[f[t].port], st1_lower_waves(cnt, t / kStWave, f[t].port), rank[t]);
        CHECK(slot < total, "slot %u outside [0, %u)", slot, total);
        out[slot] = f[t].id;  // (ASan: an index past the array's end stops here)
        ++stored[slot];
    }
    for (uint32_t s = 0; s < total; ++s) CHECK(stored[s] == 1, "slot %u stored %u times", s, stored[s]);
    // the stable partition by port, and the prefix counts
    std::vector<Frame> want;
    for (const Frame& x : f)
        if (x.redirect) want.push_back(x);
    std::stable_sort(want.begin(), want.end(), [](const Frame& a, const Frame& b) { return a.port < b.port; });
    CHECK(want.size() == total, "total %u, want %zu", total, want.size());
    for (uint32_t s = 0; s < total; ++s) CHECK(out[s] == want[s].id, "slot %u holds %llu", s, (unsigned long long)out[s]);
    uint32_t before = 0;
    for (uint32_t p = 0; p <= n_ports; ++p) {
        CHECK(off[p] == before, "d_off[%u] = %u, want %u", p, off[p], before);
        if (p < n_ports)
            for (const Frame& x : want) before += x.port == p ? 1u : 0u;
    }
    free(out);
    free(off);
    free(cnt);
}

static void steer_cases() {
    const uint32_t ns[] = {0, 1, 63, 64, 65, 1023, 1024}, ports[] = {1, 2, 3, 64};
    for (uint32_t n : ns)
        for (uint32_t np : ports)
            for (int kind = 0; kind < 5; ++kind) {
                std::vector<Frame> f(n);
                for (uint32_t i = 0; i < n; ++i) {
                    f[i].id = 0x1000 + i;
                    f[i].redirect = true;
                    switch (kind) {
                        case 0: f[i].port = np - 1u; break;                              // all frames on one port
                        case 1: f[i].port = i % np; break;                               // round-robin
                        case 2: f[i].port = i % np; f[i].redirect = i < np; break;       // one frame per port
                        case 3: f[i].port = i % np; f[i].redirect = false; break;        // nothing redirected
                        default: f[i].port = (uint32_t)(rnd64() % np); f[i].redirect = rnd64() % 3 != 0; break;
                    }
                }
                replay(f, np);
            }
}

static void pack_cases() {
    const uint64_t ptrs[] = {0x10ull, 0x7F0012345670ull, (1ull << 47) | 0x123456789ABCull, (1ull << 47) | 0xFFFFFFFFFFF0ull,
                             (1ull << 55) | 0x40ull, (1ull << 56) - 16u};
    for (uint32_t l = 0; l <= kPkMaxLog2; ++l) {
        const uint32_t size = 1u << l;  // 1, 2, ..., 2^31
        for (uint64_t a : ptrs)
            for (uint64_t b : ptrs) {
                const uint64_t prod = a + 4u, cons = b + 8u, ring = a ^ (b & 0xFFF0u);
                CHECK(pk_packable(ring, size), "packable");
                const UnpackedRing u = pk_unpack(pk_pack(prod, cons, ring, size));
                CHECK(u.prod == prod && u.cons == cons && u.ring == ring && u.size == size, "round trip at 2^%u", l);
            }
    }
    const UnpackedRing absent = pk_unpack(pk_pack(0u, 0u, 0u, 1u));
    CHECK(absent.prod == 0 && absent.cons == 0 && absent.ring == 0 && absent.size == 1, "the absent ring");
    CHECK(!pk_packable(0x10u, 0u) && !pk_packable(0x10u, 3u) && !pk_packable(0x10u, 0x80000001u), "sizes refused");
    CHECK(!pk_packable(1ull << 56, 8u) && !pk_packable(~0ull, 8u) && pk_packable((1ull << 56) - 8u, 8u), "pointers refused");
    // 132 packed rings, the pool and the scalars stay inside an argument segment of 4096 B with 256 B of hidden arguments
    static_assert(sizeof(PackedRing) == 24 && 132u * sizeof(PackedRing) + 256u + 512u <= 4096u, "the kernel arguments");
}

int main() {
    steer_cases();
    pack_cases();
    printf("loop fused ok\n");
    return 0;
}
