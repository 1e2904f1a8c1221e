// xsk_steer.h (xsknet_amd/csrc) compiled for the host: the per-frame decision, the table search and the partition
// arithmetic of xsk_gpu_steer_dev().  Every array is a heap allocation of exactly its size and the test builds this file
// with -fsanitize=address,undefined, so a byte read past a frame's end, a probe outside a table or a slot past the
// list's end is a failure here, not a stray access on a device.
//
//   1. Frames that end flush with their allocation (the UMEM is the frame): the 34-byte IPv4 echo request, the IPv6
//      frame of l3 + 40 and of l3 + 48 bytes, each with 0, 1 and 2 tags, and every shorter cut of them, under every
//      option word; the action against classify_wire_one() / the reference's rules under the degenerate map, and the
//      port against the table.
//   2. Tables of 0, 1, 2, 1023 and 1024 entries, staged into exactly n * 6 words: every key present is found, keys
//      between them miss; the same tables unsorted (not prepared) are searched for the bounds alone.
//   3. The three stages replayed sequentially -- per-wave ballots and counts, the 1024-thread scan of every row over
//      runs with the row's total in its first cell, the ports' first slots, the slot -- for n around the wave and
//      workgroup sizes and at 262145 frames (1025 workgroups: a scan thread owns two cells), against a stable sort by
//      port.
// Stand-alone: prints "steer ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/xsk_gpu.h"
#include "../../xsknet_amd/csrc/xsk_steer.h"
#include "compact_replay.h"  // CHECK, and the scan stage replayed

using namespace xskgpu;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {  // xorshift64*
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}
static uint32_t rnd(uint32_t bound) { return (uint32_t)((rnd64() >> 33) % ((uint64_t)bound + 1)); }  // [0, bound]

template <class T>
static T* exact(size_t count) {  // exactly count entries (count == 0: a pointer to nothing)
    T* p = (T*)malloc(count * sizeof(T));
    CHECK(p || !count, "malloc");
    return p;
}

static xsk_gpu_steer_entry entry(int family, const uint8_t* addr, uint8_t port) {
    xsk_gpu_steer_entry e;
    memset(&e, 0, sizeof(e));
    memcpy(e.addr, addr, family == 4 ? 4 : 16);
    e.family = (uint8_t)family;
    e.port = port;
    return e;
}

static bool entry_less(const xsk_gpu_steer_entry& a, const xsk_gpu_steer_entry& b) {
    if (a.family != b.family) return a.family < b.family;
    return memcmp(a.addr, b.addr, 16) < 0;
}

// The staged form of a table, in exactly n * kStEntryWords words.
static uint32_t* stage(const std::vector<xsk_gpu_steer_entry>& t) {
    uint32_t* s = exact<uint32_t>(t.size() * kStEntryWords);
    for (size_t i = 0; i < t.size(); ++i) st_stage_entry(&t[i], s + i * kStEntryWords);
    return s;
}

// ---- 1. frames ----
static const uint8_t kDst4[4] = {10, 0, 0, 2}, kDst6[16] = {0x20, 0x01, 0x0d, 0xb8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xfe};

// An ICMP / ICMPv6 echo request behind `tags` VLAN tags, l3 + 48 bytes at least (IPv4: padded).
static std::vector<uint8_t> frame(int family, int tags) {
    std::vector<uint8_t> f(12, 0x02);
    static const uint8_t tpid[2][2] = {{0x88, 0xA8}, {0x81, 0x00}};
    for (int t = 0; t < tags; ++t) {
        const uint8_t* tp = tpid[tags == 1 ? 1 : t];
        f.insert(f.end(), {tp[0], tp[1], 0x00, 0x64});
    }
    if (family == 4) {
        f.insert(f.end(), {0x08, 0x00});
        const uint8_t ip[20] = {0x45, 0, 0, 28, 0x12, 0x34, 0x40, 0, 64, 1, 0, 0, 10, 0, 0, 1, 10, 0, 0, 2};
        f.insert(f.end(), ip, ip + 20);
        const uint8_t icmp[8] = {8, 0, 0, 0, 0x12, 0x34, 0, 7};
        f.insert(f.end(), icmp, icmp + 8);
        f.resize(f.size() + 20, 0);
    } else {
        f.insert(f.end(), {0x86, 0xDD});
        const uint8_t h[8] = {0x60, 0, 0, 0, 0, 8, 58, 64};
        f.insert(f.end(), h, h + 8);
        for (int k = 0; k < 16; ++k) f.push_back(k == 15 ? 1 : kDst6[k]);  // source
        f.insert(f.end(), kDst6, kDst6 + 16);
        const uint8_t icmp[8] = {128, 0, 0, 0, 0x12, 0x34, 0, 7};
        f.insert(f.end(), icmp, icmp + 8);
    }
    return f;
}

static uint32_t ref_rules(const uint8_t* p, uint32_t len) {  // xdp_sock_prog, src/kern/inner_xdp.c:35-60, bound
    if (len < 14) return XSK_GPU_XDP_DROP;
    if (p[12] != 0x08 || p[13] != 0x00) return XSK_GPU_XDP_PASS;
    if (len < 34) return XSK_GPU_XDP_DROP;
    if (p[23] != 1) return XSK_GPU_XDP_PASS;
    return XSK_GPU_XDP_REDIRECT;
}

static void test_frames() {
    std::vector<xsk_gpu_steer_entry> t = {entry(4, kDst4, 3), entry(6, kDst6, 9)};
    std::sort(t.begin(), t.end(), entry_less);
    uint32_t* tab = stage(t);
    const uint32_t words[] = {0u, 0x2u, 0x10u, 0x12u, 0x17u, 0x5u};
    unsigned redirected = 0, flush4 = 0, flush6 = 0;
    for (int family = 4; family <= 6; family += 2)
        for (int tags = 0; tags <= 2; ++tags) {
            const std::vector<uint8_t> full = frame(family, tags);
            const uint32_t l3 = 14 + 4 * tags;
            for (uint32_t len = 0; len <= full.size(); ++len) {
                uint8_t* um = exact<uint8_t>(len);  // the UMEM is the frame: it ends flush with the allocation
                if (len) memcpy(um, full.data(), len);
                const xsk_gpu_desc d = {0, len, 0};
                for (uint32_t opts : words) {
                    // the degenerate map is the filter
                    const uint32_t want = opts ? classify_wire_one(um, len, d, opts, 1) : ref_rules(um, len);
                    const StVerdict v0 = st_steer_one(um, len, d, opts, nullptr, 0, 0, 1, 1ull);
                    CHECK(v0.act == want, "family %d tags %d len %u opts %#x: action %u, filter %u", family, tags, len,
                          opts, v0.act, want);
                    CHECK(v0.port == (want == XSK_GPU_XDP_REDIRECT ? 0u : kStPass), "port under the degenerate map");
                    const StVerdict u0 = st_steer_one(um, len, d, opts, nullptr, 0, 0, 1, 0ull);
                    CHECK(u0.act == (want == XSK_GPU_XDP_REDIRECT ? (uint32_t)XSK_GPU_XDP_DROP : want), "unbound");
                    // the table decides the port; an address it does not hold is left to the stack
                    const StVerdict v = st_steer_one(um, len, d, opts, tab, 2, kStPass, 16, ~0ull);
                    CHECK(v.act == want, "table: action");
                    CHECK(v.port == (want == XSK_GPU_XDP_REDIRECT ? (family == 4 ? 3u : 9u) : kStPass),
                          "family %d tags %d len %u opts %#x: port %u", family, tags, len, opts, v.port);
                    const StVerdict m = st_steer_one(um, len, d, opts, tab, 1, kStPass, 16, ~0ull);  // IPv4 entry only
                    if (want == XSK_GPU_XDP_REDIRECT && family == 6)
                        CHECK(m.act == XSK_GPU_XDP_PASS && m.port == kStPass, "a miss with the PASS default");
                    // port >= n_ports and an unbound port: DROP
                    const StVerdict hi = st_steer_one(um, len, d, opts, tab, 2, kStPass, 3, ~0ull);
                    const StVerdict ub = st_steer_one(um, len, d, opts, tab, 2, kStPass, 16, ~((1ull << 3) | (1ull << 9)));
                    if (want == XSK_GPU_XDP_REDIRECT) {
                        CHECK(hi.act == XSK_GPU_XDP_DROP && hi.port == kStPass, "port >= n_ports");
                        CHECK(ub.act == XSK_GPU_XDP_DROP && ub.port == kStPass, "unbound port");
                        ++redirected;
                        flush4 += family == 4 && len == l3 + 20;
                        flush6 += family == 6 && len == l3 + 48;
                    }
                    if (family == 6 && len == l3 + 40 && (opts & XSK_GPU_OPT_IPV6) && (tags == 0 || (opts & XSK_GPU_OPT_VLAN)))
                        CHECK(v.act == XSK_GPU_XDP_DROP, "the destination as the last sixteen bytes: rule 5, no lookup");
                }
                // a descriptor that leaves the UMEM by one byte
                const xsk_gpu_desc over = {0, len + 1, 0};
                for (uint32_t opts : words)
                    if (opts) CHECK(st_steer_one(um, len, over, opts, tab, 2, 0, 16, ~0ull).act == XSK_GPU_XDP_DROP, "rule 1");
                free(um);
            }
        }
    // opts == 0: 34 bytes of a longer frame inside the UMEM are enough (classify_one's rule), the destination its last four
    {
        const std::vector<uint8_t> full = frame(4, 0);
        uint8_t* um = exact<uint8_t>(34);
        memcpy(um, full.data(), 34);
        const xsk_gpu_desc d = {0, 1500, 0};
        const StVerdict v = st_steer_one(um, 34, d, 0, tab, 2, kStPass, 16, ~0ull);
        CHECK(v.act == XSK_GPU_XDP_REDIRECT && v.port == 3, "opts == 0, 34 bytes in the UMEM");
        free(um);
    }
    CHECK(redirected > 0 && flush4 >= 3 && flush6 >= 3, "conditions of the input: %u %u %u", redirected, flush4, flush6);
    free(tab);
}

// ---- 2. tables ----
static void test_tables() {
    const uint32_t sizes[] = {0, 1, 2, 1023, 1024};
    for (uint32_t n : sizes) {
        std::vector<xsk_gpu_steer_entry> t;
        for (uint32_t i = 0; i < n; ++i) {  // even counters are keys, odd ones lie between them
            uint8_t a[16] = {0};
            const uint32_t c = 2 * i + 2;
            const int family = i % 3 ? 6 : 4;
            a[0] = (uint8_t)(i % 5);
            a[2] = (uint8_t)(c >> 8);
            a[3] = (uint8_t)c;
            if (family == 6) a[15] = (uint8_t)(i * 7);
            t.push_back(entry(family, a, (uint8_t)(i % 64)));
        }
        std::vector<xsk_gpu_steer_entry> sorted = t;
        std::sort(sorted.begin(), sorted.end(), entry_less);
        uint32_t* tab = stage(sorted);
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t e[kStEntryWords];
            st_stage_entry(&t[i], e);
            CHECK(st_lookup(tab, n, e, kStPass) == t[i].port, "n %u: entry %u not found", n, i);
            e[1] ^= 1u;  // the odd counter: a key between two entries
            CHECK(st_lookup(tab, n, e, 77u) == 77u, "n %u: a key that is not there was found", n);
            e[1] ^= 1u;
            e[0] ^= 2u;  // the same address in the other family
            CHECK(st_lookup(tab, n, e, 77u) == 77u, "n %u: the family is part of the key", n);
        }
        const uint32_t below[5] = {0, 0, 0, 0, 0}, above[5] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        CHECK(st_lookup(tab, n, below, 77u) == 77u && st_lookup(tab, n, above, 77u) == 77u, "outside the table");
        free(tab);
        // not prepared: the insertion order above is not sorted (a[0] = i % 5 leads).  A search may miss; it may not
        // probe outside the n entries, and what it finds is an entry with that key.
        CHECK(n < 3 || !std::is_sorted(t.begin(), t.end(), entry_less), "the unprepared table is really unsorted");
        tab = stage(t);
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t e[kStEntryWords];
            st_stage_entry(&t[i], e);
            const uint32_t p = st_lookup(tab, n, e, kStPass);
            CHECK(p == kStPass || p == t[i].port, "n %u: an unprepared table gave a port of another key", n);
        }
        free(tab);
    }
}

// ---- 3. the partition ----
static unsigned popc(uint64_t m) { return (unsigned)__builtin_popcountll(m); }

// The wave's ballots of xsk_steer.hip: cnt[port] for every port present, rank[lane] among the lower lanes of its port.
static void wave(const uint8_t* red, const uint8_t* port, uint32_t lanes, uint32_t* cnt, uint32_t* rank) {
    uint64_t todo = 0;
    for (uint32_t l = 0; l < lanes; ++l) todo |= (uint64_t)red[l] << l;
    while (todo) {
        const uint32_t p = port[__builtin_ctzll(todo)];
        uint64_t m = 0;
        for (uint32_t l = 0; l < lanes; ++l) m |= (uint64_t)(red[l] && port[l] == p) << l;
        for (uint32_t l = 0; l < lanes; ++l)
            if ((m >> l) & 1) rank[l] = popc(m & ((1ull << l) - 1ull));
        cnt[p] = popc(m);
        todo &= ~m;
    }
}

static void partition_case(uint32_t n, uint32_t n_ports, int pattern) {
    uint8_t* red = exact<uint8_t>(n);
    uint8_t* port = exact<uint8_t>(n);
    xsk_gpu_desc* descs = exact<xsk_gpu_desc>(n);
    uint32_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t p;
        switch (pattern) {
            case 0: p = rnd(n_ports - 1); red[i] = rnd(3) != 0; break;          // random
            case 1: p = i % n_ports; red[i] = 1; break;                         // every lane another port, ascending
            case 2: p = (n_ports - 1) - i % n_ports; red[i] = 1; break;         // descending
            case 3: p = n_ports - 1; red[i] = 1; break;                         // one port only, the last
            default: p = (i / 7) % 2 ? 0 : n_ports - 1; red[i] = i % 5 != 0; break;  // nothing in the middle
        }
        port[i] = red[i] ? (uint8_t)p : (uint8_t)kStPass;
        descs[i] = xsk_gpu_desc{0x1000ull * i + 7, 60 + i % 1000, i};
        total += red[i];
    }
    const uint32_t nwg = cp_nwg(n), cells = st_cells(n_ports, nwg);
    CHECK(st_workspace_bytes(n, n_ports) == (size_t)cells * 4, "workspace");
    uint32_t* count = exact<uint32_t>(cells);
    uint32_t* off = exact<uint32_t>(n_ports + 1);
    uint32_t* rank = exact<uint32_t>(n);
    std::vector<uint32_t> wave_cnt((size_t)nwg * kStWaves * kStMaxPorts, 0u);
    // stage 1
    for (uint32_t wg = 0; wg < nwg; ++wg) {
        for (uint32_t w = 0; w < kStWaves; ++w) {
            const uint32_t i0 = wg * kStFrames + w * kStWave;
            if (i0 >= n) break;
            wave(red + i0, port + i0, std::min(kStWave, n - i0), &wave_cnt[((size_t)wg * kStWaves + w) * kStMaxPorts], rank + i0);
        }
        for (uint32_t p = 0; p < n_ports; ++p) {
            uint32_t c = 0;
            for (uint32_t w = 0; w < kStWaves; ++w) c += wave_cnt[((size_t)wg * kStWaves + w) * kStMaxPorts + p];
            count[st_cell(p, wg, nwg)] = c;
        }
    }
    // stage 2, a workgroup per row: thread t's run, the exclusive prefix of the runs before it; the total in cell 0
    for (uint32_t p = 0; p < n_ports; ++p) {
        uint32_t* row = count + st_cell(p, 0, nwg);
        uint32_t row_total = 0;
        for (uint32_t j = 0; j < nwg; ++j) row_total += row[j];
        CHECK(replay_scan_cells(row, nwg, st_scanned_cell) == row_total, "the row's total");
    }
    // stage 3's prologue: the totals -> the ports' first slots
    std::vector<uint32_t> base(n_ports);
    uint32_t run = 0;
    for (uint32_t p = 0; p < n_ports; ++p) {
        base[p] = off[p] = run;
        run += count[st_cell(p, 0, nwg)];
    }
    off[n_ports] = run;
    CHECK(run == total, "total");
    // stage 3 into a list of exactly `total` entries
    xsk_gpu_desc* out = exact<xsk_gpu_desc>(total);
    uint8_t* hit = exact<uint8_t>(total);
    if (total) memset(hit, 0, total);
    for (uint32_t i = 0; i < n; ++i) {
        if (!red[i]) continue;
        const uint32_t wg = i / kStFrames, w = (i % kStFrames) / kStWave;
        uint32_t lower = 0;
        for (uint32_t k = 0; k < w; ++k) lower += wave_cnt[((size_t)wg * kStWaves + k) * kStMaxPorts + port[i]];
        const uint32_t slot = st_slot(base[port[i]], st_cell_offset(wg, count[st_cell(port[i], wg, nwg)]), lower, rank[i]);
        CHECK(slot < total && !hit[slot], "slot %u of %u", slot, total);
        hit[slot] = 1;
        out[slot] = descs[i];
    }
    // a stable sort by port
    std::vector<uint32_t> order;
    for (uint32_t i = 0; i < n; ++i)
        if (red[i]) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return port[a] < port[b]; });
    for (uint32_t k = 0; k < total; ++k) CHECK(out[k].options == order[k], "n %u ports %u pattern %d: slot %u", n, n_ports, pattern, k);
    CHECK(off[0] == 0, "d_off[0]");
    for (uint32_t p = 0; p < n_ports; ++p) {
        CHECK(off[p] <= off[p + 1], "monotone");
        for (uint32_t k = off[p]; k < off[p + 1]; ++k) CHECK(port[out[k].options] == p, "group %u", p);
    }
    free(red); free(port); free(descs); free(count); free(off); free(rank); free(out); free(hit);
}

static void test_partition() {
    const uint32_t ns[] = {1, 63, 64, 65, 255, 256, 257, 1025, 4097};
    const uint32_t ports[] = {1, 2, 3, 64};
    for (uint32_t n : ns)
        for (uint32_t np : ports)
            for (int pattern = 0; pattern < 5; ++pattern) partition_case(n, np, pattern);
    // 1025 workgroups: the first batch at which a thread of a row's scan owns two cells
    CHECK(cp_scan_per(cp_nwg(262145)) == 2 && cp_scan_per(cp_nwg(262144)) == 1, "262145 frames");
    for (uint32_t np : {3u, 64u})
        for (int pattern = 0; pattern < 2; ++pattern) partition_case(262145, np, pattern);
    for (int k = 0; k < 200; ++k) partition_case(1 + rnd(3000), 1 + rnd(63), 0);
    CHECK(st_workspace_bytes(1u << 20, 64) == (size_t)1 << 20, "1 MiB at 1 M frames and 64 ports");
}

int main() {
    test_frames();
    test_tables();
    test_partition();
    printf("steer ok\n");
    return 0;
}
