// The arithmetic of xsk_gpu_egress_dev() (xsknet_amd/csrc/xsk_egress.h) compiled for the host: both paths of
// xsk_egress.hip replayed thread by thread with the header's functions -- the one-workgroup path (wave ballots, sixteen
// counts, prefix, slot) and the three-stage path (per-workgroup counts -> the 1024-thread scan over runs -> per-lane
// slot) -- and compared with the sequential loop of xsk_gpu__rx_emit() (xsk_gpu_rx.c).  Every array is a heap
// allocation of exactly its size: descriptors and verdicts n entries (nothing at an index >= n may be read), the TX
// list n_tx, the free list n_free, the workspace eg_workspace_bytes(n_max); the test builds this file with
// -fsanitize=address,undefined, so a slot one past a list's end is a failure here, not a stray store on a device.
//
// n_max in {1, 63, 64, 65, 1023, 1024, 1025, 1279, 1281, 262147, 2^20 + 1}; n in {0, 1, n_max - 1, n_max} crossed with
// every reply pattern (all, none, alternating, random, only lane 0 / lane 63 of each wave, only the last workgroup) and
// every room (0, 1, 37, R - 1, R, R + 1, unlimited); then 300 random n per size, crossed the same way up to n_max =
// 1281, and for the two large sizes each with one pattern and one room, taken in turn.  A word above n_max in *d_n
// (the clamp) and d_n == NULL are run for every size.  Stand-alone: prints "egress slots ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/xsk_gpu.h"
#include "../../xsknet_amd/csrc/xsk_egress.h"
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

struct Result {
    xsk_gpu_desc* tx;
    uint64_t* fr;
    EgCounts c;
    uint64_t lost_packets, lost_bytes, atomic_pairs;
};

static unsigned popc(uint64_t m) { return (unsigned)__builtin_popcountll(m); }

// ---- xsk_gpu__rx_emit()'s loop, with `room` as the slots the ring gave ----
static void sequential(const xsk_gpu_desc* descs, const uint8_t* verdict, uint32_t n, uint32_t ring_free, Result* r,
                       size_t cap_tx, size_t cap_free) {
    uint32_t nrep = 0;
    for (uint32_t i = 0; i < n; i++) nrep += verdict[i] == XSK_GPU_TX_REPLY;
    uint32_t room = ring_free < nrep ? ring_free : nrep, sent = 0, freed = 0, tx_full = 0;
    uint64_t lost = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (verdict[i] == XSK_GPU_TX_REPLY && sent < room) {
            CHECK(sent < cap_tx, "reference tx overflow");
            r->tx[sent].addr = descs[i].addr;
            r->tx[sent].len = descs[i].len;
            r->tx[sent].options = 0;
            sent++;
        } else {
            if (verdict[i] == XSK_GPU_TX_REPLY) {
                tx_full++;
                lost += descs[i].len;
            }
            CHECK(freed < cap_free, "reference free overflow");
            r->fr[freed++] = descs[i].addr;
        }
    }
    r->c.n = n;
    r->c.n_tx = sent;
    r->c.n_tx_full = tx_full;
    r->c.n_free = freed;
    r->lost_packets = tx_full;
    r->lost_bytes = lost;
}

// One workgroup's lanes behind their ballots: the part the two scatter kernels share.  `off` = replies below the
// workgroup, i0 = its first frame, threads = its size.
static void scatter_wg(const xsk_gpu_desc* descs, const uint8_t* verdict, uint32_t n, uint32_t room, uint32_t i0,
                       uint32_t threads, uint32_t off, Result* r, uint32_t* wg_total) {
    const uint32_t nw = threads / kEgWave;
    uint64_t m[kEgSmallThreads / kEgWave];
    uint32_t s_w[kEgSmallThreads / kEgWave];
    for (uint32_t w = 0; w < nw; ++w) {
        m[w] = 0;
        for (uint32_t lane = 0; lane < kEgWave; ++lane) {
            const uint64_t i = (uint64_t)i0 + w * kEgWave + lane;
            if (i < n && verdict[i] == XSK_GPU_TX_REPLY) m[w] |= 1ull << lane;  // (nothing at an index >= n is read)
        }
        s_w[w] = popc(m[w]);
    }
    uint32_t total = off;
    for (uint32_t w = 0; w < nw; ++w) total += s_w[w];
    uint64_t lost_p = 0, lost_b = 0;
    for (uint32_t w = 0; w < nw; ++w) {
        uint32_t base = off;
        for (uint32_t k = 0; k < w; ++k) base += s_w[k];
        for (uint32_t lane = 0; lane < kEgWave; ++lane) {
            const uint64_t i64 = (uint64_t)i0 + w * kEgWave + lane;
            if (i64 >= n) continue;
            const uint32_t i = (uint32_t)i64;
            const bool reply = (m[w] >> lane) & 1u;
            const uint32_t r_below = base + popc(m[w] & ((1ull << lane) - 1ull));
            const EgSlot s = eg_slot(reply, i, r_below, room);
            if (s.tx) {  // (exact heap arrays: an out-of-range slot is an AddressSanitizer report)
                r->tx[s.slot].addr = descs[i].addr;
                r->tx[s.slot].len = descs[i].len;
                r->tx[s.slot].options = 0;
            } else {
                r->fr[s.slot] = descs[i].addr;
            }
            if (eg_unsent(reply, r_below, room)) {
                lost_p++;
                lost_b += descs[i].len;
            }
        }
    }
    if (total > off && total > room) {  // the kernels' workgroup-uniform condition for the stats pass
        CHECK(lost_p > 0, "stats pass taken with nothing to take back");
        r->atomic_pairs++;
    } else {
        CHECK(lost_p == 0, "a reply past the room outside the stats pass");
    }
    r->lost_packets += lost_p;
    r->lost_bytes += lost_b;
    *wg_total = total;
}

// ---- the device paths, as xsk_gpu_egress_dev() dispatches them ----
static void device_paths(const xsk_gpu_desc* descs, const uint8_t* verdict, bool have_n, uint32_t word_n,
                         uint32_t n_max, bool have_room, uint32_t word_room, Result* r) {
    const uint32_t n = eg_count(have_n, word_n, n_max), room = eg_room(have_room, word_room);
    r->lost_packets = r->lost_bytes = r->atomic_pairs = 0;
    if (n_max <= kEgSmallMax) {
        CHECK(eg_workspace_bytes(n_max) == 0, "the small path has no workspace");
        uint32_t total = 0;
        scatter_wg(descs, verdict, n, room, 0, kEgSmallThreads, 0, r, &total);
        r->c = eg_counts(n, total, room);
        return;
    }
    const uint32_t nwg = cp_nwg(n_max);
    CHECK((uint64_t)nwg * kEgFrames >= n_max && (uint64_t)(nwg - 1) * kEgFrames < n_max, "nwg");
    CHECK(eg_workspace_bytes(n_max) == (size_t)nwg * 4, "workspace");
    uint32_t* ws = (uint32_t*)malloc(eg_workspace_bytes(n_max));
    CHECK(ws, "malloc");
    uint64_t covered = 0;
    for (uint32_t wg = 0; wg < nwg; ++wg) {  // stage 1
        const uint32_t frames = eg_wg_frames(n, wg);
        covered += frames;
        uint32_t c = 0;
        for (uint32_t t = 0; t < frames; ++t) c += verdict[(size_t)wg * kEgFrames + t] == XSK_GPU_TX_REPLY;
        ws[wg] = c;
    }
    CHECK(covered == n, "the workgroups' frames do not add up to n");
    // stage 2: thread t owns a run; the runs partition [0, nwg)
    const uint32_t r_total = replay_scan_cells(ws, nwg, replay_put_before);
    r->c = eg_counts(n, r_total, room);
    for (uint32_t wg = 0; wg < nwg; ++wg) {  // stage 3
        if (eg_wg_frames(n, wg) == 0) continue;
        uint32_t total = 0;
        scatter_wg(descs, verdict, n, room, wg * kEgFrames, kEgFrames, ws[wg], r, &total);
        CHECK(total == (wg + 1 < nwg ? ws[wg + 1] : r_total), "offsets are not the running reply count");
    }
    free(ws);
}

enum { P_ALL, P_NONE, P_ALT, P_RANDOM, P_LANE0, P_LANE63, P_LAST_WG, P_COUNT };
enum { R_0, R_1, R_37, R_RM1, R_R, R_RP1, R_UNLIMITED, R_COUNT };

static void fill_verdicts(uint8_t* v, uint32_t n, int pattern) {
    static const uint8_t other[] = {1, 2, 3, 4, 5, 6, 7, 8, 0x80, 0xEE, 0xFF};
    const uint32_t last = n ? ((n - 1) / kEgFrames) * kEgFrames : 0;
    for (uint32_t i = 0; i < n; ++i) {
        bool reply = false;
        switch (pattern) {
            case P_ALL: reply = true; break;
            case P_NONE: reply = false; break;
            case P_ALT: reply = !(i & 1u); break;
            case P_RANDOM: reply = rnd64() >> 63; break;
            case P_LANE0: reply = i % 64 == 0; break;
            case P_LANE63: reply = i % 64 == 63; break;
            case P_LAST_WG: reply = i >= last; break;
        }
        v[i] = reply ? (uint8_t)XSK_GPU_TX_REPLY : other[rnd(sizeof(other) - 1)];
    }
}

static uint64_t g_cases = 0;

// One (n_max, word in *d_n or NULL, pattern, room kind): inputs of exactly n entries, outputs of exactly the
// reference's counts.
static void one_case(uint32_t n_max, bool have_n, uint32_t word_n, int pattern, int room_kind) {
    const uint32_t n = eg_count(have_n, word_n, n_max);
    CHECK(n <= n_max && (!have_n || n == (word_n < n_max ? word_n : n_max)), "clamp");
    xsk_gpu_desc* descs = exact<xsk_gpu_desc>(n);
    uint8_t* verdict = exact<uint8_t>(n);
    fill_verdicts(verdict, n, pattern);
    uint32_t R = 0;
    for (uint32_t i = 0; i < n; ++i) {
        descs[i].addr = (uint64_t)i * 2048 + rnd(255);
        descs[i].len = 14 + rnd(1500);
        descs[i].options = 1 + rnd(0xFFFFFFF0u);  // never 0: a copied descriptor shows
        R += verdict[i] == XSK_GPU_TX_REPLY;
    }
    bool have_room = true;
    uint32_t word_room = 0;
    switch (room_kind) {
        case R_0: word_room = 0; break;
        case R_1: word_room = 1; break;
        case R_37: word_room = 37; break;
        case R_RM1: word_room = R ? R - 1 : 0; break;
        case R_R: word_room = R; break;
        case R_RP1: word_room = R + 1; break;
        case R_UNLIMITED: have_room = false; break;
    }
    const uint32_t room = eg_room(have_room, word_room);
    const uint32_t n_tx = R < room ? R : room, n_free = n - n_tx;
    Result ref, got;
    ref.tx = exact<xsk_gpu_desc>(n_tx);
    ref.fr = exact<uint64_t>(n_free);
    got.tx = exact<xsk_gpu_desc>(n_tx);
    got.fr = exact<uint64_t>(n_free);
    if (n_tx) memset(got.tx, 0xEE, (size_t)n_tx * sizeof(xsk_gpu_desc));
    if (n_free) memset(got.fr, 0xEE, (size_t)n_free * sizeof(uint64_t));
    sequential(descs, verdict, n, room, &ref, n_tx, n_free);
    device_paths(descs, verdict, have_n, word_n, n_max, have_room, word_room, &got);
    CHECK(ref.c.n == n && ref.c.n_tx == n_tx && ref.c.n_free == n_free && ref.c.n_tx_full == R - n_tx, "reference");
    CHECK(got.c.n == ref.c.n && got.c.n_tx == ref.c.n_tx && got.c.n_tx_full == ref.c.n_tx_full &&
              got.c.n_free == ref.c.n_free,
          "counts: n_max %u n %u pattern %d room %u: got %u %u %u %u, want %u %u %u %u", n_max, n, pattern, room, got.c.n,
          got.c.n_tx, got.c.n_tx_full, got.c.n_free, ref.c.n, ref.c.n_tx, ref.c.n_tx_full, ref.c.n_free);
    CHECK(!n_tx || !memcmp(got.tx, ref.tx, (size_t)n_tx * sizeof(xsk_gpu_desc)), "tx list: n_max %u n %u pattern %d room %u",
          n_max, n, pattern, room);
    CHECK(!n_free || !memcmp(got.fr, ref.fr, (size_t)n_free * sizeof(uint64_t)), "free list: n_max %u n %u pattern %d room %u",
          n_max, n, pattern, room);
    CHECK(got.lost_packets == ref.lost_packets && got.lost_bytes == ref.lost_bytes && got.lost_packets == got.c.n_tx_full,
          "counters: n_max %u n %u pattern %d room %u", n_max, n, pattern, room);
    CHECK(got.c.n_tx_full || !got.atomic_pairs, "atomics issued with n_tx_full == 0");
    CHECK(got.atomic_pairs <= (n_max <= kEgSmallMax ? 1u : cp_nwg(n_max)), "more than one pair per workgroup");
    free(descs);
    free(verdict);
    free(ref.tx);
    free(ref.fr);
    free(got.tx);
    free(got.fr);
    ++g_cases;
}

// cp_scan_run against the expression the filter's scan used before it took cp_scan_run -- b = t * per, e = min(b + per,
// nwg) in 32 bits, the run taken when b < e -- at every thread: the same cells, and a partition of [0, nwg).  0xFFFFFF is
// cp_nwg(XSK_GPU_MAX_BATCH); with per <= 16384 nothing in the 32-bit form wraps.
static void scan_runs_agree() {
    const uint32_t nwgs[] = {0, 1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 65536, 0xFFFFFF};
    static_assert(XSK_GPU_MAX_BATCH / kCpFrames == 0xFFFFFF && XSK_GPU_MAX_BATCH % kCpFrames == 0, "the largest grid");
    for (uint32_t nwg : nwgs) {
        const uint32_t per = (nwg + 1023u) / 1024u;
        uint32_t next = 0;
        for (uint32_t t = 0; t < kCpScanThreads; ++t) {
            uint32_t b, e;
            cp_scan_run(nwg, t, &b, &e);
            CHECK(b == next && b <= e && e <= nwg, "scan runs: nwg %u thread %u", nwg, t);
            next = e;
            const uint32_t ob = t * per, oe = ob + per < nwg ? ob + per : nwg;
            CHECK(ob < oe ? b == ob && e == oe : b == e, "nwg %u thread %u: [%u, %u), formerly [%u, %u) if not empty", nwg,
                  t, b, e, ob, oe);
        }
        CHECK(next == nwg && per <= 16384u, "scan runs do not cover [0, %u)", nwg);
    }
}

int main(void) {
    static_assert(sizeof(xsk_gpu_egress_counts) == sizeof(EgCounts), "counts layout");
    static_assert(kEgSmallMax == XSK_GPU_LOWLAT_MAX, "small path bound");
    const uint32_t sizes[] = {1, 63, 64, 65, 1023, 1024, 1025, 1279, 1281, 262147, (1u << 20) + 1};
    for (uint32_t n_max : sizes) {
        const uint32_t fixed[] = {0, 1, n_max - 1, n_max};
        for (uint32_t n : fixed)
            for (int p = 0; p < P_COUNT; ++p)
                for (int rk = 0; rk < R_COUNT; ++rk) one_case(n_max, true, n, p, rk);
        for (int rk = 0; rk < R_COUNT; ++rk) {
            one_case(n_max, true, n_max + 5, P_RANDOM, rk);  // the clamp
            one_case(n_max, false, 0, P_RANDOM, rk);         // d_n == NULL
        }
        const bool cross = n_max <= 2048;
        for (uint32_t k = 0; k < 300; ++k) {
            const uint32_t n = rnd(n_max);
            if (cross) {
                for (int p = 0; p < P_COUNT; ++p)
                    for (int rk = 0; rk < R_COUNT; ++rk) one_case(n_max, true, n, p, rk);
            } else {
                one_case(n_max, true, n, (int)(k % P_COUNT), (int)((k / P_COUNT) % R_COUNT));
            }
        }
    }
    // the largest bound the call accepts: the sizes stay inside 32 bits, the scan's runs inside the counts
    const uint32_t big = XSK_GPU_MAX_BATCH, nwg = cp_nwg(big);
    CHECK((uint64_t)nwg * kEgFrames >= big && eg_workspace_bytes(big) == (size_t)nwg * 4, "largest bound");
    uint32_t b, e;
    cp_scan_run(nwg, kEgScanThreads - 1, &b, &e);
    CHECK(e == nwg && b <= e, "largest bound: the last run");
    CHECK(eg_wg_frames(big, nwg - 1) == big - (nwg - 1) * kEgFrames && eg_wg_frames(big, nwg) == 0, "largest bound");
    scan_runs_agree();
    printf("egress slots ok (%llu cases)\n", (unsigned long long)g_cases);
    return 0;
}
