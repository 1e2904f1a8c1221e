// xsk_unreach.h (xsknet_amd/csrc) compiled for the host: the per-frame decision, the two rewrites and the serve plan of
// xsk_gpu_unreach_dev() / xsk_gpu_unreach_serve_dev().  Every array is a heap allocation of exactly its size and the
// test builds this file with -fsanitize=address,undefined, so a byte read past a frame's end, a byte of the reply
// written past the chunk's end or an entry stored past a ring's end is a failure here, not a stray access on a device.
//
//   1. UDP probes over IPv4 (ihl 5 and 15) and IPv6 (pl 8, 41 and 1193: a quote of 48, an odd one, the capped one) with
//      0, 1 and 2 tags under every option word.  Cut at every length the frame is a heap buffer of exactly len bytes (the
//      UMEM is the frame) and no cut is answered.  Whole, it stands at the END of a chunk-sized allocation that is the
//      UMEM, max(len, R) bytes in front of its end: the reply fits to the byte, and one byte further on it is NO_ROOM.
//      The reply is checked field by field against the request, its checksums by summing, and the wave's rewrite --
//      64 lanes replayed, every load in front of every store -- against the one-thread rewrite byte for byte.  A reply
//      fed back is not answered (an error about an error: RFC 1122 §3.2.2).
//   2. The open-port map at its first and last bit; the port rule; an empty table.
//   3. The serve plan replayed lane by lane (the rank among the eligible, LIMITED, destination, rank, the stopping lane,
//      the job slot, the entry stored, the budget left) into rings of exactly their sizes, against the rule stated
//      sequentially: random verdicts, rooms from 0 to more than enough, budgets from 0 to more than enough.
// Stand-alone: prints "unreach ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/xsk_gpu.h"
#include "../../xsknet_amd/csrc/xsk_ring_dev.h"
#include "../../xsknet_amd/csrc/xsk_unreach.h"
#include "compact_replay.h"  // CHECK

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

typedef std::vector<uint8_t> Bytes;
static void put(Bytes& b, std::initializer_list<int> v) {
    for (int x : v) b.push_back((uint8_t)x);
}
static void put(Bytes& b, const uint8_t* p, size_t n) { b.insert(b.end(), p, p + n); }

static const uint8_t kPeerMac[6] = {0x02, 0xaa, 0xbb, 0xcc, 0xdd, 0x01}, kOwnMac[6] = {0x02, 0, 0, 0, 0x0a, 0x03};
static const uint8_t kPeer4[4] = {192, 0, 2, 77}, kOwn4[4] = {192, 0, 2, 1};
static const uint8_t kPeer6[16] = {0x20, 0x01, 0x0d, 0xb8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x77};
static const uint8_t kOwn6[16] = {0x20, 0x01, 0x0d, 0xb8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xfe};
static const uint32_t kChunk = 2048;

static uint32_t fold(const uint8_t* p, size_t n, uint64_t s = 0) {  // an odd last byte is a high byte
    for (size_t i = 0; i < n; ++i) s += (i & 1) ? (uint32_t)p[i] : (uint32_t)p[i] << 8;
    while (s >> 16) s = (s & 0xFFFF) + (s >> 16);
    return (uint32_t)s;
}

static Bytes eth(int tags, int ethertype) {
    Bytes f;
    put(f, kOwnMac, 6);
    put(f, kPeerMac, 6);
    for (int k = 0; k < tags; ++k) put(f, {k ? 0x81 : 0x88, k ? 0x00 : 0xA8, 0x00, 0x64 + k});
    put(f, {ethertype >> 8, ethertype & 0xFF});
    return f;
}
static Bytes udp4(int tags, int ihl, int data, int dport) {
    Bytes f = eth(tags, 0x0800);
    const size_t l3 = f.size();
    const int tl = 4 * ihl + 8 + data;
    put(f, {0x40 | ihl, 0x10, tl >> 8, tl & 0xFF, 0xBE, 0xEF, 0x40, 0, 57, 17, 0, 0});
    put(f, kPeer4, 4);
    put(f, kOwn4, 4);
    for (int k = 20; k < 4 * ihl; ++k) put(f, {k + 1 < 4 * ihl ? 1 : 0});
    const uint32_t cs = ~fold(&f[l3], 4 * (size_t)ihl) & 0xFFFFu;
    f[l3 + 10] = (uint8_t)(cs >> 8);
    f[l3 + 11] = (uint8_t)cs;
    put(f, {0x9C, 0x40, dport >> 8, dport & 0xFF, (8 + data) >> 8, (8 + data) & 0xFF, 0x12, 0x34});
    for (int k = 0; k < data; ++k) put(f, {(7 * k + 3) & 0xFF});
    return f;
}
static Bytes udp6(int tags, int data, int dport) {
    Bytes f = eth(tags, 0x86DD);
    const int pl = 8 + data;
    put(f, {0x60, 0xB5, 0x43, 0x21, pl >> 8, pl & 0xFF, 17, 61});
    put(f, kPeer6, 16);
    put(f, kOwn6, 16);
    put(f, {0x9C, 0x40, dport >> 8, dport & 0xFF, pl >> 8, pl & 0xFF, 0x12, 0x34});
    for (int k = 0; k < data; ++k) put(f, {(5 * k + 1) & 0xFF});
    return f;
}

static xsk_gpu_neigh_entry entry(int family, const uint8_t* addr, uint8_t port, const uint8_t* mac) {
    xsk_gpu_neigh_entry e;
    memset(&e, 0, sizeof(e));
    memcpy(e.addr, addr, family == 4 ? 4 : 16);
    e.family = (uint8_t)family;
    e.port = port;
    memcpy(e.mac, mac, 6);
    return e;
}
static uint32_t* stage(const std::vector<xsk_gpu_neigh_entry>& t) {
    uint32_t* s = exact<uint32_t>(t.size() * kNgEntryWords);
    for (size_t i = 0; i < t.size(); ++i) ng_stage_entry(&t[i], s + i * kNgEntryWords);
    return s;
}

// The wave's rewrite on the host: 64 lanes, every load in front of the sum, the sum in front of every store.
static void wave_rewrite(uint8_t* p, const UrVerdict& v) {
    UrLane lanes[kUrWave];
    uint64_t total = 0;
    for (uint32_t l = 0; l < kUrWave; ++l) lanes[l] = ur_lane_load(p, v.l3, v.q, l);
    for (uint32_t l = 0; l < kUrWave; ++l) total += ur_lane_part(lanes[l], v.verdict, l);
    for (uint32_t l = 0; l < kUrWave; ++l) {
        const uint32_t from = ur_hdr_swap(v.verdict, l);
        ur_lane_store(p, lanes[l], v, l, total, lanes[from & (kUrWave - 1u)].b[0]);
    }
}

// The reply in `got` (R bytes and what follows) against the request `full`, field by field.
static void check_reply(const uint8_t* got, const Bytes& full, bool v6, uint32_t l3, uint32_t q, uint32_t R, size_t span) {
    CHECK(!memcmp(got, kPeerMac, 6) && !memcmp(got + 6, kOwnMac, 6), "reply macs");
    CHECK(!memcmp(got + 12, full.data() + 12, l3 - 12), "tags and ethertype");
    const uint32_t H = v6 ? 48u : 28u;
    CHECK(R == l3 + H + q, "R");
    CHECK(!memcmp(got + l3 + H, full.data() + l3, q), "the quote");
    if (span > R) CHECK(!memcmp(got + R, full.data() + R, span - R), "bytes behind the reply");
    const uint8_t* h = got + l3;
    if (v6) {
        const uint8_t want[8] = {0x60, 0, 0, 0, (uint8_t)((8 + q) >> 8), (uint8_t)(8 + q), 0x3A, 0x40};
        CHECK(!memcmp(h, want, 8) && !memcmp(h + 8, kOwn6, 16) && !memcmp(h + 24, kPeer6, 16), "IPv6 header");
        CHECK(h[40] == 1 && h[41] == 4 && !(h[44] | h[45] | h[46] | h[47]), "ICMPv6 header");
        CHECK(fold(h + 40, 8 + (size_t)q, fold(h + 8, 32) + (8 + q) + 58u) == 0xFFFFu, "ICMPv6 checksum");
    } else {
        const uint8_t want[10] = {0x45, 0, (uint8_t)((28 + q) >> 8), (uint8_t)(28 + q), 0, 0, 0x40, 0, 0x40, 1};
        CHECK(!memcmp(h, want, 10) && !memcmp(h + 12, kOwn4, 4) && !memcmp(h + 16, kPeer4, 4), "IPv4 header");
        CHECK(fold(h, 20) == 0xFFFFu, "IPv4 header checksum");
        CHECK(h[20] == 3 && h[21] == 3 && !(h[24] | h[25] | h[26] | h[27]), "ICMP header");
        CHECK(fold(h + 20, 8 + (size_t)q) == 0xFFFFu, "ICMP checksum");
    }
}

static void frames() {
    std::vector<xsk_gpu_neigh_entry> t = {entry(4, kOwn4, 3, kOwnMac), entry(6, kOwn6, 7, kOwnMac)};
    uint32_t* tab = stage(t);
    uint8_t* open = exact<uint8_t>(kUrOpenBytes);
    memset(open, 0, kUrOpenBytes);
    open[0] = 1u;                      // port 0
    open[kUrOpenBytes - 1u] = 0x80u;   // port 65535
    const uint32_t opts[] = {0u, 0x2u, 0x10u, 0x12u, 0x17u};
    struct Kind {
        bool v6;
        int ihl, data;
    };
    const Kind kinds[] = {{false, 5, 0}, {false, 5, 60}, {false, 15, 3}, {true, 0, 0}, {true, 0, 33}, {true, 0, 1185}};
    for (const Kind& k : kinds)
        for (int tags = 0; tags <= 2; ++tags) {
            const Bytes full = k.v6 ? udp6(tags, k.data, 33434) : udp4(tags, k.ihl, k.data, 33434);
            const uint32_t l3 = 14u + 4u * (uint32_t)tags;
            const uint32_t q = k.v6 ? std::min(48u + (uint32_t)k.data, kUrMaxQuote6) : 4u * (uint32_t)k.ihl + 8u;
            const uint32_t R = l3 + (k.v6 ? 48u : 28u) + q;
            const uint32_t want = k.v6 ? XSK_GPU_UNREACH_UNREACH6 : XSK_GPU_UNREACH_UNREACH4;
            for (uint32_t o : opts) {
                const bool sees = (tags == 0 || (o & XSK_GPU_OPT_VLAN)) && (!k.v6 || (o & XSK_GPU_OPT_IPV6));
                // cut at every length below the whole frame: a buffer of exactly len bytes, never answered
                for (size_t len = 0; len < full.size(); ++len) {
                    uint8_t* buf = exact<uint8_t>(len);
                    if (len) memcpy(buf, full.data(), len);
                    const xsk_gpu_desc d = {0, (uint32_t)len, 0};
                    const UrVerdict v = ur_decide(buf, len, d, o, tab, 2, 8, ~0ull, open, kChunk);
                    CHECK(len == 0 || !memcmp(buf, full.data(), len), "the decision changed a byte");
                    CHECK(!ur_is_reply(v.verdict) && v.port == 0xFFu, "v6 %d tags %d opts %x len %zu answered", k.v6, tags, o, len);
                    const xsk_gpu_desc out = {1, (uint32_t)len, 0};  // rule 1: a descriptor that leaves the UMEM reads nothing
                    CHECK(ur_decide(buf, len, out, o, tab, 2, 8, ~0ull, open, kChunk).verdict == XSK_GPU_UNREACH_NONE, "rule 1");
                    free(buf);
                }
                // whole, at the end of a chunk that is the UMEM: the reply fits to the byte
                const size_t span = std::max(full.size(), (size_t)R);
                for (int rewrite = 0; rewrite < 2; ++rewrite) {
                    uint8_t* um = exact<uint8_t>(kChunk);
                    memset(um, 0xC3, kChunk);
                    const uint64_t at = kChunk - span;
                    memcpy(um + at, full.data(), full.size());
                    const xsk_gpu_desc d = {at, (uint32_t)full.size(), 0};
                    const UrVerdict v = ur_decide(um, kChunk, d, o, tab, 2, 8, ~0ull, open, kChunk);
                    if (!sees) {
                        CHECK(v.verdict == XSK_GPU_UNREACH_NONE, "not seen");
                        free(um);
                        continue;
                    }
                    CHECK(v.verdict == want && v.port == (k.v6 ? 7u : 3u) && v.l3 == l3 && v.q == q && v.reply_len == R,
                          "v6 %d tags %d opts %x: verdict %u q %u R %u", k.v6, tags, o, v.verdict, v.q, v.reply_len);
                    Bytes before(um, um + kChunk);
                    if (rewrite)
                        wave_rewrite(um + at, v);
                    else
                        ur_rewrite(um + at, v);
                    CHECK(!memcmp(um, before.data(), at), "bytes in front of the frame");
                    Bytes tail(full);  // what lay behind the request inside the span: sentinel
                    tail.resize(span, 0xC3);
                    check_reply(um + at, tail, k.v6, l3, q, R, span);
                    if (rewrite) {  // the two rewrites leave the same bytes
                        uint8_t* um2 = exact<uint8_t>(kChunk);
                        memcpy(um2, before.data(), kChunk);
                        ur_rewrite(um2 + at, v);
                        CHECK(!memcmp(um, um2, kChunk), "v6 %d tags %d: the wave's rewrite differs", k.v6, tags);
                        free(um2);
                    }
                    // an error about an error is never due: protocol 1 / next header 58
                    const xsk_gpu_desc back = {at, R, 0};
                    CHECK(ur_decide(um, kChunk, back, o, tab, 2, 8, ~0ull, open, kChunk).verdict == XSK_GPU_UNREACH_NONE, "fed back");
                    free(um);
                }
                if (!sees) continue;
                // one byte further on, or a UMEM that ends one byte early: NO_ROOM; the other rules of the resolve step
                {
                    uint8_t* um = exact<uint8_t>(2u * kChunk - 1u);
                    memset(um, 0xC3, 2u * kChunk - 1u);
                    if (R > full.size()) {
                        const uint64_t at = kChunk - R + 1u;  // the chunk ends one byte early
                        memcpy(um + at, full.data(), full.size());
                        const xsk_gpu_desc d = {at, (uint32_t)full.size(), 0};
                        CHECK(ur_decide(um, 2u * kChunk - 1u, d, o, tab, 2, 8, ~0ull, open, kChunk).verdict == XSK_GPU_UNREACH_NO_ROOM,
                              "no room");
                        CHECK(ur_decide(um, 2u * kChunk - 1u, d, o, tab, 2, 8, ~0ull, open, 2u * kChunk).verdict == want,
                              "room in a larger chunk");
                        const uint64_t at2 = 2u * kChunk - R;  // the chunk has room, the UMEM ends one byte early
                        memcpy(um + at2, full.data(), full.size());
                        const xsk_gpu_desc d2 = {at2, (uint32_t)full.size(), 0};
                        CHECK(ur_decide(um, 2u * kChunk - 1u, d2, o, tab, 2, 8, ~0ull, open, kChunk).verdict == XSK_GPU_UNREACH_NO_ROOM,
                              "the UMEM's end");
                        CHECK(ur_decide(um, 2u * kChunk - 1u, d2, o, tab, 2, 8, ~0ull, open, 2u * kChunk).verdict ==
                                  XSK_GPU_UNREACH_NO_ROOM, "the UMEM's end, a larger chunk");
                    }
                    memcpy(um, full.data(), full.size());
                    const xsk_gpu_desc d0 = {0, (uint32_t)full.size(), 0};
                    CHECK(ur_decide(um, kChunk, d0, o, tab, 2, 3, ~0ull, open, kChunk).verdict == XSK_GPU_UNREACH_UNBOUND, "n_ports");
                    CHECK(ur_decide(um, kChunk, d0, o, tab, 2, 4, ~0ull, open, kChunk).verdict ==
                              (k.v6 ? (uint32_t)XSK_GPU_UNREACH_UNBOUND : want), "n_ports 4");
                    CHECK(ur_decide(um, kChunk, d0, o, tab, 2, 8, ~(1ull << (k.v6 ? 7 : 3)), open, kChunk).verdict ==
                              XSK_GPU_UNREACH_UNBOUND, "bound bit");
                    CHECK(ur_decide(um, kChunk, d0, o, tab, 0, 8, ~0ull, open, kChunk).verdict == XSK_GPU_UNREACH_UNKNOWN, "empty table");
                    CHECK(ur_decide(um, kChunk, d0, o, tab, 2, 8, ~0ull, NULL, kChunk).verdict == want, "no map");
                    free(um);
                }
            }
            // the map's first and last bit
            for (int dport : {0, 65535, 1, 65534}) {
                const Bytes f = k.v6 ? udp6(tags, k.data, dport) : udp4(tags, k.ihl, k.data, dport);
                uint8_t* um = exact<uint8_t>(kChunk);
                memcpy(um, f.data(), f.size());
                const xsk_gpu_desc d = {0, (uint32_t)f.size(), 0};
                const uint32_t got = ur_decide(um, kChunk, d, 0x17u, tab, 2, 8, ~0ull, open, kChunk).verdict;
                CHECK(got == ((dport == 0 || dport == 65535) ? (uint32_t)XSK_GPU_UNREACH_LEFT : want), "port %d: %u", dport, got);
                free(um);
            }
        }
    free(open);
    free(tab);
}

// ---- the serve plan ----
struct HostRing {
    xsk_gpu_desc* e;
    uint32_t size, prod, cons;
};
static HostRing ring(uint32_t size, uint32_t prod, uint32_t used) {
    HostRing r = {exact<xsk_gpu_desc>(size), size, prod, prod - used};
    for (uint32_t i = 0; i < size; ++i) r.e[i] = xsk_gpu_desc{~0ull, 0xEEEEEEEEu, 0xDDDDDDDDu};
    return r;
}

static void serve() {
    for (int round = 0; round < 300; ++round) {
        const uint32_t n_ports = 1u + rnd(63), max = 1u + rnd(1023);
        const uint32_t ssize = 1u << rnd(10), sused = rnd(ssize) + (rnd(9) == 0 ? 5u : 0u);  // now and then above the size
        const uint32_t start = rnd(3) ? 0xFFFFFFF0u + rnd(15) : (uint32_t)rnd64();
        const uint32_t budget0 = rnd(3) == 0 ? 0xFFFFFFFFu - rnd(2) : (rnd(3) == 0 ? 0u : rnd(sused / 2u + 1u));
        HostRing up = ring(ssize, start + sused, sused);
        std::vector<UrVerdict> v(ssize);
        for (uint32_t i = 0; i < ssize; ++i) {
            up.e[i] = xsk_gpu_desc{(uint64_t)i * 2048u + (1ull << 33), 60u + rnd(200), rnd(7)};
            const uint32_t verdict = rnd(9) < 5 ? 1u + rnd(1) : (rnd(1) ? 0u : 3u + rnd(4));
            v[i] = ur_none();
            v[i].verdict = verdict;
            if (ur_is_reply(verdict)) {
                v[i].port = rnd(n_ports - 1u);
                v[i].l3 = 14u + 4u * rnd(2);
                v[i].q = verdict == XSK_GPU_UNREACH_UNREACH6 ? 48u + rnd(1184) : 28u + 4u * rnd(10);
                v[i].reply_len = v[i].l3 + ur_hdr(verdict) + v[i].q;
                v[i].mac_lo = (uint32_t)rnd64();
                v[i].mac_hi = (uint32_t)rnd64() & 0xFFFFu;
            }
        }
        std::vector<HostRing> a, b;  // the replay's destinations and the sequential rule's: ports, then rest
        for (uint32_t dst = 0; dst <= n_ports; ++dst) {
            const uint32_t size = 1u << rnd(dst == n_ports ? 10 : 5), used = rnd(3) == 0 ? size : rnd(size);
            const uint32_t prod = rnd(1) ? 0xFFFFFFFAu + rnd(5) : (uint32_t)rnd64();
            a.push_back(ring(size, prod, used));
            b.push_back(ring(size, prod, used));
        }
        // the replay: every lane for itself
        const uint32_t m = ng_serve_m(rd_used(up.prod, up.cons, up.size), max);
        std::vector<uint32_t> rank(m), dest(m), erank(m);
        std::vector<UrVerdict> w(m);
        uint32_t eligible = 0, c = m;
        for (uint32_t j = 0; j < m; ++j) {
            w[j] = v[rd_slot(up.cons + j, up.size)];
            erank[j] = eligible;
            eligible += ur_is_reply(w[j].verdict);
            w[j].verdict = ur_limit(w[j].verdict, erank[j], budget0);
        }
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t d = ur_dest(w[j].verdict, w[j].port);
            dest[j] = d == kNgUp ? n_ports : d;
            rank[j] = 0;
            for (uint32_t i = 0; i < j; ++i) rank[j] += (ur_dest(w[i].verdict, w[i].port) == d);
            const HostRing& r = a[dest[j]];
            c = std::min(c, ng_stop_at(j, m, rank[j], rd_free(r.prod, r.cons, r.size)));
        }
        std::vector<uint32_t> got(n_ports + 1u, 0u);
        UrJob* jobs = exact<UrJob>(m);  // a slot per eligible entry at the most
        std::vector<int> job_set(m, 0);
        uint32_t n_jobs = 0;
        for (uint32_t j = 0; j < c; ++j) {
            const uint32_t s = rd_slot(up.cons + j, up.size);
            HostRing& r = a[dest[j]];
            r.e[rd_slot(r.prod + rank[j], r.size)] = ur_out_entry(up.e[s], w[j]);
            ++got[dest[j]];
            if (ur_is_reply(w[j].verdict)) {
                CHECK(erank[j] < m && !job_set[erank[j]], "round %d: job slot %u", round, erank[j]);
                jobs[erank[j]] = ur_job(up.e[s].addr, w[j]);
                job_set[erank[j]] = 1;
                ++n_jobs;
            }
        }
        for (uint32_t dst = 0; dst <= n_ports; ++dst) a[dst].prod += got[dst];
        // the rule, sequentially
        uint32_t cs = 0, left = budget0, sent = 0;
        std::vector<uint32_t> given(n_ports + 1u, 0u), room(n_ports + 1u);
        for (uint32_t dst = 0; dst <= n_ports; ++dst) room[dst] = b[dst].size - std::min(b[dst].prod - b[dst].cons, b[dst].size);
        for (uint32_t j = 0; j < std::min(std::min(up.prod - up.cons, up.size), max); ++j) {
            const uint32_t s = (up.cons + j) & (up.size - 1u);
            UrVerdict x = v[s];
            if (ur_is_reply(x.verdict) && left == 0u) x.verdict = XSK_GPU_UNREACH_LIMITED;
            const uint32_t dst = ur_is_reply(x.verdict) ? x.port : n_ports;
            if (given[dst] >= room[dst]) break;
            xsk_gpu_desc e = up.e[s];
            if (ur_is_reply(x.verdict)) {
                // the job in slot `sent` is this entry's rewrite
                CHECK(sent < m && job_set[sent], "round %d: job %u missing", round, sent);
                const UrVerdict jv = ur_job_verdict(jobs[sent]);
                CHECK(ur_job_addr(jobs[sent]) == e.addr && jv.verdict == x.verdict && jv.l3 == x.l3 && jv.q == x.q &&
                          jv.reply_len == x.reply_len && jv.mac_lo == x.mac_lo && jv.mac_hi == x.mac_hi,
                      "round %d: job %u", round, sent);
                e = xsk_gpu_desc{e.addr, x.reply_len, 0u};
                --left;
                ++sent;
            }
            b[dst].e[(b[dst].prod + given[dst]) & (b[dst].size - 1u)] = e;
            ++given[dst];
            ++cs;
        }
        CHECK(c == cs && n_jobs == sent && budget0 - n_jobs == left, "round %d: c %u against %u, jobs %u against %u", round, c,
              cs, n_jobs, sent);
        for (uint32_t dst = 0; dst <= n_ports; ++dst) {
            CHECK(a[dst].prod == b[dst].prod + given[dst], "round %d: producer of %u", round, dst);
            CHECK(!memcmp(a[dst].e, b[dst].e, (size_t)a[dst].size * sizeof(xsk_gpu_desc)), "round %d: entries of %u", round, dst);
            free(a[dst].e);
            free(b[dst].e);
        }
        free(jobs);
        free(up.e);
    }
}

int main() {
    CHECK(ur_chunk_ok(2048) && ur_chunk_ok(1u << 20) && !ur_chunk_ok(1024) && !ur_chunk_ok(1u << 21) && !ur_chunk_ok(3000) &&
              !ur_chunk_ok(0), "chunk sizes");
    frames();
    serve();
    printf("unreach ok\n");
    return 0;
}
