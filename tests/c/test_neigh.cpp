// xsk_neigh.h (xsknet_amd/csrc) compiled for the host: the per-frame decision, the table search, the two rewrites and
// the serve plan of xsk_gpu_neigh_dev() / xsk_gpu_neigh_serve_dev().  Every array is a heap allocation of exactly its
// size and the test builds this file with -fsanitize=address,undefined, so a byte read past a frame's end, a probe
// outside a table or an entry stored past a ring's end is a failure here, not a stray access on a device.
//
//   1. Frames in heap buffers of exactly len bytes (the UMEM is the frame): the ARP request and two neighbour
//      solicitations -- one whose reply fills the frame, one whose options run to the frame's last byte -- with 0, 1 and
//      2 tags, cut at every length from 0 to the full request, under every option word.  The full request is answered
//      where the option word lets the responder see it, no cut of it is; an answered frame, decided again, is NONE, and
//      a neighbour advertisement sums to 0xFFFF under its own pseudo-header.
//   2. Tables of 0, 1, 1023 and 1024 entries staged into exactly n * 8 words: every key present is found with its port
//      and mac, keys between them miss; the same tables filled with garbage are searched for the bounds alone.
//   3. The serve plan replayed lane by lane (destination, rank, the stopping lane, the entry stored) into rings of
//      exactly their sizes, against the rule stated sequentially: random verdicts, rooms from 0 to more than enough,
//      producer words around the wrap.
// Stand-alone: prints "neigh ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/xsk_gpu.h"
#include "../../xsknet_amd/csrc/xsk_neigh.h"
#include "../../xsknet_amd/csrc/xsk_ring_dev.h"
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

static uint32_t fold(const uint8_t* p, size_t n, uint64_t s = 0) {
    for (size_t i = 0; i + 1 < n; i += 2) s += ((uint32_t)p[i] << 8) | p[i + 1];
    while (s >> 16) s = (s & 0xFFFF) + (s >> 16);
    return (uint32_t)s;
}

static Bytes eth(int tags, int ethertype) {
    Bytes f;
    put(f, {0xff, 0xff, 0xff, 0xff, 0xff, 0xff});
    put(f, kPeerMac, 6);
    for (int k = 0; k < tags; ++k) put(f, {k ? 0x81 : 0x88, k ? 0x00 : 0xA8, 0x00, 0x64 + k});
    put(f, {ethertype >> 8, ethertype & 0xFF});
    return f;
}
static Bytes arp_request(int tags) {
    Bytes f = eth(tags, 0x0806);
    put(f, {0, 1, 8, 0, 6, 4, 0, 1});
    put(f, kPeerMac, 6);
    put(f, kPeer4, 4);
    put(f, {0, 0, 0, 0, 0, 0});
    put(f, kOwn4, 4);
    return f;
}
// A solicitation for kOwn6 with `opt16` false: the 8-byte source link-layer option (pl == 32); true: one 16-byte
// option that runs to the frame's last byte (pl == 40).
static Bytes ns_request(int tags, bool opt16) {
    Bytes f = eth(tags, 0x86DD);
    const size_t l3 = f.size();
    const int pl = opt16 ? 40 : 32;
    put(f, {0x60, 0, 0, 0, 0, pl, 58, 255});
    put(f, kPeer6, 16);
    put(f, {0xff, 0x02, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x01, 0xff, 0, 0, 0xfe});
    put(f, {135, 0, 0, 0, 0, 0, 0, 0});
    put(f, kOwn6, 16);
    if (opt16)
        put(f, {14, 2, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14});
    else {
        put(f, {1, 1});
        put(f, kPeerMac, 6);
    }
    const uint32_t cs = ~fold(&f[l3 + 8], 32 + (size_t)pl, (uint64_t)pl + 58) & 0xFFFFu;
    f[l3 + 42] = (uint8_t)(cs >> 8);
    f[l3 + 43] = (uint8_t)cs;
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

static void frames() {
    std::vector<xsk_gpu_neigh_entry> t = {entry(4, kOwn4, 3, kOwnMac), entry(6, kOwn6, 7, kOwnMac)};
    uint32_t* tab = stage(t);
    const uint32_t opts[] = {0u, 0x2u, 0x10u, 0x12u, 0x17u};
    for (int kind = 0; kind < 3; ++kind)
        for (int tags = 0; tags <= 2; ++tags) {
            const Bytes full = kind == 0 ? arp_request(tags) : ns_request(tags, kind == 2);
            const uint32_t l3 = 14u + 4u * (uint32_t)tags;
            for (uint32_t o : opts)
                for (size_t len = 0; len <= full.size(); ++len) {
                    uint8_t* buf = exact<uint8_t>(len);
                    if (len) memcpy(buf, full.data(), len);
                    const xsk_gpu_desc d = {0, (uint32_t)len, 0};
                    const NgVerdict v = ng_decide(buf, len, d, o, tab, 2, 8, ~0ull);
                    CHECK(len == 0 || !memcmp(buf, full.data(), len), "the decision changed a byte");
                    const bool sees = (tags == 0 || (o & XSK_GPU_OPT_VLAN)) && (kind == 0 || (o & XSK_GPU_OPT_IPV6));
                    const uint32_t want = kind == 0 ? XSK_GPU_NEIGH_ARP_REPLY : XSK_GPU_NEIGH_NA_REPLY;
                    if (len == full.size() && sees) {
                        CHECK(v.verdict == want && v.port == (kind ? 7u : 3u) && v.l3 == l3, "kind %d tags %d opts %x: %u",
                              kind, tags, o, v.verdict);
                        CHECK(v.reply_len == (kind ? l3 + 72u : (uint32_t)len) && v.reply_len <= len, "reply length");
                        ng_rewrite(buf, v);
                        CHECK(!memcmp(buf + 6, kOwnMac, 6) && !memcmp(buf, kPeerMac, 6), "reply macs");
                        if (kind) CHECK(fold(buf + l3 + 8, 64, 32 + 58) == 0xFFFFu, "advertisement checksum");
                        if (kind == 2) CHECK(!memcmp(buf + l3 + 72, full.data() + l3 + 72, 8), "bytes behind the reply");
                        CHECK(ng_decide(buf, len, d, o, tab, 2, 8, ~0ull).verdict == XSK_GPU_NEIGH_NONE, "a reply fed back");
                    } else {
                        CHECK(!ng_is_reply(v.verdict) && v.port == 0xFFu, "kind %d tags %d opts %x len %zu answered", kind,
                              tags, o, len);
                    }
                    // rule 1: a descriptor that leaves the UMEM reads nothing
                    const xsk_gpu_desc out = {1, (uint32_t)len, 0};
                    CHECK(ng_decide(buf, len, out, o, tab, 2, 8, ~0ull).verdict == XSK_GPU_NEIGH_NONE, "rule 1");
                    // an unbound port and a port at or above n_ports
                    if (len == full.size() && sees) {
                        memcpy(buf, full.data(), len);
                        CHECK(ng_decide(buf, len, d, o, tab, 2, 3, ~0ull).verdict == XSK_GPU_NEIGH_UNBOUND, "n_ports");
                        CHECK(ng_decide(buf, len, d, o, tab, 2, 8, ~(1ull << (kind ? 7 : 3))).verdict == XSK_GPU_NEIGH_UNBOUND,
                              "bound bit");
                        CHECK(ng_decide(buf, len, d, o, tab, 0, 8, ~0ull).verdict == XSK_GPU_NEIGH_UNKNOWN, "empty table");
                    }
                    free(buf);
                }
        }
    free(tab);
}

static void tables() {
    for (uint32_t n : {0u, 1u, 1023u, 1024u}) {
        std::vector<xsk_gpu_neigh_entry> t;
        for (uint32_t i = 0; i < n; ++i) {  // keys 2 apart, half of them IPv4, ascending
            uint8_t a[16] = {0};
            const bool v4 = i < n / 2;
            const uint32_t k = 2u * i + 2u;
            a[v4 ? 2 : 14] = (uint8_t)(k >> 8);
            a[v4 ? 3 : 15] = (uint8_t)k;
            const uint8_t mac[6] = {2, 0, 0, 0, (uint8_t)(i >> 8), (uint8_t)i};
            t.push_back(entry(v4 ? 4 : 6, a, (uint8_t)(i & 63u), mac));
        }
        uint32_t* tab = stage(t);
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t key[5];
            memcpy(key, tab + i * kNgEntryWords, sizeof(key));
            const uint32_t at = ng_lookup(tab, n, key);
            CHECK(at == i && tab[at * kNgEntryWords + 5] == (i & 63u) && tab[at * kNgEntryWords + 7] == ((i & 0xFF) << 8 | i >> 8),
                  "n %u key %u found at %u", n, i, at);
            key[key[0] == 4 ? 1 : 4] += 1u;  // the key between two entries
            CHECK(ng_lookup(tab, n, key) == kNgMiss, "a key between entries was found");
        }
        const uint32_t none[5] = {4, 0, 0, 0, 0};
        CHECK(ng_lookup(tab, n, none) == kNgMiss, "below every key");
        for (size_t w = 0; w < (size_t)n * kNgEntryWords; ++w) tab[w] = (uint32_t)rnd64();  // garbage: bounds only
        for (int r = 0; r < 2000; ++r) {
            uint32_t key[5];
            for (uint32_t& w : key) w = (uint32_t)rnd64();
            const uint32_t at = ng_lookup(tab, n, key);
            CHECK(at == kNgMiss || at < n, "a probe left the table");
        }
        free(tab);
    }
}

// ---- 3. the serve plan ----
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
        HostRing stack = ring(ssize, start + sused, sused);
        std::vector<NgVerdict> v(ssize);
        for (uint32_t i = 0; i < ssize; ++i) {
            stack.e[i] = xsk_gpu_desc{(uint64_t)i * 2048u, 60u + rnd(200), rnd(7)};
            const uint32_t verdict = rnd(9) < 5 ? 1u + rnd(1) : (rnd(1) ? 0u : 3u + rnd(3));
            v[i] = NgVerdict{verdict, ng_is_reply(verdict) ? rnd(n_ports - 1u) : 0xFFu, 42u + rnd(100), 14u, 0u, 0u};
        }
        std::vector<HostRing> a, b;  // the replay's destinations and the sequential rule's: ports, then up
        for (uint32_t dst = 0; dst <= n_ports; ++dst) {
            const uint32_t size = 1u << rnd(dst == n_ports ? 10 : 5), used = rnd(3) == 0 ? size : rnd(size);
            const uint32_t prod = rnd(1) ? 0xFFFFFFFAu + rnd(5) : (uint32_t)rnd64();
            a.push_back(ring(size, prod, used));
            b.push_back(ring(size, prod, used));
        }
        auto dest_of = [&](const NgVerdict& x) { return ng_is_reply(x.verdict) ? x.port : n_ports; };
        // the replay: every lane for itself
        const uint32_t m = ng_serve_m(rd_used(stack.prod, stack.cons, stack.size), max);
        std::vector<uint32_t> rank(m), dest(m);
        uint32_t c = m;
        for (uint32_t j = 0; j < m; ++j) {
            const NgVerdict& x = v[rd_slot(stack.cons + j, stack.size)];
            dest[j] = ng_dest(x.verdict, x.port) == kNgUp ? n_ports : x.port;
            rank[j] = 0;
            for (uint32_t i = 0; i < j; ++i) rank[j] += dest_of(v[rd_slot(stack.cons + i, stack.size)]) == dest[j];
            const HostRing& r = a[dest[j]];
            c = std::min(c, ng_stop_at(j, m, rank[j], rd_free(r.prod, r.cons, r.size)));
        }
        std::vector<uint32_t> got(n_ports + 1u, 0u);
        for (uint32_t j = 0; j < c; ++j) {
            const uint32_t s = rd_slot(stack.cons + j, stack.size);
            HostRing& r = a[dest[j]];
            r.e[rd_slot(r.prod + rank[j], r.size)] = ng_out_entry(stack.e[s], v[s]);
            ++got[dest[j]];
        }
        for (uint32_t dst = 0; dst <= n_ports; ++dst) a[dst].prod += got[dst];
        // the rule, sequentially
        uint32_t cs = 0;
        std::vector<uint32_t> given(n_ports + 1u, 0u), room(n_ports + 1u);
        for (uint32_t dst = 0; dst <= n_ports; ++dst) room[dst] = b[dst].size - std::min(b[dst].prod - b[dst].cons, b[dst].size);
        for (uint32_t j = 0; j < std::min(std::min(stack.prod - stack.cons, stack.size), max); ++j) {
            const uint32_t s = (stack.cons + j) & (stack.size - 1u);
            const uint32_t dst = dest_of(v[s]);
            if (given[dst] >= room[dst]) break;
            xsk_gpu_desc e = stack.e[s];
            if (ng_is_reply(v[s].verdict)) e = xsk_gpu_desc{e.addr, v[s].reply_len, 0u};
            b[dst].e[(b[dst].prod + given[dst]) & (b[dst].size - 1u)] = e;
            ++given[dst];
            ++cs;
        }
        CHECK(c == cs, "round %d: c %u against %u", round, c, cs);
        for (uint32_t dst = 0; dst <= n_ports; ++dst) {
            CHECK(a[dst].prod == b[dst].prod + given[dst], "round %d: producer of %u", round, dst);
            CHECK(!memcmp(a[dst].e, b[dst].e, (size_t)a[dst].size * sizeof(xsk_gpu_desc)), "round %d: entries of %u", round, dst);
            free(a[dst].e);
            free(b[dst].e);
        }
        free(stack.e);
    }
}

int main() {
    frames();
    tables();
    serve();
    printf("neigh ok\n");
    return 0;
}
