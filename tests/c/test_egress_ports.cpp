// The arithmetic of xsk_gpu_egress_ports_dev() (xsknet_amd/csrc/xsk_egress_ports.h) compiled for the host: both paths
// of xsk_egress_ports.hip replayed thread by thread with the header's functions -- the prologue (a wave's max-scan of
// the offset words, the clamp), the one-workgroup path (wave ballots, sixteen counts and masks, the prefix at every
// boundary, owner, slot) and the three-stage path (per-workgroup counts over [o_0, o_n) -> the 1024-thread scan over
// runs -> a prefix per boundary -> owner and slot per lane -> the per-port counter records and their sum) -- and compared
// with a plain sequential loop per port.
//
// Inputs are heap arrays of exactly n_max entries (n_ports + 1 words, n_ports rooms), the outputs of exactly n_max, the
// workspace of ep_workspace_bytes(); the test builds this file with -fsanitize=address,undefined.  The lists of all
// ports share the two output arrays, so AddressSanitizer alone does not see one port writing into another's span: every
// store of the replay is therefore checked to land inside [o_p, o_p + n_tx_p) or [o_p, o_p + n_free_p) of the port that
// owns the frame by the sequential loop, and every such slot to be written exactly once; then both arrays are compared
// whole, sentinels included.
//
// n_max in {1, 64, 65, 1023, 1024, 1025, 4099, 262147, 2^20 + 1} x n_ports in {1, 2, 8, 63, 64} x ten layouts (one port
// owning everything; all segments empty; empty segments at the front, in the middle, at the end; segments of 3 frames
// inside one workgroup; boundaries on wave and workgroup edges and one off either side; random with repeats; o_0 > 0
// and o_n < n_max; words not ascending and above the bound) x rooms (NULL, 0, R_p - 1, R_p, mixed) x the seven reply
// patterns; the two largest bounds take pattern and room in turn.  Stand-alone: prints "egress ports ok".
#include <initializer_list>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/xsk_gpu.h"
#include "../../xsknet_amd/csrc/xsk_egress_ports.h"
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

static unsigned popc(uint64_t m) { return (unsigned)__builtin_popcountll(m); }

struct Case {
    uint32_t n_max, n_ports;
    const uint32_t* words;  // n_ports + 1
    const uint32_t* rooms;  // n_ports, or NULL
    const xsk_gpu_desc* descs;
    const uint8_t* verdict;
    const char* what;
};

struct PortSums {
    uint64_t rx_packets, rx_bytes, tx_packets, tx_bytes;
};

struct Out {
    xsk_gpu_desc* tx;  // n_max
    uint64_t* fr;      // n_max
    EgCounts c[kEpMaxPorts];
    PortSums ps[kEpMaxPorts];
    uint64_t lost_packets, lost_bytes;
};

struct Ref : Out {
    uint32_t o[kEpMaxBounds];
    int32_t* owner;  // n_max: the port of position i, -1 on no list
};

struct Got : Out {
    uint8_t *wtx, *wfr;  // n_max each: how often a slot was written
    uint64_t port_sets, sum_sets, shared_sets, workgroups;  // sets of atomics: scatter per port, stage 4, shared block
};

// ---- the plain loop: per port, what xsk_gpu__rx_emit() does over the port's segment ----
static void sequential(const Case& k, Ref* r) {
    uint32_t run = 0;
    for (uint32_t p = 0; p <= k.n_ports; ++p) {
        if (k.words[p] > run) run = k.words[p];
        r->o[p] = run < k.n_max ? run : k.n_max;
    }
    for (uint32_t i = 0; i < k.n_max; ++i) r->owner[i] = -1;
    r->lost_packets = r->lost_bytes = 0;
    for (uint32_t p = 0; p < k.n_ports; ++p) {
        const uint32_t room = k.rooms ? k.rooms[p] : 0xFFFFFFFFu, o = r->o[p];
        uint32_t sent = 0, freed = 0, full = 0;
        PortSums s = {0, 0, 0, 0};
        for (uint32_t i = o; i < r->o[p + 1]; ++i) {
            r->owner[i] = (int32_t)p;
            s.rx_packets++;
            s.rx_bytes += k.descs[i].len;
            if (k.verdict[i] == XSK_GPU_TX_REPLY && sent < room) {
                r->tx[o + sent].addr = k.descs[i].addr;
                r->tx[o + sent].len = k.descs[i].len;
                r->tx[o + sent].options = 0;
                sent++;
                s.tx_packets++;
                s.tx_bytes += k.descs[i].len;
            } else {
                if (k.verdict[i] == XSK_GPU_TX_REPLY) {
                    full++;
                    r->lost_packets++;
                    r->lost_bytes += k.descs[i].len;
                }
                r->fr[o + freed++] = k.descs[i].addr;
            }
        }
        r->c[p].n = r->o[p + 1] - o;
        r->c[p].n_tx = sent;
        r->c[p].n_tx_full = full;
        r->c[p].n_free = freed;
        r->ps[p] = s;
    }
}

// ---- the kernels' prologue: wave 0, lane l takes word l; Hillis-Steele inclusive max over the wave; the clamp ----
struct Staged {
    uint32_t o[kEpMaxBounds], g[kEpMaxBounds], room[kEpMaxPorts];
};

static void stage(const Case& k, Staged* s) {
    uint32_t w[kEgWave], v[kEgWave];
    for (uint32_t l = 0; l < kEgWave; ++l) w[l] = l <= k.n_ports ? k.words[l] : 0u;  // (only words[0, n_ports] are read)
    for (uint32_t d = 1; d < kEgWave; d <<= 1) {
        for (uint32_t l = 0; l < kEgWave; ++l) v[l] = l >= d ? w[l - d] : w[l];  // __shfl_up
        for (uint32_t l = 0; l < kEgWave; ++l)
            if (l >= d) w[l] = ep_max(w[l], v[l]);
    }
    for (uint32_t l = 0; l < kEgWave; ++l)
        if (l <= k.n_ports) s->o[l] = ep_clamp(w[l], k.n_max);
    if (k.n_ports == kEpMaxPorts) s->o[kEpMaxPorts] = ep_clamp(ep_max(w[kEgWave - 1], k.words[kEpMaxPorts]), k.n_max);
    for (uint32_t l = 0; l < k.n_ports; ++l) s->room[l] = eg_room(k.rooms != NULL, k.rooms ? k.rooms[l] : 0u);
    uint32_t seq[kEpMaxBounds];
    ep_offsets(k.words, k.n_ports, k.n_max, seq);
    for (uint32_t p = 0; p <= k.n_ports; ++p) {
        CHECK(seq[p] == s->o[p], "%s: the wave scan and ep_offsets differ at %u", k.what, p);
        CHECK(s->o[p] <= k.n_max && (!p || s->o[p - 1] <= s->o[p]), "%s: offsets not ascending inside the bound", k.what);
    }
}

// ---- what ep_finish() does for the lanes of one workgroup ----
struct Lane {
    bool reply;
    uint32_t g_i;
};

static void finish_wg(const Case& k, const Ref& ref, const Staged& s, uint32_t i0, uint32_t threads, const Lane* lanes,
                      Got* r, EpPart* part, uint8_t* wpart, uint32_t wg) {
    struct {
        uint64_t bytes, tx_bytes, unsent_bytes;
        uint32_t n, n_tx, n_unsent;
    } acc[kEpMaxPorts];
    memset(acc, 0, sizeof(acc));
    r->workgroups++;
    for (uint32_t w = 0; w < threads / kEgWave; ++w) {
        uint32_t key[kEgWave];
        bool sub[kEgWave], uns[kEgWave];
        uint32_t len[kEgWave];
        for (uint32_t lane = 0; lane < kEgWave; ++lane) {
            const uint64_t i64 = (uint64_t)i0 + w * kEgWave + lane;
            CHECK(i64 <= 0xFFFFFFFFull, "index");
            const uint32_t i = (uint32_t)i64;
            const Lane& L = lanes[w * kEgWave + lane];
            const EpOwner ow = ep_owner(s.o, k.n_ports, i);
            key[lane] = ow.on ? ow.port : 0xFFFFFFFFu;
            sub[lane] = uns[lane] = false;
            len[lane] = 0;
            CHECK(ow.on == (i < k.n_max && ref.owner[i] >= 0), "%s: frame %u on a list: %d", k.what, i, (int)ow.on);
            if (!ow.on) continue;
            const uint32_t p = ow.port;
            CHECK((int32_t)p == ref.owner[i], "%s: frame %u owner %u, want %d", k.what, i, p, ref.owner[i]);
            CHECK(s.o[p] <= i && i < s.o[p + 1], "%s: owner's segment", k.what);
            const EgSlot sl = ep_slot(L.reply, i, s.o[p], L.g_i, s.g[p], s.room[p]);
            const uint32_t o = ref.o[p];
            if (sl.tx) {
                CHECK(sl.slot >= o && sl.slot < o + ref.c[p].n_tx, "%s: frame %u port %u tx slot %u outside [%u, %u)", k.what,
                      i, p, sl.slot, o, o + ref.c[p].n_tx);
                CHECK(r->wtx[sl.slot]++ == 0, "%s: tx slot %u written twice", k.what, sl.slot);
                r->tx[sl.slot].addr = k.descs[i].addr;
                r->tx[sl.slot].len = k.descs[i].len;
                r->tx[sl.slot].options = 0;
            } else {
                CHECK(sl.slot >= o && sl.slot < o + ref.c[p].n_free, "%s: frame %u port %u free slot %u outside [%u, %u)",
                      k.what, i, p, sl.slot, o, o + ref.c[p].n_free);
                CHECK(r->wfr[sl.slot]++ == 0, "%s: free slot %u written twice", k.what, sl.slot);
                r->fr[sl.slot] = k.descs[i].addr;
            }
            sub[lane] = sl.tx;
            uns[lane] = ep_unsent(L.reply, L.g_i, s.g[p], s.room[p]);
            len[lane] = k.descs[i].len;
        }
        bool uniform = true;
        for (uint32_t lane = 1; lane < kEgWave; ++lane) uniform = uniform && key[lane] == key[0];
        if (uniform) {  // ballots and shuffles, lane 0 adds
            if (key[0] == 0xFFFFFFFFu) continue;
            acc[key[0]].n += kEgWave;
            for (uint32_t lane = 0; lane < kEgWave; ++lane) {
                acc[key[0]].bytes += len[lane];
                acc[key[0]].n_tx += sub[lane];
                acc[key[0]].tx_bytes += sub[lane] ? len[lane] : 0u;
                acc[key[0]].n_unsent += uns[lane];
                acc[key[0]].unsent_bytes += uns[lane] ? len[lane] : 0u;
            }
        } else {
            for (uint32_t lane = 0; lane < kEgWave; ++lane) {
                if (key[lane] == 0xFFFFFFFFu) continue;
                acc[key[lane]].n += 1;
                acc[key[lane]].bytes += len[lane];
                acc[key[lane]].n_tx += sub[lane];
                acc[key[lane]].tx_bytes += sub[lane] ? len[lane] : 0u;
                acc[key[lane]].n_unsent += uns[lane];
                acc[key[lane]].unsent_bytes += uns[lane] ? len[lane] : 0u;
            }
        }
    }
    uint64_t nu = 0, bu = 0;
    uint32_t carry = 0xFFFFFFFFu;  // the port whose sums this workgroup leaves as a record (three-stage path)
    if (part && ep_wg_carries(wg, s.o[0], s.o[k.n_ports])) carry = ep_owner(s.o, k.n_ports, wg * kEgFrames).port;
    for (uint32_t p = 0; p < k.n_ports; ++p) {
        if (p == carry) {
            CHECK(acc[p].n > 0 && ref.owner[wg * kEgFrames] == (int32_t)p, "%s: record of a port without frames", k.what);
            CHECK(wpart[wg]++ == 0, "%s: record %u written twice", k.what, wg);
            EpPart* q = part + wg;
            q->n = acc[p].n;
            q->n_tx = acc[p].n_tx;
            q->bytes_lo = (uint32_t)acc[p].bytes;
            q->bytes_hi = (uint32_t)(acc[p].bytes >> 32);
            q->tx_bytes_lo = (uint32_t)acc[p].tx_bytes;
            q->tx_bytes_hi = (uint32_t)(acc[p].tx_bytes >> 32);
        } else if (acc[p].n) {
            r->port_sets++;
            r->ps[p].rx_packets += acc[p].n;
            r->ps[p].rx_bytes += acc[p].bytes;
            r->ps[p].tx_packets += acc[p].n_tx;
            r->ps[p].tx_bytes += acc[p].tx_bytes;
        }
        nu += acc[p].n_unsent;
        bu += acc[p].unsent_bytes;
    }
    if (nu) {
        r->shared_sets++;
        r->lost_packets += nu;
        r->lost_bytes += bu;
    }
}

// ---- the device paths, as xsk_gpu_egress_ports_dev() dispatches them ----
static void device_paths(const Case& k, const Ref& ref, Got* r) {
    static Lane lanes[kEgSmallThreads];
    Staged s;
    memset(&s, 0xEE, sizeof(s));
    stage(k, &s);
    const uint32_t lo = s.o[0], hi = s.o[k.n_ports];
    r->lost_packets = r->lost_bytes = r->port_sets = r->sum_sets = r->shared_sets = r->workgroups = 0;
    memset(r->ps, 0, sizeof(r->ps));
    if (k.n_max <= kEgSmallMax) {
        CHECK(ep_workspace_bytes(k.n_max, k.n_ports) == 0, "the small path has no workspace");
        constexpr uint32_t NW = kEgSmallThreads / kEgWave;
        uint32_t s_w[NW];
        uint64_t s_m[NW];
        for (uint32_t w = 0; w < NW; ++w) {
            s_m[w] = 0;
            for (uint32_t lane = 0; lane < kEgWave; ++lane) {
                const uint32_t t = w * kEgWave + lane;
                lanes[t].reply = ep_in(t, lo, hi) && k.verdict[t] == XSK_GPU_TX_REPLY;  // (nothing outside is read)
                if (lanes[t].reply) s_m[w] |= 1ull << lane;
            }
            s_w[w] = popc(s_m[w]);
        }
        for (uint32_t b = 0; b <= k.n_ports; ++b) s.g[b] = ep_prefix_at(s_w, s_m, NW, s.o[b]);
        for (uint32_t t = 0; t < kEgSmallThreads; ++t) lanes[t].g_i = ep_prefix_at(s_w, s_m, NW, t);
        for (uint32_t p = 0; p < k.n_ports; ++p) r->c[p] = ep_counts(s.o[p], s.o[p + 1], s.g[p], s.g[p + 1], s.room[p]);
        finish_wg(k, ref, s, 0, kEgSmallThreads, lanes, r, NULL, NULL, 0);
        CHECK(r->port_sets <= k.n_ports, "%s: more per-port sets than ports", k.what);
        return;
    }
    const uint32_t nwg = cp_nwg(k.n_max);
    CHECK(ep_part_offset(k.n_max, k.n_ports) == ((size_t)nwg + k.n_ports + 1) * 4 && sizeof(EpPart) == 32 &&
              ep_workspace_bytes(k.n_max, k.n_ports) == ep_part_offset(k.n_max, k.n_ports) + (size_t)nwg * 32,
          "workspace");
    uint32_t* ws = (uint32_t*)malloc(ep_workspace_bytes(k.n_max, k.n_ports));
    CHECK(ws, "malloc");
    EpPart* part = (EpPart*)((char*)ws + ep_part_offset(k.n_max, k.n_ports));
    uint8_t* wpart = (uint8_t*)calloc(nwg, 1);
    CHECK(wpart, "calloc");
    for (uint32_t wg = 0; wg < nwg; ++wg) {  // stage 1
        uint32_t c = 0;
        for (uint32_t t = 0; t < kEgFrames; ++t) {
            const uint32_t i = wg * kEgFrames + t;
            c += ep_in(i, lo, hi) && k.verdict[i] == XSK_GPU_TX_REPLY;
        }
        ws[wg] = c;
    }
    // stage 2: the scan over runs, then a prefix per boundary
    const uint32_t total = replay_scan_cells(ws, nwg, replay_put_before);
    for (uint32_t b = 0; b <= k.n_ports; ++b) {
        const uint32_t o = s.o[b], wg = ep_bound_wg(o);
        uint32_t g = total;
        if (wg < nwg) {
            const uint32_t from = ep_bound_from(o, lo);
            CHECK(from <= o && o - from < kEgFrames, "%s: more than 255 verdicts in front of a boundary", k.what);
            uint32_t c = 0;
            for (uint32_t q = 0; q < kEgFrames; ++q) {
                const uint32_t i = wg * kEgFrames + q;
                c += i >= from && i < o && k.verdict[i] == XSK_GPU_TX_REPLY;
            }
            g = ws[wg] + c;
        } else {
            CHECK(o == hi, "%s: a boundary behind the last workgroup that is not the end", k.what);
        }
        s.g[b] = ws[nwg + b] = g;
    }
    for (uint32_t p = 0; p < k.n_ports; ++p) r->c[p] = ep_counts(s.o[p], s.o[p + 1], s.g[p], s.g[p + 1], s.room[p]);
    for (uint32_t wg = 0; wg < nwg; ++wg) {  // stage 3
        if (!ep_wg_live(wg, lo, hi)) {
            for (uint32_t t = 0; t < kEgFrames; ++t) {
                const uint64_t i = (uint64_t)wg * kEgFrames + t;
                CHECK(i >= k.n_max || ref.owner[i] < 0, "%s: a workgroup with a listed frame does not run", k.what);
            }
            continue;
        }
        constexpr uint32_t NW = kEgFrames / kEgWave;
        uint32_t s_w[NW];
        uint64_t m[NW];
        for (uint32_t w = 0; w < NW; ++w) {
            m[w] = 0;
            for (uint32_t lane = 0; lane < kEgWave; ++lane) {
                const uint32_t t = w * kEgWave + lane, i = wg * kEgFrames + t;
                lanes[t].reply = ep_in(i, lo, hi) && k.verdict[i] == XSK_GPU_TX_REPLY;
                if (lanes[t].reply) m[w] |= 1ull << lane;
            }
            s_w[w] = popc(m[w]);
        }
        for (uint32_t w = 0; w < NW; ++w)
            for (uint32_t lane = 0; lane < kEgWave; ++lane) {
                uint32_t g_i = ws[wg] + popc(m[w] & ((1ull << lane) - 1ull));
                for (uint32_t q = 0; q < NW; ++q) g_i += q < w ? s_w[q] : 0u;
                lanes[w * kEgWave + lane].g_i = g_i;
            }
        for (uint32_t b = 0; b <= k.n_ports; ++b) s.g[b] = ws[nwg + b];
        finish_wg(k, ref, s, wg * kEgFrames, kEgFrames, lanes, r, part, wpart, wg);
    }
    // stage 4: a workgroup per port over the records of the workgroups whose first position the port owns
    uint64_t records = 0;
    for (uint32_t p = 0; p < k.n_ports; ++p) {
        const uint32_t b = ep_carry_begin(s.o[p]), e = ep_carry_begin(s.o[p + 1]);
        if (b >= e) continue;
        CHECK(e <= nwg, "%s: records behind the grid", k.what);
        r->sum_sets++;
        for (uint32_t wg = b; wg < e; ++wg) {
            CHECK(wpart[wg] == 1 && ref.owner[wg * kEgFrames] == (int32_t)p, "%s: port %u reads record %u", k.what, p, wg);
            ++records;
            r->ps[p].rx_packets += part[wg].n;
            r->ps[p].tx_packets += part[wg].n_tx;
            r->ps[p].rx_bytes += ep_u64(part[wg].bytes_lo, part[wg].bytes_hi);
            r->ps[p].tx_bytes += ep_u64(part[wg].tx_bytes_lo, part[wg].tx_bytes_hi);
        }
    }
    uint64_t written = 0;
    for (uint32_t wg = 0; wg < nwg; ++wg) written += wpart[wg];
    CHECK(written == records, "%s: %llu records written, %llu read", k.what, (unsigned long long)written,
          (unsigned long long)records);
    CHECK(r->port_sets <= k.n_ports && r->sum_sets <= k.n_ports, "%s: %llu + %llu per-port sets for %u ports", k.what,
          (unsigned long long)r->port_sets, (unsigned long long)r->sum_sets, k.n_ports);
    free(wpart);
    free(ws);
}

enum { P_ALL, P_NONE, P_ALT, P_RANDOM, P_LANE0, P_LANE63, P_LAST_WG, P_COUNT };
enum { R_UNLIMITED, R_0, R_RM1, R_R, R_MIXED, R_COUNT };
enum { L_ONE, L_ALL_EMPTY, L_EMPTY_FRONT, L_EMPTY_MID, L_EMPTY_END, L_THREE, L_EDGES, L_RANDOM, L_INNER, L_WILD, L_COUNT };

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

static int cmp_u32(const void* a, const void* b) {
    const uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b;
    return x < y ? -1 : x > y;
}

// Ports [e0, e1) get no frames, the others share [0, n_max) evenly.
static void split_without(uint32_t* w, uint32_t n_ports, uint32_t n_max, uint32_t e0, uint32_t e1) {
    const uint32_t live = n_ports - (e1 - e0);
    uint32_t seen = 0;
    w[0] = 0;
    for (uint32_t p = 0; p < n_ports; ++p) {
        if (p < e0 || p >= e1) ++seen;
        w[p + 1] = live ? (uint32_t)((uint64_t)n_max * seen / live) : 0u;
    }
}

static void fill_layout(uint32_t* w, uint32_t n_ports, uint32_t n_max, int layout) {
    const uint32_t third = n_ports / 3 ? n_ports / 3 : 1;
    switch (layout) {
        case L_ONE:
            w[0] = 0;
            for (uint32_t p = 1; p <= n_ports; ++p) w[p] = n_max;
            break;
        case L_ALL_EMPTY:
            for (uint32_t p = 0; p <= n_ports; ++p) w[p] = n_max / 2;
            break;
        case L_EMPTY_FRONT: split_without(w, n_ports, n_max, 0, n_ports > 1 ? third : 0); break;
        case L_EMPTY_MID: split_without(w, n_ports, n_max, n_ports > 2 ? third : 0, n_ports > 2 ? 2 * third : 0); break;
        case L_EMPTY_END: split_without(w, n_ports, n_max, n_ports > 1 ? n_ports - third : 0, n_ports > 1 ? n_ports : 0); break;
        case L_THREE:  // n_ports segments of 3 frames from frame 5 on: 64 x 3 = 192 frames inside one workgroup
            for (uint32_t p = 0; p <= n_ports; ++p) w[p] = eg_min(5 + 3 * p, n_max);
            break;
        case L_EDGES: {  // on a wave or a workgroup edge, one below, one above
            const uint32_t units = n_max / kEgFrames + 1;
            w[0] = 0;
            for (uint32_t p = 1; p < n_ports; ++p) {
                const uint32_t unit = (p & 1u) ? kEgWave : kEgFrames;
                const uint32_t e = ((p * 37u) % units + 1u) * unit + p % 3u - 1u;
                w[p] = eg_min(e, n_max);
            }
            w[n_ports] = n_max;
            qsort(w, n_ports + 1, sizeof(*w), cmp_u32);
            break;
        }
        case L_RANDOM:
            for (uint32_t p = 0; p <= n_ports; ++p) w[p] = rnd(n_max);
            if (n_ports > 3) w[2] = w[3];  // an empty segment in any case
            qsort(w, n_ports + 1, sizeof(*w), cmp_u32);
            break;
        case L_INNER: {
            const uint32_t a = n_max / 5, b = n_max - n_max / 7;
            for (uint32_t p = 0; p <= n_ports; ++p) w[p] = a + rnd(b - a);
            w[0] = a;
            w[n_ports] = b;
            qsort(w, n_ports + 1, sizeof(*w), cmp_u32);
            break;
        }
        case L_WILD:  // not ascending, above the bound
            for (uint32_t p = 0; p <= n_ports; ++p) w[p] = rnd(n_max + n_max / 2 + 1);
            w[0] = rnd(n_max / 3);
            w[1 + rnd(n_ports - 1)] = (rnd(1) ? 0xFFFFFFFFu : n_max + 5);
            if (n_ports > 1) w[n_ports] = rnd(n_max / 2);  // descending at the end
            break;
    }
}

static uint64_t g_cases = 0;

static void one_case(uint32_t n_max, uint32_t n_ports, int layout, int pattern, int room_kind) {
    char what[96];
    snprintf(what, sizeof(what), "n_max %u ports %u layout %d pattern %d rooms %d", n_max, n_ports, layout, pattern,
             room_kind);
    xsk_gpu_desc* descs = exact<xsk_gpu_desc>(n_max);
    uint8_t* verdict = exact<uint8_t>(n_max);
    uint32_t* words = exact<uint32_t>(n_ports + 1);
    uint32_t* rooms = room_kind == R_UNLIMITED ? NULL : exact<uint32_t>(n_ports);
    fill_verdicts(verdict, n_max, pattern);
    for (uint32_t i = 0; i < n_max; ++i) {
        descs[i].addr = (uint64_t)i * 2048 + rnd(255);
        descs[i].len = 14 + rnd(1500);
        descs[i].options = 1 + rnd(0xFFFFFFF0u);  // never 0: a copied descriptor shows
    }
    fill_layout(words, n_ports, n_max, layout);
    if (rooms) {  // R_p by a loop of its own
        uint32_t run = 0, o[kEpMaxBounds];
        for (uint32_t p = 0; p <= n_ports; ++p) {
            if (words[p] > run) run = words[p];
            o[p] = run < n_max ? run : n_max;
        }
        for (uint32_t p = 0; p < n_ports; ++p) {
            uint32_t R = 0;
            for (uint32_t i = o[p]; i < o[p + 1]; ++i) R += verdict[i] == XSK_GPU_TX_REPLY;
            switch (room_kind) {
                case R_0: rooms[p] = 0; break;
                case R_RM1: rooms[p] = R ? R - 1 : 0; break;
                case R_R: rooms[p] = R; break;
                default:  // mixed: cut and uncut ports side by side
                    rooms[p] = p % 4 == 0 ? 0xFFFFFFFFu : p % 4 == 1 ? 0u : p % 4 == 2 ? (R ? R - 1 : 0) : R / 2;
                    break;
            }
        }
    }
    const Case k = {n_max, n_ports, words, rooms, descs, verdict, what};
    Ref ref;
    Got got;
    ref.tx = exact<xsk_gpu_desc>(n_max);
    ref.fr = exact<uint64_t>(n_max);
    ref.owner = exact<int32_t>(n_max);
    got.tx = exact<xsk_gpu_desc>(n_max);
    got.fr = exact<uint64_t>(n_max);
    got.wtx = exact<uint8_t>(n_max);
    got.wfr = exact<uint8_t>(n_max);
    memset(ref.tx, 0xEE, (size_t)n_max * sizeof(xsk_gpu_desc));
    memset(got.tx, 0xEE, (size_t)n_max * sizeof(xsk_gpu_desc));
    memset(ref.fr, 0xEE, (size_t)n_max * sizeof(uint64_t));
    memset(got.fr, 0xEE, (size_t)n_max * sizeof(uint64_t));
    memset(got.wtx, 0, n_max);
    memset(got.wfr, 0, n_max);
    sequential(k, &ref);
    device_paths(k, ref, &got);
    uint64_t full = 0;
    for (uint32_t p = 0; p < n_ports; ++p) {
        const EgCounts &a = got.c[p], &b = ref.c[p];
        CHECK(a.n == b.n && a.n_tx == b.n_tx && a.n_tx_full == b.n_tx_full && a.n_free == b.n_free,
              "%s: counts of port %u: got %u %u %u %u, want %u %u %u %u", what, p, a.n, a.n_tx, a.n_tx_full, a.n_free, b.n,
              b.n_tx, b.n_tx_full, b.n_free);
        CHECK(b.n_tx + b.n_free == b.n && b.n_tx + b.n_tx_full <= b.n, "reference");
        for (uint32_t j = 0; j < b.n; ++j) {  // every slot of the port's two lists exactly once, nothing behind them
            CHECK(got.wtx[ref.o[p] + j] == (j < b.n_tx), "%s: port %u tx slot %u written %u times", what, p, j,
                  got.wtx[ref.o[p] + j]);
            CHECK(got.wfr[ref.o[p] + j] == (j < b.n_free), "%s: port %u free slot %u written %u times", what, p, j,
                  got.wfr[ref.o[p] + j]);
        }
        CHECK(!memcmp(&got.ps[p], &ref.ps[p], sizeof(PortSums)), "%s: per-port counters of port %u", what, p);
        full += b.n_tx_full;
    }
    CHECK(!memcmp(got.tx, ref.tx, (size_t)n_max * sizeof(xsk_gpu_desc)), "%s: d_tx", what);
    CHECK(!memcmp(got.fr, ref.fr, (size_t)n_max * sizeof(uint64_t)), "%s: d_free", what);
    CHECK(got.lost_packets == ref.lost_packets && got.lost_bytes == ref.lost_bytes && got.lost_packets == full,
          "%s: shared counters", what);
    CHECK(full || !got.shared_sets, "%s: shared atomics with nothing left out", what);
    CHECK(got.shared_sets <= got.workgroups, "%s: more than one shared pair per workgroup", what);
    CHECK(got.port_sets + got.sum_sets <= got.workgroups + n_ports, "%s: %llu per-port sets from %llu workgroups", what,
          (unsigned long long)(got.port_sets + got.sum_sets), (unsigned long long)got.workgroups);
    free(descs);
    free(verdict);
    free(words);
    free(rooms);
    free(ref.tx);
    free(ref.fr);
    free(ref.owner);
    free(got.tx);
    free(got.fr);
    free(got.wtx);
    free(got.wfr);
    ++g_cases;
}

// ep_upper against a linear count, on offsets with repeats.
static void owner_cases(void) {
    for (uint32_t n_ports : {1u, 2u, 8u, 63u, 64u})
        for (int rep = 0; rep < 50; ++rep) {
            uint32_t o[kEpMaxBounds];
            for (uint32_t p = 0; p <= n_ports; ++p) o[p] = rnd(rep % 2 ? 40 : 5000);
            qsort(o, n_ports + 1, sizeof(*o), cmp_u32);
            for (uint32_t i = 0; i < 5002; ++i) {
                uint32_t ub = 0;
                while (ub <= n_ports && o[ub] <= i) ++ub;
                CHECK(ep_upper(o, n_ports, i) == ub, "upper bound");
                const EpOwner w = ep_owner(o, n_ports, i);
                CHECK(w.on == (ub >= 1 && ub <= n_ports), "owner");
                if (w.on) CHECK(o[w.port] <= i && i < o[w.port + 1], "owner's segment is not empty and holds i");
            }
        }
}

int main(void) {
    static_assert(sizeof(xsk_gpu_egress_counts) == sizeof(EgCounts), "counts layout");
    static_assert(kEgSmallMax == XSK_GPU_LOWLAT_MAX && kEpMaxPorts == XSK_GPU_STEER_MAX_PORTS, "bounds");
    owner_cases();
    const uint32_t sizes[] = {1, 64, 65, 1023, 1024, 1025, 4099, 262147, (1u << 20) + 1};
    const uint32_t ports[] = {1, 2, 8, 63, 64};
    for (uint32_t n_max : sizes) {
        uint32_t turn = 0;
        for (uint32_t n_ports : ports)
            for (int layout = 0; layout < L_COUNT; ++layout) {
                if (n_max <= 8192) {
                    for (int p = 0; p < P_COUNT; ++p)
                        for (int rk = 0; rk < R_COUNT; ++rk) one_case(n_max, n_ports, layout, p, rk);
                } else {
                    one_case(n_max, n_ports, layout, (int)(turn % P_COUNT), (int)(turn % R_COUNT));
                    ++turn;
                }
            }
    }
    // the largest bound the call accepts: the sizes stay inside 32 bits
    const uint32_t big = XSK_GPU_MAX_BATCH, nwg = cp_nwg(big);
    CHECK(ep_workspace_bytes(big, 64) == ((size_t)nwg + 65) * 4 + (size_t)nwg * 32 && (uint64_t)nwg * kEgFrames <= 0x100000000ull,
          "largest bound");
    CHECK(ep_carry_begin(big) == nwg && ep_carry_begin(0) == 0 && ep_carry_begin(1) == 1 && ep_carry_begin(256) == 1 &&
              ep_wg_carries(nwg - 1, 0, big) && !ep_wg_carries(0, 1, big),
          "records");
    CHECK(ep_wg_live(nwg - 1, 0, big) && !ep_wg_live(nwg - 1, 0, big - kEgFrames) && !ep_wg_live(0, 7, 7), "live");
    CHECK(ep_bound_wg(big) == nwg && ep_bound_from(big - 1, 0) == big - kEgFrames, "largest bound: the last boundary");
    printf("egress ports ok (%llu cases)\n", (unsigned long long)g_cases);
    return 0;
}
