// The arithmetic of xsk_gpu_rx_prepare_ports_dev() and xsk_gpu_rx_ports_end_dev() (xsknet_amd/csrc/xsk_ring_ports.h)
// compiled for the host: both paths of xsk_ring_ports.hip replayed thread by thread with the header's functions -- the
// one-workgroup path (decide, the rest list by wave ballots, 1024 lanes copy in strides, publish) and the path of kernel
// boundaries (count / scan / scatter of the rest list, a grid of 256-lane workgroups, a one-wave publish) -- and
// compared with a sequential restatement of the rule of include/xsk_gpu.h.  Every ring is a heap allocation of exactly
// `size` entries, the pool of `capacity`, every linear array of n_max, the offsets of n_ports + 1, the compacted rest of
// exactly |rest|; the test builds this file with -fsanitize=address,undefined, so an index one past an array's end is a
// failure here, not a stray store on a device.  Every store into a ring or the pool is also checked: at most once per
// slot, only inside the part that was free when the call began.
//
// 1, 2, 3 and 64 ports; ring sizes 1 to 4096, different per port; index words starting at 0, mid-ring and 0xFFFFFFFD;
// 0 to 1300 frames with bounds on both sides of 1024; port 0's ring full (room 0) and the last port's ring cut below
// its reply count; with three or more ports port 1 gets no frame (an empty segment); a pool that takes none, some and
// all of the list.  With a pool that takes all, every received address ends exactly once on some TX ring or on the
// pool.  Then garbage: offsets, counts, the plan's count and every index word hold anything.  Stand-alone: prints
// "ring ports ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/xsk_gpu.h"
#include "../../xsknet_amd/csrc/xsk_egress_ports.h"
#include "../../xsknet_amd/csrc/xsk_ring_dev.h"
#include "../../xsknet_amd/csrc/xsk_ring_ports.h"
#include "compact_replay.h"

using namespace xskgpu;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {  // xorshift64*
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}

template <class T>
static T* exact(size_t count) {  // exactly count entries (count == 0: a pointer to nothing)
    T* p = (T*)malloc(count * sizeof(T));
    CHECK(p || !count, "malloc");
    return p;
}
template <class T>
static T* copy_of(const T* src, size_t count) {
    T* p = exact<T>(count);
    if (count) memcpy(p, src, count * sizeof(T));
    return p;
}

struct TxRing {
    uint32_t prod, cons, size;
    xsk_gpu_desc* ent;
};
struct State {
    uint32_t rx_prod, rx_cons;  // (end touches the RX ring's consumer word only)
    uint32_t n_ports;
    TxRing tx[kEpMaxPorts];
    uint64_t* pool;
    uint32_t n_free, capacity;
};
struct Inputs {  // what end reads beside the rings: every array exactly as long as the call may index it
    uint32_t n_max, received_word, refilled;
    xsk_gpu_desc* descs;  // n_max
    uint8_t* actions;     // n_max
    uint32_t* off;        // n_ports + 1
    xsk_gpu_desc* d_tx;   // n_max
    uint64_t* d_free;     // n_max
    EgCounts* counts;     // n_ports
};
struct Result {
    uint32_t received, redirected, replied, tx_full, refilled, freed;
};

static State state_copy(const State& s) {
    State c = s;
    for (uint32_t p = 0; p < s.n_ports; ++p) c.tx[p].ent = copy_of(s.tx[p].ent, s.tx[p].size);
    c.pool = copy_of(s.pool, s.capacity);
    return c;
}
static void state_free(State& s) {
    for (uint32_t p = 0; p < s.n_ports; ++p) free(s.tx[p].ent);
    free(s.pool);
}
static void inputs_free(Inputs& in) {
    free(in.descs);
    free(in.actions);
    free(in.off);
    free(in.d_tx);
    free(in.d_free);
    free(in.counts);
}
static void state_same(const State& a, const State& b, const char* tag) {
    CHECK(a.rx_cons == b.rx_cons && a.rx_prod == b.rx_prod, "%s: rx words %u against %u", tag, a.rx_cons, b.rx_cons);
    for (uint32_t p = 0; p < a.n_ports; ++p) {
        CHECK(a.tx[p].prod == b.tx[p].prod && a.tx[p].cons == b.tx[p].cons, "%s: port %u words %u/%u against %u/%u", tag,
              p, a.tx[p].prod, a.tx[p].cons, b.tx[p].prod, b.tx[p].cons);
        CHECK(!memcmp(a.tx[p].ent, b.tx[p].ent, a.tx[p].size * sizeof(xsk_gpu_desc)), "%s: port %u entries differ", tag, p);
    }
    CHECK(a.n_free == b.n_free, "%s: pool count %u against %u", tag, a.n_free, b.n_free);
    CHECK(!memcmp(a.pool, b.pool, rd_pool_n(a.n_free, a.capacity) * sizeof(uint64_t)), "%s: pool stack differs", tag);
}
static void result_same(const Result& a, const Result& b, const char* tag) {
    CHECK(a.received == b.received && a.redirected == b.redirected && a.replied == b.replied && a.tx_full == b.tx_full &&
              a.refilled == b.refilled && a.freed == b.freed,
          "%s: result %u %u %u %u %u %u against %u %u %u %u %u %u", tag, a.received, a.redirected, a.replied, a.tx_full,
          a.refilled, a.freed, b.received, b.redirected, b.replied, b.tx_full, b.refilled, b.freed);
}

// ---- a slot may be stored once, and only inside what was free when the call began ----
struct Guard {
    uint8_t* seen;
    uint32_t first, room, size;  // slots first, first + 1, ... (room of them), modulo size (a ring) or plain
    bool ring;
    Guard(uint32_t first_, uint32_t room_, uint32_t size_, bool ring_) : first(first_), room(room_), size(size_), ring(ring_) {
        seen = exact<uint8_t>(size);
        if (size) memset(seen, 0, size);
    }
    Guard(const Guard&) = delete;
    ~Guard() { free(seen); }
    void hit(uint32_t slot, const char* what) {
        CHECK(slot < size, "%s: slot %u outside", what, slot);
        CHECK(ring || slot >= first, "%s: slot %u below the free part", what, slot);
        const uint32_t off = ring ? ((slot - first) & (size - 1u)) : slot - first;
        CHECK(off < room, "%s: slot %u is not free (first %u room %u)", what, slot, first, room);
        CHECK(!seen[slot], "%s: slot %u stored twice", what, slot);
        seen[slot] = 1;
    }
};

// ---- the device side, thread by thread ----
struct Lanes {  // the (first, stride) of every lane of a copy launch, in turn
    bool small;
    uint32_t nwg;
    template <class F>
    void each(F f) const {
        if (small) {
            for (uint32_t t = 0; t < kRpSmallThreads; ++t) f((uint64_t)t, (uint64_t)kRpSmallThreads);
        } else {
            for (uint32_t wg = 0; wg < nwg; ++wg)
                for (uint32_t lane = 0; lane < kRdCopy; ++lane) f(rd_copy_first(wg, lane), rd_copy_stride(nwg));
        }
    }
};
static Lanes lanes_for(uint32_t bound) { return Lanes{bound <= kRpSmallMax, rd_nwg(bound)}; }

// prepare: d_tx_room (exactly n_ports words) and the pads
static void dev_prepare(const State& s, uint32_t received_word, xsk_gpu_desc* descs, uint32_t n_max, uint32_t* room) {
    Guard gr(0, s.n_ports, s.n_ports, false), gd(0, n_max, n_max, false);
    const uint32_t r = rp_received(received_word, n_max);
    const Lanes l = lanes_for(n_max);
    for (uint32_t lane = 0; lane < (l.small ? kRpSmallThreads : kRdCopy); ++lane)  // (workgroup 0 on the launched path)
        if (lane < s.n_ports) {
            gr.hit(lane, "d_tx_room");
            room[lane] = rd_free(s.tx[lane].prod, s.tx[lane].cons, s.tx[lane].size);
        }
    l.each([&](uint64_t first, uint64_t stride) {
        for (uint64_t i = first; i < n_max; i += stride)
            if (rp_pad((uint32_t)i, r, n_max)) {
                gd.hit((uint32_t)i, "pad");
                memset(&descs[i], 0, sizeof(xsk_gpu_desc));
            }
    });
}

struct Decided {  // EndLds of xsk_ring_ports.hip
    uint32_t raw[kEpMaxBounds], o[kEpMaxBounds], F[kEpMaxBounds];
    uint32_t t[kEpMaxPorts], f[kEpMaxPorts], prod[kEpMaxPorts], full[kEpMaxPorts];
    uint32_t r, pool_n;
};
// end_decide(): each phase ends at a barrier; within a phase a lane per port
static void decide(const State& s, const Inputs& in, Decided* d) {
    const uint32_t np = s.n_ports;
    for (uint32_t p = 0; p <= np; ++p) d->raw[p] = in.off[p];
    d->r = rp_received(in.received_word, in.n_max);
    d->pool_n = rd_pool_n(s.n_free, s.capacity);
    for (uint32_t p = 0; p <= np; ++p) d->o[p] = rp_offset(d->raw, p, in.n_max);
    for (uint32_t p = 0; p < np; ++p) {
        const uint32_t n_p = d->o[p + 1u] - d->o[p];
        d->prod[p] = s.tx[p].prod;
        d->t[p] = rp_port_tx(in.counts[p].n_tx, n_p, rd_free(s.tx[p].prod, s.tx[p].cons, s.tx[p].size));
        d->f[p] = rp_port_free(in.counts[p].n_free, n_p);
        d->full[p] = in.counts[p].n_tx_full;
    }
    for (uint32_t p = 0; p <= np; ++p) d->F[p] = rp_prefix(d->f, p);
}

// The rest list as a workgroup of `threads` lanes at frame `base` leaves it: wave ballots, the counts of the lower
// waves, the lanes below.  Returns the workgroup's count; with `rest`, stores at wg_offset + rank.
static uint32_t wg_rest(const Inputs& in, uint32_t r, uint64_t base, uint32_t threads, uint32_t wg_offset, uint64_t* rest,
                        Guard* g) {
    uint32_t below = 0;
    for (uint32_t t = 0; t < threads; ++t) {
        const uint64_t i = base + t;
        const bool hit = i < r && rp_rest((uint32_t)i, r, in.actions[i]);
        if (!hit) continue;
        if (rest) {
            g->hit(wg_offset + below, "rest");
            rest[wg_offset + below] = in.descs[i].addr;
        }
        below++;
    }
    return below;
}

static Result dev_end(State& s, const Inputs& in) {
    const uint32_t np = s.n_ports, n_max = in.n_max;
    Decided d;
    decide(s, in, &d);
    // the rest list
    uint64_t* rest;
    uint32_t n_rest;
    if (n_max <= kRpSmallMax) {
        n_rest = wg_rest(in, d.r, 0, kRpSmallThreads, 0, nullptr, nullptr);
        rest = exact<uint64_t>(n_rest);
        Guard g(0, n_rest, n_rest, false);
        wg_rest(in, d.r, 0, kRpSmallThreads, 0, rest, &g);
    } else {
        const uint32_t nwg = cp_nwg(n_max);
        uint32_t* cells = exact<uint32_t>(nwg + 1u);
        for (uint32_t wg = 0; wg < nwg; ++wg) cells[wg] = wg_rest(in, d.r, (uint64_t)wg * kCpFrames, kCpFrames, 0, nullptr, nullptr);
        cells[nwg] = replay_scan_cells(cells, nwg, replay_put_before);
        n_rest = rd_min(cells[nwg], n_max);
        rest = exact<uint64_t>(n_rest);
        Guard g(0, n_rest, n_rest, false);
        for (uint32_t wg = 0; wg < nwg; ++wg) wg_rest(in, d.r, (uint64_t)wg * kCpFrames, kCpFrames, cells[wg], rest, &g);
        free(cells);
    }
    // the copy
    std::vector<Guard*> gt;
    for (uint32_t p = 0; p < np; ++p)
        gt.push_back(new Guard(rd_slot(s.tx[p].prod, s.tx[p].size), rd_free(s.tx[p].prod, s.tx[p].cons, s.tx[p].size),
                               s.tx[p].size, true));
    Guard gp(d.pool_n, s.capacity - d.pool_n, s.capacity, false);
    const uint32_t pushed = rp_pushed(d.F[np], n_rest, s.capacity, d.pool_n);
    lanes_for(n_max).each([&](uint64_t first, uint64_t stride) {
        for (uint64_t j = first; j < d.o[np]; j += stride) {
            const RpTx x = rp_tx_lane(d.o, d.t, np, (uint32_t)j);
            if (!x.on) continue;
            CHECK(x.port < np, "tx owner");
            const uint32_t slot = rd_slot(d.prod[x.port] + x.k, s.tx[x.port].size);
            gt[x.port]->hit(slot, "tx ring");
            s.tx[x.port].ent[slot] = in.d_tx[j];
        }
        for (uint64_t L = first; L < pushed; L += stride) {
            const RpSrc src = rp_pool_src(d.F, d.o, np, (uint32_t)L);
            gp.hit(d.pool_n + (uint32_t)L, "pool");
            CHECK(src.rest ? src.idx < n_rest : src.idx < n_max, "pool source");
            s.pool[d.pool_n + (uint32_t)L] = src.rest ? rest[src.idx] : in.d_free[src.idx];
        }
    });
    for (Guard* g : gt) delete g;
    free(rest);
    // publish
    Result res = {d.r, d.o[np], 0, 0, in.refilled, pushed};
    for (uint32_t p = 0; p < np; ++p) {
        if (d.t[p]) s.tx[p].prod = d.prod[p] + d.t[p];
        res.replied += d.t[p];
        res.tx_full += d.full[p];
    }
    s.n_free = d.pool_n + pushed;
    if (d.r) s.rx_cons += d.r;
    return res;
}

// ---- the rule of include/xsk_gpu.h, sequentially, for any content of the words ----
static uint32_t min2(uint32_t a, uint32_t b) { return a < b ? a : b; }
static Result spec_end(State& s, const Inputs& in, std::vector<uint64_t>* tx_addrs, std::vector<uint64_t>* pool_addrs,
                       bool* all_pushed) {
    const uint32_t np = s.n_ports, n_max = in.n_max;
    std::vector<uint32_t> o(np + 1u);
    uint32_t run = 0;
    for (uint32_t p = 0; p <= np; ++p) {
        run = run > in.off[p] ? run : in.off[p];
        o[p] = min2(run, n_max);
    }
    const uint32_t r = min2(in.received_word, n_max);
    Result res = {r, o[np], 0, 0, in.refilled, 0};
    std::vector<uint64_t> list;
    for (uint32_t p = 0; p < np; ++p) {
        TxRing& t = s.tx[p];
        const uint32_t n_p = o[p + 1u] - o[p], used = min2(t.prod - t.cons, t.size);
        const uint32_t t_p = min2(min2(in.counts[p].n_tx, n_p), t.size - used);
        for (uint32_t k = 0; k < t_p; ++k) {
            t.ent[(t.prod + k) & (t.size - 1u)] = in.d_tx[o[p] + k];
            if (tx_addrs) tx_addrs->push_back(in.d_tx[o[p] + k].addr);
        }
        t.prod += t_p;
        res.replied += t_p;
        res.tx_full += in.counts[p].n_tx_full;
        for (uint32_t j = 0; j < min2(in.counts[p].n_free, n_p); ++j) list.push_back(in.d_free[o[p] + j]);
    }
    for (uint32_t i = 0; i < r; ++i)
        if (in.actions[i] != XSK_GPU_XDP_REDIRECT) list.push_back(in.descs[i].addr);
    const uint32_t pool_n = min2(s.n_free, s.capacity);
    const uint32_t pushed = (uint32_t)std::min<uint64_t>(list.size(), s.capacity - pool_n);
    for (uint32_t j = 0; j < pushed; ++j) {
        s.pool[pool_n + j] = list[j];
        if (pool_addrs) pool_addrs->push_back(list[j]);
    }
    s.n_free = pool_n + pushed;
    s.rx_cons += r;
    res.freed = pushed;
    if (all_pushed) *all_pushed = pushed == list.size();
    return res;
}

// ---- building a case ----
static uint64_t g_frame = 1;  // every frame address of a run is distinct
static xsk_gpu_desc fresh_desc() {
    xsk_gpu_desc d;
    const uint64_t k = g_frame++;
    d.addr = k * 2048u + (k * 37u) % 256u;
    d.len = 60u + (uint32_t)(k % 1400u);
    d.options = 0x1000u + (uint32_t)(k & 0xFFFFFFu);
    return d;
}
static bool reply_of(const xsk_gpu_desc& d) { return (d.addr / 2048u) % 3u != 0; }

static TxRing make_tx(uint32_t size, uint32_t start, uint32_t room) {
    TxRing t;
    t.size = size;
    t.cons = start;
    t.prod = start + (size - room);
    t.ent = exact<xsk_gpu_desc>(size);
    for (uint32_t i = 0; i < size; ++i) t.ent[i] = fresh_desc();  // unconsumed entries and stale ones: all distinct
    return t;
}

static const uint32_t kSizes[] = {1u, 2u, 8u, 64u, 512u, 4096u};
static uint64_t g_cases = 0, g_cut = 0, g_conserved = 0, g_tail = 0;

// `frames` received frames steered to n_ports ports and served by the egress's rule; pool_kind 0: full (takes none),
// 1: room for about half the list, 2: room for all.
static void steered_case(uint32_t n_ports, uint32_t start, uint32_t frames, uint32_t n_max, int pool_kind, uint32_t seed) {
    char tag[160];
    snprintf(tag, sizeof tag, "ports %u start %u frames %u n_max %u pool %d seed %u", n_ports, start, frames, n_max,
             pool_kind, seed);
    CHECK(frames <= n_max, "%s: case", tag);
    Inputs in;
    in.n_max = n_max;
    in.received_word = frames;
    in.refilled = seed * 3u + 1u;
    in.descs = exact<xsk_gpu_desc>(n_max);
    in.actions = exact<uint8_t>(n_max);
    std::vector<uint8_t> port(n_max, 0xFF);
    for (uint32_t i = 0; i < n_max; ++i) {
        if (i < frames) {
            in.descs[i] = fresh_desc();
            const uint32_t k = (uint32_t)(rnd64() % 10u);
            in.actions[i] = k < 6u ? XSK_GPU_XDP_REDIRECT : k < 8u ? XSK_GPU_XDP_DROP : XSK_GPU_XDP_PASS;
            if (in.actions[i] == XSK_GPU_XDP_REDIRECT) {
                uint32_t p = (uint32_t)(rnd64() % n_ports);
                if (n_ports >= 3u && p == 1u) p = 2u;  // port 1: an empty segment
                port[i] = (uint8_t)p;
            }
        } else {
            memset(&in.descs[i], 0xCC, sizeof(xsk_gpu_desc));  // prepare pads these below
            in.actions[i] = XSK_GPU_XDP_DROP;
        }
    }
    // the steered list and its offsets (xsk_gpu_steer_dev(): a stable partition by port)
    std::vector<xsk_gpu_desc> out;
    in.off = exact<uint32_t>(n_ports + 1u);
    for (uint32_t p = 0; p < n_ports; ++p) {
        in.off[p] = (uint32_t)out.size();
        for (uint32_t i = 0; i < frames; ++i)
            if (port[i] == p) out.push_back(in.descs[i]);
    }
    in.off[n_ports] = (uint32_t)out.size();
    // the rings: port 0 full, the last port cut below its replies, the others empty; sizes differ per port
    State s;
    s.n_ports = n_ports;
    s.rx_cons = start;
    s.rx_prod = start + frames;
    for (uint32_t p = 0; p < n_ports; ++p) {
        uint32_t R = 0;
        for (uint32_t i = in.off[p]; i < in.off[p + 1u]; ++i) R += reply_of(out[i]);
        const uint32_t size = kSizes[(p * 5u + seed) % 6u];
        uint32_t room = size;
        if (p == 0u && n_ports > 1u) room = 0u;
        if (p == n_ports - 1u && R) room = min2(R - 1u, size);
        s.tx[p] = make_tx(size, start + 2u * p, room);
    }
    // prepare, replayed: the rooms and the pads
    uint32_t* room = exact<uint32_t>(n_ports);
    dev_prepare(s, frames, in.descs, n_max, room);
    for (uint32_t i = frames; i < n_max; ++i)
        CHECK(in.descs[i].addr == 0 && in.descs[i].len == 0 && in.descs[i].options == 0, "%s: pad %u", tag, i);
    // the egress's rule per port (its own arithmetic is tests/c/test_egress_ports.cpp's)
    in.d_tx = exact<xsk_gpu_desc>(n_max);
    in.d_free = exact<uint64_t>(n_max);
    memset(in.d_tx, 0xEE, n_max * sizeof(xsk_gpu_desc));
    memset(in.d_free, 0xEE, n_max * sizeof(uint64_t));
    in.counts = exact<EgCounts>(n_ports);
    uint32_t cut = 0;
    for (uint32_t p = 0; p < n_ports; ++p) {
        CHECK(room[p] == rd_free(s.tx[p].prod, s.tx[p].cons, s.tx[p].size), "%s: room %u", tag, p);
        const uint32_t o_p = in.off[p];
        uint32_t nt = 0, nf = 0, R = 0;
        for (uint32_t i = o_p; i < in.off[p + 1u]; ++i) {
            if (reply_of(out[i]) && nt < room[p]) {
                in.d_tx[o_p + nt].addr = out[i].addr;
                in.d_tx[o_p + nt].len = out[i].len;
                in.d_tx[o_p + nt].options = 0;
                nt++;
            } else {
                in.d_free[o_p + nf++] = out[i].addr;
            }
            R += reply_of(out[i]);
        }
        in.counts[p] = eg_counts(in.off[p + 1u] - o_p, R, room[p]);
        CHECK(in.counts[p].n_tx == nt && in.counts[p].n_free == nf, "%s: egress lists", tag);
        cut += in.counts[p].n_tx_full;
    }
    free(room);
    // the pool
    const uint32_t list = frames;  // every received frame is on exactly one list, or on a TX ring
    s.capacity = frames + 5u;
    s.n_free = pool_kind == 0 ? s.capacity : pool_kind == 1 ? s.capacity - list / 2u : 3u;
    s.pool = exact<uint64_t>(s.capacity);
    for (uint32_t i = 0; i < s.capacity; ++i) s.pool[i] = (g_frame++) * 2048u;

    State d = state_copy(s), sp = state_copy(s);
    std::vector<uint64_t> tx_addrs, pool_addrs;
    bool all_pushed = false;
    const Result rd = dev_end(d, in), rs = spec_end(sp, in, &tx_addrs, &pool_addrs, &all_pushed);
    result_same(rd, rs, tag);
    state_same(d, sp, tag);
    CHECK(rs.received == frames && rs.redirected == out.size() && rs.tx_full == cut, "%s: counts", tag);
    if (frames == 0) state_same(d, s, tag);  // nothing received: nothing changes
    if (all_pushed) {  // conservation: every received address exactly once, on a TX ring or on the pool
        std::vector<uint64_t> got(tx_addrs), want;
        got.insert(got.end(), pool_addrs.begin(), pool_addrs.end());
        for (uint32_t i = 0; i < frames; ++i) want.push_back(in.descs[i].addr);
        std::sort(got.begin(), got.end());
        std::sort(want.begin(), want.end());
        CHECK(got == want, "%s: conservation", tag);
        g_conserved++;
    } else {
        g_tail++;
    }
    g_cut += cut != 0;
    state_free(d);
    state_free(sp);
    state_free(s);
    inputs_free(in);
    g_cases++;
}

// Garbage: every word holds anything.  The device side against the rule, and never outside an array.
static void garbage_case(uint32_t n_ports, uint32_t n_max, uint32_t k) {
    char tag[100];
    snprintf(tag, sizeof tag, "garbage ports %u n_max %u case %u", n_ports, n_max, k);
    auto word = [&](uint32_t sane) { return rnd64() % 3u ? (uint32_t)rnd64() : sane; };
    Inputs in;
    in.n_max = n_max;
    in.received_word = k % 2u ? (uint32_t)rnd64() : (uint32_t)(rnd64() % (n_max + 1u));
    in.refilled = (uint32_t)rnd64();
    in.descs = exact<xsk_gpu_desc>(n_max);
    in.actions = exact<uint8_t>(n_max);
    in.d_tx = exact<xsk_gpu_desc>(n_max);
    in.d_free = exact<uint64_t>(n_max);
    for (uint32_t i = 0; i < n_max; ++i) {
        in.descs[i] = fresh_desc();
        in.d_tx[i] = fresh_desc();
        in.d_free[i] = (g_frame++) * 2048u;
        in.actions[i] = (uint8_t)(rnd64() % 6u);
    }
    in.off = exact<uint32_t>(n_ports + 1u);
    in.counts = exact<EgCounts>(n_ports);
    State s;
    s.n_ports = n_ports;
    s.rx_cons = (uint32_t)rnd64();
    s.rx_prod = (uint32_t)rnd64();
    for (uint32_t p = 0; p <= n_ports; ++p)
        in.off[p] = rnd64() % 4u ? (uint32_t)(rnd64() % (n_max + n_max / 2u + 2u)) : (uint32_t)rnd64();
    for (uint32_t p = 0; p < n_ports; ++p) {
        in.counts[p] = EgCounts{(uint32_t)rnd64(), word((uint32_t)(rnd64() % (n_max + 1u))), (uint32_t)rnd64() >> 8,
                                word((uint32_t)(rnd64() % (n_max + 1u)))};
        const uint32_t size = kSizes[(p + k) % 6u];
        s.tx[p] = make_tx(size, (uint32_t)rnd64(), (uint32_t)(rnd64() % (size + 1u)));
        s.tx[p].prod = word(s.tx[p].prod);
        s.tx[p].cons = word(s.tx[p].cons);
    }
    s.capacity = 1u + (uint32_t)(rnd64() % (2u * n_max + 8u));
    s.n_free = k % 4u == 0 ? s.capacity + 1u + (uint32_t)(rnd64() % 1000u) : word((uint32_t)(rnd64() % (s.capacity + 1u)));
    s.pool = exact<uint64_t>(s.capacity);
    for (uint32_t i = 0; i < s.capacity; ++i) s.pool[i] = (g_frame++) * 2048u;
    State d = state_copy(s), sp = state_copy(s);
    const Result rd = dev_end(d, in), rs = spec_end(sp, in, nullptr, nullptr, nullptr);
    result_same(rd, rs, tag);
    state_same(d, sp, tag);
    // prepare over the same words
    uint32_t* room = exact<uint32_t>(n_ports);
    xsk_gpu_desc* before = copy_of(in.descs, n_max);
    dev_prepare(s, in.received_word, in.descs, n_max, room);
    const uint32_t r = min2(in.received_word, n_max);
    CHECK(!r || !memcmp(before, in.descs, r * sizeof(xsk_gpu_desc)), "%s: prepare touched a received entry", tag);
    for (uint32_t i = r; i < n_max; ++i) CHECK(in.descs[i].addr == 0 && in.descs[i].len == 0, "%s: pad", tag);
    for (uint32_t p = 0; p < n_ports; ++p) {
        const uint32_t used = min2(s.tx[p].prod - s.tx[p].cons, s.tx[p].size);
        CHECK(room[p] == s.tx[p].size - used, "%s: room", tag);
    }
    free(room);
    free(before);
    state_free(d);
    state_free(sp);
    state_free(s);
    inputs_free(in);
    g_cases++;
}

int main() {
    // the layouts: aligned, disjoint, in order
    const uint32_t bounds[] = {1u, 63u, 64u, 1024u, 1025u, 1300u, 65536u, XSK_GPU_MAX_BATCH};
    const uint32_t ports[] = {1u, 2u, 3u, 64u};
    for (uint32_t mb : bounds)
        for (uint32_t np : ports) {
            const size_t sb = (size_t)cp_nwg(mb) * np * 4u, eb = ep_workspace_bytes(mb, np);
            const RpLayout l = rp_layout(mb, np, sb, eb);
            CHECK(l.plan == 0 && l.room == 32 && l.off == l.room + np * 4u && l.counts == l.off + (np + 1u) * 4u, "layout head");
            CHECK(l.descs >= l.counts + np * 16u && l.descs % 16 == 0 && l.out == l.descs + (size_t)mb * 16 &&
                      l.tx == l.out + (size_t)mb * 16 && l.free_list == l.tx + (size_t)mb * 16 && l.free_list % 8 == 0,
                  "layout lists");
            CHECK(l.verdicts == l.free_list + (size_t)mb * 8 && l.actions == l.verdicts + mb && l.ports == l.actions + mb &&
                      l.steer >= l.ports + mb && l.steer % 4 == 0 && l.egress >= l.steer + sb && l.egress % 4 == 0,
                  "layout bytes");
            CHECK(l.end >= l.egress + eb && l.end % 16 == 0 && l.bytes >= l.end + rp_end_workspace_bytes(mb) && l.bytes % 16 == 0,
                  "layout tail");
            if (mb > kRpSmallMax)
                CHECK(rp_end_rest(mb) == 0 && rp_end_cells(mb) == (size_t)mb * 8 &&
                          rp_end_total(mb) == rp_end_cells(mb) + (size_t)cp_nwg(mb) * 4 &&
                          rp_end_workspace_bytes(mb) >= rp_end_total(mb) + 4,
                      "end workspace");
            else
                CHECK(rp_end_workspace_bytes(mb) == 0, "no end workspace on the one-workgroup path");
        }

    const uint32_t starts[] = {0u, 0x12345u * 64u + 31u, 0xFFFFFFFDu};
    const uint32_t frames[] = {0u, 1u, 63u, 64u, 65u, 300u, 1024u, 1025u, 1300u};
    uint32_t seed = 0;
    for (uint32_t np : ports)
        for (uint32_t start : starts)
            for (uint32_t fr : frames) {
                const uint32_t maxes[] = {fr ? fr : 1u, fr + 7u, 1025u + fr};
                for (uint32_t n_max : maxes)
                    for (int pool_kind = 0; pool_kind < 3; ++pool_kind) steered_case(np, start, fr, n_max, pool_kind, seed++);
            }
    for (uint32_t np : ports)
        for (uint32_t k = 0; k < 150; ++k)
            garbage_case(np, k % 2u ? 1u + (uint32_t)(rnd64() % 1024u) : 1025u + (uint32_t)(rnd64() % 400u), k);
    CHECK(g_cut > 50 && g_conserved > 100 && g_tail > 100, "the cases never cut (%llu), conserved (%llu) or dropped (%llu)",
          (unsigned long long)g_cut, (unsigned long long)g_conserved, (unsigned long long)g_tail);
    printf("ring ports ok: %llu cases, %llu with a reply left out, %llu conserved, %llu with the pool's tail dropped\n",
           (unsigned long long)g_cases, (unsigned long long)g_cut, (unsigned long long)g_conserved,
           (unsigned long long)g_tail);
    return 0;
}
