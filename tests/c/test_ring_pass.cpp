// The arithmetic of xsk_gpu_rx_pass_end_dev() (xsknet_amd/csrc/xsk_ring_pass.h over xsk_ring_ports.h) compiled for the
// host: both paths of xsk_ring_pass.hip replayed thread by thread with the headers' functions -- the one-workgroup path
// (decide, two ballots per wave, the taken PASS descriptors onto the stack ring and the rest into the workgroup's list,
// 1024 lanes copy in strides, publish) and the path of kernel boundaries (count / scan / scatter over two count rows, a
// grid of 256-lane workgroups, a one-wave publish) -- and compared with a sequential restatement of the rule of
// include/xsk_gpu.h.  Every ring is a heap allocation of exactly `size` entries, the pool of `capacity`, every linear
// array of n_max, the offsets of n_ports + 1, the compacted rest of exactly N - s; the test builds this file with
// -fsanitize=address,undefined, so an index one past an array's end is a failure here, not a stray store on a device.
// Every store into a ring or the pool is also checked: at most once per slot, only inside the part that was free when
// the call began.
//
// 1, 3 and 64 ports; stack ring sizes 1 to 4096 and no stack ring; the stack ring's producer word at 0, mid-ring and
// 0xFFFFFFFD; 0 to 1300 frames with bounds on both sides of 1024 (255, 256, 257, 1024, 1025 among them); room_s of 0, 1,
// Q - 1, Q and above; mixed, all-PASS, no-PASS and all-REDIRECT batches; a pool that takes none, some and all of the
// list.  With a pool that takes all, every received address ends exactly once on some TX ring, on the stack ring or on
// the pool.  Without a stack ring, or with a full one, the call leaves what xsk_gpu_rx_ports_end_dev()'s rule leaves.
// Then garbage: actions, offsets, counts, the plan's count and every index word hold anything.  Stand-alone: prints
// "ring pass ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/xsk_gpu.h"
#include "../../xsknet_amd/csrc/xsk_egress_ports.h"
#include "../../xsknet_amd/csrc/xsk_ring_dev.h"
#include "../../xsknet_amd/csrc/xsk_ring_pass.h"
#include "../../xsknet_amd/csrc/xsk_ring_ports.h"
#include "compact_replay.h"

using namespace xskgpu;

static uint64_t g_rng = 0xD1B54A32D192ED03ull;
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

struct DescRing {
    uint32_t prod, cons, size;
    xsk_gpu_desc* ent;
};
struct State {
    uint32_t rx_prod, rx_cons;  // (end touches the RX ring's consumer word only)
    uint32_t n_ports;
    DescRing tx[kEpMaxPorts];
    bool has_stack;
    DescRing stack;
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
    uint32_t received, redirected, replied, tx_full, refilled, freed, passed, pass_full;
};

static State state_copy(const State& s) {
    State c = s;
    for (uint32_t p = 0; p < s.n_ports; ++p) c.tx[p].ent = copy_of(s.tx[p].ent, s.tx[p].size);
    if (s.has_stack) c.stack.ent = copy_of(s.stack.ent, s.stack.size);
    c.pool = copy_of(s.pool, s.capacity);
    return c;
}
static void state_free(State& s) {
    for (uint32_t p = 0; p < s.n_ports; ++p) free(s.tx[p].ent);
    if (s.has_stack) free(s.stack.ent);
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
static void ring_same(const DescRing& a, const DescRing& b, const char* tag, const char* what, uint32_t p) {
    CHECK(a.prod == b.prod && a.cons == b.cons, "%s: %s %u words %u/%u against %u/%u", tag, what, p, a.prod, a.cons, b.prod,
          b.cons);
    CHECK(!memcmp(a.ent, b.ent, a.size * sizeof(xsk_gpu_desc)), "%s: %s %u entries differ", tag, what, p);
}
// (with_stack false: a compares a state that has a stack ring with one that has none)
static void state_same(const State& a, const State& b, const char* tag, bool with_stack = true) {
    CHECK(a.rx_cons == b.rx_cons && a.rx_prod == b.rx_prod, "%s: rx words %u against %u", tag, a.rx_cons, b.rx_cons);
    for (uint32_t p = 0; p < a.n_ports; ++p) ring_same(a.tx[p], b.tx[p], tag, "port", p);
    if (with_stack) {
        CHECK(a.has_stack == b.has_stack, "%s: stack", tag);
        if (a.has_stack) ring_same(a.stack, b.stack, tag, "stack", 0);
    }
    CHECK(a.n_free == b.n_free, "%s: pool count %u against %u", tag, a.n_free, b.n_free);
    CHECK(!memcmp(a.pool, b.pool, rd_pool_n(a.n_free, a.capacity) * sizeof(uint64_t)), "%s: pool stack differs", tag);
}
static void result_same(const Result& a, const Result& b, const char* tag) {
    CHECK(!memcmp(&a, &b, sizeof a), "%s: result %u %u %u %u %u %u %u %u against %u %u %u %u %u %u %u %u", tag, a.received,
          a.redirected, a.replied, a.tx_full, a.refilled, a.freed, a.passed, a.pass_full, b.received, b.redirected,
          b.replied, b.tx_full, b.refilled, b.freed, b.passed, b.pass_full);
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
            for (uint32_t t = 0; t < kPsSmallThreads; ++t) f((uint64_t)t, (uint64_t)kPsSmallThreads);
        } else {
            for (uint32_t wg = 0; wg < nwg; ++wg)
                for (uint32_t lane = 0; lane < kRdCopy; ++lane) f(rd_copy_first(wg, lane), rd_copy_stride(nwg));
        }
    }
};
static Lanes lanes_for(uint32_t bound) { return Lanes{bound <= kPsSmallMax, rd_nwg(bound)}; }

struct Decided {  // EndLds of xsk_ring_ports_device.h
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

// stack_words() and pass_plan() of xsk_ring_pass.hip
struct Plan {
    uint32_t prod, taken, full, n_rest;
};
static Plan plan_of(const State& s, uint32_t n_total, uint32_t q_total) {
    Plan p;
    p.prod = s.has_stack ? s.stack.prod : 0u;
    const uint32_t room = ps_room(s.has_stack, p.prod, s.has_stack ? s.stack.cons : 0u, s.has_stack ? s.stack.size : 1u);
    p.taken = ps_taken(q_total, room);
    p.full = q_total - p.taken;
    p.n_rest = ps_n_rest(n_total, p.taken);
    return p;
}

// A workgroup of `threads` lanes (waves of kCpWave) at frame `base`: the two ballots of every wave, their counts.  With
// `plan`, every lane with nr set then places its frame: rank = the row's workgroup offset + the counts of the lower
// waves + the ballot bits below the lane; onto the stack ring or into `rest`.  Returns the workgroup's two counts.
struct WgCounts {
    uint32_t n, q;
};
static WgCounts wg_pass(State& s, const Inputs& in, uint32_t r, uint64_t base, uint32_t threads, uint32_t off_n,
                        uint32_t off_q, const Plan* plan, uint64_t* rest, Guard* g_rest, Guard* g_stack) {
    const uint32_t waves = threads / kCpWave;
    std::vector<uint64_t> mn(waves, 0), mq(waves, 0);
    std::vector<uint32_t> wn(waves, 0), wq(waves, 0);
    for (uint32_t t = 0; t < threads; ++t) {
        const uint64_t i = base + t;
        const uint8_t a = i < r ? in.actions[i] : (uint8_t)XSK_GPU_XDP_REDIRECT;
        if (i < r && rp_rest((uint32_t)i, r, a)) mn[t / kCpWave] |= 1ull << (t % kCpWave);
        if (i < r && ps_pass((uint32_t)i, r, a)) mq[t / kCpWave] |= 1ull << (t % kCpWave);
    }
    WgCounts c = {0, 0};
    for (uint32_t w = 0; w < waves; ++w) {
        wn[w] = (uint32_t)__builtin_popcountll(mn[w]);
        wq[w] = (uint32_t)__builtin_popcountll(mq[w]);
        c.n += wn[w];
        c.q += wq[w];
    }
    if (!plan) return c;
    for (uint32_t t = 0; t < threads; ++t) {
        const uint32_t w = t / kCpWave, lane = t % kCpWave;
        if (!(mn[w] >> lane & 1u)) continue;
        const uint64_t i = base + t, below = (1ull << lane) - 1ull;
        uint32_t n_i = off_n, q_i = off_q;
        for (uint32_t k = 0; k < w; ++k) {
            n_i += wn[k];
            q_i += wq[k];
        }
        n_i += (uint32_t)__builtin_popcountll(mn[w] & below);
        q_i += (uint32_t)__builtin_popcountll(mq[w] & below);
        if (ps_on_stack(mq[w] >> lane & 1u, q_i, plan->taken)) {
            CHECK(s.has_stack, "a stack entry without a stack ring");
            const uint32_t slot = ps_stack_slot(plan->prod, q_i, s.stack.size);
            g_stack->hit(slot, "stack ring");
            s.stack.ent[slot] = in.descs[i];
        } else {
            const uint32_t pos = ps_rest_pos(n_i, q_i, plan->taken);
            g_rest->hit(pos, "rest");
            rest[pos] = in.descs[i].addr;
        }
    }
    return c;
}

static Result dev_end(State& s, const Inputs& in) {
    const uint32_t np = s.n_ports, n_max = in.n_max;
    Decided d;
    decide(s, in, &d);
    Guard g_stack(s.has_stack ? rd_slot(s.stack.prod, s.stack.size) : 0u,
                  s.has_stack ? rd_free(s.stack.prod, s.stack.cons, s.stack.size) : 0u, s.has_stack ? s.stack.size : 0u,
                  true);
    Plan plan;
    uint64_t* rest;
    if (n_max <= kPsSmallMax) {
        const WgCounts c = wg_pass(s, in, d.r, 0, kPsSmallThreads, 0, 0, nullptr, nullptr, nullptr, nullptr);
        plan = plan_of(s, c.n, c.q);
        rest = exact<uint64_t>(plan.n_rest);
        Guard g(0, plan.n_rest, plan.n_rest, false);
        wg_pass(s, in, d.r, 0, kPsSmallThreads, 0, 0, &plan, rest, &g, &g_stack);
    } else {
        const uint32_t nwg = cp_nwg(n_max);
        CHECK(ps_end_row(n_max, kPsRowPass) - ps_end_row(n_max, kPsRowRest) == (size_t)nwg * 4u, "rows");
        uint32_t* cells = exact<uint32_t>((size_t)kPsRows * nwg + kPsRows);  // the two rows, the two totals
        uint32_t *row_n = cells + kPsRowRest * nwg, *row_q = cells + kPsRowPass * nwg, *totals = cells + kPsRows * nwg;
        for (uint32_t wg = 0; wg < nwg; ++wg) {
            const WgCounts c = wg_pass(s, in, d.r, (uint64_t)wg * kCpFrames, kCpFrames, 0, 0, nullptr, nullptr, nullptr, nullptr);
            row_n[wg] = c.n;
            row_q[wg] = c.q;
        }
        totals[kPsRowRest] = replay_scan_cells(row_n, nwg, replay_put_before);
        totals[kPsRowPass] = replay_scan_cells(row_q, nwg, replay_put_before);
        const uint32_t n_total = ps_total_rest(totals[kPsRowRest], n_max);
        plan = plan_of(s, n_total, ps_total_pass(totals[kPsRowPass], n_total));
        rest = exact<uint64_t>(plan.n_rest);
        Guard g(0, plan.n_rest, plan.n_rest, false);
        for (uint32_t wg = 0; wg < nwg; ++wg)
            wg_pass(s, in, d.r, (uint64_t)wg * kCpFrames, kCpFrames, row_n[wg], row_q[wg], &plan, rest, &g, &g_stack);
        free(cells);
    }
    const uint32_t n_rest = plan.n_rest;
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
    Result res = {d.r, d.o[np], 0, 0, in.refilled, pushed, plan.taken, plan.full};
    for (uint32_t p = 0; p < np; ++p) {
        if (d.t[p]) s.tx[p].prod = d.prod[p] + d.t[p];
        res.replied += d.t[p];
        res.tx_full += d.full[p];
    }
    s.n_free = d.pool_n + pushed;
    if (d.r) s.rx_cons += d.r;
    if (plan.taken) s.stack.prod = plan.prod + plan.taken;
    return res;
}

// ---- the rule of include/xsk_gpu.h, sequentially, for any content of the words ----
static uint32_t min2(uint32_t a, uint32_t b) { return a < b ? a : b; }
struct Where {  // where the received addresses went
    std::vector<uint64_t> tx, stack, pool;
    bool all_pushed;
};
static Result spec_end(State& s, const Inputs& in, bool use_stack, Where* w) {
    const uint32_t np = s.n_ports, n_max = in.n_max;
    std::vector<uint32_t> o(np + 1u);
    uint32_t run = 0;
    for (uint32_t p = 0; p <= np; ++p) {
        run = run > in.off[p] ? run : in.off[p];
        o[p] = min2(run, n_max);
    }
    const uint32_t r = min2(in.received_word, n_max);
    Result res = {r, o[np], 0, 0, in.refilled, 0, 0, 0};
    std::vector<uint64_t> list;
    for (uint32_t p = 0; p < np; ++p) {
        DescRing& t = s.tx[p];
        const uint32_t n_p = o[p + 1u] - o[p], used = min2(t.prod - t.cons, t.size);
        const uint32_t t_p = min2(min2(in.counts[p].n_tx, n_p), t.size - used);
        for (uint32_t k = 0; k < t_p; ++k) {
            t.ent[(t.prod + k) & (t.size - 1u)] = in.d_tx[o[p] + k];
            if (w) w->tx.push_back(in.d_tx[o[p] + k].addr);
        }
        t.prod += t_p;
        res.replied += t_p;
        res.tx_full += in.counts[p].n_tx_full;
        for (uint32_t j = 0; j < min2(in.counts[p].n_free, n_p); ++j) list.push_back(in.d_free[o[p] + j]);
    }
    uint32_t room_s = 0;
    if (use_stack && s.has_stack) room_s = s.stack.size - min2(s.stack.prod - s.stack.cons, s.stack.size);
    for (uint32_t i = 0; i < r; ++i) {
        if (in.actions[i] == XSK_GPU_XDP_REDIRECT) continue;
        if (in.actions[i] == XSK_GPU_XDP_PASS) {
            if (res.passed < room_s) {
                s.stack.ent[(s.stack.prod + res.passed) & (s.stack.size - 1u)] = in.descs[i];
                if (w) w->stack.push_back(in.descs[i].addr);
                res.passed++;
                continue;
            }
            res.pass_full++;
        }
        list.push_back(in.descs[i].addr);
    }
    if (res.passed) s.stack.prod += res.passed;
    const uint32_t pool_n = min2(s.n_free, s.capacity);
    const uint32_t pushed = (uint32_t)std::min<uint64_t>(list.size(), s.capacity - pool_n);
    for (uint32_t j = 0; j < pushed; ++j) {
        s.pool[pool_n + j] = list[j];
        if (w) w->pool.push_back(list[j]);
    }
    s.n_free = pool_n + pushed;
    s.rx_cons += r;
    res.freed = pushed;
    if (w) w->all_pushed = pushed == list.size();
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

static DescRing make_ring(uint32_t size, uint32_t start, uint32_t room) {
    DescRing t;
    t.size = size;
    t.cons = start;
    t.prod = start + (size - room);
    t.ent = exact<xsk_gpu_desc>(size);
    for (uint32_t i = 0; i < size; ++i) t.ent[i] = fresh_desc();  // unconsumed entries and stale ones: all distinct
    return t;
}
static uint32_t pow2_at_least(uint32_t n) {
    uint32_t s = 1;
    while (s < n) s <<= 1;
    return s;
}

static const uint32_t kSizes[] = {1u, 2u, 8u, 64u, 512u, 4096u};
enum Mix { kMixed, kAllPass, kNoPass, kAllRedirect };
enum StackKind { kNoStack, kRoom0, kRoom1, kRoomQm1, kRoomQ, kRoomAbove, kStackKinds };
static uint64_t g_cases = 0, g_cut = 0, g_conserved = 0, g_tail = 0, g_some = 0, g_all = 0, g_none = 0, g_identity = 0;
static uint64_t g_bad_back = 0;  // a descriptor that does not fit any UMEM was dropped and its address reached the pool
static const uint64_t kBadAddr = 0xFFFFFFFFFFFFFFF0ull;

// `frames` received frames steered to n_ports ports and served by the egress's rule; pool_kind 0: full (takes none),
// 1: room for about half the list, 2: room for all.
static void steered_case(uint32_t n_ports, uint32_t start, uint32_t frames, uint32_t n_max, int pool_kind, int stack_kind,
                         Mix mix, uint32_t seed) {
    char tag[200];
    snprintf(tag, sizeof tag, "ports %u start %u frames %u n_max %u pool %d stack %d mix %d seed %u", n_ports, start,
             frames, n_max, pool_kind, stack_kind, (int)mix, seed);
    CHECK(frames <= n_max, "%s: case", tag);
    Inputs in;
    in.n_max = n_max;
    in.received_word = frames;
    in.refilled = seed * 3u + 1u;
    in.descs = exact<xsk_gpu_desc>(n_max);
    in.actions = exact<uint8_t>(n_max);
    std::vector<uint8_t> port(n_max, 0xFF);
    uint32_t Q = 0;
    for (uint32_t i = 0; i < n_max; ++i) {
        if (i < frames) {
            in.descs[i] = fresh_desc();
            const uint32_t k = (uint32_t)(rnd64() % 10u);
            uint8_t a = k < 4u ? XSK_GPU_XDP_REDIRECT : k < 6u ? XSK_GPU_XDP_DROP : XSK_GPU_XDP_PASS;
            if (mix == kAllPass) a = XSK_GPU_XDP_PASS;
            if (mix == kNoPass && a == XSK_GPU_XDP_PASS) a = XSK_GPU_XDP_DROP;
            if (mix == kAllRedirect) a = XSK_GPU_XDP_REDIRECT;
            if (mix == kMixed && i == frames / 2u) {  // the row the filter drops unread: an address no UMEM holds
                in.descs[i].addr = kBadAddr;
                in.descs[i].len = 64u;
                a = XSK_GPU_XDP_DROP;
            }
            in.actions[i] = a;
            Q += a == XSK_GPU_XDP_PASS;
            if (a == XSK_GPU_XDP_REDIRECT) {
                uint32_t p = (uint32_t)(rnd64() % n_ports);
                if (n_ports >= 3u && p == 1u) p = 2u;  // port 1: an empty segment
                port[i] = (uint8_t)p;
            }
        } else {
            memset(&in.descs[i], 0, sizeof(xsk_gpu_desc));  // the pad
            in.actions[i] = XSK_GPU_XDP_PASS;               // (behind r: never read as a frame's)
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
    in.d_tx = exact<xsk_gpu_desc>(n_max);
    in.d_free = exact<uint64_t>(n_max);
    memset(in.d_tx, 0xEE, n_max * sizeof(xsk_gpu_desc));
    memset(in.d_free, 0xEE, n_max * sizeof(uint64_t));
    in.counts = exact<EgCounts>(n_ports);
    uint32_t cut = 0;
    for (uint32_t p = 0; p < n_ports; ++p) {
        uint32_t R = 0;
        for (uint32_t i = in.off[p]; i < in.off[p + 1u]; ++i) R += reply_of(out[i]);
        const uint32_t size = kSizes[(p * 5u + seed) % 6u];
        uint32_t room = size;
        if (p == 0u && n_ports > 1u) room = 0u;
        if (p == n_ports - 1u && R) room = min2(R - 1u, size);
        s.tx[p] = make_ring(size, start + 2u * p, room);
        // the egress's rule for this port (its own arithmetic is tests/c/test_egress_ports.cpp's)
        const uint32_t o_p = in.off[p];
        uint32_t nt = 0, nf = 0;
        for (uint32_t i = o_p; i < in.off[p + 1u]; ++i) {
            if (reply_of(out[i]) && nt < room) {
                in.d_tx[o_p + nt].addr = out[i].addr;
                in.d_tx[o_p + nt].len = out[i].len;
                in.d_tx[o_p + nt].options = 0;
                nt++;
            } else {
                in.d_free[o_p + nf++] = out[i].addr;
            }
        }
        in.counts[p] = eg_counts(in.off[p + 1u] - o_p, R, room);
        CHECK(in.counts[p].n_tx == nt && in.counts[p].n_free == nf, "%s: egress lists", tag);
        cut += in.counts[p].n_tx_full;
    }
    // the stack ring
    s.has_stack = stack_kind != kNoStack;
    uint32_t room_s = 0;
    if (s.has_stack) {
        room_s = stack_kind == kRoom0 ? 0u : stack_kind == kRoom1 ? 1u : stack_kind == kRoomQm1 ? (Q ? Q - 1u : 0u)
                 : stack_kind == kRoomQ ? Q : Q + 3u;
        const uint32_t size = seed % 3u == 0u ? 4096u : pow2_at_least(room_s ? room_s : 1u);
        room_s = min2(room_s, size);
        s.stack = make_ring(size, start + 77u, room_s);
    }
    // the pool
    s.capacity = frames + 5u;
    s.n_free = pool_kind == 0 ? s.capacity : pool_kind == 1 ? s.capacity - frames / 2u : 3u;
    s.pool = exact<uint64_t>(s.capacity);
    for (uint32_t i = 0; i < s.capacity; ++i) s.pool[i] = (g_frame++) * 2048u;

    State d = state_copy(s), sp = state_copy(s);
    Where w;
    const Result rd = dev_end(d, in), rs = spec_end(sp, in, true, &w);
    result_same(rd, rs, tag);
    state_same(d, sp, tag);
    const uint32_t want_s = min2(Q, room_s);
    CHECK(rs.received == frames && rs.redirected == out.size() && rs.tx_full == cut && rs.passed == want_s &&
              rs.pass_full == Q - want_s,
          "%s: counts", tag);
    // batch order on the stack ring: its new entries are the first s PASS descriptors, whole
    for (uint32_t i = 0, q = 0; i < frames && q < want_s; ++i)
        if (in.actions[i] == XSK_GPU_XDP_PASS) {
            CHECK(!memcmp(&d.stack.ent[(s.stack.prod + q) & (s.stack.size - 1u)], &in.descs[i], sizeof(xsk_gpu_desc)),
                  "%s: stack entry %u", tag, q);
            q++;
        }
    if (frames == 0) state_same(d, s, tag);  // nothing received: nothing changes
    if (want_s == 0) {  // no stack ring, or a full one: xsk_gpu_rx_ports_end_dev()'s rule
        State id = state_copy(s);
        const Result ri = spec_end(id, in, false, nullptr);
        state_same(d, id, tag);
        CHECK(!memcmp(&rd, &ri, 6 * sizeof(uint32_t)) && rd.passed == 0 && rd.pass_full == Q, "%s: identity", tag);
        state_free(id);
        g_identity++;
    }
    if (w.all_pushed) {  // conservation: every received address exactly once, on a TX ring, the stack ring or the pool
        std::vector<uint64_t> got(w.tx), want;
        got.insert(got.end(), w.stack.begin(), w.stack.end());
        got.insert(got.end(), w.pool.begin(), w.pool.end());
        for (uint32_t i = 0; i < frames; ++i) want.push_back(in.descs[i].addr);
        std::sort(got.begin(), got.end());
        std::sort(want.begin(), want.end());
        CHECK(got == want, "%s: conservation", tag);
        g_conserved++;
        if (mix == kMixed && frames) {  // the end stage returns the dropped row's address as a number, like any other
            CHECK(std::count(w.pool.begin(), w.pool.end(), kBadAddr) == 1, "%s: the bad descriptor's address", tag);
            g_bad_back++;
        }
    } else {
        g_tail++;
    }
    g_cut += cut != 0;
    g_none += Q && want_s == 0;
    g_some += want_s && want_s < Q;
    g_all += Q && want_s == Q;
    state_free(d);
    state_free(sp);
    state_free(s);
    inputs_free(in);
    g_cases++;
}

// Garbage: every word and byte holds anything.  The device side against the rule, and never outside an array.
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
        in.actions[i] = k % 3u ? (uint8_t)(rnd64() % 6u) : (uint8_t)rnd64();
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
        s.tx[p] = make_ring(size, (uint32_t)rnd64(), (uint32_t)(rnd64() % (size + 1u)));
        s.tx[p].prod = word(s.tx[p].prod);
        s.tx[p].cons = word(s.tx[p].cons);
    }
    s.has_stack = k % 5u != 0u;
    if (s.has_stack) {
        const uint32_t size = kSizes[(k / 5u) % 6u];
        s.stack = make_ring(size, (uint32_t)rnd64(), (uint32_t)(rnd64() % (size + 1u)));
        s.stack.prod = word(s.stack.prod);
        s.stack.cons = word(s.stack.cons);
    }
    s.capacity = 1u + (uint32_t)(rnd64() % (2u * n_max + 8u));
    s.n_free = k % 4u == 0 ? s.capacity + 1u + (uint32_t)(rnd64() % 1000u) : word((uint32_t)(rnd64() % (s.capacity + 1u)));
    s.pool = exact<uint64_t>(s.capacity);
    for (uint32_t i = 0; i < s.capacity; ++i) s.pool[i] = (g_frame++) * 2048u;
    State d = state_copy(s), sp = state_copy(s);
    const Result rd = dev_end(d, in), rs = spec_end(sp, in, true, nullptr);
    result_same(rd, rs, tag);
    state_same(d, sp, tag);
    state_free(d);
    state_free(sp);
    state_free(s);
    inputs_free(in);
    g_cases++;
}

int main() {
    // the layouts: end's part grown by the second row and its total; everything in front of it the steered step's
    const uint32_t bounds[] = {1u, 63u, 64u, 1024u, 1025u, 1300u, 65536u, XSK_GPU_MAX_BATCH};
    const uint32_t ports[] = {1u, 3u, 64u};
    for (uint32_t mb : bounds)
        for (uint32_t np : ports) {
            const size_t sb = (size_t)cp_nwg(mb) * np * 4u, eb = ep_workspace_bytes(mb, np);
            const RpLayout a = rp_layout(mb, np, sb, eb), b = ps_layout(mb, np, sb, eb);
            CHECK(a.plan == b.plan && a.room == b.room && a.off == b.off && a.counts == b.counts && a.descs == b.descs &&
                      a.out == b.out && a.tx == b.tx && a.free_list == b.free_list && a.verdicts == b.verdicts &&
                      a.actions == b.actions && a.ports == b.ports && a.steer == b.steer && a.egress == b.egress &&
                      a.end == b.end && b.end % 16 == 0,
                  "layout head");
            CHECK(b.bytes >= b.end + ps_end_workspace_bytes(mb) && b.bytes % 16 == 0 && b.bytes >= a.bytes, "layout tail");
            if (mb > kPsSmallMax) {
                const size_t nwg = cp_nwg(mb);
                CHECK(ps_end_rest(mb) == 0 && ps_end_cells(mb) == (size_t)mb * 8 && ps_end_row(mb, 0) == ps_end_cells(mb) &&
                          ps_end_row(mb, 1) == ps_end_cells(mb) + nwg * 4 && ps_end_totals(mb) == ps_end_cells(mb) + nwg * 8 &&
                          ps_end_workspace_bytes(mb) == rd_align((size_t)mb * 8 + nwg * 8 + 8, 16),
                      "end workspace");
                CHECK(b.bytes - a.bytes == ps_end_workspace_bytes(mb) - rp_end_workspace_bytes(mb), "the growth");
            } else {
                CHECK(ps_end_workspace_bytes(mb) == 0 && a.bytes == b.bytes, "no end workspace on the one-workgroup path");
            }
        }

    const uint32_t starts[] = {0u, 0x12345u * 64u + 31u, 0xFFFFFFFDu};
    const uint32_t frames[] = {0u, 1u, 64u, 255u, 256u, 257u, 1024u, 1025u, 1300u};
    uint32_t seed = 0;
    for (uint32_t np : ports)
        for (uint32_t start : starts)
            for (uint32_t fr : frames) {
                const uint32_t maxes[] = {fr ? fr : 1u, fr + 7u, 1025u + fr};
                for (int sk = 0; sk < kStackKinds; ++sk) {
                    // (the bound and the pool rotate over the stack kinds; every pair occurs over the starts and ports)
                    const uint32_t n_max = maxes[(seed + sk) % 3u];
                    steered_case(np, start, fr, n_max, (int)((seed / 3u + sk) % 3u), sk, kMixed, seed);
                    seed++;
                }
            }
    for (Mix mix : {kAllPass, kNoPass, kAllRedirect})
        for (uint32_t np : ports)
            for (uint32_t fr : {1u, 64u, 257u, 1024u, 1300u})
                for (int sk = 0; sk < kStackKinds; ++sk) {
                    steered_case(np, starts[seed % 3u], fr, seed % 2u ? fr : 1025u + fr, 2 - (int)(seed % 3u), sk, mix, seed);
                    seed++;
                }
    for (uint32_t np : ports)
        for (uint32_t k = 0; k < 150; ++k)
            garbage_case(np, k % 2u ? 1u + (uint32_t)(rnd64() % 1024u) : 1025u + (uint32_t)(rnd64() % 400u), k);
    CHECK(g_bad_back > 50, "the bad descriptor's address never reached the pool (%llu)", (unsigned long long)g_bad_back);
    CHECK(g_cut > 50 && g_conserved > 100 && g_tail > 100 && g_none > 50 && g_some > 100 && g_all > 100 && g_identity > 100,
          "the cases never cut (%llu), conserved (%llu), dropped (%llu), took none (%llu), some (%llu), all (%llu) or met the "
          "identity (%llu)",
          (unsigned long long)g_cut, (unsigned long long)g_conserved, (unsigned long long)g_tail, (unsigned long long)g_none,
          (unsigned long long)g_some, (unsigned long long)g_all, (unsigned long long)g_identity);
    printf("ring pass ok: %llu cases, %llu with a reply left out, %llu conserved, %llu with the pool's tail dropped; the "
           "stack ring took none %llu, some %llu, all %llu times\n",
           (unsigned long long)g_cases, (unsigned long long)g_cut, (unsigned long long)g_conserved,
           (unsigned long long)g_tail, (unsigned long long)g_none, (unsigned long long)g_some, (unsigned long long)g_all);
    return 0;
}
