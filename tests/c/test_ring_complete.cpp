// The arithmetic of xsk_gpu_tx_complete_rings_dev() (xsknet_amd/csrc/xsk_ring_complete.h over xsk_ring_dev.h) compiled
// for the host: both paths of xsk_ring_complete.hip replayed lane by lane with the header's functions -- the
// one-workgroup path (a lane per ring decides, the prefix A, 1024 lanes stride over the positions, publish) and the path
// of a kernel boundary (a grid of 256-lane workgroups sized by rc_nwg(rc_span()), every workgroup deciding for itself,
// a 128-lane publish launch that decides again) -- and compared with a sequential restatement of the rule of
// include/xsk_gpu.h: xsk_gpu_tx_complete_dev()'s rule applied to ring 0, 1, ... in turn.  Every ring is a heap allocation
// of exactly `size` entries, the pool of `capacity`, d_moved of n_rings words; the test builds this file with
// -fsanitize=address,undefined, so an index one past an array's end is a failure here, not a stray store on a device.
// Every store into the pool is also checked: once per slot, only inside the part that was free when the call began, and
// all of [pool_n, pool_n + pushed) is stored.
//
// 1, 2, 3, 64 and 65 rings; ring sizes 1 to 4096; consumer words at 0, mid-ring and 0xFFFFFFFD; rings empty, holding one
// entry, partly used, full, and all of these mixed in one call; max 1, 4, 1024, 1025 and 1300; a pool with room for
// nothing, for one entry, with a cut strictly inside a ring, a cut exactly on a ring boundary, a cut inside the last ring
// that gives anything, and room for all.  The larger path also with grids of 1 and 3 workgroups (what the cap of
// rc_nwg() leaves: the positions are walked in strides).  Then garbage: every index word and the pool's count hold
// anything.  Then the prefix at its limits: 65 rings of 2^31 entries against a room of 2^32 - 1.  Stand-alone: prints
// "ring complete ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/xsk_gpu.h"
#include "../../xsknet_amd/csrc/xsk_ring_complete.h"
#include "../../xsknet_amd/csrc/xsk_ring_dev.h"

#define CHECK(c, ...)                     \
    do {                                  \
        if (!(c)) {                       \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            exit(1);                      \
        }                                 \
    } while (0)

using namespace xskgpu;

static_assert(kRcMaxRings == XSK_GPU_COMPLETE_MAX_RINGS && kRcSmallMax == XSK_GPU_LOWLAT_MAX, "the header's constants");

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

struct AddrRing {
    uint32_t prod, cons, size;
    uint64_t* ent;
};
struct State {
    uint32_t n_rings;
    AddrRing comp[kRcMaxRings];
    uint64_t* pool;
    uint32_t n_free, capacity;
};
struct Out {
    uint32_t moved[kRcMaxRings];
    uint32_t pushed;
};

static State state_copy(const State& s) {
    State c = s;
    for (uint32_t q = 0; q < s.n_rings; ++q) c.comp[q].ent = copy_of(s.comp[q].ent, s.comp[q].size);
    c.pool = copy_of(s.pool, s.capacity);
    return c;
}
static void state_free(State& s) {
    for (uint32_t q = 0; q < s.n_rings; ++q) free(s.comp[q].ent);
    free(s.pool);
}
static void state_same(const State& a, const State& b, const char* tag) {
    for (uint32_t q = 0; q < a.n_rings; ++q) {
        CHECK(a.comp[q].prod == b.comp[q].prod && a.comp[q].cons == b.comp[q].cons, "%s: ring %u words %u/%u against %u/%u",
              tag, q, a.comp[q].prod, a.comp[q].cons, b.comp[q].prod, b.comp[q].cons);
        CHECK(!memcmp(a.comp[q].ent, b.comp[q].ent, a.comp[q].size * sizeof(uint64_t)), "%s: ring %u entries differ", tag, q);
    }
    CHECK(a.n_free == b.n_free, "%s: pool count %u against %u", tag, a.n_free, b.n_free);
    CHECK(a.n_free <= a.capacity, "%s: the count ends above the capacity", tag);
    CHECK(!memcmp(a.pool, b.pool, a.n_free * sizeof(uint64_t)), "%s: pool stack differs", tag);
}
static void out_same(const Out& a, const Out& b, uint32_t n_rings, const char* tag) {
    for (uint32_t q = 0; q < n_rings; ++q) CHECK(a.moved[q] == b.moved[q], "%s: moved[%u] %u against %u", tag, q, a.moved[q], b.moved[q]);
    CHECK(a.pushed == b.pushed, "%s: pushed %u against %u", tag, a.pushed, b.pushed);
}

// ---- the rule, sequentially: xsk_gpu_tx_complete_dev()'s for ring 0, 1, ... ----
static void reference(State& s, uint32_t max, Out* out) {
    uint32_t total = 0;
    for (uint32_t q = 0; q < s.n_rings; ++q) {
        AddrRing& r = s.comp[q];
        uint32_t used = r.prod - r.cons;
        if (used > r.size) used = r.size;
        const uint32_t n = used < max ? used : max;
        const uint32_t cnt = s.n_free < s.capacity ? s.n_free : s.capacity;
        const uint32_t pushed = n < s.capacity - cnt ? n : s.capacity - cnt;
        for (uint32_t j = 0; j < pushed; ++j) s.pool[cnt + j] = r.ent[(r.cons + j) & (r.size - 1u)];
        s.n_free = cnt + pushed;
        r.cons += n;
        out->moved[q] = n;
        total += pushed;
    }
    out->pushed = total;
}

// ---- the device side, lane by lane ----
struct Decided {  // CompLds of xsk_ring_complete.hip
    uint32_t n[kRcMaxRings], cons[kRcMaxRings], A[kRcMaxBounds], pool_n;
};
// comp_decide(): a lane per ring, a barrier, a lane per prefix
static void decide(const State& s, uint32_t max, Decided* d) {
    for (uint32_t q = 0; q < s.n_rings; ++q) {
        d->cons[q] = s.comp[q].cons;
        d->n[q] = rc_take(s.comp[q].prod, s.comp[q].cons, s.comp[q].size, max);
    }
    d->pool_n = rd_pool_n(s.n_free, s.capacity);
    const uint32_t room = rc_room(d->pool_n, s.capacity);
    for (uint32_t q = 0; q <= s.n_rings; ++q) {
        d->A[q] = rc_prefix(d->n, q, room);
        CHECK(d->A[q] <= room && (q == 0 ? d->A[0] == 0u : d->A[q] >= d->A[q - 1u]), "the prefix");
    }
}
static bool decided_same(const Decided& a, const Decided& b, uint32_t n_rings) {
    return !memcmp(a.n, b.n, n_rings * 4u) && !memcmp(a.cons, b.cons, n_rings * 4u) && !memcmp(a.A, b.A, (n_rings + 1u) * 4u) &&
           a.pool_n == b.pool_n;
}

// comp_copy() of one lane; every pool store once, inside [pool_n, capacity)
static void copy_lane(State& s, const Decided& d, uint8_t* seen, uint64_t first, uint64_t stride) {
    const uint32_t total = d.A[s.n_rings];
    for (uint64_t L = first; L < total; L += stride) {
        const RcSrc src = rc_src(d.A, s.n_rings, (uint32_t)L);
        CHECK(src.ring < s.n_rings && d.A[src.ring] <= L && L < d.A[src.ring + 1u], "owner of %llu", (unsigned long long)L);
        CHECK(src.j < d.n[src.ring], "entry %u of ring %u is not one it gives up", src.j, src.ring);
        const uint32_t slot = rc_pool_slot(d.pool_n, (uint32_t)L);
        CHECK(slot >= d.pool_n && slot < s.capacity, "pool slot %u outside what was free", slot);
        CHECK(!seen[slot], "pool slot %u stored twice", slot);
        seen[slot] = 1;
        const AddrRing& r = s.comp[src.ring];
        s.pool[slot] = r.ent[rc_ring_slot(d.cons[src.ring], src.j, r.size)];
    }
}

// grid 0: the grid the host launch takes; else that many workgroups (the larger path only)
static void replay(State& s, uint32_t max, Out* out, uint32_t* d_moved /* n_rings words exactly, or NULL */, uint32_t grid) {
    if (max == 0) {  // nothing launches; the outputs are zeroed
        for (uint32_t q = 0; q < s.n_rings; ++q) out->moved[q] = 0;
        if (d_moved) memset(d_moved, 0, s.n_rings * 4u);
        out->pushed = 0;
        return;
    }
    Decided d;
    decide(s, max, &d);
    uint8_t* seen = exact<uint8_t>(s.capacity);
    memset(seen, 0, s.capacity);
    if (max <= kRcSmallMax) {
        for (uint32_t t = 0; t < kRcSmallThreads; ++t) copy_lane(s, d, seen, t, kRcSmallThreads);
    } else {
        uint32_t sizes[kRcMaxRings];
        for (uint32_t q = 0; q < s.n_rings; ++q) sizes[q] = s.comp[q].size;
        const uint64_t span = rc_span(sizes, s.n_rings, max);
        CHECK(span >= d.A[s.n_rings], "the grid's span is below what the rings give");
        const uint32_t nwg = grid ? grid : rc_nwg(span);
        CHECK(nwg >= 1u && nwg <= kRcMaxGrid, "grid");
        CHECK(grid || (uint64_t)nwg * kRdCopy >= span || nwg == kRcMaxGrid, "an uncapped grid covers its span in one pass");
        for (uint32_t wg = 0; wg < nwg; ++wg) {
            Decided dw;  // every workgroup decides for itself: nothing has stored a word yet
            decide(s, max, &dw);
            CHECK(decided_same(d, dw, s.n_rings), "a workgroup decides differently");
            for (uint32_t lane = 0; lane < kRdCopy; ++lane) copy_lane(s, dw, seen, rd_copy_first(wg, lane), rd_copy_stride(nwg));
        }
        Decided dp;  // the publish launch decides again from the same words
        decide(s, max, &dp);
        CHECK(decided_same(d, dp, s.n_rings), "the publish launch decides differently");
    }
    for (uint32_t k = 0; k < s.capacity; ++k)
        CHECK(seen[k] == (k >= d.pool_n && k - d.pool_n < d.A[s.n_rings] ? 1 : 0), "pool slot %u: stored %u", k, seen[k]);
    free(seen);
    // comp_publish(): lane q, then lane 0
    for (uint32_t q = 0; q < s.n_rings; ++q) {
        if (d.n[q]) s.comp[q].cons = rc_cons_after(d.cons[q], d.n[q]);
        if (d_moved) d_moved[q] = d.n[q];
        out->moved[q] = d.n[q];
    }
    s.n_free = rc_pool_after(d.pool_n, d.A[s.n_rings]);
    out->pushed = d.A[s.n_rings];
}

// ---- cases ----
enum Fill { kEmpty, kOne, kPartial, kFull, kMixed };
enum Room { kNone, kSingle, kInside, kBoundary, kLast, kAll, kRooms };
static const uint32_t kStarts[] = {0u, 0x12345u, 0xFFFFFFFDu};

static uint32_t used_for(Fill f, uint32_t size, uint32_t q) {
    switch (f) {
        case kEmpty: return 0;
        case kOne: return 1;
        case kPartial: return size > 2u ? 1u + (uint32_t)(rnd64() % (size - 1u)) : 1u;
        case kFull: return size;
        default: return used_for((Fill)(q % 4u), size, q);
    }
}

static uint64_t g_next_addr = 1;
static State make(uint32_t n_rings, Fill f, uint32_t start, uint32_t big_size) {
    State s;
    memset(&s, 0, sizeof s);
    s.n_rings = n_rings;
    for (uint32_t q = 0; q < n_rings; ++q) {
        AddrRing& r = s.comp[q];
        r.size = big_size ? big_size : 1u << (rnd64() % 13u);  // 1 .. 4096
        r.ent = exact<uint64_t>(r.size);
        for (uint32_t k = 0; k < r.size; ++k) r.ent[k] = (g_next_addr++) << 12;
        r.cons = start + q * 7u;
        r.prod = r.cons + used_for(f, r.size, q);
    }
    return s;
}
// a pool whose free part is `room` entries, with a stack of `below` beneath it
static void give_pool(State& s, uint32_t room, uint32_t below) {
    s.capacity = below + room;
    if (s.capacity == 0) {
        s.capacity = 1;  // (capacity >= 1 is a rule of the call)
        below = 1;
    }
    s.pool = exact<uint64_t>(s.capacity);
    for (uint32_t k = 0; k < s.capacity; ++k) s.pool[k] = 0xF00D000000000000ull | k;
    s.n_free = below;
}

static uint64_t g_cases = 0, g_cut_inside = 0, g_cut_boundary = 0;

static void run(State& s, uint32_t max, const char* tag, uint32_t grid = 0) {
    State want = state_copy(s);
    Out ow, og;
    reference(want, max, &ow);
    uint32_t* d_moved = exact<uint32_t>(s.n_rings);
    replay(s, max, &og, d_moved, grid);
    if (max) state_same(s, want, tag);  // (max == 0 stores no word: a count above the capacity stays)
    out_same(og, ow, s.n_rings, tag);
    CHECK(!memcmp(d_moved, ow.moved, s.n_rings * 4u), "%s: d_moved", tag);
    free(d_moved);
    state_free(want);
    ++g_cases;
}

static void matrix() {
    static const uint32_t rings[] = {1, 2, 3, 64, 65}, maxes[] = {1, 4, 1024, 1025, 1300};
    char tag[160];
    for (uint32_t n_rings : rings)
        for (int f = kEmpty; f <= kMixed; ++f)
            for (uint32_t max : maxes)
                for (int room = kNone; room < kRooms; ++room) {
                    const uint32_t start = kStarts[(g_cases / 3u) % 3u];
                    // the larger path needs rings that hold more than 1024 entries to differ from the other
                    State s = make(n_rings, (Fill)f, start, max > kRcSmallMax && (g_cases & 1u) ? 2048u : 0u);
                    std::vector<uint32_t> n(n_rings);
                    uint64_t sum = 0;
                    uint32_t last = n_rings;  // the last ring that gives anything
                    for (uint32_t q = 0; q < n_rings; ++q) {
                        n[q] = rc_take(s.comp[q].prod, s.comp[q].cons, s.comp[q].size, max);
                        sum += n[q];
                        if (n[q]) last = q;
                    }
                    uint32_t want_room = 0;
                    switch (room) {
                        case kNone: want_room = 0; break;
                        case kSingle: want_room = 1; break;
                        case kAll: want_room = (uint32_t)sum + 5u; break;
                        case kInside: {  // strictly inside the first ring that gives two or more
                            uint64_t a = 0;
                            want_room = (uint32_t)sum;
                            for (uint32_t q = 0; q < n_rings; ++q) {
                                if (n[q] >= 2u) {
                                    want_room = (uint32_t)a + 1u + (uint32_t)(rnd64() % (n[q] - 1u));
                                    ++g_cut_inside;
                                    break;
                                }
                                a += n[q];
                            }
                            break;
                        }
                        case kBoundary: {  // exactly behind a ring that gives something, with more behind it
                            uint64_t a = 0;
                            want_room = (uint32_t)sum;
                            for (uint32_t q = 0; q + 1u < n_rings; ++q) {
                                a += n[q];
                                if (n[q] && a < sum) {
                                    want_room = (uint32_t)a;
                                    ++g_cut_boundary;
                                    if (rnd64() & 1u) break;
                                }
                            }
                            break;
                        }
                        default:  // inside the last ring that gives anything
                            want_room = last < n_rings ? (uint32_t)(sum - n[last]) + n[last] / 2u : 0u;
                            break;
                    }
                    give_pool(s, want_room, (uint32_t)(rnd64() % 9u));
                    snprintf(tag, sizeof tag, "rings %u fill %d max %u room %d(%u of %llu) start %#x", n_rings, f, max, room,
                             want_room, (unsigned long long)sum, start);
                    if (max > kRcSmallMax && room == kAll) {  // what a capped grid leaves: strides
                        for (uint32_t grid : {1u, 3u}) {
                            State c = state_copy(s);
                            run(c, max, tag, grid);
                            state_free(c);
                        }
                    }
                    run(s, max, tag);
                    state_free(s);
                }
    CHECK(g_cut_inside >= 50 && g_cut_boundary >= 50, "the cut cases were not reached (%llu, %llu)",
          (unsigned long long)g_cut_inside, (unsigned long long)g_cut_boundary);
}

static void zero_max() {
    for (uint32_t n_rings : {1u, 3u, 65u}) {
        State s = make(n_rings, kMixed, 0xFFFFFFFDu, 0);
        give_pool(s, 100, 3);
        s.n_free = s.capacity + 9u;  // stays: nothing is stored
        State before = state_copy(s);
        Out o;
        uint32_t* d_moved = exact<uint32_t>(n_rings);
        memset(d_moved, 0xEE, n_rings * 4u);
        replay(s, 0, &o, d_moved, 0);
        for (uint32_t q = 0; q < n_rings; ++q) CHECK(d_moved[q] == 0 && o.moved[q] == 0, "max 0: moved");
        CHECK(o.pushed == 0 && s.n_free == before.n_free, "max 0: the pool");
        for (uint32_t q = 0; q < n_rings; ++q) CHECK(s.comp[q].cons == before.comp[q].cons, "max 0: a consumer word");
        free(d_moved);
        state_free(before);
        state_free(s);
    }
}

static void garbage() {
    char tag[96];
    for (uint32_t it = 0; it < 600; ++it) {
        const uint32_t n_rings = 1u + (uint32_t)(rnd64() % kRcMaxRings);
        State s = make(n_rings, kMixed, (uint32_t)rnd64(), 0);
        for (uint32_t q = 0; q < n_rings; ++q) {
            if (rnd64() % 3u) s.comp[q].prod = (uint32_t)rnd64();
            if (rnd64() % 3u) s.comp[q].cons = (uint32_t)rnd64();
        }
        give_pool(s, (uint32_t)(rnd64() % 5000u), (uint32_t)(rnd64() % 50u));
        if (rnd64() & 1u) s.n_free = (uint32_t)rnd64();  // above the capacity, mostly
        static const uint32_t maxes[] = {1, 7, 1024, 1025, 5000, XSK_GPU_MAX_BATCH};
        const uint32_t max = maxes[rnd64() % 6u];
        snprintf(tag, sizeof tag, "garbage %u: rings %u max %u", it, n_rings, max);
        run(s, max, tag);
        state_free(s);
    }
}

static void limits() {
    // 65 rings of 2^31 entries, all full, against a pool of 2^32 - 1 free entries: every partial sum stays below 2^32
    uint32_t n[kRcMaxRings], sizes[kRcMaxRings];
    for (uint32_t q = 0; q < kRcMaxRings; ++q) {
        sizes[q] = kRdMaxSize;
        n[q] = rc_take(5u + kRdMaxSize, 5u, kRdMaxSize, XSK_GPU_MAX_BATCH);
        CHECK(n[q] == kRdMaxSize, "a full ring of 2^31 entries");
    }
    const uint32_t room = rc_room(0u, 0xFFFFFFFFu);
    uint32_t prev = 0;
    for (uint32_t q = 0; q <= kRcMaxRings; ++q) {
        const uint32_t a = rc_prefix(n, q, room);
        const uint64_t plain = (uint64_t)q * kRdMaxSize;
        CHECK(a == (plain < room ? plain : room) && a >= prev, "prefix %u", q);
        prev = a;
    }
    CHECK(rc_span(sizes, kRcMaxRings, XSK_GPU_MAX_BATCH) == (uint64_t)kRcMaxRings * kRdMaxSize, "span");
    CHECK(rc_nwg(0) == 1u && rc_nwg(1) == 1u && rc_nwg(256) == 1u && rc_nwg(257) == 2u, "grid, small");
    CHECK(rc_nwg((uint64_t)kRcMaxGrid * kRdCopy) == kRcMaxGrid && rc_nwg((uint64_t)kRcMaxGrid * kRdCopy + 1u) == kRcMaxGrid &&
              rc_nwg((uint64_t)kRcMaxRings * kRdMaxSize) == kRcMaxGrid,
          "grid, capped");
    // the owner search over 66 ascending bounds with empty shares among them
    uint32_t A[kRcMaxBounds];
    uint32_t acc = 0;
    for (uint32_t q = 0; q <= kRcMaxRings; ++q) {
        A[q] = acc;
        acc += (q % 3u == 1u) ? 0u : q % 5u;
    }
    for (uint32_t L = 0; L < A[kRcMaxRings]; ++L) {
        const RcSrc s = rc_src(A, kRcMaxRings, L);
        CHECK(s.ring < kRcMaxRings && A[s.ring] <= L && L < A[s.ring + 1u] && s.j == L - A[s.ring], "owner of %u", L);
    }
}

int main() {
    matrix();
    zero_max();
    garbage();
    limits();
    printf("ring complete ok (%llu cases)\n", (unsigned long long)g_cases);
    return 0;
}
