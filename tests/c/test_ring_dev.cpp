// The arithmetic of xsk_gpu_rx_begin_dev(), xsk_gpu_rx_end_dev() and xsk_gpu_tx_complete_dev()
// (xsknet_amd/csrc/xsk_ring_dev.h) compiled for the host: both paths of xsk_ring_dev.hip replayed thread by thread with
// the header's functions -- the one-workgroup path (decide, 1024 lanes copy in strides, publish) and the path of kernel
// boundaries (plan, a grid of 256-lane workgroups, publish) -- and compared with a sequential restatement of
// xsk_gpu__rx_refill() / xsk_gpu__rx_emit() / xsk_gpu_tx_complete() (xsk_gpu_rx.c) that drives xr_*() (xsk_ring.h) on
// host rings whose caches are initialised so that they refresh (both cached words equal to the ring's own index word).
// Every array is a heap allocation of exactly its size: a ring `size` entries, the pool `capacity`, the batch's
// descriptors `received`, the TX list n_tx, the free list n_free; the test builds this file with
// -fsanitize=address,undefined, so an index one past an array's end is a failure here, not a stray store on a device.
// Every store into a ring or the pool is also checked: at most once per slot, only inside the part that was free when
// the call began, so no unconsumed entry is overwritten.
//
// Ring sizes 1, 8, 64, 4096 (the pool holds size + 3 frames); index words starting at 0, mid-ring and 0xFFFFFFFD (the
// 32-bit wrap); 0, 1, 63, 64, 65, 1024, 1025, 1300 frames offered (as many as the ring holds); max_batch equal to the
// offer, half of it, and 1025 + the offer (the other path); fill ring full, one free, all free; pool empty, one entry,
// full, capacity - 1; TX room 0, R - 1, R, R + 1, unlimited.  Then garbage words -- used > size, *d_n_free > capacity,
// counts above n_max -- against the rule of include/xsk_gpu.h stated sequentially.  Stand-alone: prints "ring dev ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/xsk_gpu.h"
#include "../../xsknet_amd/csrc/xsk_ring.h"
#include "../../xsknet_amd/csrc/xsk_ring_dev.h"

using namespace xskgpu;

#define CHECK(c, ...)                     \
    do {                                  \
        if (!(c)) {                       \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            exit(1);                      \
        }                                 \
    } while (0)

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

template <class E>
struct RingS {
    uint32_t prod, cons, size;
    E* ent;
    RdWords words() const { return RdWords{prod, cons}; }
};
struct PoolS {
    uint64_t* addr;
    uint32_t n_free, capacity;
};
struct State {
    RingS<xsk_gpu_desc> rx, tx;
    RingS<uint64_t> fill, comp;
    PoolS pool;
};

template <class E>
static RingS<E> ring_copy(const RingS<E>& r) {
    RingS<E> c = r;
    c.ent = exact<E>(r.size);
    memcpy(c.ent, r.ent, r.size * sizeof(E));
    return c;
}
static State state_copy(const State& s) {
    State c;
    c.rx = ring_copy(s.rx);
    c.tx = ring_copy(s.tx);
    c.fill = ring_copy(s.fill);
    c.comp = ring_copy(s.comp);
    c.pool = s.pool;
    c.pool.addr = exact<uint64_t>(s.pool.capacity);
    memcpy(c.pool.addr, s.pool.addr, s.pool.capacity * sizeof(uint64_t));
    return c;
}
static void state_free(State& s) {
    free(s.rx.ent);
    free(s.tx.ent);
    free(s.fill.ent);
    free(s.comp.ent);
    free(s.pool.addr);
}
template <class E>
static void ring_same(const RingS<E>& a, const RingS<E>& b, const char* what, const char* tag) {
    CHECK(a.prod == b.prod && a.cons == b.cons, "%s: %s words %u/%u against %u/%u", tag, what, a.prod, a.cons, b.prod,
          b.cons);
    CHECK(!memcmp(a.ent, b.ent, a.size * sizeof(E)), "%s: %s entries differ", tag, what);
}
static void state_same(const State& a, const State& b, const char* tag) {
    ring_same(a.rx, b.rx, "rx", tag);
    ring_same(a.tx, b.tx, "tx", tag);
    ring_same(a.fill, b.fill, "fill", tag);
    ring_same(a.comp, b.comp, "comp", tag);
    CHECK(a.pool.n_free == b.pool.n_free, "%s: pool count %u against %u", tag, a.pool.n_free, b.pool.n_free);
    const uint32_t n = rd_pool_n(a.pool.n_free, a.pool.capacity);
    CHECK(!memcmp(a.pool.addr, b.pool.addr, n * sizeof(uint64_t)), "%s: pool stack differs", tag);
}

static uint8_t verdict_of(const xsk_gpu_desc& d) {  // a function of the frame, so every side derives the same
    const uint64_t k = d.addr / 2048u;
    return k % 3u == 0 ? (uint8_t)XSK_GPU_TX_REPLY : (uint8_t)(1u + k % 7u);
}

// ---- a slot may be stored once, and only inside what was free when the call began ----
struct Guard {
    uint8_t* seen;
    uint32_t first, room, size;  // slots first, first + 1, ... (room of them), modulo size (a ring) or plain (the pool)
    bool ring;
    Guard(uint32_t first_, uint32_t room_, uint32_t size_, bool ring_)
        : first(first_), room(room_), size(size_), ring(ring_) {
        seen = exact<uint8_t>(size);
        if (size) memset(seen, 0, size);
    }
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
struct Lanes {  // the (first, stride) of every lane of a launch, in turn
    bool small;
    uint32_t nwg;
    template <class F>
    void each(F f) const {
        if (small) {
            for (uint32_t t = 0; t < kRdSmallThreads; ++t) f((uint64_t)t, (uint64_t)kRdSmallThreads);
        } else {
            for (uint32_t wg = 0; wg < nwg; ++wg)
                for (uint32_t lane = 0; lane < kRdCopy; ++lane) f(rd_copy_first(wg, lane), rd_copy_stride(nwg));
        }
    }
};
static Lanes lanes_for(uint32_t bound) { return Lanes{bound <= kRdSmallMax, rd_nwg(bound)}; }

// begin: returns the plan; *descs is an allocation of exactly plan.received entries
static RdPlan dev_begin(State& s, uint32_t max_batch, xsk_gpu_desc** descs) {
    const RdPlan p = rd_begin_plan(s.rx.words(), s.rx.size, s.fill.words(), s.fill.size, s.tx.words(), s.tx.size,
                                   s.pool.n_free, s.pool.capacity, max_batch);
    CHECK(p.received <= max_batch && p.received <= s.rx.size && p.refilled <= s.fill.size, "begin plan");
    xsk_gpu_desc* const d = exact<xsk_gpu_desc>(p.received);
    Guard g(rd_slot(s.fill.prod, s.fill.size), rd_free(s.fill.prod, s.fill.cons, s.fill.size), s.fill.size, true);
    Guard gd(0, p.received, p.received, false);
    lanes_for(max_batch).each([&](uint64_t first, uint64_t stride) {
        for (uint64_t i = first; i < p.received; i += stride) {
            gd.hit((uint32_t)i, "d_descs");
            d[i] = s.rx.ent[rd_slot(p.rx_cons + (uint32_t)i, s.rx.size)];
        }
        for (uint64_t i = first; i < p.refilled; i += stride) {
            const uint32_t slot = rd_slot(p.fq_prod + (uint32_t)i, s.fill.size), src = rd_pop(p.pool_n, (uint32_t)i);
            g.hit(slot, "fill ring");
            CHECK(src < s.pool.capacity, "pop outside the pool");
            s.fill.ent[slot] = s.pool.addr[src];
        }
    });
    if (p.received) {  // publish
        if (p.refilled) s.fill.prod = rd_begin_fq_prod(p);
        s.pool.n_free = rd_begin_pool_n(p);
    }
    *descs = d;
    return p;
}

// end: d_tx and d_free are allocations of exactly what the clamps allow the lanes to read
static xsk_gpu_rx_result dev_end(State& s, const RdPlan& plan, const xsk_gpu_desc* d_tx, const uint64_t* d_free,
                                 const EgCounts& c, uint32_t n_max) {
    const RdEnd e = rd_end_plan(c.n_tx, c.n_free, n_max, s.tx.words(), s.tx.size, s.pool.n_free, s.pool.capacity,
                                plan.received);
    Guard gt(rd_slot(s.tx.prod, s.tx.size), rd_free(s.tx.prod, s.tx.cons, s.tx.size), s.tx.size, true);
    Guard gp(e.pool_n, s.pool.capacity - e.pool_n, s.pool.capacity, false);
    lanes_for(n_max).each([&](uint64_t first, uint64_t stride) {
        for (uint64_t k = first; k < e.n_tx; k += stride) {
            const uint32_t slot = rd_slot(e.tx_prod + (uint32_t)k, s.tx.size);
            gt.hit(slot, "tx ring");
            s.tx.ent[slot] = d_tx[k];
        }
        for (uint64_t j = first; j < e.pushed; j += stride) {
            gp.hit(e.pool_n + (uint32_t)j, "pool");
            s.pool.addr[e.pool_n + (uint32_t)j] = d_free[j];
        }
    });
    if (e.n_tx) s.tx.prod = e.tx_prod + e.n_tx;
    s.pool.n_free = e.pool_n + e.pushed;
    if (e.release) s.rx.cons = s.rx.cons + e.release;
    return xsk_gpu_rx_result{e.release, e.n_tx, c.n_tx_full, plan.refilled};
}

static uint32_t dev_complete(State& s, uint32_t max) {
    const RdComplete c = rd_complete_plan(s.comp.words(), s.comp.size, max, s.pool.n_free, s.pool.capacity);
    Guard gp(c.pool_n, s.pool.capacity - c.pool_n, s.pool.capacity, false);
    lanes_for(max).each([&](uint64_t first, uint64_t stride) {
        for (uint64_t j = first; j < c.pushed; j += stride) {
            gp.hit(c.pool_n + (uint32_t)j, "pool");
            s.pool.addr[c.pool_n + (uint32_t)j] = s.comp.ent[rd_slot(c.cons + (uint32_t)j, s.comp.size)];
        }
    });
    s.pool.n_free = c.pool_n + c.pushed;
    if (c.n) s.comp.cons = c.cons + c.n;
    return c.n;
}

// The egress between begin and end (xsk_gpu_egress_dev()'s rule, sequentially; its own arithmetic is
// tests/c/test_egress_slots.cpp's): lists of exactly n_tx and n_free entries.
static EgCounts egress(const xsk_gpu_desc* descs, uint32_t n, uint32_t room, xsk_gpu_desc** d_tx, uint64_t** d_free) {
    uint32_t R = 0;
    for (uint32_t i = 0; i < n; ++i) R += verdict_of(descs[i]) == XSK_GPU_TX_REPLY;
    const EgCounts c = eg_counts(n, R, room);
    xsk_gpu_desc* const t = exact<xsk_gpu_desc>(c.n_tx);
    uint64_t* const f = exact<uint64_t>(c.n_free);
    uint32_t nt = 0, nf = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (verdict_of(descs[i]) == XSK_GPU_TX_REPLY && nt < room) {
            t[nt].addr = descs[i].addr;
            t[nt].len = descs[i].len;
            t[nt].options = 0;
            nt++;
        } else {
            f[nf++] = descs[i].addr;
        }
    }
    CHECK(nt == c.n_tx && nf == c.n_free, "egress lists");
    *d_tx = t;
    *d_free = f;
    return c;
}

static xsk_gpu_rx_result dev_step(State& s, uint32_t max_batch) {
    xsk_gpu_desc *descs, *d_tx;
    uint64_t* d_free;
    const RdPlan p = dev_begin(s, max_batch, &descs);
    const EgCounts c = egress(descs, rd_min(p.received, max_batch), p.tx_room, &d_tx, &d_free);
    const xsk_gpu_rx_result r = dev_end(s, p, d_tx, d_free, c, max_batch);
    free(descs);
    free(d_tx);
    free(d_free);
    return r;
}

// ---- the host side: xsk_gpu_rx.c restated over xr_*() ----
template <class E>
static xsk_gpu_ring host_ring(RingS<E>& r, bool consumer) {
    xsk_gpu_ring h;
    h.cached_prod = h.cached_cons = consumer ? r.cons : r.prod;  // the first use refreshes
    h.mask = r.size - 1u;
    h.size = r.size;
    h.producer = &r.prod;
    h.consumer = &r.cons;
    h.ring = r.ent;
    h.flags = NULL;
    return h;
}
static void pool_push(PoolS* p, uint64_t a) {
    if (p->n_free < p->capacity) p->addr[p->n_free++] = a;
}
static uint32_t host_refill(xsk_gpu_ring* fill, PoolS* pool) {  // xsk_gpu__rx_refill()
    uint32_t stock = xr_prod_free(fill, pool->n_free);
    if (stock > pool->n_free) stock = pool->n_free;
    if (!stock) return 0;
    uint32_t idx_fq = 0;
    if (xr_prod_reserve(fill, stock, &idx_fq) != stock) return 0;
    for (uint32_t i = 0; i < stock; i++) *xr_addr(fill, idx_fq + i) = pool->addr[--pool->n_free];
    xr_prod_submit(fill, stock);
    return stock;
}
static xsk_gpu_rx_result host_step(State& s, uint32_t max_batch) {  // xsk_gpu_rx_step() around the transform
    xsk_gpu_rx_result r = {0, 0, 0, 0};
    xsk_gpu_ring rx = host_ring(s.rx, true), fill = host_ring(s.fill, false), tx = host_ring(s.tx, false);
    if (!xr_cons_avail(&rx, 1)) return r;
    uint32_t idx_rx = 0;
    const uint32_t rcvd = xr_cons_peek(&rx, max_batch, &idx_rx);
    r.refilled = host_refill(&fill, &s.pool);
    xsk_gpu_desc* const descs = exact<xsk_gpu_desc>(rcvd);
    for (uint32_t i = 0; i < rcvd; i++) descs[i] = *xr_desc(&rx, idx_rx + i);
    // xsk_gpu__rx_emit()
    uint32_t nrep = 0;
    for (uint32_t i = 0; i < rcvd; i++) nrep += verdict_of(descs[i]) == XSK_GPU_TX_REPLY;
    uint32_t idx_tx = 0, room = 0, sent = 0;
    if (nrep) {
        room = xr_prod_free(&tx, nrep);
        if (room > nrep) room = nrep;
        if (room) xr_prod_reserve(&tx, room, &idx_tx);
    }
    for (uint32_t i = 0; i < rcvd; i++) {
        if (verdict_of(descs[i]) == XSK_GPU_TX_REPLY && sent < room) {
            xsk_gpu_desc* t = xr_desc(&tx, idx_tx + sent);
            t->addr = descs[i].addr;
            t->len = descs[i].len;
            t->options = 0;
            sent++;
        } else {
            if (verdict_of(descs[i]) == XSK_GPU_TX_REPLY) r.tx_full++;
            pool_push(&s.pool, descs[i].addr);
        }
    }
    if (sent) xr_prod_submit(&tx, sent);
    r.replied = sent;
    xr_cons_release(&rx, rcvd);
    r.received = rcvd;
    free(descs);
    return r;
}
static uint32_t host_complete(State& s, uint32_t max) {  // xsk_gpu_tx_complete()
    xsk_gpu_ring comp = host_ring(s.comp, true);
    if (max == 0) return 0;
    uint32_t idx = 0;
    const uint32_t n = xr_cons_peek(&comp, max, &idx);
    for (uint32_t i = 0; i < n; i++) pool_push(&s.pool, *xr_addr(&comp, idx + i));
    if (n) xr_cons_release(&comp, n);
    return n;
}

// ---- the rule of include/xsk_gpu.h, sequentially, for any content of the words ----
static uint32_t spec_used(uint32_t prod, uint32_t cons, uint32_t size) {
    const uint32_t d = prod - cons;
    return d < size ? d : size;
}
static xsk_gpu_rx_result spec_step(State& s, uint32_t max_batch) {
    xsk_gpu_rx_result r = {0, 0, 0, 0};
    uint32_t rcvd = spec_used(s.rx.prod, s.rx.cons, s.rx.size);
    if (rcvd > max_batch) rcvd = max_batch;
    const uint32_t tx_room = s.tx.size - spec_used(s.tx.prod, s.tx.cons, s.tx.size);
    uint32_t pool_n = s.pool.n_free < s.pool.capacity ? s.pool.n_free : s.pool.capacity;
    xsk_gpu_desc* const descs = exact<xsk_gpu_desc>(rcvd);
    if (rcvd) {
        uint32_t stock = s.fill.size - spec_used(s.fill.prod, s.fill.cons, s.fill.size);
        if (stock > pool_n) stock = pool_n;
        for (uint32_t i = 0; i < stock; i++) s.fill.ent[(s.fill.prod + i) & (s.fill.size - 1u)] = s.pool.addr[--pool_n];
        s.fill.prod += stock;
        s.pool.n_free = pool_n;
        for (uint32_t i = 0; i < rcvd; i++) descs[i] = s.rx.ent[(s.rx.cons + i) & (s.rx.size - 1u)];
        r.refilled = stock;
    }
    xsk_gpu_desc* d_tx;
    uint64_t* d_free;
    const EgCounts c = egress(descs, rcvd, tx_room, &d_tx, &d_free);
    for (uint32_t k = 0; k < c.n_tx; k++) s.tx.ent[(s.tx.prod + k) & (s.tx.size - 1u)] = d_tx[k];  // n_tx <= tx_room
    s.tx.prod += c.n_tx;
    pool_n = s.pool.n_free < s.pool.capacity ? s.pool.n_free : s.pool.capacity;
    uint32_t pushed = c.n_free;
    if (pushed > s.pool.capacity - pool_n) pushed = s.pool.capacity - pool_n;
    for (uint32_t j = 0; j < pushed; j++) s.pool.addr[pool_n + j] = d_free[j];
    s.pool.n_free = pool_n + pushed;
    r.received = rcvd;
    s.rx.cons += rcvd;
    r.replied = c.n_tx;
    r.tx_full = c.n_tx_full;
    free(descs);
    free(d_tx);
    free(d_free);
    return r;
}
static uint32_t spec_complete(State& s, uint32_t max) {
    uint32_t n = spec_used(s.comp.prod, s.comp.cons, s.comp.size);
    if (n > max) n = max;
    const uint32_t pool_n = s.pool.n_free < s.pool.capacity ? s.pool.n_free : s.pool.capacity;
    const uint32_t pushed = n < s.pool.capacity - pool_n ? n : s.pool.capacity - pool_n;
    for (uint32_t j = 0; j < pushed; j++) s.pool.addr[pool_n + j] = s.comp.ent[(s.comp.cons + j) & (s.comp.size - 1u)];
    s.pool.n_free = pool_n + pushed;
    s.comp.cons += n;
    return n;
}

// ---- building a state ----
static uint64_t g_frame = 1;  // every frame address of a run is distinct
static xsk_gpu_desc fresh_desc() {
    xsk_gpu_desc d;
    const uint64_t k = g_frame++;
    d.addr = k * 2048u + (k * 37u) % 256u;
    d.len = 60u + (uint32_t)(k % 1400u);
    d.options = 0x1000u + (uint32_t)(k & 0xFFFFFFu);  // nonzero: a ring entry is copied whole, a TX entry carries 0
    return d;
}
static uint64_t fresh_addr() { return (g_frame++) * 2048u; }

template <class E>
static RingS<E> make_ring(uint32_t size, uint32_t start, uint32_t used) {
    RingS<E> r;
    r.size = size;
    r.cons = start;
    r.prod = start + used;
    r.ent = exact<E>(size);
    memset(r.ent, 0xA5, size * sizeof(E));  // what a consumed slot holds: stale bytes
    return r;
}
static State make_state(uint32_t size, uint32_t start, uint32_t frames, uint32_t fill_free, uint32_t pool_n,
                        uint32_t tx_room, uint32_t comp_used) {
    State s;
    s.rx = make_ring<xsk_gpu_desc>(size, start, frames);
    for (uint32_t i = 0; i < frames; i++) s.rx.ent[(start + i) & (size - 1u)] = fresh_desc();
    s.fill = make_ring<uint64_t>(size, start + 1u, size - fill_free);
    for (uint32_t i = 0; i < size - fill_free; i++) s.fill.ent[(start + 1u + i) & (size - 1u)] = fresh_addr();
    s.tx = make_ring<xsk_gpu_desc>(size, start + 2u, size - tx_room);
    for (uint32_t i = 0; i < size - tx_room; i++) s.tx.ent[(start + 2u + i) & (size - 1u)] = fresh_desc();
    s.comp = make_ring<uint64_t>(size, start + 3u, comp_used);
    for (uint32_t i = 0; i < comp_used; i++) s.comp.ent[(start + 3u + i) & (size - 1u)] = fresh_addr();
    s.pool.capacity = size + 3u;
    s.pool.n_free = pool_n;
    s.pool.addr = exact<uint64_t>(s.pool.capacity);
    memset(s.pool.addr, 0x5A, s.pool.capacity * sizeof(uint64_t));
    for (uint32_t i = 0; i < pool_n && i < s.pool.capacity; i++) s.pool.addr[i] = fresh_addr();
    return s;
}

static uint32_t replies_of(const State& s, uint32_t n) {
    uint32_t R = 0;
    for (uint32_t i = 0; i < n; i++) R += verdict_of(s.rx.ent[(s.rx.cons + i) & (s.rx.size - 1u)]) == XSK_GPU_TX_REPLY;
    return R;
}

static void same_result(const xsk_gpu_rx_result& a, const xsk_gpu_rx_result& b, const char* tag) {
    CHECK(a.received == b.received && a.replied == b.replied && a.tx_full == b.tx_full && a.refilled == b.refilled,
          "%s: result %u %u %u %u against %u %u %u %u", tag, a.received, a.replied, a.tx_full, a.refilled, b.received,
          b.replied, b.tx_full, b.refilled);
}

static uint64_t g_cases = 0, g_cut = 0;

static void one_case(uint32_t size, uint32_t start, uint32_t offered, uint32_t max_batch, uint32_t fill_free,
                     uint32_t pool_n, int room_kind) {
    const uint32_t frames = offered < size ? offered : size;
    State probe = make_state(size, start, frames, fill_free, pool_n, size, 0);
    const uint32_t R = replies_of(probe, frames < max_batch ? frames : max_batch);
    uint32_t room = room_kind == 0 ? 0u : room_kind == 1 ? (R ? R - 1u : 0u) : room_kind == 2 ? R : room_kind == 3 ? R + 1u : size;
    if (room > size) room = size;
    // the same frames again, with the TX ring holding size - room entries
    State base = make_state(size, start, 0, fill_free, pool_n, room, 0);
    free(base.rx.ent);
    base.rx = ring_copy(probe.rx);
    state_free(probe);
    char tag[160];
    snprintf(tag, sizeof tag, "size %u start %u offered %u max_batch %u fill_free %u pool %u room %u", size, start,
             offered, max_batch, fill_free, pool_n, room);
    State h = state_copy(base), d = state_copy(base), sp = state_copy(base);
    const xsk_gpu_rx_result rh = host_step(h, max_batch), rd = dev_step(d, max_batch), rs = spec_step(sp, max_batch);
    same_result(rd, rh, tag);
    same_result(rs, rh, tag);
    state_same(d, h, tag);
    state_same(sp, h, tag);
    if (frames == 0) state_same(d, base, tag);  // nothing received: nothing changes
    g_cut += rh.tx_full != 0;
    state_free(h);
    state_free(d);
    state_free(sp);
    state_free(base);
    g_cases++;
}

static void complete_cases(uint32_t size, uint32_t start) {
    const uint32_t cap = size + 3u;
    const uint32_t useds[] = {0u, 1u, size / 2u, size};
    const uint32_t pools[] = {0u, 1u, cap - 1u, cap, cap > 5u ? cap - 5u : 0u};
    const uint32_t maxes[] = {1u, size, size + 1u, 1024u, 1025u, 5000u};
    for (uint32_t used : useds)
        for (uint32_t pool_n : pools)
            for (uint32_t max : maxes) {
                State base = make_state(size, start, 0, 0, pool_n, size, used);
                State h = state_copy(base), d = state_copy(base), sp = state_copy(base);
                char tag[120];
                snprintf(tag, sizeof tag, "complete size %u start %u used %u pool %u max %u", size, start, used, pool_n, max);
                const uint32_t nh = host_complete(h, max), nd = dev_complete(d, max), ns = spec_complete(sp, max);
                CHECK(nh == nd && nh == ns, "%s: moved %u %u %u", tag, nh, nd, ns);
                state_same(d, h, tag);
                state_same(sp, h, tag);
                state_free(h);
                state_free(d);
                state_free(sp);
                state_free(base);
                g_cases++;
            }
}

// Garbage: the words hold anything.  The device side against the rule, and never outside an array.
static void garbage_cases(uint32_t size) {
    for (int k = 0; k < 400; ++k) {
        State base = make_state(size, (uint32_t)rnd64(), size, size / 2u, size / 2u, size / 2u, size / 2u);
        for (uint32_t i = 0; i < size; i++) {  // every slot holds something comparable
            base.rx.ent[i] = fresh_desc();
            base.tx.ent[i] = fresh_desc();
            base.fill.ent[i] = fresh_addr();
            base.comp.ent[i] = fresh_addr();
        }
        for (uint32_t i = 0; i < base.pool.capacity; i++) base.pool.addr[i] = fresh_addr();
        auto word = [&](uint32_t sane) { return rnd64() % 3u ? (uint32_t)rnd64() : sane; };
        base.rx.prod = word(base.rx.prod);
        base.rx.cons = word(base.rx.cons);
        base.fill.prod = word(base.fill.prod);
        base.fill.cons = word(base.fill.cons);
        base.tx.prod = word(base.tx.prod);
        base.tx.cons = word(base.tx.cons);
        base.comp.prod = word(base.comp.prod);
        base.comp.cons = word(base.comp.cons);
        base.pool.n_free = k % 4 == 0 ? base.pool.capacity + 1u + (uint32_t)(rnd64() % 1000u) : word(base.pool.n_free);
        const uint32_t max_batch = k % 2 ? 1u + (uint32_t)(rnd64() % 1024u) : 1025u + (uint32_t)(rnd64() % 400u);
        char tag[100];
        snprintf(tag, sizeof tag, "garbage size %u case %d max_batch %u", size, k, max_batch);
        State d = state_copy(base), sp = state_copy(base);
        const xsk_gpu_rx_result rd = dev_step(d, max_batch), rs = spec_step(sp, max_batch);
        same_result(rd, rs, tag);
        state_same(d, sp, tag);
        const uint32_t nd = dev_complete(d, max_batch), ns = spec_complete(sp, max_batch);
        CHECK(nd == ns, "%s: complete", tag);
        state_same(d, sp, tag);
        state_free(d);
        state_free(sp);
        // counts above n_max, and a received word above it, in front of end: the clamps keep every lane inside lists
        // of exactly n_max entries
        {
            State e = state_copy(base);
            const uint32_t n_max = 1u + (uint32_t)(rnd64() % 64u);
            xsk_gpu_desc* d_tx = exact<xsk_gpu_desc>(n_max);
            uint64_t* d_free = exact<uint64_t>(n_max);
            for (uint32_t i = 0; i < n_max; i++) {
                d_tx[i] = fresh_desc();
                d_free[i] = fresh_addr();
            }
            RdPlan p;
            memset(&p, 0, sizeof p);
            p.received = n_max + 1u + (uint32_t)(rnd64() % 100000u);
            p.refilled = 7;
            const EgCounts c = {0xFFFFFFFFu, n_max + 1u + (uint32_t)(rnd64() % 1000u), 5u, (uint32_t)rnd64() | 0x80000000u};
            const uint32_t tx_free = rd_free(e.tx.prod, e.tx.cons, e.tx.size), pn = rd_pool_n(e.pool.n_free, e.pool.capacity);
            const uint32_t rx_cons = e.rx.cons;
            const xsk_gpu_rx_result r = dev_end(e, p, d_tx, d_free, c, n_max);
            CHECK(r.received == n_max && e.rx.cons == rx_cons + n_max, "%s: release clamp", tag);
            CHECK(r.replied == (n_max < tx_free ? n_max : tx_free) && r.tx_full == 5u && r.refilled == 7u, "%s: end result", tag);
            CHECK(e.pool.n_free == pn + (n_max < e.pool.capacity - pn ? n_max : e.pool.capacity - pn), "%s: push clamp", tag);
            free(d_tx);
            free(d_free);
            state_free(e);
        }
        state_free(base);
        g_cases++;
    }
}

int main() {
    // the layout of the step's workspace: aligned, disjoint, in order
    const uint32_t bounds[] = {1u, 63u, 64u, 1024u, 1025u, 1300u, 65536u, XSK_GPU_MAX_BATCH};
    for (uint32_t mb : bounds) {
        const RdLayout l = rd_layout(mb);
        CHECK(l.plan == 0 && l.counts == 32 && l.descs == 48 && l.descs % 16 == 0, "layout head");
        CHECK(l.tx == l.descs + (size_t)mb * 16 && l.free_list == l.tx + (size_t)mb * 16 && l.free_list % 8 == 0, "layout lists");
        CHECK(l.verdicts == l.free_list + (size_t)mb * 8 && l.egress >= l.verdicts + mb && l.egress % 4 == 0, "layout tail");
        CHECK(l.bytes >= l.egress + eg_workspace_bytes(mb) && l.bytes % 16 == 0 && l.bytes < l.egress + eg_workspace_bytes(mb) + 16, "layout size");
    }
    CHECK(rd_size_ok(1) && rd_size_ok(0x80000000u) && !rd_size_ok(0) && !rd_size_ok(3) && !rd_size_ok(0xC0000000u), "sizes");
    CHECK(rd_nwg(1025) == 5 && rd_nwg(1024) == 4 && rd_nwg(XSK_GPU_MAX_BATCH) == XSK_GPU_MAX_BATCH / 256u, "grid");

    const uint32_t sizes[] = {1u, 8u, 64u, 4096u};
    const uint32_t offers[] = {0u, 1u, 63u, 64u, 65u, 1024u, 1025u, 1300u};
    for (uint32_t size : sizes) {
        const uint32_t starts[] = {0u, size / 2u + 0x10000u * size, 0xFFFFFFFDu};
        const uint32_t cap = size + 3u;
        for (uint32_t start : starts) {
            for (uint32_t offered : offers) {
                const uint32_t batches[] = {offered ? offered : 1u, offered / 2u ? offered / 2u : 1u, 1025u + offered};
                const uint32_t fills[] = {0u, 1u, size};
                const uint32_t pools[] = {0u, 1u, cap, cap - 1u};
                for (uint32_t mb : batches)
                    for (uint32_t ff : fills)
                        for (uint32_t pn : pools)
                            for (int room_kind = 0; room_kind < 5; ++room_kind)
                                one_case(size, start, offered, mb, ff < size ? ff : size, pn, room_kind);
            }
            complete_cases(size, start);
        }
        garbage_cases(size);
    }
    CHECK(g_cut > 100, "the cut rooms never cut");
    printf("ring dev ok: %llu cases, %llu with a reply left out\n", (unsigned long long)g_cases, (unsigned long long)g_cut);
    return 0;
}
