// xsk_neigh_device.h — the one-workgroup body of xsk_gpu_neigh_serve_dev()'s kernel as a function that takes its LDS
// from its caller, as §9.11 has the other stage bodies (include/xsk_gpu.h, "Neighbour responder"; DESIGN.md §9.13,
// §9.15).  The responder kernels (xsk_responder_body.h) call it behind the RX loop's stages with the rings that body has
// already unpacked.  xsk_neigh.hip keeps its own text of the body and of the three helpers below (see there: called
// from that kernel, this function changed the order of its instructions), so they are stated again here under ng_
// names, and tests/test_responder_spec.py holds the two texts against each other.  The decision, the lookup, the
// rewrites and the serve plan are xsk_neigh.h's (host and device), one text for all.
#ifndef XSK_NEIGH_DEVICE_H
#define XSK_NEIGH_DEVICE_H

#include "xsk_hip_util.h"
#include "xsk_neigh.h"
#include "xsk_ring_dev.h"
#include "xsk_ring_ports_device.h"
#include "xsk_steer.h"

namespace xskgpu {
namespace {

typedef unsigned long long u64;

constexpr uint32_t kNgServeThreads = kSt1Frames;  // the serve call's one workgroup
constexpr uint32_t kNgServeWaves = kSt1Waves;
constexpr uint32_t kNgStack = kNgDests;           // the stack ring's place behind the 65 destinations
constexpr uint32_t kNgRings = kNgDests + 1u;
static_assert(kNgServeThreads == XSK_GPU_LOWLAT_MAX && kNgServeWaves * kStMaxPorts == kNgServeThreads,
              "a lane per entry, and a lane per word of the count matrix");

// The counters of one wave into s_red[wave]: seen, ARP replies, NAs, reply bytes.
__device__ __forceinline__ void ng_wave_counters(bool seen, const NgVerdict& v, u64 (*s_red)[4]) {
    const u64 ms = __ballot(seen), ma = __ballot(seen && v.verdict == XSK_GPU_NEIGH_ARP_REPLY),
              mn = __ballot(seen && v.verdict == XSK_GPU_NEIGH_NA_REPLY);
    const u64 bytes = cp_wave_sum(seen && ng_is_reply(v.verdict) ? (u64)v.reply_len : 0ull);
    if (cp_lane() == 0) {
        s_red[cp_wave()][0] = (u64)__popcll(ms);
        s_red[cp_wave()][1] = (u64)__popcll(ma);
        s_red[cp_wave()][2] = (u64)__popcll(mn);
        s_red[cp_wave()][3] = bytes;
    }
}
// Behind the barrier: thread w < 4 adds the workgroup's sum of word w, when it is not zero.
template <uint32_t NW>
__device__ __forceinline__ void ng_add_counters(const u64 (*s_red)[4], xsk_gpu_neigh_stats* nstats) {
    const uint32_t w = threadIdx.x;
    if (w >= 4u || !nstats) return;
    u64 sum = 0;
    for (uint32_t k = 0; k < NW; ++k) sum += s_red[k][w];
    if (sum) atomicAdd(reinterpret_cast<u64*>(nstats) + w, sum);
}

__device__ __forceinline__ xsk_gpu_desc ng_desc_of(const uint4& r) {
    xsk_gpu_desc d;
    d.addr = ((uint64_t)r.y << 32) | r.x;
    d.len = r.z;
    d.options = r.w;
    return d;
}

// The serve call's scalar arguments, by these names in whatever struct the caller hands the body.
struct NgServeParams {
    uint8_t* umem;
    uint64_t umem_size;
    const xsk_gpu_neigh_entry* table;
    const uint64_t* d_bound;
    xsk_gpu_neigh_stats* d_nstats;
    xsk_gpu_neigh_result* d_res;
    uint32_t n_ports, max, opts, n_entries;
};

// The serve call's LDS as one struct, for a kernel that overlays it with other stages' (xsk_loop_fused_body.h).
struct NgServeLds {
    __attribute__((aligned(16))) uint32_t tab[kNgMaxEntries * kNgEntryWords];  // 32 KiB
    Ring ring[kNgRings];  // tx[0 .. 64), up, stack
    uint32_t cnt[kNgServeWaves][kStMaxPorts];
    u64 red[kNgServeWaves][4];
    uint32_t prod[kNgDests], room[kNgDests];
    uint32_t wu[kNgServeWaves], wstop[kNgServeWaves];
    uint32_t cons, used;
};

// The serve call's one workgroup of 1024 threads, statement for statement the body of neigh_serve_kernel (xsk_neigh.hip,
// which keeps its own text: see there); every lane calls it.  A has the members of NgServeParams, read where they are
// used.  ring_at(k), k < kNgRings, is ring k -- port k's TX ring (the absent ring at or above n_ports), `up` at kNgUp,
// the stack ring at kNgStack -- and lane k asks for it once.  Every index word is read here, through load_word, as it
// is when this function runs, and the table is staged here: a caller that ran other stages first calls it behind a
// fence and a barrier and hands in nothing it read before them.
template <class Args, class RingAt>
__device__ __forceinline__ void ng_serve_body(const Args& A, RingAt ring_at, uint32_t* s_tab,
                                              Ring (&s_ring)[kNgRings], uint32_t (&s_cnt)[kNgServeWaves][kStMaxPorts],
                                              u64 (&s_red)[kNgServeWaves][4], uint32_t (&s_prod)[kNgDests],
                                              uint32_t (&s_room)[kNgDests], uint32_t (&s_wu)[kNgServeWaves],
                                              uint32_t (&s_wstop)[kNgServeWaves], uint32_t& s_cons, uint32_t& s_used) {
    const uint32_t t = threadIdx.x;
    for (uint32_t k = t; k < A.n_entries; k += kNgServeThreads) ng_stage_entry(A.table + k, s_tab + k * kNgEntryWords);
    (&s_cnt[0][0])[t] = 0u;
    if (t < kNgRings) {  // a lane per ring: unpack, and the index words as they are at execution
        const Ring r = ring_at(t);
        s_ring[t] = r;
        if (t == kNgStack) {
            const uint32_t cons = load_word(r.cons);
            s_cons = cons;
            s_used = rd_used(load_word(r.prod), cons, r.size);
        } else if (t == kNgUp || t < A.n_ports) {
            const uint32_t prod = load_word(r.prod);
            s_prod[t] = prod;
            s_room[t] = rd_free(prod, load_word(r.cons), r.size);
        } else {
            s_prod[t] = 0u;
            s_room[t] = 0u;
        }
    }
    const u64 bound = A.d_bound ? *A.d_bound : ~0ull;
    __syncthreads();
    // 1. every lane decides its entry
    const uint32_t m = ng_serve_m(s_used, A.max);
    const bool live = t < m;
    NgVerdict v = {XSK_GPU_NEIGH_NONE, 0xFFu, 0u, 14u, 0u, 0u};
    uint4 raw = make_uint4(0u, 0u, 0u, 0u);
    if (live) {
        raw = *desc_slot(s_ring[kNgStack], s_cons + t);
        v = ng_decide(A.umem, A.umem_size, ng_desc_of(raw), A.opts, s_tab, A.n_entries, A.n_ports, bound);
    }
    // 2. the rank among the lower entries with the same destination
    const bool reply = live && ng_is_reply(v.verdict);
    const uint32_t port = reply ? v.port & (kStMaxPorts - 1u) : 0u;  // (a reply's port is below n_ports <= 64)
    const uint32_t in_wave = wave_ranks(reply, port, s_cnt);
    const u64 mu = cp_wg_ballot(live && !reply, s_wu);
    const uint32_t dest = ng_dest(v.verdict, port);  // (a lane without an entry: NONE, up; it is not below m)
    const uint32_t rank = reply ? st1_lower_waves(s_cnt, cp_wave(), port) + in_wave
                                : cp_waves_below<kNgServeWaves>(s_wu, cp_wave(), 0u) + cp_below(mu, cp_lane());
    // 3. c: the lowest lane whose rank is not below its destination's room
    const u64 ms = __ballot(ng_stop_at(t, m, rank, s_room[dest]) != m);
    if (cp_lane() == 0) s_wstop[cp_wave()] = ms ? cp_wave() * kStWave + (uint32_t)__builtin_ctzll(ms) : m;
    __syncthreads();
    uint32_t c = m;
    for (uint32_t k = 0; k < kNgServeWaves; ++k) c = rd_min(c, s_wstop[k]);
    // 4. the lanes below c rewrite and store
    const bool handled = t < c;
    if (handled) {
        const xsk_gpu_desc e = ng_desc_of(raw);
        if (reply) ng_rewrite(A.umem + e.addr, v);
        const xsk_gpu_desc o = ng_out_entry(e, v);
        *desc_slot(s_ring[dest], s_prod[dest] + rank) =
            make_uint4((uint32_t)o.addr, (uint32_t)(o.addr >> 32), o.len, o.options);
    }
    // what every port received: the partition again over the handled replies.  A thread zeroes a word of its own
    // wave's row, which only its own wave writes; every read of the first matrix lies in front of the barrier above.
    (&s_cnt[0][0])[t] = 0u;
    wave_ranks(reply && handled, port, s_cnt);
    ng_wave_counters(handled, v, s_red);
    __threadfence();  // the entries before the words that cover them
    __syncthreads();
    // 5. wave 0 publishes
    if (t >= kStWave) return;
    if (t < A.n_ports) {
        const uint32_t got = st1_port_total(s_cnt, t);
        if (got) *s_ring[t].prod = s_prod[t] + got;
    }
    if (t == 0) {
        u64 arp = 0, na = 0;
        for (uint32_t k = 0; k < kNgServeWaves; ++k) {
            arp += s_red[k][1];
            na += s_red[k][2];
        }
        const uint32_t n_up = c - (uint32_t)arp - (uint32_t)na;
        if (n_up) *s_ring[kNgUp].prod = s_prod[kNgUp] + n_up;
        if (c) *s_ring[kNgStack].cons = s_cons + c;
        if (A.d_res) {
            A.d_res->consumed = c;
            A.d_res->arp_replies = (uint32_t)arp;
            A.d_res->na_replies = (uint32_t)na;
            A.d_res->up = n_up;
            A.d_res->backlog = s_used - c;
            A.d_res->reserved[0] = 0u;
            A.d_res->reserved[1] = 0u;
            A.d_res->reserved[2] = 0u;
        }
    }
    ng_add_counters<kNgServeWaves>(s_red, A.d_nstats);
}

}  // namespace
}  // namespace xskgpu

#endif  // XSK_NEIGH_DEVICE_H
