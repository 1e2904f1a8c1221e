// xsk_loop_fused_body.h — the RX loop body as one launch of one workgroup: the kernel of xsk_gpu_rx_fused_loop_dev()
// (include/xsk_gpu.h).  The seven stages of xsk_gpu_rx_loop_dev() at a bound of at most 1024 frames
// -- begin, prepare, steer, transform, egress per port, end, completion -- run one after another in 1024 threads, each
// behind a fence and a workgroup barrier where the loop call has a kernel boundary.  The fence between two stages is of
// workgroup scope: writer and reader are waves of this one workgroup on one CU, and with `__threadfence()` there (an L2
// write-back and an invalidate per stage) the kernel was no faster than the chain of launches.  The
// `__threadfence()` in front of every publish of index words is the stage bodies' own and stays.  Every stage but the steering
// compaction is the one-workgroup body of the loop call's own small kernel, from the device headers those kernels are
// built from; the compaction is new (steer_small(), the slot arithmetic in xsk_steer.h).  Three instances: reference
// mode and wire mode in xsk_loop_fused.hip, the dual-stack one in xsk_loop_fused_ds.hip (its own compiler flag).
//
// Kernel arguments: the up to 132 rings travel packed (xsk_ring_pack.h, 24 B each) and are unpacked into LDS first, so
// that the stage bodies take them as the Rings / CompRings they know.  Words the kernel wrote itself -- the plan, d_off,
// the rooms, the counts, the pool's count word -- reach a later stage through LDS (the plan, the received count, the
// REDIRECT total) or are read back behind that fence and barrier through pointers that carry no `const __restrict__`;
// every index word goes through load_word.  All stores are vector stores from plain C++.  The stages' LDS is one union:
// the transform's Echo6Smem is the largest member.
#ifndef XSK_LOOP_FUSED_BODY_H
#define XSK_LOOP_FUSED_BODY_H

#include "xsk_echo_device.h"
#include "xsk_egress_ports_device.h"
#include "xsk_neigh_device.h"
#include "xsk_ring_complete_device.h"
#include "xsk_ring_dev_device.h"
#include "xsk_ring_pack.h"
#include "xsk_ring_pass_device.h"
#include "xsk_ring_ports_device.h"
#include "xsk_steer.h"

namespace xskgpu {
namespace {

constexpr uint32_t kLfThreads = 1024;
constexpr uint32_t kLfMax = XSK_GPU_LOWLAT_MAX;
static_assert(kLfThreads == (uint32_t)kThreads6 && kLfThreads == kRdSmallThreads && kLfThreads == kEgSmallThreads &&
                  kLfThreads == kPsSmallThreads && kLfThreads == kRcSmallThreads && kLfThreads == kSt1Frames,
              "every stage is the one-workgroup form of 1024 threads");
static_assert(kLfMax == kRdSmallMax && kLfMax == kPsSmallMax && kLfMax == kRcSmallMax, "and serves up to 1024 frames");

// The kernel's arguments, one struct by value.
struct LoopFusedArgs {
    PackedRing tx[kEpMaxPorts];    // ports at or above n_ports: the absent ring
    PackedRing comp[kRcMaxRings];  // rings at or above n_comp: the absent ring
    PackedRing rx, fill, stack;    // stack: the absent ring for NULL
    Pool pool;
    uint8_t* umem;
    uint64_t umem_size;
    const xsk_gpu_steer_entry* table;
    const uint64_t* d_bound;
    uint8_t* d_actions;  // the caller's or NULL (then the workspace's), as d_ports and d_port_counts
    uint8_t* d_ports;
    xsk_gpu_egress_counts* d_port_counts;
    xsk_gpu_stats* d_stats;
    xsk_gpu_stats* d_port_stats;
    xsk_gpu_rx_pass_result* d_res;
    uint32_t* d_moved;
    uint32_t* d_pushed;
    uint8_t* ws;
    RpLayout l;  // the workspace's layout, xsk_gpu_rx_pass_step_dev_workspace_size()'s
    uint32_t max_batch, opts, n_entries, default_port, n_ports, n_comp, complete_max;
};
// the argument segment holds 4096 B, and the 256 B of hidden arguments behind the explicit ones count
static_assert(sizeof(LoopFusedArgs) + 256 <= 4096, "the kernel arguments");

__device__ __forceinline__ Ring lf_ring_dev(const PackedRing& p) {
    const UnpackedRing u = pk_unpack(p);
    return Ring{(uint32_t*)u.prod, (uint32_t*)u.cons, (void*)u.ring, u.size};
}
inline PackedRing lf_pack(const xsk_gpu_ring_dev* r) {  // NULL: the absent ring, { NULL, NULL, NULL, 1 }
    return r ? pk_pack((uint64_t)(uintptr_t)r->d_producer, (uint64_t)(uintptr_t)r->d_consumer,
                       (uint64_t)(uintptr_t)r->d_ring, r->size)
             : pk_pack(0u, 0u, 0u, 1u);
}

// The steering stage's LDS: the staged table, the count matrix, the ports' first slots.
struct SteerLds {
    __attribute__((aligned(16))) uint32_t tab[kStMaxEntries * kStEntryWords];  // 24 KiB
    uint32_t cnt[kSt1Waves][kStMaxPorts];                                      // 4 KiB
    uint32_t base[kStMaxPorts];
};
struct EgressLds {
    EpLds s;
    EpAcc acc;
    uint32_t s_w[kEgSmallWaves];
    uint64_t s_m[kEgSmallWaves];
};
struct EndStageLds {
    EndLds s;
    uint32_t s_wn[kPsSmallWaves], s_wq[kPsSmallWaves];
    uint64_t s_rest[kPsSmallMax];
};
// The stages' needs are disjoint in time: one overlay.  What outlives a stage stands beside it.
union LoopStageLds {
    SteerLds steer;
    Echo6Smem<1> echo;
    EgressLds egress;
    EndStageLds end;
    CompLds comp;
    NgServeLds serve;  // the responder's stage behind the loop body (xsk_responder_body.h); smaller than echo
};
static_assert(sizeof(NgServeLds) <= sizeof(Echo6Smem<1>), "the serve stage adds nothing to the overlay");
// Where the stages' arrays are: the workspace's, or the caller's where the caller gave one.  In LDS, so that no stage
// holds them in scalar registers across the transform's body.
struct LoopPtrs {
    xsk_gpu_rx_plan* plan;
    uint32_t* room;
    uint32_t* off;
    xsk_gpu_egress_counts* counts;
    xsk_gpu_desc* descs;
    xsk_gpu_desc* out;
    xsk_gpu_desc* d_tx;
    uint64_t* d_free;
    uint8_t* verdicts;
    uint8_t* actions;
    uint8_t* ports;
};
struct LoopFusedLds {
    LoopStageLds u;
    Rings tx;        // unpacked from the arguments
    CompRings comp;
    Ring rx, fill, stack;
    LoopPtrs p;      // the workspace's arrays and the caller's outputs, resolved once
    RdPlan plan;     // stage 1's, read by every later stage that needs the received count
    uint32_t total;  // the REDIRECT count, d_off[n_ports]
};
static_assert(sizeof(LoopFusedLds) <= 160u * 1024u, "the CU's LDS");

__device__ __forceinline__ void lf_stage_fence() {
    // what a stage stored before what the next one reads: both are waves of this one workgroup, on one CU
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Stage 3, the one-workgroup form of xsk_gpu_steer_dev() over descs[0, r): d_actions and d_ports over all n_max entries
// (an entry at or above r is what the pad descriptor would make it: DROP, XSK_GPU_STEER_PASS), the REDIRECT descriptors
// as a stable partition by port in out[], d_off[0 .. n_ports].  Returns nothing; the total is left in *s_total.
__device__ __forceinline__ void steer_small(const uint8_t* umem, uint64_t umem_size, const xsk_gpu_desc* descs, uint32_t r,
                                            uint32_t n_max, uint32_t opts, const xsk_gpu_steer_entry* table,
                                            uint32_t n_entries, uint32_t default_port, uint32_t n_ports,
                                            const uint64_t* d_bound, uint8_t* actions, uint8_t* ports, xsk_gpu_desc* out,
                                            uint32_t* d_off, SteerLds* s, uint32_t* s_total) {
    const uint32_t t = threadIdx.x;
    for (uint32_t k = t; k < n_entries; k += kLfThreads) st_stage_entry(table + k, s->tab + k * kStEntryWords);
    (&s->cnt[0][0])[t] = 0u;  // kSt1Waves * kStMaxPorts == kLfThreads
    const unsigned long long bound = d_bound ? *d_bound : ~0ull;
    __syncthreads();
    StVerdict v = {XSK_GPU_XDP_DROP, kStPass};
    uint4 d = make_uint4(0u, 0u, 0u, 0u);
    if (t < r) {
        d = reinterpret_cast<const uint4*>(descs)[t];
        xsk_gpu_desc dd;
        dd.addr = ((uint64_t)d.y << 32) | d.x;
        dd.len = d.z;
        dd.options = d.w;
        v = st_steer_one(umem, umem_size, dd, opts, s->tab, n_entries, default_port, n_ports, bound);
    }
    if (t < n_max) {
        actions[t] = (uint8_t)v.act;
        ports[t] = (uint8_t)v.port;
    }
    const bool red = v.act == XSK_GPU_XDP_REDIRECT;
    const uint32_t port = v.port & (kStMaxPorts - 1u);  // (a REDIRECT frame's port is below n_ports <= 64)
    const uint32_t rank = wave_ranks(red, port, s->cnt);
    __syncthreads();
    if (t < kStWave) {  // wave 0, a lane per port: the column sums and their exclusive prefix
        const uint32_t tot = t < n_ports ? st1_port_total(s->cnt, t) : 0u;
        uint32_t inc = tot;
        for (uint32_t o = 1; o < kStWave; o <<= 1) {
            const uint32_t u = __shfl_up(inc, o, kStWave);
            inc += t >= o ? u : 0u;
        }
        s->base[t] = inc - tot;
        if (t < n_ports) d_off[t] = inc - tot;
        if (t == n_ports - 1u) {
            d_off[n_ports] = inc;
            *s_total = inc;
        }
    }
    __syncthreads();
    if (red) reinterpret_cast<uint4*>(out)[st1_slot(s->base[port], st1_lower_waves(s->cnt, cp_wave(), port), rank)] = d;
}
static_assert(kSt1Waves * kStMaxPorts == kLfThreads && kStMaxPorts == kStWave, "the zeroing and the lane per port above");

// Stage 7's decision: xsk_ring_complete.hip's comp_decide, stated again here because that file keeps its own (see
// xsk_ring_complete_device.h).  Every lane of the workgroup calls it; two barriers.  Lanes walk the rings in strides of
// the workgroup's size.
__device__ __forceinline__ void lf_comp_decide(const CompRings& comp, uint32_t n_rings, const Pool& pool, uint32_t max,
                                            CompLds* s) {
    const uint32_t t = threadIdx.x, nt = blockDim.x;
    for (uint32_t q = t; q < n_rings; q += nt) {
        const Ring& ring = comp.r[q];
        const uint32_t cons = load_word(ring.cons);
        s->cons[q] = cons;
        s->n[q] = rc_take(load_word(ring.prod), cons, ring.size, max);
    }
    if (t == 0) s->pool_n = rd_pool_n(load_word(pool.n_free), pool.capacity);
    __syncthreads();
    const uint32_t room = rc_room(s->pool_n, pool.capacity);
    for (uint32_t q = t; q <= n_rings; q += nt) s->A[q] = rc_prefix(s->n, q, room);
    __syncthreads();
}

// The kernel's body.  C is the transform's config: RoundCfg<WIRE, true, V6>, the sub-tile form.
template <class C>
__device__ __forceinline__ void loop_fused_body(const LoopFusedArgs& A, LoopFusedLds& L) {
    static_assert(C::SUBT && C::TPW == 1 && !C::TRACE && !C::DLDS, "the sub-tile config");
    const uint32_t t = threadIdx.x;
    // ---- the rings, from the arguments into LDS ----
    if (t < kEpMaxPorts) L.tx.r[t] = lf_ring_dev(A.tx[t]);
    else if (t - kEpMaxPorts < kRcMaxRings) L.comp.r[t - kEpMaxPorts] = lf_ring_dev(A.comp[t - kEpMaxPorts]);
    else if (t == kEpMaxPorts + kRcMaxRings) L.rx = lf_ring_dev(A.rx);
    else if (t == kEpMaxPorts + kRcMaxRings + 1u) L.fill = lf_ring_dev(A.fill);
    else if (t == kEpMaxPorts + kRcMaxRings + 2u) L.stack = lf_ring_dev(A.stack);
    else if (t == kEpMaxPorts + kRcMaxRings + 3u) {
        uint8_t* const ws = A.ws;
        L.p.plan = (xsk_gpu_rx_plan*)(ws + A.l.plan);
        L.p.room = (uint32_t*)(ws + A.l.room);
        L.p.off = (uint32_t*)(ws + A.l.off);
        L.p.counts = A.d_port_counts ? A.d_port_counts : (xsk_gpu_egress_counts*)(ws + A.l.counts);
        L.p.descs = (xsk_gpu_desc*)(ws + A.l.descs);
        L.p.out = (xsk_gpu_desc*)(ws + A.l.out);
        L.p.d_tx = (xsk_gpu_desc*)(ws + A.l.tx);
        L.p.d_free = (uint64_t*)(ws + A.l.free_list);
        L.p.verdicts = ws + A.l.verdicts;
        L.p.actions = A.d_actions ? A.d_actions : ws + A.l.actions;
        L.p.ports = A.d_ports ? A.d_ports : ws + A.l.ports;
    }
    const Pool pool = A.pool;
    const uint32_t n_max = A.max_batch, n_ports = A.n_ports;
    __syncthreads();
    const Ring &rx = L.rx, &fill = L.fill, &stack = L.stack;  // (in LDS, not in SGPRs across the transform's body)
    const LoopPtrs& P = L.p;

    // ---- 1. begin (xsk_gpu_rx_begin_dev(): tx[0] is the ring whose room the plan records) ----
    const RdPlan p = rx_begin_small_body(rx, fill, L.tx.r[0], pool, n_max, P.descs, P.plan, &L.plan);
    const uint32_t r = rp_received(p.received, n_max);
    // ---- 2. prepare: every port's TX room.  r is known to every lane, so no pad descriptor is written ----
    if (t < n_ports) P.room[t] = rd_free(load_word(L.tx.r[t].prod), load_word(L.tx.r[t].cons), L.tx.r[t].size);
    lf_stage_fence();

    // ---- 3. steer ----
    steer_small(A.umem, A.umem_size, P.descs, r, n_max, A.opts, A.table, A.n_entries, A.default_port, n_ports, A.d_bound,
                P.actions, P.ports, P.out, P.off, &L.u.steer, &L.total);
    lf_stage_fence();

    // ---- 4. transform: echo6_body over out[0, total), tiled as the resident kernels tile a batch ----
    {
        EchoArgs a;
        a.umem = A.umem;
        a.umem_size = A.umem_size;
        a.descs = P.out;
        a.n = uniform(L.total);  // (outside the union: the body's LDS does not overlay it)
        a.verdicts = P.verdicts;
        a.recs = nullptr;
        a.partials = nullptr;
        a.opts = A.opts;
        a.stats_direct = A.d_stats ? (unsigned long long*)&A.d_stats->rx_packets : nullptr;  // device-scope atomics
        uint32_t tl = ((a.n + kWaves6 - 1) / kWaves6 + 3u) & ~3u;
        tl = tl < 4u ? 4u : (tl > (uint32_t)kTile ? (uint32_t)kTile : tl);
        a.tile_live = tl;
        const uint32_t ntiles = (a.n + tl - 1) / tl;
        if (ntiles) echo6_body<C>(a, 0u, ntiles, L.u.echo);  // workgroup-uniform
    }
    lf_stage_fence();

    // ---- 5. egress per port ----
    egress_ports_small_body(P.out, P.verdicts, P.off, n_ports, n_max, P.room, P.d_tx, P.d_free, P.counts, A.d_stats,
                            A.d_port_stats, L.u.egress.s, L.u.egress.acc, L.u.egress.s_w, L.u.egress.s_m);
    lf_stage_fence();

    // ---- 6. end ----
    rx_pass_end_small_body(rx, L.tx, n_ports, stack, pool, P.plan, P.descs, P.actions, P.off, P.d_tx, P.d_free, P.counts,
                           n_max, A.d_res, L.u.end.s, L.u.end.s_wn, L.u.end.s_wq, L.u.end.s_rest);
    if (!A.n_comp) return;  // workgroup-uniform
    // ---- 7. completion: reads the pool's count word behind end's publish and this barrier ----
    lf_stage_fence();
    if (A.complete_max == 0) {  // as the loop call's two memsets
        if (t < A.n_comp && A.d_moved) A.d_moved[t] = 0u;
        if (t == 0 && A.d_pushed) *A.d_pushed = 0u;
        return;
    }
    tx_complete_rings_small_body(L.comp, A.n_comp, pool, A.complete_max, A.d_moved, A.d_pushed, &L.u.comp, lf_comp_decide);
}

}  // namespace
}  // namespace xskgpu

#endif  // XSK_LOOP_FUSED_BODY_H
