// xsk_egress_ports_device.h — the device code xsk_egress_ports.hip's kernels share (xsk_gpu_egress_ports_dev(),
// DESIGN.md §9.5): what a workgroup stages of the offsets and the rooms (EpLds, ep_stage), the per-port sums that meet
// in LDS before the global atomics (EpAcc), a frame's store and its counters (ep_finish), and the whole one-workgroup
// form (egress_ports_small_body), which is also stage 5 of the fused loop kernel (xsk_loop_fused_body.h, §9.11).  The
// arithmetic is xsk_egress_ports.h's.  Everything here is in an anonymous namespace: nothing is exported.
#ifndef XSK_EGRESS_PORTS_DEVICE_H
#define XSK_EGRESS_PORTS_DEVICE_H

#include <hip/hip_runtime.h>

#include "../../include/xsk_gpu.h"
#include "xsk_egress_ports.h"

namespace xskgpu {
namespace {

typedef unsigned long long u64;

// What the prologue stages per workgroup: the offsets o_p, the prefixes G(o_p), the rooms.
struct EpLds {
    uint32_t o[kEpMaxBounds];
    uint32_t g[kEpMaxBounds];
    uint32_t room[kEpMaxPorts];
};

// Per-port sums of one workgroup, met in LDS before the global atomics.
struct EpAcc {
    u64 bytes[kEpMaxPorts], tx_bytes[kEpMaxPorts], unsent_bytes[kEpMaxPorts];
    uint32_t n[kEpMaxPorts], n_tx[kEpMaxPorts], n_unsent[kEpMaxPorts];
};

// The prologue (wave 0; the caller's next barrier publishes it): lane l takes word l, an inclusive max-scan over the
// wave leaves max(d_off[0..l]), the clamp makes it o_l; with 64 ports lane 63 adds the 65th word.  Only
// d_off[0, n_ports] and d_room[0, n_ports) are read.
template <bool ROOMS>
__device__ __forceinline__ void ep_stage(const uint32_t* __restrict__ d_off, uint32_t n_ports, uint32_t n_max,
                                         const uint32_t* __restrict__ d_room, EpLds* s) {
    if (cp_wave() != 0) return;
    const uint32_t l = cp_lane();
    uint32_t w = l <= n_ports ? d_off[l] : 0u;
    for (uint32_t d = 1; d < kEgWave; d <<= 1) {
        const uint32_t v = __shfl_up(w, d, kEgWave);
        if (l >= d) w = ep_max(w, v);
    }
    if (l <= n_ports) s->o[l] = ep_clamp(w, n_max);
    if (n_ports == kEpMaxPorts && l == kEgWave - 1u) s->o[kEpMaxPorts] = ep_clamp(ep_max(w, d_off[kEpMaxPorts]), n_max);
    if (ROOMS && l < n_ports) s->room[l] = eg_room(d_room != nullptr, d_room ? d_room[l] : 0u);
}

__device__ __forceinline__ void acc_zero(EpAcc* a) {
    const uint32_t t = threadIdx.x;
    if (t < kEpMaxPorts) {
        a->bytes[t] = a->tx_bytes[t] = a->unsent_bytes[t] = 0ull;
        a->n[t] = a->n_tx[t] = a->n_unsent[t] = 0u;
    }
}

// A lane's frame i with g_i = G(i): its owner from the staged offsets, its slot, the store ({ addr, len, 0 } as one 16-B
// store, or the address as one 8-B store), and -- only when a counter block was given -- the per-port sums.  A port's
// frames are consecutive lanes, so most waves lie inside one port: such a wave reduces by ballots and shuffles and its
// lane 0 adds to the port's LDS cells; a wave that holds a boundary adds lane by lane.  After the barrier wave 0, a lane
// per port, issues the device-scope atomics: four into d_port_stats[p] for a port with frames here, and one pair into
// d_stats for the whole workgroup, none when no reply of it lies past its port's room.  On the three-stage path
// (`part` given) the port that owns the workgroup's first position leaves its sums as a record instead, part[wg], for
// egress_ports_sum_kernel: with few ports nearly every workgroup's set would otherwise meet on one block.
__device__ __forceinline__ void ep_finish(const uint4& d, bool reply, uint32_t i, uint32_t g_i, const EpLds* s,
                                          uint32_t n_ports, xsk_gpu_desc* __restrict__ tx,
                                          uint64_t* __restrict__ free_list, xsk_gpu_stats* stats,
                                          xsk_gpu_stats* port_stats, EpAcc* acc, EpPart* part, uint32_t wg) {
    const EpOwner ow = ep_owner(s->o, n_ports, i);
    bool sub = false, uns = false;
    if (ow.on) {
        const uint32_t o_p = s->o[ow.port], g_p = s->g[ow.port], room = s->room[ow.port];
        const EgSlot sl = ep_slot(reply, i, o_p, g_i, g_p, room);
        eg_store_frame(d, sl, tx, free_list);
        sub = sl.tx;
        uns = ep_unsent(reply, g_i, g_p, room);
    }
    if (!stats && !port_stats) return;  // kernel-uniform
    const uint32_t key = ow.on ? ow.port : 0xFFFFFFFFu;
    const uint32_t k0 = __shfl(key, 0, kEgWave);
    const u64 mu = stats ? __ballot(uns) : 0ull;
    if (__all(key == k0)) {
        if (k0 != 0xFFFFFFFFu && (port_stats || mu)) {  // wave-uniform
            const u64 ms = __ballot(sub);
            u64 b = 0, bt = 0, bu = 0;
            if (port_stats) b = cp_wave_sum((u64)d.z);
            if (port_stats && ms) bt = cp_wave_sum(sub ? (u64)d.z : 0ull);
            if (mu) bu = cp_wave_sum(uns ? (u64)d.z : 0ull);
            if (cp_lane() == 0) {
                if (port_stats) {
                    atomicAdd(&acc->n[k0], kEgWave);
                    atomicAdd(&acc->bytes[k0], b);
                    if (ms) {
                        atomicAdd(&acc->n_tx[k0], (uint32_t)__popcll(ms));
                        atomicAdd(&acc->tx_bytes[k0], bt);
                    }
                }
                if (mu) {
                    atomicAdd(&acc->n_unsent[k0], (uint32_t)__popcll(mu));
                    atomicAdd(&acc->unsent_bytes[k0], bu);
                }
            }
        }
    } else if (ow.on) {
        if (port_stats) {
            atomicAdd(&acc->n[ow.port], 1u);
            atomicAdd(&acc->bytes[ow.port], (u64)d.z);
            if (sub) {
                atomicAdd(&acc->n_tx[ow.port], 1u);
                atomicAdd(&acc->tx_bytes[ow.port], (u64)d.z);
            }
        }
        if (stats && uns) {
            atomicAdd(&acc->n_unsent[ow.port], 1u);
            atomicAdd(&acc->unsent_bytes[ow.port], (u64)d.z);
        }
    }
    __syncthreads();
    if (cp_wave() != 0) return;
    const uint32_t p = cp_lane();
    uint32_t nu = 0, carry = 0xFFFFFFFFu;
    u64 bu = 0;
    if (part && port_stats && ep_wg_carries(wg, s->o[0], s->o[n_ports]))  // wave-uniform
        carry = ep_owner(s->o, n_ports, wg * kEgFrames).port;
    if (p < n_ports) {
        if (port_stats && p == carry) {
            EpPart* r = part + wg;
            r->n = acc->n[p];
            r->n_tx = acc->n_tx[p];
            r->bytes_lo = (uint32_t)acc->bytes[p];
            r->bytes_hi = (uint32_t)(acc->bytes[p] >> 32);
            r->tx_bytes_lo = (uint32_t)acc->tx_bytes[p];
            r->tx_bytes_hi = (uint32_t)(acc->tx_bytes[p] >> 32);
        } else if (port_stats && acc->n[p]) {
            xsk_gpu_stats* ps = port_stats + p;
            atomicAdd((u64*)&ps->rx_packets, (u64)acc->n[p]);
            atomicAdd((u64*)&ps->rx_bytes, acc->bytes[p]);
            if (acc->n_tx[p]) {
                atomicAdd((u64*)&ps->tx_packets, (u64)acc->n_tx[p]);
                atomicAdd((u64*)&ps->tx_bytes, acc->tx_bytes[p]);
            }
        }
        if (stats) {
            nu = acc->n_unsent[p];
            bu = acc->unsent_bytes[p];
        }
    }
    if (stats) {
        const u64 c = cp_wave_sum((u64)nu);
        const u64 t = cp_wave_sum(bu);
        if (p == 0 && c) {
            atomicAdd((u64*)&stats->tx_packets, 0ull - c);
            atomicAdd((u64*)&stats->tx_bytes, 0ull - t);
        }
    }
}

// ---- n_max <= 1024: everything in one workgroup of kEgSmallThreads.  Its LDS, and the body every lane calls ----
// (s, acc, s_w[kEgSmallWaves] and s_m[kEgSmallWaves] are the caller's, in LDS: as one struct the kernel came out as other
// instructions)
constexpr uint32_t kEgSmallWaves = kEgSmallThreads / kEgWave;
// (no __restrict__ here: in the fused kernel every list is one that kernel wrote itself)
__device__ __forceinline__ void egress_ports_small_body(const xsk_gpu_desc* descs, const uint8_t* verdicts,
                                                        const uint32_t* d_off, uint32_t n_ports, uint32_t n_max,
                                                        const uint32_t* d_room, xsk_gpu_desc* tx, uint64_t* free_list,
                                                        xsk_gpu_egress_counts* counts, xsk_gpu_stats* stats,
                                                        xsk_gpu_stats* port_stats, EpLds& s, EpAcc& acc, uint32_t (&s_w)[kEgSmallWaves],
                                                        uint64_t (&s_m)[kEgSmallWaves]) {
    constexpr uint32_t NW = kEgSmallThreads / kEgWave;
    const uint32_t t = threadIdx.x;
    ep_stage<true>(d_off, n_ports, n_max, d_room, &s);
    acc_zero(&acc);
    __syncthreads();
    uint4 d;
    const bool reply = eg_load_frame(descs, verdicts, t, s.o[0], s.o[n_ports], &d);
    const u64 m = __ballot(reply);
    if (cp_lane() == 0) {
        s_w[cp_wave()] = (uint32_t)__popcll(m);
        s_m[cp_wave()] = m;
    }
    __syncthreads();
    if (t <= n_ports) s.g[t] = ep_prefix_at(s_w, s_m, NW, s.o[t]);  // G at every boundary (o_p <= 1024: all NW waves)
    const uint32_t g_i = ep_prefix_at(s_w, s_m, NW, t);
    __syncthreads();
    if (t < n_ports) eg_store_counts(counts + t, ep_counts(s.o[t], s.o[t + 1u], s.g[t], s.g[t + 1u], s.room[t]));
    ep_finish(d, reply, t, g_i, &s, n_ports, tx, free_list, stats, port_stats, &acc, nullptr, 0u);
}

}  // namespace
}  // namespace xskgpu

#endif  // XSK_EGRESS_PORTS_DEVICE_H
