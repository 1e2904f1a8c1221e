// xsk_egress_ports.hip — xsk_gpu_egress_ports_dev(): xsk_gpu_egress_dev()'s rule once per steered port.  Behind
// xsk_gpu_ingress_steer_dev() the redirected descriptors lie grouped by port, port p's at [d_off[p], d_off[p + 1]) with
// the offsets in device memory; every port gets what the reference keeps per socket (struct xsk_socket_info,
// src/lib/xsk_utils.h): its own TX list cut at its own ring's room, its own free-frame list, its own stats_record.  Both
// lists of port p lie inside the port's own span of d_tx / d_free, in batch order (include/xsk_gpu.h).
//
// Two paths, the arithmetic of both in xsk_egress_ports.h (host and device):
//   n_max <= 1024: one launch of one 1024-thread workgroup -- lane per frame, wave ballots, sixteen counts and masks in
//                  LDS, the prefix at every port boundary from them;
//   larger:        the three launches of the compaction core (xsk_compact.h) -- per-workgroup reply counts, one scan
//                  (which also takes the prefix at each of the n_ports + 1 boundaries, a wave per boundary, and writes
//                  d_counts), the in-order scatter -- and, only with d_port_stats, a fourth that adds up the scatter's
//                  per-workgroup sums, a workgroup per port.
// Every kernel stages the offsets (a wave's max-scan of the words, then the clamp) and the rooms into LDS in a prologue.
// A frame's slot is R_p(i) = G(i) - G(o_p) below its port's start: no atomic hands out a slot, no workgroup waits on
// another.  HBM / latency bound: 17 B in and at most 16 B out per frame, no frame byte touched, no MFMA.
#include <errno.h>

#include "../../include/xsk_gpu.h"
#include "xsk_egress_ports.h"
#include "xsk_egress_ports_device.h"
#include "xsk_hip_util.h"

using namespace xskgpu;

static_assert(kEgSmallMax == XSK_GPU_LOWLAT_MAX, "the one-launch path serves the RX loop's sizes");
static_assert(kEpMaxPorts == XSK_GPU_STEER_MAX_PORTS, "one offset per steered port and one behind");
static_assert(kEpMaxPorts == kEgWave, "the prologue scans the offsets in one wave; wave 0 issues the counter atomics");
static_assert(sizeof(xsk_gpu_egress_counts) == sizeof(EgCounts) && sizeof(EgCounts) == 16, "counts layout");
static_assert(sizeof(xsk_gpu_desc) == 16, "one 16-B load and store per descriptor");

namespace {

// (EpLds, EpAcc, ep_stage, acc_zero, ep_finish: xsk_egress_ports_device.h)

// ---- n_max <= 1024: everything in one workgroup.  (The fused loop kernel runs the same statements as
// egress_ports_small_body(), xsk_egress_ports_device.h; called from here, with the LDS objects handed in, the compiler
// emitted 939 instructions for this kernel's 937, so the kernel keeps its own text: profiles/rx_loop_fused/README.md) ----
__global__ __launch_bounds__(kEgSmallThreads) void egress_ports_small_kernel(
    const xsk_gpu_desc* __restrict__ descs, const uint8_t* __restrict__ verdicts, const uint32_t* __restrict__ d_off,
    uint32_t n_ports, uint32_t n_max, const uint32_t* __restrict__ d_room, xsk_gpu_desc* __restrict__ tx,
    uint64_t* __restrict__ free_list, xsk_gpu_egress_counts* __restrict__ counts, xsk_gpu_stats* stats,
    xsk_gpu_stats* port_stats) {
    constexpr uint32_t NW = kEgSmallThreads / kEgWave;
    __shared__ EpLds s;
    __shared__ EpAcc acc;
    __shared__ uint32_t s_w[NW];
    __shared__ uint64_t s_m[NW];
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

// ---- larger bounds, stage 1: per-workgroup reply counts over [o_0, o_{n_ports}) (a workgroup outside writes 0) ----
__global__ __launch_bounds__(kEgFrames) void egress_ports_count_kernel(const uint8_t* __restrict__ verdicts,
                                                                       const uint32_t* __restrict__ d_off,
                                                                       uint32_t n_ports, uint32_t n_max,
                                                                       uint32_t* __restrict__ wg_count) {
    constexpr uint32_t NW = kEgFrames / kEgWave;
    __shared__ EpLds s;
    __shared__ uint32_t s_w[NW];
    ep_stage<false>(d_off, n_ports, n_max, nullptr, &s);
    __syncthreads();
    const uint32_t i = blockIdx.x * kEgFrames + threadIdx.x;
    const bool reply = ep_in(i, s.o[0], s.o[n_ports]) && verdicts[i] == XSK_GPU_TX_REPLY;
    cp_wg_count(reply, s_w, wg_count);
}

// ---- stage 2: exclusive scan of the nwg counts in place (one workgroup of 1024; thread t owns a contiguous run:
// cp_scan_cells), then the prefix at each boundary -- a wave per boundary in turn: the scanned count of the
// boundary's workgroup plus the replies among the at most 255 verdicts in front of it -- into ws[nwg + p], and
// d_counts[p] from their differences ----
__global__ __launch_bounds__(kEgScanThreads) void egress_ports_scan_kernel(
    uint32_t* ws, uint32_t nwg, const uint8_t* __restrict__ verdicts, const uint32_t* __restrict__ d_off,
    uint32_t n_ports, uint32_t n_max, const uint32_t* __restrict__ d_room,
    xsk_gpu_egress_counts* __restrict__ counts) {
    __shared__ uint32_t sc[kEgScanThreads];
    __shared__ EpLds s;
    const uint32_t t = threadIdx.x;
    ep_stage<true>(d_off, n_ports, n_max, d_room, &s);
    uint32_t b, e;
    cp_scan_run(nwg, t, &b, &e);
    cp_scan_cells(ws, b, e, sc, cp_put_before);  // (its total is read behind the barrier, with the staged offsets)
    __syncthreads();  // the offsets just written are read below by other waves of this workgroup
    const uint32_t total = sc[kEgScanThreads - 1u], lo = s.o[0], lane = cp_lane();
    for (uint32_t k = cp_wave(); k <= n_ports; k += kEgScanThreads / kEgWave) {  // wave-uniform
        const uint32_t o = s.o[k], wg = ep_bound_wg(o);
        uint32_t g = total;
        if (wg < nwg) {
            const uint32_t from = ep_bound_from(o, lo);
            uint32_t c = 0;
#pragma unroll
            for (uint32_t q = 0; q < kEgFrames / kEgWave; ++q) {
                const uint32_t i = wg * kEgFrames + q * kEgWave + lane;
                const bool r = i >= from && i < o && verdicts[i] == XSK_GPU_TX_REPLY;
                c += (uint32_t)__popcll(__ballot(r));
            }
            g = ws[wg] + c;
        }
        if (lane == 0) s.g[k] = g;
    }
    __syncthreads();
    if (t <= n_ports) ws[nwg + t] = s.g[t];
    if (t < n_ports) eg_store_counts(counts + t, ep_counts(s.o[t], s.o[t + 1u], s.g[t], s.g[t + 1u], s.room[t]));
}

// ---- stage 3: the in-order scatter of every port's two lists ----
__global__ __launch_bounds__(kEgFrames) void egress_ports_scatter_kernel(
    const xsk_gpu_desc* __restrict__ descs, const uint8_t* __restrict__ verdicts, const uint32_t* __restrict__ d_off,
    uint32_t n_ports, uint32_t n_max, const uint32_t* __restrict__ d_room, const uint32_t* __restrict__ ws, uint32_t nwg,
    EpPart* __restrict__ part, xsk_gpu_desc* __restrict__ tx, uint64_t* __restrict__ free_list, xsk_gpu_stats* stats,
    xsk_gpu_stats* port_stats) {
    constexpr uint32_t NW = kEgFrames / kEgWave;
    __shared__ EpLds s;
    __shared__ EpAcc acc;
    __shared__ uint32_t s_w[NW];
    const uint32_t t = threadIdx.x;
    ep_stage<true>(d_off, n_ports, n_max, d_room, &s);
    if (t <= n_ports) s.g[t] = ws[nwg + t];
    acc_zero(&acc);
    __syncthreads();
    if (!ep_wg_live(blockIdx.x, s.o[0], s.o[n_ports])) return;  // workgroup-uniform
    const uint32_t i = blockIdx.x * kEgFrames + t;
    uint4 d;
    const bool reply = eg_load_frame(descs, verdicts, i, s.o[0], s.o[n_ports], &d);
    const u64 m = cp_wg_ballot(reply, s_w);
    uint32_t g_i = ws[blockIdx.x] + cp_below(m, cp_lane());
    for (uint32_t k = 0; k < NW; ++k) g_i += k < cp_wave() ? s_w[k] : 0u;  // (cp_waves_below here builds other code)
    ep_finish(d, reply, i, g_i, &s, n_ports, tx, free_list, stats, port_stats, &acc, part, blockIdx.x);
}

// ---- stage 4, only with d_port_stats: a workgroup per port adds up the records of the scatter workgroups whose first
// position the port owns and issues the port's one set of atomics ----
__global__ __launch_bounds__(kEgFrames) void egress_ports_sum_kernel(const uint32_t* __restrict__ d_off, uint32_t n_ports,
                                                                     uint32_t n_max, const EpPart* __restrict__ part,
                                                                     xsk_gpu_stats* port_stats) {
    constexpr uint32_t NW = kEgFrames / kEgWave;
    __shared__ EpLds s;
    __shared__ u64 s_r[NW][4];
    ep_stage<false>(d_off, n_ports, n_max, nullptr, &s);
    __syncthreads();
    const uint32_t p = blockIdx.x, b = ep_carry_begin(s.o[p]), e = ep_carry_begin(s.o[p + 1u]);
    if (b >= e) return;  // workgroup-uniform: no record is this port's
    u64 n = 0, n_tx = 0, bytes = 0, tx_bytes = 0;
    for (uint32_t wg = b + threadIdx.x; wg < e; wg += kEgFrames) {
        const EpPart* r = part + wg;
        n += r->n;
        n_tx += r->n_tx;
        bytes += ep_u64(r->bytes_lo, r->bytes_hi);
        tx_bytes += ep_u64(r->tx_bytes_lo, r->tx_bytes_hi);
    }
    n = cp_wave_sum(n);
    n_tx = cp_wave_sum(n_tx);
    bytes = cp_wave_sum(bytes);
    tx_bytes = cp_wave_sum(tx_bytes);
    if (cp_lane() == 0) {
        s_r[cp_wave()][0] = n;
        s_r[cp_wave()][1] = n_tx;
        s_r[cp_wave()][2] = bytes;
        s_r[cp_wave()][3] = tx_bytes;
    }
    __syncthreads();
    if (threadIdx.x < 4u) {
        u64 v = 0;
        for (uint32_t w = 0; w < NW; ++w) v += s_r[w][threadIdx.x];
        xsk_gpu_stats* ps = port_stats + p;
        u64* cell = threadIdx.x == 0 ? (u64*)&ps->rx_packets : threadIdx.x == 1 ? (u64*)&ps->tx_packets
                  : threadIdx.x == 2 ? (u64*)&ps->rx_bytes : (u64*)&ps->tx_bytes;
        if (v) atomicAdd(cell, v);
    }
}

}  // namespace

extern "C" {

size_t xsk_gpu_egress_ports_workspace_size(uint32_t n_max, uint32_t n_ports) {
    return ep_workspace_bytes(n_max, n_ports);
}

int xsk_gpu_egress_ports_dev(const struct xsk_gpu_desc* d_descs, const uint8_t* d_verdicts, const uint32_t* d_off,
                             uint32_t n_ports, uint32_t n_max, const uint32_t* d_tx_room, struct xsk_gpu_desc* d_tx,
                             uint64_t* d_free, struct xsk_gpu_egress_counts* d_counts, struct xsk_gpu_stats* d_stats,
                             struct xsk_gpu_stats* d_port_stats, void* d_workspace, void* stream) {
    if (!d_descs || !d_tx || !d_free || !d_counts || !d_verdicts || !d_off || ((uintptr_t)d_descs & 15u) ||
        ((uintptr_t)d_tx & 15u) || ((uintptr_t)d_free & 7u) || ((uintptr_t)d_counts & 3u) || ((uintptr_t)d_off & 3u) ||
        ((uintptr_t)d_tx_room & 3u) || ((uintptr_t)d_stats & 7u) || ((uintptr_t)d_port_stats & 7u) || n_ports < 1u ||
        n_ports > kEpMaxPorts || n_max > XSK_GPU_MAX_BATCH || (const void*)d_tx == (const void*)d_descs ||
        (!d_workspace && n_max > kEgSmallMax))
        return -EINVAL;
    const hipStream_t s = (hipStream_t)stream;
    if (n_max == 0) {
        HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)n_ports * sizeof(*d_counts), s));
        return 0;
    }
    if (n_max <= kEgSmallMax) {
        egress_ports_small_kernel<<<dim3(1), dim3(kEgSmallThreads), 0, s>>>(
            d_descs, d_verdicts, d_off, n_ports, n_max, d_tx_room, d_tx, d_free, d_counts, d_stats, d_port_stats);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const uint32_t nwg = cp_nwg(n_max);
    uint32_t* ws = (uint32_t*)d_workspace;
    EpPart* part = (EpPart*)((char*)d_workspace + ep_part_offset(n_max, n_ports));
    egress_ports_count_kernel<<<dim3(nwg), dim3(kEgFrames), 0, s>>>(d_verdicts, d_off, n_ports, n_max, ws);
    HIP_TRY(hipGetLastError());
    egress_ports_scan_kernel<<<dim3(1), dim3(kEgScanThreads), 0, s>>>(ws, nwg, d_verdicts, d_off, n_ports, n_max,
                                                                      d_tx_room, d_counts);
    HIP_TRY(hipGetLastError());
    egress_ports_scatter_kernel<<<dim3(nwg), dim3(kEgFrames), 0, s>>>(d_descs, d_verdicts, d_off, n_ports, n_max,
                                                                      d_tx_room, (const uint32_t*)ws, nwg, part, d_tx,
                                                                      d_free, d_stats, d_port_stats);
    HIP_TRY(hipGetLastError());
    if (d_port_stats) {
        egress_ports_sum_kernel<<<dim3(n_ports), dim3(kEgFrames), 0, s>>>(d_off, n_ports, n_max, part, d_port_stats);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
