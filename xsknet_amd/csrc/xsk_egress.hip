// xsk_egress.hip — xsk_gpu_egress_dev(): the step the reference's RX loop takes behind process_packet()
// (handle_receive_packets(), src/lib/xsk_receive.c:174-186, 226-227) as a device pass over a batch: every TX_REPLY
// frame onto the TX descriptor list, as many as the TX ring has room for, every other frame's address onto the free
// list, both in batch order, their counts, and the tx counters taken back for replies that found the ring full.  The
// host modes do this in xsk_gpu__rx_emit() (xsk_gpu_rx.c), a sequential loop; the result here is that loop's, exactly
// (include/xsk_gpu.h).  The frame count and the ring's room are words in device memory, read when the
// kernels execute, so the call chains behind xsk_gpu_ingress_dev_opts() on one stream and in one captured graph.
//
// Two paths, the arithmetic of both in xsk_egress.h (host and device):
//   n_max <= 1024: one launch of one 1024-thread workgroup — lane per frame, wave ballots, sixteen counts in LDS;
//   larger:        the three launches of the compaction core (xsk_compact.h) — per-workgroup reply counts, one
//                  exclusive scan (which also writes the counts), the in-order scatter of both lists.
// Every kernel reads the count and the room in a prologue of scalar loads.  HBM / latency bound: 17 B in and at most
// 16 B out per frame, no frame byte touched, no MFMA.
#include <errno.h>

#include "../../include/xsk_gpu.h"
#include "xsk_egress.h"
#include "xsk_hip_util.h"

using namespace xskgpu;

static_assert(kEgSmallMax == XSK_GPU_LOWLAT_MAX, "the one-launch path serves the RX loop's sizes");
static_assert(sizeof(xsk_gpu_egress_counts) == sizeof(EgCounts) && sizeof(EgCounts) == 16, "counts layout");
static_assert(sizeof(xsk_gpu_desc) == 16, "one 16-B load and store per descriptor");

namespace {

typedef unsigned long long u64;

// The prologue: the two words as scalar loads (uniform addresses of read-only memory), then the clamp.
struct EgIn {
    uint32_t n, room;
};
__device__ __forceinline__ EgIn eg_prologue(const uint32_t* __restrict__ d_n, uint32_t n_max,
                                            const uint32_t* __restrict__ d_room) {
    EgIn in;
    in.n = eg_count(d_n != nullptr, d_n ? *d_n : 0u, n_max);
    in.room = eg_room(d_room != nullptr, d_room ? *d_room : 0u);
    return in;
}

// tx_packets / tx_bytes taken back for the workgroup's replies past the room: each wave reduces its own, wave 0 the
// NW partials, lane 0 issues the one pair of device-scope atomics -- none when the workgroup has no such reply.
template <uint32_t NW>
__device__ __forceinline__ void take_back(bool unsent, uint32_t len, uint32_t* s_c, u64* s_b, xsk_gpu_stats* stats) {
    const u64 um = __ballot(unsent);
    u64 b = 0;
    if (um) b = cp_wave_sum(unsent ? (u64)len : 0ull);  // wave-uniform
    if (cp_lane() == 0) {
        s_c[cp_wave()] = (uint32_t)__popcll(um);
        s_b[cp_wave()] = b;
    }
    __syncthreads();
    if (cp_wave() == 0) {
        uint32_t c = cp_lane() < NW ? s_c[cp_lane()] : 0u;
        u64 t = cp_lane() < NW ? s_b[cp_lane()] : 0ull;
        for (int o = 32; o > 0; o >>= 1) {
            c += __shfl_xor(c, o, 64);
            t += __shfl_xor(t, o, 64);
        }
        if (cp_lane() == 0 && c) {
            atomicAdd((u64*)&stats->tx_packets, 0ull - (u64)c);
            atomicAdd((u64*)&stats->tx_bytes, 0ull - t);
        }
    }
}

// What both scatters do, one lane per frame: frame i of a workgroup of NW waves with `off` replies below the workgroup.
// Wave ballots give the NW per-wave reply counts, which meet in LDS; every lane reads all of them (LDS broadcasts),
// sums those of the waves below it and adds the ballot bits below its lane: R(i).  Then the frame goes to its list, and
// a workgroup that holds a reply past the room takes it back out of the counters.  Returns the replies below the
// workgroup's end (workgroup-uniform).
template <uint32_t NW>
__device__ __forceinline__ uint32_t scatter_wg(const xsk_gpu_desc* __restrict__ descs,
                                               const uint8_t* __restrict__ verdicts, uint32_t i, const EgIn& in,
                                               uint32_t off, xsk_gpu_desc* __restrict__ tx,
                                               uint64_t* __restrict__ free_list, xsk_gpu_stats* stats) {
    __shared__ uint32_t s_w[NW];
    __shared__ uint32_t s_c[NW];
    __shared__ u64 s_b[NW];
    const uint32_t lane = cp_lane(), w = cp_wave();  // (ahead of the loads: the order the kernels were built from)
    uint4 d;
    const bool reply = eg_load_frame(descs, verdicts, i, 0u, in.n, &d);
    const u64 m = cp_wg_ballot(reply, s_w);
    uint32_t total = off;
    for (uint32_t k = 0; k < NW; ++k) total += s_w[k];
    const uint32_t r_below = cp_waves_below<NW>(s_w, w, off) + cp_below(m, lane);
    if (i < in.n) eg_store_frame(d, eg_slot(reply, i, r_below, in.room), tx, free_list);
    if (stats && total > off && total > in.room)  // workgroup-uniform: a reply of this workgroup lies past the room
        take_back<NW>(eg_unsent(reply, r_below, in.room), d.z, s_c, s_b, stats);
    return total;
}

// ---- n_max <= 1024: everything in one workgroup ----
__global__ __launch_bounds__(kEgSmallThreads) void egress_small_kernel(
    const xsk_gpu_desc* __restrict__ descs, const uint8_t* __restrict__ verdicts, const uint32_t* __restrict__ d_n,
    uint32_t n_max, const uint32_t* __restrict__ d_room, xsk_gpu_desc* __restrict__ tx, uint64_t* __restrict__ free_list,
    xsk_gpu_egress_counts* __restrict__ counts, xsk_gpu_stats* stats) {
    const EgIn in = eg_prologue(d_n, n_max, d_room);
    const uint32_t total = scatter_wg<kEgSmallThreads / kEgWave>(descs, verdicts, threadIdx.x, in, 0u, tx, free_list, stats);
    if (threadIdx.x == 0) eg_store_counts(counts, eg_counts(in.n, total, in.room));
}

// ---- larger batches, stage 1: per-workgroup reply counts (a workgroup past n writes 0) ----
__global__ __launch_bounds__(kEgFrames) void egress_count_kernel(const uint8_t* __restrict__ verdicts,
                                                                 const uint32_t* __restrict__ d_n, uint32_t n_max,
                                                                 uint32_t* __restrict__ wg_count) {
    constexpr uint32_t NW = kEgFrames / kEgWave;
    __shared__ uint32_t s_w[NW];
    const uint32_t n = eg_count(d_n != nullptr, d_n ? *d_n : 0u, n_max);
    const uint32_t t = threadIdx.x;
    const bool reply = t < eg_wg_frames(n, blockIdx.x) && verdicts[(size_t)blockIdx.x * kEgFrames + t] == XSK_GPU_TX_REPLY;
    cp_wg_count(reply, s_w, wg_count);
}

// ---- stage 2: exclusive scan of the nwg counts in place, and the batch's counts (one workgroup of 1024; thread t owns
// a contiguous run of the counts: cp_scan_cells) ----
__global__ __launch_bounds__(kEgScanThreads) void egress_scan_kernel(uint32_t* __restrict__ wg_count, uint32_t nwg,
                                                                     const uint32_t* __restrict__ d_n, uint32_t n_max,
                                                                     const uint32_t* __restrict__ d_room,
                                                                     xsk_gpu_egress_counts* __restrict__ counts) {
    __shared__ uint32_t s[kEgScanThreads];
    const EgIn in = eg_prologue(d_n, n_max, d_room);
    uint32_t b, e;
    cp_scan_run(nwg, threadIdx.x, &b, &e);
    const uint32_t total = cp_scan_cells(wg_count, b, e, s, cp_put_before);
    if (threadIdx.x == kEgScanThreads - 1u) eg_store_counts(counts, eg_counts(in.n, total, in.room));
}

// ---- stage 3: the in-order scatter of both lists ----
__global__ __launch_bounds__(kEgFrames) void egress_scatter_kernel(
    const xsk_gpu_desc* __restrict__ descs, const uint8_t* __restrict__ verdicts, const uint32_t* __restrict__ d_n,
    uint32_t n_max, const uint32_t* __restrict__ d_room, const uint32_t* __restrict__ wg_off,
    xsk_gpu_desc* __restrict__ tx, uint64_t* __restrict__ free_list, xsk_gpu_stats* stats) {
    const EgIn in = eg_prologue(d_n, n_max, d_room);
    if (eg_wg_frames(in.n, blockIdx.x) == 0u) return;  // workgroup-uniform, before the first barrier
    scatter_wg<kEgFrames / kEgWave>(descs, verdicts, blockIdx.x * kEgFrames + threadIdx.x, in, wg_off[blockIdx.x], tx,
                                    free_list, stats);
}

}  // namespace

extern "C" {

size_t xsk_gpu_egress_workspace_size(uint32_t n_max) { return eg_workspace_bytes(n_max); }

int xsk_gpu_egress_dev(const struct xsk_gpu_desc* d_descs, const uint8_t* d_verdicts, const uint32_t* d_n,
                       uint32_t n_max, const uint32_t* d_tx_room, struct xsk_gpu_desc* d_tx, uint64_t* d_free,
                       struct xsk_gpu_egress_counts* d_counts, struct xsk_gpu_stats* d_stats, void* d_workspace,
                       void* stream) {
    if (!d_descs || !d_tx || !d_free || !d_counts || !d_verdicts || ((uintptr_t)d_descs & 15u) ||
        ((uintptr_t)d_tx & 15u) || ((uintptr_t)d_free & 7u) || ((uintptr_t)d_counts & 3u) || ((uintptr_t)d_n & 3u) ||
        ((uintptr_t)d_tx_room & 3u) || ((uintptr_t)d_stats & 7u) || n_max > XSK_GPU_MAX_BATCH ||
        (const void*)d_tx == (const void*)d_descs || (!d_workspace && n_max > kEgSmallMax))
        return -EINVAL;
    const hipStream_t s = (hipStream_t)stream;
    if (n_max == 0) {
        HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(*d_counts), s));
        return 0;
    }
    if (n_max <= kEgSmallMax) {
        egress_small_kernel<<<dim3(1), dim3(kEgSmallThreads), 0, s>>>(d_descs, d_verdicts, d_n, n_max, d_tx_room, d_tx,
                                                                      d_free, d_counts, d_stats);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const uint32_t nwg = cp_nwg(n_max);
    uint32_t* wg = (uint32_t*)d_workspace;
    egress_count_kernel<<<dim3(nwg), dim3(kEgFrames), 0, s>>>(d_verdicts, d_n, n_max, wg);
    HIP_TRY(hipGetLastError());
    egress_scan_kernel<<<dim3(1), dim3(kEgScanThreads), 0, s>>>(wg, nwg, d_n, n_max, d_tx_room, d_counts);
    HIP_TRY(hipGetLastError());
    egress_scatter_kernel<<<dim3(nwg), dim3(kEgFrames), 0, s>>>(d_descs, d_verdicts, d_n, n_max, d_tx_room,
                                                                (const uint32_t*)wg, d_tx, d_free, d_stats);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
