// xsk_ring_ports.hip — the steered RX step over rings in device memory, one TX ring per port:
// xsk_gpu_rx_prepare_ports_dev() (every port's ring room from that port's ring; the descriptors behind the received
// count padded so that the host-sized steering call is exact), xsk_gpu_rx_ports_end_dev() (port p's span of d_tx onto
// port p's TX ring; every port's free list and then the frames the filter did not redirect onto the pool, as one
// ordered list; the RX entries released) and xsk_gpu_rx_step_steer_dev() (xsk_gpu_rx_begin_dev(), prepare,
// xsk_gpu_ingress_steer_dev(), xsk_gpu_egress_ports_dev(), end on one stream).  include/xsk_gpu.h; DESIGN.md §9.8.
// Every index and count is a word in device memory, read when the kernels execute; the up to 64 ring structs travel by
// value in the kernel arguments (2 KiB).
//
// Two paths, the arithmetic of both in xsk_ring_ports.h (host and device):
//   bound <= 1024: prepare and end are one launch of one 1024-thread workgroup each -- end: the offsets, every port's
//                  t_p, f_p and F_p and the pool's count meet in LDS, the rest list is compacted into LDS by wave
//                  ballots (xsk_compact.h), a lane per entry copies, a fence and a barrier, lane p stores port p's
//                  producer word and lane 0 the pool's count, the RX consumer word and *d_res;
//   larger:        kernel boundaries in place of the barriers -- prepare: one grid; end: the count / scan / scatter of
//                  the compaction core leave the rest list in the workspace, the copy grid (256 lanes per workgroup,
//                  every workgroup decides from the same words), a one-wave publish launch.
// No launch stores an index word for entries another launch stores, no atomic hands out a slot, no workgroup waits on
// another, nothing is polled.  The words a launch stores are read through the vector path (relaxed agent-scope atomic
// loads), never as read-only memory.  Latency bound: 16 B or 8 B in and out per entry, no frame byte touched, no MFMA.
#include <errno.h>

#include "../../include/xsk_gpu.h"
#include "xsk_hip_util.h"
#include "xsk_ring_ports.h"
#include "xsk_ring_ports_device.h"

using namespace xskgpu;

static_assert(kRpSmallMax == XSK_GPU_LOWLAT_MAX && kRpSmallMax == kEgSmallMax, "the one-launch path serves the RX loop's sizes");
static_assert(kEpMaxPorts == XSK_GPU_STEER_MAX_PORTS && kEpMaxPorts == kRdWave, "the publish launch: a lane per port");
static_assert(sizeof(xsk_gpu_rx_steer_result) == 32 && sizeof(xsk_gpu_rx_plan) == 32, "result and plan layout");
static_assert(sizeof(xsk_gpu_egress_counts) == sizeof(EgCounts) && sizeof(xsk_gpu_desc) == 16, "counts and descriptors");

namespace {

__device__ __forceinline__ uint32_t ring_free(const Ring& r) { return rd_free(load_word(r.prod), load_word(r.cons), r.size); }

// ---- prepare ----
__device__ __forceinline__ void prepare_rooms(const Rings& tx, uint32_t n_ports, uint32_t* d_tx_room, uint32_t lane) {
    if (lane < n_ports) d_tx_room[lane] = ring_free(tx.r[lane]);
}
__device__ __forceinline__ void prepare_pad(const xsk_gpu_rx_plan* d_plan, xsk_gpu_desc* descs, uint32_t n_max,
                                            uint64_t first, uint64_t stride) {
    const uint32_t r = rp_received(d_plan->received, n_max);
    for (uint64_t i = first; i < n_max; i += stride)
        if (rp_pad((uint32_t)i, r, n_max)) reinterpret_cast<uint4*>(descs)[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(kRpSmallThreads) void rx_prepare_ports_small_kernel(Rings tx, uint32_t n_ports,
                                                                                 const xsk_gpu_rx_plan* d_plan,
                                                                                 xsk_gpu_desc* descs, uint32_t n_max,
                                                                                 uint32_t* d_tx_room) {
    prepare_rooms(tx, n_ports, d_tx_room, threadIdx.x);
    prepare_pad(d_plan, descs, n_max, threadIdx.x, kRpSmallThreads);
}

__global__ __launch_bounds__(kRdCopy) void rx_prepare_ports_kernel(Rings tx, uint32_t n_ports,
                                                                   const xsk_gpu_rx_plan* d_plan, xsk_gpu_desc* descs,
                                                                   uint32_t n_max, uint32_t* d_tx_room) {
    if (blockIdx.x == 0) prepare_rooms(tx, n_ports, d_tx_room, threadIdx.x);
    prepare_pad(d_plan, descs, n_max, rd_copy_first(blockIdx.x, threadIdx.x), rd_copy_stride(gridDim.x));
}

// ---- end (EndLds, end_decide, end_copy, end_publish: xsk_ring_ports_device.h) ----
__global__ __launch_bounds__(kRpSmallThreads) void rx_end_ports_small_kernel(
    Ring rx, Rings tx, uint32_t n_ports, Pool pool, const xsk_gpu_rx_plan* d_plan, const xsk_gpu_desc* descs,
    const uint8_t* actions, const uint32_t* d_off, const xsk_gpu_desc* d_tx, const uint64_t* d_free,
    const xsk_gpu_egress_counts* counts, uint32_t n_max, xsk_gpu_rx_steer_result* d_res) {
    __shared__ EndLds s;
    __shared__ uint32_t s_w[kRpSmallWaves];
    __shared__ uint64_t s_rest[kRpSmallMax];
    const uint32_t i = threadIdx.x;
    end_decide(tx, n_ports, pool, d_plan, d_off, counts, n_max, &s);
    // the rest list, compacted in batch order: a lane per frame
    const bool hit = i < s.r && rp_rest(i, s.r, actions[i]);  // (r <= n_max: no action behind the bound is read)
    const unsigned long long m = cp_wg_ballot(hit, s_w);
    if (hit) s_rest[cp_waves_below<kRpSmallWaves>(s_w, cp_wave(), 0u) + cp_below(m, cp_lane())] = desc_addr(descs, i);
    const uint32_t n_rest = cp_waves_below<kRpSmallWaves>(s_w, kRpSmallWaves, 0u);
    __syncthreads();
    end_copy(tx, n_ports, pool, &s, n_rest, d_tx, d_free, s_rest, i, kRpSmallThreads);
    __threadfence();  // the entries before the words that cover them
    __syncthreads();
    end_publish(rx, tx, n_ports, pool, &s, n_rest, d_plan, d_res);
}

// ---- larger bounds: the rest list by count / scan / scatter into the workspace ----
__global__ __launch_bounds__(kCpFrames) void rx_end_ports_count_kernel(const xsk_gpu_rx_plan* d_plan,
                                                                       const uint8_t* __restrict__ actions,
                                                                       uint32_t n_max, uint32_t* __restrict__ cells) {
    __shared__ uint32_t s_w[kCpWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kCpFrames + threadIdx.x;
    const uint32_t r = rp_received(d_plan->received, n_max);
    cp_wg_count(i < r && rp_rest((uint32_t)i, r, actions[i]), s_w, cells);
}

__global__ __launch_bounds__(kCpScanThreads) void rx_end_ports_scan_kernel(uint32_t* cells, uint32_t nwg) {
    __shared__ uint32_t sc[kCpScanThreads];
    uint32_t b, e;
    cp_scan_run(nwg, threadIdx.x, &b, &e);
    const uint32_t total = cp_scan_cells(cells, b, e, sc, cp_put_before);
    if (threadIdx.x == 0) cells[nwg] = total;  // the word behind the cells: |rest|
}

__global__ __launch_bounds__(kCpFrames) void rx_end_ports_scatter_kernel(const xsk_gpu_rx_plan* d_plan,
                                                                         const xsk_gpu_desc* __restrict__ descs,
                                                                         const uint8_t* __restrict__ actions,
                                                                         uint32_t n_max,
                                                                         const uint32_t* __restrict__ cells,
                                                                         uint64_t* __restrict__ rest) {
    __shared__ uint32_t s_w[kCpWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kCpFrames + threadIdx.x;
    const uint32_t r = rp_received(d_plan->received, n_max);
    const bool hit = i < r && rp_rest((uint32_t)i, r, actions[i]);
    const unsigned long long m = cp_wg_ballot(hit, s_w);
    if (hit)
        rest[cp_waves_below<kCpWaves>(s_w, cp_wave(), cells[blockIdx.x]) + cp_below(m, cp_lane())] =
            desc_addr(descs, (uint32_t)i);
}

__global__ __launch_bounds__(kRdCopy) void rx_end_ports_copy_kernel(Rings tx, uint32_t n_ports, Pool pool,
                                                                    const xsk_gpu_rx_plan* d_plan,
                                                                    const uint32_t* d_off, const xsk_gpu_desc* d_tx,
                                                                    const uint64_t* d_free,
                                                                    const xsk_gpu_egress_counts* counts, uint32_t n_max,
                                                                    const uint64_t* rest, const uint32_t* d_n_rest) {
    __shared__ EndLds s;
    end_decide(tx, n_ports, pool, d_plan, d_off, counts, n_max, &s);
    end_copy(tx, n_ports, pool, &s, rd_min(*d_n_rest, n_max), d_tx, d_free, rest, rd_copy_first(blockIdx.x, threadIdx.x),
             rd_copy_stride(gridDim.x));
}

__global__ __launch_bounds__(kRdWave) void rx_end_ports_publish_kernel(Ring rx, Rings tx, uint32_t n_ports, Pool pool,
                                                                       const xsk_gpu_rx_plan* d_plan,
                                                                       const uint32_t* d_off,
                                                                       const xsk_gpu_egress_counts* counts,
                                                                       uint32_t n_max, const uint32_t* d_n_rest,
                                                                       xsk_gpu_rx_steer_result* d_res) {
    __shared__ EndLds s;
    end_decide(tx, n_ports, pool, d_plan, d_off, counts, n_max, &s);
    end_publish(rx, tx, n_ports, pool, &s, rd_min(*d_n_rest, n_max), d_plan, d_res);
}

// ---- the argument rules (a ring, a pool, a bound, the ports, end: xsk_ring_ports_device.h) ----
bool prepare_ok(const xsk_gpu_ring_dev* tx, uint32_t n_ports, const void* d_plan, const void* d_descs, uint32_t n_max,
                const void* d_tx_room) {
    return ports_ok(tx, n_ports) && bound_ok(n_max) && d_plan && !((uintptr_t)d_plan & 3u) && d_descs &&
           !((uintptr_t)d_descs & 15u) && d_tx_room && !((uintptr_t)d_tx_room & 3u);
}
// The launches, behind the checks.
int prepare_launch(const xsk_gpu_ring_dev* tx, uint32_t n_ports, const xsk_gpu_rx_plan* d_plan, xsk_gpu_desc* d_descs,
                   uint32_t n_max, uint32_t* d_tx_room, hipStream_t s) {
    const Rings t = rings_of(tx, n_ports);
    if (n_max <= kRpSmallMax)
        rx_prepare_ports_small_kernel<<<dim3(1), dim3(kRpSmallThreads), 0, s>>>(t, n_ports, d_plan, d_descs, n_max,
                                                                                d_tx_room);
    else
        rx_prepare_ports_kernel<<<dim3(rd_nwg(n_max)), dim3(kRdCopy), 0, s>>>(t, n_ports, d_plan, d_descs, n_max,
                                                                              d_tx_room);
    HIP_TRY(hipGetLastError());
    return 0;
}

int end_launch(const xsk_gpu_ring_dev* rx, const xsk_gpu_ring_dev* tx, uint32_t n_ports, const xsk_gpu_pool_dev* pool,
               const xsk_gpu_rx_plan* d_plan, const xsk_gpu_desc* d_descs, const uint8_t* d_actions,
               const uint32_t* d_off, const xsk_gpu_desc* d_tx, const uint64_t* d_free,
               const xsk_gpu_egress_counts* d_counts, uint32_t n_max, xsk_gpu_rx_steer_result* d_res, void* d_workspace,
               hipStream_t s) {
    const Ring r = ring_of(rx);
    const Rings t = rings_of(tx, n_ports);
    const Pool p = pool_of(pool);
    if (n_max <= kRpSmallMax) {
        rx_end_ports_small_kernel<<<dim3(1), dim3(kRpSmallThreads), 0, s>>>(r, t, n_ports, p, d_plan, d_descs, d_actions,
                                                                            d_off, d_tx, d_free, d_counts, n_max, d_res);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    uint8_t* const ws = (uint8_t*)d_workspace;
    uint64_t* const rest = (uint64_t*)(ws + rp_end_rest(n_max));
    uint32_t* const cells = (uint32_t*)(ws + rp_end_cells(n_max));
    const uint32_t* const d_n_rest = (const uint32_t*)(ws + rp_end_total(n_max));
    const uint32_t nwg = cp_nwg(n_max);
    rx_end_ports_count_kernel<<<dim3(nwg), dim3(kCpFrames), 0, s>>>(d_plan, d_actions, n_max, cells);
    HIP_TRY(hipGetLastError());
    rx_end_ports_scan_kernel<<<dim3(1), dim3(kCpScanThreads), 0, s>>>(cells, nwg);
    HIP_TRY(hipGetLastError());
    rx_end_ports_scatter_kernel<<<dim3(nwg), dim3(kCpFrames), 0, s>>>(d_plan, d_descs, d_actions, n_max, cells, rest);
    HIP_TRY(hipGetLastError());
    rx_end_ports_copy_kernel<<<dim3(rd_nwg(n_max)), dim3(kRdCopy), 0, s>>>(t, n_ports, p, d_plan, d_off, d_tx, d_free,
                                                                           d_counts, n_max, rest, d_n_rest);
    HIP_TRY(hipGetLastError());
    rx_end_ports_publish_kernel<<<dim3(1), dim3(kRdWave), 0, s>>>(r, t, n_ports, p, d_plan, d_off, d_counts, n_max,
                                                                  d_n_rest, d_res);
    HIP_TRY(hipGetLastError());
    return 0;
}

RpLayout layout_of(uint32_t max_batch, uint32_t n_ports) {
    return rp_layout(max_batch, n_ports, xsk_gpu_steer_workspace_size(max_batch, n_ports),
                     xsk_gpu_egress_ports_workspace_size(max_batch, n_ports));
}

}  // namespace

extern "C" {

size_t xsk_gpu_rx_step_steer_dev_workspace_size(uint32_t max_batch, uint32_t n_ports) {
    if (n_ports > kEpMaxPorts) n_ports = kEpMaxPorts;
    return layout_of(max_batch, n_ports).bytes;
}

int xsk_gpu_rx_prepare_ports_dev(const struct xsk_gpu_ring_dev* tx, uint32_t n_ports,
                                 const struct xsk_gpu_rx_plan* d_plan, struct xsk_gpu_desc* d_descs, uint32_t n_max,
                                 uint32_t* d_tx_room, void* stream) {
    if (!prepare_ok(tx, n_ports, d_plan, d_descs, n_max, d_tx_room)) return -EINVAL;
    return prepare_launch(tx, n_ports, d_plan, d_descs, n_max, d_tx_room, (hipStream_t)stream);
}

int xsk_gpu_rx_ports_end_dev(const struct xsk_gpu_ring_dev* rx, const struct xsk_gpu_ring_dev* tx, uint32_t n_ports,
                             const struct xsk_gpu_pool_dev* pool, const struct xsk_gpu_rx_plan* d_plan,
                             const struct xsk_gpu_desc* d_descs, const uint8_t* d_actions, const uint32_t* d_off,
                             const struct xsk_gpu_desc* d_tx, const uint64_t* d_free,
                             const struct xsk_gpu_egress_counts* d_counts, uint32_t n_max,
                             struct xsk_gpu_rx_steer_result* d_res, void* d_workspace, void* stream) {
    if (!end_ok(rx, tx, n_ports, pool, d_plan, d_descs, d_actions, d_off, d_tx, d_free, d_counts, n_max, d_res,
                d_workspace))
        return -EINVAL;
    return end_launch(rx, tx, n_ports, pool, d_plan, d_descs, d_actions, d_off, d_tx, d_free, d_counts, n_max, d_res,
                      d_workspace, (hipStream_t)stream);
}

int xsk_gpu_rx_step_steer_dev(void* d_umem, uint64_t umem_size, const struct xsk_gpu_ring_dev* rx,
                              const struct xsk_gpu_ring_dev* fill, const struct xsk_gpu_ring_dev* tx,
                              const struct xsk_gpu_pool_dev* pool, uint32_t max_batch, uint32_t opts,
                              const struct xsk_gpu_steer_entry* d_table, uint32_t n_entries, uint32_t default_port,
                              uint32_t n_ports, const uint64_t* d_bound, uint8_t* d_actions, uint8_t* d_ports,
                              struct xsk_gpu_egress_counts* d_port_counts, struct xsk_gpu_stats* d_stats,
                              struct xsk_gpu_stats* d_port_stats, struct xsk_gpu_rx_steer_result* d_res,
                              void* d_workspace, void* stream) {
    // the workspace's arrays satisfy the rules of the five composed calls by layout; what is left of those rules is the
    // caller's: the rings and the pool, the UMEM, the option bits, the table and the port rule, the counters
    if (!d_workspace || ((uintptr_t)d_workspace & 15u) || !d_umem || ((uintptr_t)d_umem & 15u) || (umem_size & 15u) ||
        (umem_size >> 48) || (opts & ~XSK_GPU_OPT_MASK) || ((uintptr_t)d_stats & 7u) || ((uintptr_t)d_port_stats & 7u) ||
        ((uintptr_t)d_res & 3u) || ((uintptr_t)d_port_counts & 3u) || !bound_ok(max_batch) || !ports_ok(tx, n_ports) ||
        !ring_ok(rx, 16u) || !ring_ok(fill, 8u) || !pool_ok(pool) ||
        (default_port >= n_ports && default_port != XSK_GPU_STEER_PASS) || n_entries > XSK_GPU_STEER_MAX_ENTRIES ||
        (n_entries && (!d_table || ((uintptr_t)d_table & 7u))) || ((uintptr_t)d_bound & 7u))
        return -EINVAL;
    uint8_t* const ws = (uint8_t*)d_workspace;
    const RpLayout l = layout_of(max_batch, n_ports);
    xsk_gpu_rx_plan* const plan = (xsk_gpu_rx_plan*)(ws + l.plan);
    uint32_t* const room = (uint32_t*)(ws + l.room);
    uint32_t* const off = (uint32_t*)(ws + l.off);
    xsk_gpu_egress_counts* const counts = d_port_counts ? d_port_counts : (xsk_gpu_egress_counts*)(ws + l.counts);
    xsk_gpu_desc* const descs = (xsk_gpu_desc*)(ws + l.descs);
    xsk_gpu_desc* const out = (xsk_gpu_desc*)(ws + l.out);
    xsk_gpu_desc* const d_tx = (xsk_gpu_desc*)(ws + l.tx);
    uint64_t* const d_free = (uint64_t*)(ws + l.free_list);
    uint8_t* const verdicts = ws + l.verdicts;
    uint8_t* const actions = d_actions ? d_actions : ws + l.actions;
    uint8_t* const ports = d_ports ? d_ports : ws + l.ports;
    int rc = xsk_gpu_rx_begin_dev(rx, fill, &tx[0], pool, max_batch, descs, plan, stream);
    if (rc) return rc;
    rc = prepare_launch(tx, n_ports, plan, descs, max_batch, room, (hipStream_t)stream);
    if (rc) return rc;
    rc = xsk_gpu_ingress_steer_dev(d_umem, umem_size, descs, max_batch, opts, d_table, n_entries, default_port, n_ports,
                                   d_bound, actions, ports, out, off, verdicts, NULL, d_stats, ws + l.steer, stream);
    if (rc) return rc;
    rc = xsk_gpu_egress_ports_dev(out, verdicts, off, n_ports, max_batch, room, d_tx, d_free, counts, d_stats,
                                  d_port_stats, ws + l.egress, stream);
    if (rc) return rc;
    return end_launch(rx, tx, n_ports, pool, plan, descs, actions, off, d_tx, d_free, counts, max_batch, d_res,
                      ws + l.end, (hipStream_t)stream);
}

}  // extern "C"
