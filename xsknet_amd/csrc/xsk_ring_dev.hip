// xsk_ring_dev.hip — the RX ring step over rings and a frame pool in device memory: xsk_gpu_rx_begin_dev() (peek the RX
// ring, refill the fill ring: steps 1 and 2 of xsk_gpu_rx_step(), xsk_gpu_rx.c), xsk_gpu_rx_end_dev() (replies onto the
// TX ring, freed frames onto the pool, release the RX entries: the ring half of step 4, and step 5),
// xsk_gpu_rx_step_dev() (begin, xsk_gpu_echo_dev_indirect(), xsk_gpu_egress_dev(), end on one stream) and
// xsk_gpu_tx_complete_dev() (xsk_gpu_tx_complete()).  After a call the rings and the pool hold what the host functions
// leave from the same state (include/xsk_gpu.h).  Every index and count is a word in device memory,
// read when the kernels execute, so the calls chain on one stream and replay in one captured graph.
//
// Two paths, the arithmetic of both in xsk_ring_dev.h (host and device):
//   bound <= 1024: one launch of one 1024-thread workgroup — lane 0 reads the words and decides, the decision meets the
//                  other lanes in LDS, a lane per entry copies, a fence and a barrier, lane 0 stores the new words;
//   larger:        kernel boundaries in place of the two barriers — begin: a one-wave plan launch (writes *d_plan), the
//                  copy grid (256 entries per workgroup; reads *d_plan and entries), a one-wave publish launch (stores
//                  the words); end and tx_complete: the copy grid, then the publish launch, both deciding from the same
//                  words, which nothing stores before the publish launch.
// No launch stores an index word for entries another launch stores, no workgroup waits on another, nothing is polled.
// The words a launch stores are read through the vector path (relaxed agent-scope atomic loads), never as read-only
// memory.  Latency bound: 16 B or 8 B in and out per entry, no frame byte touched, no MFMA.
#include <errno.h>

#include "../../include/xsk_gpu.h"
#include "xsk_hip_util.h"
#include "xsk_ring_dev.h"
#include "xsk_ring_dev_device.h"

using namespace xskgpu;

static_assert(kRdSmallMax == XSK_GPU_LOWLAT_MAX && kRdSmallMax == kEgSmallMax, "the one-launch path serves the RX loop's sizes");
static_assert(sizeof(xsk_gpu_ring_dev) == 32 && sizeof(xsk_gpu_pool_dev) == 24, "ring and pool layout");
static_assert(sizeof(xsk_gpu_rx_plan) == sizeof(RdPlan) && sizeof(RdPlan) == 32, "plan layout");
static_assert(sizeof(xsk_gpu_rx_result) == 16 && sizeof(xsk_gpu_egress_counts) == 16, "result and counts layout");
static_assert(sizeof(xsk_gpu_desc) == 16, "one 16-B load and store per descriptor");

namespace {

// (Ring, Pool, load_word and the begin stage -- begin_decide, begin_copy, begin_publish, rx_begin_small_body:
// xsk_ring_dev_device.h)

// ---- begin ----
__global__ __launch_bounds__(kRdSmallThreads) void rx_begin_small_kernel(Ring rx, Ring fill, Ring tx, Pool pool,
                                                                         uint32_t max_batch, xsk_gpu_desc* descs,
                                                                         xsk_gpu_rx_plan* d_plan) {
    __shared__ RdPlan s_plan;
    rx_begin_small_body(rx, fill, tx, pool, max_batch, descs, d_plan, &s_plan);
}

__global__ __launch_bounds__(kRdWave) void rx_begin_plan_kernel(Ring rx, Ring fill, Ring tx, Pool pool,
                                                                uint32_t max_batch, xsk_gpu_rx_plan* d_plan) {
    if (threadIdx.x == 0) store_plan(d_plan, begin_decide(rx, fill, tx, pool, max_batch));
}

__global__ __launch_bounds__(kRdCopy) void rx_begin_copy_kernel(Ring rx, Ring fill, Pool pool,
                                                                const xsk_gpu_rx_plan* __restrict__ d_plan,
                                                                xsk_gpu_desc* descs) {
    const RdPlan p = load_plan(d_plan);  // written by the launch before this one: uniform loads of read-only memory
    begin_copy(rx, fill, pool, p, descs, rd_copy_first(blockIdx.x, threadIdx.x), rd_copy_stride(gridDim.x));
}

__global__ __launch_bounds__(kRdWave) void rx_begin_publish_kernel(Ring fill, Pool pool,
                                                                   const xsk_gpu_rx_plan* __restrict__ d_plan) {
    if (threadIdx.x == 0) begin_publish(fill, pool, load_plan(d_plan));
}

// ---- end ----
__device__ __forceinline__ RdEnd end_decide(const Ring& tx, const Pool& pool, const xsk_gpu_rx_plan* d_plan,
                                            const xsk_gpu_egress_counts* counts, uint32_t n_max) {
    return rd_end_plan(counts->n_tx, counts->n_free, n_max, load_words(tx), tx.size, load_word(pool.n_free),
                       pool.capacity, d_plan->received);
}
__device__ __forceinline__ void end_copy(const Ring& tx, const Pool& pool, const RdEnd& e, const xsk_gpu_desc* d_tx,
                                         const uint64_t* d_free, uint64_t first, uint64_t stride) {
    for (uint64_t k = first; k < e.n_tx; k += stride)
        *desc_slot(tx, e.tx_prod + (uint32_t)k) = reinterpret_cast<const uint4*>(d_tx)[k];
    for (uint64_t j = first; j < e.pushed; j += stride)
        reinterpret_cast<uint2*>(pool.addr)[e.pool_n + (uint32_t)j] = reinterpret_cast<const uint2*>(d_free)[j];
}
__device__ __forceinline__ void end_publish(const Ring& rx, const Ring& tx, const Pool& pool, const RdEnd& e,
                                            const xsk_gpu_rx_plan* d_plan, const xsk_gpu_egress_counts* counts,
                                            xsk_gpu_rx_result* d_res) {
    const uint32_t tx_full = counts->n_tx_full, refilled = d_plan->refilled;
    if (e.n_tx) *tx.prod = e.tx_prod + e.n_tx;
    *pool.n_free = e.pool_n + e.pushed;
    if (e.release) *rx.cons = load_word(rx.cons) + e.release;
    if (d_res) {
        d_res->received = e.release;
        d_res->replied = e.n_tx;
        d_res->tx_full = tx_full;
        d_res->refilled = refilled;
    }
}

__global__ __launch_bounds__(kRdSmallThreads) void rx_end_small_kernel(Ring rx, Ring tx, Pool pool,
                                                                       const xsk_gpu_rx_plan* d_plan,
                                                                       const xsk_gpu_desc* d_tx, const uint64_t* d_free,
                                                                       const xsk_gpu_egress_counts* counts,
                                                                       uint32_t n_max, xsk_gpu_rx_result* d_res) {
    __shared__ RdEnd s_end;
    if (threadIdx.x == 0) s_end = end_decide(tx, pool, d_plan, counts, n_max);
    __syncthreads();
    const RdEnd e = s_end;
    end_copy(tx, pool, e, d_tx, d_free, threadIdx.x, kRdSmallThreads);
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) end_publish(rx, tx, pool, e, d_plan, counts, d_res);
}

__global__ __launch_bounds__(kRdCopy) void rx_end_copy_kernel(Ring tx, Pool pool, const xsk_gpu_rx_plan* d_plan,
                                                              const xsk_gpu_desc* d_tx, const uint64_t* d_free,
                                                              const xsk_gpu_egress_counts* counts, uint32_t n_max) {
    __shared__ RdEnd s_end;
    if (threadIdx.x == 0) s_end = end_decide(tx, pool, d_plan, counts, n_max);
    __syncthreads();
    end_copy(tx, pool, s_end, d_tx, d_free, rd_copy_first(blockIdx.x, threadIdx.x), rd_copy_stride(gridDim.x));
}

__global__ __launch_bounds__(kRdWave) void rx_end_publish_kernel(Ring rx, Ring tx, Pool pool,
                                                                 const xsk_gpu_rx_plan* d_plan,
                                                                 const xsk_gpu_egress_counts* counts, uint32_t n_max,
                                                                 xsk_gpu_rx_result* d_res) {
    if (threadIdx.x == 0) end_publish(rx, tx, pool, end_decide(tx, pool, d_plan, counts, n_max), d_plan, counts, d_res);
}

// ---- tx_complete ----
__device__ __forceinline__ RdComplete complete_decide(const Ring& comp, const Pool& pool, uint32_t max) {
    return rd_complete_plan(load_words(comp), comp.size, max, load_word(pool.n_free), pool.capacity);
}
__device__ __forceinline__ void complete_copy(const Ring& comp, const Pool& pool, const RdComplete& c, uint64_t first,
                                              uint64_t stride) {
    for (uint64_t j = first; j < c.pushed; j += stride)
        reinterpret_cast<uint2*>(pool.addr)[c.pool_n + (uint32_t)j] = *addr_slot(comp, c.cons + (uint32_t)j);
}
__device__ __forceinline__ void complete_publish(const Ring& comp, const Pool& pool, const RdComplete& c,
                                                 uint32_t* d_moved) {
    *pool.n_free = c.pool_n + c.pushed;
    if (c.n) *comp.cons = c.cons + c.n;
    if (d_moved) *d_moved = c.n;
}

__global__ __launch_bounds__(kRdSmallThreads) void tx_complete_small_kernel(Ring comp, Pool pool, uint32_t max,
                                                                            uint32_t* d_moved) {
    __shared__ RdComplete s_c;
    if (threadIdx.x == 0) s_c = complete_decide(comp, pool, max);
    __syncthreads();
    const RdComplete c = s_c;
    complete_copy(comp, pool, c, threadIdx.x, kRdSmallThreads);
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) complete_publish(comp, pool, c, d_moved);
}

__global__ __launch_bounds__(kRdCopy) void tx_complete_copy_kernel(Ring comp, Pool pool, uint32_t max) {
    __shared__ RdComplete s_c;
    if (threadIdx.x == 0) s_c = complete_decide(comp, pool, max);
    __syncthreads();
    complete_copy(comp, pool, s_c, rd_copy_first(blockIdx.x, threadIdx.x), rd_copy_stride(gridDim.x));
}

__global__ __launch_bounds__(kRdWave) void tx_complete_publish_kernel(Ring comp, Pool pool, uint32_t max,
                                                                      uint32_t* d_moved) {
    if (threadIdx.x == 0) complete_publish(comp, pool, complete_decide(comp, pool, max), d_moved);
}

// ---- the argument rules ----
// (a ring, a pool, a bound: xsk_ring_ports_device.h)
bool begin_ok(const xsk_gpu_ring_dev* rx, const xsk_gpu_ring_dev* fill, const xsk_gpu_ring_dev* tx,
              const xsk_gpu_pool_dev* pool, uint32_t max_batch, const void* d_descs, const void* d_plan) {
    return ring_ok(rx, 16u) && ring_ok(fill, 8u) && ring_ok(tx, 16u) && pool_ok(pool) && bound_ok(max_batch) &&
           d_descs && !((uintptr_t)d_descs & 15u) && d_plan && !((uintptr_t)d_plan & 3u);
}
bool end_ok(const xsk_gpu_ring_dev* rx, const xsk_gpu_ring_dev* tx, const xsk_gpu_pool_dev* pool, const void* d_plan,
            const void* d_tx, const void* d_free, const void* d_counts, uint32_t n_max, const void* d_res) {
    return ring_ok(rx, 16u) && ring_ok(tx, 16u) && pool_ok(pool) && bound_ok(n_max) && d_plan &&
           !((uintptr_t)d_plan & 3u) && d_tx && !((uintptr_t)d_tx & 15u) && d_free && !((uintptr_t)d_free & 7u) &&
           d_counts && !((uintptr_t)d_counts & 3u) && !((uintptr_t)d_res & 3u);
}

// The launches, behind the checks.
int begin_launch(const xsk_gpu_ring_dev* rx, const xsk_gpu_ring_dev* fill, const xsk_gpu_ring_dev* tx,
                 const xsk_gpu_pool_dev* pool, uint32_t max_batch, xsk_gpu_desc* d_descs, xsk_gpu_rx_plan* d_plan,
                 hipStream_t s) {
    const Ring r = ring_of(rx), f = ring_of(fill), t = ring_of(tx);
    const Pool p = pool_of(pool);
    if (max_batch <= kRdSmallMax) {
        rx_begin_small_kernel<<<dim3(1), dim3(kRdSmallThreads), 0, s>>>(r, f, t, p, max_batch, d_descs, d_plan);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    rx_begin_plan_kernel<<<dim3(1), dim3(kRdWave), 0, s>>>(r, f, t, p, max_batch, d_plan);
    HIP_TRY(hipGetLastError());
    rx_begin_copy_kernel<<<dim3(rd_nwg(max_batch)), dim3(kRdCopy), 0, s>>>(r, f, p, d_plan, d_descs);
    HIP_TRY(hipGetLastError());
    rx_begin_publish_kernel<<<dim3(1), dim3(kRdWave), 0, s>>>(f, p, d_plan);
    HIP_TRY(hipGetLastError());
    return 0;
}

int end_launch(const xsk_gpu_ring_dev* rx, const xsk_gpu_ring_dev* tx, const xsk_gpu_pool_dev* pool,
               const xsk_gpu_rx_plan* d_plan, const xsk_gpu_desc* d_tx, const uint64_t* d_free,
               const xsk_gpu_egress_counts* d_counts, uint32_t n_max, xsk_gpu_rx_result* d_res, hipStream_t s) {
    const Ring r = ring_of(rx), t = ring_of(tx);
    const Pool p = pool_of(pool);
    if (n_max <= kRdSmallMax) {
        rx_end_small_kernel<<<dim3(1), dim3(kRdSmallThreads), 0, s>>>(r, t, p, d_plan, d_tx, d_free, d_counts, n_max,
                                                                      d_res);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    rx_end_copy_kernel<<<dim3(rd_nwg(n_max)), dim3(kRdCopy), 0, s>>>(t, p, d_plan, d_tx, d_free, d_counts, n_max);
    HIP_TRY(hipGetLastError());
    rx_end_publish_kernel<<<dim3(1), dim3(kRdWave), 0, s>>>(r, t, p, d_plan, d_counts, n_max, d_res);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

size_t xsk_gpu_rx_step_dev_workspace_size(uint32_t max_batch) { return rd_layout(max_batch).bytes; }

int xsk_gpu_rx_begin_dev(const struct xsk_gpu_ring_dev* rx, const struct xsk_gpu_ring_dev* fill,
                         const struct xsk_gpu_ring_dev* tx, const struct xsk_gpu_pool_dev* pool, uint32_t max_batch,
                         struct xsk_gpu_desc* d_descs, struct xsk_gpu_rx_plan* d_plan, void* stream) {
    if (!begin_ok(rx, fill, tx, pool, max_batch, d_descs, d_plan)) return -EINVAL;
    return begin_launch(rx, fill, tx, pool, max_batch, d_descs, d_plan, (hipStream_t)stream);
}

int xsk_gpu_rx_end_dev(const struct xsk_gpu_ring_dev* rx, const struct xsk_gpu_ring_dev* tx,
                       const struct xsk_gpu_pool_dev* pool, const struct xsk_gpu_rx_plan* d_plan,
                       const struct xsk_gpu_desc* d_tx, const uint64_t* d_free,
                       const struct xsk_gpu_egress_counts* d_counts, uint32_t n_max, struct xsk_gpu_rx_result* d_res,
                       void* stream) {
    if (!end_ok(rx, tx, pool, d_plan, d_tx, d_free, d_counts, n_max, d_res)) return -EINVAL;
    return end_launch(rx, tx, pool, d_plan, d_tx, d_free, d_counts, n_max, d_res, (hipStream_t)stream);
}

int xsk_gpu_rx_step_dev(void* d_umem, uint64_t umem_size, const struct xsk_gpu_ring_dev* rx,
                        const struct xsk_gpu_ring_dev* fill, const struct xsk_gpu_ring_dev* tx,
                        const struct xsk_gpu_pool_dev* pool, uint32_t max_batch, uint32_t opts,
                        struct xsk_gpu_stats* d_stats, struct xsk_gpu_rx_result* d_res, void* d_workspace, void* stream) {
    // the workspace's arrays satisfy the rules of begin, the two composed calls and end by layout; what is left of those
    // rules is the caller's: the UMEM, the option bits, the counters
    if (!d_workspace || ((uintptr_t)d_workspace & 15u) || !d_umem || ((uintptr_t)d_umem & 15u) || (umem_size & 15u) ||
        (umem_size >> 48) || (opts & ~XSK_GPU_OPT_MASK) || ((uintptr_t)d_stats & 7u) || ((uintptr_t)d_res & 3u))
        return -EINVAL;
    uint8_t* const ws = (uint8_t*)d_workspace;
    const RdLayout l = rd_layout(bound_ok(max_batch) ? max_batch : 1u);
    xsk_gpu_rx_plan* const plan = (xsk_gpu_rx_plan*)(ws + l.plan);
    xsk_gpu_egress_counts* const counts = (xsk_gpu_egress_counts*)(ws + l.counts);
    xsk_gpu_desc* const descs = (xsk_gpu_desc*)(ws + l.descs);
    xsk_gpu_desc* const d_tx = (xsk_gpu_desc*)(ws + l.tx);
    uint64_t* const d_free = (uint64_t*)(ws + l.free_list);
    uint8_t* const verdicts = ws + l.verdicts;
    if (!begin_ok(rx, fill, tx, pool, max_batch, descs, plan) ||
        !end_ok(rx, tx, pool, plan, d_tx, d_free, counts, max_batch, d_res))
        return -EINVAL;
    const hipStream_t s = (hipStream_t)stream;
    int rc = begin_launch(rx, fill, tx, pool, max_batch, descs, plan, s);
    if (rc) return rc;
    rc = xsk_gpu_echo_dev_indirect(d_umem, umem_size, descs, &plan->received, max_batch, opts, verdicts, NULL, d_stats,
                                   stream);
    if (rc) return rc;
    rc = xsk_gpu_egress_dev(descs, verdicts, &plan->received, max_batch, &plan->tx_room, d_tx, d_free, counts, d_stats,
                            ws + l.egress, stream);
    if (rc) return rc;
    return end_launch(rx, tx, pool, plan, d_tx, d_free, counts, max_batch, d_res, s);
}

int xsk_gpu_tx_complete_dev(const struct xsk_gpu_ring_dev* comp, const struct xsk_gpu_pool_dev* pool, uint32_t max,
                            uint32_t* d_moved, void* stream) {
    if (!ring_ok(comp, 8u) || !pool_ok(pool) || max > XSK_GPU_MAX_BATCH || ((uintptr_t)d_moved & 3u)) return -EINVAL;
    const hipStream_t s = (hipStream_t)stream;
    if (max == 0) {
        if (d_moved) HIP_TRY(hipMemsetAsync(d_moved, 0, sizeof(*d_moved), s));
        return 0;
    }
    const Ring c = ring_of(comp);
    const Pool p = pool_of(pool);
    if (max <= kRdSmallMax) {
        tx_complete_small_kernel<<<dim3(1), dim3(kRdSmallThreads), 0, s>>>(c, p, max, d_moved);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    tx_complete_copy_kernel<<<dim3(rd_nwg(max)), dim3(kRdCopy), 0, s>>>(c, p, max);
    HIP_TRY(hipGetLastError());
    tx_complete_publish_kernel<<<dim3(1), dim3(kRdWave), 0, s>>>(c, p, max, d_moved);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
