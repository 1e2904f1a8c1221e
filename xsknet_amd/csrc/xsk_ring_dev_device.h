// xsk_ring_dev_device.h — the begin stage of the RX ring step as device code (xsk_gpu_rx_begin_dev()):
// peek the RX ring, linearise its descriptors, refill the fill ring from the pool, the plan.  What xsk_ring_dev.hip's
// begin kernels are built from, and stage 1 of the fused loop kernel (xsk_loop_fused_body.h, §9.11).  The ring and pool
// arguments, load_word and the rules of a ring and a pool are xsk_ring_ports_device.h's; the arithmetic is
// xsk_ring_dev.h's.  Everything here is in an anonymous namespace: nothing is exported.
#ifndef XSK_RING_DEV_DEVICE_H
#define XSK_RING_DEV_DEVICE_H

#include <hip/hip_runtime.h>

#include "../../include/xsk_gpu.h"
#include "xsk_ring_dev.h"
#include "xsk_ring_ports_device.h"

namespace xskgpu {
namespace {

__device__ __forceinline__ RdWords load_words(const Ring& r) {
    RdWords w;
    w.prod = load_word(r.prod);
    w.cons = load_word(r.cons);
    return w;
}

__device__ __forceinline__ uint2* addr_slot(const Ring& r, uint32_t idx) {
    return reinterpret_cast<uint2*>(r.ring) + rd_slot(idx, r.size);
}

// The plan is only 4-B aligned: eight word loads / stores.
__device__ __forceinline__ RdPlan load_plan(const xsk_gpu_rx_plan* d_plan) {
    RdPlan p;
    p.received = d_plan->received;
    p.tx_room = d_plan->tx_room;
    p.refilled = d_plan->refilled;
    p.rx_cons = d_plan->rx_cons;
    p.fq_prod = d_plan->fq_prod;
    p.pool_n = d_plan->pool_n;
    p.reserved[0] = p.reserved[1] = 0u;
    return p;
}
__device__ __forceinline__ void store_plan(xsk_gpu_rx_plan* d_plan, const RdPlan& p) {
    d_plan->received = p.received;
    d_plan->tx_room = p.tx_room;
    d_plan->refilled = p.refilled;
    d_plan->rx_cons = p.rx_cons;
    d_plan->fq_prod = p.fq_prod;
    d_plan->pool_n = p.pool_n;
    d_plan->reserved[0] = 0u;
    d_plan->reserved[1] = 0u;
}

// ---- begin ----
__device__ __forceinline__ RdPlan begin_decide(const Ring& rx, const Ring& fill, const Ring& tx, const Pool& pool,
                                               uint32_t max_batch) {
    return rd_begin_plan(load_words(rx), rx.size, load_words(fill), fill.size, load_words(tx), tx.size,
                         load_word(pool.n_free), pool.capacity, max_batch);
}
// The lanes first, first + stride, ...: a descriptor is one 16-B load and store, an address one 8-B load and store.
__device__ __forceinline__ void begin_copy(const Ring& rx, const Ring& fill, const Pool& pool, const RdPlan& p,
                                           xsk_gpu_desc* descs, uint64_t first, uint64_t stride) {
    for (uint64_t i = first; i < p.received; i += stride)
        reinterpret_cast<uint4*>(descs)[i] = *desc_slot(rx, p.rx_cons + (uint32_t)i);
    for (uint64_t i = first; i < p.refilled; i += stride)
        *addr_slot(fill, p.fq_prod + (uint32_t)i) = reinterpret_cast<const uint2*>(pool.addr)[rd_pop(p.pool_n, (uint32_t)i)];
}
__device__ __forceinline__ void begin_publish(const Ring& fill, const Pool& pool, const RdPlan& p) {
    if (p.received) {  // (a count word above the capacity ends clamped, whatever was popped)
        if (p.refilled) *fill.prod = rd_begin_fq_prod(p);
        *pool.n_free = rd_begin_pool_n(p);
    }
}

// The one-workgroup form, every lane of kRdSmallThreads: lane 0 decides, the plan meets the other lanes in *s_plan
// (LDS), a lane per entry copies, a fence and a barrier, lane 0 stores the plan and the new words.  Returns the plan.
__device__ __forceinline__ RdPlan rx_begin_small_body(const Ring& rx, const Ring& fill, const Ring& tx, const Pool& pool,
                                                      uint32_t max_batch, xsk_gpu_desc* descs, xsk_gpu_rx_plan* d_plan,
                                                      RdPlan* s_plan) {
    if (threadIdx.x == 0) *s_plan = begin_decide(rx, fill, tx, pool, max_batch);
    __syncthreads();
    const RdPlan p = *s_plan;
    begin_copy(rx, fill, pool, p, descs, threadIdx.x, kRdSmallThreads);
    __threadfence();  // the entries before the words that cover them
    __syncthreads();
    if (threadIdx.x == 0) {
        store_plan(d_plan, p);
        begin_publish(fill, pool, p);
    }
    return p;
}

}  // namespace
}  // namespace xskgpu

#endif  // XSK_RING_DEV_DEVICE_H
