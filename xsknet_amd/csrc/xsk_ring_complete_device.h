// xsk_ring_complete_device.h — every completion ring of a caller in one workgroup, as device code
// (xsk_gpu_tx_complete_rings_dev()): the rings by value (CompRings), what a workgroup decides from the
// words (CompLds), the copy (comp_copy), the publish (comp_publish) and the whole one-workgroup form
// (tx_complete_rings_small_body), which is also stage 7 of the fused loop kernel (xsk_loop_fused_body.h, §9.11); and the
// argument rules of that call and of the loop calls, xsk_gpu_rx_loop_dev() and xsk_gpu_rx_fused_loop_dev(), which check
// through one function (loop_complete_ok).  The ring and pool arguments and load_word are xsk_ring_ports_device.h's, the
// arithmetic xsk_ring_complete.h's.  Everything here is in an anonymous namespace: nothing is exported.
#ifndef XSK_RING_COMPLETE_DEVICE_H
#define XSK_RING_COMPLETE_DEVICE_H

#include <hip/hip_runtime.h>

#include "../../include/xsk_gpu.h"
#include "xsk_ring_complete.h"
#include "xsk_ring_pass_device.h"
#include "xsk_ring_ports_device.h"

namespace xskgpu {
namespace {

struct CompRings {  // the completion rings, by value in the kernel arguments
    Ring r[kRcMaxRings];
};
static_assert(sizeof(CompRings) + sizeof(Pool) + 4 * 8 <= 4096, "the kernel arguments");

__device__ __forceinline__ uint2* comp_addr_slot(const Ring& r, uint32_t slot) {
    return reinterpret_cast<uint2*>(r.ring) + slot;
}

// What one workgroup decides from the words, in LDS.
struct CompLds {
    uint32_t n[kRcMaxRings], cons[kRcMaxRings];
    uint32_t A[kRcMaxBounds];
    uint32_t pool_n;
};

// (comp_decide -- every lane of the workgroup reads the words, two barriers -- stays in xsk_ring_complete.hip, whose text
// tests/test_tx_complete_rings_spec.py reads for its load_word calls; the fused loop kernel has its own statement of
// it, lf_comp_decide in xsk_loop_fused_body.h, and the one-workgroup body below takes either.)

// The lanes first, first + stride, ...: an address is one 8-B load and store.
__device__ __forceinline__ void comp_copy(const CompRings& comp, uint32_t n_rings, const Pool& pool, const CompLds* s,
                                          uint64_t first, uint64_t stride) {
    const uint32_t total = s->A[n_rings];
    for (uint64_t L = first; L < total; L += stride) {
        const RcSrc src = rc_src(s->A, n_rings, (uint32_t)L);
        const Ring& ring = comp.r[src.ring];
        reinterpret_cast<uint2*>(pool.addr)[rc_pool_slot(s->pool_n, (uint32_t)L)] =
            *comp_addr_slot(ring, rc_ring_slot(s->cons[src.ring], src.j, ring.size));
    }
}

// Lane q stores ring q's consumer word and d_moved[q]; lane 0 the pool's count and *d_pushed.
__device__ __forceinline__ void comp_publish(const CompRings& comp, uint32_t n_rings, const Pool& pool, const CompLds* s,
                                             uint32_t* d_moved, uint32_t* d_pushed) {
    const uint32_t t = threadIdx.x, nt = blockDim.x;
    for (uint32_t q = t; q < n_rings; q += nt) {
        const uint32_t n = s->n[q];
        if (n) *comp.r[q].cons = rc_cons_after(s->cons[q], n);
        if (d_moved) d_moved[q] = n;
    }
    if (t == 0) {
        *pool.n_free = rc_pool_after(s->pool_n, s->A[n_rings]);
        if (d_pushed) *d_pushed = s->A[n_rings];
    }
}

// ---- max <= 1024: one workgroup of kRcSmallThreads; the body every lane calls, *s in LDS ----
template <class Decide>
__device__ __forceinline__ void tx_complete_rings_small_body(const CompRings& comp, uint32_t n_rings, const Pool& pool,
                                                             uint32_t max, uint32_t* d_moved, uint32_t* d_pushed,
                                                             CompLds* s, Decide decide) {
    decide(comp, n_rings, pool, max, s);
    comp_copy(comp, n_rings, pool, s, threadIdx.x, kRcSmallThreads);
    __threadfence();  // the entries before the words that cover them
    __syncthreads();
    comp_publish(comp, n_rings, pool, s, d_moved, d_pushed);
}

// ---- the argument rules ----
inline bool shares(const xsk_gpu_ring_dev* a, const xsk_gpu_ring_dev* b) {
    return a->d_ring == b->d_ring || a->d_consumer == b->d_consumer;
}
// n_rings address rings, each valid, no two sharing an entry array or a consumer word; a pool, a bound, two outputs
inline bool complete_ok(const xsk_gpu_ring_dev* comp, uint32_t n_rings, const xsk_gpu_pool_dev* pool, uint32_t max,
                 const uint32_t* d_moved, const uint32_t* d_pushed) {
    if (!comp || n_rings < 1u || n_rings > kRcMaxRings || !pool_ok(pool) || max > XSK_GPU_MAX_BATCH ||
        ((uintptr_t)d_moved & 3u) || ((uintptr_t)d_pushed & 3u))
        return false;
    for (uint32_t q = 0; q < n_rings; ++q) {
        if (!ring_ok(comp + q, 8u)) return false;
        for (uint32_t k = 0; k < q; ++k)
            if (shares(comp + k, comp + q)) return false;
    }
    return true;
}
// no completion ring shares its entry array or its consumer word with a ring of the step (the step's own rules are the
// step's: a ring it will refuse anyway refuses here too)
inline bool loop_rings_ok(const xsk_gpu_ring_dev* comp, uint32_t n_comp, const xsk_gpu_ring_dev* rx,
                   const xsk_gpu_ring_dev* fill, const xsk_gpu_ring_dev* tx, uint32_t n_ports,
                   const xsk_gpu_ring_dev* stack) {
    if (!rx || !fill || !tx || n_ports < 1u || n_ports > kEpMaxPorts) return false;
    for (uint32_t q = 0; q < n_comp; ++q) {
        if (shares(comp + q, rx) || shares(comp + q, fill) || (stack && shares(comp + q, stack))) return false;
        for (uint32_t p = 0; p < n_ports; ++p)
            if (shares(comp + q, tx + p)) return false;
    }
    return true;
}

// Every rule of xsk_gpu_rx_loop_dev(): with completion rings the completion call's and the aliasing with the step's
// rings (n_comp == 0 ignores comp, complete_max and the two outputs), then the step's own (pass_step_ok).
inline bool loop_complete_ok(const void* d_umem, uint64_t umem_size, const xsk_gpu_ring_dev* rx,
                             const xsk_gpu_ring_dev* fill, const xsk_gpu_ring_dev* tx, const xsk_gpu_ring_dev* stack,
                             const xsk_gpu_pool_dev* pool, uint32_t max_batch, uint32_t opts,
                             const xsk_gpu_steer_entry* d_table, uint32_t n_entries, uint32_t default_port,
                             uint32_t n_ports, const uint64_t* d_bound, const void* d_port_counts, const void* d_stats,
                             const void* d_port_stats, const void* d_res, const xsk_gpu_ring_dev* comp, uint32_t n_comp,
                             uint32_t complete_max, const uint32_t* d_moved, const uint32_t* d_pushed,
                             const void* d_workspace) {
    if (n_comp && (!complete_ok(comp, n_comp, pool, complete_max, d_moved, d_pushed) ||
                   !loop_rings_ok(comp, n_comp, rx, fill, tx, n_ports, stack)))
        return false;
    return pass_step_ok(d_umem, umem_size, rx, fill, tx, stack, pool, max_batch, opts, d_table, n_entries, default_port,
                        n_ports, d_bound, d_port_counts, d_stats, d_port_stats, d_res, d_workspace);
}

}  // namespace
}  // namespace xskgpu

#endif  // XSK_RING_COMPLETE_DEVICE_H
