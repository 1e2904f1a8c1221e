// xsk_ring_complete.hip — every completion ring of a caller in one call: xsk_gpu_tx_complete_rings_dev() (what
// xsk_gpu_tx_complete_dev() leaves when it is called for ring 0, 1, ... in turn, from up to 65 rings into one pool) and
// xsk_gpu_rx_loop_dev() (xsk_gpu_rx_pass_step_dev(), then that call, on one stream: the whole body of the reference's
// handle_receive_packets() over all sockets).  include/xsk_gpu.h; DESIGN.md §9.10.  Every index and count is a word in
// device memory, read when the kernels execute; the 65 ring structs travel by value in the kernel arguments.
//
// Two paths, the arithmetic of both in xsk_ring_complete.h (host and device); the ring and pool arguments, load_word and
// the rules of a ring and a pool are xsk_ring_ports_device.h's:
//   max <= 1024: one launch of one 1024-thread workgroup -- lane q reads ring q's two words, the n_q and the clamped
//                prefix A meet in LDS, the lanes stride over the positions L < A_{n_rings}, find each one's ring by
//                search in A and move its entry as one 8-B load and store; a fence and a barrier; lane q stores ring
//                q's consumer word and d_moved[q], lane 0 the pool's count and *d_pushed;
//   larger:      a kernel boundary in place of the last barrier -- the copy grid (256 entries a workgroup, strided
//                over L, every workgroup deciding for itself from the same words), then a 128-lane publish launch, the
//                only launch that stores a word.
// No launch stores an index word for entries another launch stores, no atomic hands out a slot, no workgroup waits on
// another, nothing is polled.  Index words are read through the vector path (load_word).  Latency bound: 8 B in and out
// per entry, no frame byte touched, no MFMA.
#include <errno.h>
#include <stddef.h>

#include "../../include/xsk_gpu.h"
#include "xsk_hip_util.h"
#include "xsk_ring_complete.h"
#include "xsk_ring_complete_device.h"
#include "xsk_ring_ports_device.h"

using namespace xskgpu;

static_assert(kRcSmallMax == XSK_GPU_LOWLAT_MAX, "the one-launch path serves the RX loop's sizes");
static_assert(kRcMaxRings == XSK_GPU_COMPLETE_MAX_RINGS && kRcMaxRings == XSK_GPU_STEER_MAX_PORTS + 1u,
              "a completion ring per port, and the stack consumer's");
static_assert(kRcPublish >= kRcMaxRings, "the publish launch has a lane per ring");

namespace {

// (CompRings, CompLds, comp_copy, comp_publish and the one-workgroup form,
// tx_complete_rings_small_body: xsk_ring_complete_device.h)

// Every lane of the workgroup calls it; two barriers.  Lanes walk the rings in strides of the workgroup's size.
__device__ __forceinline__ void comp_decide(const CompRings& comp, uint32_t n_rings, const Pool& pool, uint32_t max,
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

__global__ __launch_bounds__(kRcSmallThreads) void tx_complete_rings_small_kernel(CompRings comp, uint32_t n_rings,
                                                                                  Pool pool, uint32_t max,
                                                                                  uint32_t* d_moved, uint32_t* d_pushed) {
    __shared__ CompLds s;
    tx_complete_rings_small_body(comp, n_rings, pool, max, d_moved, d_pushed, &s, comp_decide);
}

__global__ __launch_bounds__(kRdCopy) void tx_complete_rings_copy_kernel(CompRings comp, uint32_t n_rings, Pool pool,
                                                                         uint32_t max) {
    __shared__ CompLds s;
    comp_decide(comp, n_rings, pool, max, &s);
    comp_copy(comp, n_rings, pool, &s, rd_copy_first(blockIdx.x, threadIdx.x), rd_copy_stride(gridDim.x));
}

__global__ __launch_bounds__(kRcPublish) void tx_complete_rings_publish_kernel(CompRings comp, uint32_t n_rings, Pool pool,
                                                                               uint32_t max, uint32_t* d_moved,
                                                                               uint32_t* d_pushed) {
    __shared__ CompLds s;
    comp_decide(comp, n_rings, pool, max, &s);
    comp_publish(comp, n_rings, pool, &s, d_moved, d_pushed);
}

// ---- the argument rules (complete_ok, loop_rings_ok, loop_complete_ok: xsk_ring_complete_device.h) ----

// The launches, behind the checks.
int complete_launch(const xsk_gpu_ring_dev* comp, uint32_t n_rings, const xsk_gpu_pool_dev* pool, uint32_t max,
                    uint32_t* d_moved, uint32_t* d_pushed, hipStream_t s) {
    if (max == 0) {
        if (d_moved) HIP_TRY(hipMemsetAsync(d_moved, 0, (size_t)n_rings * sizeof(*d_moved), s));
        if (d_pushed) HIP_TRY(hipMemsetAsync(d_pushed, 0, sizeof(*d_pushed), s));
        return 0;
    }
    CompRings c;
    uint32_t sizes[kRcMaxRings];
    for (uint32_t q = 0; q < kRcMaxRings; ++q) {
        c.r[q] = q < n_rings ? ring_of(comp + q) : Ring{nullptr, nullptr, nullptr, 1u};
        sizes[q] = c.r[q].size;
    }
    const Pool p = pool_of(pool);
    if (max <= kRcSmallMax) {
        tx_complete_rings_small_kernel<<<dim3(1), dim3(kRcSmallThreads), 0, s>>>(c, n_rings, p, max, d_moved, d_pushed);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    tx_complete_rings_copy_kernel<<<dim3(rc_nwg(rc_span(sizes, n_rings, max))), dim3(kRdCopy), 0, s>>>(c, n_rings, p, max);
    HIP_TRY(hipGetLastError());
    tx_complete_rings_publish_kernel<<<dim3(1), dim3(kRcPublish), 0, s>>>(c, n_rings, p, max, d_moved, d_pushed);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int xsk_gpu_tx_complete_rings_dev(const struct xsk_gpu_ring_dev* comp, uint32_t n_rings,
                                  const struct xsk_gpu_pool_dev* pool, uint32_t max, uint32_t* d_moved,
                                  uint32_t* d_pushed, void* stream) {
    if (!complete_ok(comp, n_rings, pool, max, d_moved, d_pushed)) return -EINVAL;
    return complete_launch(comp, n_rings, pool, max, d_moved, d_pushed, (hipStream_t)stream);
}

int xsk_gpu_rx_loop_dev(void* d_umem, uint64_t umem_size, const struct xsk_gpu_ring_dev* rx,
                        const struct xsk_gpu_ring_dev* fill, const struct xsk_gpu_ring_dev* tx,
                        const struct xsk_gpu_ring_dev* stack, const struct xsk_gpu_pool_dev* pool, uint32_t max_batch,
                        uint32_t opts, const struct xsk_gpu_steer_entry* d_table, uint32_t n_entries,
                        uint32_t default_port, uint32_t n_ports, const uint64_t* d_bound, uint8_t* d_actions,
                        uint8_t* d_ports, struct xsk_gpu_egress_counts* d_port_counts, struct xsk_gpu_stats* d_stats,
                        struct xsk_gpu_stats* d_port_stats, struct xsk_gpu_rx_pass_result* d_res,
                        const struct xsk_gpu_ring_dev* comp, uint32_t n_comp, uint32_t complete_max, uint32_t* d_moved,
                        uint32_t* d_pushed, void* d_workspace, void* stream) {
    // every rule of the call -- the completion call's, the aliasing with the step's rings and the step's own -- before
    // the step launches anything; the fused call (xsk_loop_fused.hip) checks through the same function
    if (!loop_complete_ok(d_umem, umem_size, rx, fill, tx, stack, pool, max_batch, opts, d_table, n_entries, default_port,
                          n_ports, d_bound, d_port_counts, d_stats, d_port_stats, d_res, comp, n_comp, complete_max,
                          d_moved, d_pushed, d_workspace))
        return -EINVAL;
    const int rc = xsk_gpu_rx_pass_step_dev(d_umem, umem_size, rx, fill, tx, stack, pool, max_batch, opts, d_table,
                                            n_entries, default_port, n_ports, d_bound, d_actions, d_ports, d_port_counts,
                                            d_stats, d_port_stats, d_res, d_workspace, stream);
    if (rc || !n_comp) return rc;
    return complete_launch(comp, n_comp, pool, complete_max, d_moved, d_pushed, (hipStream_t)stream);
}

}  // extern "C"
