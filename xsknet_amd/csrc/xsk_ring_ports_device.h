// xsk_ring_ports_device.h — what the end kernels of xsk_ring_ports.hip (xsk_gpu_rx_ports_end_dev()) and
// of xsk_ring_pass.hip (xsk_gpu_rx_pass_end_dev(), §9.9) share: the ring and pool arguments as the kernels take them,
// the decision a workgroup makes from the words (EndLds, end_decide), the copy (end_copy) and the publish (end_publish),
// and the argument rules of a ring, a pool, a bound and a set of ports.  Device code and host checks of those two files,
// and the ring and pool arguments, load_word and the ring and pool rules for xsk_ring_complete.hip (§9.10); the
// arithmetic is xsk_ring_ports.h's.  Everything here is in an anonymous namespace: nothing is exported.
#ifndef XSK_RING_PORTS_DEVICE_H
#define XSK_RING_PORTS_DEVICE_H

#include <hip/hip_runtime.h>

#include "../../include/xsk_gpu.h"
#include "xsk_ring_ports.h"

namespace xskgpu {
namespace {

// What the kernels take of a struct xsk_gpu_ring_dev / xsk_gpu_pool_dev (read when the call is made).
struct Ring {
    uint32_t* prod;
    uint32_t* cons;
    void* ring;
    uint32_t size;
};
struct Rings {  // one TX ring per port, by value in the kernel arguments
    Ring r[kEpMaxPorts];
};
struct Pool {
    uint64_t* addr;
    uint32_t* n_free;
    uint32_t capacity;
};
static_assert(sizeof(Rings) == 2048, "the rings of 64 ports fit the kernel arguments");

// A word this or a later launch of the call stores: a vector load, never the scalar cache.
__device__ __forceinline__ uint32_t load_word(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint4* desc_slot(const Ring& r, uint32_t idx) {
    return reinterpret_cast<uint4*>(r.ring) + rd_slot(idx, r.size);
}

// ---- end ----
// What one workgroup decides from the words, in LDS: the offsets, every port's ring share, list share and producer
// word, where its addresses begin in the pool's list.
struct EndLds {
    uint32_t raw[kEpMaxBounds];  // d_off as read
    uint32_t o[kEpMaxBounds];
    uint32_t F[kEpMaxBounds];
    uint32_t t[kEpMaxPorts], f[kEpMaxPorts], prod[kEpMaxPorts], full[kEpMaxPorts];
    uint32_t r, pool_n;
};

// Every lane of the workgroup calls it; four barriers.  Lanes walk the ports in strides of the workgroup's size, so a
// single wave serves the 65 offsets of 64 ports too.
__device__ __forceinline__ void end_decide(const Rings& tx, uint32_t n_ports, const Pool& pool,
                                           const xsk_gpu_rx_plan* d_plan, const uint32_t* d_off,
                                           const xsk_gpu_egress_counts* counts, uint32_t n_max, EndLds* s) {
    const uint32_t t = threadIdx.x, nt = blockDim.x;
    for (uint32_t p = t; p <= n_ports; p += nt) s->raw[p] = d_off[p];
    if (t == 0) {
        s->r = rp_received(d_plan->received, n_max);
        s->pool_n = rd_pool_n(load_word(pool.n_free), pool.capacity);
    }
    __syncthreads();
    for (uint32_t p = t; p <= n_ports; p += nt) s->o[p] = rp_offset(s->raw, p, n_max);
    __syncthreads();
    for (uint32_t p = t; p < n_ports; p += nt) {
        const Ring& ring = tx.r[p];
        const uint32_t n_p = s->o[p + 1u] - s->o[p];
        s->prod[p] = load_word(ring.prod);
        s->t[p] = rp_port_tx(counts[p].n_tx, n_p, rd_free(s->prod[p], load_word(ring.cons), ring.size));
        s->f[p] = rp_port_free(counts[p].n_free, n_p);
        s->full[p] = counts[p].n_tx_full;
    }
    __syncthreads();
    for (uint32_t p = t; p <= n_ports; p += nt) s->F[p] = rp_prefix(s->f, p);
    __syncthreads();
}

// The lanes first, first + stride, ...: a TX entry is one 16-B load and store, an address one 8-B load and store.
__device__ __forceinline__ void end_copy(const Rings& tx, uint32_t n_ports, const Pool& pool, const EndLds* s,
                                         uint32_t n_rest, const xsk_gpu_desc* d_tx, const uint64_t* d_free,
                                         const uint64_t* rest, uint64_t first, uint64_t stride) {
    for (uint64_t j = first; j < s->o[n_ports]; j += stride) {
        const RpTx x = rp_tx_lane(s->o, s->t, n_ports, (uint32_t)j);
        if (x.on) *desc_slot(tx.r[x.port], s->prod[x.port] + x.k) = reinterpret_cast<const uint4*>(d_tx)[j];
    }
    const uint32_t pushed = rp_pushed(s->F[n_ports], n_rest, pool.capacity, s->pool_n);
    for (uint64_t L = first; L < pushed; L += stride) {
        const RpSrc src = rp_pool_src(s->F, s->o, n_ports, (uint32_t)L);
        pool.addr[s->pool_n + (uint32_t)L] = src.rest ? rest[src.idx] : d_free[src.idx];
    }
}

// Lane p stores port p's producer word; lane 0 the pool's count, the RX consumer word and *d_res.
__device__ __forceinline__ void end_publish(const Ring& rx, const Rings& tx, uint32_t n_ports, const Pool& pool,
                                            const EndLds* s, uint32_t n_rest, const xsk_gpu_rx_plan* d_plan,
                                            xsk_gpu_rx_steer_result* d_res) {
    const uint32_t p = threadIdx.x;
    if (p < n_ports && s->t[p]) *tx.r[p].prod = s->prod[p] + s->t[p];
    if (p != 0) return;
    const uint32_t pushed = rp_pushed(s->F[n_ports], n_rest, pool.capacity, s->pool_n);
    *pool.n_free = s->pool_n + pushed;
    if (s->r) *rx.cons = load_word(rx.cons) + s->r;
    if (d_res) {
        uint32_t replied = 0, tx_full = 0;
        for (uint32_t q = 0; q < n_ports; ++q) {
            replied += s->t[q];
            tx_full += s->full[q];
        }
        d_res->received = s->r;
        d_res->redirected = s->o[n_ports];
        d_res->replied = replied;
        d_res->tx_full = tx_full;
        d_res->refilled = d_plan->refilled;
        d_res->freed = pushed;
        d_res->reserved[0] = 0u;
        d_res->reserved[1] = 0u;
    }
}

__device__ __forceinline__ uint64_t desc_addr(const xsk_gpu_desc* descs, uint32_t i) {
    const uint2 a = *reinterpret_cast<const uint2*>(descs + i);
    return ((uint64_t)a.y << 32) | a.x;
}

// ---- the argument rules (those of xsk_ring_dev.hip for a ring, a pool and a bound) ----
inline bool ring_ok(const xsk_gpu_ring_dev* r, uintptr_t entry_align) {
    return r && r->d_producer && r->d_consumer && r->d_ring && !((uintptr_t)r->d_producer & 3u) &&
           !((uintptr_t)r->d_consumer & 3u) && !((uintptr_t)r->d_ring & (entry_align - 1u)) && rd_size_ok(r->size) &&
           r->reserved == 0u;
}
inline bool pool_ok(const xsk_gpu_pool_dev* p) {
    return p && p->d_addr && p->d_n_free && !((uintptr_t)p->d_addr & 7u) && !((uintptr_t)p->d_n_free & 3u) &&
           p->capacity >= 1u && p->reserved == 0u;
}
inline bool bound_ok(uint32_t n) { return n >= 1u && n <= XSK_GPU_MAX_BATCH; }
// n_ports rings, each valid, no two sharing an entry array or a producer word
inline bool ports_ok(const xsk_gpu_ring_dev* tx, uint32_t n_ports) {
    if (!tx || n_ports < 1u || n_ports > kEpMaxPorts) return false;
    for (uint32_t p = 0; p < n_ports; ++p) {
        if (!ring_ok(tx + p, 16u)) return false;
        for (uint32_t q = 0; q < p; ++q)
            if (tx[q].d_ring == tx[p].d_ring || tx[q].d_producer == tx[p].d_producer) return false;
    }
    return true;
}
inline bool end_ok(const xsk_gpu_ring_dev* rx, const xsk_gpu_ring_dev* tx, uint32_t n_ports, const xsk_gpu_pool_dev* pool,
                   const void* d_plan, const void* d_descs, const void* d_actions, const void* d_off, const void* d_tx,
                   const void* d_free, const void* d_counts, uint32_t n_max, const void* d_res, const void* d_workspace) {
    return ring_ok(rx, 16u) && ports_ok(tx, n_ports) && pool_ok(pool) && bound_ok(n_max) && d_plan &&
           !((uintptr_t)d_plan & 3u) && d_descs && !((uintptr_t)d_descs & 15u) && d_actions && d_off &&
           !((uintptr_t)d_off & 3u) && d_tx && !((uintptr_t)d_tx & 15u) && d_free && !((uintptr_t)d_free & 7u) &&
           d_counts && !((uintptr_t)d_counts & 3u) && !((uintptr_t)d_res & 3u) && d_workspace &&
           !((uintptr_t)d_workspace & 15u);
}

inline Ring ring_of(const xsk_gpu_ring_dev* r) { return Ring{r->d_producer, r->d_consumer, r->d_ring, r->size}; }
inline Pool pool_of(const xsk_gpu_pool_dev* p) { return Pool{p->d_addr, p->d_n_free, p->capacity}; }
inline Rings rings_of(const xsk_gpu_ring_dev* tx, uint32_t n_ports) {
    Rings r;
    for (uint32_t p = 0; p < kEpMaxPorts; ++p) r.r[p] = p < n_ports ? ring_of(tx + p) : Ring{nullptr, nullptr, nullptr, 1u};
    return r;
}

}  // namespace
}  // namespace xskgpu

#endif  // XSK_RING_PORTS_DEVICE_H
