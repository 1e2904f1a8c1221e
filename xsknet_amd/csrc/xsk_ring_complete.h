// xsk_ring_complete.h — the arithmetic of xsk_gpu_tx_complete_rings_dev() and xsk_gpu_rx_loop_dev() (include/xsk_gpu.h;
// DESIGN.md §9.10): every completion ring of a caller drained into the pool by one call.  What each ring gives up, how
// much of it the pool still takes, which ring and entry a position of the pool's new part comes from, and the grid
// sizes.  Host and device: xsk_ring_complete.hip's kernels and its host launch call these functions, and
// tests/c/test_ring_complete.cpp replays both paths with them on the CPU, into heap arrays of exactly the rings' and the
// pool's sizes under AddressSanitizer.
//
// The ring and pool rules are xsk_ring_dev.h's (rd_used, rd_pool_n, rd_slot), the owner search xsk_egress_ports.h's
// (ep_owner).  With pool_n = min(*d_n_free, capacity), room = capacity - pool_n and, for ascending q < n_rings,
//   n_q     = min(used(comp[q]), max)           what ring q's consumer word advances by
//   A_0     = 0
//   p_q     = min(n_q, room - A_q)              what the pool takes of ring q
//   A_{q+1} = A_q + p_q                         <= room <= capacity: no sum wraps, whatever the rings hold
// position L < A_{n_rings} of the pool's new part, d_addr[pool_n + L], is entry rd_slot(cons_q + (L - A_q)) of the ring q
// with A_q <= L < A_{q+1}.  That is xsk_gpu_tx_complete_dev() applied to ring 0, 1, ... in turn: the pool's count after
// ring q is pool_n + A_{q+1}, and ring q + 1 meets the room that is left.
#ifndef XSK_RING_COMPLETE_H
#define XSK_RING_COMPLETE_H

#include "xsk_egress_ports.h"
#include "xsk_ring_dev.h"

namespace xskgpu {

constexpr uint32_t kRcMaxRings = kEpMaxPorts + 1u;  // == XSK_GPU_COMPLETE_MAX_RINGS: a ring per port, and the stack's
constexpr uint32_t kRcMaxBounds = kRcMaxRings + 1u;  // A_0 .. A_{n_rings}
constexpr uint32_t kRcSmallMax = kRdSmallMax;        // == XSK_GPU_LOWLAT_MAX: one launch of one workgroup up to here
constexpr uint32_t kRcSmallThreads = kRdSmallThreads;
constexpr uint32_t kRcPublish = 128;   // the publish launch of the larger bounds: a lane per ring
constexpr uint32_t kRcMaxGrid = 4096;  // workgroups of the copy launch at most; what is left is walked in strides

// n_q
XSK_RD_FN uint32_t rc_take(uint32_t prod, uint32_t cons, uint32_t size, uint32_t max) {
    return rd_min(rd_used(prod, cons, size), max);
}
// room
XSK_RD_FN uint32_t rc_room(uint32_t pool_n, uint32_t capacity) { return capacity - pool_n; }
// p_q, given A_q <= room
XSK_RD_FN uint32_t rc_share(uint32_t n_q, uint32_t room, uint32_t a_q) { return rd_min(n_q, room - a_q); }
// A_q from n[0, q): lane q takes A_q (q <= n_rings <= 65 steps; the running clamp keeps every partial sum <= room).
XSK_RD_FN uint32_t rc_prefix(const uint32_t* n, uint32_t q, uint32_t room) {
    uint32_t a = 0;
    for (uint32_t k = 0; k < q; ++k) a += rc_share(n[k], room, a);
    return a;
}

// Position L < A_{n_rings}: the ring it comes from and the entry's distance from that ring's consumer word.  A_0 == 0
// and A ascends, so every such L has an owner, and empty shares are never returned; j < p_ring <= used(ring) <= size.
struct RcSrc {
    uint32_t ring, j;
};
XSK_RD_FN RcSrc rc_src(const uint32_t* A, uint32_t n_rings, uint32_t L) {
    const EpOwner ow = ep_owner(A, n_rings, L);
    RcSrc s;
    s.ring = ow.port;
    s.j = L - A[ow.port];
    return s;
}
// where it lands, and where it lies: pool_n + L < pool_n + room == capacity
XSK_RD_FN uint32_t rc_pool_slot(uint32_t pool_n, uint32_t L) { return pool_n + L; }
XSK_RD_FN uint32_t rc_ring_slot(uint32_t cons, uint32_t j, uint32_t size) { return rd_slot(cons + j, size); }
// what the call leaves in the words
XSK_RD_FN uint32_t rc_cons_after(uint32_t cons, uint32_t n_q) { return cons + n_q; }
XSK_RD_FN uint32_t rc_pool_after(uint32_t pool_n, uint32_t a_total) { return pool_n + a_total; }

// ---- grids ----
// One workgroup of kRcSmallThreads up to kRcSmallMax.  Above: a copy launch of rc_nwg() workgroups of kRdCopy lanes
// walking rd_copy_first() + k * rd_copy_stride() over L, sized on the host from what the rings can give at most, the
// sum of min(max, size_q) (the words are the device's), then a publish launch of kRcPublish lanes.
XSK_RD_FN uint64_t rc_span(const uint32_t* sizes, uint32_t n_rings, uint32_t max) {
    uint64_t sum = 0;
    for (uint32_t q = 0; q < n_rings; ++q) sum += rd_min(max, sizes[q]);
    return sum;
}
XSK_RD_FN uint32_t rc_nwg(uint64_t span) {
    const uint64_t nwg = (span + kRdCopy - 1u) / kRdCopy;
    return nwg < 1u ? 1u : nwg > kRcMaxGrid ? kRcMaxGrid : (uint32_t)nwg;
}

}  // namespace xskgpu

#endif  // XSK_RING_COMPLETE_H
