// xsk_ring_ports.h — the arithmetic of xsk_gpu_rx_prepare_ports_dev(), xsk_gpu_rx_ports_end_dev() and
// xsk_gpu_rx_step_steer_dev() (include/xsk_gpu.h): the steered RX step, one TX ring per port.  What a
// port's ring takes of its TX list, where every address of the pool's one ordered list comes from, which descriptors
// are pads, which frames are the rest, and the grid and workspace sizes.  Host and device: xsk_ring_ports.hip's kernels
// and its host launch call these functions, and tests/c/test_ring_ports.cpp replays both paths with them on the CPU,
// into heap arrays of exactly the rings' sizes under AddressSanitizer.
//
// The ring and pool rules are xsk_ring_dev.h's (rd_used, rd_free, rd_pool_n, rd_slot), the segments xsk_egress_ports.h's
// (o_p = the clamped running maximum of d_off; ep_owner).  With r = min(received, n_max), n_p = o_{p+1} - o_p and
// c_p = d_counts[p]:
//   t_p = min(c_p.n_tx, n_p, free(tx[p]))       TX entries of port p, from d_tx[o_p + k]
//   f_p = min(c_p.n_free, n_p)                  addresses of port p's free list, from d_free[o_p + j]
//   F_p = f_0 + ... + f_{p-1}                   where port p's addresses begin in the pool's list
//   rest = { i < r : d_actions[i] != REDIRECT } in batch order, behind F_{n_ports}
// Position L of the list lands at d_addr[pool_n + L] iff L < pushed = min(F_{n_ports} + |rest|, capacity - pool_n).
#ifndef XSK_RING_PORTS_H
#define XSK_RING_PORTS_H

#include "xsk_egress_ports.h"
#include "xsk_ring_dev.h"

namespace xskgpu {

constexpr uint32_t kRpSmallMax = kRdSmallMax;  // == XSK_GPU_LOWLAT_MAX: one launch of one workgroup up to here
constexpr uint32_t kRpSmallThreads = kRdSmallThreads;
constexpr uint32_t kRpSmallWaves = kRpSmallThreads / kCpWave;

// r: the frames begin took, as every launch of prepare and end clamps the plan's word.
XSK_RD_FN uint32_t rp_received(uint32_t word, uint32_t n_max) { return rd_min(word, n_max); }

// ---- prepare ----
// d_descs[i] for i in [r, n_max) becomes the pad descriptor { 0, 0, 0 }: len < 14, which every option word's filter
// rule drops, so a steering call over all n_max descriptors redirects exactly what it would over the first r.
XSK_RD_FN bool rp_pad(uint32_t i, uint32_t r, uint32_t n_max) { return i >= r && i < n_max; }

// ---- end: the segments and what each port's ring and the pool take ----
// o_p from the raw offset words (ep_offsets() one element at a time: lane p takes o_p).
XSK_RD_FN uint32_t rp_offset(const uint32_t* raw, uint32_t p, uint32_t n_max) {
    uint32_t run = 0;
    for (uint32_t q = 0; q <= p; ++q) run = ep_max(run, raw[q]);
    return ep_clamp(run, n_max);
}
XSK_RD_FN uint32_t rp_port_tx(uint32_t c_n_tx, uint32_t n_p, uint32_t room) { return rd_min(rd_min(c_n_tx, n_p), room); }
XSK_RD_FN uint32_t rp_port_free(uint32_t c_n_free, uint32_t n_p) { return rd_min(c_n_free, n_p); }
// F_p: the sum of f[0, p).  At most n_max, because the segments are disjoint parts of [0, n_max).
XSK_RD_FN uint32_t rp_prefix(const uint32_t* f, uint32_t p) {
    uint32_t sum = 0;
    for (uint32_t q = 0; q < p; ++q) sum += f[q];
    return sum;
}
// A frame of the rest: received, and not on any port's list.
XSK_RD_FN bool rp_rest(uint32_t i, uint32_t r, uint8_t action) { return i < r && action != XSK_GPU_XDP_REDIRECT; }
// pushed: the list is at most 2 * n_max long, so its length is taken in 64 bits.
XSK_RD_FN uint32_t rp_pushed(uint32_t f_total, uint32_t n_rest, uint32_t capacity, uint32_t pool_n) {
    const uint64_t total = (uint64_t)f_total + n_rest, room = capacity - pool_n;
    return (uint32_t)(total < room ? total : room);
}

// Index j of [0, o_{n_ports}): the TX entry it carries, if any.  TX entry rd_slot(prod_port + k) = d_tx[j].
struct RpTx {
    bool on;
    uint32_t port, k;
};
XSK_RD_FN RpTx rp_tx_lane(const uint32_t* o, const uint32_t* t, uint32_t n_ports, uint32_t j) {
    const EpOwner ow = ep_owner(o, n_ports, j);
    RpTx x;
    x.port = ow.port;
    x.k = ow.on ? j - o[ow.port] : 0u;
    x.on = ow.on && x.k < t[ow.port];
    return x;
}

// Position L (< F_{n_ports} + |rest|) of the pool's list: d_free[idx], or entry idx of the compacted rest.  The port is
// found among the ascending F_0 .. F_{n_ports} with the search that finds a segment's owner; F_0 == 0, so every
// position below F_{n_ports} has one, and idx < o_port + f_port <= o_{port+1} <= n_max.
struct RpSrc {
    bool rest;
    uint32_t idx;
};
XSK_RD_FN RpSrc rp_pool_src(const uint32_t* F, const uint32_t* o, uint32_t n_ports, uint32_t L) {
    RpSrc s;
    s.rest = L >= F[n_ports];
    if (s.rest) {
        s.idx = L - F[n_ports];
    } else {
        const EpOwner ow = ep_owner(F, n_ports, L);
        s.idx = o[ow.port] + (L - F[ow.port]);
    }
    return s;
}

// ---- grids ----
// One workgroup up to kRpSmallMax.  Above: prepare and end's copy launch are rd_nwg(n_max) workgroups of kRdCopy lanes
// walking rd_copy_first() + k * rd_copy_stride(); the rest list's count and scatter launches are cp_nwg(n_max)
// workgroups of kCpFrames lanes, a lane per frame; the scan is one workgroup of kCpScanThreads, the publish one wave.

// ---- end's workspace above kRpSmallMax: the compacted rest (8 B each), the per-workgroup counts / offsets, the total
XSK_RD_FN size_t rp_end_rest(uint32_t) { return 0; }
XSK_RD_FN size_t rp_end_cells(uint32_t n_max) { return (size_t)n_max * 8u; }
XSK_RD_FN size_t rp_end_total(uint32_t n_max) { return rp_end_cells(n_max) + (size_t)cp_nwg(n_max) * 4u; }
XSK_RD_FN size_t rp_end_workspace_bytes(uint32_t n_max) {
    return n_max <= kRpSmallMax ? (size_t)0 : rd_align(rp_end_total(n_max) + 4u, 16u);
}

// ---- the workspace of xsk_gpu_rx_step_steer_dev(max_batch, n_ports): the plan, the rooms, the offsets, the counts,
// then the batch's descriptors, the steered list, the TX and free lists, verdicts, actions, ports and the workspaces of
// the steering call (steer_bytes), the egress (egress_bytes) and end; every offset a multiple of the alignment its array
// needs given a 16-B aligned base ----
struct RpLayout {
    size_t plan, room, off, counts, descs, out, tx, free_list, verdicts, actions, ports, steer, egress, end, bytes;
};
XSK_RD_FN RpLayout rp_layout(uint32_t max_batch, uint32_t n_ports, size_t steer_bytes, size_t egress_bytes) {
    RpLayout l;
    l.plan = 0;  // 32 B
    l.room = 32;
    l.off = l.room + (size_t)n_ports * 4u;
    l.counts = l.off + ((size_t)n_ports + 1u) * 4u;
    l.descs = rd_align(l.counts + (size_t)n_ports * 16u, 16u);
    l.out = l.descs + (size_t)max_batch * 16u;
    l.tx = l.out + (size_t)max_batch * 16u;
    l.free_list = l.tx + (size_t)max_batch * 16u;
    l.verdicts = l.free_list + (size_t)max_batch * 8u;
    l.actions = l.verdicts + (size_t)max_batch;
    l.ports = l.actions + (size_t)max_batch;
    l.steer = rd_align(l.ports + (size_t)max_batch, 4u);
    l.egress = rd_align(l.steer + steer_bytes, 4u);
    l.end = rd_align(l.egress + egress_bytes, 16u);
    l.bytes = rd_align(l.end + rp_end_workspace_bytes(max_batch), 16u);
    return l;
}

}  // namespace xskgpu

#endif  // XSK_RING_PORTS_H
