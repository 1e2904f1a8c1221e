// xsk_egress.h — the arithmetic of xsk_gpu_egress_dev() (include/xsk_gpu.h): the slot rule that turns
// (is this frame a reply, how many replies lie below it, the TX ring's room) into "which list, which slot", the counts
// of a batch, and the workgroup and workspace sizes of both paths (the grid and the scan's runs are xsk_compact.h's).
// Host and device: xsk_egress.hip's kernels and its host launch call these functions, and tests/c/test_egress_slots.cpp
// replays both paths with them on the CPU, into heap arrays of exactly n_tx and n_free entries under AddressSanitizer.
// A device section at the end holds what xsk_egress.hip and xsk_egress_ports.hip both do with a frame.
//
// With reply(i) = (verdict[i] == XSK_GPU_TX_REPLY) for i < n, R(i) = replies below i, R = R(n):
//   a reply with R(i) < room is submitted at tx[R(i)];
//   every other frame is freed at free[i - min(R(i), room)]  (min(R(i), room) frames below i were submitted).
// This is xsk_gpu__rx_emit()'s sequential loop (xsk_gpu_rx.c) with `sent` = min(R(i), room) at frame i.
#ifndef XSK_EGRESS_H
#define XSK_EGRESS_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/xsk_gpu.h"
#include "xsk_compact.h"

#define XSK_EG_FN XSK_CP_FN

namespace xskgpu {

constexpr uint32_t kEgSmallMax = 1024;  // == XSK_GPU_LOWLAT_MAX: one launch of one workgroup up to here
constexpr uint32_t kEgSmallThreads = 1024;
constexpr uint32_t kEgWave = kCpWave;
constexpr uint32_t kEgFrames = kCpFrames;            // frames (and threads) per workgroup of the three-stage path
constexpr uint32_t kEgScanThreads = kCpScanThreads;  // the scan's one workgroup

struct EgCounts {  // == struct xsk_gpu_egress_counts
    uint32_t n, n_tx, n_tx_full, n_free;
};

struct EgSlot {
    bool tx;        // true: d_tx[slot], false: d_free[slot]
    uint32_t slot;
};

XSK_EG_FN uint32_t eg_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// n = d_n ? min(*d_n, n_max) : n_max and room = d_tx_room ? *d_tx_room : UINT32_MAX, from the words the kernel read
// (have == the pointer was given).
XSK_EG_FN uint32_t eg_count(bool have, uint32_t word, uint32_t n_max) { return have ? eg_min(word, n_max) : n_max; }
XSK_EG_FN uint32_t eg_room(bool have, uint32_t word) { return have ? word : 0xFFFFFFFFu; }

// Frame i (< n) with r_below = R(i) replies below it.
XSK_EG_FN EgSlot eg_slot(bool reply, uint32_t i, uint32_t r_below, uint32_t room) {
    EgSlot s;
    s.tx = reply && r_below < room;
    s.slot = s.tx ? r_below : i - eg_min(r_below, room);
    return s;
}

// A reply that found the ring full: freed, and taken back out of tx_packets / tx_bytes.
XSK_EG_FN bool eg_unsent(bool reply, uint32_t r_below, uint32_t room) { return reply && r_below >= room; }

XSK_EG_FN EgCounts eg_counts(uint32_t n, uint32_t r_total, uint32_t room) {
    EgCounts c;
    c.n = n;
    c.n_tx = eg_min(r_total, room);
    c.n_tx_full = r_total - c.n_tx;
    c.n_free = n - c.n_tx;
    return c;
}

// ---- the three-stage path (n_max > kEgSmallMax) ----
// Stages 1 and 3 run cp_nwg(n_max) workgroups, sized from the bound the host knows.
// Frames of workgroup wg in a batch of n: clamp(n - wg * 256, 0, 256); 0 for a workgroup past n.
XSK_EG_FN uint32_t eg_wg_frames(uint32_t n, uint32_t wg) {
    const uint64_t b = (uint64_t)wg * kEgFrames;
    if (b >= n) return 0u;
    return n - b < kEgFrames ? (uint32_t)(n - b) : kEgFrames;
}

// Workspace: one uint32_t per workgroup (its reply count, then its exclusive offset); none on the small path.
XSK_EG_FN size_t eg_workspace_bytes(uint32_t n_max) {
    return n_max <= kEgSmallMax ? (size_t)0 : (size_t)cp_nwg(n_max) * sizeof(uint32_t);
}

#ifdef __HIPCC__
// ---- what both egress files do with a frame (device) ----
// Frame i of the batch: the descriptor as one 16-B load, the verdict as a byte (any alignment; consecutive lanes read
// consecutive bytes).  Nothing outside [lo, hi) is read.
__device__ __forceinline__ bool eg_load_frame(const xsk_gpu_desc* __restrict__ descs,
                                              const uint8_t* __restrict__ verdicts, uint32_t i, uint32_t lo,
                                              uint32_t hi, uint4* d) {
    *d = make_uint4(0u, 0u, 0u, 0u);
    if (i < lo || i >= hi) return false;
    *d = reinterpret_cast<const uint4*>(descs)[i];
    return verdicts[i] == XSK_GPU_TX_REPLY;
}

// A frame to its list: { addr, len, 0 } as one 16-B store, or the address as one 8-B store.
__device__ __forceinline__ void eg_store_frame(const uint4& d, const EgSlot& s, xsk_gpu_desc* __restrict__ tx,
                                               uint64_t* __restrict__ free_list) {
    if (s.tx)
        reinterpret_cast<uint4*>(tx)[s.slot] = make_uint4(d.x, d.y, d.z, 0u);  // options = 0, as xsk_gpu__rx_emit()
    else
        reinterpret_cast<uint2*>(free_list)[s.slot] = make_uint2(d.x, d.y);
}

// *d_counts is only 4-B aligned: four word stores.
__device__ __forceinline__ void eg_store_counts(xsk_gpu_egress_counts* __restrict__ counts, const EgCounts& c) {
    counts->n = c.n;
    counts->n_tx = c.n_tx;
    counts->n_tx_full = c.n_tx_full;
    counts->n_free = c.n_free;
}
#endif  // __HIPCC__

}  // namespace xskgpu

#endif  // XSK_EGRESS_H
