// xsk_egress.h — the arithmetic of xsk_gpu_egress_dev() (include/xsk_gpu.h): the slot rule that turns
// (is this frame a reply, how many replies lie below it, the TX ring's room) into "which list, which slot", the counts
// of a batch, and the grid, workgroup and workspace sizes of both paths.  Host and device: xsk_egress.hip's kernels and
// its host launch call these functions, and tests/c/test_egress_slots.cpp replays both paths with them on the CPU, into
// heap arrays of exactly n_tx and n_free entries under AddressSanitizer.
//
// With reply(i) = (verdict[i] == XSK_GPU_TX_REPLY) for i < n, R(i) = replies below i, R = R(n):
//   a reply with R(i) < room is submitted at tx[R(i)];
//   every other frame is freed at free[i - min(R(i), room)]  (min(R(i), room) frames below i were submitted).
// This is xsk_gpu__rx_emit()'s sequential loop (xsk_gpu_rx.c) with `sent` = min(R(i), room) at frame i.
#ifndef XSK_EGRESS_H
#define XSK_EGRESS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define XSK_EG_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define XSK_EG_FN static inline
#endif

namespace xskgpu {

constexpr uint32_t kEgSmallMax = 1024;  // == XSK_GPU_LOWLAT_MAX: one launch of one workgroup up to here
constexpr uint32_t kEgSmallThreads = 1024;
constexpr uint32_t kEgWave = 64;
constexpr uint32_t kEgFrames = 256;       // frames (and threads) per workgroup of the three-stage path
constexpr uint32_t kEgScanThreads = 1024; // the scan's one workgroup

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
// Workgroups of stages 1 and 3, sized from the bound the host knows.
XSK_EG_FN uint32_t eg_nwg(uint32_t n_max) { return n_max / kEgFrames + (n_max % kEgFrames ? 1u : 0u); }

// Frames of workgroup wg in a batch of n: clamp(n - wg * 256, 0, 256); 0 for a workgroup past n.
XSK_EG_FN uint32_t eg_wg_frames(uint32_t n, uint32_t wg) {
    const uint64_t b = (uint64_t)wg * kEgFrames;
    if (b >= n) return 0u;
    return n - b < kEgFrames ? (uint32_t)(n - b) : kEgFrames;
}

// The scan: thread t owns the counts [t * per, min(t * per + per, nwg)).
XSK_EG_FN uint32_t eg_scan_per(uint32_t nwg) { return nwg / kEgScanThreads + (nwg % kEgScanThreads ? 1u : 0u); }
XSK_EG_FN void eg_scan_run(uint32_t nwg, uint32_t t, uint32_t* b, uint32_t* e) {
    const uint64_t per = eg_scan_per(nwg), lo = t * per, hi = lo + per;
    *b = (uint32_t)(lo < nwg ? lo : nwg);
    *e = (uint32_t)(hi < nwg ? hi : nwg);
}

// Workspace: one uint32_t per workgroup (its reply count, then its exclusive offset); none on the small path.
XSK_EG_FN size_t eg_workspace_bytes(uint32_t n_max) {
    return n_max <= kEgSmallMax ? (size_t)0 : (size_t)eg_nwg(n_max) * sizeof(uint32_t);
}

}  // namespace xskgpu

#endif  // XSK_EGRESS_H
