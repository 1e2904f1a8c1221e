// xsk_echo_indirect.h — the device prologue of xsk_gpu_echo_dev_indirect() (include/xsk_gpu.h): the
// transform whose frame count is a word in device memory, read when the kernel executes.  The host knows only the bound
// n_max, so it sizes the launches from n_max with the one launch geometry (xsk_echo_geometry.h) and every workgroup
// works out its own share from the count it reads, with the three functions here (host and device:
// tests/c/test_indirect_geometry.cpp checks that the shares partition the tiles and equal the direct launch's).
//
// The direct launch gives a batch of n frames, ntiles = ceil(n / 64) tiles, to g = min(ncu, ntiles) workgroups
// (echo6_max_grid) in contiguous shares of per = ceil(ntiles / g) tiles; workgroups whose share would start past the
// last tile are not launched.  The indirect launch starts G = echo6_max_grid(n_max) workgroups.  For n <= n_max,
// min(G, ntiles(n)) = min(ncu, ntiles(n)): workgroup b computes the direct launch's `per` and takes the direct launch's
// share [b * per, b * per + per), or nothing where the direct launch has no workgroup b.  Of the consecutive launches of
// a long share (echo6_pieces at n_max), piece p owns the descriptors [i0, i0 + len) and serves ind_piece_n(n, i0, len).
#ifndef XSK_ECHO_INDIRECT_H
#define XSK_ECHO_INDIRECT_H

#include <stdint.h>

#include "xsk_echo_geometry.h"

#ifdef __HIPCC__
#define XSK_IND_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define XSK_IND_FN static inline
#endif

namespace xskgpu {

XSK_IND_FN uint32_t ind_ntiles(uint32_t n) { return n / kTile + (n % kTile ? 1u : 0u); }

// Frames of piece [i0, i0 + len) in a batch of n: clamp(n - i0, 0, len).
XSK_IND_FN uint32_t ind_piece_n(uint32_t n, uint32_t i0, uint32_t len) {
    if (n <= i0) return 0u;
    return n - i0 < len ? n - i0 : len;
}

// The tiles [*t_begin, *t_end) of workgroup `wg` of a launch of `launched` workgroups over n frames; empty for n == 0
// and for a workgroup the direct launch of n would not have.
XSK_IND_FN void ind_share(uint32_t n, uint32_t launched, uint32_t wg, uint32_t* t_begin, uint32_t* t_end) {
    const uint32_t ntiles = ind_ntiles(n);
    uint32_t g = launched < ntiles ? launched : ntiles;
    if (g < 1u) g = 1u;
    const uint32_t per = (ntiles + g - 1u) / g;
    const uint64_t b = (uint64_t)wg * per, e = b + per;
    *t_begin = (uint32_t)(b < ntiles ? b : ntiles);
    *t_end = (uint32_t)(e < ntiles ? e : ntiles);
}

}  // namespace xskgpu

#endif  // XSK_ECHO_INDIRECT_H
