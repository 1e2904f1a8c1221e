// xsk_compact.h — the count / scan / scatter core of every in-order compaction here: the ingress
// filter (xsk_classify.hip), the steering partition (xsk_steer.hip) and the two egress passes (xsk_egress.hip,
// xsk_egress_ports.hip).  All four count hits per workgroup of 256 frames with wave ballots, turn the counts into
// exclusive offsets in one 1024-thread workgroup, and scatter a lane per frame again: workgroup offset + the counts of
// the lower waves + the ballot bits below the lane.  What a hit is, what a scanned cell receives and where a frame goes
// stay with each user.
//
// The geometry and "which cells does scan thread t own" are host and device, so that the CPU replays (tests/c/
// compact_replay.h) walk the same runs as the kernels; the rest is device code.
#ifndef XSK_COMPACT_H
#define XSK_COMPACT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define XSK_CP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define XSK_CP_FN static inline
#endif

namespace xskgpu {

constexpr uint32_t kCpWave = 64;
constexpr uint32_t kCpFrames = 256;  // frames (and threads) per workgroup of the count and scatter stages
constexpr uint32_t kCpWaves = kCpFrames / kCpWave;
constexpr uint32_t kCpScanThreads = 1024;  // the scan's one workgroup

// Workgroups of the count and scatter stages over n frames.
XSK_CP_FN uint32_t cp_nwg(uint32_t n) { return n / kCpFrames + (n % kCpFrames ? 1u : 0u); }

// The scan: thread t owns the cells [t * per, min(t * per + per, nwg)), clamped in 64 bits so that the runs of the
// trailing threads are empty at nwg, whatever nwg is.
XSK_CP_FN uint32_t cp_scan_per(uint32_t nwg) { return nwg / kCpScanThreads + (nwg % kCpScanThreads ? 1u : 0u); }
XSK_CP_FN void cp_scan_run(uint32_t nwg, uint32_t t, uint32_t* b, uint32_t* e) {
    const uint64_t per = cp_scan_per(nwg), lo = t * per, hi = lo + per;
    *b = (uint32_t)(lo < nwg ? lo : nwg);
    *e = (uint32_t)(hi < nwg ? hi : nwg);
}

#ifdef __HIPCC__

__device__ __forceinline__ uint32_t cp_lane() { return threadIdx.x & (kCpWave - 1u); }
__device__ __forceinline__ uint32_t cp_wave() { return threadIdx.x / kCpWave; }
__device__ __forceinline__ uint32_t cp_below(unsigned long long m, uint32_t lane) {
    return (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}
__device__ __forceinline__ unsigned long long cp_wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kCpWave);
    return v;
}

// The wave's ballot of `hit`, its count into s_w[wave], and the barrier that publishes the workgroup's counts.
__device__ __forceinline__ unsigned long long cp_wg_ballot(bool hit, uint32_t* s_w) {
    const unsigned long long m = __ballot(hit);
    if (cp_lane() == 0) s_w[cp_wave()] = (uint32_t)__popcll(m);
    __syncthreads();
    return m;
}

// Stage 1 of a workgroup of kCpFrames threads: its hits into wg_count[blockIdx.x].  Thread 0 stores, and the cell is
// indexed here: with the cell's address computed by the caller egress_count_kernel is built in another order.
__device__ __forceinline__ void cp_wg_count(bool hit, uint32_t* s_w, uint32_t* wg_count) {
    cp_wg_ballot(hit, s_w);
    if (threadIdx.x == 0) wg_count[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
static_assert(kCpWaves == 4, "the sum above");

// Stage 3: `base` plus the counts of the waves below `wave`, behind cp_wg_ballot() in a workgroup of NW waves.  Selects,
// not a loop of `wave` trips: no lane diverges.
template <uint32_t NW>
__device__ __forceinline__ uint32_t cp_waves_below(const uint32_t* s_w, uint32_t wave, uint32_t base) {
    for (uint32_t k = 0; k < NW; ++k) base += k < wave ? s_w[k] : 0u;
    return base;
}

// Stage 2, one workgroup of kCpScanThreads with s[kCpScanThreads] in LDS: the exclusive scan of `cells` in place,
// this thread owning the run [b, e).  Cell j receives put(j, before, total); returns the total (workgroup-uniform).
template <class Put>
__device__ __forceinline__ uint32_t cp_scan_cells(uint32_t* cells, uint32_t b, uint32_t e, uint32_t* s, Put put) {
    const uint32_t t = threadIdx.x;
    uint32_t sum = 0;
    for (uint32_t j = b; j < e; ++j) sum += cells[j];
    s[t] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < kCpScanThreads; o <<= 1) {  // Hillis-Steele inclusive scan
        const uint32_t v = t >= o ? s[t - o] : 0u;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    uint32_t run = s[t] - sum;  // exclusive prefix of this run
    for (uint32_t j = b; j < e; ++j) {
        const uint32_t c = cells[j];
        cells[j] = put(j, run, s[kCpScanThreads - 1u]);
        run += c;
    }
    return s[kCpScanThreads - 1u];
}
// What a plain exclusive scan leaves in a cell.
__device__ __forceinline__ uint32_t cp_put_before(uint32_t, uint32_t before, uint32_t) { return before; }

#endif  // __HIPCC__

}  // namespace xskgpu

#endif  // XSK_COMPACT_H
