// xsk_unreach_device.h — one wave rewrites one request into its port-unreachable error (include/xsk_gpu.h,
// "Port-unreachable responder").  Device only: the three phases of xsk_unreach.h's lane pieces with the
// wave's reduction and one shuffle between them.  Kept apart from the kernels so that a fused responder can call it.
#ifndef XSK_UNREACH_DEVICE_H
#define XSK_UNREACH_DEVICE_H

#include <hip/hip_runtime.h>

#include "xsk_compact.h"
#include "xsk_unreach.h"

namespace xskgpu {
namespace {

static_assert(kUrWave == kCpWave, "a lane of the rewrite is a lane of the wave");

// Every lane of the wave calls it with the same p and v (v.verdict UNREACH4 or UNREACH6).  The quote is read whole into
// registers (at most 20 bytes a lane), summed across the wave, and only then stored 28 or 48 bytes further on: the sum
// needs every lane's loads back, and the fence keeps every store behind it in program order, so the overlapping move
// needs no barrier and no second buffer.
__device__ __forceinline__ void ur_wave_rewrite(uint8_t* p, const UrVerdict& v) {
    const uint32_t lane = cp_lane();
    const UrLane r = ur_lane_load(p, v.l3, v.q, lane);
    const unsigned long long total = cp_wave_sum(ur_lane_part(r, v.verdict, lane));
    const uint32_t from = ur_hdr_swap(v.verdict, lane);
    const uint32_t swapped = (uint32_t)__shfl((int)r.b[0], (int)(from & (kUrWave - 1u)), kUrWave);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (no instruction: an order for the compiler)
    ur_lane_store(p, r, v, lane, total, swapped);
}

}  // namespace
}  // namespace xskgpu

#endif  // XSK_UNREACH_DEVICE_H
