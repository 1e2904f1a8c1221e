// The forms of the quad re-arm that were measured against each other (profiles/rearm/README.md), behind one entry
// point for tools/rearm_bench.py, on rearm_chunk and rearm_bytes of xsknet_amd/csrc/xsk_rearm_device.h.  The shipped
// library holds the form that won: variant 1 at one frame per lane.  variant = nt | bcast << 1 | fpl_index << 2 | stride << 4:
//   nt        nontemporal frame loads
//   bcast     verdict and descriptor loaded by lane 0 of a quad and broadcast by DPP (else by all four lanes)
//   fpl_index 0, 1, 2: one, two, four frames per lane per pass
//   stride    a fixed grid of 8 workgroups per CU, grid-stride (else one pass per wave)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../xsknet_amd/csrc/xsk_rearm_device.h"

using namespace xskgpu;

namespace {

constexpr uint32_t kVarBlock = 256;  // threads per workgroup: four waves

__device__ __forceinline__ uint32_t quad_lane0(uint32_t x) {  // quad_perm:[0,0,0,0]
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x00, 0xF, 0xF, false);
}

// One pass of one wave over the 16 * FPL frames from f0 on: lane 4f + k owns 16-B chunk k of frame f0 + 16 u + f
// (u < FPL), so a wave instruction moves 16 whole 64-B sectors.  Called by all 64 lanes (the DPP moves read
// neighbouring lanes); a quad is uniform in everything but k.
//   NT    : the frame loads are nontemporal
//   BCAST : verdict and descriptor are loaded by lane 0 of the quad and handed on by DPP, else by all four lanes
// A 16-B aligned frame (every frame the bench generates) is re-armed as its whole sector, chunk 3 stored back
// unchanged: no partial-sector writes (the frame owns [addr, addr + max(len, 64)), include/xsk_gpu.h).  Any other
// frame is done byte by byte by lane 0 of its quad.  A frame that is not TX_REPLY is neither loaded nor stored.
// When every frame of the pass is an aligned TX_REPLY (a bench batch but for its last wave), all FPL loads of a lane
// are issued before the first store; otherwise the frames go one after the other, each under its own conditions.
template <int FPL, bool NT, bool BCAST>
__device__ __forceinline__ void rearm_var(uint8_t* umem, const xsk_gpu_desc* descs, const uint8_t* verdicts, uint32_t n,
                                            uint32_t f0, uint32_t lane) {
    const uint32_t k = lane & 3u;
    uint32_t tx[FPL], lo[FPL], hi[FPL];
#pragma unroll
    for (int u = 0; u < FPL; ++u) tx[u] = lo[u] = hi[u] = 0;
    if (!BCAST || k == 0) {
#pragma unroll
        for (int u = 0; u < FPL; ++u) {
            const uint32_t f = f0 + 16u * (uint32_t)u + (lane >> 2), fc = f < n ? f : n - 1;  // clamped: no branch
            const uint32_t t = verdicts[fc];
            const uint64_t a = descs[fc].addr;
            tx[u] = f < n && t == XSK_GPU_TX_REPLY ? 1u : 0u;
            lo[u] = (uint32_t)a;
            hi[u] = (uint32_t)(a >> 32);
        }
    }
    u32x4* q[FPL];
    bool every = true;
#pragma unroll
    for (int u = 0; u < FPL; ++u) {
        if (BCAST) {
            tx[u] = quad_lane0(tx[u]);
            lo[u] = quad_lane0(lo[u]);
            hi[u] = quad_lane0(hi[u]);
        }
        q[u] = (u32x4*)(umem + ((uint64_t)hi[u] << 32 | lo[u])) + k;
        every = every && tx[u] && (lo[u] & 15u) == 0;
    }
    if (__all(every)) {
        u32x4 v[FPL];
#pragma unroll
        for (int u = 0; u < FPL; ++u) v[u] = NT ? __builtin_nontemporal_load(q[u]) : *q[u];
#pragma unroll
        for (int u = 0; u < FPL; ++u) *q[u] = rearm_chunk(v[u], k);
        return;
    }
#pragma unroll
    for (int u = 0; u < FPL; ++u) {
        const bool vec = tx[u] && (lo[u] & 15u) == 0;
        u32x4 x = u32x4{0u, 0u, 0u, 0u};
        if (vec) x = NT ? __builtin_nontemporal_load(q[u]) : *q[u];
        x = rearm_chunk(x, k);
        if (vec) *q[u] = x;
        else if (tx[u] && k == 0) rearm_bytes((uint8_t*)q[u]);  // k == 0: q[u] is the frame's first byte
    }
}


// frames one workgroup covers per pass
template <int FPL>
constexpr uint32_t var_block_frames() {
    return kVarBlock / 4u * (uint32_t)FPL;
}

// One pass per wave: (n + var_block_frames<FPL>() - 1) / var_block_frames<FPL>() workgroups.
template <int FPL, bool NT, bool BCAST>
__global__ __launch_bounds__(kVarBlock) void rearm_var_kernel(uint8_t* umem, const xsk_gpu_desc* descs,
                                                                  const uint8_t* verdicts, uint32_t n) {
    const uint32_t f0 = (blockIdx.x * (kVarBlock / 64u) + uniform(threadIdx.x >> 6)) * (16u * (uint32_t)FPL);
    if (f0 >= n) return;
    rearm_var<FPL, NT, BCAST>(umem, descs, verdicts, n, f0, threadIdx.x & 63u);
}

// The same over a grid of any size: wave w of the grid takes passes w, w + waves, ...  (n < 2^31: f0 cannot wrap)
template <int FPL, bool NT, bool BCAST>
__global__ __launch_bounds__(kVarBlock) void rearm_var_stride_kernel(uint8_t* umem, const xsk_gpu_desc* descs,
                                                                         const uint8_t* verdicts, uint32_t n) {
    const uint32_t per = 16u * (uint32_t)FPL, step = gridDim.x * (kVarBlock / 64u) * per;
    for (uint32_t f0 = (blockIdx.x * (kVarBlock / 64u) + uniform(threadIdx.x >> 6)) * per; f0 < n; f0 += step)
        rearm_var<FPL, NT, BCAST>(umem, descs, verdicts, n, f0, threadIdx.x & 63u);
}


template <int FPL, bool NT, bool BCAST>
int run(bool stride, int cus, uint8_t* umem, const xsk_gpu_desc* descs, const uint8_t* verd, uint32_t n, hipStream_t s) {
    constexpr uint32_t per = var_block_frames<FPL>();
    const uint32_t need = (n + per - 1) / per, fixed = (uint32_t)cus * 8u;
    if (stride)
        hipLaunchKernelGGL((rearm_var_stride_kernel<FPL, NT, BCAST>), dim3(need < fixed ? need : fixed), dim3(kVarBlock),
                           0, s, umem, descs, verd, n);
    else
        hipLaunchKernelGGL((rearm_var_kernel<FPL, NT, BCAST>), dim3(need), dim3(kVarBlock), 0, s, umem, descs, verd, n);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <int FPL>
int run_fpl(int v, int cus, uint8_t* u, const xsk_gpu_desc* d, const uint8_t* vd, uint32_t n, hipStream_t s) {
    const bool st = (v >> 4) & 1;
    switch (v & 3) {
        case 0: return run<FPL, false, false>(st, cus, u, d, vd, n, s);
        case 1: return run<FPL, true, false>(st, cus, u, d, vd, n, s);
        case 2: return run<FPL, false, true>(st, cus, u, d, vd, n, s);
        default: return run<FPL, true, true>(st, cus, u, d, vd, n, s);
    }
}

}  // namespace

extern "C" int rearm_variant_run(int variant, void* umem, const void* descs, const void* verd, uint32_t n, void* stream) {
    if (variant < 0 || variant >= 32 || ((variant >> 2) & 3) == 3 || n == 0 || n > (1u << 28)) return -1;
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            return -3;
    }
    uint8_t* u = (uint8_t*)umem;
    const xsk_gpu_desc* d = (const xsk_gpu_desc*)descs;
    const uint8_t* vd = (const uint8_t*)verd;
    const hipStream_t s = (hipStream_t)stream;
    switch ((variant >> 2) & 3) {
        case 0: return run_fpl<1>(variant, cus, u, d, vd, n, s);
        case 1: return run_fpl<2>(variant, cus, u, d, vd, n, s);
        default: return run_fpl<4>(variant, cus, u, d, vd, n, s);
    }
}
