// xsk_rearm_device.h — the device side of xsk_gpu_rearm_dev: TX_REPLY frames back to requests, four lanes per frame.
// Included by xsk_aux.hip; tools/rearm_variants.hip builds the other forms that were measured against this one
// (profiles/rearm/README.md) on rearm_chunk and rearm_bytes.
#pragma once

#include <stdint.h>

#include "../../include/xsk_gpu.h"
#include "xsk_echo_kernels.h"

namespace xskgpu {

// csum_replace2(csum, 0, 8) on the LE-loaded field: the inverse of the transform's (8 -> 0) patch
__device__ __forceinline__ uint32_t rearm_csum(uint32_t c) {
    uint32_t x = (~c) & 0xFFFFu;
    x = (x + 0xFFFFu) & 0xFFFFu;
    x += x < 0xFFFFu ? 1u : 0u;
    x = (x + 8u) & 0xFFFFu;
    x += x < 8u ? 1u : 0u;
    return (~x) & 0xFFFFu;
}

// A frame that is not 16-B aligned: byte by byte, only bytes [0, 38) touched.
__device__ __forceinline__ void rearm_bytes(uint8_t* p) {
    uint8_t t[6];
    for (int k = 0; k < 6; ++k) t[k] = p[k];
    for (int k = 0; k < 6; ++k) p[k] = p[6 + k];
    for (int k = 0; k < 6; ++k) p[6 + k] = t[k];
    for (int k = 0; k < 4; ++k) {
        const uint8_t x = p[26 + k];
        p[26 + k] = p[30 + k];
        p[30 + k] = x;
    }
    p[34] = 8;
    const uint32_t x = rearm_csum((uint32_t)p[36] | ((uint32_t)p[37] << 8));
    p[36] = (uint8_t)x;
    p[37] = (uint8_t)(x >> 8);
}

// DPP quad_perm: every lane reads the lane of its own quad (lanes 4f .. 4f + 3) that the control word names.
__device__ __forceinline__ uint32_t quad_mirror(uint32_t x) {  // quad_perm:[3,2,1,0]: lanes 1 and 2 trade places
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x1B, 0xF, 0xF, false);
}

// Chunk k of a frame's first sector, re-armed: each lane of a quad patches its own 16 bytes (branch-free).  Called by all four lanes of the quad: the address swap crosses chunks 1
// and 2, which trade dwords 7 and 8 by DPP.
__device__ __forceinline__ u32x4 rearm_chunk(u32x4 x, uint32_t k) {
    // dwords 6, 7 live in chunk 1 (.z, .w), dword 8 in chunk 2 (.x): lane 1 hands on dword 7, lane 2 dword 8
    const uint32_t got = quad_mirror(k == 1 ? x.w : x.x);
    // chunk 0, bytes 0-11: MACs swapped back (the same shuffle as the transform's, xsk_receive.c:148-151)
    const uint32_t n0 = (x.y >> 16) | (x.z << 16), n1 = (x.z >> 16) | (x.x << 16), n2 = (x.x >> 16) | (x.y << 16);
    // dwords 6, 7, 8 = bytes 24-35: IPv4 addresses swapped back (:153-155), type 0 -> 8 (byte 34)
    const uint32_t b6 = (x.z & 0xFFFFu) | (x.w & 0xFFFF0000u), b7 = (got & 0xFFFFu) | (x.z & 0xFFFF0000u);  // chunk 1
    const uint32_t c8 = (got & 0xFFFFu) | (x.x & 0xFF000000u) | (8u << 16);                                 // chunk 2
    const uint32_t c9 = (x.y & 0xFFFF0000u) | rearm_csum(x.y & 0xFFFFu);                                    // bytes 36-37
    u32x4 r;
    r.x = k == 0 ? n0 : k == 2 ? c8 : x.x;
    r.y = k == 0 ? n1 : k == 2 ? c9 : x.y;
    r.z = k == 0 ? n2 : k == 1 ? b6 : x.z;
    r.w = k == 1 ? b7 : x.w;
    return r;  // chunk 3 unchanged
}

constexpr uint32_t kRearmBlock = 256;                 // threads per workgroup: four waves
constexpr uint32_t kRearmBlockFrames = kRearmBlock / 4;  // frames per workgroup: four lanes per frame
// Four threads per frame: a launch takes at most 2^28 frames (2^30 threads), a grid's thread count must stay below 2^32.
constexpr uint32_t kRearmChunk = 1u << 28;

// Launches that n frames take, and the frames of launch c (which starts at frame c * kRearmChunk).
constexpr uint32_t rearm_launches(uint32_t n) { return (uint32_t)(((uint64_t)n + kRearmChunk - 1) / kRearmChunk); }
constexpr uint32_t rearm_launch_frames(uint32_t n, uint32_t c) {
    return (uint64_t)n - (uint64_t)c * kRearmChunk < kRearmChunk ? (uint32_t)((uint64_t)n - (uint64_t)c * kRearmChunk)
                                                                  : kRearmChunk;
}
constexpr bool rearm_launches_cover(uint32_t n) {  // the launches of n frames are whole but the last, and add up to n
    uint64_t sum = 0;
    for (uint32_t c = 0; c < rearm_launches(n); ++c) {
        const uint32_t m = rearm_launch_frames(n, c);
        if (m == 0 || m > kRearmChunk || (c + 1 < rearm_launches(n) && m != kRearmChunk)) return false;
        sum += m;
    }
    return sum == n;
}
static_assert(rearm_launches(XSK_GPU_MAX_BATCH) == 16 && rearm_launches_cover(XSK_GPU_MAX_BATCH), "largest batch");
static_assert(rearm_launches(0xF0000001u) == 16 && rearm_launch_frames(0xF0000001u, 15) == 1, "one frame past 15 chunks");
static_assert(rearm_launches(kRearmChunk) == 1 && rearm_launches(kRearmChunk + 1) == 2 && rearm_launches(1) == 1, "edges");
static_assert(rearm_launches_cover(1) && rearm_launches_cover(kRearmChunk) && rearm_launches_cover(kRearmChunk + 1) &&
              rearm_launches_cover(0xF0000000u) && rearm_launches_cover(0xF0000001u), "launches cover the batch");
static_assert((uint64_t)(kRearmChunk / kRearmBlockFrames) * kRearmBlock < (1ull << 32), "grid too large");

// Lane 4f + k of a wave owns 16-B chunk k of the wave's frame f, so a wave instruction moves 16 whole 64-B sectors;
// (n + kRearmBlockFrames - 1) / kRearmBlockFrames workgroups.  A quad is uniform in everything but k.
// A 16-B aligned frame (every frame the bench generates) is re-armed as its whole sector, chunk 3 stored back
// unchanged: no partial-sector writes (the frame owns [addr, addr + max(len, 64)), include/xsk_gpu.h).  Any other
// frame is done byte by byte by lane 0 of its quad.  A frame that is not TX_REPLY is neither loaded nor stored.
// The sector load is nontemporal: 1-4 us per 1 M frames ahead of the plain load at c3's, c4's and the packed layout
// in both measured sessions; at c5's layout, the one bench.py times this kernel at, 1.4 us ahead in one session and
// 0.9 us behind in the other, inside the runs' spread either way (profiles/rearm/README.md).
[[maybe_unused]] static __global__ __launch_bounds__(kRearmBlock) void rearm_quads_kernel(
    uint8_t* umem, const xsk_gpu_desc* descs, const uint8_t* verdicts, uint32_t n) {
    const uint32_t f0 = (blockIdx.x * (kRearmBlock / 64u) + uniform(threadIdx.x >> 6)) * 16u;
    if (f0 >= n) return;  // whole waves only: the DPP move of rearm_chunk reads neighbouring lanes
    const uint32_t lane = threadIdx.x & 63u, k = lane & 3u;
    const uint32_t f = f0 + (lane >> 2), fc = f < n ? f : n - 1;  // clamped: every lane loads, no branch
    const uint32_t t = verdicts[fc];
    const uint64_t a = descs[fc].addr;
    const bool tx = f < n && t == XSK_GPU_TX_REPLY, vec = tx && (a & 15u) == 0;
    u32x4* q = (u32x4*)(umem + a) + k;
    u32x4 x = u32x4{0u, 0u, 0u, 0u};
    if (vec) x = __builtin_nontemporal_load(q);
    x = rearm_chunk(x, k);
    if (vec) *q = x;
    else if (tx && k == 0) rearm_bytes((uint8_t*)q);  // k == 0: q is the frame's first byte
}

}  // namespace xskgpu
