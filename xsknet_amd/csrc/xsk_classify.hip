// xsk_classify.hip — the XDP ingress filter of the reference as a device pass over a batch:
// xdp_sock_prog() (src/kern/inner_xdp.c:26-61; phy_xdp.c:39-81 makes the same tests) decides per frame
// DROP / PASS / REDIRECT, and the REDIRECT frames are compacted in order into a descriptor list that
// feeds xsk_gpu_echo_dev() ("XDP pre-filter parity").
//
// Three launches, the compaction core of xsk_compact.h, all HBM/latency bound (no MFMA):
//   1. classify: lane per frame — descriptor, bounds check, bytes 12-13 and 23 of the frame, action;
//      per-workgroup count of REDIRECT frames (wave ballots);
//   2. scan: one 1024-thread workgroup turns the per-workgroup counts into exclusive offsets and the
//      total;
//   3. scatter: lane per frame again — wave ballot prefix + workgroup offset -> output slot.
//
// xsk_gpu_classify_dev_opts() with nonzero options replaces launch 1 by classify_wire_kernel, the VLAN- and
// IPv6-aware filter specified in include/xsk_gpu.h; launches 2 and 3 are the same.
#include <errno.h>

#include "../../include/xsk_gpu.h"
#include "xsk_classify_wire.h"
#include "xsk_compact.h"
#include "xsk_echo_kernels.h"
#include "xsk_hip_util.h"

using namespace xskgpu;

namespace {

constexpr uint32_t kMaxLen = XSK_GPU_MAX_LEN;

__device__ __forceinline__ uint32_t classify_one(const uint8_t* umem, uint64_t umem_size, const xsk_gpu_desc& d,
                                                 int bound) {
    const uint64_t a = d.addr;
    const uint32_t len = d.len;
    const uint32_t need = len < 34 ? (len < 14 ? 0u : 14u) : 34u;
    if (len > kMaxLen || a > umem_size || need > umem_size - a) return XSK_GPU_XDP_DROP;  // build-added
    if (len < 14) return XSK_GPU_XDP_DROP;                                               // :35-36
    // the three bytes the program reads, loaded together (one round trip; byte 23 only when the IPv4
    // header is inside the frame, so nothing past the frame is read)
    const uint8_t* p = umem + a;
    const uint32_t e0 = p[12], e1 = p[13];
    const uint32_t pr = len >= 34 ? (uint32_t)p[23] : 0u;
    if (e0 != 0x08 || e1 != 0x00) return XSK_GPU_XDP_PASS;                              // :38-39
    if (len < 34) return XSK_GPU_XDP_DROP;                                               // :41-42
    if (pr != 1) return XSK_GPU_XDP_PASS;                                                // :44-45
    return bound ? XSK_GPU_XDP_REDIRECT : XSK_GPU_XDP_DROP;                              // :57-60
}

__global__ __launch_bounds__(kCpFrames) void classify_kernel(const uint8_t* umem, uint64_t umem_size,
                                                             const xsk_gpu_desc* descs, uint32_t n, int bound,
                                                             uint8_t* actions, uint32_t* wg_count) {
    __shared__ uint32_t s_w[kCpWaves];
    const uint32_t i = blockIdx.x * kCpFrames + threadIdx.x;
    uint32_t act = 0;
    if (i < n) {
        act = classify_one(umem, umem_size, descs[i], bound);
        actions[i] = (uint8_t)act;
    }
    cp_wg_count(act == XSK_GPU_XDP_REDIRECT, s_w, wg_count);
}

// First stage for nonzero options: classify_wire_one() of xsk_classify_wire.h per lane, the same counts as above.
__global__ __launch_bounds__(kCpFrames) void classify_wire_kernel(const uint8_t* umem, uint64_t umem_size,
                                                                  const xsk_gpu_desc* descs, uint32_t n, uint32_t opts,
                                                                  int bound, uint8_t* actions, uint32_t* wg_count) {
    __shared__ uint32_t s_w[kCpWaves];
    const uint32_t i = blockIdx.x * kCpFrames + threadIdx.x;
    uint32_t act = 0;
    if (i < n) {
        act = classify_wire_one(umem, umem_size, descs[i], opts, bound);
        actions[i] = (uint8_t)act;
    }
    cp_wg_count(act == XSK_GPU_XDP_REDIRECT, s_w, wg_count);
}

// Exclusive scan of nwg counts in place (one workgroup of 1024): thread t owns a contiguous run.
__global__ __launch_bounds__(kCpScanThreads) void scan_kernel(uint32_t* wg_count, uint32_t nwg, uint32_t* d_total) {
    __shared__ uint32_t s[kCpScanThreads];
    uint32_t b, e;
    cp_scan_run(nwg, threadIdx.x, &b, &e);
    const uint32_t total = cp_scan_cells(wg_count, b, e, s, cp_put_before);
    if (threadIdx.x == kCpScanThreads - 1u) *d_total = total;
}

__global__ __launch_bounds__(kCpFrames) void scatter_kernel(const xsk_gpu_desc* descs, uint32_t n,
                                                            const uint8_t* actions, const uint32_t* wg_off,
                                                            xsk_gpu_desc* out) {
    __shared__ uint32_t s_w[kCpWaves];
    const uint32_t i = blockIdx.x * kCpFrames + threadIdx.x;
    const bool r = i < n && actions[i] == XSK_GPU_XDP_REDIRECT;
    const uint32_t lane = cp_lane(), w = cp_wave();
    const uint64_t m = cp_wg_ballot(r, s_w);
    uint32_t base = wg_off[blockIdx.x];
    for (uint32_t k = 0; k < w; ++k) base += s_w[k];  // this kernel's own form: cp_waves_below's selects build other code
    if (r) out[base + cp_below(m, lane)] = descs[i];
}

}  // namespace

extern "C" {

size_t xsk_gpu_classify_workspace_size(uint32_t n) { return ((size_t)cp_nwg(n) + 1) * sizeof(uint32_t); }

// opts == 0: the reference's filter (classify_kernel); nonzero: classify_wire_kernel.  Same scan and scatter.
static int classify_launch(const void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, uint32_t n,
                           uint32_t opts, int target_bound, uint8_t* d_actions, struct xsk_gpu_desc* d_out,
                           uint32_t* d_nout, void* d_workspace, void* stream) {
    if (n == 0) {
        if (d_nout) HIP_TRY(hipMemsetAsync(d_nout, 0, sizeof(uint32_t), (hipStream_t)stream));
        return 0;
    }
    if (!d_umem || !d_descs || !d_actions || !d_workspace || (d_out && !d_nout) || ((uintptr_t)d_descs & 15u) ||
        ((uintptr_t)d_out & 15u) || n > XSK_GPU_MAX_BATCH)
        return -EINVAL;
    const uint32_t nwg = cp_nwg(n);
    hipStream_t s = (hipStream_t)stream;
    uint32_t* wg = (uint32_t*)d_workspace;
    if (opts)
        hipLaunchKernelGGL(classify_wire_kernel, dim3(nwg), dim3(kCpFrames), 0, s, (const uint8_t*)d_umem, umem_size,
                           d_descs, n, opts, target_bound, d_actions, wg);
    else
        hipLaunchKernelGGL(classify_kernel, dim3(nwg), dim3(kCpFrames), 0, s, (const uint8_t*)d_umem, umem_size,
                           d_descs, n, target_bound, d_actions, wg);
    HIP_TRY(hipGetLastError());
    if (d_out) {
        hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kCpScanThreads), 0, s, wg, nwg, d_nout);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(scatter_kernel, dim3(nwg), dim3(kCpFrames), 0, s, d_descs, n, (const uint8_t*)d_actions,
                           (const uint32_t*)wg, d_out);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int xsk_gpu_classify_dev(const void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, uint32_t n,
                         int target_bound, uint8_t* d_actions, struct xsk_gpu_desc* d_out, uint32_t* d_nout,
                         void* d_workspace, void* stream) {
    return classify_launch(d_umem, umem_size, d_descs, n, 0, target_bound, d_actions, d_out, d_nout, d_workspace,
                           stream);
}

int xsk_gpu_classify_dev_opts(const void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, uint32_t n,
                              uint32_t opts, int target_bound, uint8_t* d_actions, struct xsk_gpu_desc* d_out,
                              uint32_t* d_nout, void* d_workspace, void* stream) {
    if (opts & ~XSK_GPU_OPT_MASK) return -EINVAL;
    return classify_launch(d_umem, umem_size, d_descs, n, opts, target_bound, d_actions, d_out, d_nout, d_workspace,
                           stream);
}

}  // extern "C"
