// xsk_echo_indirect.hip — xsk_gpu_echo_dev_indirect(): the transform with its frame count in device memory, and
// xsk_gpu_ingress_dev_opts(): the ingress filter and that transform as one stream-ordered unit (include/xsk_gpu.h;
// DESIGN.md §9.2).  The filter leaves its REDIRECT count in a device word; these kernels read it when they execute,
// so nothing between filter and transform comes back to the host and the pair can be captured in a graph.
//
// The kernels are echo6_body at RoundCfg<WIRE, false>, the config of the launched 64-frame-tile kernels of xsk_echo.hip,
// behind a prologue that reads the count and takes the workgroup's share of it (xsk_echo_indirect.h); the host sizes
// the launches with the direct launch's geometry (xsk_echo_geometry.h).  A file of its own: the kernels of xsk_echo.hip
// keep their instruction streams (tests/golden/kernel_isa.json).  The dual-stack instance is in
// xsk_echo_ds_indirect.hip (its own compiler flag, as xsk_echo_ds.hip).
#include <errno.h>

#include "xsk_echo_device.h"
#include "xsk_echo_indirect.h"
#include "xsk_gpu_internal.h"
#include "xsk_hip_util.h"

using namespace xskgpu;

extern "C" uint32_t xsk_gpu__num_cu(int device);  // xsk_echo.hip

namespace {

// The launched round kernel (WIRE, 64-frame tiles) for the piece [i0, i0 + len) of a batch of *d_n descriptors; a.descs,
// a.verdicts and a.recs point at the piece's first entry.  Every workgroup reads the count with one uniform load; one
// whose share is empty leaves as a whole, before the body's first barrier.
template <bool WIRE>
__global__ __launch_bounds__(kThreads6, 1) void echo_indirect_kernel(EchoArgs a, const uint32_t* d_n, uint32_t i0,
                                                                     uint32_t len) {
    __shared__ Echo6Smem<kRefTPW> sm;
    a.n = ind_piece_n(uniform(*d_n), i0, len);
    uint32_t t_begin, t_end;
    ind_share(a.n, gridDim.x, blockIdx.x, &t_begin, &t_end);
    if (t_begin >= t_end) return;  // workgroup-uniform
    echo6_body<RoundCfg<WIRE, false>>(a, t_begin, t_end, sm);
}

// The launches of a batch of *d_n <= n_max frames; `args` from echo_args_init() (the kernels take their n from *d_n).
int indirect_launch(EchoArgs args, const uint32_t* d_n, uint32_t n_max, struct xsk_gpu_stats* d_stats, void* stream) {
    if (d_stats) args.stats_direct = (unsigned long long*)&d_stats->rx_packets;  // device-scope atomics
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    const uint32_t ncu = xsk_gpu__num_cu(device);
    if (!ncu) return xsk_gpu__hip_fail(hipErrorInvalidDevice);
    const hipStream_t s = (hipStream_t)stream;
    uint32_t piece_tiles = 0;
    echo6_pieces(n_max, ncu, &piece_tiles);
    const uint32_t ntiles = ind_ntiles(n_max);
    for (uint32_t t0 = 0; t0 < ntiles; t0 += piece_tiles) {
        const uint32_t i0 = t0 * kTile;  // < n_max
        const uint64_t cap = (uint64_t)piece_tiles * kTile;
        const uint32_t len = (uint32_t)(n_max - i0 < cap ? n_max - i0 : cap);
        EchoArgs pa = args;
        pa.descs = args.descs + i0;
        pa.verdicts = args.verdicts ? args.verdicts + i0 : nullptr;
        pa.recs = args.recs ? args.recs + i0 : nullptr;
        const uint32_t pg = echo6_max_grid(len, ncu);
        if (args.opts & XSK_GPU_OPT_IPV6)
            xsk_gpu__echo_ds_indirect_launch(&pa, d_n, i0, len, pg, s);
        else if (args.opts == 0)
            echo_indirect_kernel<false><<<dim3(pg), dim3(kThreads6), 0, s>>>(pa, d_n, i0, len);
        else
            echo_indirect_kernel<true><<<dim3(pg), dim3(kThreads6), 0, s>>>(pa, d_n, i0, len);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" {

int xsk_gpu_echo_dev_indirect(void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs,
                              const uint32_t* d_n, uint32_t n_max, uint32_t opts, uint8_t* d_verdicts,
                              struct xsk_gpu_rec* d_recs, struct xsk_gpu_stats* d_stats, void* stream) {
    EchoArgs args;
    if (!d_n || ((uintptr_t)d_n & 3u) ||
        !echo_args_init(&args, d_umem, umem_size, d_descs, n_max, opts, d_verdicts, d_recs))
        return -EINVAL;
    if (n_max == 0) return 0;
    return indirect_launch(args, d_n, n_max, d_stats, stream);
}

int xsk_gpu_ingress_dev_opts(void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, uint32_t n,
                             uint32_t opts, int target_bound, uint8_t* d_actions, struct xsk_gpu_desc* d_out,
                             uint32_t* d_nout, uint8_t* d_verdicts, struct xsk_gpu_rec* d_recs,
                             struct xsk_gpu_stats* d_stats, void* d_workspace, void* stream) {
    // the filter's rules (xsk_classify.hip) with d_out and d_nout required, then the transform's over d_out
    if (!d_out || !d_nout || !d_actions || !d_workspace || ((uintptr_t)d_out & 15u) || ((uintptr_t)d_nout & 3u) ||
        !d_descs || ((uintptr_t)d_descs & 15u))
        return -EINVAL;
    EchoArgs args;  // (the transform's: over d_out, the count in *d_nout)
    if (!echo_args_init(&args, d_umem, umem_size, d_out, n, opts, d_verdicts, d_recs)) return -EINVAL;
    const int rc = xsk_gpu_classify_dev_opts(d_umem, umem_size, d_descs, n, opts, target_bound, d_actions, d_out, d_nout,
                                             d_workspace, stream);
    if (rc || n == 0) return rc;  // (n == 0: the filter has written *d_nout = 0)
    return indirect_launch(args, d_nout, n, d_stats, stream);
}

}  // extern "C"
