// xsk_echo_indirect.hip — xsk_gpu_echo_dev_indirect(): the transform with its frame count in device memory, and
// xsk_gpu_ingress_dev_opts(): the ingress filter and that transform as one stream-ordered unit (include/xsk_gpu.h;
// DESIGN.md §9.2).  The filter leaves its REDIRECT count in a device word; these kernels read it when they execute,
// so nothing between filter and transform comes back to the host and the pair can be captured in a graph.
//
// The kernels are echo6_body (xsk_echo_device.h) at the switch values of the launched 64-frame-tile kernels of
// xsk_echo.hip, behind a prologue that reads the count and takes the workgroup's share of it (xsk_echo_indirect.h).
// A file of its own: the pinned kernels of xsk_echo.hip keep their instruction streams (tests/golden/kernel_isa.json).
// The dual-stack instance is in xsk_echo_ds_indirect.hip (its own compiler flag, as xsk_echo_ds.hip).
#include <errno.h>

#include "xsk_echo_device.h"
#include "xsk_echo_indirect.h"
#include "xsk_gpu_internal.h"
#include "xsk_hip_util.h"

using namespace xskgpu;

extern "C" uint32_t xsk_gpu__num_cu(int device);  // xsk_echo.hip

namespace {

static_assert(kIndRound == (uint32_t)kWaves6 * kRefTPW && kIndTile == (uint32_t)kTile, "xsk_echo_indirect.h");

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
    echo6_body<kRefTPW, 2, WIRE, false, false, false, true, kRefHeavy, kUR, true, true, kRefSlack, true>(a, t_begin,
                                                                                                          t_end, sm);
}

// The argument rules of xsk_gpu_echo_dev_indirect, with no device call.
int indirect_check(const void* d_umem, uint64_t umem_size, const void* d_descs, const void* d_n, uint32_t n_max,
                   uint32_t opts, const void* d_recs) {
    if (opts & ~XSK_GPU_OPT_MASK) return -EINVAL;
    if (!d_n || ((uintptr_t)d_n & 3u) || n_max > XSK_GPU_MAX_BATCH) return -EINVAL;
    if (!d_umem || !d_descs || ((uintptr_t)d_umem & 15u) || (umem_size & 15u) || ((uintptr_t)d_descs & 15u) ||
        ((uintptr_t)d_recs & 15u))
        return -EINVAL;
    if (umem_size >> 48) return -EINVAL;  // FrameMeta6 carries 48-bit UMEM offsets
    return 0;
}

int indirect_launch(void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, const uint32_t* d_n,
                    uint32_t n_max, uint32_t opts, uint8_t* d_verdicts, struct xsk_gpu_rec* d_recs,
                    struct xsk_gpu_stats* d_stats, void* stream) {
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    const uint32_t ncu = xsk_gpu__num_cu(device);
    if (!ncu) return xsk_gpu__hip_fail(hipErrorInvalidDevice);
    const hipStream_t s = (hipStream_t)stream;
    EchoArgs args;
    args.umem = (uint8_t*)d_umem;
    args.umem_size = umem_size;
    args.n = 0;  // (the kernel's, from *d_n)
    args.partials = nullptr;
    args.opts = opts;
    if (d_stats) args.stats_direct = (unsigned long long*)&d_stats->rx_packets;  // device-scope atomics
    uint32_t piece_tiles = 0;
    ind_pieces(n_max, ncu, &piece_tiles);
    const uint32_t ntiles = ind_ntiles(n_max);
    for (uint32_t t0 = 0; t0 < ntiles; t0 += piece_tiles) {
        const uint32_t i0 = t0 * kIndTile;  // < n_max
        const uint64_t cap = (uint64_t)piece_tiles * kIndTile;
        const uint32_t len = (uint32_t)(n_max - i0 < cap ? n_max - i0 : cap);
        EchoArgs pa = args;
        pa.descs = d_descs + i0;
        pa.verdicts = d_verdicts ? d_verdicts + i0 : nullptr;
        pa.recs = d_recs ? d_recs + i0 : nullptr;
        const uint32_t pg = ind_grid(len, ncu);
        if (opts & XSK_GPU_OPT_IPV6)
            xsk_gpu__echo_ds_indirect_launch(&pa, d_n, i0, len, pg, s);
        else if (opts == 0)
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
    const int rc = indirect_check(d_umem, umem_size, d_descs, d_n, n_max, opts, d_recs);
    if (rc) return rc;
    if (n_max == 0) return 0;
    return indirect_launch(d_umem, umem_size, d_descs, d_n, n_max, opts, d_verdicts, d_recs, d_stats, stream);
}

int xsk_gpu_ingress_dev_opts(void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, uint32_t n,
                             uint32_t opts, int target_bound, uint8_t* d_actions, struct xsk_gpu_desc* d_out,
                             uint32_t* d_nout, uint8_t* d_verdicts, struct xsk_gpu_rec* d_recs,
                             struct xsk_gpu_stats* d_stats, void* d_workspace, void* stream) {
    // the filter's rules (xsk_classify.hip) with d_out and d_nout required, then the transform's over d_out
    if (!d_out || !d_nout || !d_actions || !d_workspace || ((uintptr_t)d_out & 15u)) return -EINVAL;
    int rc = indirect_check(d_umem, umem_size, d_descs, d_nout, n, opts, d_recs);
    if (rc) return rc;
    rc = xsk_gpu_classify_dev_opts(d_umem, umem_size, d_descs, n, opts, target_bound, d_actions, d_out, d_nout,
                                   d_workspace, stream);
    if (rc || n == 0) return rc;  // (n == 0: the filter has written *d_nout = 0)
    return indirect_launch(d_umem, umem_size, d_out, d_nout, n, opts, d_verdicts, d_recs, d_stats, stream);
}

}  // extern "C"
