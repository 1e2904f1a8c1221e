// xsk_echo_ds_indirect.hip — the dual-stack instance (XSK_GPU_OPT_IPV6) of xsk_gpu_echo_dev_indirect()'s kernels:
// echo_ds_kernel<false>'s config, RoundCfg<true, false, true>, behind the prologue of xsk_echo_indirect.hip (the count
// read from device memory, the workgroup's share of it: xsk_echo_indirect.h).  A file of its own as xsk_echo_ds.hip is:
// the round body with the IPv6 phase needs the larger `#pragma unroll` budget (Makefile), which must not reach the
// other kernels.
#include "xsk_echo_device.h"
#include "xsk_echo_indirect.h"
#include "xsk_gpu_internal.h"

using namespace xskgpu;

namespace {

__global__ __launch_bounds__(kThreads6, 1) void echo_ds_indirect_kernel(EchoArgs a, const uint32_t* d_n, uint32_t i0,
                                                                        uint32_t len) {
    __shared__ Echo6Smem<kRefTPW> sm;
    a.n = ind_piece_n(uniform(*d_n), i0, len);
    uint32_t t_begin, t_end;
    ind_share(a.n, gridDim.x, blockIdx.x, &t_begin, &t_end);
    if (t_begin >= t_end) return;  // workgroup-uniform
    echo6_body<RoundCfg<true, false, true>>(a, t_begin, t_end, sm);
}

}  // namespace

extern "C" void xsk_gpu__echo_ds_indirect_launch(const void* args, const uint32_t* d_n, uint32_t i0, uint32_t len,
                                                 uint32_t grid, void* stream) {
    const EchoArgs& a = *(const EchoArgs*)args;  // (this file's copy of the header's struct: one layout)
    echo_ds_indirect_kernel<<<dim3(grid), dim3(kThreads6), 0, (hipStream_t)stream>>>(a, d_n, i0, len);
}
