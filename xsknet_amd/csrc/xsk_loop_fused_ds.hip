// xsk_loop_fused_ds.hip — the dual-stack instance (XSK_GPU_OPT_IPV6) of xsk_gpu_rx_fused_loop_dev()'s kernel
// (xsk_loop_fused_body.h): the transform stage at RoundCfg<true, true, true>.  A file of its own as
// xsk_echo_ds.hip and xsk_echo_ds_indirect.hip are: the round body with the IPv6 phase needs the larger `#pragma unroll`
// budget (Makefile), which must not reach the other kernels.
#include "xsk_gpu_internal.h"
#include "xsk_loop_fused_body.h"

using namespace xskgpu;

namespace {

__global__ __launch_bounds__(kLfThreads, 1) void rx_loop_fused_ds_kernel(LoopFusedArgs A) {
    __shared__ LoopFusedLds L;
    loop_fused_body<RoundCfg<true, true, true>>(A, L);
}

}  // namespace

extern "C" void xsk_gpu__loop_fused_ds_launch(const void* args, void* stream) {
    const LoopFusedArgs& a = *(const LoopFusedArgs*)args;  // (this file's copy of the header's struct: one layout)
    rx_loop_fused_ds_kernel<<<dim3(1), dim3(kLfThreads), 0, (hipStream_t)stream>>>(a);
}
