// xsk_rx_queues_ds.hip — the dual-stack instance (XSK_GPU_OPT_IPV6) of xsk_gpu_rx_queues_dev()'s kernel
// (xsk_rx_queues.hip): the loop body's transform stage at RoundCfg<true, true, true>.  A file of its
// own as xsk_loop_fused_ds.hip is: the round body with the IPv6 phase needs the larger `#pragma unroll` budget
// (Makefile), which must not reach the other kernels.
#include "xsk_gpu_internal.h"
#include "xsk_loop_fused_body.h"
#include "xsk_rx_queues.h"

using namespace xskgpu;

namespace {

using QueuesLds = RqLds<LoopFusedLds, LoopFusedArgs>;  // (this file's copy of the headers' structs: one layout)
static_assert(sizeof(QueuesLds) <= 160u * 1024u, "the CU's LDS: the loop body's and the staged record");

__global__ __launch_bounds__(kLfThreads, 1) void rx_queues_ds_kernel(const uint8_t* block, uint32_t n_queues,
                                                                     uint32_t opts) {
    __shared__ QueuesLds M;
    if (!rq_stage(block, n_queues, opts, M.S)) return;  // workgroup-uniform, before the first store
    loop_fused_body<RoundCfg<true, true, true>>(M.S.a, M.L);
}

}  // namespace

extern "C" void xsk_gpu__rx_queues_ds_launch(const void* d_block, uint32_t n_queues, uint32_t opts, void* stream) {
    rx_queues_ds_kernel<<<dim3(n_queues), dim3(kLfThreads), 0, (hipStream_t)stream>>>((const uint8_t*)d_block, n_queues,
                                                                                       opts);
}
