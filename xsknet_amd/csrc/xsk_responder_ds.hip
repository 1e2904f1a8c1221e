// xsk_responder_ds.hip — the dual-stack instances (XSK_GPU_OPT_IPV6) of the responder kernels (xsk_responder.hip;
// DESIGN.md §9.15): the loop body's transform stage at RoundCfg<true, true, true>.  A file of its own as
// xsk_loop_fused_ds.hip and xsk_rx_queues_ds.hip are: the round body with the IPv6 phase needs the larger
// `#pragma unroll` budget (Makefile), which must not reach the other kernels.
#include "xsk_gpu_internal.h"
#include "xsk_responder_block.h"
#include "xsk_responder_body.h"

using namespace xskgpu;

namespace {

using ResponderQueuesLds = RsLds<LoopFusedLds, ResponderArgs>;  // (this file's copy of the headers' structs: one layout)
static_assert(sizeof(ResponderQueuesLds) <= 160u * 1024u, "the CU's LDS: the loop body's and the staged record");

__global__ __launch_bounds__(kLfThreads, 1) void responder_ds_kernel(ResponderArgs A) {
    __shared__ LoopFusedLds L;
    responder_body<RoundCfg<true, true, true>>(A, L);
}

__global__ __launch_bounds__(kLfThreads, 1) void responder_queues_ds_kernel(const uint8_t* block, uint32_t n_queues,
                                                                            uint32_t opts) {
    __shared__ ResponderQueuesLds M;
    if (!rs_stage(block, n_queues, opts, M.S)) return;  // workgroup-uniform, before the first store
    responder_body<RoundCfg<true, true, true>>(M.S.a, M.L);
}

}  // namespace

extern "C" void xsk_gpu__responder_ds_launch(const void* args, void* stream) {
    const ResponderArgs& a = *(const ResponderArgs*)args;
    responder_ds_kernel<<<dim3(1), dim3(kLfThreads), 0, (hipStream_t)stream>>>(a);
}

extern "C" void xsk_gpu__responder_queues_ds_launch(const void* d_block, uint32_t n_queues, uint32_t opts, void* stream) {
    responder_queues_ds_kernel<<<dim3(n_queues), dim3(kLfThreads), 0, (hipStream_t)stream>>>((const uint8_t*)d_block,
                                                                                             n_queues, opts);
}
