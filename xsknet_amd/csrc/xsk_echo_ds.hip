// xsk_echo_ds.hip — the dual-stack transform kernel (XSK_GPU_OPT_IPV6): the wire-mode round kernel whose header phase
// also answers ICMPv6 echo requests (wire_v6_phase, xsk_echo_device.h; spec: include/xsk_gpu.h).  echo_launch() of
// xsk_echo.hip launches it, with every batch's geometry (xsk_echo_geometry.h), large or small, iff the option bit is set.
//
// A kernel and a file of its own: the IPv4-only kernels keep their instruction streams (tests/golden/kernel_isa.json),
// and this file is compiled with a larger `#pragma unroll` budget (Makefile) -- with the IPv6 phase the round body's
// loop over its two tiles no longer fits the default one.
#include "xsk_echo_device.h"
#include "xsk_gpu_internal.h"

using namespace xskgpu;

namespace {

// echo_round_kernel<true, SUBT> with V6 set: the same config family, RoundCfg<true, SUBT, true>.
template <bool SUBT>
__global__ __launch_bounds__(kThreads6, 1) void echo_ds_kernel(EchoArgs a, uint32_t tiles_per_wg) {
    using Cfg = RoundCfg<true, SUBT, true>;
    __shared__ Echo6Smem<Cfg::TPW> sm;
    const uint32_t tl = SUBT ? a.tile_live : (uint32_t)kTile;
    const uint32_t ntiles = (a.n + tl - 1) / tl;
    const uint32_t t_begin = blockIdx.x * tiles_per_wg;
    const uint32_t t_end = min(ntiles, t_begin + tiles_per_wg);
    echo6_body<Cfg>(a, t_begin, t_end, sm);
}

}  // namespace

extern "C" void xsk_gpu__echo_ds_launch(const void* args, uint32_t grid, uint32_t tiles_per_wg, int small, void* stream) {
    const EchoArgs& a = *(const EchoArgs*)args;  // (this file's copy of the header's struct: one layout)
    const hipStream_t s = (hipStream_t)stream;
    if (small) echo_ds_kernel<true><<<dim3(grid), dim3(kThreads6), 0, s>>>(a, tiles_per_wg);
    else echo_ds_kernel<false><<<dim3(grid), dim3(kThreads6), 0, s>>>(a, tiles_per_wg);
}
