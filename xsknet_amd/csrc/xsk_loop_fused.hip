// xsk_loop_fused.hip — xsk_gpu_rx_fused_loop_dev(): the body of the reference's handle_receive_packets() over all
// sockets as ONE launch of one workgroup, for bounds up to XSK_GPU_LOWLAT_MAX frames (include/xsk_gpu.h; DESIGN.md
// §9.11).  From the same state it leaves what xsk_gpu_rx_loop_dev() leaves; where that call is a chain of about ten
// dependent launches of one or four workgroups, this one runs the same stages behind workgroup barriers
// (xsk_loop_fused_body.h).  The reference-mode and wire-mode instances are here, the dual-stack one in
// xsk_loop_fused_ds.hip.  A file of its own: no existing translation unit's kernels change.
//
// One 1024-thread workgroup on one CU: latency bound at the reference's batch of 64 frames, and at 1024 long frames
// bound by what one CU streams (DESIGN.md §9.11 says up to which size the call is the one to use).  No MFMA.
#include <errno.h>

#include "xsk_gpu_internal.h"
#include "xsk_hip_util.h"
#include "xsk_loop_fused_body.h"

using namespace xskgpu;

namespace {

template <bool WIRE>
__global__ __launch_bounds__(kLfThreads, 1) void rx_loop_fused_kernel(LoopFusedArgs A) {
    __shared__ LoopFusedLds L;
    loop_fused_body<RoundCfg<WIRE, true>>(A, L);
}

// The packed form carries every ring the rules accept on this platform; a ring it cannot carry is refused with them.
bool packable(const xsk_gpu_ring_dev* r) { return !r || pk_packable((uint64_t)(uintptr_t)r->d_ring, r->size); }

// Every rule of xsk_gpu_rx_loop_dev() through its own function, and the two bounds of the one-workgroup form.
bool fused_ok(const void* d_umem, uint64_t umem_size, const xsk_gpu_ring_dev* rx, const xsk_gpu_ring_dev* fill,
              const xsk_gpu_ring_dev* tx, const xsk_gpu_ring_dev* stack, const xsk_gpu_pool_dev* pool, uint32_t max_batch,
              uint32_t opts, const xsk_gpu_steer_entry* d_table, uint32_t n_entries, uint32_t default_port,
              uint32_t n_ports, const uint64_t* d_bound, const void* d_port_counts, const void* d_stats,
              const void* d_port_stats, const void* d_res, const xsk_gpu_ring_dev* comp, uint32_t n_comp,
              uint32_t complete_max, const uint32_t* d_moved, const uint32_t* d_pushed, const void* d_workspace) {
    if (!loop_complete_ok(d_umem, umem_size, rx, fill, tx, stack, pool, max_batch, opts, d_table, n_entries, default_port,
                          n_ports, d_bound, d_port_counts, d_stats, d_port_stats, d_res, comp, n_comp, complete_max,
                          d_moved, d_pushed, d_workspace))
        return false;
    if (max_batch > kLfMax || (n_comp && complete_max > kLfMax)) return false;
    if (!packable(rx) || !packable(fill) || !packable(stack)) return false;
    for (uint32_t p = 0; p < n_ports; ++p)
        if (!packable(tx + p)) return false;
    for (uint32_t q = 0; q < n_comp; ++q)
        if (!packable(comp + q)) return false;
    return true;
}

// The one launch, behind the checks.
int fused_launch(const LoopFusedArgs& a, hipStream_t s) {
    if (a.opts & XSK_GPU_OPT_IPV6)
        xsk_gpu__loop_fused_ds_launch(&a, s);
    else if (a.opts == 0)
        rx_loop_fused_kernel<false><<<dim3(1), dim3(kLfThreads), 0, s>>>(a);
    else
        rx_loop_fused_kernel<true><<<dim3(1), dim3(kLfThreads), 0, s>>>(a);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int xsk_gpu_rx_fused_loop_dev(void* d_umem, uint64_t umem_size, const struct xsk_gpu_ring_dev* rx,
                              const struct xsk_gpu_ring_dev* fill, const struct xsk_gpu_ring_dev* tx,
                              const struct xsk_gpu_ring_dev* stack, const struct xsk_gpu_pool_dev* pool,
                              uint32_t max_batch, uint32_t opts, const struct xsk_gpu_steer_entry* d_table,
                              uint32_t n_entries, uint32_t default_port, uint32_t n_ports, const uint64_t* d_bound,
                              uint8_t* d_actions, uint8_t* d_ports, struct xsk_gpu_egress_counts* d_port_counts,
                              struct xsk_gpu_stats* d_stats, struct xsk_gpu_stats* d_port_stats,
                              struct xsk_gpu_rx_pass_result* d_res, const struct xsk_gpu_ring_dev* comp, uint32_t n_comp,
                              uint32_t complete_max, uint32_t* d_moved, uint32_t* d_pushed, void* d_workspace,
                              void* stream) {
    if (!fused_ok(d_umem, umem_size, rx, fill, tx, stack, pool, max_batch, opts, d_table, n_entries, default_port, n_ports,
                  d_bound, d_port_counts, d_stats, d_port_stats, d_res, comp, n_comp, complete_max, d_moved, d_pushed,
                  d_workspace))
        return -EINVAL;
    LoopFusedArgs a;
    for (uint32_t p = 0; p < kEpMaxPorts; ++p) a.tx[p] = lf_pack(p < n_ports ? tx + p : nullptr);
    for (uint32_t q = 0; q < kRcMaxRings; ++q) a.comp[q] = lf_pack(q < n_comp ? comp + q : nullptr);
    a.rx = lf_pack(rx);
    a.fill = lf_pack(fill);
    a.stack = lf_pack(stack);
    a.pool = pool_of(pool);
    a.umem = (uint8_t*)d_umem;
    a.umem_size = umem_size;
    a.table = d_table;
    a.d_bound = d_bound;
    a.d_actions = d_actions;
    a.d_ports = d_ports;
    a.d_port_counts = d_port_counts;
    a.d_stats = d_stats;
    a.d_port_stats = d_port_stats;
    a.d_res = d_res;
    a.d_moved = d_moved;
    a.d_pushed = d_pushed;
    a.ws = (uint8_t*)d_workspace;
    a.l = ps_layout(max_batch, n_ports, xsk_gpu_steer_workspace_size(max_batch, n_ports),
                    xsk_gpu_egress_ports_workspace_size(max_batch, n_ports));
    a.max_batch = max_batch;
    a.opts = opts;
    a.n_entries = n_entries;
    a.default_port = default_port;
    a.n_ports = n_ports;
    a.n_comp = n_comp;
    a.complete_max = complete_max;
    return fused_launch(a, (hipStream_t)stream);
}

}  // extern "C"
