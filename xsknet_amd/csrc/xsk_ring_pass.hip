// xsk_ring_pass.hip — the steered RX step with a stack ring: xsk_gpu_rx_pass_end_dev() (xsk_gpu_rx_ports_end_dev()'s
// rule with the frames the filter passes to the kernel stack put on a descriptor ring of their own, as many as it has
// room for, and only the others freed) and xsk_gpu_rx_pass_step_dev() (xsk_gpu_rx_begin_dev(),
// xsk_gpu_rx_prepare_ports_dev(), xsk_gpu_ingress_steer_dev(), xsk_gpu_egress_ports_dev(), end on one stream).
// include/xsk_gpu.h; DESIGN.md §9.9.  Every index and count is a word in device memory, read when the kernels execute;
// the 64 TX ring structs and the stack ring's travel by value in the kernel arguments.
//
// Two paths, the arithmetic of both in xsk_ring_pass.h over xsk_ring_ports.h (host and device); what a workgroup
// decides from the words, the copy and the publish are those of xsk_gpu_rx_ports_end_dev() (xsk_ring_ports_device.h):
//   bound <= 1024: one launch of one 1024-thread workgroup -- decide; two ballots per wave rank every frame among the
//                  frames not redirected and among the PASS frames; a PASS frame the stack ring takes goes from d_descs
//                  to its ring entry as one 16-B load and store, every other frame not redirected into the rest list in
//                  LDS; a lane per entry copies, a fence and a barrier, lane p stores port p's producer word, lane 0
//                  the pool's count, the RX consumer word and *d_res, the last lane the stack ring's producer word;
//   larger:        kernel boundaries in place of the barriers -- count, scan and scatter of the compaction core over two
//                  count rows (not redirected, PASS); the scatter leaves the rest list in the workspace and the taken
//                  PASS descriptors on the stack ring, every workgroup deciding the stack ring's share from the ring's
//                  two index words and the two totals; then the copy grid and a one-wave publish launch, the only
//                  launch that stores an index word.
// No launch stores an index word for entries another launch stores, no atomic hands out a slot, no workgroup waits on
// another, nothing is polled.  Index words are read through the vector path (load_word).  Latency bound: 16 B or 8 B in
// and out per entry, no frame byte touched, no MFMA.
#include <errno.h>
#include <stddef.h>

#include "../../include/xsk_gpu.h"
#include "xsk_hip_util.h"
#include "xsk_ring_pass.h"
#include "xsk_ring_pass_device.h"
#include "xsk_ring_ports_device.h"

using namespace xskgpu;

static_assert(kPsSmallMax == XSK_GPU_LOWLAT_MAX, "the one-launch path serves the RX loop's sizes");
static_assert(sizeof(xsk_gpu_rx_pass_result) == 32 && sizeof(xsk_gpu_rx_pass_result) == sizeof(xsk_gpu_rx_steer_result),
              "result layout");
static_assert(offsetof(xsk_gpu_rx_pass_result, freed) == offsetof(xsk_gpu_rx_steer_result, freed) &&
                  offsetof(xsk_gpu_rx_pass_result, passed) == offsetof(xsk_gpu_rx_steer_result, reserved),
              "the first six words are xsk_gpu_rx_steer_result's: end_publish() writes them");
static_assert(sizeof(Rings) + 2 * sizeof(Ring) + sizeof(Pool) + 12 * 8 <= 4096, "the kernel arguments");

namespace {

// (StackWords, PassPlan, pass_place, pass_publish and the one-workgroup form, rx_pass_end_small_body:
// xsk_ring_pass_device.h)

// (The fused loop kernel runs the same statements as rx_pass_end_small_body(), xsk_ring_pass_device.h; called from here
// the compiler emitted this kernel's 1009 instructions with two registers exchanged, so the kernel keeps its own text.)
__global__ __launch_bounds__(kPsSmallThreads) void rx_pass_end_small_kernel(
    Ring rx, Rings tx, uint32_t n_ports, Ring stack, Pool pool, const xsk_gpu_rx_plan* d_plan, const xsk_gpu_desc* descs,
    const uint8_t* actions, const uint32_t* d_off, const xsk_gpu_desc* d_tx, const uint64_t* d_free,
    const xsk_gpu_egress_counts* counts, uint32_t n_max, xsk_gpu_rx_pass_result* d_res) {
    __shared__ EndLds s;
    __shared__ uint32_t s_wn[kPsSmallWaves], s_wq[kPsSmallWaves];
    __shared__ uint64_t s_rest[kPsSmallMax];
    const uint32_t i = threadIdx.x;
    const StackWords w = stack_words(stack);
    end_decide(tx, n_ports, pool, d_plan, d_off, counts, n_max, &s);
    // a lane per frame: its rank among the frames not redirected and among the PASS frames, in batch order
    const uint8_t a = i < s.r ? actions[i] : (uint8_t)XSK_GPU_XDP_REDIRECT;  // (r <= n_max: no action behind the bound is read)
    const bool nr = rp_rest(i, s.r, a), pass = ps_pass(i, s.r, a);
    const unsigned long long mn = cp_wg_ballot(nr, s_wn), mq = cp_wg_ballot(pass, s_wq);
    const PassPlan p = pass_plan(w, cp_waves_below<kPsSmallWaves>(s_wn, kPsSmallWaves, 0u),
                                 cp_waves_below<kPsSmallWaves>(s_wq, kPsSmallWaves, 0u));
    if (nr)
        pass_place(stack, p, pass, cp_waves_below<kPsSmallWaves>(s_wn, cp_wave(), 0u) + cp_below(mn, cp_lane()),
                   cp_waves_below<kPsSmallWaves>(s_wq, cp_wave(), 0u) + cp_below(mq, cp_lane()), descs, i, s_rest);
    __syncthreads();
    end_copy(tx, n_ports, pool, &s, p.n_rest, d_tx, d_free, s_rest, i, kPsSmallThreads);
    __threadfence();  // the entries before the words that cover them
    __syncthreads();
    end_publish(rx, tx, n_ports, pool, &s, p.n_rest, d_plan, reinterpret_cast<xsk_gpu_rx_steer_result*>(d_res));
    pass_publish(stack, p, d_res);
}

// ---- larger bounds: the two count rows, the rest list by count / scan / scatter into the workspace ----
__global__ __launch_bounds__(kCpFrames) void rx_pass_end_count_kernel(const xsk_gpu_rx_plan* d_plan,
                                                                      const uint8_t* __restrict__ actions, uint32_t n_max,
                                                                      uint32_t* __restrict__ row_rest,
                                                                      uint32_t* __restrict__ row_pass) {
    __shared__ uint32_t s_wn[kCpWaves], s_wq[kCpWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kCpFrames + threadIdx.x;
    const uint32_t r = rp_received(d_plan->received, n_max);
    const uint8_t a = i < r ? actions[i] : (uint8_t)XSK_GPU_XDP_REDIRECT;
    cp_wg_count(i < r && rp_rest((uint32_t)i, r, a), s_wn, row_rest);
    cp_wg_count(i < r && ps_pass((uint32_t)i, r, a), s_wq, row_pass);
}

// A workgroup per row; the word behind the rows that belongs to the row receives its total.
__global__ __launch_bounds__(kCpScanThreads) void rx_pass_end_scan_kernel(uint32_t* cells, uint32_t nwg, uint32_t* totals) {
    __shared__ uint32_t sc[kCpScanThreads];
    uint32_t b, e;
    cp_scan_run(nwg, threadIdx.x, &b, &e);
    const uint32_t total = cp_scan_cells(cells + (size_t)blockIdx.x * nwg, b, e, sc, cp_put_before);
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

__global__ __launch_bounds__(kCpFrames) void rx_pass_end_scatter_kernel(Ring stack, const xsk_gpu_rx_plan* d_plan,
                                                                        const xsk_gpu_desc* descs, const uint8_t* actions,
                                                                        uint32_t n_max, const uint32_t* row_rest,
                                                                        const uint32_t* row_pass, const uint32_t* totals,
                                                                        uint64_t* rest) {
    __shared__ uint32_t s_wn[kCpWaves], s_wq[kCpWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kCpFrames + threadIdx.x;
    // the stack ring's words do not change before the publish launch: every workgroup decides the same share
    const StackWords w = stack_words(stack);
    const uint32_t r = rp_received(d_plan->received, n_max);
    const uint8_t a = i < r ? actions[i] : (uint8_t)XSK_GPU_XDP_REDIRECT;
    const bool nr = i < r && rp_rest((uint32_t)i, r, a), pass = i < r && ps_pass((uint32_t)i, r, a);
    const unsigned long long mn = cp_wg_ballot(nr, s_wn), mq = cp_wg_ballot(pass, s_wq);
    if (!nr) return;
    const PassPlan p = pass_plan_ws(w, totals, n_max);
    pass_place(stack, p, pass, cp_waves_below<kCpWaves>(s_wn, cp_wave(), row_rest[blockIdx.x]) + cp_below(mn, cp_lane()),
               cp_waves_below<kCpWaves>(s_wq, cp_wave(), row_pass[blockIdx.x]) + cp_below(mq, cp_lane()), descs,
               (uint32_t)i, rest);
}

__global__ __launch_bounds__(kRdCopy) void rx_pass_end_copy_kernel(Rings tx, uint32_t n_ports, Ring stack, Pool pool,
                                                                   const xsk_gpu_rx_plan* d_plan, const uint32_t* d_off,
                                                                   const xsk_gpu_desc* d_tx, const uint64_t* d_free,
                                                                   const xsk_gpu_egress_counts* counts, uint32_t n_max,
                                                                   const uint64_t* rest, const uint32_t* totals) {
    __shared__ EndLds s;
    const StackWords w = stack_words(stack);
    end_decide(tx, n_ports, pool, d_plan, d_off, counts, n_max, &s);
    end_copy(tx, n_ports, pool, &s, pass_plan_ws(w, totals, n_max).n_rest, d_tx, d_free, rest,
             rd_copy_first(blockIdx.x, threadIdx.x), rd_copy_stride(gridDim.x));
}

__global__ __launch_bounds__(kRdWave) void rx_pass_end_publish_kernel(Ring rx, Rings tx, uint32_t n_ports, Ring stack,
                                                                      Pool pool, const xsk_gpu_rx_plan* d_plan,
                                                                      const uint32_t* d_off,
                                                                      const xsk_gpu_egress_counts* counts, uint32_t n_max,
                                                                      const uint32_t* totals,
                                                                      xsk_gpu_rx_pass_result* d_res) {
    __shared__ EndLds s;
    const StackWords w = stack_words(stack);
    end_decide(tx, n_ports, pool, d_plan, d_off, counts, n_max, &s);
    const PassPlan p = pass_plan_ws(w, totals, n_max);
    end_publish(rx, tx, n_ports, pool, &s, p.n_rest, d_plan, reinterpret_cast<xsk_gpu_rx_steer_result*>(d_res));
    pass_publish(stack, p, d_res);
}

// ---- the argument rules: those of xsk_gpu_rx_ports_end_dev(), and the stack ring's (stack_ok, pass_step_ok:
// xsk_ring_pass_device.h) ----
int pass_end_launch(const xsk_gpu_ring_dev* rx, const xsk_gpu_ring_dev* tx, uint32_t n_ports,
                    const xsk_gpu_ring_dev* stack, const xsk_gpu_pool_dev* pool, const xsk_gpu_rx_plan* d_plan,
                    const xsk_gpu_desc* d_descs, const uint8_t* d_actions, const uint32_t* d_off,
                    const xsk_gpu_desc* d_tx, const uint64_t* d_free, const xsk_gpu_egress_counts* d_counts,
                    uint32_t n_max, xsk_gpu_rx_pass_result* d_res, void* d_workspace, hipStream_t s) {
    const Ring r = ring_of(rx), k = stack ? ring_of(stack) : Ring{nullptr, nullptr, nullptr, 1u};
    const Rings t = rings_of(tx, n_ports);
    const Pool p = pool_of(pool);
    if (n_max <= kPsSmallMax) {
        rx_pass_end_small_kernel<<<dim3(1), dim3(kPsSmallThreads), 0, s>>>(r, t, n_ports, k, p, d_plan, d_descs,
                                                                           d_actions, d_off, d_tx, d_free, d_counts,
                                                                           n_max, d_res);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    uint8_t* const ws = (uint8_t*)d_workspace;
    uint64_t* const rest = (uint64_t*)(ws + ps_end_rest(n_max));
    uint32_t* const row_rest = (uint32_t*)(ws + ps_end_row(n_max, kPsRowRest));
    uint32_t* const row_pass = (uint32_t*)(ws + ps_end_row(n_max, kPsRowPass));
    uint32_t* const totals = (uint32_t*)(ws + ps_end_totals(n_max));
    const uint32_t nwg = cp_nwg(n_max);
    rx_pass_end_count_kernel<<<dim3(nwg), dim3(kCpFrames), 0, s>>>(d_plan, d_actions, n_max, row_rest, row_pass);
    HIP_TRY(hipGetLastError());
    rx_pass_end_scan_kernel<<<dim3(kPsRows), dim3(kCpScanThreads), 0, s>>>(row_rest, nwg, totals);
    HIP_TRY(hipGetLastError());
    rx_pass_end_scatter_kernel<<<dim3(nwg), dim3(kCpFrames), 0, s>>>(k, d_plan, d_descs, d_actions, n_max, row_rest,
                                                                     row_pass, totals, rest);
    HIP_TRY(hipGetLastError());
    rx_pass_end_copy_kernel<<<dim3(rd_nwg(n_max)), dim3(kRdCopy), 0, s>>>(t, n_ports, k, p, d_plan, d_off, d_tx, d_free,
                                                                          d_counts, n_max, rest, totals);
    HIP_TRY(hipGetLastError());
    rx_pass_end_publish_kernel<<<dim3(1), dim3(kRdWave), 0, s>>>(r, t, n_ports, k, p, d_plan, d_off, d_counts, n_max,
                                                                 totals, d_res);
    HIP_TRY(hipGetLastError());
    return 0;
}

RpLayout layout_of(uint32_t max_batch, uint32_t n_ports) {
    return ps_layout(max_batch, n_ports, xsk_gpu_steer_workspace_size(max_batch, n_ports),
                     xsk_gpu_egress_ports_workspace_size(max_batch, n_ports));
}

}  // namespace

extern "C" {

size_t xsk_gpu_rx_pass_step_dev_workspace_size(uint32_t max_batch, uint32_t n_ports) {
    if (n_ports > kEpMaxPorts) n_ports = kEpMaxPorts;
    return layout_of(max_batch, n_ports).bytes;
}

int xsk_gpu_rx_pass_end_dev(const struct xsk_gpu_ring_dev* rx, const struct xsk_gpu_ring_dev* tx, uint32_t n_ports,
                            const struct xsk_gpu_ring_dev* stack, const struct xsk_gpu_pool_dev* pool,
                            const struct xsk_gpu_rx_plan* d_plan, const struct xsk_gpu_desc* d_descs,
                            const uint8_t* d_actions, const uint32_t* d_off, const struct xsk_gpu_desc* d_tx,
                            const uint64_t* d_free, const struct xsk_gpu_egress_counts* d_counts, uint32_t n_max,
                            struct xsk_gpu_rx_pass_result* d_res, void* d_workspace, void* stream) {
    if (!end_ok(rx, tx, n_ports, pool, d_plan, d_descs, d_actions, d_off, d_tx, d_free, d_counts, n_max, d_res,
                d_workspace) ||
        !stack_ok(stack, rx, tx, n_ports))
        return -EINVAL;
    return pass_end_launch(rx, tx, n_ports, stack, pool, d_plan, d_descs, d_actions, d_off, d_tx, d_free, d_counts, n_max,
                           d_res, d_workspace, (hipStream_t)stream);
}

int xsk_gpu_rx_pass_step_dev(void* d_umem, uint64_t umem_size, const struct xsk_gpu_ring_dev* rx,
                             const struct xsk_gpu_ring_dev* fill, const struct xsk_gpu_ring_dev* tx,
                             const struct xsk_gpu_ring_dev* stack, const struct xsk_gpu_pool_dev* pool,
                             uint32_t max_batch, uint32_t opts, const struct xsk_gpu_steer_entry* d_table,
                             uint32_t n_entries, uint32_t default_port, uint32_t n_ports, const uint64_t* d_bound,
                             uint8_t* d_actions, uint8_t* d_ports, struct xsk_gpu_egress_counts* d_port_counts,
                             struct xsk_gpu_stats* d_stats, struct xsk_gpu_stats* d_port_stats,
                             struct xsk_gpu_rx_pass_result* d_res, void* d_workspace, void* stream) {
    if (!pass_step_ok(d_umem, umem_size, rx, fill, tx, stack, pool, max_batch, opts, d_table, n_entries, default_port,
                      n_ports, d_bound, d_port_counts, d_stats, d_port_stats, d_res, d_workspace))
        return -EINVAL;
    uint8_t* const ws = (uint8_t*)d_workspace;
    const RpLayout l = layout_of(max_batch, n_ports);
    xsk_gpu_rx_plan* const plan = (xsk_gpu_rx_plan*)(ws + l.plan);
    uint32_t* const room = (uint32_t*)(ws + l.room);
    uint32_t* const off = (uint32_t*)(ws + l.off);
    xsk_gpu_egress_counts* const counts = d_port_counts ? d_port_counts : (xsk_gpu_egress_counts*)(ws + l.counts);
    xsk_gpu_desc* const descs = (xsk_gpu_desc*)(ws + l.descs);
    xsk_gpu_desc* const out = (xsk_gpu_desc*)(ws + l.out);
    xsk_gpu_desc* const d_tx = (xsk_gpu_desc*)(ws + l.tx);
    uint64_t* const d_free = (uint64_t*)(ws + l.free_list);
    uint8_t* const verdicts = ws + l.verdicts;
    uint8_t* const actions = d_actions ? d_actions : ws + l.actions;
    uint8_t* const ports = d_ports ? d_ports : ws + l.ports;
    int rc = xsk_gpu_rx_begin_dev(rx, fill, &tx[0], pool, max_batch, descs, plan, stream);
    if (rc) return rc;
    rc = xsk_gpu_rx_prepare_ports_dev(tx, n_ports, plan, descs, max_batch, room, stream);
    if (rc) return rc;
    rc = xsk_gpu_ingress_steer_dev(d_umem, umem_size, descs, max_batch, opts, d_table, n_entries, default_port, n_ports,
                                   d_bound, actions, ports, out, off, verdicts, NULL, d_stats, ws + l.steer, stream);
    if (rc) return rc;
    rc = xsk_gpu_egress_ports_dev(out, verdicts, off, n_ports, max_batch, room, d_tx, d_free, counts, d_stats,
                                  d_port_stats, ws + l.egress, stream);
    if (rc) return rc;
    return pass_end_launch(rx, tx, n_ports, stack, pool, plan, descs, actions, off, d_tx, d_free, counts, max_batch, d_res,
                           ws + l.end, (hipStream_t)stream);
}

}  // extern "C"
