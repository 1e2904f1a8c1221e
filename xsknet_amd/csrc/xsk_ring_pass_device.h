// xsk_ring_pass_device.h — the end stage with a stack ring as device code (xsk_gpu_rx_pass_end_dev()):
// the stack ring's words and share (StackWords, PassPlan), a frame's place (pass_place), the publish (pass_publish) and
// the whole one-workgroup form (rx_pass_end_small_body), which is also stage 6 of the fused loop kernel
// (xsk_loop_fused_body.h, §9.11); and the argument rules of xsk_gpu_rx_pass_step_dev(), which that call, the loop call
// and the fused loop call check through one function.  EndLds, end_decide, end_copy and end_publish are
// xsk_ring_ports_device.h's; the arithmetic is xsk_ring_pass.h's.  Everything here is in an anonymous namespace.
#ifndef XSK_RING_PASS_DEVICE_H
#define XSK_RING_PASS_DEVICE_H

#include <hip/hip_runtime.h>

#include "../../include/xsk_gpu.h"
#include "xsk_ring_pass.h"
#include "xsk_ring_ports_device.h"

namespace xskgpu {
namespace {

// The stack ring's producer word and room as a lane reads them at the top of its kernel (the loads are in flight while
// the workgroup decides); nothing without a stack ring.
struct StackWords {
    uint32_t prod, room;
};
__device__ __forceinline__ StackWords stack_words(const Ring& stack) {
    const bool has = stack.ring != nullptr;
    StackWords w;
    w.prod = has ? load_word(stack.prod) : 0u;
    w.room = ps_room(has, w.prod, has ? load_word(stack.cons) : 0u, stack.size);
    return w;
}

// What a launch decides about the stack ring from those words and the two totals.
struct PassPlan {
    uint32_t prod;    // the stack ring's producer word as read
    uint32_t taken;   // s
    uint32_t full;    // Q - s
    uint32_t n_rest;  // N - s
};
__device__ __forceinline__ PassPlan pass_plan(const StackWords& w, uint32_t n_total, uint32_t q_total) {
    PassPlan p;
    p.prod = w.prod;
    p.taken = ps_taken(q_total, w.room);
    p.full = q_total - p.taken;
    p.n_rest = ps_n_rest(n_total, p.taken);
    return p;
}
// The totals the scan left behind the count rows.
__device__ __forceinline__ PassPlan pass_plan_ws(const StackWords& w, const uint32_t* totals, uint32_t n_max) {
    const uint32_t n_total = ps_total_rest(totals[kPsRowRest], n_max);
    return pass_plan(w, n_total, ps_total_pass(totals[kPsRowPass], n_total));
}

// Frame i, not redirected, with ranks n_i and q_i: onto the stack ring, or into the rest.
__device__ __forceinline__ void pass_place(const Ring& stack, const PassPlan& p, bool pass, uint32_t n_i, uint32_t q_i,
                                           const xsk_gpu_desc* descs, uint32_t i, uint64_t* rest) {
    if (ps_on_stack(pass, q_i, p.taken))
        *desc_slot(stack, p.prod + q_i) = reinterpret_cast<const uint4*>(descs)[i];
    else
        rest[ps_rest_pos(n_i, q_i, p.taken)] = desc_addr(descs, i);
}

// Behind end_publish(): lane 0 completes *d_res, the workgroup's last lane stores the stack ring's producer word.
__device__ __forceinline__ void pass_publish(const Ring& stack, const PassPlan& p, xsk_gpu_rx_pass_result* d_res) {
    if (threadIdx.x == 0 && d_res) {
        d_res->passed = p.taken;
        d_res->pass_full = p.full;
    }
    if (threadIdx.x == blockDim.x - 1u && p.taken) *stack.prod = p.prod + p.taken;
}

// ---- bound <= 1024: one workgroup of kPsSmallThreads.  Its LDS, and the body every lane calls ----
// (s, s_wn[kPsSmallWaves], s_wq[kPsSmallWaves] and s_rest[kPsSmallMax] are the caller's, in LDS: as one struct the kernel
// came out as other instructions)
__device__ __forceinline__ void rx_pass_end_small_body(const Ring& rx, const Rings& tx, uint32_t n_ports, const Ring& stack,
                                                       const Pool& pool, const xsk_gpu_rx_plan* d_plan,
                                                       const xsk_gpu_desc* descs, const uint8_t* actions,
                                                       const uint32_t* d_off, const xsk_gpu_desc* d_tx,
                                                       const uint64_t* d_free, const xsk_gpu_egress_counts* counts,
                                                       uint32_t n_max, xsk_gpu_rx_pass_result* d_res, EndLds& s,
                                                       uint32_t* s_wn, uint32_t* s_wq, uint64_t* s_rest) {
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

// ---- the argument rules: those of xsk_gpu_rx_ports_end_dev(), and the stack ring's ----
// NULL, or a descriptor ring that shares neither its entry array nor its producer word with rx or a port's ring
inline bool stack_ok(const xsk_gpu_ring_dev* stack, const xsk_gpu_ring_dev* rx, const xsk_gpu_ring_dev* tx, uint32_t n_ports) {
    if (!stack) return true;
    if (!ring_ok(stack, 16u) || stack->d_ring == rx->d_ring || stack->d_producer == rx->d_producer) return false;
    for (uint32_t p = 0; p < n_ports; ++p)
        if (stack->d_ring == tx[p].d_ring || stack->d_producer == tx[p].d_producer) return false;
    return true;
}

// The rules of xsk_gpu_rx_pass_step_dev(): those of xsk_gpu_rx_step_steer_dev() (the workspace's arrays satisfy the
// composed calls' by layout), and the stack ring's.
inline bool pass_step_ok(const void* d_umem, uint64_t umem_size, const xsk_gpu_ring_dev* rx, const xsk_gpu_ring_dev* fill,
                         const xsk_gpu_ring_dev* tx, const xsk_gpu_ring_dev* stack, const xsk_gpu_pool_dev* pool,
                         uint32_t max_batch, uint32_t opts, const xsk_gpu_steer_entry* d_table, uint32_t n_entries,
                         uint32_t default_port, uint32_t n_ports, const uint64_t* d_bound, const void* d_port_counts,
                         const void* d_stats, const void* d_port_stats, const void* d_res, const void* d_workspace) {
    return !(!d_workspace || ((uintptr_t)d_workspace & 15u) || !d_umem || ((uintptr_t)d_umem & 15u) || (umem_size & 15u) ||
             (umem_size >> 48) || (opts & ~XSK_GPU_OPT_MASK) || ((uintptr_t)d_stats & 7u) ||
             ((uintptr_t)d_port_stats & 7u) || ((uintptr_t)d_res & 3u) || ((uintptr_t)d_port_counts & 3u) ||
             !bound_ok(max_batch) || !ports_ok(tx, n_ports) || !ring_ok(rx, 16u) || !ring_ok(fill, 8u) || !pool_ok(pool) ||
             !stack_ok(stack, rx, tx, n_ports) || (default_port >= n_ports && default_port != XSK_GPU_STEER_PASS) ||
             n_entries > XSK_GPU_STEER_MAX_ENTRIES || (n_entries && (!d_table || ((uintptr_t)d_table & 7u))) ||
             ((uintptr_t)d_bound & 7u));
}

}  // namespace
}  // namespace xskgpu

#endif  // XSK_RING_PASS_DEVICE_H
