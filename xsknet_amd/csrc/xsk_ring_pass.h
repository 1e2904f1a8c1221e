// xsk_ring_pass.h — the arithmetic of xsk_gpu_rx_pass_end_dev() and xsk_gpu_rx_pass_step_dev() (include/xsk_gpu.h;
// DESIGN.md §9.9): the steered RX step with a stack ring, a descriptor ring for the frames the filter passes to the
// kernel stack.  Which frames are PASS frames, how many the stack ring takes, which slot a taken frame gets, where every
// other frame the filter did not redirect lands in the rest of the pool's list, and the grid and workspace sizes.  Host
// and device: xsk_ring_pass.hip's kernels and its host launch call these functions, and tests/c/test_ring_pass.cpp
// replays both paths with them on the CPU, into heap arrays of exactly the rings' sizes under AddressSanitizer.
//
// Everything that is not about the stack ring is xsk_ring_ports.h's (r, o_p, t_p, f_p, F_p, pushed, rp_tx_lane,
// rp_pool_src).  With nr(i) = d_actions[i] != REDIRECT, ps(i) = d_actions[i] == PASS for i < r, N(i) / Q(i) the frames
// below i with nr / ps set, N = N(r), Q = Q(r):
//   s      = min(Q, free(stack))              PASS descriptors the stack ring takes (0 without a stack ring)
//   ps(i) and Q(i) < s:  stack entry (stack_prod + Q(i)) & mask = d_descs[i]
//   every other nr(i):   position N(i) - min(Q(i), s) of the rest, which is N - s long
// ps implies nr, so Q(i) <= N(i) and s <= Q <= N: neither difference wraps.
#ifndef XSK_RING_PASS_H
#define XSK_RING_PASS_H

#include "xsk_ring_ports.h"

namespace xskgpu {

constexpr uint32_t kPsSmallMax = kRpSmallMax;  // == XSK_GPU_LOWLAT_MAX: one launch of one workgroup up to here
constexpr uint32_t kPsSmallThreads = kRpSmallThreads;
constexpr uint32_t kPsSmallWaves = kRpSmallWaves;
constexpr uint32_t kPsRows = 2;     // the count rows of the larger bounds: nr, ps
constexpr uint32_t kPsRowRest = 0;  // frames the filter did not redirect
constexpr uint32_t kPsRowPass = 1;  // PASS frames

// A PASS frame: received, and left to the kernel stack.  An action byte that is none of 1, 2, 4 is a rest frame
// (rp_rest) and no PASS frame.
XSK_RD_FN bool ps_pass(uint32_t i, uint32_t r, uint8_t action) { return i < r && action == XSK_GPU_XDP_PASS; }

// The totals as the launches behind the scan clamp them: N <= n_max, Q <= N.
XSK_RD_FN uint32_t ps_total_rest(uint32_t word, uint32_t n_max) { return rd_min(word, n_max); }
XSK_RD_FN uint32_t ps_total_pass(uint32_t word, uint32_t n_rest_all) { return rd_min(word, n_rest_all); }

// room_s: the stack ring's free entries as read at execution; 0 without a stack ring.
XSK_RD_FN uint32_t ps_room(bool has_stack, uint32_t prod, uint32_t cons, uint32_t size) {
    return has_stack ? rd_free(prod, cons, size) : 0u;
}
// s
XSK_RD_FN uint32_t ps_taken(uint32_t q_total, uint32_t room) { return rd_min(q_total, room); }
// Frame i with ps(i) and rank q = Q(i): on the stack ring iff q < s; its slot then.  q < s <= free(stack) <= size, so
// the slot is one of the ring's free entries and no two frames share it.
XSK_RD_FN bool ps_on_stack(bool pass, uint32_t q, uint32_t s) { return pass && q < s; }
XSK_RD_FN uint32_t ps_stack_slot(uint32_t prod, uint32_t q, uint32_t size) { return rd_slot(prod + q, size); }
// Frame i with nr(i) that is not on the stack ring: its position in the rest.  Below N - s.
XSK_RD_FN uint32_t ps_rest_pos(uint32_t n_i, uint32_t q_i, uint32_t s) { return n_i - rd_min(q_i, s); }
XSK_RD_FN uint32_t ps_n_rest(uint32_t n_total, uint32_t s) { return n_total - s; }

// ---- grids ----
// One workgroup up to kPsSmallMax.  Above: the count and scatter launches are cp_nwg(n_max) workgroups of kCpFrames
// lanes, a lane per frame; the scan is kPsRows workgroups of kCpScanThreads, a workgroup per row; the copy launch is
// rd_nwg(n_max) workgroups of kRdCopy lanes, the publish one wave.

// ---- end's workspace above kPsSmallMax: the compacted rest (8 B each), kPsRows rows of per-workgroup counts /
// offsets (row kPsRowRest, then row kPsRowPass), the kPsRows totals ----
XSK_RD_FN size_t ps_end_rest(uint32_t) { return 0; }
XSK_RD_FN size_t ps_end_cells(uint32_t n_max) { return (size_t)n_max * 8u; }
XSK_RD_FN size_t ps_end_row(uint32_t n_max, uint32_t row) { return ps_end_cells(n_max) + (size_t)row * cp_nwg(n_max) * 4u; }
XSK_RD_FN size_t ps_end_totals(uint32_t n_max) { return ps_end_row(n_max, kPsRows); }
XSK_RD_FN size_t ps_end_workspace_bytes(uint32_t n_max) {
    return n_max <= kPsSmallMax ? (size_t)0 : rd_align(ps_end_totals(n_max) + kPsRows * 4u, 16u);
}

// ---- the workspace of xsk_gpu_rx_pass_step_dev(max_batch, n_ports): xsk_gpu_rx_step_steer_dev()'s layout with end's
// part grown by the second count row and its total ----
XSK_RD_FN RpLayout ps_layout(uint32_t max_batch, uint32_t n_ports, size_t steer_bytes, size_t egress_bytes) {
    RpLayout l = rp_layout(max_batch, n_ports, steer_bytes, egress_bytes);
    l.bytes = rd_align(l.end + ps_end_workspace_bytes(max_batch), 16u);
    return l;
}

}  // namespace xskgpu

#endif  // XSK_RING_PASS_H
