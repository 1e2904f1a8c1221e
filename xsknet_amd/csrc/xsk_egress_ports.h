// xsk_egress_ports.h — the arithmetic of xsk_gpu_egress_ports_dev() (include/xsk_gpu.h): the segments of
// the steered list from the n_ports + 1 offset words, "which port owns position i", the per-port slot (xsk_egress.h's
// rule over the port's own segment), the reply prefix at a port boundary, and the grid, workgroup and workspace sizes of
// both paths.  Host and device: xsk_egress_ports.hip's kernels and its host launch call these functions, and
// tests/c/test_egress_ports.cpp replays both paths with them on the CPU under AddressSanitizer.
//
// Segments: o_p = min(max(d_off[0..p]), n_max) for p = 0 .. n_ports -- ascending and inside [0, n_max] for any words.
// Port p owns [o_p, o_{p+1}).  With G(x) = the replies in [o_0, x):
//   R_p(i) = G(i) - G(o_p);  frame i of port p goes where eg_slot(reply, i - o_p, R_p(i), room_p) says, plus o_p.
#ifndef XSK_EGRESS_PORTS_H
#define XSK_EGRESS_PORTS_H

#include "xsk_egress.h"

namespace xskgpu {

constexpr uint32_t kEpMaxPorts = 64;                 // == XSK_GPU_STEER_MAX_PORTS
constexpr uint32_t kEpMaxBounds = kEpMaxPorts + 1u;  // offsets, and boundary prefixes, of one call

// ---- the offsets ----
// The running maximum is taken over the raw words, the clamp on what it leaves: o_p = ep_clamp(max(words[0..p]), n_max).
XSK_EG_FN uint32_t ep_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
XSK_EG_FN uint32_t ep_clamp(uint32_t run_max, uint32_t n_max) { return eg_min(run_max, n_max); }

// All n_ports + 1 offsets, in sequence (the kernels' prologue does the same as a wave's inclusive max-scan).
XSK_EG_FN void ep_offsets(const uint32_t* words, uint32_t n_ports, uint32_t n_max, uint32_t* o) {
    uint32_t run = 0;
    for (uint32_t p = 0; p <= n_ports; ++p) {
        run = ep_max(run, words[p]);
        o[p] = ep_clamp(run, n_max);
    }
}

// Position i is read and listed iff o_0 <= i < o_{n_ports}.
XSK_EG_FN bool ep_in(uint32_t i, uint32_t lo, uint32_t hi) { return i >= lo && i < hi; }

// ---- which port owns position i ----
// The number of offsets o[0 .. n_ports] that are <= i: an upper bound over at most 65 ascending words, at most 7 probes.
XSK_EG_FN uint32_t ep_upper(const uint32_t* o, uint32_t n_ports, uint32_t i) {
    uint32_t lo = 0, hi = n_ports + 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (o[mid] <= i)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo;
}

struct EpOwner {
    bool on;        // i lies in a segment
    uint32_t port;  // the one with o_port <= i < o_{port + 1}; empty segments (o_p == o_{p + 1}) are never returned
};

XSK_EG_FN EpOwner ep_owner(const uint32_t* o, uint32_t n_ports, uint32_t i) {
    const uint32_t ub = ep_upper(o, n_ports, i);
    EpOwner w;
    w.on = ub >= 1u && ub <= n_ports;  // 0: below o_0; n_ports + 1: at or above o_{n_ports}
    w.port = w.on ? ub - 1u : 0u;
    return w;
}

// ---- the per-port slot ----
// Frame i of the port with offset o_p, g_i = G(i), g_p = G(o_p): the index into d_tx or d_free, inside the port's span.
XSK_EG_FN EgSlot ep_slot(bool reply, uint32_t i, uint32_t o_p, uint32_t g_i, uint32_t g_p, uint32_t room) {
    EgSlot s = eg_slot(reply, i - o_p, g_i - g_p, room);
    s.slot += o_p;
    return s;
}
XSK_EG_FN bool ep_unsent(bool reply, uint32_t g_i, uint32_t g_p, uint32_t room) {
    return eg_unsent(reply, g_i - g_p, room);
}
// d_counts[p] from the port's two offsets and the prefixes at them.
XSK_EG_FN EgCounts ep_counts(uint32_t o_p, uint32_t o_p1, uint32_t g_p, uint32_t g_p1, uint32_t room) {
    return eg_counts(o_p1 - o_p, g_p1 - g_p, room);
}

// ---- the reply prefix inside one workgroup, from its per-wave counts and ballot masks ----
// Replies of the workgroup at lanes below `pos` (pos may be the workgroup's size: all of them).
XSK_EG_FN uint32_t ep_prefix_at(const uint32_t* s_w, const uint64_t* s_m, uint32_t nw, uint32_t pos) {
    const uint32_t w = pos / kEgWave, lane = pos % kEgWave;
    uint32_t g = 0;
    for (uint32_t k = 0; k < nw; ++k) g += k < w ? s_w[k] : 0u;
    if (w < nw) g += (uint32_t)__builtin_popcountll(s_m[w] & ((1ull << lane) - 1ull));
    return g;
}

// ---- the three-stage path (n_max > kEgSmallMax) ----
// Grid of stages 1 and 3: cp_nwg(n_max) workgroups of kEgFrames frames; workgroup wg takes part iff it holds a position
// of [lo, hi).
XSK_EG_FN bool ep_wg_live(uint32_t wg, uint32_t lo, uint32_t hi) {
    const uint64_t b = (uint64_t)wg * kEgFrames;
    return lo < hi && b < hi && b + kEgFrames > lo;
}

// The prefix at boundary o: the scanned count of workgroup ep_bound_wg(o) plus the replies in [ep_bound_from(o, lo), o),
// at most kEgFrames - 1 verdicts; a boundary on or behind the last workgroup's end (ep_bound_wg(o) >= nwg) is the total.
XSK_EG_FN uint32_t ep_bound_wg(uint32_t o) { return o / kEgFrames; }
XSK_EG_FN uint32_t ep_bound_from(uint32_t o, uint32_t lo) { return ep_max(ep_bound_wg(o) * kEgFrames, lo); }

// ---- the per-port counter blocks on the three-stage path ----
// With one port every scatter workgroup's sums belong to the same block, and a set of atomics per workgroup on one
// block costs ten times the rest of the call.  So a workgroup whose FIRST position wg * kEgFrames is
// listed leaves the sums of the port that owns that position as a plain store, EpPart[wg], and a fourth launch, a
// workgroup per port, adds up the port's records and issues one set of atomics; the ports that BEGIN inside a
// workgroup (at most n_ports such pairs in all) take their atomics from the scatter.
struct EpPart {  // 32 B of words (the workspace is word-aligned): the two byte sums as halves
    uint32_t n, n_tx, bytes_lo, bytes_hi, tx_bytes_lo, tx_bytes_hi, pad[2];
};
XSK_EG_FN uint64_t ep_u64(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

// Workgroup wg leaves a record iff its first position is listed.
XSK_EG_FN bool ep_wg_carries(uint32_t wg, uint32_t lo, uint32_t hi) {
    const uint64_t b = (uint64_t)wg * kEgFrames;
    return b >= lo && b < hi;
}
// The records of the port with offsets [o_p, o_p1): workgroups [ep_carry_begin(o_p), ep_carry_begin(o_p1)) -- those
// whose first position the port owns; none for an empty port or one that lies inside a workgroup behind its start.
XSK_EG_FN uint32_t ep_carry_begin(uint32_t o) { return o / kEgFrames + (o % kEgFrames ? 1u : 0u); }

// Workspace: words [0, nwg) the per-workgroup reply counts, then their exclusive offsets; words [nwg, nwg + n_ports + 1)
// the boundary prefixes G(o_p); from ep_part_offset() on nwg records EpPart.  None on the small path.
XSK_EG_FN size_t ep_part_offset(uint32_t n_max, uint32_t n_ports) {
    return ((size_t)cp_nwg(n_max) + n_ports + 1u) * sizeof(uint32_t);
}
XSK_EG_FN size_t ep_workspace_bytes(uint32_t n_max, uint32_t n_ports) {
    return n_max <= kEgSmallMax ? (size_t)0 : ep_part_offset(n_max, n_ports) + (size_t)cp_nwg(n_max) * sizeof(EpPart);
}

}  // namespace xskgpu

#endif  // XSK_EGRESS_PORTS_H
