// xsk_responder_body.h — the RX loop body and the neighbour responder as one launch: the kernels of
// xsk_gpu_responder_dev() and xsk_gpu_responder_queues_dev() (include/xsk_gpu.h).  It is
// loop_fused_body<C>() (xsk_loop_fused_body.h), a fence and a barrier, then the serve call's one-workgroup body
// (ng_serve_body(), xsk_neigh_device.h) in the same 1024 threads.
//
// What the design rests on:
//   - loop_fused_body() leaves through three exits (no completion rings; a completion bound of zero; its end).  It is
//     an inlined function, so each `return` ends only that function; all three are workgroup-uniform, so every lane
//     reaches the fence below.
//   - The serve stage reads every index word -- the TX rings' producer and consumer words, the stack ring's, `up`'s --
//     inside ng_serve_body(), through load_word, behind that fence and barrier: what stage 6 published is what it sees.
//     Nothing stage 2 put into P.room[] and no word read in front of the fence reaches it.
//   - The TX rings and the stack ring are the ones the loop body unpacked into LDS (L.tx, L.stack; the ports at or above
//     n_ports are the absent ring there too); `up` is one more packed ring of the arguments.
//   - The serve stage's LDS is a member of the stages' overlay (LoopStageLds::serve), and the neighbour table is staged
//     into it behind the fence, when no earlier stage needs the overlay any more.
//   - Nothing of the loop body is live across the call but the arguments and the LDS block.
#ifndef XSK_RESPONDER_BODY_H
#define XSK_RESPONDER_BODY_H

#include "xsk_loop_fused_body.h"
#include "xsk_neigh_device.h"

namespace xskgpu {
namespace {

// The kernel's arguments, one struct by value (one record of a block in the many-queue form): the loop body's, then the
// serve stage's.
struct ResponderArgs {
    LoopFusedArgs f;  // f.stack is a real ring: the call requires it
    PackedRing up;
    const xsk_gpu_neigh_entry* ntable;
    xsk_gpu_neigh_stats* d_nstats;
    xsk_gpu_neigh_result* d_nres;
    uint32_t n_nentries, serve_max;
};
static_assert(sizeof(ResponderArgs) + 256 <= 4096, "the kernel arguments");

template <class C>
__device__ __forceinline__ void responder_body(const ResponderArgs& A, LoopFusedLds& L) {
    loop_fused_body<C>(A.f, L);
    lf_stage_fence();  // behind every exit of the loop body: its publishes before the serve stage's reads
    NgServeParams p;
    p.umem = A.f.umem;
    p.umem_size = A.f.umem_size;
    p.table = A.ntable;
    p.d_bound = A.f.d_bound;
    p.d_nstats = A.d_nstats;
    p.d_res = A.d_nres;
    p.n_ports = A.f.n_ports;
    p.max = A.serve_max;
    p.opts = A.f.opts;
    p.n_entries = A.n_nentries;
    NgServeLds& S = L.u.serve;
    ng_serve_body(
        p,
        [&](uint32_t k) { return k < kNgUp ? L.tx.r[k] : (k == kNgUp ? lf_ring_dev(A.up) : L.stack); },
        S.tab, S.ring, S.cnt, S.red, S.prod, S.room, S.wu, S.wstop, S.cons, S.used);
}
static_assert(kNgMaxPorts == kEpMaxPorts && kNgServeThreads == kLfThreads, "one ring per port and one workgroup size");

}  // namespace
}  // namespace xskgpu

#endif  // XSK_RESPONDER_BODY_H
