// xsk_responder.hip — xsk_gpu_responder_dev() and xsk_gpu_responder_queues_dev(): the RX loop body and the neighbour
// responder as ONE launch (include/xsk_gpu.h).  From the same state the one-queue call leaves what
// xsk_gpu_rx_fused_loop_dev() followed by xsk_gpu_neigh_serve_dev() leaves; the serve stage runs in the loop kernel's
// own 1024 threads behind a fence and a barrier (xsk_responder_body.h) where the two calls have a kernel boundary.  The
// many-queue call is that kernel once per queue, a workgroup a queue, its records in a block that
// xsk_gpu_responder_prepare() writes on the host (xsk_responder_block.h), as xsk_gpu_rx_queues_dev() has it.  The
// reference-mode and wire-mode instances of both kernels are here, the dual-stack ones in xsk_responder_ds.hip.  A file
// of its own: no existing translation unit's kernels change.
//
// One 1024-thread workgroup a CU, latency bound as both halves are.  No MFMA.
#include <errno.h>

#include <algorithm>
#include <new>
#include <utility>
#include <vector>

#include "xsk_gpu_internal.h"
#include "xsk_hip_util.h"
#include "xsk_responder_block.h"
#include "xsk_responder_body.h"

using namespace xskgpu;

namespace {

using ResponderQueuesLds = RsLds<LoopFusedLds, ResponderArgs>;
static_assert(sizeof(ResponderQueuesLds) <= 160u * 1024u, "the CU's LDS: the loop body's and the staged record");
static_assert(sizeof(ResponderQueuesLds) > 80u * 1024u, "and one workgroup a CU, as the launch bounds say");
// the record's layout as xsk_responder_block.h states it for the host
static_assert(sizeof(ResponderArgs) == kRsRecordBytes && alignof(ResponderArgs) <= 16, "a record");
static_assert(offsetof(ResponderArgs, f) == 0 && sizeof(LoopFusedArgs) == kRqRecordBytes &&
                  offsetof(ResponderArgs, up) == kRsUpOff,
              "the loop body's record first, `up` behind it");

template <bool WIRE>
__global__ __launch_bounds__(kLfThreads, 1) void responder_kernel(ResponderArgs A) {
    __shared__ LoopFusedLds L;
    responder_body<RoundCfg<WIRE, true>>(A, L);
}

template <bool WIRE>
__global__ __launch_bounds__(kLfThreads, 1) void responder_queues_kernel(const uint8_t* block, uint32_t n_queues,
                                                                         uint32_t opts) {
    __shared__ ResponderQueuesLds M;
    if (!rs_stage(block, n_queues, opts, M.S)) return;  // workgroup-uniform, before the first store
    responder_body<RoundCfg<WIRE, true>>(M.S.a, M.L);
}

bool share(const xsk_gpu_ring_dev* a, const xsk_gpu_ring_dev* b) {
    return a->d_ring == b->d_ring || a->d_producer == b->d_producer || a->d_consumer == b->d_consumer;
}

// One queue's rules: every rule of the fused call and every rule of the serve call, each through the function that
// call checks with, then what only the pair has -- `up` apart from the rings the serve call does not know.
bool responder_ok(const xsk_gpu_responder_queue* r, uint32_t opts) {
    if (!r || !r->q.stack || !r->up) return false;
    const xsk_gpu_rx_queue& q = r->q;
    if (!xsk_gpu__rxq_ok(&q, opts)) return false;
    if (!xsk_gpu__serve_ok(q.d_umem, q.stack, q.tx, q.n_ports, r->up, r->serve_max, opts, r->d_ntable, r->n_nentries,
                           q.d_bound, r->d_nstats, r->d_nres))
        return false;
    if (share(r->up, q.rx) || share(r->up, q.fill)) return false;
    for (uint32_t c = 0; c < q.n_comp; ++c)
        if (share(r->up, q.comp + c)) return false;
    return true;
}

// One queue's record; `a` arrives as zero bytes.
void pack_responder(const xsk_gpu_responder_queue& r, uint32_t opts, ResponderArgs& a) {
    xsk_gpu__rxq_pack(&r.q, opts, &a.f);
    a.up = lf_pack(r.up);
    a.ntable = r.d_ntable;
    a.d_nstats = r.d_nstats;
    a.d_nres = r.d_nres;
    a.n_nentries = r.n_nentries;
    a.serve_max = r.serve_max;
}

// No two queues share a pointer a kernel writes through: xsk_gpu_rx_queues_prepare()'s list, and up's three pointers,
// d_nstats and d_nres.  Every queue has passed responder_ok().
bool responders_disjoint(const xsk_gpu_responder_queue* queues, uint32_t n_queues) {
    std::vector<std::pair<uintptr_t, uint32_t>> v;
    std::vector<const void*> one(XSK_GPU__RXQ_OWNED_MAX);
    for (uint32_t k = 0; k < n_queues; ++k) {
        const xsk_gpu_responder_queue& r = queues[k];
        const uint32_t n = xsk_gpu__rxq_owned(&r.q, one.data());
        for (uint32_t i = 0; i < n; ++i) v.emplace_back((uintptr_t)one[i], k);
        const void* const more[5] = {r.up->d_ring, r.up->d_producer, r.up->d_consumer, r.d_nstats, r.d_nres};
        for (const void* p : more)
            if (p) v.emplace_back((uintptr_t)p, k);
    }
    std::sort(v.begin(), v.end());
    for (size_t i = 1; i < v.size(); ++i)
        if (v[i].first == v[i - 1].first && v[i].second != v[i - 1].second) return false;
    return true;
}

int responder_launch(const ResponderArgs& a, hipStream_t s) {
    if (a.f.opts & XSK_GPU_OPT_IPV6)
        xsk_gpu__responder_ds_launch(&a, s);
    else if (a.f.opts == 0)
        responder_kernel<false><<<dim3(1), dim3(kLfThreads), 0, s>>>(a);
    else
        responder_kernel<true><<<dim3(1), dim3(kLfThreads), 0, s>>>(a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int responder_queues_launch(const uint8_t* d_block, uint32_t n_queues, uint32_t opts, hipStream_t s) {
    if (opts & XSK_GPU_OPT_IPV6)
        xsk_gpu__responder_queues_ds_launch(d_block, n_queues, opts, s);
    else if (opts == 0)
        responder_queues_kernel<false><<<dim3(n_queues), dim3(kLfThreads), 0, s>>>(d_block, n_queues, opts);
    else
        responder_queues_kernel<true><<<dim3(n_queues), dim3(kLfThreads), 0, s>>>(d_block, n_queues, opts);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int xsk_gpu_responder_dev(const struct xsk_gpu_responder_queue* r, uint32_t opts, void* stream) {
    if (!responder_ok(r, opts)) return -EINVAL;
    ResponderArgs a;
    memset((void*)&a, 0, sizeof a);
    pack_responder(*r, opts, a);
    return responder_launch(a, (hipStream_t)stream);
}

size_t xsk_gpu_responder_block_size(uint32_t n_queues) { return rs_block_size(n_queues); }

int xsk_gpu_responder_prepare(const struct xsk_gpu_responder_queue* queues, uint32_t n_queues, uint32_t opts,
                              void* h_block) {
    if (!queues || !h_block || !rs_count_ok(n_queues)) return -EINVAL;
    for (uint32_t k = 0; k < n_queues; ++k)
        if (!responder_ok(queues + k, opts)) return -EINVAL;
    try {
        if (!responders_disjoint(queues, n_queues)) return -EINVAL;
    } catch (const std::bad_alloc&) {
        return -ENOMEM;
    }
    rs_write_block<ResponderArgs>((uint8_t*)h_block, n_queues, opts,
                                  [&](uint32_t k, ResponderArgs& a) { pack_responder(queues[k], opts, a); });
    return 0;
}

int xsk_gpu_responder_queues_dev(const void* d_block, uint32_t n_queues, uint32_t opts, void* stream) {
    if (!d_block || ((uintptr_t)d_block & (kRsAlign - 1u)) || !rs_count_ok(n_queues) || (opts & ~XSK_GPU_OPT_MASK))
        return -EINVAL;
    return responder_queues_launch((const uint8_t*)d_block, n_queues, opts, (hipStream_t)stream);
}

}  // extern "C"
