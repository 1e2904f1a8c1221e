// xsk_rx_queues.hip — xsk_gpu_rx_queues_dev(): the fused loop body (xsk_loop_fused_body.h) for Q independent RX queues
// as ONE launch of Q workgroups, one queue per workgroup (include/xsk_gpu.h).  The queues share nothing
// a kernel writes and no workgroup waits for another, so the grid is Q times the one-workgroup kernel of
// xsk_gpu_rx_fused_loop_dev(), on Q CUs.  What does not fit is the argument segment: one queue's LoopFusedArgs is
// 3448 B, with the hidden arguments 3704 B of its 4096 B, so the records live in device memory in a block that
// xsk_gpu_rx_queues_prepare() writes on the host (xsk_rx_queues.h), and workgroup q stages record q into LDS before it
// calls the body, unchanged.  The reference-mode and wire-mode instances are here, the dual-stack one in xsk_rx_queues_ds.hip.  A file of its own: no
// existing translation unit's kernels change.
//
// One 1024-thread workgroup a CU: the body's LDS and the staged record are above half of a CU's 160 KiB.  No MFMA.
#include <errno.h>

#include <algorithm>
#include <new>
#include <utility>
#include <vector>

#include "xsk_gpu_internal.h"
#include "xsk_hip_util.h"
#include "xsk_loop_fused_body.h"
#include "xsk_rx_queues.h"

using namespace xskgpu;

namespace {

using QueuesLds = RqLds<LoopFusedLds, LoopFusedArgs>;
static_assert(sizeof(QueuesLds) <= 160u * 1024u, "the CU's LDS: the loop body's and the staged record");
static_assert(sizeof(QueuesLds) > 80u * 1024u, "and one workgroup a CU, as the launch bounds say");
// the record's layout as xsk_rx_queues.h states it for the host
static_assert(sizeof(LoopFusedArgs) == kRqRecordBytes && alignof(LoopFusedArgs) <= 16, "a record");
static_assert(offsetof(LoopFusedArgs, tx) == kRqTxOff && offsetof(LoopFusedArgs, comp) == kRqCompOff &&
                  offsetof(LoopFusedArgs, rx) == kRqRxOff && offsetof(LoopFusedArgs, fill) == kRqFillOff &&
                  offsetof(LoopFusedArgs, stack) == kRqStackOff,
              "the packed rings of a record");
static_assert(kRqTxPorts == kEpMaxPorts && kRqCompRings == kRcMaxRings, "and their counts");

template <bool WIRE>
__global__ __launch_bounds__(kLfThreads, 1) void rx_queues_kernel(const uint8_t* block, uint32_t n_queues, uint32_t opts) {
    __shared__ QueuesLds M;
    if (!rq_stage(block, n_queues, opts, M.S)) return;  // workgroup-uniform, before the first store
    loop_fused_body<RoundCfg<WIRE, true>>(M.S.a, M.L);
}

// ---- the argument rules of one queue: every rule of xsk_gpu_rx_fused_loop_dev() ----
bool packable(const xsk_gpu_ring_dev* r) { return !r || pk_packable((uint64_t)(uintptr_t)r->d_ring, r->size); }

// fused_ok() of xsk_loop_fused.hip stated again (that file keeps its own: a test reads it there): the loop call's rules
// through the loop call's function, the two bounds of the one-workgroup form, a ring the packed form cannot carry.
bool queue_ok(const xsk_gpu_rx_queue& q, uint32_t opts) {
    if (!loop_complete_ok(q.d_umem, q.umem_size, q.rx, q.fill, q.tx, q.stack, q.pool, q.max_batch, opts, q.d_table,
                          q.n_entries, q.default_port, q.n_ports, q.d_bound, q.d_port_counts, q.d_stats, q.d_port_stats,
                          q.d_res, q.comp, q.n_comp, q.complete_max, q.d_moved, q.d_pushed, q.d_workspace))
        return false;
    if (q.max_batch > kLfMax || (q.n_comp && q.complete_max > kLfMax)) return false;
    if (!packable(q.rx) || !packable(q.fill) || !packable(q.stack)) return false;
    for (uint32_t p = 0; p < q.n_ports; ++p)
        if (!packable(q.tx + p)) return false;
    for (uint32_t c = 0; c < q.n_comp; ++c)
        if (!packable(q.comp + c)) return false;
    return true;
}

// ---- no two queues share a pointer a kernel writes through ----
using Owned = std::pair<uintptr_t, uint32_t>;  // the pointer, the queue

void own(std::vector<Owned>& v, const void* p, uint32_t q) {
    if (p) v.emplace_back((uintptr_t)p, q);
}
void own_ring(std::vector<Owned>& v, const xsk_gpu_ring_dev* r, uint32_t q) {
    own(v, r->d_ring, q);
    own(v, r->d_producer, q);
    own(v, r->d_consumer, q);
}
// Every queue has passed queue_ok().  Sorted by pointer, then by queue: two queues that hold the same pointer stand
// next to each other (what one queue may hold twice is that queue's own rules' business).
void queue_owned(std::vector<Owned>& v, const xsk_gpu_rx_queue& q, uint32_t k) {
    own_ring(v, q.rx, k);
    own_ring(v, q.fill, k);
    if (q.stack) own_ring(v, q.stack, k);
    for (uint32_t p = 0; p < q.n_ports; ++p) own_ring(v, q.tx + p, k);
    for (uint32_t c = 0; c < q.n_comp; ++c) own_ring(v, q.comp + c, k);
    own(v, q.pool->d_addr, k);
    own(v, q.pool->d_n_free, k);
    own(v, q.d_workspace, k);
    own(v, q.d_actions, k);
    own(v, q.d_ports, k);
    own(v, q.d_port_counts, k);
    own(v, q.d_stats, k);
    own(v, q.d_port_stats, k);
    own(v, q.d_res, k);
    if (q.n_comp) {  // (ignored without completion rings, as the fused call ignores them)
        own(v, q.d_moved, k);
        own(v, q.d_pushed, k);
    }
}
bool queues_disjoint(const xsk_gpu_rx_queue* queues, uint32_t n_queues) {
    std::vector<Owned> v;
    for (uint32_t k = 0; k < n_queues; ++k) queue_owned(v, queues[k], k);
    std::sort(v.begin(), v.end());
    for (size_t i = 1; i < v.size(); ++i)
        if (v[i].first == v[i - 1].first && v[i].second != v[i - 1].second) return false;
    return true;
}

// One queue's record, exactly as xsk_gpu_rx_fused_loop_dev() packs its own; `a` arrives as zero bytes and the structs
// with padding are filled in member by member, so that a block is the same bytes on every call.
void pack_queue(const xsk_gpu_rx_queue& q, uint32_t opts, LoopFusedArgs& a) {
    for (uint32_t p = 0; p < kEpMaxPorts; ++p) a.tx[p] = lf_pack(p < q.n_ports ? q.tx + p : nullptr);
    for (uint32_t c = 0; c < kRcMaxRings; ++c) a.comp[c] = lf_pack(c < q.n_comp ? q.comp + c : nullptr);
    a.rx = lf_pack(q.rx);
    a.fill = lf_pack(q.fill);
    a.stack = lf_pack(q.stack);
    const Pool pool = pool_of(q.pool);
    a.pool.addr = pool.addr;
    a.pool.n_free = pool.n_free;
    a.pool.capacity = pool.capacity;
    a.umem = (uint8_t*)q.d_umem;
    a.umem_size = q.umem_size;
    a.table = q.d_table;
    a.d_bound = q.d_bound;
    a.d_actions = q.d_actions;
    a.d_ports = q.d_ports;
    a.d_port_counts = q.d_port_counts;
    a.d_stats = q.d_stats;
    a.d_port_stats = q.d_port_stats;
    a.d_res = q.d_res;
    a.d_moved = q.d_moved;
    a.d_pushed = q.d_pushed;
    a.ws = (uint8_t*)q.d_workspace;
    a.l = ps_layout(q.max_batch, q.n_ports, xsk_gpu_steer_workspace_size(q.max_batch, q.n_ports),
                    xsk_gpu_egress_ports_workspace_size(q.max_batch, q.n_ports));
    a.max_batch = q.max_batch;
    a.opts = opts;
    a.n_entries = q.n_entries;
    a.default_port = q.default_port;
    a.n_ports = q.n_ports;
    a.n_comp = q.n_comp;
    a.complete_max = q.complete_max;
}

// The one launch, behind the checks: the instance is chosen as xsk_gpu_rx_fused_loop_dev() chooses its own.
int queues_launch(const uint8_t* d_block, uint32_t n_queues, uint32_t opts, hipStream_t s) {
    if (opts & XSK_GPU_OPT_IPV6)
        xsk_gpu__rx_queues_ds_launch(d_block, n_queues, opts, s);
    else if (opts == 0)
        rx_queues_kernel<false><<<dim3(n_queues), dim3(kLfThreads), 0, s>>>(d_block, n_queues, opts);
    else
        rx_queues_kernel<true><<<dim3(n_queues), dim3(kLfThreads), 0, s>>>(d_block, n_queues, opts);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

// For xsk_responder.hip (xsk_gpu_internal.h): one queue's rules, its record and what it owns, each stated once, here.
extern "C" int xsk_gpu__rxq_ok(const struct xsk_gpu_rx_queue* q, uint32_t opts) { return queue_ok(*q, opts) ? 1 : 0; }
extern "C" void xsk_gpu__rxq_pack(const struct xsk_gpu_rx_queue* q, uint32_t opts, void* args) {
    pack_queue(*q, opts, *(LoopFusedArgs*)args);
}
extern "C" uint32_t xsk_gpu__rxq_owned(const struct xsk_gpu_rx_queue* q, const void** out) {
    std::vector<Owned> v;
    queue_owned(v, *q, 0u);
    for (size_t i = 0; i < v.size(); ++i) out[i] = (const void*)v[i].first;
    return (uint32_t)v.size();
}

extern "C" {

size_t xsk_gpu_rx_queues_block_size(uint32_t n_queues) { return rq_block_size(n_queues); }

int xsk_gpu_rx_queues_prepare(const struct xsk_gpu_rx_queue* queues, uint32_t n_queues, uint32_t opts, void* h_block) {
    if (!queues || !h_block || !rq_count_ok(n_queues)) return -EINVAL;
    for (uint32_t k = 0; k < n_queues; ++k)
        if (!queue_ok(queues[k], opts)) return -EINVAL;
    try {
        if (!queues_disjoint(queues, n_queues)) return -EINVAL;
    } catch (const std::bad_alloc&) {
        return -ENOMEM;
    }
    rq_write_block<LoopFusedArgs>((uint8_t*)h_block, n_queues, opts,
                                  [&](uint32_t k, LoopFusedArgs& a) { pack_queue(queues[k], opts, a); });
    return 0;
}

int xsk_gpu_rx_queues_dev(const void* d_block, uint32_t n_queues, uint32_t opts, void* stream) {
    if (!d_block || ((uintptr_t)d_block & (kRqAlign - 1u)) || !rq_count_ok(n_queues) || (opts & ~XSK_GPU_OPT_MASK))
        return -EINVAL;
    return queues_launch((const uint8_t*)d_block, n_queues, opts, (hipStream_t)stream);
}

}  // extern "C"
