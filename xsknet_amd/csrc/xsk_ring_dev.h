// xsk_ring_dev.h — the arithmetic of xsk_gpu_rx_begin_dev(), xsk_gpu_rx_end_dev(), xsk_gpu_rx_step_dev() and
// xsk_gpu_tx_complete_dev() (include/xsk_gpu.h): what a ring holds and has room for, what one step
// decides from the index words, which entry every lane copies, and the grid and workspace sizes.  Host and device:
// xsk_ring_dev.hip's kernels and its host launch call these functions, and tests/c/test_ring_dev.cpp replays both paths
// with them on the CPU, into heap arrays of exactly the rings' sizes under AddressSanitizer.
//
// The rules are those of xsk_ring.h with the cached indices left out (the device reads the real words) and two clamps
// that make them total for any content of the words:
//   used(r) = min((producer - consumer) mod 2^32, size),  free(r) = size - used(r);  pool_n = min(*d_n_free, capacity).
// Entry i of a ring lives at ring[i & (size - 1)], entry j of the pool at d_addr[j], j < capacity.
#ifndef XSK_RING_DEV_H
#define XSK_RING_DEV_H

#include <stddef.h>
#include <stdint.h>

#include "xsk_egress.h"

#ifdef __HIPCC__
#define XSK_RD_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define XSK_RD_FN static inline
#endif

namespace xskgpu {

constexpr uint32_t kRdSmallMax = 1024;  // == XSK_GPU_LOWLAT_MAX: one launch of one workgroup up to here
constexpr uint32_t kRdSmallThreads = 1024;
constexpr uint32_t kRdWave = 64;        // the one-wave plan and publish launches
constexpr uint32_t kRdCopy = 256;       // entries (and threads) per workgroup of the copy launch
constexpr uint32_t kRdMaxSize = 0x80000000u;

XSK_RD_FN uint32_t rd_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// size is a power of two in [1, 2^31]
XSK_RD_FN bool rd_size_ok(uint32_t size) { return size != 0u && (size & (size - 1u)) == 0u && size <= kRdMaxSize; }

XSK_RD_FN uint32_t rd_used(uint32_t prod, uint32_t cons, uint32_t size) { return rd_min(prod - cons, size); }
XSK_RD_FN uint32_t rd_free(uint32_t prod, uint32_t cons, uint32_t size) { return size - rd_used(prod, cons, size); }
XSK_RD_FN uint32_t rd_pool_n(uint32_t word, uint32_t capacity) { return rd_min(word, capacity); }
XSK_RD_FN uint32_t rd_slot(uint32_t idx, uint32_t size) { return idx & (size - 1u); }

// The index and count words one launch reads, as read.
struct RdWords {
    uint32_t prod, cons;
};

struct RdPlan {  // == struct xsk_gpu_rx_plan
    uint32_t received, tx_room, refilled, rx_cons, fq_prod, pool_n, reserved[2];
};

// ---- begin: steps 1 and 2 of xsk_gpu_rx_step() ----
// rcvd = min(used(rx), max_batch); nothing received: nothing refilled (the host step returns before its refill).
// Otherwise stock = min(free(fill), pool_n), the LIFO pop of xsk_gpu__rx_refill().  tx_room = free(tx) either way.
XSK_RD_FN RdPlan rd_begin_plan(RdWords rx, uint32_t rx_size, RdWords fill, uint32_t fill_size, RdWords tx,
                               uint32_t tx_size, uint32_t pool_word, uint32_t capacity, uint32_t max_batch) {
    RdPlan p;
    p.received = rd_min(rd_used(rx.prod, rx.cons, rx_size), max_batch);
    p.tx_room = rd_free(tx.prod, tx.cons, tx_size);
    p.pool_n = rd_pool_n(pool_word, capacity);
    p.refilled = p.received ? rd_min(rd_free(fill.prod, fill.cons, fill_size), p.pool_n) : 0u;
    p.rx_cons = rx.cons;
    p.fq_prod = fill.prod;
    p.reserved[0] = p.reserved[1] = 0u;
    return p;
}
// d_descs[i] = RX entry rd_slot(rx_cons + i) for i < received; fill entry rd_slot(fq_prod + i) = d_addr[rd_pop(i)] for
// i < refilled.  pool_n - 1 - i lies in [0, capacity) because i < refilled <= pool_n <= capacity.
XSK_RD_FN uint32_t rd_pop(uint32_t pool_n, uint32_t i) { return pool_n - 1u - i; }
// What begin leaves in the fill ring's producer word and in the pool's count.
XSK_RD_FN uint32_t rd_begin_fq_prod(const RdPlan& p) { return p.fq_prod + p.refilled; }
XSK_RD_FN uint32_t rd_begin_pool_n(const RdPlan& p) { return p.pool_n - p.refilled; }

// ---- end: the ring half of step 4, and step 5 ----
struct RdEnd {
    uint32_t n_tx;     // TX entry rd_slot(tx_prod + k) = d_tx[k] for k < n_tx
    uint32_t pushed;   // d_addr[pool_n + j] = d_free[j] for j < pushed; pool_n + pushed <= capacity
    uint32_t release;  // the RX consumer word's advance
    uint32_t tx_prod, pool_n;
};
XSK_RD_FN RdEnd rd_end_plan(uint32_t c_n_tx, uint32_t c_n_free, uint32_t n_max, RdWords tx, uint32_t tx_size,
                            uint32_t pool_word, uint32_t capacity, uint32_t received) {
    RdEnd e;
    e.tx_prod = tx.prod;
    e.pool_n = rd_pool_n(pool_word, capacity);
    e.n_tx = rd_min(rd_min(c_n_tx, n_max), rd_free(tx.prod, tx.cons, tx_size));
    e.pushed = rd_min(rd_min(c_n_free, n_max), capacity - e.pool_n);
    e.release = rd_min(received, n_max);
    return e;
}

// ---- tx_complete: xsk_gpu_tx_complete() ----
struct RdComplete {
    uint32_t n;       // the consumer word's advance
    uint32_t pushed;  // d_addr[pool_n + j] = completion entry rd_slot(cons + j) for j < pushed
    uint32_t cons, pool_n;
};
XSK_RD_FN RdComplete rd_complete_plan(RdWords comp, uint32_t size, uint32_t max, uint32_t pool_word,
                                      uint32_t capacity) {
    RdComplete c;
    c.cons = comp.cons;
    c.pool_n = rd_pool_n(pool_word, capacity);
    c.n = rd_min(rd_used(comp.prod, comp.cons, size), max);
    c.pushed = rd_min(c.n, capacity - c.pool_n);
    return c;
}

// ---- the copy launch of the larger bounds: lane `lane` of workgroup `wg` of a grid of `nwg` copies the entries
// first, first + stride, ... below the count (a count above the grid's span is walked in strides: the fill ring's
// refill is bounded by the ring and the pool, not by max_batch) ----
XSK_RD_FN uint32_t rd_nwg(uint32_t n_max) { return n_max / kRdCopy + (n_max % kRdCopy ? 1u : 0u); }
XSK_RD_FN uint64_t rd_copy_first(uint32_t wg, uint32_t lane) { return (uint64_t)wg * kRdCopy + lane; }
XSK_RD_FN uint64_t rd_copy_stride(uint32_t nwg) { return (uint64_t)nwg * kRdCopy; }

// ---- the workspace of xsk_gpu_rx_step_dev(max_batch): the plan, the egress counts, then the batch's descriptors, TX
// list, free list, verdicts and the egress call's own workspace; every offset a multiple of the alignment its array
// needs (16, 16, 8, 1, 4) given a 16-B aligned base ----
XSK_RD_FN size_t rd_align(size_t x, size_t a) { return (x + a - 1u) / a * a; }
struct RdLayout {
    size_t plan, counts, descs, tx, free_list, verdicts, egress, bytes;
};
XSK_RD_FN RdLayout rd_layout(uint32_t max_batch) {
    RdLayout l;
    l.plan = 0;                                       // 32 B
    l.counts = 32;                                    // 16 B
    l.descs = 48;
    l.tx = l.descs + (size_t)max_batch * 16u;
    l.free_list = l.tx + (size_t)max_batch * 16u;
    l.verdicts = l.free_list + (size_t)max_batch * 8u;
    l.egress = rd_align(l.verdicts + (size_t)max_batch, 4u);
    l.bytes = rd_align(l.egress + eg_workspace_bytes(max_batch), 16u);
    return l;
}

}  // namespace xskgpu

#endif  // XSK_RING_DEV_H
