// xsk_rx_queues.h — the argument block of xsk_gpu_rx_queues_dev() (include/xsk_gpu.h): a 64-B header
// and behind it one record per RX queue, the fused loop kernel's LoopFusedArgs (xsk_loop_fused_body.h) exactly as
// xsk_gpu_rx_fused_loop_dev() packs its own, at a stride rounded up to 64 B.  One queue's record is 3448 B -- with the
// 256 B of hidden arguments behind it, 3704 B of the 4096 B an argument segment holds -- so the records of Q queues live
// in device memory: xsk_gpu_rx_queues_prepare() writes the block on the host, the caller copies it once, and workgroup q
// of the kernel checks the header and brings record q into LDS.  Host and device, and plain C++ for the host: the layout, the header, the check every workgroup makes in
// front of its first store (rq_header_ok) and the writer of a block (rq_write_block) are what tests/c/test_rx_queues.cpp
// replays on the CPU.  The record's own type is not named here (its header needs the device compiler); its size and the
// places of its rings are, and xsk_rx_queues.hip asserts them against the struct.
#ifndef XSK_RX_QUEUES_H
#define XSK_RX_QUEUES_H

#include <stdint.h>
#include <string.h>

#include "../../include/xsk_gpu.h"
#include "xsk_ring_pack.h"

#ifdef __HIPCC__
#define XSK_RQ_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define XSK_RQ_FN static inline
#endif

namespace xskgpu {

constexpr uint32_t kRqMagic = 0x51525358u;   // "XSRQ", little-endian
constexpr uint32_t kRqHeaderBytes = 64;
constexpr uint32_t kRqAlign = 64;            // of the block, the header and every record
constexpr uint32_t kRqRecordBytes = 3448;    // sizeof(LoopFusedArgs)
constexpr uint32_t kRqStride = (kRqRecordBytes + kRqAlign - 1u) / kRqAlign * kRqAlign;  // 3456
constexpr uint32_t kRqVecs = kRqStride / 16u;  // a record as the kernel loads it: 216 loads of 16 B
constexpr uint32_t kRqMaxQueues = XSK_GPU_RX_MAX_QUEUES;
// the packed rings of a record (LoopFusedArgs begins with them): tx[64], comp[65], rx, fill, stack
constexpr uint32_t kRqTxPorts = XSK_GPU_STEER_MAX_PORTS, kRqCompRings = XSK_GPU_COMPLETE_MAX_RINGS;
constexpr uint32_t kRqTxOff = 0;
constexpr uint32_t kRqCompOff = kRqTxOff + kRqTxPorts * (uint32_t)sizeof(PackedRing);
constexpr uint32_t kRqRxOff = kRqCompOff + kRqCompRings * (uint32_t)sizeof(PackedRing);
constexpr uint32_t kRqFillOff = kRqRxOff + (uint32_t)sizeof(PackedRing);
constexpr uint32_t kRqStackOff = kRqFillOff + (uint32_t)sizeof(PackedRing);
static_assert(kRqStride % kRqAlign == 0 && kRqStride >= kRqRecordBytes && kRqStride % 16u == 0, "the stride");
static_assert(kRqStackOff + sizeof(PackedRing) <= kRqRecordBytes, "the rings lie inside a record");

struct RqHeader {  // 64 B, the block's first bytes
    uint32_t magic, abi_version, n_queues, opts, stride, record_bytes;
    uint32_t zero[10];
};
static_assert(sizeof(RqHeader) == kRqHeaderBytes, "the header");

XSK_RQ_FN bool rq_count_ok(uint32_t n_queues) { return n_queues >= 1u && n_queues <= kRqMaxQueues; }
XSK_RQ_FN size_t rq_block_size(uint32_t n_queues) {
    return rq_count_ok(n_queues) ? (size_t)kRqHeaderBytes + (size_t)n_queues * kRqStride : (size_t)0;
}
XSK_RQ_FN size_t rq_record_off(uint32_t q) { return (size_t)kRqHeaderBytes + (size_t)q * kRqStride; }

XSK_RQ_FN RqHeader rq_header(uint32_t n_queues, uint32_t opts) {
    RqHeader h;
    h.magic = kRqMagic;
    h.abi_version = XSK_GPU_ABI_VERSION;
    h.n_queues = n_queues;
    h.opts = opts;
    h.stride = kRqStride;
    h.record_bytes = kRqRecordBytes;
    for (uint32_t k = 0; k < 10u; ++k) h.zero[k] = 0u;
    return h;
}

// What every workgroup asks of the header before its first store: the block was prepared by this version of the
// library, for this many queues and these options, at the layout this kernel was built for.  The words are taken one by
// one, so that the kernel passes what it loaded.
XSK_RQ_FN bool rq_header_ok(uint32_t magic, uint32_t abi_version, uint32_t h_queues, uint32_t h_opts, uint32_t stride,
                            uint32_t record_bytes, uint32_t n_queues, uint32_t opts) {
    return magic == kRqMagic && abi_version == (uint32_t)XSK_GPU_ABI_VERSION && h_queues == n_queues && h_opts == opts &&
           stride == kRqStride && record_bytes == kRqRecordBytes;
}

// The block of n_queues records (the caller has checked the count): the header, then record q as one(q, record) fills
// it in -- into a record of zero bytes, so that the struct's padding is zero in the block -- and the bytes between a
// record's end and the next one's start zeroed.  Rec is LoopFusedArgs in the library and a stand-in of the same size in
// the CPU replay; nothing outside [0, rq_block_size(n_queues)) is written.
template <class Rec, class One>
inline void rq_write_block(uint8_t* block, uint32_t n_queues, uint32_t opts, One one) {
    static_assert(sizeof(Rec) == kRqRecordBytes, "a record");
    const RqHeader h = rq_header(n_queues, opts);
    memcpy(block, &h, sizeof h);
    for (uint32_t q = 0; q < n_queues; ++q) {
        uint8_t* const at = block + rq_record_off(q);
        Rec r;
        memset((void*)&r, 0, sizeof r);
        one(q, r);
        memcpy(at, &r, sizeof r);
        memset(at + sizeof r, 0, kRqStride - sizeof r);
    }
}

// Ring k of a record in a block, for the replay and the tests: k counts tx[0..64), comp[0..65), rx, fill, stack.
constexpr uint32_t kRqRings = kRqTxPorts + kRqCompRings + 3u;
inline PackedRing rq_ring_at(const uint8_t* block, uint32_t q, uint32_t k) {
    PackedRing p;
    memcpy(&p, block + rq_record_off(q) + kRqTxOff + (size_t)k * sizeof(PackedRing), sizeof p);
    return p;
}

#ifdef __HIPCC__
// ---- the kernel's side: workgroup blockIdx.x checks the header, then brings its record into LDS ----
// A record in LDS, as the 16-B vectors it is loaded in and as the struct the loop body reads.
template <class Rec>
union RqArgsLds {
    uint4 v[kRqVecs];
    Rec a;
};
// The workgroup's LDS: the loop body's own, and the staged record beside it.
template <class Lds, class Rec>
struct RqLds {
    Lds L;
    RqArgsLds<Rec> S;
};

// Every lane of the workgroup calls it.  false -- for the whole workgroup, and before any store -- when the block's
// header does not match the call; true behind a barrier with record blockIdx.x in S.  The block is 64-B aligned and so
// is every record (the host checks the pointer, the layout does the rest): 16-B loads, the lanes striding the record.
// The stride is the kernel's own constant, never a word of the block.
template <class Rec>
__device__ __forceinline__ bool rq_stage(const uint8_t* block, uint32_t n_queues, uint32_t opts, RqArgsLds<Rec>& S) {
    static_assert(sizeof(Rec) == kRqRecordBytes && sizeof(RqArgsLds<Rec>) == kRqStride, "a record, padded to the stride");
    const uint4 h0 = *reinterpret_cast<const uint4*>(block);
    const uint2 h1 = *reinterpret_cast<const uint2*>(block + 16);
    const uint32_t q = blockIdx.x;
    if (!rq_header_ok(h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, n_queues, opts) || q >= n_queues) return false;
    const uint4* const src = reinterpret_cast<const uint4*>(block + rq_record_off(q));
    for (uint32_t k = threadIdx.x; k < kRqVecs; k += blockDim.x) S.v[k] = src[k];
    __syncthreads();
    return true;
}
#endif  // __HIPCC__

}  // namespace xskgpu

#endif  // XSK_RX_QUEUES_H
