// xsk_responder_block.h — the argument block of xsk_gpu_responder_queues_dev() (include/xsk_gpu.h): the
// sibling of xsk_rx_queues.h.  A 64-B header and behind it one record per queue, the responder kernel's ResponderArgs
// (xsk_responder_body.h) exactly as xsk_gpu_responder_dev() packs its own: the fused loop kernel's 3448-B record, then
// the packed `up` ring, three pointers and two words -- 3504 B, with the 256 B of hidden arguments 3760 B of the 4096 B
// an argument segment holds -- at a stride rounded up to 64 B.  The header has the words of xsk_rx_queues.h's in the
// same places and a magic word of its own, so either kernel finds the other's block foreign and returns before its
// first store.  Host and device, and plain C++ for the host: tests/c/test_responder.cpp replays the layout, the writer
// and the header check on the CPU.  The record's own type is not named here; xsk_responder.hip asserts its size and the
// places of its rings against the struct.
#ifndef XSK_RESPONDER_BLOCK_H
#define XSK_RESPONDER_BLOCK_H

#include <stdint.h>
#include <string.h>

#include "../../include/xsk_gpu.h"
#include "xsk_ring_pack.h"
#include "xsk_rx_queues.h"

namespace xskgpu {

constexpr uint32_t kRsMagic = 0x50525358u;  // "XSRP", little-endian
static_assert(kRsMagic != kRqMagic, "a block of one call is foreign to the other");
constexpr uint32_t kRsHeaderBytes = kRqHeaderBytes;
constexpr uint32_t kRsAlign = kRqAlign;
constexpr uint32_t kRsUpOff = kRqRecordBytes;  // the packed `up` ring, behind the loop body's record
constexpr uint32_t kRsRecordBytes = kRqRecordBytes + (uint32_t)sizeof(PackedRing) + 3u * 8u + 2u * 4u;  // 3504
constexpr uint32_t kRsStride = (kRsRecordBytes + kRsAlign - 1u) / kRsAlign * kRsAlign;                   // 3520
constexpr uint32_t kRsVecs = kRsStride / 16u;
constexpr uint32_t kRsMaxQueues = XSK_GPU_RX_MAX_QUEUES;
constexpr uint32_t kRsRings = kRqRings + 1u;  // tx[0..64), comp[0..65), rx, fill, stack, up
static_assert(kRsStride % kRsAlign == 0 && kRsStride >= kRsRecordBytes && kRsStride % 16u == 0, "the stride");
static_assert(kRsRecordBytes + 256u <= 4096u, "a record is what the one-queue call passes as kernel arguments");
static_assert(kRqRings * sizeof(PackedRing) <= kRsUpOff && kRsUpOff + sizeof(PackedRing) <= kRsRecordBytes,
              "the rings lie inside a record");

XSK_RQ_FN bool rs_count_ok(uint32_t n_queues) { return n_queues >= 1u && n_queues <= kRsMaxQueues; }
XSK_RQ_FN size_t rs_block_size(uint32_t n_queues) {
    return rs_count_ok(n_queues) ? (size_t)kRsHeaderBytes + (size_t)n_queues * kRsStride : (size_t)0;
}
XSK_RQ_FN size_t rs_record_off(uint32_t q) { return (size_t)kRsHeaderBytes + (size_t)q * kRsStride; }

XSK_RQ_FN RqHeader rs_header(uint32_t n_queues, uint32_t opts) {
    RqHeader h = rq_header(n_queues, opts);
    h.magic = kRsMagic;
    h.stride = kRsStride;
    h.record_bytes = kRsRecordBytes;
    return h;
}

// What every workgroup asks of the header before its first store, as rq_header_ok().
XSK_RQ_FN bool rs_header_ok(uint32_t magic, uint32_t abi_version, uint32_t h_queues, uint32_t h_opts, uint32_t stride,
                            uint32_t record_bytes, uint32_t n_queues, uint32_t opts) {
    return magic == kRsMagic && abi_version == (uint32_t)XSK_GPU_ABI_VERSION && h_queues == n_queues && h_opts == opts &&
           stride == kRsStride && record_bytes == kRsRecordBytes;
}

// The block of n_queues records, as rq_write_block(): nothing outside [0, rs_block_size(n_queues)) is written.
template <class Rec, class One>
inline void rs_write_block(uint8_t* block, uint32_t n_queues, uint32_t opts, One one) {
    static_assert(sizeof(Rec) == kRsRecordBytes, "a record");
    const RqHeader h = rs_header(n_queues, opts);
    memcpy(block, &h, sizeof h);
    for (uint32_t q = 0; q < n_queues; ++q) {
        uint8_t* const at = block + rs_record_off(q);
        Rec r;
        memset((void*)&r, 0, sizeof r);
        one(q, r);
        memcpy(at, &r, sizeof r);
        memset(at + sizeof r, 0, kRsStride - sizeof r);
    }
}

// Ring k of a record in a block, for the replay and the tests: k counts as kRsRings does.
inline PackedRing rs_ring_at(const uint8_t* block, uint32_t q, uint32_t k) {
    PackedRing p;
    const size_t off = k < kRqRings ? kRqTxOff + (size_t)k * sizeof(PackedRing) : (size_t)kRsUpOff;
    memcpy(&p, block + rs_record_off(q) + off, sizeof p);
    return p;
}

#ifdef __HIPCC__
// ---- the kernel's side: workgroup blockIdx.x checks the header, then brings its record into LDS, as rq_stage() ----
template <class Rec>
union RsArgsLds {
    uint4 v[kRsVecs];
    Rec a;
};
template <class Lds, class Rec>
struct RsLds {
    Lds L;
    RsArgsLds<Rec> S;
};

// Every lane of the workgroup calls it.  false -- for the whole workgroup, and before any store -- when the block's
// header does not match the call; true behind a barrier with record blockIdx.x in S.  Only the header's first 24 bytes
// are read; the stride is the kernel's own constant, never a word of the block.
template <class Rec>
__device__ __forceinline__ bool rs_stage(const uint8_t* block, uint32_t n_queues, uint32_t opts, RsArgsLds<Rec>& S) {
    static_assert(sizeof(Rec) == kRsRecordBytes && sizeof(RsArgsLds<Rec>) == kRsStride, "a record, padded to the stride");
    const uint4 h0 = *reinterpret_cast<const uint4*>(block);
    const uint2 h1 = *reinterpret_cast<const uint2*>(block + 16);
    const uint32_t q = blockIdx.x;
    if (!rs_header_ok(h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, n_queues, opts) || q >= n_queues) return false;
    const uint4* const src = reinterpret_cast<const uint4*>(block + rs_record_off(q));
    for (uint32_t k = threadIdx.x; k < kRsVecs; k += blockDim.x) S.v[k] = src[k];
    __syncthreads();
    return true;
}
#endif  // __HIPCC__

}  // namespace xskgpu

#endif  // XSK_RESPONDER_BLOCK_H
