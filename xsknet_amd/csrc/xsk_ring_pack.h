// xsk_ring_pack.h — a ring's three pointers and its size in 24 bytes, as xsk_gpu_rx_fused_loop_dev()'s kernel takes
// its up to 132 rings (include/xsk_gpu.h).  64 TX rings and 65 completion rings at the 32 B of the
// kernels' own Ring are 4128 B, more than the 4096 B a kernel's argument segment holds; packed they are 3096 B, and
// rx, fill and the stack ring travel the same way.  A size is a power of two (rd_size_ok), so its log2 is all of it: it
// rides in the top byte of the entry array's pointer, which no address of this platform uses (an address is below 2^56;
// pk_packable() says so, and the call refuses what is not).  Host and device: the host packs when the call is made, the
// kernel's first act is to unpack into LDS, and tests/c/test_loop_fused.cpp round-trips both on the CPU.
#ifndef XSK_RING_PACK_H
#define XSK_RING_PACK_H

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define XSK_PK_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define XSK_PK_FN static inline
#endif

namespace xskgpu {

constexpr uint32_t kPkWords = 6;          // 24 B, 4-B aligned: 132 of them are 3168 B
constexpr uint32_t kPkPtrBits = 56;       // the entry array's address is below 2^56
constexpr uint32_t kPkMaxLog2 = 31;       // rd_size_ok: a size is at most 2^31

struct PackedRing {
    uint32_t w[kPkWords];  // prod lo, hi; cons lo, hi; ring lo; ring hi | log2(size) << 24
};
static_assert(sizeof(PackedRing) == 24, "the packed form");

struct UnpackedRing {  // what the kernels' Ring holds, as integers (the host replay has no device pointers)
    uint64_t prod, cons, ring;
    uint32_t size;
};

XSK_PK_FN uint32_t pk_log2(uint32_t size) {  // of a power of two; 0 for 0, which rd_size_ok refuses anyway
    uint32_t l = 0;
    while (l < kPkMaxLog2 && (1u << l) < size) ++l;
    return l;
}

// What the packed form can carry: a power-of-two size and an entry array below 2^56.
XSK_PK_FN bool pk_packable(uint64_t ring, uint32_t size) {
    return size != 0u && (size & (size - 1u)) == 0u && (ring >> kPkPtrBits) == 0u;
}

XSK_PK_FN PackedRing pk_pack(uint64_t prod, uint64_t cons, uint64_t ring, uint32_t size) {
    PackedRing p;
    p.w[0] = (uint32_t)prod;
    p.w[1] = (uint32_t)(prod >> 32);
    p.w[2] = (uint32_t)cons;
    p.w[3] = (uint32_t)(cons >> 32);
    p.w[4] = (uint32_t)ring;
    p.w[5] = ((uint32_t)(ring >> 32) & 0x00FFFFFFu) | (pk_log2(size) << 24);
    return p;
}

XSK_PK_FN UnpackedRing pk_unpack(const PackedRing& p) {
    UnpackedRing u;
    u.prod = ((uint64_t)p.w[1] << 32) | p.w[0];
    u.cons = ((uint64_t)p.w[3] << 32) | p.w[2];
    u.ring = ((uint64_t)(p.w[5] & 0x00FFFFFFu) << 32) | p.w[4];
    u.size = 1u << ((p.w[5] >> 24) & 31u);
    return u;
}

}  // namespace xskgpu

#endif  // XSK_RING_PACK_H
