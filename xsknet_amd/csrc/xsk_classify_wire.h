// xsk_classify_wire.h — the per-frame decision of xsk_gpu_classify_dev_opts() for nonzero options (include/xsk_gpu.h,
// "Ingress filter with wire-format options").  A header of its own so that the same function also
// compiles for the host: tests/c/test_classify_wire.cpp runs it under AddressSanitizer on frames that end flush with
// their allocation, which no run on the device can check.
//
// Every read is of a byte index below len -- an index that could reach len is clamped to len - 1 and its value never
// used -- and rule 1 has put [addr, addr + len) inside the UMEM by then, so a frame that ends flush with the UMEM is
// read up to its last byte and no further.  Clamping instead of branching also keeps the loads of one round trip in one
// basic block, so none waits for another.  Two dependent round trips at most behind the descriptor:
//   1. bytes 12-23 in one 12-byte load (twelve byte loads below 24 B): the ethertype chain of up to two tags and, for
//      an untagged frame, the IPv4 protocol (23) -- an untagged IPv4 frame decides here;
//   2. byte l3 + 9 (IPv4) or l3 + 6 (IPv6) and the ICMPv6 type l3 + 40, issued together.
#ifndef XSK_CLASSIFY_WIRE_H
#define XSK_CLASSIFY_WIRE_H

#include <stdint.h>

#include "../../include/xsk_gpu.h"

#ifdef __HIPCC__
#define XSK_CW_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define XSK_CW_FN static inline
#endif

namespace xskgpu {

XSK_CW_FN uint32_t cw_be16lo(uint32_t w) { return ((w & 0xFFu) << 8) | ((w >> 8) & 0xFFu); }
XSK_CW_FN bool cw_is_tpid(uint32_t et) { return et == 0x8100u || et == 0x88A8u; }
XSK_CW_FN uint32_t cw_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

XSK_CW_FN uint32_t classify_wire_one(const uint8_t* umem, uint64_t umem_size, const xsk_gpu_desc& d, uint32_t opts,
                                     int bound) {
    const uint64_t a = d.addr;
    const uint32_t len = d.len;
    if (len > XSK_GPU_MAX_LEN || a > umem_size || len > umem_size - a) return XSK_GPU_XDP_DROP;  // rule 1
    if (len < 14) return XSK_GPU_XDP_DROP;                                                       // rule 2
    const uint8_t* p = umem + a;
    const uint32_t last = len - 1;
    uint32_t w[3] = {0u, 0u, 0u};  // bytes 12-23 as little-endian dwords; a byte at or past len is never used
    if (len >= 24) {
        __builtin_memcpy(w, p + 12, 12);
    } else {
        for (uint32_t k = 12; k < 24; ++k) w[(k - 12) >> 2] |= (uint32_t)p[cw_min(k, last)] << (8u * ((k - 12) & 3u));
    }
    uint32_t l3 = 14, et = cw_be16lo(w[0]);                                              // rule 3
    if ((opts & XSK_GPU_OPT_VLAN) && cw_is_tpid(et)) {
        if (len < 18) return XSK_GPU_XDP_DROP;
        et = cw_be16lo(w[1]);
        l3 = 18;
        if (cw_is_tpid(et)) {
            if (len < 22) return XSK_GPU_XDP_DROP;
            et = cw_be16lo(w[2]);
            l3 = 22;
        }
    }
    const bool v4 = et == 0x0800u;
    const bool v6 = et == 0x86DDu && (opts & XSK_GPU_OPT_IPV6);
    if (!v4 && !v6) return XSK_GPU_XDP_PASS;                                             // rule 6
    if (len < l3 + (v4 ? 20u : 40u)) return XSK_GPU_XDP_DROP;                            // rules 4, 5: header cut
    const uint32_t redirect = bound ? XSK_GPU_XDP_REDIRECT : XSK_GPU_XDP_DROP;
    if (v4 && l3 == 14) return (w[2] >> 24) != 1u ? XSK_GPU_XDP_PASS : redirect;         // rule 4, one round trip
    const uint32_t pr = p[v4 ? l3 + 9 : l3 + 6];     // below l3 + 20 <= len
    const uint32_t type = p[cw_min(l3 + 40, last)];  // the ICMPv6 type when len >= l3 + 48, else unused
    // both bytes meet in bitwise arithmetic, not in nested conditionals: a load the compiler could move under a branch
    // on the other byte would become a third round trip
    const uint32_t pr_ok = pr == (v4 ? 1u : 58u), cut = len < l3 + 48, echo = type == 128u;
    const uint32_t hit = pr_ok & ((uint32_t)v4 | (~cut & echo & 1u));                     // rules 4, 5: REDIRECT
    const uint32_t drop = pr_ok & ~(uint32_t)v4 & cut & 1u;                               // rule 5: ICMPv6 header cut
    return hit ? redirect : drop ? XSK_GPU_XDP_DROP : XSK_GPU_XDP_PASS;
}

}  // namespace xskgpu

#endif  // XSK_CLASSIFY_WIRE_H
