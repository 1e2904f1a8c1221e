// The host side of xsk_gpu_rx_queues_dev()'s argument block compiled for the host: the layout, the
// writer and the header check of xsknet_amd/csrc/xsk_rx_queues.h, with the packed ring form of xsk_ring_pack.h.  Blocks
// of 1, 2 and 1024 queues are written into heap arrays of exactly rq_block_size(n) bytes; the test builds this file with
// -fsanitize=address,undefined, so a byte written one past a block's end is a failure here, not a stray store into
// a caller's memory.  A record here is a stand-in of the library's size whose first bytes are the 132 packed rings, at
// the offsets the header states and xsk_rx_queues.hip asserts against the kernel's struct.
// Asserted: the block's size (0 outside [1, 1024]; 64 + n * stride, the stride a multiple of 64 and of 16 and at least
// a record); every ring of every record unpacks (pk_unpack) to what went in, absent rings included; the bytes between
// a record's end and the next record are zero; a second write gives the same bytes; a block written in the middle of a
// larger array leaves every byte outside [0, block_size) as it was; the header check accepts the matching call and
// refuses each of the four mismatches (magic, ABI version, queue count, options) and a foreign stride.
// Stand-alone: prints "rx queues ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/xsk_gpu.h"
#include "../../xsknet_amd/csrc/xsk_ring_pack.h"
#include "../../xsknet_amd/csrc/xsk_rx_queues.h"

#define CHECK(c, ...)                     \
    do {                                  \
        if (!(c)) {                       \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            exit(1);                      \
        }                                 \
    } while (0)

using namespace xskgpu;

static_assert(kRqStride % 64u == 0 && kRqStride % 16u == 0 && kRqStride >= kRqRecordBytes, "the stride");
static_assert(kRqRings == 132 && kRqRings * sizeof(PackedRing) <= kRqRecordBytes, "the rings of a record");
static_assert(kRqRecordBytes + 256u <= 4096u, "a record is an argument segment's worth");

// The stand-in for LoopFusedArgs: the packed rings, then the rest as words (with a hole the writer must leave zero).
struct Rec {
    PackedRing ring[kRqRings];
    uint32_t rest[(kRqRecordBytes - kRqRings * sizeof(PackedRing)) / 4u];
};
static_assert(sizeof(Rec) == kRqRecordBytes, "the stand-in's size");

// Ring k of queue q, absent for some (k, q): what the test packs and expects back.
static UnpackedRing ring_of(uint32_t q, uint32_t k) {
    UnpackedRing u;
    if ((q + k) % 7u == 3u) {  // the absent ring
        u.prod = u.cons = u.ring = 0;
        u.size = 1;
        return u;
    }
    const uint64_t base = ((uint64_t)1 << 47) | ((uint64_t)q << 28) | ((uint64_t)k << 16);
    u.prod = base + 4u;
    u.cons = base + 8u;
    u.ring = (base ^ ((uint64_t)(k & 1u) << 55)) + 0x1000u;
    u.size = 1u << ((q + k) % (kPkMaxLog2 + 1u));
    return u;
}

static void fill(uint32_t q, Rec& r) {
    for (uint32_t k = 0; k < kRqRings; ++k) {
        const UnpackedRing u = ring_of(q, k);
        CHECK(pk_packable(u.ring, u.size), "packable");
        r.ring[k] = pk_pack(u.prod, u.cons, u.ring, u.size);
    }
    const uint32_t n = (uint32_t)(sizeof r.rest / 4u);
    for (uint32_t i = 0; i + 1u < n; ++i) r.rest[i] = 0x9E3779B9u * (q + 1u) + i;  // (the last word: left as it came)
}

static void block_cases() {
    CHECK(rq_block_size(0) == 0 && rq_block_size(kRqMaxQueues + 1u) == 0 && rq_block_size(0xFFFFFFFFu) == 0, "size 0");
    CHECK(kRqMaxQueues == 1024u, "the bound");
    const uint32_t ns[] = {1, 2, 1024};
    for (uint32_t n : ns) {
        const size_t bytes = rq_block_size(n);
        CHECK(bytes == 64u + (size_t)n * kRqStride, "size of %u", n);
        uint8_t* a = (uint8_t*)malloc(bytes);  // exactly the block: ASan stops a store past its end
        uint8_t* b = (uint8_t*)malloc(bytes);
        memset(a, 0xEE, bytes);
        memset(b, 0x11, bytes);
        rq_write_block<Rec>(a, n, 0x17u, fill);
        rq_write_block<Rec>(b, n, 0x17u, fill);
        CHECK(memcmp(a, b, bytes) == 0, "two writes differ at %u queues", n);
        RqHeader h;
        memcpy(&h, a, sizeof h);
        CHECK(h.magic == kRqMagic && h.abi_version == XSK_GPU_ABI_VERSION && h.n_queues == n && h.opts == 0x17u &&
                  h.stride == kRqStride && h.record_bytes == kRqRecordBytes,
              "header");
        for (uint32_t z : h.zero) CHECK(z == 0, "header padding");
        for (uint32_t q = 0; q < n; ++q) {
            for (uint32_t k = 0; k < kRqRings; ++k) {
                const UnpackedRing got = pk_unpack(rq_ring_at(a, q, k)), want = ring_of(q, k);
                CHECK(got.prod == want.prod && got.cons == want.cons && got.ring == want.ring && got.size == want.size,
                      "queue %u ring %u", q, k);
            }
            const uint8_t* rec = a + rq_record_off(q);
            CHECK(rq_record_off(q) % 64u == 0, "record alignment");
            for (uint32_t i = kRqRecordBytes - 4u; i < kRqStride; ++i) CHECK(rec[i] == 0, "queue %u byte %u not zero", q, i);
        }
        free(a);
        free(b);
    }
    // the places of the rings, as the kernel's struct has them
    CHECK(kRqTxOff == 0 && kRqCompOff == 64u * 24u && kRqRxOff == 129u * 24u && kRqFillOff == 130u * 24u &&
              kRqStackOff == 131u * 24u,
          "ring offsets");
}

static void bounds_case() {
    const uint32_t n = 3, margin = 4096;
    const size_t bytes = rq_block_size(n);
    std::vector<uint8_t> big(bytes + 2u * margin, 0xC3);
    rq_write_block<Rec>(big.data() + margin, n, 0u, fill);
    for (uint32_t i = 0; i < margin; ++i)
        CHECK(big[i] == 0xC3 && big[margin + bytes + i] == 0xC3, "a byte outside the block was written (%u)", i);
    CHECK(big[margin] != 0xC3 || big[margin + 1] != 0xC3, "the block was written");
}

static void header_cases() {
    const RqHeader h = rq_header(5u, 0x17u);
    auto ok = [](const RqHeader& x, uint32_t n, uint32_t opts) {
        return rq_header_ok(x.magic, x.abi_version, x.n_queues, x.opts, x.stride, x.record_bytes, n, opts);
    };
    CHECK(ok(h, 5u, 0x17u), "the matching call");
    RqHeader m = h;
    m.magic ^= 1u;
    CHECK(!ok(m, 5u, 0x17u), "magic");
    m = h;
    m.abi_version += 1u;
    CHECK(!ok(m, 5u, 0x17u), "ABI version");
    CHECK(!ok(h, 4u, 0x17u) && !ok(h, 6u, 0x17u) && !ok(h, 1u, 0x17u), "queue count");
    CHECK(!ok(h, 5u, 0x7u) && !ok(h, 5u, 0u) && !ok(h, 5u, 0x10u), "options");
    m = h;
    m.stride += 64u;
    CHECK(!ok(m, 5u, 0x17u), "stride");
    m = h;
    m.record_bytes -= 8u;
    CHECK(!ok(m, 5u, 0x17u), "record size");
    RqHeader z;
    memset(&z, 0, sizeof z);
    CHECK(!ok(z, 0u, 0u), "a zeroed block");
}

int main() {
    block_cases();
    bounds_case();
    header_cases();
    printf("rx queues ok\n");
    return 0;
}
