// The host side of xsk_gpu_responder_queues_dev()'s argument block compiled for the host: the layout, the
// writer and the header check of xsknet_amd/csrc/xsk_responder_block.h, with the packed ring form of xsk_ring_pack.h.
// Blocks of 1, 2 and 1024 records are written into heap arrays of exactly rs_block_size(n) bytes; the test builds this
// file with -fsanitize=address,undefined, so a byte written one past a block's end is a failure here, not a stray store
// into a caller's memory.  A record here is a stand-in of the library's size: the 132 packed rings of the loop body's
// record at its start, words up to that record's end, then the packed `up` ring and the serve stage's words.
// Asserted: the block's size (0 outside [1, 1024]; 64 + n * stride, the stride a multiple of 64 and of 16 and at least
// a record); every ring of every record, `up` included, unpacks (pk_unpack) to what went in, absent rings included; the
// bytes between a record's end and the next record are zero; a second write gives the same bytes; a block written in
// the middle of a larger array leaves every byte outside [0, block_size) as it was; the header check accepts the
// matching call and refuses each single mismatch (magic, ABI version, queue count, options, stride, record size), a
// zeroed block and the header of an rx-queues block -- and the rx-queues check refuses this block's header.
// Stand-alone: prints "responder ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/xsk_gpu.h"
#include "../../xsknet_amd/csrc/xsk_responder_block.h"
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

static_assert(kRsStride % 64u == 0 && kRsStride % 16u == 0 && kRsStride >= kRsRecordBytes, "the stride");
static_assert(kRsRings == 133 && kRsRecordBytes == 3504 && kRsStride == 3520, "the record");
static_assert(kRsRecordBytes + 256u <= 4096u, "a record is an argument segment's worth");
static_assert(kRsMagic != kRqMagic, "the two blocks are told apart");

// The stand-in for ResponderArgs.
struct Rec {
    PackedRing ring[kRqRings];
    uint32_t rest[(kRqRecordBytes - kRqRings * sizeof(PackedRing)) / 4u];
    PackedRing up;
    uint32_t tail[(kRsRecordBytes - kRsUpOff - sizeof(PackedRing)) / 4u];
};
static_assert(sizeof(Rec) == kRsRecordBytes && offsetof(Rec, up) == kRsUpOff, "the stand-in's layout");

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

static PackedRing packed(uint32_t q, uint32_t k) {
    const UnpackedRing u = ring_of(q, k);
    CHECK(pk_packable(u.ring, u.size), "packable");
    return pk_pack(u.prod, u.cons, u.ring, u.size);
}

static void fill(uint32_t q, Rec& r) {
    for (uint32_t k = 0; k < kRqRings; ++k) r.ring[k] = packed(q, k);
    r.up = packed(q, kRqRings);
    const uint32_t n = (uint32_t)(sizeof r.rest / 4u);
    for (uint32_t i = 0; i < n; ++i) r.rest[i] = 0x9E3779B9u * (q + 1u) + i;
    const uint32_t m = (uint32_t)(sizeof r.tail / 4u);
    for (uint32_t i = 0; i + 1u < m; ++i) r.tail[i] = 0x85EBCA6Bu * (q + 1u) + i;  // (the last word: left as it came)
}

static void block_cases() {
    CHECK(rs_block_size(0) == 0 && rs_block_size(kRsMaxQueues + 1u) == 0 && rs_block_size(0xFFFFFFFFu) == 0, "size 0");
    CHECK(kRsMaxQueues == 1024u, "the bound");
    const uint32_t ns[] = {1, 2, 1024};
    for (uint32_t n : ns) {
        const size_t bytes = rs_block_size(n);
        CHECK(bytes == 64u + (size_t)n * kRsStride, "size of %u", n);
        uint8_t* a = (uint8_t*)malloc(bytes);  // exactly the block: ASan stops a store past its end
        uint8_t* b = (uint8_t*)malloc(bytes);
        memset(a, 0xEE, bytes);
        memset(b, 0x11, bytes);
        rs_write_block<Rec>(a, n, 0x17u, fill);
        rs_write_block<Rec>(b, n, 0x17u, fill);
        CHECK(memcmp(a, b, bytes) == 0, "two writes differ at %u queues", n);
        RqHeader h;
        memcpy(&h, a, sizeof h);
        CHECK(h.magic == kRsMagic && h.abi_version == XSK_GPU_ABI_VERSION && h.n_queues == n && h.opts == 0x17u &&
                  h.stride == kRsStride && h.record_bytes == kRsRecordBytes,
              "header");
        for (uint32_t z : h.zero) CHECK(z == 0, "header padding");
        for (uint32_t q = 0; q < n; ++q) {
            for (uint32_t k = 0; k < kRsRings; ++k) {
                const UnpackedRing got = pk_unpack(rs_ring_at(a, q, k)), want = ring_of(q, k);
                CHECK(got.prod == want.prod && got.cons == want.cons && got.ring == want.ring && got.size == want.size,
                      "queue %u ring %u", q, k);
            }
            const uint8_t* rec = a + rs_record_off(q);
            CHECK(rs_record_off(q) % 64u == 0, "record alignment");
            for (uint32_t i = kRsRecordBytes - 4u; i < kRsStride; ++i) CHECK(rec[i] == 0, "queue %u byte %u not zero", q, i);
        }
        free(a);
        free(b);
    }
    CHECK(kRsUpOff == 3448u && kRsUpOff == kRqRecordBytes, "up lies behind the loop body's record");
}

static void bounds_case() {
    const uint32_t n = 3, margin = 4096;
    const size_t bytes = rs_block_size(n);
    std::vector<uint8_t> big(bytes + 2u * margin, 0xC3);
    rs_write_block<Rec>(big.data() + margin, n, 0u, fill);
    for (uint32_t i = 0; i < margin; ++i)
        CHECK(big[i] == 0xC3 && big[margin + bytes + i] == 0xC3, "a byte outside the block was written (%u)", i);
    CHECK(big[margin] != 0xC3 || big[margin + 1] != 0xC3, "the block was written");
}

static void header_cases() {
    const RqHeader h = rs_header(5u, 0x17u);
    auto ok = [](const RqHeader& x, uint32_t n, uint32_t opts) {
        return rs_header_ok(x.magic, x.abi_version, x.n_queues, x.opts, x.stride, x.record_bytes, n, opts);
    };
    auto rq_ok = [](const RqHeader& x, uint32_t n, uint32_t opts) {
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
    // the other call's block, for the same count and options: foreign both ways, by each of magic, stride and record size
    const RqHeader r = rq_header(5u, 0x17u);
    CHECK(rq_ok(r, 5u, 0x17u) && !ok(r, 5u, 0x17u) && !rq_ok(h, 5u, 0x17u), "an rx-queues header");
    m = r;
    m.magic = kRsMagic;
    CHECK(!ok(m, 5u, 0x17u), "an rx-queues header under this magic: its stride and record size");
}

int main() {
    block_cases();
    bounds_case();
    header_cases();
    printf("responder ok\n");
    return 0;
}
