// The read bound of classify_wire_one() (xsknet_amd/csrc/xsk_classify_wire.h), on the host: built with
// -fsanitize=address,undefined by tests/test_classify_wire_host.py, which also writes the input file from the Python
// spec.  The kernel may read no byte outside the UMEM and none at or past addr + len; a GPU run cannot show that
// (device allocations are padded), a heap allocation of exactly the UMEM's size under AddressSanitizer can.
//
// Input: records of five little-endian u32 -- opts, bound, len, expected action, nbytes -- followed by nbytes frame
// bytes (nbytes >= len, or the whole frame when it is shorter than len).  Every record runs
//   - as a UMEM of exactly min(len, nbytes) bytes, the frame flush with both ends (a len beyond it: DROP, nothing read);
//   - behind 1, 5 and 16 bytes of padding, flush with the end at an unaligned and an aligned start;
//   - in a UMEM one byte too short for len: DROP by the descriptor rule, nothing read past the end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../xsknet_amd/csrc/xsk_classify_wire.h"

static uint32_t run(const uint8_t* frame, uint32_t have, uint32_t pad, uint32_t len, uint32_t opts, int bound) {
    const uint64_t size = (uint64_t)pad + have;
    uint8_t* umem = (uint8_t*)malloc(size ? size : 1);  // exactly the UMEM: one byte further is a heap overflow
    if (!umem) abort();
    memset(umem, 0xA5, size ? size : 1);
    if (have) memcpy(umem + pad, frame, have);
    xsk_gpu_desc d;
    d.addr = pad;
    d.len = len;
    d.options = 0;
    const uint32_t act = xskgpu::classify_wire_one(umem, size, d, opts, bound);
    free(umem);
    return act;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned long records = 0, runs = 0, bad = 0;
    uint32_t h[5];
    std::vector<uint8_t> frame;
    while (fread(h, sizeof(uint32_t), 5, f) == 5) {
        const uint32_t opts = h[0], bound = h[1], len = h[2], want = h[3], nbytes = h[4];
        frame.resize(nbytes ? nbytes : 1);
        if (nbytes && fread(frame.data(), 1, nbytes, f) != nbytes) return 2;
        ++records;
        const uint32_t have = len < nbytes ? len : nbytes;
        // a frame cut below len lies outside its UMEM: DROP whatever its bytes say
        const uint32_t expect = have == len ? want : (uint32_t)XSK_GPU_XDP_DROP;
        const uint32_t pads[4] = {0, 1, 5, 16};
        for (uint32_t pad : pads) {
            const uint32_t got = run(frame.data(), have, pad, len, opts, (int)bound);
            ++runs;
            if (got != expect) {
                if (bad++ < 10) fprintf(stderr, "record %lu pad %u opts 0x%x len %u: got %u want %u\n", records, pad, opts, len, got, expect);
            }
        }
        if (have == len && len > 0) {  // the same frame in a UMEM one byte too short
            const uint32_t got = run(frame.data(), len - 1, 3, len, opts, (int)bound);
            ++runs;
            if (got != XSK_GPU_XDP_DROP && bad++ < 10) fprintf(stderr, "record %lu short UMEM: got %u\n", records, got);
        }
    }
    fclose(f);
    if (bad || !records) {
        fprintf(stderr, "%lu mismatches in %lu records\n", bad, records);
        return 1;
    }
    printf("classify wire ok: %lu records, %lu runs\n", records, runs);
    return 0;
}
