// The scan stage of the compaction core (xsknet_amd/csrc/xsk_compact.h) replayed on the CPU, thread by thread as
// cp_scan_cells runs it: every thread's run from cp_scan_run, the run sums, the inclusive scan of the 1024 sums, the
// write-back.  The runs are checked to partition [0, nwg) in thread order.  With the CHECK of the stand-alone C tests
// that include it.
#ifndef COMPACT_REPLAY_H
#define COMPACT_REPLAY_H

#include <stdio.h>
#include <stdlib.h>

#include "../../xsknet_amd/csrc/xsk_compact.h"

#define CHECK(c, ...)                     \
    do {                                  \
        if (!(c)) {                       \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            exit(1);                      \
        }                                 \
    } while (0)

// cells[0, nwg) scanned in place: cell j receives put(j, before, total).  Returns the total.
template <class Put>
static uint32_t replay_scan_cells(uint32_t* cells, uint32_t nwg, Put put) {
    using namespace xskgpu;
    static uint32_t s[kCpScanThreads], sum[kCpScanThreads];
    uint32_t next = 0;
    for (uint32_t t = 0; t < kCpScanThreads; ++t) {
        uint32_t b, e;
        cp_scan_run(nwg, t, &b, &e);
        CHECK(b == next && b <= e && e <= nwg, "scan runs");
        next = e;
        sum[t] = 0;
        for (uint32_t j = b; j < e; ++j) sum[t] += cells[j];
    }
    CHECK(next == nwg, "scan runs do not cover the counts");
    uint32_t acc = 0;
    for (uint32_t t = 0; t < kCpScanThreads; ++t) s[t] = (acc += sum[t]);  // (what the Hillis-Steele rounds leave)
    const uint32_t total = s[kCpScanThreads - 1];
    for (uint32_t t = 0; t < kCpScanThreads; ++t) {
        uint32_t b, e, run = s[t] - sum[t];
        cp_scan_run(nwg, t, &b, &e);
        for (uint32_t j = b; j < e; ++j) {
            const uint32_t c = cells[j];
            cells[j] = put(j, run, total);
            run += c;
        }
    }
    return total;
}

static inline uint32_t replay_put_before(uint32_t, uint32_t before, uint32_t) { return before; }

#endif  // COMPACT_REPLAY_H
