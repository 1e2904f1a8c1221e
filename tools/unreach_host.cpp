// unreach_host.cpp — xsk_unreach.h's rule compiled for the host, as one call over host copies of the consumed ring, the
// frames and the destination rings: the CPU stage of the host round trip that xsk_gpu_unreach_serve_dev() replaces.
// tools/unreach_bench.py builds it with g++ into a temporary directory and times it between a D2H and an H2D copy
// (DESIGN.md §9.16); nothing of the product links it.
#include <stdint.h>

#include <vector>

#include "../include/xsk_gpu.h"
#include "../xsknet_amd/csrc/xsk_ring_dev.h"
#include "../xsknet_amd/csrc/xsk_unreach.h"

using namespace xskgpu;

// The sequential rule of xsk_gpu_unreach_serve_dev().  words: { producer, consumer } per ring; tx_ent and tx_words hold
// the n_ports TX rings back to back, tx_size entries each; budget NULL: unlimited.  Returns c and advances the words.
extern "C" uint32_t unreach_host_serve(uint8_t* umem, uint64_t umem_size, const xsk_gpu_desc* up_ent, uint32_t up_size,
                                       uint32_t* up_words, xsk_gpu_desc* tx_ent, uint32_t tx_size, uint32_t* tx_words,
                                       uint32_t n_ports, xsk_gpu_desc* rest_ent, uint32_t rest_size, uint32_t* rest_words,
                                       uint32_t max, uint32_t opts, const xsk_gpu_neigh_entry* table, uint32_t n_entries,
                                       uint64_t bound, const uint8_t* open, uint32_t chunk_size, uint32_t* budget) {
    std::vector<uint32_t> tab((size_t)n_entries * kNgEntryWords);
    for (uint32_t k = 0; k < n_entries; ++k) ng_stage_entry(table + k, tab.data() + (size_t)k * kNgEntryWords);
    uint32_t room[kNgDests], given[kNgDests] = {0};
    for (uint32_t p = 0; p < n_ports; ++p) room[p] = rd_free(tx_words[2 * p], tx_words[2 * p + 1], tx_size);
    room[kNgUp] = rd_free(rest_words[0], rest_words[1], rest_size);
    const uint32_t m = ng_serve_m(rd_used(up_words[0], up_words[1], up_size), max);
    uint32_t c = 0, eligible = 0, left = budget ? *budget : 0xFFFFFFFFu;
    for (; c < m; ++c) {
        const xsk_gpu_desc e = up_ent[rd_slot(up_words[1] + c, up_size)];
        UrVerdict v = ur_decide(umem, umem_size, e, opts, tab.data(), n_entries, n_ports, bound, open, chunk_size);
        const bool due = ur_is_reply(v.verdict);
        v.verdict = ur_limit(v.verdict, eligible, left);  // (the rank among the eligible against the budget at entry)
        eligible += due;
        const uint32_t dest = ur_dest(v.verdict, v.port);
        if (given[dest] >= room[dest]) break;
        if (ur_is_reply(v.verdict)) ur_rewrite(umem + e.addr, v);
        if (dest == kNgUp)
            rest_ent[rd_slot(rest_words[0] + given[dest], rest_size)] = ur_out_entry(e, v);
        else
            tx_ent[(size_t)dest * tx_size + rd_slot(tx_words[2 * dest] + given[dest], tx_size)] = ur_out_entry(e, v);
        ++given[dest];
    }
    uint32_t sent = 0;
    for (uint32_t p = 0; p < n_ports; ++p) {
        tx_words[2 * p] += given[p];
        sent += given[p];
    }
    rest_words[0] += given[kNgUp];
    up_words[1] += c;
    if (budget && sent) *budget = left - sent;
    return c;
}
