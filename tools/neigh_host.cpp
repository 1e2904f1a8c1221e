// neigh_host.cpp — xsk_neigh.h's rule compiled for the host, as one call over host copies of the stack ring, the
// frames and the destination rings: the CPU stage of the host round trip that xsk_gpu_neigh_serve_dev() replaces.
// tools/neigh_bench.py builds it with g++ into a temporary directory and times it between a D2H and an H2D copy
// (DESIGN.md §9.13); nothing of the product links it.
#include <stdint.h>

#include <vector>

#include "../include/xsk_gpu.h"
#include "../xsknet_amd/csrc/xsk_neigh.h"
#include "../xsknet_amd/csrc/xsk_ring_dev.h"

using namespace xskgpu;

// The sequential rule of xsk_gpu_neigh_serve_dev().  words: { producer, consumer } per ring; tx_ent and tx_words hold
// the n_ports TX rings back to back, tx_size entries each.  Returns c and advances the words.
extern "C" uint32_t neigh_host_serve(uint8_t* umem, uint64_t umem_size, const xsk_gpu_desc* stack_ent, uint32_t stack_size,
                                     uint32_t* stack_words, xsk_gpu_desc* tx_ent, uint32_t tx_size, uint32_t* tx_words,
                                     uint32_t n_ports, xsk_gpu_desc* up_ent, uint32_t up_size, uint32_t* up_words,
                                     uint32_t max, uint32_t opts, const xsk_gpu_neigh_entry* table, uint32_t n_entries,
                                     uint64_t bound) {
    std::vector<uint32_t> tab((size_t)n_entries * kNgEntryWords);
    for (uint32_t k = 0; k < n_entries; ++k) ng_stage_entry(table + k, tab.data() + (size_t)k * kNgEntryWords);
    uint32_t room[kNgDests], given[kNgDests] = {0};
    for (uint32_t p = 0; p < n_ports; ++p) room[p] = rd_free(tx_words[2 * p], tx_words[2 * p + 1], tx_size);
    room[kNgUp] = rd_free(up_words[0], up_words[1], up_size);
    const uint32_t m = ng_serve_m(rd_used(stack_words[0], stack_words[1], stack_size), max);
    uint32_t c = 0;
    for (; c < m; ++c) {
        const xsk_gpu_desc e = stack_ent[rd_slot(stack_words[1] + c, stack_size)];
        const NgVerdict v = ng_decide(umem, umem_size, e, opts, tab.data(), n_entries, n_ports, bound);
        const uint32_t dest = ng_dest(v.verdict, v.port);
        if (given[dest] >= room[dest]) break;
        if (ng_is_reply(v.verdict)) ng_rewrite(umem + e.addr, v);
        if (dest == kNgUp)
            up_ent[rd_slot(up_words[0] + given[dest], up_size)] = ng_out_entry(e, v);
        else
            tx_ent[(size_t)dest * tx_size + rd_slot(tx_words[2 * dest] + given[dest], tx_size)] = ng_out_entry(e, v);
        ++given[dest];
    }
    for (uint32_t p = 0; p < n_ports; ++p) tx_words[2 * p] += given[p];
    up_words[0] += given[kNgUp];
    stack_words[1] += c;
    return c;
}
