// xsk_steer.h — the per-frame decision and the index arithmetic of xsk_gpu_steer_dev() (include/xsk_gpu.h; DESIGN.md
// §9.4): the ingress filter whose REDIRECT carries a port, looked up by the frame's destination address in a sorted
// table of at most 1024 entries, and the stable partition of the REDIRECT descriptors by port.  Host and device:
// xsk_steer.hip's kernels and its host code call these functions, and tests/c/test_steer.cpp runs them on the CPU under
// AddressSanitizer -- the decision on frames that end flush with their allocation, the search on tables of exactly
// n_entries entries, the partition replayed lane by lane into a list of exactly the REDIRECT count.
//
// The decision is xsk_classify.hip's classify_one() for opts == 0 and xsk_classify_wire.h's classify_wire_one() for
// nonzero opts, rule for rule, with the point where those say REDIRECT replaced by the lookup.  The reads keep their
// shape: only bytes of [addr, addr + len) (opts == 0: of the first 34, as classify_one()), two dependent round trips
// at most behind the descriptor, and the destination address rides in the round trip that reads its IP header --
//   1. bytes 12-23, and with them bytes 30-33: the destination of an untagged IPv4 frame, which decides here;
//   2. byte l3 + 9 / l3 + 6, the ICMPv6 type, and the 16 bytes that hold the destination: [l3 + 8, l3 + 20) and
//      [l3 + 16, l3 + 20) of an IPv4 header, [l3 + 24, l3 + 40) of an IPv6 header.  Both ranges lie below the header's
//      end, which rules 4 and 5 have put at or below len by then.
#ifndef XSK_STEER_H
#define XSK_STEER_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/xsk_gpu.h"
#include "xsk_classify_wire.h"
#include "xsk_compact.h"

#define XSK_ST_FN XSK_CW_FN

namespace xskgpu {

constexpr uint32_t kStWave = kCpWave;
constexpr uint32_t kStFrames = kCpFrames;  // frames (and threads) per workgroup of the classify and scatter stages
constexpr uint32_t kStWaves = kCpWaves;
constexpr uint32_t kStScanThreads = kCpScanThreads;  // a scan workgroup: one per port, over that port's row
constexpr uint32_t kStMaxPorts = XSK_GPU_STEER_MAX_PORTS;
constexpr uint32_t kStMaxEntries = XSK_GPU_STEER_MAX_ENTRIES;
constexpr uint32_t kStPass = XSK_GPU_STEER_PASS;
constexpr uint32_t kStKeyWords = 5;    // family, then the address as four big-endian dwords: integer order == memcmp order
constexpr uint32_t kStEntryWords = 6;  // a staged entry: the key, then the port

// ---- the table ----
XSK_ST_FN uint32_t st_bswap(uint32_t w) { return __builtin_bswap32(w); }

// One entry of the caller's table (24 bytes, 8-B aligned) as six dwords: what the kernel keeps in LDS.
XSK_ST_FN void st_stage_entry(const xsk_gpu_steer_entry* e, uint32_t* out) {
    uint32_t w[6];
    __builtin_memcpy(w, e, 24);
    out[0] = w[4] & 0xFFu;  // family
    out[1] = st_bswap(w[0]);
    out[2] = st_bswap(w[1]);
    out[3] = st_bswap(w[2]);
    out[4] = st_bswap(w[3]);
    out[5] = (w[4] >> 8) & 0xFFu;  // port
}

// The port of the staged entry whose key is `key`, or `miss`.  Binary search with a three-way compare: every probe is
// of an index in [0, n), whatever the table holds, so a table that was not prepared can only miss.  At most
// floor(log2(n)) + 1 probes: 10 up to 1023 entries, 11 at 1024.
XSK_ST_FN uint32_t st_lookup(const uint32_t* tab, uint32_t n, const uint32_t* key, uint32_t miss) {
    uint32_t lo = 0, hi = n, port = miss;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t* e = tab + (size_t)mid * kStEntryWords;
        int c = 0;  // sign of entry - key
        for (uint32_t k = kStKeyWords; k-- > 0;) c = e[k] != key[k] ? (e[k] < key[k] ? -1 : 1) : c;
        if (c == 0) {
            port = e[kStKeyWords];
            break;
        }
        if (c < 0)
            lo = mid + 1;
        else
            hi = mid;
    }
    return port;
}

// ---- the decision ----
struct StParsed {
    uint32_t act;     // the action of the filter's rules with a bound target: REDIRECT means "look the port up"
    uint32_t key[5];  // valid with REDIRECT: family (4 or 6), the destination as big-endian dwords (IPv4: three zeros)
};

XSK_ST_FN void st_key4(StParsed* r, uint32_t dst_le) {
    r->key[0] = 4u;
    r->key[1] = st_bswap(dst_le);
    r->key[2] = r->key[3] = r->key[4] = 0u;
}

// opts == 0: classify_one() of xsk_classify.hip (the reference's xdp_sock_prog, src/kern/inner_xdp.c:26-61).  One round
// trip: bytes 12, 13, 23 and the destination, bytes 30-33, all only when the IPv4 header is inside the frame.
XSK_ST_FN StParsed st_parse_ref(const uint8_t* umem, uint64_t umem_size, const xsk_gpu_desc& d) {
    StParsed r = {XSK_GPU_XDP_DROP, {0u, 0u, 0u, 0u, 0u}};
    const uint64_t a = d.addr;
    const uint32_t len = d.len;
    const uint32_t need = len < 34 ? (len < 14 ? 0u : 14u) : 34u;
    if (len > XSK_GPU_MAX_LEN || a > umem_size || need > umem_size - a) return r;  // build-added
    if (len < 14) return r;                                                        // :35-36
    const uint8_t* p = umem + a;
    const uint32_t e0 = p[12], e1 = p[13];
    uint32_t pr = 0u, dst = 0u;
    if (len >= 34) {
        pr = p[23];
        __builtin_memcpy(&dst, p + 30, 4);
    }
    r.act = XSK_GPU_XDP_PASS;
    if (e0 != 0x08 || e1 != 0x00) return r;  // :38-39
    r.act = XSK_GPU_XDP_DROP;
    if (len < 34) return r;                  // :41-42
    r.act = XSK_GPU_XDP_PASS;
    if (pr != 1) return r;                   // :44-45
    r.act = XSK_GPU_XDP_REDIRECT;            // :57-60, the map lookup
    st_key4(&r, dst);
    return r;
}

// Nonzero opts: classify_wire_one() of xsk_classify_wire.h, rules 1-6 of include/xsk_gpu.h.
XSK_ST_FN StParsed st_parse_wire(const uint8_t* umem, uint64_t umem_size, const xsk_gpu_desc& d, uint32_t opts) {
    StParsed r = {XSK_GPU_XDP_DROP, {0u, 0u, 0u, 0u, 0u}};
    const uint64_t a = d.addr;
    const uint32_t len = d.len;
    if (len > XSK_GPU_MAX_LEN || a > umem_size || len > umem_size - a) return r;  // rule 1
    if (len < 14) return r;                                                       // rule 2
    const uint8_t* p = umem + a;
    const uint32_t last = len - 1;
    uint32_t w[3] = {0u, 0u, 0u};  // bytes 12-23 as little-endian dwords; a byte at or past len is never used
    uint32_t dst14 = 0u;           // bytes 30-33: the destination behind an untagged IPv4 header, used only when len >= 34
    if (len >= 24) {
        __builtin_memcpy(w, p + 12, 12);
        __builtin_memcpy(&dst14, p + (len >= 34 ? 30u : 12u), 4);  // the same round trip; a frame below 34 re-reads 12-15
    } else {
        for (uint32_t k = 12; k < 24; ++k) w[(k - 12) >> 2] |= (uint32_t)p[cw_min(k, last)] << (8u * ((k - 12) & 3u));
    }
    uint32_t l3 = 14, et = cw_be16lo(w[0]);  // rule 3
    if ((opts & XSK_GPU_OPT_VLAN) && cw_is_tpid(et)) {
        if (len < 18) return r;
        et = cw_be16lo(w[1]);
        l3 = 18;
        if (cw_is_tpid(et)) {
            if (len < 22) return r;
            et = cw_be16lo(w[2]);
            l3 = 22;
        }
    }
    const bool v4 = et == 0x0800u;
    const bool v6 = et == 0x86DDu && (opts & XSK_GPU_OPT_IPV6);
    r.act = XSK_GPU_XDP_PASS;
    if (!v4 && !v6) return r;  // rule 6
    r.act = XSK_GPU_XDP_DROP;
    if (len < l3 + (v4 ? 20u : 40u)) return r;  // rules 4, 5: header cut
    if (v4 && l3 == 14) {                       // rule 4, one round trip
        r.act = (w[2] >> 24) != 1u ? XSK_GPU_XDP_PASS : XSK_GPU_XDP_REDIRECT;
        st_key4(&r, dst14);
        return r;
    }
    const uint32_t pr = p[v4 ? l3 + 9 : l3 + 6];     // below l3 + 20 <= len
    const uint32_t type = p[cw_min(l3 + 40, last)];  // the ICMPv6 type when len >= l3 + 48, else unused
    // the destination with them, two loads at addresses that depend on l3 and the family alone: its first four bytes,
    // and twelve more that are the rest of an IPv6 address -- for IPv4 twelve bytes of the header that go unused, so
    // that neither load stands under a condition.  IPv4: [l3 + 16, l3 + 20), [l3 + 8, l3 + 20).  IPv6: [l3 + 24,
    // l3 + 28), [l3 + 28, l3 + 40).  All below the header's end <= len.
    uint32_t d0 = 0u, d1[3] = {0u, 0u, 0u};
    __builtin_memcpy(&d0, p + (v4 ? l3 + 16 : l3 + 24), 4);
    __builtin_memcpy(d1, p + (v4 ? l3 + 8 : l3 + 28), 12);
    const uint32_t pr_ok = pr == (v4 ? 1u : 58u), cut = len < l3 + 48, echo = type == 128u;
    const uint32_t hit = pr_ok & ((uint32_t)v4 | (~cut & echo & 1u));  // rules 4, 5: REDIRECT
    const uint32_t drop = pr_ok & ~(uint32_t)v4 & cut & 1u;           // rule 5: ICMPv6 header cut
    r.act = hit ? XSK_GPU_XDP_REDIRECT : drop ? XSK_GPU_XDP_DROP : XSK_GPU_XDP_PASS;
    r.key[0] = v4 ? 4u : 6u;
    r.key[1] = st_bswap(d0);
    r.key[2] = v4 ? 0u : st_bswap(d1[0]);
    r.key[3] = v4 ? 0u : st_bswap(d1[1]);
    r.key[4] = v4 ? 0u : st_bswap(d1[2]);
    return r;
}

struct StVerdict {
    uint32_t act;   // XSK_GPU_XDP_*
    uint32_t port;  // the port of a REDIRECT frame, XSK_GPU_STEER_PASS for every other
};

// Rules 2-5 of the steering spec, from the port the table (or the default) gave a frame the filter's rules redirect.
XSK_ST_FN StVerdict st_port_rule(uint32_t port, uint32_t n_ports, uint64_t bound) {
    StVerdict v = {XSK_GPU_XDP_PASS, kStPass};
    if (port == kStPass) return v;                                   // not ours: the kernel stack
    v.act = XSK_GPU_XDP_DROP;
    if (port >= n_ports || !((bound >> (port & 63u)) & 1ull)) return v;  // no entry in the map
    v.act = XSK_GPU_XDP_REDIRECT;
    v.port = port;
    return v;
}

// One frame.  `tab` is the staged table (st_stage_entry), n_entries of it; `bound` the word of *d_bound (all ones for
// NULL).
XSK_ST_FN StVerdict st_steer_one(const uint8_t* umem, uint64_t umem_size, const xsk_gpu_desc& d, uint32_t opts,
                                 const uint32_t* tab, uint32_t n_entries, uint32_t default_port, uint32_t n_ports,
                                 uint64_t bound) {
    const StParsed r = opts ? st_parse_wire(umem, umem_size, d, opts) : st_parse_ref(umem, umem_size, d);
    if (r.act != XSK_GPU_XDP_REDIRECT) {
        StVerdict v = {r.act, kStPass};
        return v;
    }
    const uint32_t port = n_entries ? st_lookup(tab, n_entries, r.key, default_port) : default_port;
    return st_port_rule(port, n_ports, bound);
}

// ---- the partition ----
// Stage 1 counts REDIRECT frames per workgroup and port into a matrix stored port-major, count[port][workgroup].  The
// exclusive scan of the n_ports x nwg words in that order is what a frame's slot needs; stage 2 computes it as one
// scan per row, a workgroup each (one workgroup over the whole matrix was 386 us at 64 ports and 2^20 frames, DESIGN.md
// §9.4), which leaves every cell relative to its row's start.  The cell [p][0] would always hold 0, so it carries the
// row's total instead, and stage 3 turns the n_ports totals into the rows' starts: d_off.  A frame's slot is then
// d_off[port], its workgroup's cell, the counts of the lower waves of the workgroup and the rank among the lower lanes
// of the wave.
XSK_ST_FN size_t st_cell(uint32_t port, uint32_t wg, uint32_t nwg) { return (size_t)port * nwg + wg; }
XSK_ST_FN size_t st_cells(uint32_t n_ports, uint32_t nwg) { return (size_t)n_ports * nwg; }

// What stage 2 (cp_scan_cells over a row of cp_nwg(n) cells) leaves in cell j (exclusive prefix `before`, row total
// `total`), and what stage 3 reads back
// as workgroup wg's offset inside the row.
XSK_ST_FN uint32_t st_scanned_cell(uint32_t j, uint32_t before, uint32_t total) { return j == 0u ? total : before; }
XSK_ST_FN uint32_t st_cell_offset(uint32_t wg, uint32_t cell) { return wg == 0u ? 0u : cell; }

// The slot of a REDIRECT frame.
XSK_ST_FN uint32_t st_slot(uint32_t port_start, uint32_t in_row, uint32_t lower_waves, uint32_t lower_lanes) {
    return port_start + in_row + lower_waves + lower_lanes;
}

XSK_ST_FN size_t st_workspace_bytes(uint32_t n, uint32_t n_ports) {
    return st_cells(n_ports, cp_nwg(n)) * sizeof(uint32_t);
}

// ---- the partition in one workgroup (xsk_gpu_rx_fused_loop_dev(), xsk_loop_fused_body.h) ----
// Up to kSt1Frames frames, a lane per frame, kSt1Waves waves: wave_ranks() fills a kSt1Waves x kStMaxPorts count matrix
// in LDS, cnt[wave][port].  Port p's total is its column's sum, its first slot the sum of the totals of the ports below
// it (d_off[p]; d_off[n_ports] is the REDIRECT count), and a frame's slot is its port's first slot, the column's counts
// of the lower waves and the frame's rank among the lower lanes of its wave.  Batch order holds within a port; no atomic
// hands out a slot.  Host and device: tests/c/test_loop_fused.cpp replays it lane by lane.
constexpr uint32_t kSt1Frames = XSK_GPU_LOWLAT_MAX;
constexpr uint32_t kSt1Waves = kSt1Frames / kStWave;

XSK_ST_FN uint32_t st1_port_total(const uint32_t (*cnt)[kStMaxPorts], uint32_t port) {
    uint32_t sum = 0;
    for (uint32_t w = 0; w < kSt1Waves; ++w) sum += cnt[w][port];
    return sum;
}
XSK_ST_FN uint32_t st1_lower_waves(const uint32_t (*cnt)[kStMaxPorts], uint32_t wave, uint32_t port) {
    uint32_t sum = 0;
    for (uint32_t w = 0; w < kSt1Waves; ++w) sum += w < wave ? cnt[w][port] : 0u;
    return sum;
}
XSK_ST_FN uint32_t st1_slot(uint32_t port_start, uint32_t lower_waves, uint32_t lower_lanes) {
    return st_slot(port_start, 0u, lower_waves, lower_lanes);
}

#ifdef __HIPCC__
// The wave's frames by port: one ballot per distinct port present (the port of the lowest lane not yet served, read
// into a scalar with readlane, which is readfirstlane over the lanes still to do).
// s_cnt[wave][port] gets the wave's count of every port present -- the rest of the row was zeroed by the caller -- and
// the lane learns how many lower lanes of its wave carry its port.
__device__ __forceinline__ uint32_t wave_ranks(bool redirect, uint32_t port, uint32_t (*s_cnt)[kStMaxPorts]) {
    const uint32_t lane = cp_lane(), w = cp_wave();
    uint32_t rank = 0;
    unsigned long long todo = __ballot(redirect);
    while (todo) {  // wave-uniform
        const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)port, (int)__builtin_ctzll(todo));
        const unsigned long long m = __ballot(redirect && port == p);
        if (redirect && port == p) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_cnt[w][p] = (uint32_t)__popcll(m);
        todo &= ~m;
    }
    return rank;
}
#endif  // __HIPCC__


}  // namespace xskgpu

#endif  // XSK_STEER_H
