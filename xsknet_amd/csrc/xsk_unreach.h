// xsk_unreach.h — the per-frame decision, the rewrites and the serve plan of xsk_gpu_unreach_dev() and
// xsk_gpu_unreach_serve_dev() (include/xsk_gpu.h, "Port-unreachable responder"): the responder that
// answers a UDP datagram for one of the neighbour table's addresses on a port nobody listens on with ICMP destination
// unreachable / port unreachable (RFC 792, RFC 1122 §3.2.2.1) or ICMPv6 type 1 code 4 (RFC 4443 §3.1), in place.  Host
// and device: xsk_unreach.hip's kernels call these functions, and tests/c/test_unreach.cpp runs them on the CPU under
// AddressSanitizer.  The table, its staging and its search are xsk_neigh.h's (ng_stage_entry, ng_lookup), shared, not
// restated.
//
// The decision (ur_decide) only reads, and only bytes of [addr, addr + len).  The reply quotes the request behind a
// fresh header, so it is LONGER than what it quotes and the quoted bytes move forward inside the chunk: source and
// destination overlap.  Two rewrites that leave the same bytes:
//   ur_rewrite():  one thread, no buffer -- sums the quote, then moves it from its last byte down (memmove's order for a
//                  destination above its source), then writes the headers.  The host's, and the spec the other is held to.
//   the lane pieces (ur_lane_load / ur_lane_part / ur_lane_store_quote / ur_lane_header): a wave's rewrite, lane k
//                  owning quote bytes k, k + 64, ...: every lane loads, the 64 parts are summed, and only then does any
//                  lane store.  xsk_unreach_device.h runs them with a wave reduction in between; the host test replays
//                  them over 64 lanes, all loads in front of all stores.
// Frames may lie at odd addresses: every access is a byte access.
#ifndef XSK_UNREACH_H
#define XSK_UNREACH_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/xsk_gpu.h"
#include "xsk_neigh.h"

#define XSK_UR_FN XSK_NG_FN

namespace xskgpu {

constexpr uint32_t kUrMaxQuote6 = 1232;  // rule 4e: 1280 (the minimum MTU) - 40 - 8
constexpr uint32_t kUrWave = 64;
constexpr uint32_t kUrLaneBytes = (kUrMaxQuote6 + kUrWave - 1u) / kUrWave;  // 20: the quote bytes a lane holds
constexpr uint32_t kUrOpenBytes = 8192;                                     // a bit per UDP port
constexpr uint32_t kUrMinChunk = 2048, kUrMaxChunk = 1u << 20;
constexpr uint32_t kUrStatsWords = 5;  // seen, unreach4, unreach6, reply_bytes, limited

XSK_UR_FN bool ur_chunk_ok(uint32_t chunk_size) {
    return chunk_size >= kUrMinChunk && chunk_size <= kUrMaxChunk && !(chunk_size & (chunk_size - 1u));
}
XSK_UR_FN bool ur_is_reply(uint32_t verdict) {
    return verdict == XSK_GPU_UNREACH_UNREACH4 || verdict == XSK_GPU_UNREACH_UNREACH6;
}
// "somebody listens on UDP port p": bit p & 7 of byte p >> 3; NULL: nobody.
XSK_UR_FN bool ur_open(const uint8_t* d_open, uint32_t port) {
    return d_open && ((d_open[(port & 0xFFFFu) >> 3] >> (port & 7u)) & 1u);
}

// ---- the decision ----
struct UrVerdict {
    uint32_t verdict;    // XSK_GPU_UNREACH_*
    uint32_t port;       // the entry's port with UNREACH4 / UNREACH6, 0xFF otherwise
    uint32_t reply_len;  // R, with UNREACH4 / UNREACH6
    uint32_t l3;         // where the IP header begins
    uint32_t q;          // the bytes quoted: old [l3, l3 + q)
    uint32_t mac_lo, mac_hi;  // the entry's mac: bytes 0-3 and 4-5, little-endian
};
XSK_UR_FN UrVerdict ur_none() { return UrVerdict{XSK_GPU_UNREACH_NONE, 0xFFu, 0u, 14u, 0u, 0u, 0u}; }

// Rules 3d-3g and 4d-4f behind the key: the table, the port rule, the open port, the room.
XSK_UR_FN UrVerdict ur_resolve(UrVerdict r, const uint32_t* key, const uint32_t* tab, uint32_t n_entries, uint32_t n_ports,
                               uint64_t bound, const uint8_t* d_open, uint32_t udp_port, uint64_t addr, uint64_t umem_size,
                               uint32_t chunk_size, uint32_t reply, uint32_t q, uint32_t reply_len) {
    const uint32_t at = n_entries ? ng_lookup(tab, n_entries, key) : kNgMiss;
    r.verdict = XSK_GPU_UNREACH_UNKNOWN;
    if (at == kNgMiss) return r;
    const uint32_t* e = tab + (size_t)at * kNgEntryWords;
    const uint32_t port = e[5];
    r.verdict = XSK_GPU_UNREACH_UNBOUND;
    if (port >= n_ports || !((bound >> (port & 63u)) & 1ull)) return r;
    r.verdict = XSK_GPU_UNREACH_LEFT;
    if (ur_open(d_open, udp_port)) return r;
    r.verdict = XSK_GPU_UNREACH_NO_ROOM;  // (addr <= umem_size by rule 1)
    if ((addr & (uint64_t)(chunk_size - 1u)) + reply_len > chunk_size || reply_len > umem_size - addr) return r;
    r.verdict = reply;
    r.port = port;
    r.reply_len = reply_len;
    r.q = q;
    r.mac_lo = e[6];
    r.mac_hi = e[7];
    return r;
}

// One frame.  `tab` is the staged table (ng_stage_entry), n_entries of it; `bound` the word of *d_bound (all ones for
// NULL); d_open the 8192-byte map or NULL; chunk_size a power of two in [2048, 2^20].  Changes nothing.
XSK_UR_FN UrVerdict ur_decide(const uint8_t* umem, uint64_t umem_size, const xsk_gpu_desc& d, uint32_t opts,
                              const uint32_t* tab, uint32_t n_entries, uint32_t n_ports, uint64_t bound,
                              const uint8_t* d_open, uint32_t chunk_size) {
    UrVerdict r = ur_none();
    const uint64_t a = d.addr;
    const uint32_t len = d.len;
    if (len > XSK_GPU_MAX_LEN || a > umem_size || len > umem_size - a) return r;  // rule 1
    if (len < 14) return r;
    const uint8_t* p = umem + a;
    uint32_t l3 = 14, et = ng_be16(p, 12);  // rule 2
    if ((opts & XSK_GPU_OPT_VLAN) && cw_is_tpid(et)) {
        if (len < 18) return r;
        et = ng_be16(p, 16);
        l3 = 18;
        if (cw_is_tpid(et)) {
            if (len < 22) return r;
            et = ng_be16(p, 20);
            l3 = 22;
        }
    }
    r.l3 = l3;
    uint32_t key[kNgKeyWords] = {0u, 0u, 0u, 0u, 0u};
    if (et == 0x0800u) {  // rule 3
        if (len < l3 + 20u || (p[l3] >> 4) != 4u) return r;  // a
        const uint32_t hl = 4u * (p[l3] & 0xFu);
        if (hl < 20u || len < l3 + hl || p[l3 + 9u] != 17u) return r;
        r.verdict = XSK_GPU_UNREACH_MALFORMED;  // b
        const uint32_t tl = ng_be16(p, l3 + 2u);
        if (tl < hl + 8u || l3 + tl > len) return r;
        uint64_t sum = 0;
        for (uint32_t k = 0; k < hl; k += 2u) sum += ng_be16(p, l3 + k);
        if (ng_fold(sum) != 0xFFFFu) return r;
        r.verdict = XSK_GPU_UNREACH_LEFT;  // c
        if ((ng_be16(p, l3 + 6u) & 0x1FFFu) != 0u || (p[0] & 1u) || p[l3 + 16u] >= 224u) return r;
        const uint32_t S = ng_be32(p, l3 + 12u);
        if (S == 0u || (S >> 24) >= 224u || (S >> 24) == 127u) return r;
        key[0] = 4u;  // d
        key[1] = ng_be32(p, l3 + 16u);
        return ur_resolve(r, key, tab, n_entries, n_ports, bound, d_open, ng_be16(p, l3 + hl + 2u), a, umem_size, chunk_size,
                          XSK_GPU_UNREACH_UNREACH4, hl + 8u, l3 + 28u + hl + 8u);  // e, f, g
    }
    if (et != 0x86DDu || !(opts & XSK_GPU_OPT_IPV6)) return r;  // rule 5
    // rule 4
    if (len < l3 + 40u || (p[l3] >> 4) != 6u || p[l3 + 6u] != 17u) return r;  // a
    r.verdict = XSK_GPU_UNREACH_MALFORMED;  // b
    const uint32_t pl = ng_be16(p, l3 + 4u);
    if (pl < 8u || l3 + 40u + pl > len || ng_be16(p, l3 + 46u) == 0u) return r;
    r.verdict = XSK_GPU_UNREACH_LEFT;  // c
    uint32_t src_any = 0u;
    for (uint32_t k = 0; k < 16u; ++k) src_any |= p[l3 + 8u + k];
    if ((p[0] & 1u) || p[l3 + 24u] == 0xFFu || src_any == 0u || p[l3 + 8u] == 0xFFu) return r;
    key[0] = 6u;  // d
    for (uint32_t k = 0; k < 4u; ++k) key[1u + k] = ng_be32(p, l3 + 24u + 4u * k);
    const uint32_t q = cw_min(40u + pl, kUrMaxQuote6);  // e
    return ur_resolve(r, key, tab, n_entries, n_ports, bound, d_open, ng_be16(p, l3 + 42u), a, umem_size, chunk_size,
                      XSK_GPU_UNREACH_UNREACH6, q, l3 + 48u + q);  // f
}

// ---- the reply's geometry and checksums, from the quote's sums ----
XSK_UR_FN uint32_t ur_hdr(uint32_t verdict) { return verdict == XSK_GPU_UNREACH_UNREACH6 ? 48u : 28u; }  // IP + 8
// The message checksum: `quote` the RFC 1071 sum of the quoted bytes (an odd last byte a high byte), `addrs` the sum of
// old source and destination as 16-bit words (IPv6: the pseudo-header's; IPv4: not used).
XSK_UR_FN uint32_t ur_msg_csum(uint32_t verdict, uint32_t q, uint64_t quote, uint64_t addrs) {
    const uint64_t s = verdict == XSK_GPU_UNREACH_UNREACH6 ? quote + addrs + (8u + q) + 58u + 0x0104u : quote + 0x0303u;
    return ~ng_fold(s) & 0xFFFFu;
}
// The IPv4 header's: 45 00, 28 + q, 00 00, 40 00, 40 01, the addresses.
XSK_UR_FN uint32_t ur_ip_csum(uint32_t q, uint64_t addrs) {
    return ~ng_fold(addrs + 0x4500u + (28u + q) + 0x4000u + 0x4001u) & 0xFFFFu;
}
// Byte k < ur_hdr() of the fresh headers at l3, except the swapped addresses (ur_hdr_swap() says where those come from).
XSK_UR_FN uint32_t ur_hdr_byte(uint32_t verdict, uint32_t k, uint32_t q, uint32_t ipcs, uint32_t cs) {
    if (verdict == XSK_GPU_UNREACH_UNREACH6) {
        const uint32_t plen = 8u + q;
        switch (k) {
            case 0: return 0x60u;
            case 4: return plen >> 8;
            case 5: return plen & 0xFFu;
            case 6: return 0x3Au;
            case 7: return 0x40u;
            case 40: return 1u;
            case 41: return 4u;
            case 42: return cs >> 8;
            case 43: return cs & 0xFFu;
            default: return 0u;
        }
    }
    const uint32_t tl = 28u + q;
    switch (k) {
        case 0: return 0x45u;
        case 2: return tl >> 8;
        case 3: return tl & 0xFFu;
        case 6: return 0x40u;
        case 8: return 0x40u;
        case 9: return 1u;
        case 10: return ipcs >> 8;
        case 11: return ipcs & 0xFFu;
        case 20: return 3u;
        case 21: return 3u;
        case 22: return cs >> 8;
        case 23: return cs & 0xFFu;
        default: return 0u;
    }
}
// Header byte k is the OLD header byte ur_hdr_swap(k) (src = old dst, dst = old src), or kNgMiss where it is fresh.
XSK_UR_FN uint32_t ur_hdr_swap(uint32_t verdict, uint32_t k) {
    if (verdict == XSK_GPU_UNREACH_UNREACH6) return k >= 8u && k < 24u ? k + 16u : (k >= 24u && k < 40u ? k - 16u : kNgMiss);
    return k >= 12u && k < 16u ? k + 4u : (k >= 16u && k < 20u ? k - 4u : kNgMiss);
}
// Old header byte k < 64 is one of the addresses (both sums count it: the IPv4 header's and the IPv6 pseudo-header's).
XSK_UR_FN bool ur_is_addr(uint32_t verdict, uint32_t k) {
    return verdict == XSK_GPU_UNREACH_UNREACH6 ? (k >= 8u && k < 40u) : (k >= 12u && k < 20u);
}

// ---- the rewrite, one thread (rules 3g and 4f).  `p` is the frame's first byte. ----
XSK_UR_FN void ur_rewrite(uint8_t* p, const UrVerdict& v) {
    if (!ur_is_reply(v.verdict)) return;
    const uint32_t l3 = v.l3, q = v.q, H = ur_hdr(v.verdict);
    uint64_t quote = 0, addrs = 0;
    for (uint32_t k = 0; k < q; ++k) quote += (k & 1u) ? (uint32_t)p[l3 + k] : (uint32_t)p[l3 + k] << 8;
    for (uint32_t k = 0; k < H; ++k)
        if (ur_is_addr(v.verdict, k)) addrs += (k & 1u) ? (uint32_t)p[l3 + k] : (uint32_t)p[l3 + k] << 8;
    const uint32_t cs = ur_msg_csum(v.verdict, q, quote, addrs), ipcs = ur_ip_csum(q, addrs);
    for (uint32_t k = 0; k < 6u; ++k) p[k] = p[6u + k];
    ng_put_mac(p + 6, v.mac_lo, v.mac_hi);
    for (uint32_t k = q; k-- > 0;) p[l3 + H + k] = p[l3 + k];  // the destination lies above the source: from the top down
    for (uint32_t k = 0; k < H; ++k) {  // the old header now stands at l3 + H
        const uint32_t from = ur_hdr_swap(v.verdict, k);
        p[l3 + k] = from != kNgMiss ? p[l3 + H + from] : (uint8_t)ur_hdr_byte(v.verdict, k, q, ipcs, cs);
    }
}

// ---- the rewrite, a wave of 64 lanes: lane k owns quote bytes k, k + 64, ... ----
struct UrLane {
    uint8_t b[kUrLaneBytes];  // quote byte lane + 64 j (0 behind the quote)
    uint8_t smac;             // lanes 0-5: old byte 6 + lane
};
// Phase 1: only loads.
XSK_UR_FN UrLane ur_lane_load(const uint8_t* p, uint32_t l3, uint32_t q, uint32_t lane) {
    UrLane r;
    for (uint32_t j = 0; j < kUrLaneBytes; ++j) {
        const uint32_t i = lane + kUrWave * j;
        r.b[j] = i < q ? p[l3 + i] : (uint8_t)0;
    }
    r.smac = lane < 6u ? p[6u + lane] : (uint8_t)0;
    return r;
}
// Phase 2: this lane's part of the two sums, the quote's in the low and the addresses' in the high 32 bits (64 * 20 * 255
// * 256 and 32 * 255 * 256 are below 2^32).  A lane's bytes all stand at its own parity: 64 is even, and the quote begins
// at an even offset (8) of the message.
XSK_UR_FN uint64_t ur_lane_part(const UrLane& r, uint32_t verdict, uint32_t lane) {
    uint32_t s = 0;
    for (uint32_t j = 0; j < kUrLaneBytes; ++j) s += r.b[j];
    const uint32_t sh = (lane & 1u) ? 0u : 8u;
    const uint64_t a = ur_is_addr(verdict, lane) ? (uint64_t)r.b[0] << sh : 0ull;
    return ((uint64_t)s << sh) | (a << 32);
}
// Phase 3: only stores, behind every lane's loads.  `total` is the sum of the 64 parts; `swapped` the b[0] of lane
// ur_hdr_swap(verdict, lane) (anything where that is kNgMiss).
XSK_UR_FN void ur_lane_store(uint8_t* p, const UrLane& r, const UrVerdict& v, uint32_t lane, uint64_t total,
                             uint32_t swapped) {
    const uint32_t l3 = v.l3, q = v.q, H = ur_hdr(v.verdict);
    for (uint32_t j = 0; j < kUrLaneBytes; ++j) {
        const uint32_t i = lane + kUrWave * j;
        if (i < q) p[l3 + H + i] = r.b[j];
    }
    if (lane < H) {
        const uint64_t quote = total & 0xFFFFFFFFull, addrs = total >> 32;
        const uint32_t cs = ur_msg_csum(v.verdict, q, quote, addrs), ipcs = ur_ip_csum(q, addrs);
        p[l3 + lane] = ur_hdr_swap(v.verdict, lane) != kNgMiss ? (uint8_t)swapped
                                                              : (uint8_t)ur_hdr_byte(v.verdict, lane, q, ipcs, cs);
    }
    if (lane < 6u) {
        p[lane] = r.smac;
        p[6u + lane] = (uint8_t)((lane < 4u ? v.mac_lo >> (8u * lane) : v.mac_hi >> (8u * (lane - 4u))));
    }
}

// ---- the serve plan (xsk_gpu_unreach_serve_dev(): one workgroup, lane j owns entry j of `up`) ----
// As xsk_neigh.h's (ng_serve_m, ng_stop_at: reused), with one step in front: an entry decided UNREACH4 / UNREACH6 whose
// rank among such entries is not below the budget becomes LIMITED and goes to `rest`.  Below the stopping lane the
// eligible entries that kept their verdict are exactly those of rank 0 .. n-1, n the budget spent: the rank names the
// job slot a wave finds the rewrite in.
XSK_UR_FN uint32_t ur_limit(uint32_t verdict, uint32_t eligible_rank, uint32_t budget) {
    return ur_is_reply(verdict) && eligible_rank >= budget ? (uint32_t)XSK_GPU_UNREACH_LIMITED : verdict;
}
XSK_UR_FN uint32_t ur_dest(uint32_t verdict, uint32_t port) { return ur_is_reply(verdict) ? port : kNgUp; }
XSK_UR_FN xsk_gpu_desc ur_out_entry(const xsk_gpu_desc& e, const UrVerdict& v) {
    xsk_gpu_desc o = e;
    if (ur_is_reply(v.verdict)) {
        o.len = v.reply_len;
        o.options = 0u;
    }
    return o;
}
// A rewrite as five words of LDS.
struct UrJob {
    uint32_t addr_lo, addr_hi, geo, mac_lo, mac_hi;  // geo: l3 | q << 8 | (UNREACH6 ? 1 << 24 : 0)
};
XSK_UR_FN UrJob ur_job(uint64_t addr, const UrVerdict& v) {
    return UrJob{(uint32_t)addr, (uint32_t)(addr >> 32),
                 v.l3 | (v.q << 8) | (v.verdict == XSK_GPU_UNREACH_UNREACH6 ? 1u << 24 : 0u), v.mac_lo, v.mac_hi};
}
XSK_UR_FN UrVerdict ur_job_verdict(const UrJob& j) {
    UrVerdict v = ur_none();
    v.verdict = (j.geo >> 24) & 1u ? XSK_GPU_UNREACH_UNREACH6 : XSK_GPU_UNREACH_UNREACH4;
    v.l3 = j.geo & 0xFFu;
    v.q = (j.geo >> 8) & 0xFFFFu;
    v.reply_len = v.l3 + ur_hdr(v.verdict) + v.q;
    v.mac_lo = j.mac_lo;
    v.mac_hi = j.mac_hi;
    return v;
}
XSK_UR_FN uint64_t ur_job_addr(const UrJob& j) { return ((uint64_t)j.addr_hi << 32) | j.addr_lo; }

}  // namespace xskgpu

#endif  // XSK_UNREACH_H
