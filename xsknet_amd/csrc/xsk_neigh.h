// xsk_neigh.h — the per-frame decision, the lookup, the two rewrites and the serve plan of xsk_gpu_neigh_dev() and
// xsk_gpu_neigh_serve_dev() (include/xsk_gpu.h, "Neighbour responder"): the responder that answers ARP
// requests (RFC 826) and neighbour solicitations (RFC 4861 §7.1.1, §7.2.4) for the addresses of a sorted table of at
// most 1024 entries, in place.  Host and device: xsk_neigh.hip's kernels call these functions, and
// tests/c/test_neigh.cpp runs them on the CPU under AddressSanitizer -- the decision on frames in heap buffers of
// exactly len bytes, the search on tables of exactly n_entries entries, the serve plan replayed lane by lane into rings
// of exactly their sizes.
//
// The decision (ng_decide) only reads, and only bytes of [addr, addr + len): every read stands behind the length check
// that covers it.  The rewrites (ng_rewrite_arp, ng_rewrite_na) are separate, so that xsk_gpu_neigh_serve_dev() can
// decide every entry, find where the call stops, and rewrite only what it has a slot for.  Frames may lie at odd
// addresses: every access is a byte access.
#ifndef XSK_NEIGH_H
#define XSK_NEIGH_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/xsk_gpu.h"
#include "xsk_classify_wire.h"

#define XSK_NG_FN XSK_CW_FN

namespace xskgpu {

constexpr uint32_t kNgMaxEntries = XSK_GPU_NEIGH_MAX_ENTRIES;
constexpr uint32_t kNgMaxPorts = 64;
constexpr uint32_t kNgKeyWords = 5;    // family, then the address as four big-endian dwords: integer order == memcmp order
constexpr uint32_t kNgEntryWords = 8;  // a staged entry: the key, the port, mac[0..4) and mac[4..6) little-endian
constexpr uint32_t kNgMiss = 0xFFFFFFFFu;
constexpr uint32_t kNgMaxPl = 280;     // rule 4d: the longest solicitation a lane sums
constexpr uint32_t kNgUp = kNgMaxPorts;         // the serve call's destinations: port p's TX ring is p, `up` is 64
constexpr uint32_t kNgDests = kNgMaxPorts + 1u;

// ---- the table ----
XSK_NG_FN uint32_t ng_bswap(uint32_t w) { return __builtin_bswap32(w); }

// One entry of the caller's table (24 bytes, 8-B aligned) as eight dwords: what the kernels keep in LDS.
XSK_NG_FN void ng_stage_entry(const xsk_gpu_neigh_entry* e, uint32_t* out) {
    uint32_t w[6];
    __builtin_memcpy(w, e, 24);
    out[0] = w[4] & 0xFFu;  // family
    out[1] = ng_bswap(w[0]);
    out[2] = ng_bswap(w[1]);
    out[3] = ng_bswap(w[2]);
    out[4] = ng_bswap(w[3]);
    out[5] = (w[4] >> 8) & 0xFFu;          // port
    out[6] = (w[4] >> 16) | (w[5] << 16);  // mac[0..4)
    out[7] = w[5] >> 16;                   // mac[4..6)
}

// The index of the staged entry whose key is `key`, or kNgMiss.  Binary search with a three-way compare: every probe is
// of an index in [0, n), whatever the table holds, so a table that was not prepared can only miss.
XSK_NG_FN uint32_t ng_lookup(const uint32_t* tab, uint32_t n, const uint32_t* key) {
    uint32_t lo = 0, hi = n, at = kNgMiss;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t* e = tab + (size_t)mid * kNgEntryWords;
        int c = 0;  // sign of entry - key
        for (uint32_t k = kNgKeyWords; k-- > 0;) c = e[k] != key[k] ? (e[k] < key[k] ? -1 : 1) : c;
        if (c == 0) {
            at = mid;
            break;
        }
        if (c < 0)
            lo = mid + 1;
        else
            hi = mid;
    }
    return at;
}

// ---- the decision ----
struct NgVerdict {
    uint32_t verdict;    // XSK_GPU_NEIGH_*
    uint32_t port;       // the entry's port with ARP_REPLY / NA_REPLY, 0xFF otherwise
    uint32_t reply_len;  // with ARP_REPLY / NA_REPLY
    uint32_t l3;         // where the ARP packet / the IPv6 header begins
    uint32_t mac_lo, mac_hi;  // the entry's mac: bytes 0-3 and 4-5, little-endian
};

XSK_NG_FN bool ng_is_reply(uint32_t verdict) {
    return verdict == XSK_GPU_NEIGH_ARP_REPLY || verdict == XSK_GPU_NEIGH_NA_REPLY;
}
XSK_NG_FN uint32_t ng_be16(const uint8_t* p, uint32_t o) { return ((uint32_t)p[o] << 8) | p[o + 1u]; }
XSK_NG_FN uint32_t ng_be32(const uint8_t* p, uint32_t o) { return (ng_be16(p, o) << 16) | ng_be16(p, o + 2u); }
XSK_NG_FN uint32_t ng_fold(uint64_t s) {
    while (s >> 16) s = (s & 0xFFFFu) + (s >> 16);
    return (uint32_t)s;
}

// Rules 3d-3f and 4h-4i: the table and the port rule, from a key.
XSK_NG_FN NgVerdict ng_resolve(NgVerdict r, const uint32_t* key, const uint32_t* tab, uint32_t n_entries,
                               uint32_t n_ports, uint64_t bound, uint32_t reply, uint32_t reply_len) {
    const uint32_t at = n_entries ? ng_lookup(tab, n_entries, key) : kNgMiss;
    r.verdict = XSK_GPU_NEIGH_UNKNOWN;
    if (at == kNgMiss) return r;
    const uint32_t* e = tab + (size_t)at * kNgEntryWords;
    const uint32_t port = e[5];
    r.verdict = XSK_GPU_NEIGH_UNBOUND;
    if (port >= n_ports || !((bound >> (port & 63u)) & 1ull)) return r;
    r.verdict = reply;
    r.port = port;
    r.reply_len = reply_len;
    r.mac_lo = e[6];
    r.mac_hi = e[7];
    return r;
}

// One frame.  `tab` is the staged table (ng_stage_entry), n_entries of it; `bound` the word of *d_bound (all ones for
// NULL).  Changes nothing.
XSK_NG_FN NgVerdict ng_decide(const uint8_t* umem, uint64_t umem_size, const xsk_gpu_desc& d, uint32_t opts,
                              const uint32_t* tab, uint32_t n_entries, uint32_t n_ports, uint64_t bound) {
    NgVerdict r = {XSK_GPU_NEIGH_NONE, 0xFFu, 0u, 14u, 0u, 0u};
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
    if (et == 0x0806u) {  // rule 3
        r.verdict = XSK_GPU_NEIGH_MALFORMED;
        if (len < l3 + 28u) return r;                                                                // a
        if (ng_be16(p, l3) != 1u || ng_be16(p, l3 + 2u) != 0x0800u || p[l3 + 4u] != 6u || p[l3 + 5u] != 4u) return r;  // b
        r.verdict = XSK_GPU_NEIGH_NONE;
        if (ng_be16(p, l3 + 6u) != 1u) return r;  // c
        key[0] = 4u;
        key[1] = ng_be32(p, l3 + 24u);
        return ng_resolve(r, key, tab, n_entries, n_ports, bound, XSK_GPU_NEIGH_ARP_REPLY, len);  // d, e, f
    }
    if (et != 0x86DDu || !(opts & XSK_GPU_OPT_IPV6)) return r;  // rule 5
    // rule 4
    if (len < l3 + 40u || (p[l3] >> 4) != 6u || p[l3 + 6u] != 58u) return r;  // a
    r.verdict = XSK_GPU_NEIGH_MALFORMED;
    if (len < l3 + 48u) return r;  // b
    r.verdict = XSK_GPU_NEIGH_NONE;
    if (p[l3 + 40u] != 135u) return r;
    r.verdict = XSK_GPU_NEIGH_MALFORMED;
    const uint32_t pl = ng_be16(p, l3 + 4u);
    if (p[l3 + 7u] != 255u || p[l3 + 41u] != 0u || pl < 24u || l3 + 40u + pl > len) return r;  // c
    if (p[l3 + 48u] == 0xFFu || ((pl - 24u) & 7u) != 0u) return r;
    if (pl > kNgMaxPl) {  // d
        r.verdict = XSK_GPU_NEIGH_LEFT;
        return r;
    }
    const uint8_t* msg = p + l3 + 40u;
    for (uint32_t o = 24u; o < pl;) {  // e: o and pl are multiples of 8, so o + 1 < pl
        const uint32_t L = msg[o + 1u];
        if (L == 0u || o + 8u * L > pl) return r;
        o += 8u * L;
    }
    uint64_t sum = (uint64_t)pl + 58u;  // f: source and destination, [l3 + 8, l3 + 40), lie in front of the message
    for (uint32_t k = l3 + 8u; k < l3 + 40u + pl; k += 2u) sum += ng_be16(p, k);
    if (ng_fold(sum) != 0xFFFFu) return r;
    r.verdict = XSK_GPU_NEIGH_LEFT;  // g
    uint32_t src_any = 0u;
    for (uint32_t k = 0; k < 16u; ++k) src_any |= p[l3 + 8u + k];
    if (src_any == 0u || pl < 32u) return r;
    key[0] = 6u;
    for (uint32_t k = 0; k < 4u; ++k) key[1u + k] = ng_be32(p, l3 + 48u + 4u * k);
    return ng_resolve(r, key, tab, n_entries, n_ports, bound, XSK_GPU_NEIGH_NA_REPLY, l3 + 72u);  // h, i
}

// ---- the rewrites ----
XSK_NG_FN void ng_put_mac(uint8_t* p, uint32_t lo, uint32_t hi) {
    p[0] = (uint8_t)lo;
    p[1] = (uint8_t)(lo >> 8);
    p[2] = (uint8_t)(lo >> 16);
    p[3] = (uint8_t)(lo >> 24);
    p[4] = (uint8_t)hi;
    p[5] = (uint8_t)(hi >> 8);
}

// Rule 3f.  `p` is the frame's first byte.
XSK_NG_FN void ng_rewrite_arp(uint8_t* p, const NgVerdict& v) {
    const uint32_t l3 = v.l3;
    uint8_t sha[6], spa[4], tpa[4];
    for (uint32_t k = 0; k < 6u; ++k) sha[k] = p[l3 + 8u + k];
    for (uint32_t k = 0; k < 4u; ++k) {
        spa[k] = p[l3 + 14u + k];
        tpa[k] = p[l3 + 24u + k];
    }
    for (uint32_t k = 0; k < 6u; ++k) p[k] = sha[k];
    ng_put_mac(p + 6, v.mac_lo, v.mac_hi);
    p[l3 + 6u] = 0u;
    p[l3 + 7u] = 2u;
    ng_put_mac(p + l3 + 8u, v.mac_lo, v.mac_hi);
    for (uint32_t k = 0; k < 4u; ++k) p[l3 + 14u + k] = tpa[k];
    for (uint32_t k = 0; k < 6u; ++k) p[l3 + 18u + k] = sha[k];
    for (uint32_t k = 0; k < 4u; ++k) p[l3 + 24u + k] = spa[k];
}

// Rule 4i.
XSK_NG_FN void ng_rewrite_na(uint8_t* p, const NgVerdict& v) {
    const uint32_t l3 = v.l3;
    uint8_t S[16], T[16], m[6];
    for (uint32_t k = 0; k < 16u; ++k) {
        S[k] = p[l3 + 8u + k];
        T[k] = p[l3 + 48u + k];
    }
    ng_put_mac(m, v.mac_lo, v.mac_hi);
    for (uint32_t k = 0; k < 6u; ++k) {
        p[k] = p[6u + k];
        p[6u + k] = m[k];
    }
    uint8_t* h = p + l3;
    h[0] = 0x60u;
    h[1] = h[2] = h[3] = 0u;
    h[4] = 0u;
    h[5] = 32u;
    h[6] = 58u;
    h[7] = 255u;
    for (uint32_t k = 0; k < 16u; ++k) {
        h[8u + k] = T[k];
        h[24u + k] = S[k];
        h[48u + k] = T[k];
    }
    h[40] = 0x88u;
    h[41] = 0u;
    h[44] = 0x60u;
    h[45] = h[46] = h[47] = 0u;
    h[64] = 2u;
    h[65] = 1u;
    for (uint32_t k = 0; k < 6u; ++k) h[66u + k] = m[k];
    // pseudo(T, S, 32, 58) and the message with a zero checksum: T counts twice
    uint64_t sum = 32u + 58u + 0x8800u + 0x6000u + 0x0201u;
    for (uint32_t k = 0; k < 16u; k += 2u)
        sum += 2u * (((uint32_t)T[k] << 8) | T[k + 1u]) + (((uint32_t)S[k] << 8) | S[k + 1u]);
    for (uint32_t k = 0; k < 6u; k += 2u) sum += ((uint32_t)m[k] << 8) | m[k + 1u];
    const uint32_t cs = ~ng_fold(sum) & 0xFFFFu;
    h[42] = (uint8_t)(cs >> 8);
    h[43] = (uint8_t)cs;
}

XSK_NG_FN void ng_rewrite(uint8_t* p, const NgVerdict& v) {
    if (v.verdict == XSK_GPU_NEIGH_ARP_REPLY) ng_rewrite_arp(p, v);
    if (v.verdict == XSK_GPU_NEIGH_NA_REPLY) ng_rewrite_na(p, v);
}

// ---- the serve plan (xsk_gpu_neigh_serve_dev(): one workgroup, lane j owns stack entry j) ----
// m = min(used(stack), max) entries are decided.  Entry j goes to destination ng_dest(): its port's TX ring with a reply,
// `up` otherwise, at that destination's producer word plus the entry's rank -- the number of entries below j with the
// same destination.  Entry j stops the call when its rank is not below the destination's room; c, the number of entries
// handled, is the lowest such j, or m.  Below c every rank is a count of handled entries only, so the ranks are the
// slots of the sequential rule.
XSK_NG_FN uint32_t ng_serve_m(uint32_t used, uint32_t max) { return cw_min(used, max); }
XSK_NG_FN uint32_t ng_dest(uint32_t verdict, uint32_t port) { return ng_is_reply(verdict) ? port : kNgUp; }
XSK_NG_FN uint32_t ng_stop_at(uint32_t j, uint32_t m, uint32_t rank, uint32_t room) {
    return j < m && rank >= room ? j : m;
}
// The entry a handled lane stores: the reply's descriptor, or the stack entry as it is.
XSK_NG_FN xsk_gpu_desc ng_out_entry(const xsk_gpu_desc& e, const NgVerdict& v) {
    xsk_gpu_desc o = e;
    if (ng_is_reply(v.verdict)) {
        o.len = v.reply_len;
        o.options = 0u;
    }
    return o;
}

}  // namespace xskgpu

#endif  // XSK_NEIGH_H
