#!/usr/bin/env python3
"""Golden vectors for the neighbour responder (xsk_gpu_neigh_dev, include/xsk_gpu.h "Neighbour responder").

A restatement of the rule that parses nothing: every frame is built field by field from its parameters (RFC 826 ARP,
RFC 4861 neighbour solicitation / advertisement, RFC 8200 header and §8.1 pseudo-header, RFC 1071 sums, IEEE 802.1Q /
802.1ad tags), and what the responder must make of it follows from those parameters -- which tags the option word lets
it see through, which field the case spoiled, and the reply again built field by field.  It shares no code with
tests/neigh_spec.py.

    python tests/golden/make_neigh_golden.py   ->  tests/golden/neigh.json

Every case is built with 0, 1, 2 and 3 VLAN tags and judged under opts 0, 0x2, 0x10, 0x12 and 0x17.
"""
import json
import os
import struct

_HERE = os.path.dirname(os.path.abspath(__file__))
NONE, ARP_REPLY, NA_REPLY, MALFORMED, UNKNOWN, UNBOUND, LEFT = range(7)
OPT_VLAN, OPT_IPV6 = 0x2, 0x10
OPTS = (0, 0x2, 0x10, 0x12, 0x17)
TAGS = ((), ((0x8100, 0x0064),), ((0x88A8, 0x2001), (0x8100, 0x0FFE)), ((0x8100, 1), (0x8100, 2), (0x8100, 3)))

N_PORTS = 8
BOUND = 0xFFFFFFFFFFFFFFFF & ~(1 << 5)  # port 5 is not bound
PEER_MAC = bytes.fromhex("02aabbccdd01")
PEER4 = bytes([192, 0, 2, 77])
PEER6 = bytes.fromhex("20010db8000000000000000000000077")
BCAST = b"\xff" * 6
# the addresses the process owns: (family, address, port, mac)
OWN4 = (4, bytes([192, 0, 2, 1]), 3, bytes.fromhex("020000000a03"))
OWN4_HIGH = (4, bytes([192, 0, 2, 9]), 9, bytes.fromhex("020000000a09"))   # a port at or above n_ports
OWN4_OFF = (4, bytes([192, 0, 2, 5]), 5, bytes.fromhex("020000000a05"))    # a port whose bound bit is clear
OWN6 = (6, bytes.fromhex("20010db80000000000000000000000fe"), 7, bytes.fromhex("0200000006fe"))
OWN6_LL = (6, bytes.fromhex("fe80000000000000000000fffe0006fe"), 0, bytes.fromhex("0600000006ff"))
OWN6_OFF = (6, bytes.fromhex("20010db8000000000000000000000005"), 5, bytes.fromhex("020000000605"))
TABLE = (OWN4, OWN4_HIGH, OWN4_OFF, OWN6, OWN6_LL, OWN6_OFF)
STRANGER4 = bytes([192, 0, 2, 200])
STRANGER6 = bytes.fromhex("20010db80000000000000000000000aa")


def ones_sum(data: bytes) -> int:
    """RFC 1071 over big-endian 16-bit words, folded."""
    if len(data) % 2:
        data += b"\0"
    total = sum(struct.unpack("!%dH" % (len(data) // 2), data))
    while total > 0xFFFF:
        total = (total & 0xFFFF) + (total >> 16)
    return total


def eth(dst, src, tags, ethertype):
    out = dst + src
    for tpid, tci in tags:
        out += struct.pack("!HH", tpid, tci)
    return out + struct.pack("!H", ethertype)


def arp(op, sha, spa, tha, tpa, htype=1, ptype=0x0800, hlen=6, plen=4):
    return struct.pack("!HHBBH", htype, ptype, hlen, plen, op) + sha + spa + tha + tpa


def ip6(src, dst, payload, nh=58, hlim=255, version=6, plen=None, tc_flow=0x0A12345):
    word = (version << 28) | tc_flow
    return struct.pack("!IHBB", word, len(payload) if plen is None else plen, nh, hlim) + src + dst + payload


def icmp6(src, dst, mtype, code, body, spoil=False, length=None):
    """An ICMPv6 message with its checksum over the pseudo-header (src, dst, length, 58)."""
    msg = struct.pack("!BBH", mtype, code, 0) + body
    n = len(msg) if length is None else length
    cs = ~ones_sum(src + dst + struct.pack("!IHBB", n, 0, 0, 58) + msg) & 0xFFFF
    if spoil:
        cs ^= 0x0101
    return msg[:2] + struct.pack("!H", cs) + msg[4:]


def solicited_node(target):
    return bytes.fromhex("ff0200000000000000000001ff") + target[13:]


def slla(mac):
    return bytes([1, 1]) + mac


# ---- the cases: name -> (family, builder(tags) -> frame, verdict when the responder sees the packet, reply builder) ----
def arp_case(tpa_entry=OWN4, tpa=None, op=1, pad=0, cut=None, **fields):
    tpa = tpa_entry[1] if tpa is None else tpa

    def frame(tags):
        f = eth(BCAST, PEER_MAC, tags, 0x0806) + arp(op, PEER_MAC, PEER4, bytes(6), tpa, **fields) + b"\xa5" * pad
        return f if cut is None else f[:14 + 4 * len(tags) + cut]

    def reply(tags):
        m = tpa_entry[3]
        return eth(PEER_MAC, m, tags, 0x0806) + arp(2, m, tpa, PEER_MAC, PEER4) + b"\xa5" * pad, None, tpa_entry[2]

    return frame, reply


def ns_case(target_entry=OWN6, target=None, src=PEER6, options=None, pad=0, cut=None, mtype=135, code=0, spoil=False,
            plen_delta=0, extra=b"", **ipf):
    target = target_entry[1] if target is None else target
    options = slla(PEER_MAC) if options is None else options

    def frame(tags):
        dst = solicited_node(target)
        body = bytes(4) + target + options + extra
        msg = icmp6(src, dst, mtype, code, body, spoil, length=len(body) + 4 + plen_delta if plen_delta else None)
        f = eth(b"\x33\x33\xff" + target[13:], PEER_MAC, tags, 0x86DD)
        f += ip6(src, dst, msg, plen=len(msg) + plen_delta if plen_delta else None, **ipf) + b"\x5a" * pad
        return f if cut is None else f[:14 + 4 * len(tags) + cut]

    def reply(tags):
        m = target_entry[3]
        na = icmp6(target, src, 136, 0, bytes([0x60, 0, 0, 0]) + target + bytes([2, 1]) + m)
        out = eth(PEER_MAC, m, tags, 0x86DD) + ip6(target, src, na, tc_flow=0)
        return out, len(out), target_entry[2]  # the request's bytes behind the reply's end stay

    return frame, reply


def other_case(builder):
    return (lambda tags: builder(tags)), None


def tcp4(tags):
    ip = struct.pack("!BBHHHBBH", 0x45, 0, 40, 1, 0, 64, 6, 0) + PEER4 + OWN4[1]
    return eth(OWN4[3], PEER_MAC, tags, 0x0800) + ip + bytes(20)


def tag_cut(tags):
    """The last tag cut by the frame's end (no tag: 13 bytes, below an Ethernet header)."""
    return eth(BCAST, PEER_MAC, tags, 0x0806)[:-3] if tags else (BCAST + PEER_MAC + b"\x08")


def opt_zero_len():
    return slla(PEER_MAC) + bytes([14, 0]) + bytes(6)


def opt_overrun():
    return slla(PEER_MAC) + bytes([14, 2]) + bytes(6)


def long_options(total):
    """Options that fill `total` bytes: the source link-layer address, nonce-like options of 16 bytes, one of 8."""
    out = slla(PEER_MAC)
    while len(out) + 16 <= total:
        out += bytes([14, 2]) + bytes(range(14))
    if len(out) < total:
        out += bytes([14, 1]) + bytes(range(6))
    assert len(out) == total
    return out


# (name, family, (frame, reply), verdict when seen)
CASES = [
    # rule 3
    ("arp_request", 4, arp_case(), ARP_REPLY),                                         # 3f
    ("arp_request_padded", 4, arp_case(pad=18), ARP_REPLY),                            # 3f: a minimum-size frame's padding stays
    ("arp_cut", 4, arp_case(cut=27), MALFORMED),                                       # 3a
    ("arp_cut_to_header", 4, arp_case(cut=0), MALFORMED),                              # 3a
    ("arp_htype", 4, arp_case(htype=6), MALFORMED),                                    # 3b
    ("arp_ptype", 4, arp_case(ptype=0x86DD), MALFORMED),
    ("arp_hlen", 4, arp_case(hlen=8), MALFORMED),
    ("arp_plen", 4, arp_case(plen=16), MALFORMED),
    ("arp_is_reply", 4, arp_case(op=2), NONE),                                         # 3c
    ("arp_rarp_op", 4, arp_case(op=3), NONE),
    ("arp_stranger", 4, arp_case(tpa=STRANGER4), UNKNOWN),                             # 3d
    ("arp_port_high", 4, arp_case(tpa_entry=OWN4_HIGH), UNBOUND),                      # 3e
    ("arp_port_unbound", 4, arp_case(tpa_entry=OWN4_OFF), UNBOUND),
    # rule 4
    ("ns_request", 6, ns_case(), NA_REPLY),                                            # 4i: pl == 32, reply fills the frame
    ("ns_link_local_padded", 6, ns_case(target_entry=OWN6_LL, pad=9), NA_REPLY),       # bytes behind l3 + 72 stay
    ("ns_two_options", 6, ns_case(options=slla(PEER_MAC) + bytes([14, 1]) + bytes(6)), NA_REPLY),
    ("ns_pl_280", 6, ns_case(options=long_options(256)), NA_REPLY),                    # 4d's bound itself
    ("ns_option_to_last_byte", 6, ns_case(options=bytes([14, 2]) + bytes(14)), NA_REPLY),
    ("ns_cut_header", 6, ns_case(cut=39), NONE),                                       # 4a
    ("ns_version", 6, ns_case(version=5), NONE),
    ("ns_udp", 6, ns_case(nh=17), NONE),
    ("ns_cut_icmp", 6, ns_case(cut=47), MALFORMED),                                    # 4b
    ("echo_request", 6, ns_case(mtype=128), NONE),
    ("advert", 6, ns_case(mtype=136), NONE),
    ("ns_hop_limit", 6, ns_case(hlim=64), MALFORMED),                                  # 4c, in its order
    ("ns_code", 6, ns_case(code=1), MALFORMED),
    ("ns_pl_16", 6, ns_case(plen_delta=-16), MALFORMED),
    ("ns_pl_overrun", 6, ns_case(plen_delta=8), MALFORMED),
    ("ns_cut_in_options", 6, ns_case(cut=71), MALFORMED),
    ("ns_target_multicast", 6, ns_case(target=bytes.fromhex("ff020000000000000000000000000001")), MALFORMED),
    ("ns_pl_not_8", 6, ns_case(extra=bytes(4)), MALFORMED),
    ("ns_pl_288", 6, ns_case(options=long_options(264)), LEFT),                        # 4d
    ("ns_pl_288_bad_sum", 6, ns_case(options=long_options(264), spoil=True), LEFT),    # 4d stands in front of 4f
    ("ns_option_len_0", 6, ns_case(options=opt_zero_len()), MALFORMED),                # 4e
    ("ns_option_overrun", 6, ns_case(options=opt_overrun()), MALFORMED),
    ("ns_bad_sum", 6, ns_case(spoil=True), MALFORMED),                                 # 4f
    ("ns_dad", 6, ns_case(src=bytes(16), options=b""), LEFT),                          # 4g
    ("ns_dad_with_option", 6, ns_case(src=bytes(16)), LEFT),
    ("ns_no_option", 6, ns_case(options=b""), LEFT),
    ("ns_stranger", 6, ns_case(target=STRANGER6), UNKNOWN),                            # 4h
    ("ns_port_unbound", 6, ns_case(target_entry=OWN6_OFF), UNBOUND),
    # rules 2 and 5
    ("tag_cut", 0, other_case(tag_cut), NONE),
    ("tcp4", 0, other_case(tcp4), NONE),
    ("lldp", 0, other_case(lambda tags: eth(BCAST, PEER_MAC, tags, 0x88CC) + bytes(46)), NONE),
    ("empty", 0, other_case(lambda tags: b""), NONE),
]


def expect(family, seen_verdict, reply, tags, opts, frame):
    """What the responder makes of a case under one option word: it sees the packet behind no tag, or behind up to two
    with XSK_GPU_OPT_VLAN; a solicitation only with XSK_GPU_OPT_IPV6; anything it does not see is NONE."""
    sees = not tags or (opts & OPT_VLAN and len(tags) <= 2)
    if not sees or family == 0 or (family == 6 and not opts & OPT_IPV6):
        return dict(verdict=NONE, port=0xFF)
    if seen_verdict not in (ARP_REPLY, NA_REPLY):
        return dict(verdict=seen_verdict, port=0xFF)
    out, cut, port = reply(tags)
    if cut is not None:
        out = out + frame[cut:]
    assert len(out) == len(frame)
    return dict(verdict=seen_verdict, port=port, reply=out.hex(), reply_len=len(frame) if cut is None else cut)


def main():
    cases = []
    for name, family, (frame, reply), verdict in CASES:
        for k, tags in enumerate(TAGS):
            f = frame(tags)
            exp = {}
            for opts in OPTS:
                exp["0x%x" % opts] = expect(family, verdict, reply, tags, opts, f)
            cases.append(dict(name=name, tags=k, frame=f.hex(), expect=exp))
    doc = dict(n_ports=N_PORTS, bound="0x%016x" % BOUND, opts=list(OPTS),
               table=[dict(family=e[0], addr=e[1].hex(), port=e[2], mac=e[3].hex()) for e in TABLE], cases=cases)
    with open(os.path.join(_HERE, "neigh.json"), "w") as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(len(cases), "cases")


if __name__ == "__main__":
    main()
