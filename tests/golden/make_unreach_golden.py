#!/usr/bin/env python3
"""Golden vectors for the port-unreachable responder (xsk_gpu_unreach_dev, include/xsk_gpu.h "Port-unreachable
responder").

A restatement of the rule that parses nothing: every frame is built field by field from its parameters (RFC 791 header
with options, RFC 768 UDP, RFC 8200 header, RFC 792 / RFC 4443 errors, RFC 1071 sums, IEEE 802.1Q / 802.1ad tags), and
what the responder must make of it follows from those parameters -- which tags the option word lets it see through,
which field the case spoiled, how much room the chunk leaves -- with the error again built field by field around the
header the case itself built.  It shares no code with tests/unreach_spec.py; the Ethernet and sum primitives, the table
and the peers are make_neigh_golden.py's.

    python tests/golden/make_unreach_golden.py   ->  tests/golden/unreach.json

Every case is built with 0, 1 and 2 VLAN tags and judged under opts 0, 0x2, 0x10, 0x12 and 0x17.
"""
import importlib.util
import json
import os
import struct

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_neigh_golden", os.path.join(_HERE, "make_neigh_golden.py"))
N = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(N)

NONE, UNREACH4, UNREACH6, MALFORMED, UNKNOWN, UNBOUND, LEFT, NO_ROOM, LIMITED = range(9)
OPT_VLAN, OPT_IPV6 = N.OPT_VLAN, N.OPT_IPV6
OPTS = N.OPTS
TAGS = N.TAGS[:3]
N_PORTS, BOUND, TABLE = N.N_PORTS, N.BOUND, N.TABLE
PEER_MAC, PEER4, PEER6 = N.PEER_MAC, N.PEER4, N.PEER6
OWN4, OWN4_HIGH, OWN4_OFF, OWN6, OWN6_LL, OWN6_OFF = N.OWN4, N.OWN4_HIGH, N.OWN4_OFF, N.OWN6, N.OWN6_LL, N.OWN6_OFF
STRANGER4, STRANGER6 = N.STRANGER4, N.STRANGER6
eth, ones_sum = N.eth, N.ones_sum

OPEN_PORTS = (53, 4789, 65535)  # somebody listens here
CLOSED = 33434                  # traceroute's first port


def payload(n):
    return bytes((7 * i + 3) & 0xFF for i in range(n))


def udp(src, dst, sport, dport, data, proto_pseudo, zero_sum=False):
    """A UDP datagram with its checksum over the IPv4 or IPv6 pseudo-header."""
    head = struct.pack("!HHH", sport, dport, 8 + len(data))
    if zero_sum:
        return head + b"\0\0" + data
    cs = ~ones_sum(proto_pseudo(src, dst, 8 + len(data)) + head + b"\0\0" + data) & 0xFFFF
    return head + struct.pack("!H", cs or 0xFFFF) + data


def pseudo4(src, dst, n):
    return src + dst + struct.pack("!BBH", 0, 17, n)


def pseudo6(src, dst, n, nh=17):
    return src + dst + struct.pack("!IHBB", n, 0, 0, nh)


def ip4(src, dst, body, proto=17, ihl=5, version=4, tl=None, frag=0x4000, ttl=57, ident=0xBEEF, tos=0x10, spoil=False,
        real_options=None):
    """An IPv4 header of ihl words (options: no-operation bytes, then end of list) with its checksum, and the body."""
    nopt = 4 * max(ihl, 5) - 20 if real_options is None else real_options
    options = (b"\x01" * (nopt - 1) + b"\x00") if nopt else b""
    head = struct.pack("!BBHHHBBH", (version << 4) | ihl, tos, 20 + nopt + len(body) if tl is None else tl, ident, frag,
                       ttl, proto, 0) + src + dst + options
    cs = ~ones_sum(head) & 0xFFFF
    if spoil:
        cs ^= 0x0100
    return head[:10] + struct.pack("!H", cs) + head[12:] + body


def ip6(src, dst, body, nh=17, hlim=61, version=6, plen=None, tc_flow=0x0B54321):
    return struct.pack("!IHBB", (version << 28) | tc_flow, len(body) if plen is None else plen, nh, hlim) + src + dst + body


def error4(src, dst, quote):
    """RFC 792 destination unreachable, code 3, inside a fresh header: DF, TTL 64, identification 0."""
    msg = struct.pack("!BBHI", 3, 3, 0, 0) + quote
    msg = msg[:2] + struct.pack("!H", ~ones_sum(msg) & 0xFFFF) + msg[4:]
    head = struct.pack("!BBHHHBBH", 0x45, 0, 20 + len(msg), 0, 0x4000, 64, 1, 0) + src + dst
    head = head[:10] + struct.pack("!H", ~ones_sum(head) & 0xFFFF) + head[12:]
    return head + msg


def error6(src, dst, quote):
    """RFC 4443 §3.1 destination unreachable, code 4: hop limit 64, no traffic class, no flow label."""
    msg = struct.pack("!BBHI", 1, 4, 0, 0) + quote
    cs = ~ones_sum(pseudo6(src, dst, len(msg), 58) + msg) & 0xFFFF
    msg = msg[:2] + struct.pack("!H", cs) + msg[4:]
    return struct.pack("!IHBB", 6 << 28, len(msg), 58, 64) + src + dst + msg


# ---- the cases: a case is (frame(tags), reply(tags) or None); reply(tags) -> (the error frame, the entry's port) ----
def udp4_case(entry=OWN4, dst=None, src=PEER4, dport=CLOSED, data=24, pad=0, cut=None, dst_mac=None, udp_zero=False,
              tl_delta=0, **ipf):
    dst = entry[1] if dst is None else dst
    mac = entry[3] if dst_mac is None else dst_mac
    body = udp(src, dst, 40000, dport, payload(data), pseudo4, udp_zero)
    packet = ip4(src, dst, body, tl=(4 * ipf.get("ihl", 5) + len(body) + tl_delta) if tl_delta else None, **ipf)
    hl = 4 * ipf.get("ihl", 5)

    def frame(tags):
        f = eth(mac, PEER_MAC, tags, 0x0800) + packet + b"\xa5" * pad
        return f if cut is None else f[:14 + 4 * len(tags) + cut]

    def reply(tags):
        return eth(PEER_MAC, entry[3], tags, 0x0800) + error4(dst, src, packet[:hl + 8]), entry[2]

    return frame, reply


def udp6_case(entry=OWN6, dst=None, src=PEER6, dport=CLOSED, data=24, pad=0, cut=None, dst_mac=None, udp_zero=False,
              plen_delta=0, **ipf):
    dst = entry[1] if dst is None else dst
    mac = entry[3] if dst_mac is None else dst_mac
    body = udp(src, dst, 40000, dport, payload(data), pseudo6, udp_zero)
    packet = ip6(src, dst, body, plen=len(body) + plen_delta if plen_delta else None, **ipf)

    def frame(tags):
        f = eth(mac, PEER_MAC, tags, 0x86DD) + packet + b"\x5a" * pad
        return f if cut is None else f[:14 + 4 * len(tags) + cut]

    def reply(tags):
        return eth(PEER_MAC, entry[3], tags, 0x86DD) + error6(dst, src, packet[:1232]), entry[2]

    return frame, reply


def other(builder):
    return builder, None


def tcp4(tags):
    return eth(OWN4[3], PEER_MAC, tags, 0x0800) + ip4(PEER4, OWN4[1], bytes(20), proto=6)


def arp(tags):
    return N.arp_case()[0](tags)


MCAST_MAC4, MCAST_MAC6 = bytes.fromhex("01005e000001"), bytes.fromhex("333300000001")
ALL6 = bytes.fromhex("ff020000000000000000000000000001")

# (name, family, (frame, reply), verdict when seen, room: None = plenty, or the reply length plus this many bytes)
CASES = [
    # rule 3
    ("udp4_probe", 4, udp4_case(), UNREACH4, None),                                   # 3g: q = 28; the reply is 4 bytes longer than len
    ("udp4_empty", 4, udp4_case(data=0), UNREACH4, None),                             # tl = 28: the reply is longer than len
    ("udp4_padded", 4, udp4_case(data=0, pad=40), UNREACH4, None),                    # the reply is shorter: the tail stays
    ("udp4_ihl_15", 4, udp4_case(ihl=15, data=5), UNREACH4, None),                    # q = 68: the move overlaps itself
    ("udp4_first_fragment", 4, udp4_case(frag=0x2000), UNREACH4, None),               # MF with offset 0 is a first fragment
    ("udp4_zero_udp_sum", 4, udp4_case(udp_zero=True), UNREACH4, None),               # legal over IPv4
    ("udp4_fits_to_the_byte", 4, udp4_case(data=3), UNREACH4, 0),                     # 3f's bound itself
    ("udp4_cut_header", 4, udp4_case(cut=19), NONE, None),                            # 3a
    ("udp4_version", 4, udp4_case(version=5), NONE, None),
    ("udp4_ihl_4", 4, udp4_case(ihl=4, real_options=0), NONE, None),
    ("udp4_cut_options", 4, udp4_case(ihl=8, cut=31), NONE, None),
    ("tcp4", 0, other(tcp4), NONE, None),
    ("udp4_tl_short", 4, udp4_case(tl_delta=-25), MALFORMED, None),                   # 3b: tl = 4 ihl + 7
    ("udp4_tl_overrun", 4, udp4_case(tl_delta=1), MALFORMED, None),
    ("udp4_cut_in_udp", 4, udp4_case(cut=27), MALFORMED, None),
    ("udp4_bad_header_sum", 4, udp4_case(spoil=True), MALFORMED, None),
    ("udp4_later_fragment", 4, udp4_case(frag=0x0010), LEFT, None),                   # 3c
    ("udp4_link_broadcast", 4, udp4_case(dst_mac=N.BCAST), LEFT, None),
    ("udp4_multicast", 4, udp4_case(dst=bytes([224, 0, 0, 1]), dst_mac=MCAST_MAC4), LEFT, None),
    ("udp4_multicast_unicast_mac", 4, udp4_case(dst=bytes([239, 1, 2, 3])), LEFT, None),
    ("udp4_limited_broadcast", 4, udp4_case(dst=bytes([255] * 4)), LEFT, None),
    ("udp4_source_zero", 4, udp4_case(src=bytes(4)), LEFT, None),
    ("udp4_source_multicast", 4, udp4_case(src=bytes([224, 0, 0, 9])), LEFT, None),
    ("udp4_source_loopback", 4, udp4_case(src=bytes([127, 0, 0, 1])), LEFT, None),
    ("udp4_stranger", 4, udp4_case(dst=STRANGER4), UNKNOWN, None),                    # 3d
    ("udp4_port_high", 4, udp4_case(entry=OWN4_HIGH), UNBOUND, None),
    ("udp4_port_unbound", 4, udp4_case(entry=OWN4_OFF), UNBOUND, None),
    ("udp4_open_port", 4, udp4_case(dport=53), LEFT, None),                           # 3e
    ("udp4_open_port_65535", 4, udp4_case(dport=65535, ihl=7), LEFT, None),
    ("udp4_one_byte_short", 4, udp4_case(data=3), NO_ROOM, -1),                       # 3f
    # rule 4
    ("udp6_probe", 6, udp6_case(), UNREACH6, None),                                   # 4f
    ("udp6_empty", 6, udp6_case(data=0), UNREACH6, None),                             # pl = 8, q = 48
    ("udp6_padded", 6, udp6_case(data=0, pad=70), UNREACH6, None),                    # the reply is shorter than len
    ("udp6_link_local", 6, udp6_case(entry=OWN6_LL, data=33), UNREACH6, None),        # an odd quote
    ("udp6_pl_1191", 6, udp6_case(data=1183), UNREACH6, None),                        # q = 1231
    ("udp6_pl_1192", 6, udp6_case(data=1184), UNREACH6, None),                        # q = 1232: the cap itself
    ("udp6_pl_1193", 6, udp6_case(data=1185), UNREACH6, None),                        # q = 1232: one byte not quoted
    ("udp6_fits_to_the_byte", 6, udp6_case(data=9), UNREACH6, 0),
    ("udp6_cut_header", 6, udp6_case(cut=39), NONE, None),                            # 4a
    ("udp6_version", 6, udp6_case(version=4), NONE, None),
    ("tcp6", 6, udp6_case(nh=6), NONE, None),
    ("udp6_hop_by_hop", 6, udp6_case(nh=0), NONE, None),
    ("udp6_pl_7", 6, udp6_case(data=0, plen_delta=-1), MALFORMED, None),              # 4b
    ("udp6_pl_overrun", 6, udp6_case(plen_delta=1), MALFORMED, None),
    ("udp6_cut_in_udp", 6, udp6_case(cut=47), MALFORMED, None),
    ("udp6_zero_udp_sum", 6, udp6_case(udp_zero=True), MALFORMED, None),
    ("udp6_link_multicast", 6, udp6_case(dst_mac=MCAST_MAC6), LEFT, None),            # 4c
    ("udp6_multicast", 6, udp6_case(dst=ALL6), LEFT, None),
    ("udp6_source_unspecified", 6, udp6_case(src=bytes(16)), LEFT, None),
    ("udp6_source_multicast", 6, udp6_case(src=ALL6), LEFT, None),
    ("udp6_stranger", 6, udp6_case(dst=STRANGER6), UNKNOWN, None),                    # 4d
    ("udp6_port_unbound", 6, udp6_case(entry=OWN6_OFF), UNBOUND, None),
    ("udp6_open_port", 6, udp6_case(dport=4789), LEFT, None),
    ("udp6_one_byte_short", 6, udp6_case(data=9), NO_ROOM, -1),                       # 4e
    # rules 2 and 5
    ("tag_cut", 0, other(N.tag_cut), NONE, None),
    ("arp_request", 0, other(arp), NONE, None),
    ("empty", 0, other(lambda tags: b""), NONE, None),
]


def room_of(reply, room, tags):
    """The bytes the chunk leaves the frame: None for plenty, otherwise the error's length plus `room`."""
    return None if room is None else len(reply(tags)[0]) + room


def expect(family, seen_verdict, reply, tags, opts, frame, room):
    """What the responder makes of a case under one option word: it sees the packet behind no tag, or behind up to two
    with XSK_GPU_OPT_VLAN; an IPv6 packet only with XSK_GPU_OPT_IPV6; anything it does not see is NONE.  An error that
    does not fit `room` bytes is NO_ROOM."""
    sees = not tags or (opts & OPT_VLAN and len(tags) <= 2)
    if not sees or family == 0 or (family == 6 and not opts & OPT_IPV6):
        return dict(verdict=NONE, port=0xFF)
    if seen_verdict not in (UNREACH4, UNREACH6, NO_ROOM):
        return dict(verdict=seen_verdict, port=0xFF)
    out, port = reply(tags)
    if room is not None and len(out) > room:
        return dict(verdict=NO_ROOM, port=0xFF)
    assert seen_verdict != NO_ROOM
    return dict(verdict=seen_verdict, port=port, reply=(out + frame[len(out):]).hex(), reply_len=len(out))


def main():
    cases = []
    for name, family, (frame, reply), verdict, room in CASES:
        for k, tags in enumerate(TAGS):
            f = frame(tags)
            r = room_of(reply, room, tags)
            exp = {}
            for opts in OPTS:
                exp["0x%x" % opts] = expect(family, verdict, reply, tags, opts, f, r)
            cases.append(dict(name=name, tags=k, frame=f.hex(), room=r, expect=exp))
    doc = dict(n_ports=N_PORTS, bound="0x%016x" % BOUND, opts=list(OPTS), open_ports=list(OPEN_PORTS),
               table=[dict(family=e[0], addr=e[1].hex(), port=e[2], mac=e[3].hex()) for e in TABLE], cases=cases)
    with open(os.path.join(_HERE, "unreach.json"), "w") as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(len(cases), "cases")


if __name__ == "__main__":
    main()
