#!/usr/bin/env python3
"""Golden vectors for the ICMPv6 echo widening of wire mode (XSK_GPU_OPT_IPV6, include/xsk_gpu.h).

The reference answers IPv4 only and the C oracle does not know the option bit, so these vectors are the spec of
include/xsk_gpu.h restated in plain Python (RFC 8200 header and §8.1 pseudo-header, RFC 4443 echo, RFC 1071 sums,
IEEE 802.1Q / 802.1ad tags).  Frames whose inner ethertype is not 0x86DD are delegated to make_wire_golden.expect().

    python tests/golden/make_v6_golden.py   ->  tests/golden/v6.json
"""
import importlib.util
import json
import os
import struct

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_wire_golden", os.path.join(_HERE, "make_wire_golden.py"))
W = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(W)

OPT_STRICT, OPT_VLAN, OPT_VERIFY, OPT_IPV6, OPT_MASK = 1, 2, 4, 0x10, 0x17
TX_REPLY, DROP_SHORT, DROP_NOT_IPV4, DROP_NOT_ICMP, DROP_NOT_ECHO, DROP_BAD_DESC, DROP_BAD_IP, DROP_BAD_CSUM = range(8)
F_ICMP_OK, F_VLAN, F_IPV6 = 2, 4, 0x10
csum16 = W.csum16

SRC = bytes.fromhex("20010db8000000000000000000000001")
DST = bytes.fromhex("20010db80000000000000000000000fe")


def pseudo(src: bytes, dst: bytes, mlen: int) -> bytes:
    """RFC 8200 §8.1: source, destination, upper-layer length (32 bits), three zero bytes, next header 58."""
    return src + dst + struct.pack("!I", mlen) + b"\0\0\0" + bytes([58])


def build6(vlan=(), ethertype=0x86DD, version=6, tc=0, flow=0x12345, plen=None, nh=58, hlim=64, itype=128, code=0,
           ident=0x1234, seq=7, payload=b"", pad=0, bad_icmp=False, src_mac=b"\x02\x00\x00\x00\x00\x01",
           dst_mac=b"\x02\x00\x00\x00\x00\x02", saddr=SRC, daddr=DST):
    """An Ethernet frame carrying an IPv6 ICMPv6 message; every field controllable."""
    icmp = bytearray(struct.pack("!BBHHH", itype, code, 0, ident, seq) + payload)
    c = (~csum16(pseudo(saddr, daddr, len(icmp)) + bytes(icmp))) & 0xFFFF
    if bad_icmp:
        c ^= 0x0F0F
    icmp[2:4] = struct.pack("!H", c)
    pl = len(icmp) if plen is None else plen
    ip = struct.pack("!IHBB", ((version & 15) << 28) | ((tc & 0xFF) << 20) | (flow & 0xFFFFF), pl & 0xFFFF, nh, hlim)
    eth = dst_mac + src_mac
    for tpid, tci in vlan:
        eth += struct.pack("!HH", tpid, tci)
    eth += struct.pack("!H", ethertype)
    return bytes(eth + ip + saddr + daddr + icmp + b"\0" * pad)


def replace2_le(field_le: int, old: int, new: int) -> int:
    """The reference's csum_replace2 (src/lib/xsk_receive.c:101-111) in its uint16_t arithmetic."""
    c = (~field_le) & 0xFFFF
    nold = (~old) & 0xFFFF
    c = (c + nold) & 0xFFFF
    c = (c + (1 if c < nold else 0)) & 0xFFFF
    c = (c + new) & 0xFFFF
    c = (c + (1 if c < new else 0)) & 0xFFFF
    return (~c) & 0xFFFF


def v6_l3(frame: bytes, length: int, opts: int):
    """(l3, tags) when the frame's inner ethertype -- after up to two tags with OPT_VLAN, none cut by the frame end --
    is 0x86DD, else None.  Everything up to the inner ethertype is wire mode's."""
    be = lambda i: (frame[i] << 8) | frame[i + 1]  # noqa: E731
    if length < 14:
        return None
    l3, et, tags = 14, be(12), 0
    if opts & OPT_VLAN:
        while tags < 2 and et in (0x8100, 0x88A8):
            if length < l3 + 4:
                return None
            et = be(l3 + 2)
            l3 += 4
            tags += 1
    return (l3, tags) if et == 0x86DD else None


def expect(frame: bytes, length: int, opts: int):
    """The spec of include/xsk_gpu.h for opts with XSK_GPU_OPT_IPV6: (verdict, record dict, output bytes)."""
    assert opts & OPT_IPV6 and not opts & ~OPT_MASK
    six = v6_l3(frame, length, opts)
    if six is None:
        return W.expect(frame, length, opts & 7)
    l3, tags = six
    p = bytearray(frame)
    be = lambda i: (p[i] << 8) | p[i + 1]  # noqa: E731
    rec = dict(verdict=0, flags=0, ip_proto=0, icmp_type=0, icmp_code=0, ip_vihl=0, eth_proto=0, icmp_csum_in=0,
               icmp_csum_out=0, ip_sum=0, icmp_sum=0)

    def done(v):
        rec["verdict"] = v
        return v, rec, bytes(p)

    l4 = l3 + 40
    if length < l4:
        return done(DROP_SHORT)
    end = length
    if opts & OPT_STRICT:
        plen = be(l3 + 4)
        if p[l3] >> 4 != 6 or plen < 8 or l4 + plen > length or p[l3 + 8] == 0xFF or p[l3 + 24] == 0xFF:
            return done(DROP_BAD_IP)
        end = l4 + plen
    if p[l3 + 6] != 58:
        return done(DROP_NOT_ICMP)
    if length < l4 + 8:
        return done(DROP_SHORT)
    src, dst = bytes(p[l3 + 8:l3 + 24]), bytes(p[l3 + 24:l3 + 40])
    ph = pseudo(src, dst, end - l4)
    ip_sum = csum16(ph)
    ic_sum = csum16(ph + bytes(p[l4:end]))  # (csum16 zero-pads an odd tail)
    fl = F_IPV6 | (F_ICMP_OK if ic_sum == 0xFFFF else 0) | (F_VLAN if tags else 0)
    rec.update(flags=fl, eth_proto=0x86DD, ip_vihl=p[l3], ip_proto=58, icmp_type=p[l4], icmp_code=p[l4 + 1],
               icmp_csum_in=be(l4 + 2), ip_sum=ip_sum, icmp_sum=ic_sum)
    if p[l4] != 128 or ((opts & OPT_STRICT) and p[l4 + 1] != 0):
        v = DROP_NOT_ECHO
    elif (opts & OPT_VERIFY) and ic_sum != 0xFFFF:
        v = DROP_BAD_CSUM
    else:
        v = TX_REPLY
        p[0:6], p[6:12] = frame[6:12], frame[0:6]
        p[l3 + 8:l3 + 24], p[l3 + 24:l3 + 40] = dst, src
        p[l4] = 129
        new_le = replace2_le(p[l4 + 2] | (p[l4 + 3] << 8), 128, 129)
        p[l4 + 2], p[l4 + 3] = new_le & 0xFF, new_le >> 8
    rec["icmp_csum_out"] = be(l4 + 2)
    return done(v)


def cases():
    big = bytes((i * 37 + 11) & 0xFF for i in range(1400))
    q1, q2 = [(0x8100, 0x0064)], [(0x88A8, 0x0005), (0x8100, 0x0064)]
    mc = bytes.fromhex("ff020000000000000000000000000001")
    c = {}
    c["echo_62"] = build6()
    c["payload_1"] = build6(payload=b"\xa5")
    c["payload_2"] = build6(payload=b"\xa5\x5a")
    c["payload_1400"] = build6(payload=big)
    c["vlan1"] = build6(vlan=q1, payload=b"tagged")
    c["vlan2_qinq"] = build6(vlan=q2, payload=big[:77])
    c["vlan3_too_many"] = build6(vlan=q2 + [(0x8100, 3)])
    c["bad_csum"] = build6(payload=b"ping6", bad_icmp=True)
    c["nh_udp"] = build6(nh=17)
    c["nh_hop_by_hop"] = build6(nh=0, payload=b"\x3a\x00\x01\x04\x00\x00\x00\x00")
    c["type_129"] = build6(itype=129)
    c["type_135"] = build6(itype=135, payload=b"\0" * 20)
    c["code_1"] = build6(code=1)
    c["version_4"] = build6(version=4)
    c["plen_0"] = build6(plen=0)
    c["plen_short"] = build6(plen=7, payload=b"abcd")
    c["plen_long"] = build6(plen=200, payload=b"abcd")
    c["eth_padding"] = build6(payload=b"xyz", pad=9)
    c["mcast_src"] = build6(saddr=mc)
    c["mcast_dst"] = build6(daddr=mc)
    c["csum_wraps"] = build6(ident=0, seq=0, saddr=b"\0" * 16, daddr=b"\0" * 15 + b"\x01", payload=b"\0" * 4)
    c["ipv4_plain"] = W.build()  # the IPv4 path under the same option sets
    lens = {name: [len(f)] for name, f in c.items()}
    # truncations at every boundary: l3 + 39, l3 + 40, l4 + 7, l4 + 8 (and the tag cuts)
    lens["echo_62"] += [13, 14, 53, 54, 61]
    lens["payload_2"] += [53, 54, 61, 62, 63]
    lens["vlan1"] += [17, 18, 57, 58, 65, 66]
    lens["vlan2_qinq"] += [21, 22, 61, 62, 69, 70]
    return c, lens


def main():
    c, lens = cases()
    out = []
    for name, f in c.items():
        for L in lens[name]:
            frame = f + b"\0" * max(0, 128 - len(f))  # window bytes past the frame: zeros
            res = {}
            for opts in range(0x10, 0x18):
                v, rec, o = expect(frame, L, opts)
                res[str(opts)] = {"verdict": v, "rec": rec, "out": o[:max(L, 1)].hex()}
            out.append({"name": name, "len": L, "frame": frame.hex(), "results": res})
    path = os.path.join(_HERE, "v6.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0)
    print(f"{len(out)} frames x 8 option sets -> {path}")


if __name__ == "__main__":
    main()
