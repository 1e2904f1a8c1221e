#!/usr/bin/env python3
"""Golden vectors for the ingress filter with wire-format options (xsk_gpu_classify_dev_opts, include/xsk_gpu.h).

The reference's filter (src/kern/inner_xdp.c:26-61) knows neither tags nor IPv6 and the C oracle does not learn
options, so these vectors are the header's spec restated in plain Python, independent of the HIP code.  Frames come
from make_wire_golden.build (IPv4) and make_v6_golden.build6 (IPv6).

    python tests/golden/make_classify_wire_golden.py   ->  tests/golden/classify_wire.json
"""
import importlib.util
import json
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_v6_golden", os.path.join(_HERE, "make_v6_golden.py"))
G6 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G6)
W = G6.W

OPT_STRICT, OPT_VLAN, OPT_VERIFY, OPT_IPV6, OPT_MASK = 1, 2, 4, 0x10, 0x17
XDP_DROP, XDP_PASS, XDP_REDIRECT = 1, 2, 4
OPTION_WORDS = (0x2, 0x10, 0x12, 0x17, 0x5)


def classify(frame: bytes, length: int, opts: int, bound: bool = True) -> int:
    """Rules 2-6 of the header's spec for nonzero opts (rule 1, the descriptor, belongs to the batch).  Reads no byte
    at or past `length`."""
    assert opts and not opts & ~OPT_MASK
    be = lambda i: (frame[i] << 8) | frame[i + 1]  # noqa: E731
    redirect = XDP_REDIRECT if bound else XDP_DROP
    if length < 14:
        return XDP_DROP
    l3, et, tags = 14, be(12), 0
    if opts & OPT_VLAN:
        while tags < 2 and et in (0x8100, 0x88A8):
            if length < l3 + 4:
                return XDP_DROP
            et = be(l3 + 2)
            l3 += 4
            tags += 1
    if et == 0x0800:
        if length < l3 + 20:
            return XDP_DROP
        return redirect if frame[l3 + 9] == 1 else XDP_PASS
    if et == 0x86DD and opts & OPT_IPV6:
        if length < l3 + 40:
            return XDP_DROP
        if frame[l3 + 6] != 58:
            return XDP_PASS
        if length < l3 + 48:
            return XDP_DROP
        return redirect if frame[l3 + 40] == 128 else XDP_PASS
    return XDP_PASS


def cases():
    """[(name, frame, len)]: every boundary of the spec at 0, 1 and 2 tags."""
    stacks = {0: [], 1: [(0x8100, 0x0064)], 2: [(0x88A8, 0x0005), (0x8100, 0x0064)]}
    out = []

    def add(name, frame, lens=None):
        for L in lens or [len(frame)]:
            assert L <= len(frame), name
            out.append((f"{name}@{L}", frame, L))

    for t, vlan in stacks.items():
        l3 = 14 + 4 * t
        v4 = W.build(vlan=vlan)
        v6 = G6.build6(vlan=vlan)
        assert len(v6) == l3 + 48
        # lengths 13 / 14, every byte of every tag, l3 + 19 / l3 + 20; the whole frame
        add(f"v4_t{t}", v4, sorted({13, 14, *range(14, l3 + 1), l3 + 19, l3 + 20, len(v4)}))
        # ... l3 + 39 / l3 + 40 and l3 + 47 / l3 + 48 (61 / 62 without a tag: the minimal echo request)
        add(f"v6_t{t}", v6, sorted({13, 14, *range(14, l3 + 1), l3 + 19, l3 + 20, l3 + 39, l3 + 40, l3 + 47, l3 + 48}))
        add(f"v6_t{t}_payload", G6.build6(vlan=vlan, payload=b"ping6 payload"))
        for nh in (0, 6, 17):
            add(f"v6_t{t}_nh{nh}", G6.build6(vlan=vlan, nh=nh), [l3 + 40, l3 + 47, l3 + 48])
        for ty in (129, 133, 135, 136, 1):
            add(f"v6_t{t}_type{ty}", G6.build6(vlan=vlan, itype=ty, payload=b"\0" * 16))
        for pr in (6, 17):
            add(f"v4_t{t}_proto{pr}", W.build(vlan=vlan, proto=pr), [l3 + 19, l3 + 20, l3 + 28])
        add(f"v4_t{t}_ihl6", W.build(vlan=vlan, ihl=6, options=b"\x01\x01\x01\x00"))
        add(f"v4_t{t}_version6", W.build(vlan=vlan, version=6))
        add(f"v4_t{t}_type0", W.build(vlan=vlan, itype=0))  # an echo reply is still ICMP: REDIRECT, as xdp_sock_prog
        add(f"arp_t{t}", W.build(vlan=vlan, ethertype=0x0806))
    # 0x8100 outside 0x88A8 (the stacks above are 0x88A8 outside 0x8100), and two equal TPIDs
    add("v4_q_in_ad", W.build(vlan=[(0x8100, 7), (0x88A8, 8)]))
    add("v6_q_in_ad", G6.build6(vlan=[(0x8100, 7), (0x88A8, 8)]))
    add("v6_ad_ad", G6.build6(vlan=[(0x88A8, 7), (0x88A8, 8)]))
    # a third tag is never skipped
    three = [(0x88A8, 1), (0x8100, 2), (0x8100, 3)]
    add("v4_t3", W.build(vlan=three), [22, 25, 26, 45, 46])
    add("v6_t3", G6.build6(vlan=three), [26, 73, 74])
    # bad checksums and strict-IP errors change no action: the transform sorts them out
    add("v4_bad_ip_csum", W.build(bad_ip=True))
    add("v4_fragment", W.build(frag=0x2000))
    add("v4_tot_len_long", W.build(tot_len=200))
    add("v6_bad_csum", G6.build6(bad_icmp=True))
    add("v6_version4", G6.build6(version=4))
    add("v6_plen0", G6.build6(plen=0))
    add("v6_mcast_dst", G6.build6(daddr=bytes.fromhex("ff020000000000000000000000000001")))
    # neighbour solicitation to the solicited-node multicast address: the frame that must stay with the kernel stack
    add("v6_neighbour_solicitation", G6.build6(itype=135, hlim=255, payload=b"\0" * 4 + G6.DST + b"\x01\x01" + b"\x02" * 6,
                                               daddr=bytes.fromhex("ff0200000000000000000001ff0000fe"),
                                               dst_mac=bytes.fromhex("3333ff0000fe")))
    # ICMP (1) as an IPv6 next header and ICMPv6 (58) as an IPv4 protocol belong to nobody's echo
    add("v6_nh1", G6.build6(nh=1))
    add("v4_proto58", W.build(proto=58))
    return out


def vectors():
    out = []
    for name, frame, L in cases():
        res = {str(o): {"bound": classify(frame, L, o, True), "unbound": classify(frame, L, o, False)}
               for o in OPTION_WORDS}
        out.append({"name": name, "len": L, "frame": frame.hex(), "results": res})
    return out


def main():
    out = vectors()
    path = os.path.join(_HERE, "classify_wire.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0)
    print(f"{len(out)} frames x {len(OPTION_WORDS)} option words -> {path}")


if __name__ == "__main__":
    main()
