#!/usr/bin/env python3
"""Golden vectors for the steering filter (xsk_gpu_steer_dev, include/xsk_gpu.h).

The header's spec restated in plain Python, independent of the HIP code.  Whether the filter's rules redirect a frame
is make_classify_wire_golden.classify() for nonzero options and ref_classify() below, the reference's xdp_sock_prog
(src/kern/inner_xdp.c:26-61), for opts == 0; what follows a REDIRECT is written here: where the IP header starts, the
destination address, the lookup (a dict), the port and bound rules.

    python tests/golden/make_steer_golden.py   ->  tests/golden/steer.json

Frames: every crafted frame of classify_wire.json, plus destinations in and out of the tables, broadcast and multicast,
tagged forms, a family-4 key that is the prefix of a family-6 key, and frames whose destination is their last bytes.
Each is crossed with OPTION_WORDS and 0, two tables, default_port in {0, PASS} and two bound masks.
"""
import importlib.util
import json
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_classify_wire_golden",
                                               os.path.join(_HERE, "make_classify_wire_golden.py"))
GC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GC)
G6, W = GC.G6, GC.W

XDP_DROP, XDP_PASS, XDP_REDIRECT = GC.XDP_DROP, GC.XDP_PASS, GC.XDP_REDIRECT
PASS = 0xFF      # XSK_GPU_STEER_PASS
MAX_PORTS = 64   # XSK_GPU_STEER_MAX_PORTS
OPTION_WORDS = (0,) + tuple(GC.OPTION_WORDS)

V4_LOCAL = bytes([10, 0, 0, 2])          # the builders' default destinations
V6_LOCAL = G6.DST
V4_OTHER = bytes([10, 0, 0, 77])
V6_OTHER = bytes.fromhex("20010db8000000000000000000000077")
V4_ABSENT = bytes([192, 0, 2, 9])
V6_ABSENT = bytes.fromhex("20010db800000000000000000000abcd")
V4_BCAST = bytes([255] * 4)
V4_MCAST = bytes([224, 0, 0, 1])
V6_MCAST = bytes.fromhex("ff020000000000000000000000000001")
# a family-4 key whose four bytes open a family-6 key
V4_PREFIX = bytes([0x20, 0x01, 0x0d, 0xb8])
V6_PREFIXED = V4_PREFIX + bytes(11) + b"\x05"


def key(addr: bytes):
    """(family, 16 address bytes): a family-4 address is followed by twelve zeros."""
    assert len(addr) in (4, 16)
    return (4 if len(addr) == 4 else 6, addr + bytes(16 - len(addr)))


# name -> (n_ports, {key: port}).  "unicast": three sockets, local unicast addresses only.  "wide": all 64 ports, ports
# the other table does not use, a multicast group a socket subscribed to, the prefix pair on two different ports.
TABLES = {
    "unicast": (3, {key(V4_LOCAL): 0, key(V6_LOCAL): 1, key(V4_OTHER): 2, key(V6_OTHER): 2}),
    "wide": (64, {key(V4_LOCAL): 63, key(V6_LOCAL): 17, key(V4_OTHER): 1, key(V6_OTHER): 0, key(V6_MCAST): 40,
                  key(V4_PREFIX): 5, key(V6_PREFIXED): 6}),
}
DEFAULT_PORTS = (0, PASS)
BOUND_MASKS = ((1 << 64) - 1, ((1 << 64) - 1) & ~((1 << 1) | (1 << 17) | (1 << 63)))  # all; ports 1, 17, 63 unbound


def ref_classify(frame: bytes, length: int) -> int:
    """xdp_sock_prog with a bound socket (inner_xdp.c:35-60), the rules xsk_gpu_classify_dev() lists."""
    if length < 14:
        return XDP_DROP
    if frame[12] != 0x08 or frame[13] != 0x00:
        return XDP_PASS
    if length < 34:
        return XDP_DROP
    if frame[23] != 1:
        return XDP_PASS
    return XDP_REDIRECT


def ip_header(frame: bytes, opts: int):
    """(l3, family) of a frame the filter's rules redirect: 14 for opts == 0, else behind up to two tags."""
    be = lambda i: (frame[i] << 8) | frame[i + 1]  # noqa: E731
    l3, et, tags = 14, be(12), 0
    if opts & GC.OPT_VLAN:
        while tags < 2 and et in (0x8100, 0x88A8):
            et = be(l3 + 2)
            l3 += 4
            tags += 1
    assert et in (0x0800, 0x86DD)
    return l3, (4 if et == 0x0800 else 6)


def steer(frame: bytes, length: int, opts: int, table: dict, default_port: int, n_ports: int, bound: int):
    """(action, port) of one frame whose descriptor is valid.  Reads no byte at or past `length`."""
    base = GC.classify(frame, length, opts, True) if opts else ref_classify(frame, length)
    if base != XDP_REDIRECT:
        return base, PASS
    l3, fam = ip_header(frame, opts)
    lo, hi = (l3 + 16, l3 + 20) if fam == 4 else (l3 + 24, l3 + 40)
    assert hi <= length
    port = table.get(key(bytes(frame[lo:hi])), default_port)
    if port == PASS:
        return XDP_PASS, PASS
    if port >= n_ports or not (bound >> port) & 1:
        return XDP_DROP, PASS
    return XDP_REDIRECT, port


def cases():
    """[(name, frame, len)]"""
    out = list(GC.cases())

    def add(name, frame, length=None):
        out.append((f"steer_{name}", frame, len(frame) if length is None else length))

    q1, q2 = [(0x8100, 0x0064)], [(0x88A8, 0x0005), (0x8100, 0x0064)]
    add("v4_table", W.build(daddr=V4_OTHER))
    add("v4_absent", W.build(daddr=V4_ABSENT))
    add("v4_broadcast", W.build(daddr=V4_BCAST, dst_mac=b"\xff" * 6))
    add("v4_multicast", W.build(daddr=V4_MCAST, dst_mac=bytes.fromhex("01005e000001")))
    add("v6_table", G6.build6(daddr=V6_OTHER))
    add("v6_absent", G6.build6(daddr=V6_ABSENT))
    add("v6_multicast", G6.build6(daddr=V6_MCAST, dst_mac=bytes.fromhex("333300000001")))
    add("v4_t1_table", W.build(vlan=q1, daddr=V4_OTHER))
    add("v4_t2_table", W.build(vlan=q2, daddr=V4_OTHER))
    add("v6_t1_table", G6.build6(vlan=q1, daddr=V6_OTHER))
    add("v6_t2_table", G6.build6(vlan=q2, daddr=V6_OTHER))
    add("v4_prefix_of_v6_key", W.build(daddr=V4_PREFIX))
    add("v6_prefixed_by_v4_key", G6.build6(daddr=V6_PREFIXED))
    add("v6_first_four_only", G6.build6(daddr=V4_PREFIX + bytes(12)))  # the family-4 key's 16 bytes, as family 6
    # the destination is the last four bytes of the frame: REDIRECT for opts == 0 and every option word
    add("v4_dst_last_bytes", W.build(daddr=V4_OTHER), 34)
    add("v4_t1_dst_last_bytes", W.build(vlan=q1, daddr=V4_OTHER), 38)
    add("v4_t2_dst_last_bytes", W.build(vlan=q2, daddr=V4_OTHER), 42)
    # the destination is the last sixteen bytes of the frame: the spec gives DROP under XSK_GPU_OPT_IPV6 (rule 5, the
    # ICMPv6 header is cut) before any lookup, and PASS without it (rule 6)
    add("v6_dst_last_bytes", G6.build6(daddr=V6_OTHER), 54)
    add("v6_t1_dst_last_bytes", G6.build6(vlan=q1, daddr=V6_OTHER), 58)
    add("v6_t2_dst_last_bytes", G6.build6(vlan=q2, daddr=V6_OTHER), 62)
    return out


def combos():
    """[(label, table name, default_port, bound mask)] in the order of a frame's result lists."""
    return [(f"{t}/d{d}/b{b}", t, d, m) for t in TABLES for d in DEFAULT_PORTS for b, m in enumerate(BOUND_MASKS)]


def vectors():
    out = []
    for name, frame, L in cases():
        res = {}
        for o in OPTION_WORDS:
            row = []
            for _, t, d, m in combos():
                n_ports, table = TABLES[t]
                row.append(list(steer(frame, L, o, table, d, n_ports, m)))
            res[str(o)] = row
        out.append({"name": name, "len": L, "frame": frame.hex(), "results": res})
    return out


def main():
    doc = {
        "combos": [c[0] for c in combos()],
        "tables": {t: {"n_ports": n, "entries": [[k[0], k[1].hex(), p] for k, p in sorted(tab.items())]}
                   for t, (n, tab) in TABLES.items()},
        "default_ports": list(DEFAULT_PORTS),
        "bound_masks": [f"{m:016x}" for m in BOUND_MASKS],
        "frames": vectors(),
    }
    path = os.path.join(_HERE, "steer.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{len(doc['frames'])} frames x {len(OPTION_WORDS)} option words x {len(doc['combos'])} maps -> {path}")


if __name__ == "__main__":
    main()
