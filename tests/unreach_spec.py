"""The spec of xsk_gpu_unreach_dev and xsk_gpu_unreach_serve_dev (include/xsk_gpu.h, "Port-unreachable responder") in
plain Python / numpy, written sequentially: the per-frame rule on one frame's bytes, the loop over a descriptor list, and
the serve loop over the `up` ring, one entry at a time, with the budget.

    table: {(family, addr as 16 bytes): (port, mac as 6 bytes)}        bound: the 64-bit word, ALL_BOUND for NULL
    open_ports: a set of UDP ports somebody listens on (or None)        room: the bytes the frame may grow to
    decide(frame, opts, table, n_ports, bound, open_ports, room) -> (verdict, port, reply or None, reply length)
"""
import numpy as np

import oracle
from tests import neigh_spec as NS
from tests import rx_dev_spec as RS

NONE, UNREACH4, UNREACH6, MALFORMED, UNKNOWN, UNBOUND, LEFT, NO_ROOM, LIMITED = range(9)
OPT_VLAN, OPT_IPV6, OPT_MASK = 0x2, 0x10, 0x17
MAX_LEN = 1 << 30
ALL_BOUND = (1 << 64) - 1
NO_PORT = 0xFF
MAX_QUOTE6 = 1232
STATS_KEYS = ("seen", "unreach4", "unreach6", "reply_bytes", "limited")
RESULT_KEYS = ("consumed", "unreach4", "unreach6", "rest", "backlog", "limited")
REPLIES = (UNREACH4, UNREACH6)

csum16 = NS.csum16


def pseudo(src: bytes, dst: bytes, length: int) -> bytes:
    """RFC 8200 §8.1 for next header 58."""
    return bytes(src) + bytes(dst) + length.to_bytes(4, "big") + b"\0\0\0" + bytes([58])


def open_map(open_ports) -> np.ndarray:
    """The 8192-byte map of d_open: bit p & 7 of byte p >> 3."""
    m = np.zeros(8192, np.uint8)
    for p in open_ports:
        m[p >> 3] |= 1 << (p & 7)
    return m


def _resolve(entry, n_ports, bound):
    if entry is None:
        return UNKNOWN, None
    port, mac = entry
    if port >= n_ports or not (bound >> (port & 63)) & 1:
        return UNBOUND, None
    return None, (port, bytes(mac))


def decide(frame: bytes, opts: int, table: dict, n_ports: int, bound: int = ALL_BOUND, open_ports=None, room: int = 1 << 62):
    """Rules 2-5 on the bytes of one frame whose descriptor passed rule 1 (len == len(frame)); `room` is the largest reply
    length rule 3f / 4e admits at the frame's address."""
    f = bytes(frame)
    n = len(f)
    be = lambda i: (f[i] << 8) | f[i + 1]  # noqa: E731
    out = lambda v: (v, NO_PORT, None, 0)  # noqa: E731
    if n < 14:
        return out(NONE)
    l3, et = 14, be(12)
    if opts & OPT_VLAN:
        for _ in range(2):
            if et not in (0x8100, 0x88A8):
                break
            if n < l3 + 4:
                return out(NONE)
            et = be(l3 + 2)
            l3 += 4
    if et == 0x0800:
        if n < l3 + 20 or f[l3] >> 4 != 4:
            return out(NONE)
        ihl = f[l3] & 15
        if ihl < 5 or n < l3 + 4 * ihl or f[l3 + 9] != 17:
            return out(NONE)
        tl = be(l3 + 2)
        if tl < 4 * ihl + 8 or l3 + tl > n or csum16(f[l3:l3 + 4 * ihl]) != 0xFFFF:
            return out(MALFORMED)
        S, D = f[l3 + 12:l3 + 16], f[l3 + 16:l3 + 20]
        if be(l3 + 6) & 0x1FFF or f[0] & 1 or D[0] >= 224 or S == bytes(4) or S[0] >= 224 or S[0] == 127:
            return out(LEFT)
        bad, ok = _resolve(table.get(NS.key4(D)), n_ports, bound)
        if bad is not None:
            return out(bad)
        if open_ports is not None and be(l3 + 4 * ihl + 2) in open_ports:
            return out(LEFT)
        q = 4 * ihl + 8
        R = l3 + 28 + q
        if R > room:
            return out(NO_ROOM)
        port, m = ok
        quote = f[l3:l3 + q]
        icmp = bytearray(b"\x03\x03\0\0\0\0\0\0" + quote)
        icmp[2:4] = (~csum16(bytes(icmp)) & 0xFFFF).to_bytes(2, "big")
        ip = bytearray(b"\x45\x00" + (28 + q).to_bytes(2, "big") + b"\0\0\x40\x00\x40\x01\0\0" + D + S)
        ip[10:12] = (~csum16(bytes(ip)) & 0xFFFF).to_bytes(2, "big")
        return UNREACH4, port, f[6:12] + m + f[12:l3] + bytes(ip) + bytes(icmp), R
    if et != 0x86DD or not opts & OPT_IPV6:
        return out(NONE)
    if n < l3 + 40 or f[l3] >> 4 != 6 or f[l3 + 6] != 17:
        return out(NONE)
    pl = be(l3 + 4)
    if pl < 8 or l3 + 40 + pl > n or be(l3 + 46) == 0:
        return out(MALFORMED)
    S, D = f[l3 + 8:l3 + 24], f[l3 + 24:l3 + 40]
    if f[0] & 1 or D[0] == 0xFF or S == bytes(16) or S[0] == 0xFF:
        return out(LEFT)
    bad, ok = _resolve(table.get(NS.key6(D)), n_ports, bound)
    if bad is not None:
        return out(bad)
    if open_ports is not None and be(l3 + 42) in open_ports:
        return out(LEFT)
    q = min(40 + pl, MAX_QUOTE6)
    R = l3 + 48 + q
    if R > room:
        return out(NO_ROOM)
    port, m = ok
    quote = f[l3:l3 + q]
    icmp = bytearray(b"\x01\x04\0\0\0\0\0\0" + quote)
    icmp[2:4] = (~csum16(pseudo(D, S, 8 + q) + bytes(icmp)) & 0xFFFF).to_bytes(2, "big")
    ip = b"\x60\0\0\0" + (8 + q).to_bytes(2, "big") + b"\x3a\x40" + D + S
    return UNREACH6, port, f[6:12] + m + f[12:l3] + ip + bytes(icmp), R


def room_at(addr: int, umem_size: int, chunk_size: int) -> int:
    """The largest R rule 3f / 4e admits for a frame at `addr`."""
    return min(chunk_size - (addr & (chunk_size - 1)), umem_size - addr)


def decide_desc(umem: np.ndarray, desc, opts: int, table: dict, n_ports: int, bound: int = ALL_BOUND, open_ports=None,
                chunk_size: int = 2048):
    """Rule 1, then decide() on the frame's bytes.  Returns (verdict, port, reply bytes or None, reply length)."""
    addr, length = int(desc["addr"]), int(desc["len"])
    if length > MAX_LEN or addr > len(umem) or length > len(umem) - addr:
        return NONE, NO_PORT, None, 0
    return decide(umem[addr:addr + length].tobytes(), opts, table, n_ports, bound, open_ports,
                  room_at(addr, len(umem), chunk_size))


def _count(stats, v, rlen):
    if stats is not None:
        stats["seen"] += 1
        stats["unreach4"] += v == UNREACH4
        stats["unreach6"] += v == UNREACH6
        stats["reply_bytes"] += rlen if v in REPLIES else 0
        stats["limited"] += v == LIMITED


def spec_unreach(umem: np.ndarray, descs: np.ndarray, n: int, opts: int, table: dict, n_ports: int, bound: int = ALL_BOUND,
                 open_ports=None, chunk_size: int = 2048, stats: dict = None):
    """xsk_gpu_unreach_dev over descs[:n], one frame after the other; `umem` is rewritten in place.  Returns (verdicts,
    ports, reply_len) as lists; reply_len[i] is None where the call writes nothing."""
    verdicts, ports, rlens = [], [], []
    for i in range(n):
        v, port, reply, rlen = decide_desc(umem, descs[i], opts, table, n_ports, bound, open_ports, chunk_size)
        if reply is not None:
            a = int(descs[i]["addr"])
            umem[a:a + len(reply)] = np.frombuffer(reply, np.uint8)
        verdicts.append(v)
        ports.append(port)
        rlens.append(rlen if reply is not None else None)
        _count(stats, v, rlen)
    return verdicts, ports, rlens


def spec_serve(umem: np.ndarray, up: RS.RingState, txs, rest: RS.RingState, max_entries: int, opts: int, table: dict,
               bound: int = ALL_BOUND, open_ports=None, chunk_size: int = 2048, budget=None, stats: dict = None,
               verdicts_out: list = None):
    """xsk_gpu_unreach_serve_dev: the sequential rule.  Rings and `umem` change in place; returns (result as a dict, the
    budget word afterwards -- None for NULL)."""
    used = up.used()
    m = min(used, max_entries)
    room = [tx.free() for tx in txs] + [rest.free()]  # every ring's free count as the call finds it
    rings = list(txs) + [rest]
    given = [0] * len(rings)
    c = u4 = u6 = limited = 0
    left = budget
    for j in range(m):
        e = up.entries[up.slot(up.cons + j)].copy()
        v, port, reply, rlen = decide_desc(umem, e, opts, table, len(txs), bound, open_ports, chunk_size)
        if reply is not None and left is not None and left == 0:
            v, port, reply, rlen = LIMITED, NO_PORT, None, 0
        dest = port if reply is not None else len(txs)
        if given[dest] >= room[dest]:
            break
        if reply is not None:
            if left is not None:
                left -= 1
            a = int(e["addr"])
            umem[a:a + len(reply)] = np.frombuffer(reply, np.uint8)
            e["len"], e["options"] = rlen, 0
        r = rings[dest]
        r.entries[r.slot(r.prod + given[dest])] = e
        given[dest] += 1
        c += 1
        u4 += v == UNREACH4
        u6 += v == UNREACH6
        limited += v == LIMITED
        _count(stats, v, rlen)
        if verdicts_out is not None:
            verdicts_out.append(v)
    for r, g in zip(rings, given):
        r.prod = (r.prod + g) & RS.M32
    up.cons = (up.cons + c) & RS.M32
    return dict(consumed=c, unreach4=u4, unreach6=u6, rest=given[-1], backlog=used - c, limited=limited), left


assert oracle.DESC_DTYPE.itemsize == 16
