"""The spec of xsk_gpu_neigh_dev and xsk_gpu_neigh_serve_dev (include/xsk_gpu.h, "Neighbour responder") in plain
Python / numpy, written sequentially: the per-frame rule on one frame's bytes, the loop over a descriptor list, and the
serve loop over the stack ring, one entry at a time.

    table: {(family, addr as 16 bytes): (port, mac as 6 bytes)}        bound: the 64-bit word, ALL_BOUND for NULL
    decide(frame, opts, table, n_ports, bound) -> (verdict, port, reply or None, reply length)   -- changes nothing
"""
import numpy as np

import oracle
from tests import rx_dev_spec as RS

NONE, ARP_REPLY, NA_REPLY, MALFORMED, UNKNOWN, UNBOUND, LEFT = range(7)
OPT_VLAN, OPT_IPV6, OPT_MASK = 0x2, 0x10, 0x17
MAX_LEN = 1 << 30
ALL_BOUND = (1 << 64) - 1
NO_PORT = 0xFF
STATS_KEYS = ("seen", "arp_replies", "na_replies", "reply_bytes")
RESULT_KEYS = ("consumed", "arp_replies", "na_replies", "up", "backlog")


def key4(a: bytes) -> tuple:
    return 4, bytes(a) + bytes(12)


def key6(a: bytes) -> tuple:
    return 6, bytes(a)


def csum16(data: bytes) -> int:
    """RFC 1071: the folded one's complement sum of the big-endian 16-bit words (an odd last byte is a high byte)."""
    if len(data) & 1:
        data = data + b"\0"
    s = 0
    for i in range(0, len(data), 2):
        s += (data[i] << 8) | data[i + 1]
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def pseudo(src: bytes, dst: bytes, length: int) -> bytes:
    """RFC 8200 §8.1 for next header 58."""
    return bytes(src) + bytes(dst) + length.to_bytes(4, "big") + b"\0\0\0" + bytes([58])


def _port_rule(entry, n_ports, bound):
    port, mac = entry
    if port >= n_ports or not (bound >> (port & 63)) & 1:
        return None
    return port, bytes(mac)


def decide(frame: bytes, opts: int, table: dict, n_ports: int, bound: int = ALL_BOUND):
    """Rules 2-5 on the bytes of one frame whose descriptor passed rule 1 (len == len(frame))."""
    f = bytes(frame)
    n = len(f)
    be = lambda i: (f[i] << 8) | f[i + 1]  # noqa: E731
    none = (NONE, NO_PORT, None, 0)
    bad = (MALFORMED, NO_PORT, None, 0)
    if n < 14:
        return none
    l3, et = 14, be(12)
    if opts & OPT_VLAN:
        for _ in range(2):
            if et not in (0x8100, 0x88A8):
                break
            if n < l3 + 4:
                return none
            et = be(l3 + 2)
            l3 += 4
    if et == 0x0806:
        if n < l3 + 28:
            return bad
        if be(l3) != 1 or be(l3 + 2) != 0x0800 or f[l3 + 4] != 6 or f[l3 + 5] != 4:
            return bad
        if be(l3 + 6) != 1:
            return none
        sha, spa, tpa = f[l3 + 8:l3 + 14], f[l3 + 14:l3 + 18], f[l3 + 24:l3 + 28]
        entry = table.get(key4(tpa))
        if entry is None:
            return UNKNOWN, NO_PORT, None, 0
        ok = _port_rule(entry, n_ports, bound)
        if ok is None:
            return UNBOUND, NO_PORT, None, 0
        port, m = ok
        out = bytearray(f)
        out[0:6] = sha
        out[6:12] = m
        out[l3 + 6:l3 + 8] = b"\0\2"
        out[l3 + 8:l3 + 14] = m
        out[l3 + 14:l3 + 18] = tpa
        out[l3 + 18:l3 + 24] = sha
        out[l3 + 24:l3 + 28] = spa
        return ARP_REPLY, port, bytes(out), n
    if et != 0x86DD or not opts & OPT_IPV6:
        return none
    if n < l3 + 40 or f[l3] >> 4 != 6 or f[l3 + 6] != 58:
        return none
    if n < l3 + 48:
        return bad
    if f[l3 + 40] != 135:
        return none
    pl = be(l3 + 4)
    if f[l3 + 7] != 255 or f[l3 + 41] != 0 or pl < 24 or l3 + 40 + pl > n:
        return bad
    T = f[l3 + 48:l3 + 64]
    if T[0] == 0xFF or (pl - 24) % 8:
        return bad
    if pl > 280:
        return LEFT, NO_PORT, None, 0
    msg = f[l3 + 40:l3 + 40 + pl]
    o = 24
    while o < pl:
        L = msg[o + 1]
        if L == 0 or o + 8 * L > pl:
            return bad
        o += 8 * L
    S, D = f[l3 + 8:l3 + 24], f[l3 + 24:l3 + 40]
    if csum16(pseudo(S, D, pl) + msg) != 0xFFFF:
        return bad
    if S == bytes(16) or pl < 32:
        return LEFT, NO_PORT, None, 0
    entry = table.get(key6(T))
    if entry is None:
        return UNKNOWN, NO_PORT, None, 0
    ok = _port_rule(entry, n_ports, bound)
    if ok is None:
        return UNBOUND, NO_PORT, None, 0
    port, m = ok
    out = bytearray(f)
    out[0:6] = f[6:12]
    out[6:12] = m
    na = bytearray(b"\x88\0\0\0\x60\0\0\0" + T + b"\x02\x01" + m)
    cs = ~csum16(pseudo(T, S, 32) + bytes(na)) & 0xFFFF
    na[2:4] = cs.to_bytes(2, "big")
    out[l3:l3 + 72] = b"\x60\0\0\0" + b"\0\x20" + bytes([58, 255]) + T + S + bytes(na)
    return NA_REPLY, port, bytes(out), l3 + 72


def decide_desc(umem: np.ndarray, desc, opts: int, table: dict, n_ports: int, bound: int = ALL_BOUND):
    """Rule 1, then decide() on the frame's bytes.  Returns (verdict, port, reply bytes or None, reply length)."""
    addr, length = int(desc["addr"]), int(desc["len"])
    if length > MAX_LEN or addr > len(umem) or length > len(umem) - addr:
        return NONE, NO_PORT, None, 0
    return decide(umem[addr:addr + length].tobytes(), opts, table, n_ports, bound)


def _count(stats, v, rlen):
    if stats is not None:
        stats["seen"] += 1
        stats["arp_replies"] += v == ARP_REPLY
        stats["na_replies"] += v == NA_REPLY
        stats["reply_bytes"] += rlen if v in (ARP_REPLY, NA_REPLY) else 0


def spec_neigh(umem: np.ndarray, descs: np.ndarray, n: int, opts: int, table: dict, n_ports: int,
               bound: int = ALL_BOUND, stats: dict = None):
    """xsk_gpu_neigh_dev over descs[:n], one frame after the other; `umem` is rewritten in place.  Returns (verdicts,
    ports, reply_len) as lists; reply_len[i] is None where the call writes nothing."""
    verdicts, ports, rlens = [], [], []
    for i in range(n):
        v, port, reply, rlen = decide_desc(umem, descs[i], opts, table, n_ports, bound)
        if reply is not None:
            a = int(descs[i]["addr"])
            umem[a:a + len(reply)] = np.frombuffer(reply, np.uint8)
        verdicts.append(v)
        ports.append(port)
        rlens.append(rlen if reply is not None else None)
        _count(stats, v, rlen)
    return verdicts, ports, rlens


def spec_serve(umem: np.ndarray, stack: RS.RingState, txs, up: RS.RingState, max_entries: int, opts: int, table: dict,
               bound: int = ALL_BOUND, stats: dict = None, verdicts_out: list = None):
    """xsk_gpu_neigh_serve_dev: the sequential rule.  Rings and `umem` change in place; returns the result as a dict."""
    used = stack.used()
    m = min(used, max_entries)
    room = [tx.free() for tx in txs] + [up.free()]  # every ring's free count as the call finds it
    rings = list(txs) + [up]
    given = [0] * len(rings)
    c = arp = na = 0
    for j in range(m):
        e = stack.entries[stack.slot(stack.cons + j)].copy()
        v, port, reply, rlen = decide_desc(umem, e, opts, table, len(txs), bound)
        dest = port if reply is not None else len(txs)
        if given[dest] >= room[dest]:
            break
        if reply is not None:
            a = int(e["addr"])
            umem[a:a + len(reply)] = np.frombuffer(reply, np.uint8)
            e["len"], e["options"] = rlen, 0
        r = rings[dest]
        r.entries[r.slot(r.prod + given[dest])] = e
        given[dest] += 1
        c += 1
        arp += v == ARP_REPLY
        na += v == NA_REPLY
        _count(stats, v, rlen)
        if verdicts_out is not None:
            verdicts_out.append(v)
    for r, g in zip(rings, given):
        r.prod = (r.prod + g) & RS.M32
    stack.cons = (stack.cons + c) & RS.M32
    return dict(consumed=c, arp_replies=arp, na_replies=na, up=given[-1], backlog=used - c)


def table_array(X, table: dict) -> np.ndarray:
    """The table as a neigh_table_prepare()d array of X.NEIGH_ENTRY_DTYPE."""
    arr = np.zeros(len(table), X.NEIGH_ENTRY_DTYPE)
    for k, ((family, addr), (port, mac)) in enumerate(table.items()):
        arr[k]["addr"] = np.frombuffer(addr, np.uint8)
        arr[k]["family"], arr[k]["port"] = family, port
        arr[k]["mac"] = np.frombuffer(bytes(mac), np.uint8)
    return X.neigh_table_prepare(arr) if len(arr) else arr


assert oracle.DESC_DTYPE.itemsize == 16
