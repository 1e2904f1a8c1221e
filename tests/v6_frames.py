"""Random dual-stack traffic for the ICMPv6 echo tests (XSK_GPU_OPT_IPV6).

About half the frames are IPv6, drawn from tests/golden/make_v6_golden.py's builder (VLAN stacks, versions, payload
length errors, Ethernet padding, next headers, types and codes, multicast addresses, bad checksums, truncations); the
rest come from tests/wire_frames.random_frame.  They are placed in a UMEM of random bytes at a fixed stride with
optional start offsets, so a stray write shows up.  spec_batch() runs the Python spec over a batch.
"""
import importlib.util
import os

import numpy as np

from tests.wire_frames import G_DESC, random_frame

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_v6_golden", os.path.join(_HERE, "golden", "make_v6_golden.py"))
G6 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G6)

REC_DTYPE = np.dtype([("verdict", "u1"), ("flags", "u1"), ("ip_proto", "u1"), ("icmp_type", "u1"), ("icmp_code", "u1"),
                      ("ip_vihl", "u1"), ("eth_proto", "<u2"), ("icmp_csum_in", "<u2"), ("icmp_csum_out", "<u2"),
                      ("ip_sum", "<u2"), ("icmp_sum", "<u2")])


def random_frame6(rng: np.random.Generator, max_payload: int = 1400):
    r = rng.random
    vlan = []
    nv = rng.choice([0, 1, 2, 3], p=[0.55, 0.22, 0.18, 0.05])
    for _ in range(nv):
        vlan.append((int(rng.choice([0x8100, 0x88A8])), int(rng.integers(0, 4096))))
    # short payloads often: 62- to 64-byte echoes and messages that end near the 64-B window
    npay = int(rng.integers(0, 12)) if r() < 0.4 else int(rng.integers(0, max_payload + 1))
    addr = lambda: bytes(rng.integers(0, 256, 16, dtype=np.uint8))  # noqa: E731
    kw = dict(
        vlan=vlan, payload=bytes(rng.integers(0, 256, npay, dtype=np.uint8)),
        version=6 if r() < 0.93 else int(rng.integers(0, 16)),
        tc=int(rng.integers(0, 256)), flow=int(rng.integers(0, 1 << 20)), hlim=int(rng.integers(0, 256)),
        nh=58 if r() < 0.9 else int(rng.choice([0, 6, 17, 43, 44, 1])),
        itype=128 if r() < 0.85 else int(rng.choice([129, 135, 136, 1, 8])),
        code=0 if r() < 0.9 else int(rng.integers(1, 16)),
        ident=int(rng.integers(0, 65536)), seq=int(rng.integers(0, 65536)),
        pad=int(rng.integers(1, 40)) if r() < 0.2 else 0, bad_icmp=r() < 0.08,
        src_mac=bytes(rng.integers(0, 256, 6, dtype=np.uint8)), dst_mac=bytes(rng.integers(0, 256, 6, dtype=np.uint8)),
        saddr=addr(), daddr=addr(),
    )
    if r() < 0.04:
        kw["saddr"] = b"\xff" + kw["saddr"][1:]
    if r() < 0.04:
        kw["daddr"] = b"\xff" + kw["daddr"][1:]
    if r() < 0.06:
        kw["plen"] = int(rng.choice([0, 7, 8, int(rng.integers(0, 2000))]))
    f = G6.build6(**kw)
    L = len(f)
    if r() < 0.1:
        L = int(rng.integers(0, L + 1))
    return f, L


def mixed_batch6(n: int, stride: int = 2048, seed: int = 1, offsets: bool = True, max_payload: int = 1400):
    """(umem, descs): n random frames, about half IPv6, at addr = i*stride + (i % 16 if offsets); garbage between."""
    rng = np.random.default_rng(seed)
    umem = rng.integers(0, 256, n * stride + 256, dtype=np.uint8)
    descs = np.zeros(n, G_DESC)
    for i in range(n):
        f, L = random_frame6(rng, max_payload) if rng.random() < 0.5 else random_frame(rng, max_payload)
        off = (i % 16) if offsets else 0
        a = i * stride + off
        assert off + len(f) <= stride
        umem[a:a + len(f)] = np.frombuffer(f, np.uint8)
        descs[i] = (a, L, 0)
    return umem, descs


def spec_batch(umem: np.ndarray, descs: np.ndarray, opts: int):
    """The Python spec over a batch, in place: (verdicts, records, counters).  A descriptor whose [addr, addr + len)
    leaves the UMEM (or len > 2^30) is DROP_BAD_DESC, untouched, its record zero but for the verdict."""
    n = len(descs)
    v = np.zeros(n, np.uint8)
    r = np.zeros(n, REC_DTYPE)
    st = dict(rx_packets=n, rx_bytes=0, tx_packets=0, tx_bytes=0)
    for i in range(n):
        a, L = int(descs[i]["addr"]), int(descs[i]["len"])
        st["rx_bytes"] += L
        if L > (1 << 30) or a > umem.size or L > umem.size - a:
            v[i] = G6.DROP_BAD_DESC
            r[i]["verdict"] = G6.DROP_BAD_DESC
            continue
        # expect() never reads at or past `len` once len >= 14; shorter frames are DROP_SHORT before any read
        frame = umem[a:a + L].tobytes() + b"\0" * max(0, 14 - L)
        vi, rec, out = G6.expect(frame, L, opts)
        v[i] = vi
        for k, x in rec.items():
            r[i][k] = x
        if vi == G6.TX_REPLY:
            umem[a:a + L] = np.frombuffer(out[:L], np.uint8)
            st["tx_packets"] += 1
            st["tx_bytes"] += L
    return v, r, st
