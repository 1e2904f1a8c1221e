"""The spec of xsk_gpu_egress_dev (include/xsk_gpu.h) in numpy: the sequential rule, frame by frame.

    reply(i) = verdicts[i] == TX_REPLY;  R(i) = replies below i
    a reply with R(i) < room is submitted: tx[R(i)] = (addr, len, 0)
    every other frame is freed:            free[i - min(R(i), room)] = addr

`spec_egress` walks the batch once and appends; tests/test_egress_spec.py holds an independent line-by-line restatement
of xsk_gpu__rx_emit()'s loop (xsknet_amd/csrc/xsk_gpu_rx.c) to compare it with.
"""
import numpy as np

import oracle

TX_REPLY = 0
UNLIMITED = 0xFFFFFFFF  # room when d_tx_room is NULL
COUNTS_DTYPE = np.dtype([("n", "<u4"), ("n_tx", "<u4"), ("n_tx_full", "<u4"), ("n_free", "<u4")])


def spec_egress(descs: np.ndarray, verdicts: np.ndarray, n: int, room: int = UNLIMITED):
    """(tx, free, counts, d_tx_packets, d_tx_bytes) of the first n frames: tx as DESC_DTYPE with options 0, free as
    uint64 addresses, counts as a dict of n / n_tx / n_tx_full / n_free, and the two (non-positive) counter deltas."""
    d = np.ascontiguousarray(descs, oracle.DESC_DTYPE)
    n = int(n)
    assert 0 <= n <= len(d) and n <= len(verdicts) and 0 <= room <= UNLIMITED
    tx, free = [], []
    below = 0  # R(i)
    lost_bytes = 0
    addrs, lens, verd = d["addr"][:n].tolist(), d["len"][:n].tolist(), np.asarray(verdicts[:n]).tolist()
    for i in range(n):
        addr, length = addrs[i], lens[i]
        if verd[i] == TX_REPLY:
            if below < room:
                tx.append((addr, length, 0))
            else:
                free.append(addr)
                lost_bytes += length
            below += 1
        else:
            free.append(addr)
    n_tx = min(below, room)
    counts = dict(n=n, n_tx=n_tx, n_tx_full=below - n_tx, n_free=n - n_tx)
    assert len(tx) == n_tx and len(free) == counts["n_free"]
    return (np.array(tx, oracle.DESC_DTYPE).reshape(-1), np.array(free, np.uint64).reshape(-1), counts,
            -(below - n_tx), -lost_bytes)


def counts_of(raw: np.ndarray) -> dict:
    """A struct xsk_gpu_egress_counts read back as 16 bytes -> the dict spec_egress returns."""
    c = np.ascontiguousarray(raw).view(COUNTS_DTYPE)[0]
    return {k: int(c[k]) for k in COUNTS_DTYPE.names}


PATTERNS = ("all", "none", "alternating", "random", "lane0", "lane63", "last_wg")


def verdict_pattern(name: str, n: int, seed: int = 0, wg: int = 256) -> np.ndarray:
    """n verdict bytes with the named reply pattern; the non-replies take the values 1 to 7 and a few bytes above 7
    (every value but 0 is "not a reply")."""
    rng = np.random.default_rng(0xE6E55 + seed)
    other = rng.choice(np.array([1, 2, 3, 4, 5, 6, 7, 8, 0x80, 0xEE, 0xFF], np.uint8), size=n)
    i = np.arange(n)
    if name == "all":
        reply = np.ones(n, bool)
    elif name == "none":
        reply = np.zeros(n, bool)
    elif name == "alternating":
        reply = i % 2 == 0
    elif name == "random":
        reply = rng.random(n) < 0.5
    elif name == "lane0":
        reply = i % 64 == 0
    elif name == "lane63":
        reply = i % 64 == 63
    elif name == "last_wg":
        reply = i >= ((n - 1) // wg) * wg if n else np.zeros(0, bool)
    else:
        raise ValueError(name)
    return np.where(reply, np.uint8(TX_REPLY), other).astype(np.uint8)


def random_descs(n: int, seed: int = 0) -> np.ndarray:
    """n descriptors with distinct addresses (so the lists can be compared as sets too), lengths 14..1514 and NONZERO
    options (the TX list must carry 0 there, not a copy)."""
    rng = np.random.default_rng(0xDE5C + seed)
    d = np.zeros(n, oracle.DESC_DTYPE)
    d["addr"] = (rng.permutation(n).astype(np.uint64) * np.uint64(2048)) + rng.integers(0, 256, n).astype(np.uint64)
    d["len"] = rng.integers(14, 1515, n).astype(np.uint32)
    d["options"] = rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return d
