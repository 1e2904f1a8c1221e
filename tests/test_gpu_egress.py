"""GPU parity of xsk_gpu_egress_dev against tests/egress_spec.spec_egress: the TX descriptor list, the free-frame address
list, the counts and the tx counters, on both kernel paths (one workgroup up to 1024 frames, three launches above).

Common to every case: the frame count and the ring's room are written by device-side fills on the call's stream (the
call never sees them); d_tx and d_free are pre-filled with a sentinel that must survive at or past the counts; the input
descriptors carry nonzero `options` (a copied descriptor would show); the verdicts take the values 0 to 7 and a few
bytes above 7."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import egress_spec as ES  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests.test_gpu_ingress import Ingress, _dev, same_dev, stats_of, to_dev  # noqa: E402

SENT = 0xEE
STAMP = 0x0123456789ABCDEF  # d_stats.timestamp: never touched


@functools.lru_cache(maxsize=None)
def _batch(n_max, pattern, seed=0):
    """(descs, verdicts) on the host, read-only: distinct addresses, nonzero options, the named reply pattern."""
    descs = ES.random_descs(n_max, seed=n_max + seed)
    verd = ES.verdict_pattern(pattern, n_max, seed=n_max + seed)
    assert (descs["options"] != 0).all() and set(np.unique(verd).tolist()) <= {0, 1, 2, 3, 4, 5, 6, 7, 8, 0x80, 0xEE, 0xFF}
    descs.setflags(write=False)
    verd.setflags(write=False)
    return descs, verd


def _word(value):
    """A uint32 on the device written by a fill kernel on the current stream, or None."""
    if value is None:
        return None
    t = torch.zeros(1, dtype=torch.int32, device=_dev())
    t.fill_(int(np.uint32(value).astype(np.int32)))
    return t


def preload_stats(descs, verd, n):
    """One xsk_gpu_stats as the transform leaves it over the first n frames (every reply counted as sent)."""
    st = np.zeros(1, X.STATS_DTYPE)
    st["timestamp"] = STAMP
    for k, v in IS.prefix_stats(descs, verd, n).items():
        st[k] = v
    return st


def stats_after(st, d_packets, d_bytes):
    """`st` with the two (non-positive) deltas of spec_egress applied to the tx counters."""
    want = st.copy()
    want["tx_packets"] = int(st["tx_packets"][0]) + d_packets
    want["tx_bytes"] = int(st["tx_bytes"][0]) + d_bytes
    return want


class Egress:
    """Device buffers of egress_dev calls over one (descs, verdicts) input of n_max entries, sentinels in and behind
    every output.  `voff` puts d_verdicts at that byte offset of its allocation, `coff` d_counts at that offset."""

    def __init__(self, descs, verd, voff=0, coff=0):
        dev = _dev()
        self.n_max = len(descs)
        self.descs, self.verd = descs, verd
        self.d_descs = to_dev(descs)
        self._vbuf = torch.full((self.n_max + 8,), SENT, dtype=torch.uint8, device=dev)
        self.d_verd = self._vbuf[voff:voff + self.n_max]
        self.d_verd.copy_(torch.from_numpy(np.array(verd)).to(dev))
        assert self.d_verd.data_ptr() % 4 == voff % 4
        self.tx = torch.empty((self.n_max + 4) * 16, dtype=torch.uint8, device=dev)
        self.free = torch.empty((self.n_max + 4) * 8, dtype=torch.uint8, device=dev)
        self._cbuf = torch.empty(48, dtype=torch.uint8, device=dev)
        self.counts = self._cbuf[coff:coff + 16]
        wsz = X.egress_workspace_size(self.n_max)
        assert (wsz == 0) == (self.n_max <= X.LOWLAT_MAX)
        self.ws = torch.empty(wsz, dtype=torch.uint8, device=dev) if wsz else None

    def run(self, count, room, stats=None, null_count=False):
        """Sentinels, the two device words, the call.  `count` is what *d_n holds (None with null_count: d_n NULL)."""
        for t in (self.tx, self.free, self._cbuf):
            t.fill_(SENT)
        d_n = None if null_count else _word(count)
        X.egress_dev(self.d_descs, self.d_verd, self.n_max, self.tx, self.free, self.counts, count=d_n,
                     tx_room=_word(room), stats=stats, workspace=self.ws)
        self.n = self.n_max if null_count else min(count, self.n_max)
        self.room = ES.UNLIMITED if room is None else room

    def check(self):
        """After a synchronisation: every output against spec_egress of (n, room).  Returns the spec."""
        tx, free, c, dp, db = ES.spec_egress(self.descs, self.verd, self.n, self.room)
        cb = self._cbuf.cpu().numpy()
        off = self.counts.data_ptr() - self._cbuf.data_ptr()
        got = ES.counts_of(cb[off:off + 16])
        assert got == c, (got, c, self.n, self.room)
        assert (cb[:off] == SENT).all() and (cb[off + 16:] == SENT).all()  # d_counts is 16 bytes
        same_dev(self.tx[:c["n_tx"] * 16], to_dev(tx), "d_tx")
        assert bool((self.tx[c["n_tx"] * 16:] == SENT).all()), "d_tx written at or past n_tx"
        same_dev(self.free[:c["n_free"] * 8], to_dev(free), "d_free")
        assert bool((self.free[c["n_free"] * 8:] == SENT).all()), "d_free written at or past n_free"
        assert bool((self._vbuf[:self.d_verd.data_ptr() - self._vbuf.data_ptr()] == SENT).all())
        return tx, free, c, dp, db


def _counts_for(n_max):
    return sorted({0, 1, max(n_max - 1, 0), n_max, n_max + 5})


# ---- the one-workgroup path --------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", ES.PATTERNS)
@pytest.mark.parametrize("n_max", [1, 64, 65, 1023, 1024])
def test_small_path(n_max, pattern):
    """*d_n in {0, 1, n_max - 1, n_max, n_max + 5 (the clamp)}, no workspace, unlimited room and a room of R // 2."""
    descs, verd = _batch(n_max, pattern)
    g = Egress(descs, verd)
    assert g.ws is None
    for count in _counts_for(n_max):
        n = min(count, n_max)
        R = int((verd[:n] == 0).sum())
        for room in (None, R // 2):
            st = preload_stats(descs, verd, n)
            d_st = to_dev(st)
            g.run(count, room, d_st)
            torch.cuda.synchronize()
            _, _, c, dp, db = g.check()
            assert c["n"] == n
            assert (d_st.cpu().numpy().view(X.STATS_DTYPE) == stats_after(st, dp, db)).all()


def test_small_path_with_a_null_count():
    descs, verd = _batch(1000, "random")
    g = Egress(descs, verd)
    g.run(None, 100, None, null_count=True)
    torch.cuda.synchronize()
    _, _, c, _, _ = g.check()
    assert c["n"] == 1000 and c["n_tx"] == 100 and c["n_tx_full"] > 0


# ---- the three-stage path ----------------------------------------------------------------------------------------

THREE = [
    # n_max, *d_n values: 0, inside a wave, on a wave edge (not a workgroup's), on a workgroup edge, the bound, above it
    (1025, (0, 1, 1000, 15 * 64, 1024, 1025, 1030)),   # five workgroups, the last with one frame
    (262147, (0, 131072 + 37, 64 * 2001, 256 * 700, 262146, 262147, 262152)),  # 1025 workgroups: scan runs of two
]


@pytest.mark.parametrize("pattern", ES.PATTERNS)
@pytest.mark.parametrize("n_max,counts", THREE)
def test_three_stage_path(n_max, counts, pattern):
    descs, verd = _batch(n_max, pattern)
    g = Egress(descs, verd)
    assert g.ws is not None and g.ws.numel() == ((n_max + 255) // 256) * 4
    for count in counts:
        n = min(count, n_max)
        R = int((verd[:n] == 0).sum())
        st = preload_stats(descs, verd, n)
        d_st = to_dev(st)
        room = None if count % 2 else (2 * R) // 3
        g.run(count, room, d_st)
        torch.cuda.synchronize()
        _, _, c, dp, db = g.check()
        assert c["n"] == n
        assert (d_st.cpu().numpy().view(X.STATS_DTYPE) == stats_after(st, dp, db)).all()


def test_three_stage_path_with_a_null_count():
    descs, verd = _batch(1281, "alternating")
    g = Egress(descs, verd)
    g.run(None, None, None, null_count=True)
    torch.cuda.synchronize()
    _, _, c, _, _ = g.check()
    assert c == dict(n=1281, n_tx=641, n_tx_full=0, n_free=640)


# ---- the ring's room ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", ["random", "all"])
@pytest.mark.parametrize("n_max", [1024, 4099])
def test_room(n_max, pattern):
    """d_tx_room NULL, 0, 1, a value that cuts inside a wave, one that cuts on a workgroup edge (of the three-stage
    path: frame 512; a wave edge of the one-workgroup path), R - 1, R, R + 1."""
    descs, verd = _batch(n_max, pattern)
    R = int((verd == 0).sum())
    inside = int((verd[:512 + 21] == 0).sum())   # the first reply left out lies at or behind frame 533
    edge = int((verd[:512] == 0).sum())          # ... at or behind frame 512
    g = Egress(descs, verd)
    cut = {1, inside, edge, R - 1}
    for room in (None, 0, 1, inside, edge, R - 1, R, R + 1):
        st = preload_stats(descs, verd, n_max)
        d_st = to_dev(st)
        g.run(n_max, room, d_st)
        torch.cuda.synchronize()
        _, _, c, dp, db = g.check()
        if room in cut:
            assert 0 < c["n_tx"] and 0 < c["n_tx_full"], (room, c)  # a condition of the input
        if room is None or room >= R:
            assert c["n_tx_full"] == 0 and c["n_tx"] == R
        if room == 0:
            assert c["n_tx"] == 0 and c["n_free"] == n_max and c["n_tx_full"] == R
        got = d_st.cpu().numpy().view(X.STATS_DTYPE)[0]
        assert int(got["tx_packets"]) == c["n_tx"] and int(got["tx_bytes"]) == int(st["tx_bytes"][0]) + db
        assert int(got["timestamp"]) == STAMP and got["rx_packets"] == st["rx_packets"][0] \
            and got["rx_bytes"] == st["rx_bytes"][0]


# ---- verdict and counts alignment --------------------------------------------------------------------------------

@pytest.mark.parametrize("voff", [0, 1, 3])
@pytest.mark.parametrize("n_max", [1000, 5000])
def test_verdicts_at_any_byte_alignment(n_max, voff):
    """d_verdicts at byte offsets 0, 1 and 3 of its allocation; d_counts at a 4-B (not 16-B) aligned address."""
    descs, verd = _batch(n_max, "random")
    g = Egress(descs, verd, voff=voff, coff=4 * (1 + voff % 3))
    assert g.counts.data_ptr() % 4 == 0 and g.counts.data_ptr() % 16 != 0
    R = int((verd == 0).sum())
    g.run(n_max, R - 7, None)
    torch.cuda.synchronize()
    _, _, c, _, _ = g.check()
    assert c["n_tx_full"] == 7


# ---- the counters ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_max", [777, 3000])
def test_counters(n_max):
    """d_stats preloaded with the transform's counters ends at the spec's values; d_stats == NULL runs; two calls back
    to back on one stream accumulate into one d_stats."""
    d1, v1 = _batch(n_max, "random")
    d2, v2 = _batch(n_max, "alternating", seed=1)
    g1, g2 = Egress(d1, v1), Egress(d2, v2)
    R1, R2 = int((v1 == 0).sum()), int((v2 == 0).sum())
    st = preload_stats(d1, v1, n_max)
    for k, v in IS.prefix_stats(d2, v2, n_max).items():
        st[k] += v
    d_st = to_dev(st)
    torch.cuda.synchronize()
    g1.run(n_max, R1 // 3, d_st)
    g2.run(n_max, R2 - 1, d_st)
    torch.cuda.synchronize()
    _, _, c1, dp1, db1 = g1.check()
    _, _, c2, dp2, db2 = g2.check()
    assert c1["n_tx_full"] > 0 and c2["n_tx_full"] == 1
    got = d_st.cpu().numpy().view(X.STATS_DTYPE)[0]
    assert int(got["tx_packets"]) == int(st["tx_packets"][0]) + dp1 + dp2 == c1["n_tx"] + c2["n_tx"]
    assert int(got["tx_bytes"]) == int(st["tx_bytes"][0]) + db1 + db2
    assert int(got["rx_packets"]) == 2 * n_max and int(got["timestamp"]) == STAMP
    # no counters
    g1.run(n_max, R1 // 3, None)
    torch.cuda.synchronize()
    g1.check()
    # nothing to take back: the counters stay as they are
    d_st2 = to_dev(st)
    g1.run(n_max, R1, d_st2)
    torch.cuda.synchronize()
    g1.check()
    assert (d_st2.cpu().numpy().view(X.STATS_DTYPE) == st).all()


def test_empty_bound_zeroes_the_counts_and_launches_nothing():
    descs, verd = _batch(64, "all")
    g = Egress(descs, verd)
    for t in (g.tx, g.free, g._cbuf):
        t.fill_(SENT)
    X.egress_dev(g.d_descs, g.d_verd, 0, g.tx, g.free, g.counts, count=_word(64))
    torch.cuda.synchronize()
    assert ES.counts_of(g.counts.cpu().numpy()) == dict(n=0, n_tx=0, n_tx_full=0, n_free=0)
    assert bool((g.tx == SENT).all()) and bool((g.free == SENT).all()) and bool((g._cbuf[16:] == SENT).all())


# ---- the pipeline: ingress, then egress, on one stream -----------------------------------------------------------

@pytest.mark.parametrize("cut", [False, True])
def test_ingress_then_egress(cut):
    """ingress_spec.pipeline_batch() (4096 frames, opts 0x17): ingress_dev, then egress_dev with count = nout, nothing
    between them.  Every list, count and counter against spec_ingress followed by spec_egress, every UMEM byte against
    the transform's result."""
    dev = _dev()
    opts = 0x17
    umem, descs = IS.pipeline_batch()
    after, ref = IS.pipeline_ingress(opts, True)
    n, k = len(descs), ref["nout"]
    R = int((ref["verdicts"] == IS.TX_REPLY).sum())
    assert 0 < R < k < n
    room = R // 2 if cut else None
    tx, free, c, dp, db = ES.spec_egress(ref["out"], ref["verdicts"], k, ES.UNLIMITED if room is None else room)
    g = Ingress(to_dev(umem), to_dev(descs), n)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    d_tx = torch.full(((n + 4) * 16,), SENT, dtype=torch.uint8, device=dev)
    d_free = torch.full(((n + 4) * 8,), SENT, dtype=torch.uint8, device=dev)
    d_counts = torch.full((32,), SENT, dtype=torch.uint8, device=dev)
    ws = torch.empty(X.egress_workspace_size(n), dtype=torch.uint8, device=dev)
    d_room = _word(room)
    d_after = to_dev(after)
    torch.cuda.synchronize()
    g.run(opts, True, stats)
    X.egress_dev(g.out, g.verd, n, d_tx, d_free, d_counts[:16], count=g.nout, tx_room=d_room, stats=stats, workspace=ws)
    torch.cuda.synchronize()
    g.check(d_after, ref["actions"], ref["out"], ref["verdicts"], ref["recs"])
    assert ES.counts_of(d_counts[:16].cpu().numpy()) == c and bool((d_counts[16:] == SENT).all())
    assert c["n"] == k and (c["n_tx_full"] > 0) == cut
    same_dev(d_tx[:c["n_tx"] * 16], to_dev(tx), "d_tx")
    same_dev(d_free[:c["n_free"] * 8], to_dev(free), "d_free")
    assert bool((d_tx[c["n_tx"] * 16:] == SENT).all()) and bool((d_free[c["n_free"] * 8:] == SENT).all())
    want = dict(ref["stats"])
    want["tx_packets"] += dp
    want["tx_bytes"] += db
    assert stats_of(stats) == want and want["tx_packets"] == c["n_tx"]
