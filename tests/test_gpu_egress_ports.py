"""GPU parity of xsk_gpu_egress_ports_dev against tests/egress_ports_spec.spec_egress_ports: every port's TX descriptor
list and free-frame address list inside the port's own span, the counts, the shared tx counters and the per-port
counter blocks, on both kernel paths (one workgroup up to 1024 frames, three launches above).

Common to every case: the offset words and the rooms are written by device-side copies on the call's stream (the call
never sees them); d_tx, d_free and d_counts are pre-filled with a sentinel and compared WHOLE with what the spec leaves
in a sentinel-filled array, so a store outside a port's lists, between them or behind n_max shows; the input
descriptors carry nonzero `options`; the verdicts take the values 0 to 7 and a few bytes above 7."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import egress_ports_spec as EP  # noqa: E402
from tests import egress_spec as ES  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests.test_gpu_ingress import _dev, same_dev, stats_of, to_dev  # noqa: E402

SENT = 0xEE
STAMP = 0x0123456789ABCDEF  # the timestamp of every counter block: never touched
KEYS = EP.STATS_KEYS


@functools.lru_cache(maxsize=None)
def _batch(n_max, pattern, seed=0):
    """(descs, verdicts) on the host, read-only: distinct addresses, nonzero options, the named reply pattern."""
    descs = ES.random_descs(n_max, seed=n_max + seed)
    verd = ES.verdict_pattern(pattern, n_max, seed=n_max + seed)
    assert (descs["options"] != 0).all()
    descs.setflags(write=False)
    verd.setflags(write=False)
    return descs, verd


def _words(values, buf=None):
    """uint32 words on the device, written by a copy kernel on the current stream (into `buf` when given)."""
    src = torch.from_numpy(np.array(values, np.uint32).view(np.int32)).to(_dev())
    if buf is None:
        return src.clone()
    buf.copy_(src)
    return buf


def listed_stats(descs, verd, o):
    """One xsk_gpu_stats as the transform leaves it over the listed frames [o_0, o_n) (every reply counted as sent)."""
    st = np.zeros(1, X.STATS_DTYPE)
    st["timestamp"] = STAMP
    L, v = descs["len"][o[0]:o[-1]].astype(np.int64), verd[o[0]:o[-1]]
    st["rx_packets"], st["rx_bytes"] = len(L), int(L.sum())
    st["tx_packets"], st["tx_bytes"] = int((v == 0).sum()), int(L[v == 0].sum())
    return st


def preload_port_stats(n_ports):
    ps = np.zeros(n_ports, X.STATS_DTYPE)
    ps["timestamp"] = STAMP
    for j, k in enumerate(KEYS):
        ps[k] = 1000 * (j + 1) + np.arange(n_ports)
    return ps


def port_stats_after(ps, spec, times=1):
    want = ps.copy()
    for p, d in enumerate(spec["port_stats"]):
        for k in KEYS:
            want[k][p] += times * d[k]
    return want


def stats_after(st, spec, times=1):
    want = st.copy()
    want["tx_packets"] = int(st["tx_packets"][0]) + times * spec["d_tx_packets"]
    want["tx_bytes"] = int(st["tx_bytes"][0]) + times * spec["d_tx_bytes"]
    return want


class Ports:
    """Device buffers of egress_ports_dev calls over one (descs, verdicts) input of n_max entries, sentinels in and
    behind every output.  `voff` puts d_verdicts at that byte offset of its allocation, `coff` d_counts, `ooff` d_off
    (both in bytes, multiples of 4)."""

    def __init__(self, descs, verd, n_ports, voff=0, coff=0, ooff=0):
        dev = _dev()
        self.n_max, self.n_ports = len(descs), n_ports
        self.descs, self.verd = descs, verd
        self.d_descs = to_dev(descs) if len(descs) else torch.empty(0, dtype=torch.uint8, device=dev)
        self._vbuf = torch.full((self.n_max + 8,), SENT, dtype=torch.uint8, device=dev)
        self.d_verd = self._vbuf[voff:voff + self.n_max]
        self.d_verd.copy_(torch.from_numpy(np.array(verd)).to(dev))
        self.tx = torch.empty((self.n_max + 4) * 16, dtype=torch.uint8, device=dev)
        self.free = torch.empty((self.n_max + 4) * 8, dtype=torch.uint8, device=dev)
        self._cbuf = torch.empty(n_ports * 16 + 48, dtype=torch.uint8, device=dev)
        self.counts = self._cbuf[coff:coff + n_ports * 16]
        self._obuf = torch.empty(n_ports + 1 + 8, dtype=torch.int32, device=dev)
        self.off = self._obuf[ooff // 4:ooff // 4 + n_ports + 1]
        self.rooms = torch.empty(n_ports, dtype=torch.int32, device=dev)
        wsz = X.egress_ports_workspace_size(self.n_max, n_ports)
        assert (wsz == 0) == (self.n_max <= X.LOWLAT_MAX)
        self.ws = torch.full((wsz,), SENT, dtype=torch.uint8, device=dev) if wsz else None

    def run(self, off, rooms, stats=None, port_stats=None, refill=True):
        """Sentinels, the device words, the call."""
        if refill:
            for t in (self.tx, self.free, self._cbuf):
                t.fill_(SENT)
        self._obuf.fill_(-1)
        _words(off, self.off)
        d_rooms = None if rooms is None else _words(rooms, self.rooms)
        X.egress_ports_dev(self.d_descs, self.d_verd, self.off, self.n_ports, self.n_max, self.tx, self.free,
                           self.counts, tx_room=d_rooms, stats=stats, port_stats=port_stats, workspace=self.ws)
        self.last = (list(off), None if rooms is None else list(rooms))

    def check(self):
        """After a synchronisation: every output against the spec of the last run.  Returns the spec."""
        off, rooms = self.last
        sp = EP.spec_egress_ports(self.descs, self.verd, off, self.n_ports, self.n_max, rooms)
        cb = self._cbuf.cpu().numpy()
        c0 = self.counts.data_ptr() - self._cbuf.data_ptr()
        got = [ES.counts_of(cb[c0 + 16 * p:c0 + 16 * p + 16]) for p in range(self.n_ports)]
        assert got == sp["counts"], (off, rooms, got, sp["counts"])
        assert (cb[:c0] == SENT).all() and (cb[c0 + 16 * self.n_ports:] == SENT).all()
        tx, free = EP.expected_arrays(sp, self.n_max, SENT, 4)
        same_dev(self.tx, to_dev(tx), "d_tx")      # whole arrays: the lists, and the sentinel everywhere else
        same_dev(self.free, to_dev(free), "d_free")
        assert bool((self._vbuf[:self.d_verd.data_ptr() - self._vbuf.data_ptr()] == SENT).all())
        ob = self._obuf.cpu().numpy().view(np.uint32)
        o0 = (self.off.data_ptr() - self._obuf.data_ptr()) // 4
        assert ob[o0:o0 + self.n_ports + 1].tolist() == off and (ob[:o0] == 0xFFFFFFFF).all() \
            and (ob[o0 + self.n_ports + 1:] == 0xFFFFFFFF).all()  # d_off is read, never written
        return sp


def _Rs(verd, o):
    return [int((verd[o[p]:o[p + 1]] == 0).sum()) for p in range(len(o) - 1)]


def _run_with_counters(g, off, rooms):
    """One call with both counter blocks preloaded; everything checked.  Returns the spec."""
    o = EP.offsets(off, g.n_ports, g.n_max)
    st, ps = listed_stats(g.descs, g.verd, o), preload_port_stats(g.n_ports)
    d_st, d_ps = to_dev(st), to_dev(ps)
    g.run(off, rooms, d_st, d_ps)
    torch.cuda.synchronize()
    sp = g.check()
    assert (d_st.cpu().numpy().view(X.STATS_DTYPE) == stats_after(st, sp)).all()
    got = d_ps.cpu().numpy().view(X.STATS_DTYPE)
    assert (got == port_stats_after(ps, sp)).all(), (got, port_stats_after(ps, sp))
    assert (got["timestamp"] == STAMP).all()
    return sp


# ---- the one-workgroup path --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_ports", [1, 8, 64])
@pytest.mark.parametrize("n_max", [1, 64, 65, 1023, 1024])
def test_small_path(n_max, n_ports):
    """Every layout of egress_ports_spec.LAYOUTS, three reply patterns, rooms NULL and R_p // 2; no workspace."""
    for pattern in ("random", "all", "lane63"):
        descs, verd = _batch(n_max, pattern)
        g = Ports(descs, verd, n_ports)
        assert g.ws is None
        for lay in EP.LAYOUTS:
            off = EP.layout(lay, n_ports, n_max, seed=n_ports + n_max)
            Rs = _Rs(verd, EP.offsets(off, n_ports, n_max))
            for rooms in (None, [R // 2 for R in Rs]):
                _run_with_counters(g, off, rooms)


def test_small_path_64_ports_of_3_frames_and_wave_edges():
    descs, verd = _batch(192, "random")
    g = Ports(descs, verd, 64)
    off = [3 * p for p in range(65)]
    sp = _run_with_counters(g, off, [1] * 64)
    assert all(c["n"] == 3 for c in sp["counts"]) and any(c["n_tx_full"] for c in sp["counts"])
    descs, verd = _batch(200, "alternating")
    g = Ports(descs, verd, 8)
    for off in ([0, 63, 64, 65, 127, 128, 129, 191, 200], [63, 63, 64, 64, 65, 128, 128, 128, 199]):
        sp = _run_with_counters(g, off, [2, 0, 1, 40, 0, 3, 100, 1])
        assert sum(c["n"] for c in sp["counts"]) == off[-1] - off[0]


# ---- the three-stage path ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_max,n_ports", [(1025, 1), (1025, 8), (1025, 64), (4099, 64)])
def test_three_stage_path(n_max, n_ports):
    """1025: five workgroups, the last with one frame.  4099 with 64 ports: boundaries inside one workgroup and across
    them."""
    for pattern in ("random", "all", "last_wg"):
        descs, verd = _batch(n_max, pattern)
        g = Ports(descs, verd, n_ports)
        assert g.ws is not None and g.ws.numel() == ((n_max + 255) // 256) * 36 + (n_ports + 1) * 4
        for lay in EP.LAYOUTS:
            off = EP.layout(lay, n_ports, n_max, seed=n_ports + n_max)
            Rs = _Rs(verd, EP.offsets(off, n_ports, n_max))
            rooms = None if lay in ("one", "even") else [(2 * R) // 3 for R in Rs]
            _run_with_counters(g, off, rooms)


def test_three_stage_path_scan_runs_of_two():
    """262147 frames, 8 ports: 1025 workgroups, so a scan thread owns two counts."""
    n_max = 262147
    descs, verd = _batch(n_max, "random")
    g = Ports(descs, verd, 8)
    off = [5, 256 * 300, 256 * 300 + 1, 131072 + 37, 131072 + 37, 64 * 3001, 262000, 262146, 262147]
    Rs = _Rs(verd, off)
    sp = _run_with_counters(g, off, [Rs[0] // 2, 0, 1, 7, Rs[4], Rs[5] - 1, 0xFFFFFFFF, 0])  # (port 3 is empty)
    c = sp["counts"]
    assert c[0]["n_tx_full"] > 0 and c[3]["n"] == 0 and c[4]["n_tx_full"] == 0 and c[5]["n_tx_full"] == 1


# ---- segment edge cases ------------------------------------------------------------------------------------------

EDGE_LAYOUTS = {
    "workgroup edges": [0, 255, 256, 257, 511, 512, 513, 1300],
    "empty first": [0, 0, 300, 700, 1000, 1100, 1200, 1300],
    "empty middle": [0, 256, 256, 256, 512, 900, 900, 1300],
    "empty last": [0, 100, 300, 700, 1000, 1300, 1300, 1300],
    "on no list at both ends": [260, 300, 511, 512, 800, 1000, 1023, 1024],
    "all empty": [512] * 8,
    "above the bound": [0, 400, 1200, 1301, 1305, 5000, 0xFFFFFFFF, 7],
    "descending": [1000, 900, 800, 700, 600, 500, 400, 300],
    "out of order": [10, 600, 300, 900, 100, 1290, 1280, 1299],
}


@pytest.mark.parametrize("name", list(EDGE_LAYOUTS))
def test_segment_edge_cases(name):
    """Seven ports over 1300 frames (six workgroups).  The clamp: words above n_max or descending give the spec's
    segments, and the sentinels behind n_max (and everywhere outside the lists) stay intact -- Ports.check compares the
    whole arrays."""
    n_max, off = 1300, EDGE_LAYOUTS[name]
    descs, verd = _batch(n_max, "random")
    g = Ports(descs, verd, 7)
    o = EP.offsets(off, 7, n_max)
    Rs = _Rs(verd, o)
    for rooms in (None, [R // 2 for R in Rs]):
        sp = _run_with_counters(g, off, rooms)
        assert sp["o"] == o
    if name == "on no list at both ends":
        tx, free = g.tx.cpu().numpy(), g.free.cpu().numpy()
        assert (tx[:260 * 16] == SENT).all() and (tx[1024 * 16:] == SENT).all()
        assert (free[:260 * 8] == SENT).all() and (free[1024 * 8:] == SENT).all()
    if name == "descending":
        assert o == [1000] * 8 and bool((g.tx == SENT).all()) and bool((g.free == SENT).all())


# ---- the rooms ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_max", [1024, 4099])
def test_rooms(n_max):
    """d_tx_room NULL; per port 0, R_p - 1, R_p, R_p + 1; and a mix in which some ports are cut and some are not."""
    n_ports = 8
    descs, verd = _batch(n_max, "random")
    g = Ports(descs, verd, n_ports)
    off = EP.layout("even", n_ports, n_max)
    Rs = _Rs(verd, off)
    assert min(Rs) > 8
    for kind, rooms in (("null", None), ("0", [0] * 8), ("R-1", [R - 1 for R in Rs]), ("R", Rs),
                        ("R+1", [R + 1 for R in Rs]),
                        ("mixed", [(0xFFFFFFFF, 0, R - 1, R // 2, R, R + 1, 3, R - 3)[p] for p, R in enumerate(Rs)])):
        sp = _run_with_counters(g, off, rooms)
        full = [c["n_tx_full"] for c in sp["counts"]]
        if kind in ("null", "R", "R+1"):
            assert not any(full) and [c["n_tx"] for c in sp["counts"]] == Rs
        if kind == "0":
            assert full == Rs and not any(c["n_tx"] for c in sp["counts"])
        if kind == "R-1":
            assert full == [1] * 8
        if kind == "mixed":
            assert any(full) and not all(full)  # both kinds occur: a condition of the input
            assert [f > 0 for f in full] == [False, True, True, True, False, False, True, True]


# ---- the counters ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_max", [777, 3000])
def test_counters(n_max):
    """Each block absent, both absent, two calls back to back into the same blocks, and nothing cut: d_stats as it was."""
    n_ports = 8
    descs, verd = _batch(n_max, "random")
    g = Ports(descs, verd, n_ports)
    off = EP.layout("random", n_ports, n_max, seed=5)
    o = EP.offsets(off, n_ports, n_max)
    Rs = _Rs(verd, o)
    rooms = [R // 3 for R in Rs]
    st, ps = listed_stats(descs, verd, o), preload_port_stats(n_ports)
    # d_port_stats absent
    d_st = to_dev(st)
    g.run(off, rooms, d_st, None)
    torch.cuda.synchronize()
    sp = g.check()
    assert sp["d_tx_packets"] < 0 and (d_st.cpu().numpy().view(X.STATS_DTYPE) == stats_after(st, sp)).all()
    # d_stats absent
    d_ps = to_dev(ps)
    g.run(off, rooms, None, d_ps)
    torch.cuda.synchronize()
    g.check()
    assert (d_ps.cpu().numpy().view(X.STATS_DTYPE) == port_stats_after(ps, sp)).all()
    # both absent
    g.run(off, rooms, None, None)
    torch.cuda.synchronize()
    g.check()
    # two calls back to back on one stream accumulate (the shared block preloaded for two transforms)
    st2 = st.copy()
    for k in KEYS:
        st2[k] *= 2
    d_st, d_ps = to_dev(st2), to_dev(ps)
    g.run(off, rooms, d_st, d_ps)
    g.run(off, rooms, d_st, d_ps, refill=False)
    torch.cuda.synchronize()
    g.check()
    assert (d_st.cpu().numpy().view(X.STATS_DTYPE) == stats_after(st2, sp, 2)).all()
    got = d_ps.cpu().numpy().view(X.STATS_DTYPE)
    assert (got == port_stats_after(ps, sp, 2)).all() and (got["timestamp"] == STAMP).all()
    # nothing cut: the shared block stays as it is
    d_st = to_dev(st)
    g.run(off, Rs, d_st, None)
    torch.cuda.synchronize()
    sp = g.check()
    assert sp["d_tx_packets"] == 0 and (d_st.cpu().numpy().view(X.STATS_DTYPE) == st).all()


# ---- alignment and layout ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("voff", [0, 1, 3])
@pytest.mark.parametrize("n_max", [1000, 5000])
def test_alignment(n_max, voff):
    """d_verdicts at byte offsets 0, 1 and 3 of its allocation; d_counts and d_off at 4-B (not 16-B) aligned addresses."""
    descs, verd = _batch(n_max, "random")
    g = Ports(descs, verd, 8, voff=voff, coff=4 * (1 + voff % 3), ooff=4 * (1 + (voff + 1) % 3))
    assert g.d_verd.data_ptr() % 4 == voff % 4
    for t in (g.counts, g.off):
        assert t.data_ptr() % 4 == 0 and t.data_ptr() % 16 != 0
    off = EP.layout("inner", 8, n_max, seed=voff)
    Rs = _Rs(verd, off)
    sp = _run_with_counters(g, off, [max(R - 2, 0) for R in Rs])
    assert sum(c["n_tx_full"] for c in sp["counts"]) > 0


def test_empty_bound_zeroes_the_counts_and_launches_nothing():
    descs, verd = _batch(64, "all")
    g = Ports(descs, verd, 8)
    for t in (g.tx, g.free, g._cbuf):
        t.fill_(SENT)
    X.egress_ports_dev(g.d_descs, g.d_verd, _words([0, 8, 16, 24, 32, 40, 48, 56, 64]), 8, 0, g.tx, g.free, g.counts)
    torch.cuda.synchronize()
    assert bool((g.counts == 0).all()) and bool((g._cbuf[8 * 16:] == SENT).all())
    assert bool((g.tx == SENT).all()) and bool((g.free == SENT).all())


# ---- against the shipped one-list kernels ------------------------------------------------------------------------

@pytest.mark.parametrize("n_max", [64, 1024, 1025, 4099])
def test_one_port_identity_with_egress_dev(n_max):
    """n_ports == 1, d_off = {0, k}: d_tx, d_free, d_counts[0] and the shared counters equal those of egress_dev with
    *d_n = k, device buffer to device buffer, for k above n_max too."""
    dev = _dev()
    descs, verd = _batch(n_max, "random")
    g = Ports(descs, verd, 1)
    ws = torch.empty(max(X.egress_workspace_size(n_max), 4), dtype=torch.uint8, device=dev)
    for k in sorted({0, 1, n_max - 1, n_max, n_max + 5}):
        R = int((verd[:min(k, n_max)] == 0).sum())
        for room in (None, R // 2):
            st = listed_stats(descs, verd, [0, min(k, n_max)])
            s1, s2 = to_dev(st), to_dev(st)
            g.run([0, k], None if room is None else [room], s1, None)
            tx = torch.full_like(g.tx, SENT)
            free = torch.full_like(g.free, SENT)
            counts = torch.full((16,), SENT, dtype=torch.uint8, device=dev)
            X.egress_dev(g.d_descs, g.d_verd, n_max, tx, free, counts, count=_words([k]),
                         tx_room=None if room is None else _words([room]), stats=s2, workspace=ws)
            torch.cuda.synchronize()
            same_dev(g.tx, tx, "d_tx")
            same_dev(g.free, free, "d_free")
            same_dev(g.counts, counts, "d_counts[0]")
            same_dev(s1, s2, "d_stats")
            g.check()


def test_per_port_parity_with_egress_dev_on_each_segment():
    """8 ports over 4099 frames: port p's lists and counts equal egress_dev called on descs[o_p:], verd[o_p:] with
    n_max = n_p -- the shipped kernels, independently of the Python spec."""
    dev = _dev()
    n_max, n_ports = 4099, 8
    descs, verd = _batch(n_max, "random")
    g = Ports(descs, verd, n_ports)
    off = [3, 40, 40, 1064, 1065, 2500, 2756, 4000, 4090]   # segments of 37, 0, 1024, 1, 1435, 256, 1244, 90 frames
    Rs = _Rs(verd, off)
    rooms = [5, 1, Rs[2] // 2, 0, 0xFFFFFFFF, Rs[5], Rs[6] - 1, 0]
    g.run(off, rooms, None, None)
    torch.cuda.synchronize()
    g.check()
    got_counts = g.counts.cpu().numpy()
    for p in range(n_ports):
        o_p, n_p = off[p], off[p + 1] - off[p]
        tx = torch.full(((n_p + 4) * 16,), SENT, dtype=torch.uint8, device=dev)
        free = torch.full(((n_p + 4) * 8,), SENT, dtype=torch.uint8, device=dev)
        counts = torch.full((16,), SENT, dtype=torch.uint8, device=dev)
        X.egress_dev(g.d_descs[o_p * 16:], g.d_verd[o_p:], n_p, tx, free, counts, tx_room=_words([rooms[p]]))
        torch.cuda.synchronize()
        c = ES.counts_of(counts.cpu().numpy())
        assert ES.counts_of(got_counts[16 * p:16 * p + 16]) == c and c["n"] == n_p
        same_dev(g.tx[o_p * 16:(o_p + c["n_tx"]) * 16], tx[:c["n_tx"] * 16], f"port {p} d_tx")
        same_dev(g.free[o_p * 8:(o_p + c["n_free"]) * 8], free[:c["n_free"] * 8], f"port {p} d_free")
        assert bool((g.tx[(o_p + c["n_tx"]) * 16:off[p + 1] * 16] == SENT).all())
        assert bool((g.free[(o_p + c["n_free"]) * 8:off[p + 1] * 8] == SENT).all())


# ---- the pipeline: steered ingress, then egress per port, on one stream ------------------------------------------

PIPELINE = {  # (opts, default port) -> (offsets, replies per port), worked out from the specs
    (0x17, 0): ([0, 2910, 2919, 2927, 2936, 2942, 2942, 2949, 2952], [1543, 4, 7, 7, 4, 0, 3, 2]),
    (0x17, 0xFF): (None, [8, 4, 7, 7, 4, 0, 3, 2]),
    (0x13, 0): (None, [1791, 1, 8, 6, 10, 0, 4, 6]),
    (0x13, 0xFF): (None, [4, 1, 8, 6, 10, 0, 4, 6]),
}


@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("default_port", [0, 0xFF])
@pytest.mark.parametrize("opts", [0x17, 0x13])
def test_ingress_steer_then_egress_ports(opts, default_port, cut):
    """ingress_spec.pipeline_batch() (4096 frames, 8 ports, 64 entries, port 5 unbound): ingress_steer_dev, then
    egress_ports_dev on its d_out / d_verdicts / d_off, nothing between them.  Every list, count, counter, per-port
    counter and UMEM byte against spec_ingress_steer followed by spec_egress_ports."""
    from tests.test_gpu_ingress_steer import BOUND, N_PORTS, IngressSteer, pipeline_ingress_steer, pipeline_table
    from tests.test_gpu_steer import dev_bound, dev_table
    dev = _dev()
    umem, descs = IS.pipeline_batch()
    n = len(descs)
    after, ref = pipeline_ingress_steer(opts, default_port, BOUND)
    off = [int(x) for x in ref["off"]]
    k = off[N_PORTS]
    Rs = _Rs(ref["verdicts"], off)
    want_off, want_Rs = PIPELINE[(opts, default_port)]
    assert Rs == want_Rs and (want_off is None or off == want_off)
    if default_port == 0xFF and opts == 0x17:
        assert k == 54
    rooms = [R // 2 for R in Rs] if cut else None
    # the spec over n entries: descriptors and verdicts at or above k are never read (o_8 == k)
    out_n = np.zeros(n, X.DESC_DTYPE)
    out_n[:k] = ref["out"]
    verd_n = np.full(n, SENT, np.uint8)
    verd_n[:k] = ref["verdicts"]
    sp = EP.spec_egress_ports(out_n, verd_n, off, N_PORTS, n, rooms)
    if cut:
        assert all((c["n_tx_full"] > 0) == (c["n"] > 0) for c in sp["counts"]) and sp["counts"][5]["n"] == 0
    d_table, n_entries = dev_table(pipeline_table(opts))
    g = IngressSteer(to_dev(umem), to_dev(descs), n, d_table, n_entries, N_PORTS, dev_bound(BOUND))
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    ps = preload_port_stats(N_PORTS)
    d_ps = to_dev(ps)
    d_tx = torch.full(((n + 4) * 16,), SENT, dtype=torch.uint8, device=dev)
    d_free = torch.full(((n + 4) * 8,), SENT, dtype=torch.uint8, device=dev)
    d_counts = torch.full((N_PORTS * 16 + 16,), SENT, dtype=torch.uint8, device=dev)
    ws = torch.empty(X.egress_ports_workspace_size(n, N_PORTS), dtype=torch.uint8, device=dev)
    d_rooms = None if rooms is None else _words(rooms)
    d_after = to_dev(after)
    torch.cuda.synchronize()
    g.run(opts, default_port, stats)
    X.egress_ports_dev(g.out, g.verd, g.off, N_PORTS, n, d_tx, d_free, d_counts[:N_PORTS * 16], tx_room=d_rooms,
                       stats=stats, port_stats=d_ps, workspace=ws)
    torch.cuda.synchronize()
    g.check(d_after, ref)
    cb = d_counts.cpu().numpy()
    assert [ES.counts_of(cb[16 * p:16 * p + 16]) for p in range(N_PORTS)] == sp["counts"]
    assert (cb[N_PORTS * 16:] == SENT).all()
    tx, free = EP.expected_arrays(sp, n, SENT, 4)
    same_dev(d_tx, to_dev(tx), "d_tx")
    same_dev(d_free, to_dev(free), "d_free")
    want = dict(ref["stats"])
    want["tx_packets"] += sp["d_tx_packets"]
    want["tx_bytes"] += sp["d_tx_bytes"]
    assert stats_of(stats) == want and want["tx_packets"] == sum(c["n_tx"] for c in sp["counts"])
    got = d_ps.cpu().numpy().view(X.STATS_DTYPE)
    assert (got == port_stats_after(ps, sp)).all() and (got["timestamp"] == STAMP).all()
    assert sum(d["rx_packets"] for d in sp["port_stats"]) == k == ref["stats"]["rx_packets"]
