"""GPU parity of xsk_gpu_neigh_dev: ARP requests and neighbour solicitations answered in place over a device-resident
descriptor list.  Byte-exact against tests/neigh_spec.py over every output array and the whole UMEM.

Common to every case: the UMEM, the descriptors, the verdicts, the ports, the reply lengths and the counters each sit
between two runs of the sentinel byte SENT, which must survive; the frames lie at odd addresses with sentinel bytes
between them, the last one ends at the UMEM's last byte; the outputs start out as SENT, so an index the call must not
write shows; the descriptors behind the count are real requests, so an index the call must not read shows in the UMEM.
One seeded batch of 1025 frames (tests/neigh_frames.py) serves every size as a prefix; the condition on it -- at least
a quarter answered, every verdict present -- is asserted from the spec's output."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import neigh_frames as NF  # noqa: E402
from tests import neigh_spec as NS  # noqa: E402
from tests.test_gpu_egress import SENT  # noqa: E402
from tests.test_gpu_ingress import _dev  # noqa: E402
from tests.test_gpu_rx_step_dev import Guarded  # noqa: E402

N_ALL, OPTS = 1025, 0x17
BASE = dict(seen=1 << 40, arp_replies=7, na_replies=0, reply_bytes=(1 << 33) + 5)  # the counters are accumulated


@functools.lru_cache(maxsize=None)
def batch(opts=OPTS, seed=5):
    """(UMEM, descriptors) of the shared batch; read-only."""
    frames = [f for f, _ in NF.random_frames(N_ALL, opts, seed)]
    umem, descs = NF.layout(frames)
    v, _, _ = NS.spec_neigh(umem.copy(), descs, N_ALL, opts, NF.table(), NF.N_PORTS, NF.BOUND)
    NF.check_condition(v)
    NF.check_condition(v[:257])  # the prefix most cases use
    umem.setflags(write=False)
    descs.setflags(write=False)
    return umem, descs


def dev_table(table: dict):
    """(Guarded or None, n_entries): the prepared table in device memory."""
    arr = NS.table_array(X, table)
    return (Guarded(arr.nbytes, arr.view(np.uint8)) if len(arr) else None), len(arr)


def dev_word(value, dtype):
    return None if value is None else Guarded(np.dtype(dtype).itemsize, np.array([value], dtype))


def run(umem, descs, n_max, opts, table, n_ports, bound=NS.ALL_BOUND, count=None, rlen=True, stats=True):
    """The call on guarded copies against the spec on host copies; every byte of everything compared."""
    _dev()
    n = n_max if count is None else min(count, n_max)
    d_umem, d_descs = Guarded(umem.nbytes, umem), Guarded(max(n_max, 1) * 16, descs[:n_max] if n_max else None)
    d_tab, n_entries = dev_table(table)
    d_bound = dev_word(None if bound == NS.ALL_BOUND else bound, np.uint64)
    d_n = dev_word(count, np.uint32)
    d_v, d_p = Guarded(max(n_max, 1)), Guarded(max(n_max, 1))
    d_r = Guarded(4 * max(n_max, 1)) if rlen else None
    d_s = Guarded(32, np.array([tuple(BASE[k] for k in NS.STATS_KEYS)], X.NEIGH_STATS_DTYPE)) if stats else None
    X.neigh_dev(d_umem.data, d_descs.data, n_max, d_tab.data if d_tab else None, n_entries, n_ports, d_v.data, d_p.data,
                count=d_n.data if d_n else None, bound=d_bound.data if d_bound else None,
                reply_len=d_r.data if d_r else None, nstats=d_s.data if d_s else None, opts=opts)
    torch.cuda.synchronize()
    u = umem.copy()
    st = dict(BASE)
    verdicts, ports, rlens = NS.spec_neigh(u, descs, n, opts, table, n_ports, bound, st)
    assert (d_umem.get() == u).all(), np.nonzero(d_umem.get() != u)[0][:8]
    want_v, want_p = np.full(max(n_max, 1), SENT, np.uint8), np.full(max(n_max, 1), SENT, np.uint8)
    want_v[:n], want_p[:n] = verdicts, ports
    assert (d_v.get() == want_v).all() and (d_p.get() == want_p).all()
    if rlen:
        want_r = np.full(4 * max(n_max, 1), SENT, np.uint8).view(np.uint32)
        for i, r in enumerate(rlens):
            if r is not None:
                want_r[i] = r
        assert (d_r.get(np.uint32) == want_r).all()
    if stats:
        got = d_s.get(X.NEIGH_STATS_DTYPE)[0]
        assert {k: int(got[k]) for k in NS.STATS_KEYS} == st
    if n_max:
        assert (d_descs.get() == descs[:n_max].view(np.uint8)).all()
    for g in (d_umem, d_descs, d_tab, d_bound, d_n, d_v, d_p, d_r, d_s):
        assert g is None or g.intact()
    return verdicts


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_around_the_wave_and_the_workgroup(n):
    umem, descs = batch()
    run(umem, descs, n, OPTS, NF.table(), NF.N_PORTS, NF.BOUND)


@pytest.mark.parametrize("count", [0, 700, 5000, None])
def test_the_count_word_is_read_on_the_device_and_clamped(count):
    """n_max = 1025: five workgroups, the last with one lane; *d_n = 0 touches nothing, 5000 clamps to 1025."""
    umem, descs = batch()
    v = run(umem, descs, N_ALL, OPTS, NF.table(), NF.N_PORTS, NF.BOUND, count=count)
    assert len(v) == (1025 if count in (None, 5000) else count)


def test_n_max_zero_launches_nothing():
    umem, descs = batch()
    run(umem, descs, 0, OPTS, NF.table(), NF.N_PORTS, NF.BOUND)


@pytest.mark.parametrize("n_entries", [0, 1, 1023, 1024])
def test_table_sizes(n_entries):
    """An empty table (no LDS at all), one entry, and the two sizes around the search's last probe."""
    umem, descs = batch()
    table = NF.big_table(n_entries)
    v = run(umem, descs, 257, OPTS, table, NF.N_PORTS, NF.BOUND)
    answered = sum(x in (NS.ARP_REPLY, NS.NA_REPLY) for x in v)
    assert answered == 0 if n_entries == 0 else answered >= 1
    if n_entries >= 1023:
        assert answered >= 64 and NS.UNKNOWN in v and NS.UNBOUND in v


def test_descriptors_outside_the_umem_and_a_frame_at_its_last_byte():
    umem, descs = batch()
    d = descs[:70].copy()
    size = len(umem)
    last = descs[N_ALL - 1]  # ends at the UMEM's last byte
    assert int(last["addr"]) + int(last["len"]) == size
    d[3] = last
    d[10] = (size - 10, 60, 0)        # crosses the end
    d[11] = (size + 5, 60, 0)         # begins behind it
    d[12] = (size, 0, 0)              # empty, at the end
    d[13] = (0, (1 << 30) + 1, 0)     # longer than XSK_GPU_MAX_LEN
    d[14] = (0xFFFFFFFFFFFFFFF0, 64, 0)
    d[15] = (int(descs[20]["addr"]), 0xFFFFFFFF, 0)
    v = run(umem, d, 70, OPTS, NF.table(), NF.N_PORTS, NF.BOUND)
    assert v[10:16] == [NS.NONE] * 6


def test_without_reply_lengths_and_counters():
    umem, descs = batch()
    run(umem, descs, 257, OPTS, NF.table(), NF.N_PORTS, NF.BOUND, rlen=False, stats=False)
    run(umem, descs, 65, OPTS, NF.table(), NF.N_PORTS, NF.BOUND, rlen=True, stats=False)


@pytest.mark.parametrize("n_ports,bound", [(1, NS.ALL_BOUND), (64, NS.ALL_BOUND), (8, NS.ALL_BOUND & ~(1 << 3) & ~(1 << 0)),
                                           (64, 1 << 9), (8, 0)])
def test_port_counts_and_a_bound_word_with_holes(n_ports, bound):
    umem, descs = batch()
    v = run(umem, descs, 257, OPTS, NF.table(), n_ports, bound)
    assert (NS.UNBOUND in v) == (not (n_ports == 64 and bound == NS.ALL_BOUND))  # the table's ports reach 9
    if bound == 0:
        assert NS.ARP_REPLY not in v and NS.NA_REPLY not in v
    else:
        assert NS.ARP_REPLY in v or NS.NA_REPLY in v


@pytest.mark.parametrize("opts", NF.OPTS)
def test_the_golden_cases_under_every_option_word(opts):
    cases = NF.golden_frames(opts)
    umem, descs = NF.layout([f for f, _ in cases])
    v = run(umem, descs, len(cases), opts, NF.table(), NF.N_PORTS, NF.BOUND)
    assert v == [want["verdict"] for _, want in cases]
    umem, descs = NF.layout([f for f, _ in cases], gap=0, odd=False)  # frames back to back
    run(umem, descs, len(cases), opts, NF.table(), NF.N_PORTS, NF.BOUND)
