"""GPU parity of xsk_gpu_unreach_dev: UDP probes for a closed port answered with ICMP / ICMPv6 port unreachable in place
over a device-resident descriptor list.  Byte-exact against tests/unreach_spec.py over every output array and the whole
UMEM.

Common to every case: the UMEM, the descriptors, the verdicts, the ports, the reply lengths, the open-port map and the
counters each sit between two runs of the sentinel byte SENT, which must survive; every frame has a chunk of its own
filled with sentinel bytes, so a byte the longer reply must not write shows; the outputs start out as SENT, so an index
the call must not write shows; the descriptors behind the count are real probes, so an index the call must not read
shows in the UMEM.  One seeded batch of 1025 frames (tests/unreach_frames.py) serves every size as a prefix; the
condition on it -- at least a quarter answered, every verdict present -- is asserted from the spec's output."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import unreach_frames as UF  # noqa: E402
from tests import unreach_spec as US  # noqa: E402
from tests.test_gpu_egress import SENT  # noqa: E402
from tests.test_gpu_ingress import _dev  # noqa: E402
from tests.test_gpu_neigh import dev_table, dev_word  # noqa: E402
from tests.test_gpu_rx_step_dev import Guarded  # noqa: E402

N_ALL, OPTS = 1025, 0x17
BASE = dict(seen=1 << 40, unreach4=7, unreach6=0, reply_bytes=(1 << 33) + 5, limited=3)  # the counters are accumulated
G = UF.G


@functools.lru_cache(maxsize=None)
def batch(opts=OPTS, seed=5):
    """(UMEM, descriptors) of the shared batch; read-only."""
    frames = UF.random_frames(N_ALL, opts, seed)
    umem, descs = UF.layout([f for f, _, _ in frames], [r for _, r, _ in frames])
    v, _, _ = US.spec_unreach(umem.copy(), descs, N_ALL, opts, UF.table(), UF.N_PORTS, UF.BOUND, UF.OPEN, UF.CHUNK)
    UF.check_condition(v)
    UF.check_condition(v[:257])  # the prefix most cases use
    umem.setflags(write=False)
    descs.setflags(write=False)
    return umem, descs


def dev_open(open_ports):
    return None if open_ports is None else Guarded(8192, US.open_map(open_ports))


def run(umem, descs, n_max, opts, table, n_ports, bound=US.ALL_BOUND, open_ports=UF.OPEN, chunk=UF.CHUNK, count=None,
        rlen=True, stats=True):
    """The call on guarded copies against the spec on host copies; every byte of everything compared."""
    _dev()
    n = n_max if count is None else min(count, n_max)
    d_umem, d_descs = Guarded(umem.nbytes, umem), Guarded(max(n_max, 1) * 16, descs[:n_max] if n_max else None)
    d_tab, n_entries = dev_table(table)
    d_bound = dev_word(None if bound == US.ALL_BOUND else bound, np.uint64)
    d_n = dev_word(count, np.uint32)
    d_open = dev_open(open_ports)
    d_v, d_p = Guarded(max(n_max, 1)), Guarded(max(n_max, 1))
    d_r = Guarded(4 * max(n_max, 1)) if rlen else None
    base = np.zeros(1, X.UNREACH_STATS_DTYPE)
    for k in US.STATS_KEYS:
        base[0][k] = BASE[k]
    base[0]["reserved"] = (11, 12, 13)
    d_s = Guarded(64, base) if stats else None
    X.unreach_dev(d_umem.data, d_descs.data, n_max, d_tab.data if d_tab else None, n_entries, n_ports, chunk, d_v.data,
                  d_p.data, count=d_n.data if d_n else None, bound=d_bound.data if d_bound else None,
                  open_ports=d_open.data if d_open else None, reply_len=d_r.data if d_r else None,
                  ustats=d_s.data if d_s else None, opts=opts)
    torch.cuda.synchronize()
    u = umem.copy()
    st = dict(BASE)
    verdicts, ports, rlens = US.spec_unreach(u, descs, n, opts, table, n_ports, bound, open_ports, chunk, st)
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
        got = d_s.get(X.UNREACH_STATS_DTYPE)[0]
        assert {k: int(got[k]) for k in US.STATS_KEYS} == st and list(got["reserved"]) == [11, 12, 13]
    if n_max:
        assert (d_descs.get() == descs[:n_max].view(np.uint8)).all()
    if d_open:
        assert (d_open.get() == US.open_map(open_ports)).all()
    for g in (d_umem, d_descs, d_tab, d_bound, d_n, d_open, d_v, d_p, d_r, d_s):
        assert g is None or g.intact()
    return verdicts


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1024])
def test_sizes_around_the_wave_and_the_workgroup(n):
    umem, descs = batch()
    run(umem, descs, n, OPTS, UF.table(), UF.N_PORTS, UF.BOUND)


@pytest.mark.parametrize("count", [0, 700, 5000, None])
def test_the_count_word_is_read_on_the_device_and_clamped(count):
    """n_max = 1025: five workgroups, the last with one lane; *d_n = 0 touches nothing, 5000 clamps to 1025."""
    umem, descs = batch()
    v = run(umem, descs, N_ALL, OPTS, UF.table(), UF.N_PORTS, UF.BOUND, count=count)
    assert len(v) == (1025 if count in (None, 5000) else count)


def test_n_max_zero_launches_nothing():
    umem, descs = batch()
    run(umem, descs, 0, OPTS, UF.table(), UF.N_PORTS, UF.BOUND)


def shapes():
    """The shapes the rewrite can go wrong at, field by field from the generator: ihl 5 and 15 (q = 28 and 68: the move
    does not and does overlap itself); pl 8, 1191, 1192 and 1193 (q = 48, 1231, 1232 and 1232: both sides of the cap);
    an odd quote; a reply shorter and a reply longer than len; each at 0, 1 and 2 tags; a chunk that fits to the byte and
    one that is one byte short.  Returns [(frame, room, whether that is one byte short)]."""
    cases = [G.udp4_case(), G.udp4_case(ihl=15, data=5), G.udp4_case(data=0), G.udp4_case(data=0, pad=40),
             G.udp4_case(ihl=15, data=0, pad=90), G.udp6_case(data=0), G.udp6_case(data=1183), G.udp6_case(data=1184),
             G.udp6_case(data=1185), G.udp6_case(entry=G.OWN6_LL, data=33), G.udp6_case(data=0, pad=70)]
    out = []
    for frame, reply in cases:
        for tags in G.TAGS:
            f, R = frame(tags), len(reply(tags)[0])
            if R >= len(f):
                out += [(f, None, False), (f, R, False), (f, R - 1, True), (f, R + 1, False)]
            else:  # the reply is the shorter one: the frame itself ends at its chunk's end
                out += [(f, None, False), (f, len(f), False), (f, len(f) + 1, False)]
    return out


def test_every_shape_of_the_rewrite_at_even_and_odd_addresses():
    sh = shapes()
    parities = set()
    for lead in (0, 1):  # one more frame in front moves every frame on by one of layout()'s offsets: 1 (odd), then 2 (even)
        cases = [(G.udp4_case()[0](()), None, False)] * lead + sh
        umem, descs = UF.layout([f for f, _, _ in cases], [r for _, r, _ in cases])
        v = run(umem, descs, len(cases), OPTS, UF.table(), UF.N_PORTS, UF.BOUND)
        assert [x == US.NO_ROOM for x in v] == [short for _, _, short in cases] and v.count(US.NO_ROOM) == 8 * 3
        assert v.count(US.UNREACH4) + v.count(US.UNREACH6) == len(cases) - 8 * 3
        parities |= {int(d["addr"]) & 1 for d, (_, r, _) in zip(descs, cases) if r is None}
        parities |= {2 + (int(d["addr"]) & 1) for d, (f, r, _) in zip(descs, cases) if r is not None and r >= len(f)}
    assert parities == {0, 1, 2, 3}


def test_the_umems_end_is_a_bound_of_its_own():
    """The last chunk is cut short: a reply that fits its chunk but not the UMEM is NO_ROOM, and one that ends at the
    UMEM's last byte is written."""
    frame, reply = G.udp6_case(data=600)
    f = frame(())
    R = len(reply(())[0])
    assert R > len(f)
    for spare, want in ((0, US.UNREACH6), (1, US.UNREACH6), (-1, US.NO_ROOM)):
        cut = 16 * ((UF.CHUNK - R - spare - 7) // 16)  # layout() cuts a multiple of 16; the frame's place takes the rest
        at = UF.CHUNK - cut - R - spare
        umem, descs = UF.layout([G.udp4_case()[0](()), f], [None, UF.CHUNK - at], short=cut)
        assert len(umem) - int(descs[1]["addr"]) == R + spare and 7 <= at < 23
        v = run(umem, descs, 2, OPTS, UF.table(), UF.N_PORTS, UF.BOUND)
        assert v == [US.UNREACH4, want]


@pytest.mark.parametrize("chunk", [2048, 4096, 1 << 20])
def test_chunk_sizes(chunk):
    """The same UMEM under larger chunks: a frame one byte short of room in a 2048-byte chunk has it in a larger one that
    does not end there (the byte it takes is the next slot's first, a sentinel here)."""
    sh = [s for s in shapes() if s[1] is not None][:24]  # eight shapes: fits to the byte, one byte short, one to spare
    assert [short for _, _, short in sh] == [False, True, False] * 8
    umem, descs = UF.layout([f for f, _, _ in sh], [r for _, r, _ in sh])
    v = run(umem, descs, len(sh), OPTS, UF.table(), UF.N_PORTS, UF.BOUND, chunk=chunk)
    # frame i ends at byte 2048 (i + 1): the end of a larger chunk only for some i (the short ones are i = 1, 4, 7, ...)
    assert v.count(US.NO_ROOM) == {2048: 8, 4096: 4, 1 << 20: 0}[chunk]


@pytest.mark.parametrize("open_ports", [None, frozenset({G.CLOSED}), frozenset(range(65536))])
def test_the_open_port_map_null_one_bit_and_all_bits(open_ports):
    umem, descs = batch()
    v = run(umem, descs, 257, OPTS, UF.table(), UF.N_PORTS, UF.BOUND, open_ports=open_ports)
    answered = v.count(US.UNREACH4) + v.count(US.UNREACH6)
    if open_ports is None:
        assert answered >= 64
    elif len(open_ports) == 1:
        assert 1 <= answered < 32 and US.LEFT in v  # traceroute's port is open now: only the probes of 53 and 4789 are due
    else:
        assert answered == 0 and US.LEFT in v


@pytest.mark.parametrize("n_entries", [0, 1, 1023, 1024])
def test_table_sizes(n_entries):
    from tests import neigh_frames as NF
    umem, descs = batch()
    table = NF.big_table(n_entries)
    v = run(umem, descs, 257, OPTS, table, UF.N_PORTS, UF.BOUND)
    answered = sum(x in US.REPLIES for x in v)
    assert answered == 0 if n_entries == 0 else answered >= 1


def test_descriptors_outside_the_umem():
    umem, descs = batch()
    d = descs[:70].copy()
    size = len(umem)
    d[10] = (size - 10, 60, 0)        # crosses the end
    d[11] = (size + 5, 60, 0)         # begins behind it
    d[12] = (size, 0, 0)              # empty, at the end
    d[13] = (0, (1 << 30) + 1, 0)     # longer than XSK_GPU_MAX_LEN
    d[14] = (0xFFFFFFFFFFFFFFF0, 64, 0)
    d[15] = (int(descs[20]["addr"]), 0xFFFFFFFF, 0)
    v = run(umem, d, 70, OPTS, UF.table(), UF.N_PORTS, UF.BOUND)
    assert v[10:16] == [US.NONE] * 6


def test_without_reply_lengths_and_counters():
    umem, descs = batch()
    run(umem, descs, 257, OPTS, UF.table(), UF.N_PORTS, UF.BOUND, rlen=False, stats=False)
    run(umem, descs, 65, OPTS, UF.table(), UF.N_PORTS, UF.BOUND, rlen=True, stats=False)


@pytest.mark.parametrize("n_ports,bound", [(1, US.ALL_BOUND), (64, US.ALL_BOUND), (8, US.ALL_BOUND & ~(1 << 3) & ~(1 << 0)),
                                           (64, 1 << 9), (8, 0)])
def test_port_counts_and_a_bound_word_with_holes(n_ports, bound):
    umem, descs = batch()
    v = run(umem, descs, 257, OPTS, UF.table(), n_ports, bound)
    if bound == 0:
        assert US.UNREACH4 not in v and US.UNREACH6 not in v
    else:
        assert US.UNREACH4 in v or US.UNREACH6 in v


@pytest.mark.parametrize("opts", UF.OPTS)
def test_the_golden_cases_under_every_option_word(opts):
    cases = UF.golden_frames(opts)
    umem, descs = UF.layout([f for f, _, _ in cases], [r for _, r, _ in cases])
    v = run(umem, descs, len(cases), opts, UF.table(), UF.N_PORTS, UF.BOUND)
    assert v == [want["verdict"] for _, _, want in cases]
