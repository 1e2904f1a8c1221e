"""xsk_gpu_ingress_steer_dev + xsk_gpu_egress_ports_dev captured once in a graph on one stream -- one linear chain, the
workspaces preallocated -- and replayed after the bound word, the room words and the frames changed in device memory:
the offsets, the rooms and the verdicts are read when the kernels execute, so every replay must match the specs of what
device memory held then."""
import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import egress_ports_spec as EP  # noqa: E402
from tests import egress_spec as ES  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests import steer_spec as SS  # noqa: E402
from tests.test_gpu_egress_ports import KEYS, SENT, _Rs, _words  # noqa: E402
from tests.test_gpu_ingress import STRIDE, _dev, same_dev, stats_of, to_dev  # noqa: E402
from tests.test_gpu_ingress_steer import N_ENTRIES, N_PORTS, IngressSteer, pipeline_table  # noqa: E402
from tests.test_gpu_steer import dev_bound  # noqa: E402
from tests.v6_frames import mixed_batch6  # noqa: E402

OPTS = 0x17
UNL = 0xFFFFFFFF


def _all_redirected(umem, descs, red):
    """A batch of len(descs) frames, every one a copy of a redirected frame of (umem, descs), each in its own slot."""
    n = len(descs)
    idx = np.nonzero(red)[0]
    assert len(idx) > 100
    um = np.zeros_like(umem)
    de = np.zeros(n, oracle.DESC_DTYPE)
    for i in range(n):
        s = descs[idx[i % len(idx)]]
        a, ln = int(s["addr"]), int(s["len"])
        assert a // STRIDE == (a + ln - 1) // STRIDE  # a frame lies inside one slot
        na = i * STRIDE + a % STRIDE
        um[na:na + ln] = umem[a:a + ln]
        de[i] = (na, ln, s["options"])
    return um, de


def test_graph_replay_reads_bound_rooms_and_frames_at_replay():
    dev = _dev()
    umem_a, descs = IS.pipeline_batch()
    n = len(descs)
    table = pipeline_table(OPTS)
    entries = X.steer_table_prepare(SS.entries_of(table))
    bound_1 = SS.ALL_BOUND & ~(1 << 5)
    bound_2 = bound_1 & ~(1 << 2)
    first = SS.spec_ingress_steer(umem_a.copy(), descs, OPTS, table, 0, N_PORTS, bound_1)
    R1 = _Rs(first["verdicts"], [int(x) for x in first["off"]])
    assert R1[2] > 1 and R1[0] > 100
    umem_b, descs_b = mixed_batch6(n, STRIDE, seed=9019, offsets=True)
    descs_b = np.ascontiguousarray(descs_b, oracle.DESC_DTYPE)
    umem_c, descs_c = _all_redirected(umem_a, descs, first["actions"] == X.XDP_REDIRECT)
    umem_0 = np.zeros_like(umem_a)
    assert umem_b.size == umem_a.size == umem_c.size
    cut = [R // 2 for R in R1]
    # what device memory holds at each replay: (umem, descs, bound, rooms)
    steps = [(umem_a, descs, bound_1, [UNL] * N_PORTS),
             (umem_a, descs, bound_2, [UNL] * N_PORTS),            # a port unbound: its segment becomes empty
             (umem_a, descs, bound_2, cut),                        # the room words changed: below R_p
             (umem_0, descs, bound_2, cut),                        # the frames changed: none redirected
             (umem_c, descs_c, SS.ALL_BOUND, [7, UNL, 0, 3, 1, 2, UNL, 0]),   # all redirected
             (umem_b, descs_b, bound_1, [UNL, 1, 0, UNL, 2, 0, 1, UNL])]      # some
    refs = []
    for um, de, bound, rooms in steps:
        after = um.copy()
        ref = SS.spec_ingress_steer(after, de, OPTS, table, 0, N_PORTS, bound)
        off = [int(x) for x in ref["off"]]
        k = off[N_PORTS]
        out_n = np.zeros(n, X.DESC_DTYPE)
        out_n[:k] = ref["out"]
        verd_n = np.full(n, SENT, np.uint8)
        verd_n[:k] = ref["verdicts"]
        refs.append((after, ref, EP.spec_egress_ports(out_n, verd_n, off, N_PORTS, n, rooms)))
    # conditions of the input
    o = [r["off"].tolist() for _, r, _ in refs]
    assert o[0][2] < o[0][3] and o[1][2] == o[1][3]                        # port 2's segment becomes empty
    assert sum(c["n_tx_full"] for c in refs[1][2]["counts"]) == 0 < sum(c["n_tx_full"] for c in refs[2][2]["counts"])
    assert o[3] == [0] * (N_PORTS + 1)                                     # none redirected
    assert o[4][N_PORTS] == n and (np.diff(np.array(o[4], np.int64)) > 0).sum() >= 3   # all redirected
    assert 0 < o[5][N_PORTS] < n and o[5] != o[0]                          # some

    d_bound = dev_bound(bound_1)
    d_rooms = _words([UNL] * N_PORTS)
    g = IngressSteer(to_dev(umem_a), to_dev(descs), n, to_dev(entries), N_ENTRIES, N_PORTS, d_bound)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    d_ps = torch.zeros(40 * N_PORTS, dtype=torch.uint8, device=dev)
    d_tx = torch.full(((n + 4) * 16,), SENT, dtype=torch.uint8, device=dev)
    d_free = torch.full(((n + 4) * 8,), SENT, dtype=torch.uint8, device=dev)
    d_counts = torch.full((N_PORTS * 16 + 16,), SENT, dtype=torch.uint8, device=dev)
    ws = torch.empty(X.egress_ports_workspace_size(n, N_PORTS), dtype=torch.uint8, device=dev)

    def chain():
        g.run(OPTS, 0, stats)
        X.egress_ports_dev(g.out, g.verd, g.off, N_PORTS, n, d_tx, d_free, d_counts[:N_PORTS * 16], tx_room=d_rooms,
                           stats=stats, port_stats=d_ps, workspace=ws)

    chain()  # outside the capture first: the library's kernels are loaded, the device is known
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for (um, de, bound, rooms), (after, ref, sp) in zip(steps, refs):
        g.umem.copy_(to_dev(um))
        g.descs.copy_(to_dev(de))
        d_bound.copy_(dev_bound(bound))
        _words(rooms, d_rooms)
        for t in (g.act, g.ports, g.out, g.verd, g.recs, d_tx, d_free, d_counts):
            t.fill_(SENT)
        g.off.fill_(-1)
        stats.zero_()
        d_ps.zero_()
        graph.replay()
        torch.cuda.synchronize()
        g.check(to_dev(after), ref)
        cb = d_counts.cpu().numpy()
        assert [ES.counts_of(cb[16 * p:16 * p + 16]) for p in range(N_PORTS)] == sp["counts"]
        assert (cb[N_PORTS * 16:] == SENT).all()
        tx, free = EP.expected_arrays(sp, n, SENT, 4)
        same_dev(d_tx, to_dev(tx), "d_tx")
        same_dev(d_free, to_dev(free), "d_free")
        want = dict(ref["stats"])
        want["tx_packets"] += sp["d_tx_packets"]
        want["tx_bytes"] += sp["d_tx_bytes"]
        assert stats_of(stats) == want
        got = d_ps.cpu().numpy().view(X.STATS_DTYPE)
        for p in range(N_PORTS):
            assert {k: int(got[k][p]) for k in KEYS} == sp["port_stats"][p], p
        assert (got["timestamp"] == 0).all()
