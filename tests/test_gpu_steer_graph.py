"""xsk_gpu_ingress_steer_dev captured once in a graph on one stream and replayed after the bound word, the table's
entries and the frames changed in device memory: the bound word and the table are read when the kernels execute, so
every replay must match the spec of what device memory held then.  The capture is one linear chain (classify, scan,
scatter, transform)."""
import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests import steer_spec as SS  # noqa: E402
from tests.test_gpu_ingress import STRIDE, _dev, stats_of, to_dev  # noqa: E402
from tests.test_gpu_ingress_steer import N_ENTRIES, N_PORTS, IngressSteer, pipeline_table  # noqa: E402
from tests.test_gpu_steer import dev_bound  # noqa: E402
from tests.v6_frames import mixed_batch6  # noqa: E402

OPTS = 0x17


def test_graph_replay_reads_bound_table_and_frames_at_replay():
    dev = _dev()
    umem_a, descs = IS.pipeline_batch()
    n = len(descs)
    umem_b, descs_b = mixed_batch6(n, STRIDE, seed=9019, offsets=True)
    descs_b = np.ascontiguousarray(descs_b, oracle.DESC_DTYPE)
    assert umem_b.size == umem_a.size
    table_1 = pipeline_table(OPTS)
    # the second table: the same number of entries (the count is an argument, frozen by the capture), other keys, other
    # ports -- drawn from both batches' destinations
    keys = SS.destinations(umem_a, descs, OPTS)[1:120:2] + SS.destinations(umem_b, descs_b, OPTS)
    table_2 = SS.sample_table(keys, N_ENTRIES, N_PORTS, seed=77)
    assert len(table_1) == len(table_2) == N_ENTRIES and table_1 != table_2
    e1 = X.steer_table_prepare(SS.entries_of(table_1))
    e2 = X.steer_table_prepare(SS.entries_of(table_2))
    bound_1, bound_2 = SS.ALL_BOUND, SS.ALL_BOUND & ~((1 << 1) | (1 << 3))
    # what device memory holds at each replay: (umem, descs, table, entries, bound)
    steps = [(umem_a, descs, table_1, e1, bound_1),
             (umem_a, descs, table_1, e1, bound_2),     # *d_bound changed
             (umem_a, descs, table_2, e2, bound_2),     # the entries overwritten in place
             (umem_b, descs_b, table_2, e2, bound_2),   # other frames
             (umem_b, descs_b, table_2, e2, 0)]         # everything unbound
    refs = []
    for um, de, table, _, bound in steps:
        after = um.copy()
        refs.append((after, SS.spec_ingress_steer(after, de, OPTS, table, 0, N_PORTS, bound)))
    offs = [list(r["off"]) for _, r in refs]
    assert all(offs[i] != offs[i + 1] for i in range(len(offs) - 1)) and offs[-1] == [0] * (N_PORTS + 1)
    for o in offs[:-1]:  # conditions of the input: every replay but the last spreads frames over several ports
        assert (np.diff(np.array(o, np.int64)) > 0).sum() >= 3
    d_table, d_bound = to_dev(e1), dev_bound(bound_1)
    g = IngressSteer(to_dev(umem_a), to_dev(descs), n, d_table, N_ENTRIES, N_PORTS, d_bound)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    g.run(OPTS, 0, stats)  # outside the capture first: the library's kernels are loaded, the device is known
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.run(OPTS, 0, stats)
    for (um, de, _, entries, bound), (after, ref) in zip(steps, refs):
        g.umem.copy_(to_dev(um))
        g.descs.copy_(to_dev(de))
        d_table.copy_(to_dev(entries))
        d_bound.copy_(dev_bound(bound))
        for t in (g.act, g.ports, g.out, g.verd, g.recs):
            t.fill_(0xEE)
        g.off.fill_(-1)
        stats.zero_()
        graph.replay()
        torch.cuda.synchronize()
        g.check(to_dev(after), ref)
        assert stats_of(stats) == ref["stats"]
