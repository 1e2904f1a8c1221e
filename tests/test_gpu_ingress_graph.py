"""xsk_gpu_ingress_dev_opts captured in a graph and replayed over batches with different REDIRECT counts: the case a
transform that takes its frame count from the host cannot serve, because a captured launch freezes its arguments.  The
capture is one linear chain on the capture stream (filter, scan, scatter, transform)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import ingress_spec as IS  # noqa: E402
from tests.test_gpu_ingress import STRIDE, Ingress, _dev, stats_of, to_dev  # noqa: E402

OPTS = 0x17


def _batches():
    """Three batches of 4096 frames in UMEMs of one size: none redirected, all redirected, mixed."""
    umem, descs = IS.pipeline_batch()
    _, ref = IS.pipeline_ingress(OPTS, True)
    n, k = len(descs), ref["nout"]
    nothing = np.zeros_like(umem)  # ethertype 00 00: every frame is PASS
    everything, d_all = umem.copy(), descs.copy()
    for i in range(n):  # slot i holds a copy of a redirected frame, at that frame's offset in its slot
        s = ref["out"][i % k]
        a, L = int(s["addr"]), int(s["len"])
        b = i * STRIDE + a % STRIDE
        everything[b:b + L] = umem[a:a + L]
        d_all[i] = (b, L, 0)
    return [(nothing, descs), (everything, d_all), (umem, descs)]


def test_graph_replay_serves_the_count_of_each_replay():
    dev = _dev()
    batches = _batches()
    n = len(batches[0][1])
    refs = []
    for umem, descs in batches:
        after = umem.copy()
        refs.append((after, IS.spec_ingress(after, descs, OPTS, True)))
    assert [r["nout"] for _, r in refs][:2] == [0, n] and 0 < refs[2][1]["nout"] < n  # conditions of the input
    staged = [(to_dev(u), to_dev(d), to_dev(a)) for (u, d), (a, _) in zip(batches, refs)]
    g = Ingress(staged[2][0].clone(), staged[2][1].clone(), n)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    g.run(OPTS, True, stats)  # outside the capture first: the library's kernels are loaded, the device is known
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.run(OPTS, True, stats)
    for (d_umem, d_descs, d_after), (_, ref) in zip(staged, refs):
        g.umem.copy_(d_umem)
        g.descs.copy_(d_descs)
        for t in (g.act, g.out, g.verd, g.recs):
            t.fill_(0xEE)
        g.nout.fill_(-1)
        stats.zero_()
        graph.replay()
        torch.cuda.synchronize()
        g.check(d_after, ref["actions"], ref["out"], ref["verdicts"], ref["recs"])
        assert stats_of(stats) == ref["stats"]
