"""xsk_gpu_ingress_dev_opts + xsk_gpu_egress_dev captured in one graph and replayed: the whole device pipeline, raw
traffic in, TX and free lists out, with nothing frozen into the capture but pointers -- the frame count comes from the
filter's *d_nout and the TX ring's room from a device word the caller rewrites between replays.  One linear chain on the
capture stream (filter, scan, scatter, transform, then egress' count, scan, scatter): no parallel branches."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import egress_spec as ES  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests.test_gpu_egress import SENT  # noqa: E402
from tests.test_gpu_ingress import Ingress, _dev, same_dev, stats_of, to_dev  # noqa: E402
from tests.test_gpu_ingress_graph import OPTS, _batches  # noqa: E402


def test_graph_replay_builds_the_lists_of_each_replay():
    dev = _dev()
    batches = _batches()  # none, all, some frames redirected
    n = len(batches[0][1])
    refs = []
    for umem, descs in batches:
        after = umem.copy()
        refs.append((after, IS.spec_ingress(after, descs, OPTS, True)))
    assert [r["nout"] for _, r in refs][:2] == [0, n] and 0 < refs[2][1]["nout"] < n  # conditions of the input
    replies = [int((r["verdicts"] == IS.TX_REPLY).sum()) for _, r in refs]
    assert replies[0] == 0 and replies[1] > 2 and replies[2] > 2
    rooms = [7, replies[1] // 2, ES.UNLIMITED]  # the second replay's room lies below its R
    staged = [(to_dev(u), to_dev(d), to_dev(a)) for (u, d), (a, _) in zip(batches, refs)]
    g = Ingress(staged[2][0].clone(), staged[2][1].clone(), n)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    d_tx = torch.full(((n + 4) * 16,), SENT, dtype=torch.uint8, device=dev)
    d_free = torch.full(((n + 4) * 8,), SENT, dtype=torch.uint8, device=dev)
    d_counts = torch.full((32,), SENT, dtype=torch.uint8, device=dev)
    d_room = torch.zeros(1, dtype=torch.int32, device=dev)
    ews = torch.empty(X.egress_workspace_size(n), dtype=torch.uint8, device=dev)

    def pipeline():
        g.run(OPTS, True, stats)
        X.egress_dev(g.out, g.verd, n, d_tx, d_free, d_counts[:16], count=g.nout, tx_room=d_room, stats=stats,
                     workspace=ews)

    pipeline()  # outside the capture first: the library's kernels are loaded, the device is known
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pipeline()
    for (d_umem, d_descs, d_after), (_, ref), room in zip(staged, refs, rooms):
        g.umem.copy_(d_umem)
        g.descs.copy_(d_descs)
        for t in (g.act, g.out, g.verd, g.recs, d_tx, d_free, d_counts):
            t.fill_(SENT)
        g.nout.fill_(-1)
        stats.zero_()
        d_room.fill_(int(np.uint32(room).astype(np.int32)))  # rewritten between replays
        graph.replay()
        torch.cuda.synchronize()
        g.check(d_after, ref["actions"], ref["out"], ref["verdicts"], ref["recs"])
        k = ref["nout"]
        tx, free, c, dp, db = ES.spec_egress(ref["out"], ref["verdicts"], k, room)
        assert ES.counts_of(d_counts[:16].cpu().numpy()) == c and bool((d_counts[16:] == SENT).all())
        same_dev(d_tx[:c["n_tx"] * 16], to_dev(tx), "d_tx")
        same_dev(d_free[:c["n_free"] * 8], to_dev(free), "d_free")
        assert bool((d_tx[c["n_tx"] * 16:] == SENT).all()) and bool((d_free[c["n_free"] * 8:] == SENT).all())
        want = dict(ref["stats"])
        want["tx_packets"] += dp
        want["tx_bytes"] += db
        assert stats_of(stats) == want
    assert rooms[1] < replies[1]  # a condition of the input: the second replay took replies back out of the counters
