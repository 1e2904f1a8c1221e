"""xsk_gpu_rx_step_dev captured once and replayed: a whole RX loop iteration -- peek, refill, transform, lists, TX ring,
pool, release -- with nothing frozen into the capture but pointers, sizes and the bound.  Every index and count is a
word in device memory that the replay reads when it executes; the test plays the peer between replays by device copies
(new RX entries and producer word, the TX and fill consumer words).  One linear chain on the capture stream: no parallel
branches."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import ingress_spec as IS  # noqa: E402
from tests import rx_dev_spec as RS  # noqa: E402
from tests.test_gpu_ingress import _dev, stats_of, to_dev  # noqa: E402
from tests.test_gpu_rx_step_dev import WRAP, DevState, _traffic, make_state  # noqa: E402

SIZE, MAX_BATCH, OPTS = 64, 48, 0x17
EMPTY, FULL = 2, 4  # the replay that meets an empty RX ring, and the one that meets a full TX ring
OFFERS = [40, 48, 0, 55, 33, 41]  # frames the peer puts on the RX ring before each replay (55 > max_batch: 7 stay)


def test_one_capture_replayed_six_times_wraps_the_ring():
    _dev()
    umem, descs = _traffic(sum(OFFERS))
    rx, fill, tx, pool, _ = make_state(SIZE, WRAP - 20, descs[:0], SIZE // 2, SIZE, SIZE)
    d = DevState(rx, fill, tx, pool, MAX_BATCH)
    d_umem = to_dev(umem)
    # outside the capture first: the library's kernels are loaded, the device is known (an empty ring: nothing changes)
    d.step(d_umem, OPTS)
    torch.cuda.synchronize()
    d.check(rx, fill, tx, pool)
    d.stats.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d.step(d_umem, OPTS)
    s = [x.copy() for x in (rx, fill, tx, pool)]
    u = umem.copy()
    st = dict.fromkeys(IS.KEYS, 0)
    taken, slots_seen = 0, set()
    for k, offer in enumerate(OFFERS):
        # the peer
        s[0].produce(descs[taken:taken + offer])
        taken += offer
        assert s[0].used() <= SIZE
        s[2].cons = (s[2].prod - SIZE) & RS.M32 if k == FULL else s[2].prod  # a full TX ring, or a drained one
        s[1].cons = (s[1].cons + min(s[1].used(), 30)) & RS.M32                # the kernel took fill entries
        d.rx.write(s[0])
        d.tx.write(s[2])
        d.fill.write(s[1])
        first, avail = s[0].cons, s[0].used()
        res = RS.spec_step(u, *s, MAX_BATCH, OPTS, st)
        graph.replay()
        torch.cuda.synchronize()
        d.check(*s)
        assert d.result() == res and stats_of(d.stats) == st, k
        assert res["received"] == min(avail, MAX_BATCH)
        slots_seen |= {(first + i) & (SIZE - 1) for i in range(res["received"])}
        if k == EMPTY:
            assert res == dict(received=0, replied=0, tx_full=0, refilled=0)
        if k == FULL:
            assert res["received"] > 0 and res["replied"] == 0 and res["tx_full"] >= 3
        elif k != EMPTY:
            assert res["replied"] >= 3 and res["tx_full"] == 0
    assert (d_umem.cpu().numpy() == u).all()
    assert slots_seen == set(range(SIZE)) and s[0].cons < 1000  # every slot used, the words wrapped past 2^32
    assert st["rx_packets"] == sum(OFFERS) - s[0].used()
