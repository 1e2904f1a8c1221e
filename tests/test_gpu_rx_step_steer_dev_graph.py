"""xsk_gpu_rx_step_steer_dev captured once and replayed: a whole steered RX loop iteration -- peek, refill, pad, steer,
transform, per-port lists, three TX rings, pool, release -- with nothing frozen into the capture but pointers, sizes and
the bound.  Every index, count, table entry and the bound mask is device memory that the replay reads when it executes;
the test plays the peer between replays by device copies (new RX entries and producer word, the TX and fill consumer
words) and rewrites the table entries and *d_bound in place.  One linear chain on the capture stream: no parallel
branches."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import egress_ports_spec as EP  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests import rx_dev_spec as RS  # noqa: E402
from tests import rx_steer_spec as RP  # noqa: E402
from tests import steer_spec as SS  # noqa: E402
from tests.test_gpu_ingress import _dev, stats_of, to_dev  # noqa: E402
from tests.test_gpu_rx_step_dev import WRAP  # noqa: E402
from tests.test_gpu_rx_step_steer_dev import SteerState, _table, _traffic, make_state, port_stats_of  # noqa: E402

SIZE, MAX_BATCH, OPTS, N_PORTS = 64, 48, 0x17, 3
EMPTY, FULL = 2, 4  # the replay that meets an empty RX ring, and the one that meets a full TX ring on port 0
OFFERS = [40, 48, 0, 55, 33, 41]  # frames the peer puts on the RX ring before each replay (55 > max_batch: 7 stay)
BOUNDS = [SS.ALL_BOUND, SS.ALL_BOUND & ~2, SS.ALL_BOUND, SS.ALL_BOUND & ~4, SS.ALL_BOUND, 1]


def test_one_capture_replayed_six_times_with_the_table_rewritten_in_place():
    _dev()
    umem, descs = _traffic(sum(OFFERS))
    base = _table(sum(OFFERS), OPTS, N_PORTS, entries=94)  # half of the batch's destinations
    keys = list(base)
    rx, fill, txs, pool = make_state(N_PORTS, SIZE, WRAP - 20, descs[:0], SIZE // 2, SIZE, 3 * SIZE, [4096] * N_PORTS)
    d = SteerState(rx, fill, txs, pool, MAX_BATCH, base, SS.ALL_BOUND)
    d_umem = to_dev(umem)
    # outside the capture first: the library's kernels are loaded, the device is known (an empty ring: nothing changes)
    d.step(d_umem, OPTS, 0)
    torch.cuda.synchronize()
    d.check(rx, fill, txs, pool)
    d.stats.zero_()
    d.port_stats.data.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d.step(d_umem, OPTS, 0)
    s = [rx.copy(), fill.copy(), [t.copy() for t in txs], pool.copy()]
    u = umem.copy()
    st = dict.fromkeys(IS.KEYS, 0)
    pst = [dict.fromkeys(EP.STATS_KEYS, 0) for _ in txs]
    taken, slots_seen, tables = 0, set(), []
    for k, offer in enumerate(OFFERS):
        # the peer
        s[0].produce(descs[taken:taken + offer])
        taken += offer
        assert s[0].used() <= SIZE
        for p, t in enumerate(s[2]):  # port 0's ring full once, every other ring drained
            t.cons = (t.prod - t.size) & RS.M32 if (k == FULL and p == 0) else t.prod
        s[1].cons = (s[1].cons + min(s[1].used(), 30)) & RS.M32  # the kernel took fill entries
        d.rx.write(s[0])
        d.fill.write(s[1])
        for t, dt in zip(s[2], d.txs):
            dt.write(t)
        # the control plane: the same keys, every port redrawn; the bound mask changed -- both in place
        rng = np.random.default_rng(k)
        table = {key: int(rng.integers(0, N_PORTS)) for key in keys}
        tables.append(tuple(table.values()))
        e = X.steer_table_prepare(SS.entries_of(table))
        assert len(e) == d.n_entries
        d.table.copy_(to_dev(e))
        d.bound.copy_(torch.from_numpy(np.array([BOUNDS[k]], np.uint64).view(np.int64)))
        first, avail = s[0].cons, s[0].used()
        got = RP.spec_step_steer(u, s[0], s[1], s[2], s[3], MAX_BATCH, OPTS, table, 0, BOUNDS[k], st, pst)
        res = got["result"]
        graph.replay()
        torch.cuda.synchronize()
        d.check(*s)
        d.check_outputs(got)
        assert d.result() == res and stats_of(d.stats) == st and port_stats_of(d.port_stats, N_PORTS) == pst, k
        assert res["received"] == min(avail, MAX_BATCH)
        slots_seen |= {(first + i) & (SIZE - 1) for i in range(res["received"])}
        off = [int(x) for x in got["off"]]
        if k == EMPTY:
            assert res == dict.fromkeys(RP.RESULT_KEYS, 0)
        elif k == FULL:
            assert off[1] - off[0] >= 3 and got["counts"][0]["n_tx"] == 0 and got["counts"][0]["n_tx_full"] >= 1
            assert res["replied"] >= 1 and res["tx_full"] == got["counts"][0]["n_tx_full"]
        else:
            assert res["replied"] >= 3
        if BOUNDS[k] != SS.ALL_BOUND and k != EMPTY:
            unbound = [p for p in range(N_PORTS) if not BOUNDS[k] >> p & 1]
            assert all(off[p + 1] == off[p] for p in unbound) and (got["actions"] == SS.XDP_DROP).any()
    assert len(set(tables)) == len(OFFERS)  # every replay steered by another table
    assert (d_umem.cpu().numpy() == u).all()
    assert slots_seen == set(range(SIZE)) and s[0].cons < 1000  # every slot used, the words wrapped past 2^32
    assert st["rx_packets"] < sum(OFFERS) - s[0].used()  # the counters count the redirected frames only
