"""GPU parity of xsk_gpu_ingress_steer_dev (steering filter, then the indirect-count transform over the grouped list,
with no host round trip) against tests/steer_spec.spec_ingress_steer on the 4096-frame pipeline batch."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests import steer_spec as SS  # noqa: E402
from tests.test_gpu_ingress import _dev, same_dev, stats_of, to_dev  # noqa: E402
from tests.test_gpu_steer import dev_bound, dev_table  # noqa: E402
from tests.v6_frames import spec_batch  # noqa: E402

R = X.XDP_REDIRECT
N_PORTS, N_ENTRIES = 8, 64
BOUND = SS.ALL_BOUND & ~(1 << 5)  # port 5 unbound


class IngressSteer:
    """Device buffers of one ingress_steer_dev call over n frames, sentinels behind every output."""

    def __init__(self, d_umem, d_descs, n, d_table, n_entries, n_ports, d_bound):
        dev = _dev()
        self.n, self.umem, self.descs, self.n_ports = n, d_umem, d_descs, n_ports
        self.table, self.n_entries, self.bound = d_table, n_entries, d_bound
        self.act = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device=dev)
        self.ports = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device=dev)
        self.out = torch.full(((n + 4) * 16,), 0xEE, dtype=torch.uint8, device=dev)
        self.off = torch.full((n_ports + 1 + 2,), -1, dtype=torch.int32, device=dev)
        self.verd = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device=dev)
        self.recs = torch.full(((n + 4) * 16,), 0xEE, dtype=torch.uint8, device=dev)
        self.ws = torch.empty(X.steer_workspace_size(n, n_ports), dtype=torch.uint8, device=dev)

    def run(self, opts, default_port, stats):
        X.ingress_steer_dev(self.umem, self.descs, self.n, self.table, self.n_entries, default_port, self.n_ports,
                            self.bound, self.act, self.ports, self.out, self.off, self.verd, self.recs, stats, self.ws,
                            opts=opts)

    def check(self, d_after, ref):
        """Against a spec_ingress_steer result (d_after on the device).  Call after a synchronisation."""
        n, k = self.n, len(ref["out"])
        off = self.off.cpu().numpy().view(np.uint32)
        assert list(off[:self.n_ports + 1]) == list(ref["off"]) and int(off[self.n_ports]) == k
        assert (off[self.n_ports + 1:] == 0xFFFFFFFF).all()
        same_dev(self.act[:n], to_dev(ref["actions"]), "actions")
        same_dev(self.ports[:n], to_dev(ref["ports"]), "ports")
        assert bool((self.act[n:] == 0xEE).all()) and bool((self.ports[n:] == 0xEE).all())
        same_dev(self.out[:k * 16], to_dev(ref["out"]), "d_out")
        assert bool((self.out[k * 16:] == 0xEE).all())
        same_dev(self.verd[:k], to_dev(ref["verdicts"]), "verdicts by position in d_out")
        same_dev(self.recs[:k * 16], to_dev(ref["recs"]), "records by position in d_out")
        assert bool((self.verd[k:] == 0xEE).all()) and bool((self.recs[k * 16:] == 0xEE).all())
        same_dev(self.umem, d_after, "UMEM")


@functools.lru_cache(maxsize=None)
def pipeline_table(opts):
    umem, descs = IS.pipeline_batch()
    return SS.sample_table(SS.destinations(umem, descs, opts), N_ENTRIES, N_PORTS, seed=opts)


@functools.lru_cache(maxsize=None)
def pipeline_ingress_steer(opts, default_port, bound):
    umem, descs = IS.pipeline_batch()
    after = umem.copy()
    ref = SS.spec_ingress_steer(after, descs, opts, pipeline_table(opts), default_port, N_PORTS, bound)
    after.setflags(write=False)
    return after, ref


@pytest.mark.parametrize("default_port", [0, SS.PASS])
@pytest.mark.parametrize("opts", [0x17, 0x13])
def test_ingress_steer_matches_spec(opts, default_port):
    dev = _dev()
    umem, descs = IS.pipeline_batch()
    n = len(descs)
    after, ref = pipeline_ingress_steer(opts, default_port, BOUND)
    off, red = ref["off"].astype(np.int64), ref["actions"] == R
    k = int(off[N_PORTS])
    assert 0 < k < n and (np.diff(off) > 0).sum() >= (4 if default_port == 0 else 2) and off[5] == off[6]
    d_table, n_entries = dev_table(pipeline_table(opts))
    g = IngressSteer(to_dev(umem), to_dev(descs), n, d_table, n_entries, N_PORTS, dev_bound(BOUND))
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    g.run(opts, default_port, stats)
    torch.cuda.synchronize()
    g.check(to_dev(after), ref)
    st = stats_of(stats)
    assert st == ref["stats"]
    # the transform alone over the subset the spec redirects: spec_batch on those descriptors, in batch order
    alone = umem.copy()
    v_sub, _, s_sub = spec_batch(alone, np.ascontiguousarray(descs[red]), opts)
    assert (alone == after).all()
    assert st["tx_packets"] == s_sub["tx_packets"] > 0 and st["tx_bytes"] == s_sub["tx_bytes"]
    assert st["rx_packets"] == k == int(g.off.cpu().numpy().view(np.uint32)[N_PORTS])
    assert st["rx_bytes"] == int(descs["len"][red].astype(np.int64).sum())
    # port p's verdicts are the spec's verdicts of that port's frames, in batch order
    v_frame = np.full(n, 0xEE, np.uint8)
    v_frame[red] = v_sub
    verd = g.verd.cpu().numpy()
    for p in range(N_PORTS):
        idx = np.nonzero(red & (ref["ports"] == p))[0]
        assert len(idx) == off[p + 1] - off[p]
        assert (verd[off[p]:off[p + 1]] == v_frame[idx]).all(), p


@pytest.mark.parametrize("opts", [0x17, 0x13])
def test_everything_unbound_changes_nothing(opts):
    dev = _dev()
    umem, descs = IS.pipeline_batch()
    n = len(descs)
    after, ref = pipeline_ingress_steer(opts, 0, 0)
    assert len(ref["out"]) == 0 and (after == umem).all() and not any(ref["stats"].values())
    d_table, n_entries = dev_table(pipeline_table(opts))
    g = IngressSteer(to_dev(umem), to_dev(descs), n, d_table, n_entries, N_PORTS, dev_bound(0))
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    g.run(opts, 0, stats)
    torch.cuda.synchronize()
    g.check(to_dev(umem), ref)
    assert g.off.cpu().tolist()[:N_PORTS + 1] == [0] * (N_PORTS + 1)
    assert not any(stats_of(stats).values())
