"""What the GPU tests of xsk_gpu_responder_dev and xsk_gpu_responder_queues_dev share: the device leg (the fuzz suite's
Leg with the responder's record and the one call), hand-written worlds in loop_world's shape -- so that
loop_world.spec_round is the spec and Leg.hold the comparison -- and the three-way run: the new call, the fused call
followed by the serve call, the spec, from one initial state.  Every comparison is exact."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
import xsknet_amd as X  # noqa: E402
from tests import egress_ports_spec as EP  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests import loop_world as LW  # noqa: E402
from tests import neigh_frames as NF  # noqa: E402
from tests import neigh_spec as NS  # noqa: E402
from tests import steer_spec as SS  # noqa: E402
from tests.test_gpu_loop_fuzz import Leg, problems, same_bytes, snapshot  # noqa: E402,F401
from tests.test_gpu_neigh_serve import owners, ring  # noqa: E402
from tests.test_gpu_rx_step_dev import WRAP, to_dev  # noqa: E402
from tests.test_gpu_rx_step_steer_dev import make_state, pow2_at_least  # noqa: E402
from tests.test_gpu_tx_complete_rings import make_comps  # noqa: E402
from tests.wire_frames import G as WG  # noqa: E402

G = NF.G
CHUNK = LW.CHUNK
N_PORTS = 8
OWN = owners(N_PORTS)  # an IPv4 and an IPv6 address per port: 16 entries in the steering table and in the neighbour table
PEER4 = bytes([192, 0, 2, 77])


class RLeg(Leg):
    """Leg, with the serve call's two optional outputs passed or not, the struct xsk_gpu_responder_queue of what
    fused() passes, and the one call."""

    def __init__(self, w, umem=None, nres=True, nstats=True):
        super().__init__(w, umem)
        self.with_nres, self.with_nstats = nres, nstats

    def serve_args(self):
        return dict(nstats=self.nstats.data if self.with_nstats else None, nres=self.nres.data if self.with_nres else None)

    def serve(self):
        w, a = self.w, self.serve_args()
        X.neigh_serve_dev(self.umem.data, self.stack.view, self.views, self.up.view, w.serve_max,
                          self.neigh.data if self.neigh is not None else None, self.n_neigh, bound=self.bound,
                          nstats=a["nstats"], res=a["nres"], opts=w.opts)

    def responder_record(self, *_):
        return X.responder_queue(self.record(), self.up.view, self.w.serve_max,
                                 self.neigh.data if self.neigh is not None else None, self.n_neigh, **self.serve_args())

    def responder(self):
        self.rec = self.responder_record()
        X.responder_dev(self.rec, self.w.opts)


def responder_block(legs, opts):
    """The block of one xsk_gpu_responder_queues_dev call over `legs`, in device memory; the structs stay alive on it."""
    recs = [leg.responder_record() for leg in legs]
    host = X.responder_prepare(recs, opts)
    assert host.nbytes == X.responder_block_size(len(legs))
    d_block = to_dev(host)
    assert d_block.data_ptr() % 64 == 0
    d_block._keep = recs
    return d_block


# ---- frames ----------------------------------------------------------------------------------------------------------

def echo4(port, seq=0, tags=()):
    """An IPv4 echo request to port `port`'s address."""
    return WG.build(vlan=list(tags), daddr=OWN[2 * port][1], saddr=PEER4, seq=seq, payload=bytes(range(seq % 48)))


def who_has(port, tags=()):
    return G.arp_case(tpa_entry=OWN[2 * port])[0](tags)


def solicit(port, tags=()):
    return G.ns_case(target_entry=OWN[2 * port + 1])[0](tags)


def stranger(tags=()):
    return G.arp_case(tpa=G.STRANGER4)[0](tags)


# ---- a hand-written world --------------------------------------------------------------------------------------------

def hand_world(offer, backlog=(), *, opts=0x17, max_batch=64, rooms=None, tx_size=64, tx_prod=None, stack_size=64,
               stack_prod=WRAP + 7, up_size=64, up_used=0, up_prod=WRAP - 2, serve_max=64, n_comp=0, complete_max=64,
               outputs=True, rx_start=WRAP, n_ports=N_PORTS, later=()) -> LW.World:
    """`offer` (frames, as bytes) on the RX ring and `backlog` already on the stack ring, each frame in a 2048-B chunk of
    its own; 8 ports, every port's two addresses in both tables; TX ring p with rooms[p] free entries (default: all).
    `later` frames lie in the UMEM too, for the test to offer in later rounds: their descriptors are w.later."""
    frames = list(offer) + list(backlog) + list(later)
    n = len(frames)
    rng = np.random.default_rng(n + 977)
    w = LW.World()
    w.seed, w.fused, w.garbage = 0, True, False
    w.opts, w.max_batch, w.complete_max, w.n_ports, w.serve_max = opts, max_batch, complete_max, n_ports, serve_max
    w.default_port, w.bound = SS.PASS, None
    w.umem = rng.integers(0, 256, max(n, 1) * CHUNK, dtype=np.uint8)
    descs = np.zeros(n, oracle.DESC_DTYPE)
    for i, f in enumerate(frames):
        a = i * CHUNK + (0, 1, i % 16, 256)[i % 4]
        w.umem[a:a + len(f)] = np.frombuffer(f, np.uint8)
        descs[i] = (a, len(f), 0x1000 + i)
    own = OWN[:2 * n_ports]
    w.table = {SS.GS.key(addr): port for _, addr, port, _ in own}
    w.neigh = NF.table(own)
    n_offer = len(offer)
    size = pow2_at_least(max(n_offer, len(later)))
    w.rx, w.fill, _, w.pool = make_state(n_ports, size, rx_start, descs[:n_offer], size // 2, 5, 4 * size + 8,
                                         [0] * n_ports)
    rooms = [tx_size] * n_ports if rooms is None else rooms
    tx_prod = [WRAP + 3 * p + 1 for p in range(n_ports)] if tx_prod is None else tx_prod
    w.txs = [ring(tx_size, tx_prod[p], tx_size - rooms[p], seed=p) for p in range(n_ports)]
    w.stack = ring(stack_size, stack_prod, len(backlog), seed=5, items=descs[n_offer:n_offer + len(backlog)])
    w.later = descs[n_offer + len(backlog):]
    w.up = ring(up_size, up_prod, up_used, seed=99)
    w.comps = make_comps(n_comp, [64, 8], [3, 40]) if n_comp else []
    w.outputs = dict.fromkeys(LW.OUTPUTS, bool(outputs))
    w.offers = [descs[:n_offer]]
    w.stats = dict.fromkeys(IS.KEYS, 0)
    w.port_stats = [dict.fromkeys(EP.STATS_KEYS, 0) for _ in w.txs]
    w.nstats = dict.fromkeys(NS.STATS_KEYS, 0)
    w.round = 0
    return w


def expect_serve_outputs(leg: RLeg, r):
    """An optional output of the serve stage passed as NULL kept its bytes; what the spec expects is then written into the
    stand-in buffer, so that Leg.hold -- which knows no NULL there -- compares the rest."""
    if not leg.with_nres:
        assert bool((leg.nres.data == leg.nres.buf[0]).all()), "d_nres was passed as NULL and written"
        want = np.zeros(1, X.NEIGH_RESULT_DTYPE)
        for k in NS.RESULT_KEYS:
            want[0][k] = r["nres"][k]
        leg.nres.put(want.view(np.uint8))
    if not leg.with_nstats:
        assert not bool(leg.nstats.data.any()), "d_nstats was passed as NULL and written"
        want = np.zeros(1, X.NEIGH_STATS_DTYPE)
        for k in NS.STATS_KEYS:
            want[0][k] = leg.w.nstats[k]
        leg.nstats.put(want.view(np.uint8))


def three_ways(w: LW.World, nres=True, nstats=True, tag=""):
    """From the world's state: leg R makes the one call, leg C the fused call and then the serve call, the spec runs
    loop_world.spec_round on the world itself.  Each leg is held against the spec and the legs against each other byte
    for byte.  Returns (the spec's record of the round, leg R, leg C)."""
    legs = {"R": RLeg(w, nres=nres, nstats=nstats), "C": RLeg(w, nres=nres, nstats=nstats)}
    r = LW.spec_round(w)
    legs["R"].responder()
    legs["C"].fused()
    torch.cuda.synchronize()
    wrong = []
    for name, leg in legs.items():
        wrong += problems(f"leg {name}: the serve stage's NULL outputs", expect_serve_outputs, leg, r)
        wrong += problems(f"leg {name}", leg.hold, r)
    wrong += problems("leg R against leg C", same_bytes, legs["C"], legs["R"])
    assert not wrong, f"{tag}: " + " | ".join(wrong)
    return r, legs["R"], legs["C"]
