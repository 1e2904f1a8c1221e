"""GPU parity of xsk_gpu_echo_dev_indirect (the transform whose frame count is a word in device memory) and of
xsk_gpu_ingress_dev_opts (filter, then that transform, with no host round trip) against the specs of
tests/ingress_spec.py.  Nothing here passes a frame count from the host: counts are written by a device-side fill
enqueued on the same stream, or by the filter itself."""
import functools

import numpy as np
import pytest

import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import xsknet_amd as X  # noqa: E402
from tests import ingress_spec as IS  # noqa: E402
from tests.v6_frames import mixed_batch6  # noqa: E402

KEYS = IS.KEYS
STRIDE = 2048


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def to_dev(a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(_dev())


def stats_of(t):
    s = t.cpu().numpy().view(X.STATS_DTYPE)[0]
    return {k: int(s[k]) for k in KEYS}


def same_dev(got, ref, what):
    """Two uint8 device tensors are equal (compared on the device, the first differences reported)."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = torch.nonzero(got != ref).flatten()[:8].cpu().numpy()
        raise AssertionError(f"{what}: differs, first at {bad}, got {got[bad].cpu().numpy()}, "
                             f"want {ref[bad].cpu().numpy()}")


# ---- the indirect transform --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _indirect_ref(opts):
    """A 4099-frame mixed batch, frame i inside [i * STRIDE, (i + 1) * STRIDE), and the transform's result over all of
    it, on the device: (descs, pristine UMEM, UMEM after, verdicts, records)."""
    n = 4099
    if opts:
        umem, descs = mixed_batch6(n, STRIDE, seed=4099 + opts, offsets=True)
        descs = np.ascontiguousarray(descs, oracle.DESC_DTYPE)
    else:
        umem = np.zeros(n * STRIDE, np.uint8)
        descs = oracle.synth_batch(umem, n, 0, STRIDE, seed=0x5EED4099, mode=1, len_lo=20, len_hi=1500)
    assert (descs["addr"] // STRIDE == np.arange(n)).all()
    assert ((descs["addr"] % STRIDE) + np.maximum(descs["len"], 38) <= STRIDE).all()
    after = umem.copy()
    v, r, st = IS.spec_transform(after, descs, opts)
    assert st == IS.prefix_stats(descs, v, n) and 0 < st["tx_packets"] < n  # the prefix rule, and a mixed batch
    assert (after != umem).any()
    return descs, to_dev(umem), to_dev(after), v, r


COUNTS = [(4099, c) for c in (0, 1, 63, 64, 65, 1024, 1025, 4098, 4099, 4106)] + \
         [(64, c) for c in (0, 1, 64)] + [(1, c) for c in (0, 1)]


@pytest.mark.parametrize("n_max,count", COUNTS)
@pytest.mark.parametrize("opts", [0, 7, 0x17])
def test_indirect_transform(opts, n_max, count):
    """The first min(count, n_max) descriptors are transformed as the direct call transforms them; verdicts and records
    at or above that keep their sentinel, frames of descriptors at or above it their bytes.  4106 > n_max shows the
    clamp; n_max of 64 and 1 run on the 64-frame-tile kernel too."""
    dev = _dev()
    descs, d_orig, d_after, v_ref, r_ref = _indirect_ref(opts)
    n = min(count, n_max)
    d_umem = d_orig.clone()
    d_descs = to_dev(descs[:n_max])
    verd = torch.full((n_max + 64,), 0xEE, dtype=torch.uint8, device=dev)
    recs = torch.full(((n_max + 4) * 16,), 0xEE, dtype=torch.uint8, device=dev)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    cnt.fill_(count)  # a fill kernel on the current stream: the count exists only on the device
    X.echo_dev_indirect(d_umem, d_descs, cnt, n_max, verd, recs, stats, opts=opts)
    torch.cuda.synchronize()
    assert int(cnt.cpu()[0]) == count
    cut = n * STRIDE
    same_dev(d_umem[:cut], d_after[:cut], "frames below n")
    same_dev(d_umem[cut:], d_orig[cut:], "frames at or above n")
    v, r = verd.cpu().numpy(), recs.cpu().numpy().reshape(-1, 16)
    bad = np.nonzero(v[:n] != v_ref[:n])[0]
    assert len(bad) == 0, (bad[:5], v[bad[:5]], v_ref[bad[:5]], descs[bad[:5]])
    bad = np.nonzero((r[:n] != r_ref[:n]).any(axis=1))[0]
    assert len(bad) == 0, (bad[:3], r[bad[:3]], r_ref[bad[:3]], descs[bad[:3]])
    assert (v[n:] == 0xEE).all() and (r[n:] == 0xEE).all()
    assert stats_of(stats) == IS.prefix_stats(descs, v_ref, n)


# ---- the piece rule ----------------------------------------------------------------------------------------------

def six_mask(frames: np.ndarray, lens: np.ndarray, opts: int) -> np.ndarray:
    """tests/golden/make_v6_golden.v6_l3 over n frames at once (frames: n x stride bytes, stride >= 24): True where the
    inner ethertype, behind up to two VLAN tags under XSK_GPU_OPT_VLAN, none cut by the frame's end, is 0x86DD."""
    be = lambda i: (frames[:, i].astype(np.uint32) << 8) | frames[:, i + 1]  # noqa: E731
    lens = lens.astype(np.int64)
    alive = lens >= 14
    et = be(12)
    for l3 in ((14, 18) if opts & X.OPT_VLAN else ()):  # (untagged at 14: untagged at 18)
        tagged = alive & ((et == 0x8100) | (et == 0x88A8))
        alive &= ~(tagged & (lens < l3 + 4))
        et = np.where(tagged & alive, be(l3 + 2), et)
    return alive & (et == 0x86DD)


@pytest.mark.parametrize("opts", [0, 7, 0x17])
def test_indirect_piece_rule(opts):
    """A bound of 4 rounds per workgroup plus one tile runs as consecutive launches, each taking its slice of the count:
    64-B frames at a 64-B stride against the C oracle, with the count at the bound and in the middle piece; in
    reference mode, in wire mode and on the dual-stack kernel (0x17: IPv4 traffic only, the generator's 0x86DD frames
    emptied to len 0, so that the C oracle's wire mode is the reference)."""
    from tests.v6_frames import G6
    dev = _dev()
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    n_max = ncu * 32 * 64 * 4 + 64
    thr = oracle.cpu_threads()
    umem = np.zeros(n_max * 64, np.uint8)
    descs = oracle.synth_batch(umem, n_max, 0, 64, seed=0x5EED71EC, mode=1, len_lo=64, len_hi=64, threads=thr)
    if opts & 0x10:
        six = six_mask(umem.reshape(n_max, 64), descs["len"], opts)
        for i in range(0, n_max, 509):  # the vectorised rule is the spec's, on a sample and on every frame it found
            f = umem[i * 64:i * 64 + 64].tobytes()
            assert bool(six[i]) == (G6.v6_l3(f, int(descs[i]["len"]), opts) is not None)
        for i in np.nonzero(six)[0][:2000]:
            assert G6.v6_l3(umem[i * 64:i * 64 + 64].tobytes(), int(descs[i]["len"]), opts) is not None
        descs["len"][six] = 0
    assert (descs["addr"] == np.arange(n_max, dtype=np.uint64) * 64).all() and (descs["len"] <= 64).all()
    after = umem.copy()
    if opts:
        v_ref, r_ref, _ = oracle.echo_batch_opts(after, descs, opts & 7, threads=thr)
    else:
        v_ref, r_ref, _ = oracle.echo_batch(after, descs, threads=thr)
    r_ref = r_ref.view(np.uint8).reshape(-1, 16)
    d_orig, d_after, d_descs = to_dev(umem), to_dev(after), to_dev(descs)
    d_v, d_r = to_dev(v_ref), to_dev(r_ref)
    assert 0 < int((v_ref == IS.TX_REPLY).sum()) < n_max
    for count in (n_max, n_max // 2 + 1):
        d_umem = d_orig.clone()
        verd = torch.full((n_max,), 0xEE, dtype=torch.uint8, device=dev)
        recs = torch.full((n_max * 16,), 0xEE, dtype=torch.uint8, device=dev)
        stats = torch.zeros(40, dtype=torch.uint8, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        cnt.fill_(count)
        X.echo_dev_indirect(d_umem, d_descs, cnt, n_max, verd, recs, stats, opts=opts)
        torch.cuda.synchronize()
        same_dev(d_umem[:count * 64], d_after[:count * 64], "frames below n")
        same_dev(d_umem[count * 64:], d_orig[count * 64:], "frames at or above n")
        same_dev(verd[:count], d_v[:count], "verdicts")
        same_dev(recs[:count * 16], d_r[:count * 16], "records")
        assert bool((verd[count:] == 0xEE).all()) and bool((recs[count * 16:] == 0xEE).all())
        assert stats_of(stats) == IS.prefix_stats(descs, v_ref, count)


# ---- ingress: filter -> transform --------------------------------------------------------------------------------

class Ingress:
    """Device buffers of one ingress_dev call over n frames, sentinels behind every output."""

    def __init__(self, d_umem, d_descs, n):
        dev = _dev()
        self.n, self.umem, self.descs = n, d_umem, d_descs
        self.act = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device=dev)
        self.out = torch.full(((n + 4) * 16,), 0xEE, dtype=torch.uint8, device=dev)
        self.nout = torch.full((2,), -1, dtype=torch.int32, device=dev)
        self.verd = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device=dev)
        self.recs = torch.full(((n + 4) * 16,), 0xEE, dtype=torch.uint8, device=dev)
        self.ws = torch.empty(int(X.lib().xsk_gpu_classify_workspace_size(n)), dtype=torch.uint8, device=dev)

    def run(self, opts, bound, stats):
        X.ingress_dev(self.umem, self.descs, self.n, bound, self.act, self.out, self.nout, self.verd, self.recs, stats,
                      self.ws, opts=opts)

    def check(self, d_after, actions, out, verdicts, recs):
        """Against expected arrays (host arrays; d_after on the device).  Call after a synchronisation."""
        n, k = self.n, len(out)
        nout = self.nout.cpu().numpy().view(np.uint32)
        assert int(nout[0]) == k and int(nout[1]) == 0xFFFFFFFF  # d_nout is one uint32
        same_dev(self.act[:n], to_dev(actions), "actions")
        assert bool((self.act[n:] == 0xEE).all())
        same_dev(self.out[:k * 16], to_dev(out), "d_out")
        assert bool((self.out[k * 16:] == 0xEE).all())
        same_dev(self.verd[:k], to_dev(verdicts), "verdicts by compacted position")
        same_dev(self.recs[:k * 16], to_dev(recs), "records by compacted position")
        assert bool((self.verd[k:] == 0xEE).all()) and bool((self.recs[k * 16:] == 0xEE).all())
        same_dev(self.umem, d_after, "UMEM")


@pytest.mark.parametrize("bound", [True, False])
@pytest.mark.parametrize("opts", [0, 0x13, 0x17])
def test_ingress_matches_spec(opts, bound):
    dev = _dev()
    umem, descs = IS.pipeline_batch()
    after, ref = IS.pipeline_ingress(opts, bound)
    if bound:
        assert 0 < ref["nout"] < len(descs)
    g = Ingress(to_dev(umem), to_dev(descs), len(descs))
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    g.run(opts, bound, stats)
    torch.cuda.synchronize()
    g.check(to_dev(after), ref["actions"], ref["out"], ref["verdicts"], ref["recs"])
    assert stats_of(stats) == ref["stats"]


@pytest.mark.parametrize("bound", [True, False])
@pytest.mark.parametrize("opts", [0, 0x13, 0x17])
def test_ingress_large_tiled_batch(opts, bound):
    """262 147 frames, the 4096-frame batch repeated and cut: 1025 filter workgroups (a scan thread owns more than one
    count), a partial last workgroup of the filter and a partial last tile of the transform, and more transform tiles
    than compute units.  The UMEM is tiled on the device; the expected lists are the base batch's, repeated."""
    dev = _dev()
    n = 262147
    umem, descs = IS.pipeline_batch()
    after, ref = IS.pipeline_ingress(opts, bound)
    nb, span = len(descs), len(descs) * STRIDE
    reps, tail = n // nb, n % nb
    assert reps == 64 and tail == 3
    d = np.tile(descs, reps + 1)
    d["addr"] += np.repeat(np.arange(reps + 1, dtype=np.uint64) * np.uint64(span), nb)
    d = np.ascontiguousarray(d[:n])
    red = ref["actions"] == IS.R
    kt = int(red[:tail].sum())  # redirected among the tail's frames: the first kt entries of the base lists
    actions = np.concatenate([np.tile(ref["actions"], reps), ref["actions"][:tail]])
    out = d[actions == IS.R]
    verdicts = np.concatenate([np.tile(ref["verdicts"], reps), ref["verdicts"][:kt]])
    recs = np.concatenate([np.tile(ref["recs"], (reps, 1)), ref["recs"][:kt]])
    assert len(out) == reps * ref["nout"] + kt == len(verdicts) == len(recs)
    st_tail = IS.prefix_stats(ref["out"], ref["verdicts"], kt)
    want = {k: reps * ref["stats"][k] + st_tail[k] for k in KEYS}
    # frame i of the base batch lies inside [i * STRIDE, (i + 1) * STRIDE): the tail's frames are the first `tail` slots
    d_base, d_base_after = to_dev(umem[:span]), to_dev(after[:span])
    pad = torch.zeros(256, dtype=torch.uint8, device=dev)  # (room for the 64-B window of the last frame)
    d_umem = torch.cat([d_base.repeat(reps), d_base[:tail * STRIDE], pad])
    d_after = torch.cat([d_base_after.repeat(reps), d_base_after[:tail * STRIDE], pad])
    g = Ingress(d_umem, to_dev(d), n)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    g.run(opts, bound, stats)
    torch.cuda.synchronize()
    g.check(d_after, actions, out, verdicts, recs)
    assert stats_of(stats) == want


def test_two_ingress_calls_back_to_back_accumulate():
    """Two calls over two different batches, enqueued on one stream with nothing between them, into one d_stats."""
    dev = _dev()
    opts = 0x17
    umem1, descs1 = IS.pipeline_batch()
    after1, ref1 = IS.pipeline_ingress(opts, True)
    umem2, descs2 = mixed_batch6(1027, STRIDE, seed=9018, offsets=True)
    descs2 = np.ascontiguousarray(descs2, oracle.DESC_DTYPE)
    after2 = umem2.copy()
    ref2 = IS.spec_ingress(after2, descs2, opts, True)
    assert 0 < ref2["nout"] < len(descs2)
    g1 = Ingress(to_dev(umem1), to_dev(descs1), len(descs1))
    g2 = Ingress(to_dev(umem2), to_dev(descs2), len(descs2))
    d_after1, d_after2 = to_dev(after1), to_dev(after2)
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g1.run(opts, True, stats)
    g2.run(opts, True, stats)
    torch.cuda.synchronize()
    g1.check(d_after1, ref1["actions"], ref1["out"], ref1["verdicts"], ref1["recs"])
    g2.check(d_after2, ref2["actions"], ref2["out"], ref2["verdicts"], ref2["recs"])
    assert stats_of(stats) == {k: ref1["stats"][k] + ref2["stats"][k] for k in KEYS}
    assert ref1["stats"]["tx_packets"] > 0 and ref2["stats"]["tx_packets"] > 0


def test_ingress_empty_batch_and_optional_outputs():
    """n == 0 writes *d_nout = 0 and nothing else; verdicts, records and counters are optional."""
    dev = _dev()
    opts = 0x17
    umem, descs = IS.pipeline_batch()
    after, ref = IS.pipeline_ingress(opts, True)
    g = Ingress(to_dev(umem), to_dev(descs), len(descs))
    stats = torch.zeros(40, dtype=torch.uint8, device=dev)
    X.ingress_dev(g.umem, g.descs, 0, True, g.act, g.out, g.nout, g.verd, g.recs, stats, g.ws, opts=opts)
    torch.cuda.synchronize()
    nout = g.nout.cpu().numpy().view(np.uint32)
    assert int(nout[0]) == 0 and int(nout[1]) == 0xFFFFFFFF
    for t in (g.act, g.out, g.verd, g.recs):
        assert bool((t == 0xEE).all())
    same_dev(g.umem, to_dev(umem), "UMEM")
    assert not any(stats_of(stats).values())
    X.ingress_dev(g.umem, g.descs, g.n, True, g.act, g.out, g.nout, None, None, None, g.ws, opts=opts)
    torch.cuda.synchronize()
    assert int(g.nout.cpu().numpy().view(np.uint32)[0]) == ref["nout"]
    same_dev(g.umem, to_dev(after), "UMEM")
    assert bool((g.verd == 0xEE).all()) and bool((g.recs == 0xEE).all())
