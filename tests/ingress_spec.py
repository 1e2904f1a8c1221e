"""The spec of xsk_gpu_ingress_dev_opts and xsk_gpu_echo_dev_indirect over a batch, composed of the specs the two
halves already have: the filter's (tests/classify_wire.spec_classify_batch; oracle.xdp_classify_batch for opts == 0)
and the transform's (tests/v6_frames.spec_batch with XSK_GPU_OPT_IPV6, the C oracle otherwise).

References are computed once and cached; a test that needs the result over a prefix of a batch derives it from the
result over the whole batch (prefix_stats): frames of these batches never overlap, so frame i's bytes, verdict, record
and counters do not depend on the frames after it.
"""
import functools

import numpy as np

import oracle
from tests import classify_wire as CW
from tests.v6_frames import mixed_batch6, spec_batch

TX_REPLY = 0
KEYS = ("rx_packets", "rx_bytes", "tx_packets", "tx_bytes")
R = CW.XDP_REDIRECT


def spec_transform(umem: np.ndarray, descs: np.ndarray, opts: int):
    """xsk_gpu_echo_dev_opts over the batch, in place: (verdicts, records as n x 16 bytes, counters as a dict)."""
    d = np.ascontiguousarray(descs, oracle.DESC_DTYPE)
    if opts & 0x10:
        v, r, st = spec_batch(umem, d, opts)
    elif opts:
        v, r, s = oracle.echo_batch_opts(umem, d, opts)
        st = {k: int(s[k]) for k in KEYS}
    else:
        v, r, s = oracle.echo_batch(umem, d)
        st = {k: int(s[k]) for k in KEYS}
    return v, np.ascontiguousarray(r).view(np.uint8).reshape(-1, 16), st


def prefix_stats(descs: np.ndarray, verdicts: np.ndarray, n: int):
    """The counters of the first n frames of a batch whose verdicts are known: every frame is received, a TX_REPLY
    frame is transmitted with its length."""
    L, tx = descs["len"][:n].astype(np.int64), verdicts[:n] == TX_REPLY
    return dict(rx_packets=n, rx_bytes=int(L.sum()), tx_packets=int(tx.sum()), tx_bytes=int(L[tx].sum()))


def spec_ingress(umem: np.ndarray, descs: np.ndarray, opts: int, bound: bool):
    """xsk_gpu_ingress_dev_opts over the batch, UMEM in place: dict of actions, out (the redirected descriptors in
    batch order), nout, verdicts and recs (by position in out), stats."""
    d = np.ascontiguousarray(descs, oracle.DESC_DTYPE)
    if opts:
        act, out = CW.spec_classify_batch(umem, d, opts, bound)
    else:
        act, out = oracle.xdp_classify_batch(umem, d, bound)
    out = np.ascontiguousarray(out, oracle.DESC_DTYPE)
    if len(out):
        v, r, st = spec_transform(umem, out, opts)
    else:
        v, r, st = np.zeros(0, np.uint8), np.zeros((0, 16), np.uint8), dict.fromkeys(KEYS, 0)
    return dict(actions=act, out=out, nout=len(out), verdicts=v, recs=r, stats=st)


@functools.lru_cache(maxsize=None)
def pipeline_batch():
    """The 4096-frame dual-stack batch of the filter -> transform tests (read-only)."""
    umem, descs = mixed_batch6(4096, 2048, seed=9017, offsets=True)
    descs = np.ascontiguousarray(descs, oracle.DESC_DTYPE)
    umem.setflags(write=False)
    descs.setflags(write=False)
    return umem, descs


@functools.lru_cache(maxsize=None)
def pipeline_ingress(opts: int, bound: bool):
    """(UMEM after, spec_ingress result) of pipeline_batch(), read-only."""
    umem, descs = pipeline_batch()
    after = umem.copy()
    ref = spec_ingress(after, descs, opts, bound)
    after.setflags(write=False)
    return after, ref
