"""xsk_gpu_classify_dev_opts without a GPU: the ABI surface, the argument checks, and the Python restatement of its
spec (tests/golden/make_classify_wire_golden.py) pinned by hand, against the reference's filter where the two must
agree, and against the transform's spec for the property that makes filter -> transform sound."""
import errno
import json
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from tests import classify_wire as CW
from tests import v6_frames
from tests.conftest import ROOT, golden_frames

GC, G6, W = CW.GC, v6_frames.G6, v6_frames.G6.W
D, P, R = CW.XDP_DROP, CW.XDP_PASS, CW.XDP_REDIRECT


def test_header_declares_and_library_exports_the_entry_point():
    import xsknet_amd as X
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xsk_gpu.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+xsk_gpu_classify_dev_opts\s*\(([^)]*)\)", src)
    assert m, "xsk_gpu_classify_dev_opts is not declared"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == (
        "const void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, uint32_t n, uint32_t opts, "
        "int target_bound, uint8_t* d_actions, struct xsk_gpu_desc* d_out, uint32_t* d_nout, void* d_workspace, "
        "void* stream")
    assert re.search(r"#define\s+XSK_GPU_ABI_VERSION\s+1\b", src)
    out = subprocess.run(["nm", "-D", "--defined-only", X.LIB_PATH], capture_output=True, text=True, check=True)
    assert re.search(r"\bT xsk_gpu_classify_dev_opts\b", out.stdout)
    assert hasattr(X.lib(), "xsk_gpu_classify_dev_opts") and "xsk_gpu_classify_dev_opts" in X._SIGS


def test_argument_validation_needs_no_gpu():
    import xsknet_amd as X
    f = X.lib().xsk_gpu_classify_dev_opts
    EINVAL = -errno.EINVAL
    um, de, ac, out, nout, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    for bad in (0x8, 0x20, 0x100, 0x18, 0x80000000):
        assert f(um, 4096, de, 1, bad, 1, ac, out, nout, ws, None) == EINVAL, hex(bad)
        assert f(um, 4096, de, 0, bad, 1, ac, out, nout, ws, None) == EINVAL, hex(bad)  # before the n == 0 shortcut
    for opts in (0, 0x2, 0x17):
        assert f(None, 4096, de, 1, opts, 1, ac, out, nout, ws, None) == EINVAL
        assert f(um, 4096, None, 1, opts, 1, ac, out, nout, ws, None) == EINVAL
        assert f(um, 4096, de, 1, opts, 1, None, out, nout, ws, None) == EINVAL
        assert f(um, 4096, de, 1, opts, 1, ac, out, nout, None, None) == EINVAL
        assert f(um, 4096, de, 1, opts, 1, ac, out, None, ws, None) == EINVAL      # d_out without d_nout
        assert f(um, 4096, de + 8, 1, opts, 1, ac, out, nout, ws, None) == EINVAL  # descriptors not 16-B aligned
        assert f(um, 4096, de, 1, opts, 1, ac, out + 4, nout, ws, None) == EINVAL  # d_out not 16-B aligned
        assert f(um, 4096, de, 0xFFFFFFFF, opts, 1, ac, out, nout, ws, None) == EINVAL  # > XSK_GPU_MAX_BATCH
        assert f(None, 0, None, 0, opts, 1, None, None, None, None, None) == 0  # n == 0 without d_nout: nothing to do


# name -> option word -> (bound, unbound); written from the header's rules, not from the generator's output
_ALL = (0x2, 0x10, 0x12, 0x17, 0x5)
HAND = {
    "v4_t0@46": {o: (R, D) for o in _ALL},                      # the reference's case under every option word
    "v4_t0@13": {o: (D, D) for o in _ALL},                      # rule 2
    "v4_t0@33": {o: (D, D) for o in _ALL},                      # l3 + 19
    "v4_t0@34": {o: (R, D) for o in _ALL},                      # l3 + 20
    "v4_t0_proto6@34": {o: (P, P) for o in _ALL},
    "v4_t0_proto17@33": {o: (D, D) for o in _ALL},              # the length test comes before the protocol
    "v4_t0_version6@46": {o: (R, D) for o in _ALL},             # the version nibble is the transform's business
    "v4_t0_ihl6@50": {o: (R, D) for o in _ALL},
    "v4_bad_ip_csum@46": {o: (R, D) for o in _ALL},             # VERIFY (0x17, 0x5) changes no action
    "arp_t0@46": {o: (P, P) for o in _ALL},
    "v4_proto58@46": {o: (P, P) for o in _ALL},
    "v6_t0@62": {0x2: (P, P), 0x10: (R, D), 0x12: (R, D), 0x17: (R, D), 0x5: (P, P)},  # the minimal echo request
    "v6_t0@61": {0x2: (P, P), 0x10: (D, D), 0x12: (D, D), 0x17: (D, D), 0x5: (P, P)},  # l3 + 47
    "v6_t0@54": {0x2: (P, P), 0x10: (D, D), 0x12: (D, D), 0x17: (D, D), 0x5: (P, P)},  # l3 + 40: header in, type out
    "v6_t0@53": {0x2: (P, P), 0x10: (D, D), 0x12: (D, D), 0x17: (D, D), 0x5: (P, P)},  # l3 + 39
    "v6_t0_nh17@54": {o: (P, P) for o in _ALL},                 # next header before the second length test
    "v6_t0_nh0@62": {o: (P, P) for o in _ALL},                  # extension headers are not walked
    "v6_nh1@62": {o: (P, P) for o in _ALL},
    "v6_t0_type129@78": {o: (P, P) for o in _ALL},
    "v6_t0_type135@78": {o: (P, P) for o in _ALL},
    "v6_neighbour_solicitation@90": {o: (P, P) for o in _ALL},  # the host stays reachable over IPv6
    "v6_version4@62": {0x2: (P, P), 0x10: (R, D), 0x12: (R, D), 0x17: (R, D), 0x5: (P, P)},
    "v4_t1@50": {0x2: (R, D), 0x10: (P, P), 0x12: (R, D), 0x17: (R, D), 0x5: (P, P)},  # a tag needs OPT_VLAN
    "v4_t1@17": {0x2: (D, D), 0x10: (P, P), 0x12: (D, D), 0x17: (D, D), 0x5: (P, P)},  # tag cut at its last byte
    "v4_t1@14": {0x2: (D, D), 0x10: (P, P), 0x12: (D, D), 0x17: (D, D), 0x5: (P, P)},  # ... at its first
    "v4_t1@18": {0x2: (D, D), 0x10: (P, P), 0x12: (D, D), 0x17: (D, D), 0x5: (P, P)},  # whole tag, no IPv4 header
    "v4_t2@21": {0x2: (D, D), 0x10: (P, P), 0x12: (D, D), 0x17: (D, D), 0x5: (P, P)},  # second tag cut
    "v4_t2@41": {0x2: (D, D), 0x10: (P, P), 0x12: (D, D), 0x17: (D, D), 0x5: (P, P)},  # l3 + 19 behind two tags
    "v4_t2@42": {0x2: (R, D), 0x10: (P, P), 0x12: (R, D), 0x17: (R, D), 0x5: (P, P)},
    "v6_t1@66": {0x2: (P, P), 0x10: (P, P), 0x12: (R, D), 0x17: (R, D), 0x5: (P, P)},  # needs both bits
    "v6_t2@70": {0x2: (P, P), 0x10: (P, P), 0x12: (R, D), 0x17: (R, D), 0x5: (P, P)},
    "v6_t2@69": {0x2: (P, P), 0x10: (P, P), 0x12: (D, D), 0x17: (D, D), 0x5: (P, P)},
    "v6_q_in_ad@70": {0x2: (P, P), 0x10: (P, P), 0x12: (R, D), 0x17: (R, D), 0x5: (P, P)},
    "v4_t3@46": {o: (P, P) for o in _ALL},                      # a third tag is never skipped
    "v6_t3@74": {o: (P, P) for o in _ALL},
}


def test_spec_pinned_by_hand():
    frames = {name: (f, L) for name, f, L in GC.cases()}
    assert len(HAND) >= 12
    for name, per_opts in HAND.items():
        f, L = frames[name]
        for opts, (b, u) in per_opts.items():
            assert GC.classify(f, L, opts, True) == b, (name, hex(opts))
            assert GC.classify(f, L, opts, False) == u, (name, hex(opts))


def test_crafted_frames_cover_every_boundary():
    names = {name for name, _, _ in GC.cases()}
    for t in (0, 1, 2):
        l3 = 14 + 4 * t
        want = [f"v4_t{t}@13", f"v4_t{t}@14", f"v4_t{t}@{l3 + 19}", f"v4_t{t}@{l3 + 20}", f"v6_t{t}@{l3 + 39}",
                f"v6_t{t}@{l3 + 40}", f"v6_t{t}@{l3 + 47}", f"v6_t{t}@{l3 + 48}", f"arp_t{t}@{l3 + 32}",
                f"v4_t{t}_ihl6@{l3 + 36}", f"v4_t{t}_version6@{l3 + 32}"]
        want += [f"v4_t{t}@{L}" for L in range(14, l3 + 1)] + [f"v6_t{t}@{L}" for L in range(14, l3 + 1)]  # tag cuts
        want += [f"v6_t{t}_nh{nh}@{l3 + 48}" for nh in (0, 6, 17)]
        want += [f"v6_t{t}_type{ty}@{l3 + 64}" for ty in (129, 133, 135, 136, 1)]
        want += [f"v4_t{t}_proto{pr}@{l3 + 20}" for pr in (6, 17)]
        assert not set(want) - names, sorted(set(want) - names)
    assert GC.OPTION_WORDS == (0x2, 0x10, 0x12, 0x17, 0x5)


def test_committed_json_is_the_generators_output():
    assert CW.golden() == json.loads(json.dumps(GC.vectors()))
    for v in CW.golden():  # every vector holds the bytes its length needs
        assert len(bytes.fromhex(v["frame"])) >= v["len"]


@pytest.mark.parametrize("opts", [1, 4, 5])
def test_spec_without_vlan_and_ipv6_is_the_reference_filter(opts):
    """Without OPT_VLAN and OPT_IPV6 the spec is xdp_sock_prog() on every frame whose descriptor is valid."""
    n, stride = 4096, 2048
    umem = np.zeros(n * stride, np.uint8)
    descs = oracle.synth_batch(umem, n, 0, stride, seed=0x5EED0C1A, mode=1, len_lo=0, len_hi=1500)
    for bound in (True, False):
        a_ref, r_ref = oracle.xdp_classify_batch(umem, descs, bound)
        a, r = CW.spec_classify_batch(umem, descs.view(CW.G_DESC), opts, bound)
        assert (a == a_ref).all(), np.nonzero(a != a_ref)[0][:8]
        assert (r.view(oracle.DESC_DTYPE) == r_ref).all()
        assert len(set(a_ref)) == (3 if bound else 2)
    cls = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "classify.json")))}
    for v in golden_frames():
        f = bytes.fromhex(v["input"]) + b"\0" * 64
        assert GC.classify(f, v["len"], opts, True) == cls[v["name"]]["bound"], v["name"]
        assert GC.classify(f, v["len"], opts, False) == cls[v["name"]]["unbound"], v["name"]


@pytest.fixture(scope="module")
def batch7():
    return v6_frames.mixed_batch6(4096, seed=7)


def _transform_verdict(frame: bytes, L: int, opts: int) -> int:
    if L < 14:
        frame = frame + b"\0" * 14
    return (G6.expect(frame, L, opts) if opts & GC.OPT_IPV6 else W.expect(frame, L, opts))[0]


@pytest.mark.parametrize("opts", [0x2, 0x5, 0x7, 0x10, 0x12, 0x13, 0x16, 0x17])
def test_every_frame_the_transform_answers_is_redirected(batch7, opts):
    umem, descs = batch7
    act, red = CW.spec_classify_batch(umem, descs, opts, True)
    replies = 0
    for i in range(len(descs)):
        a, L = int(descs[i]["addr"]), int(descs[i]["len"])
        if _transform_verdict(umem[a:a + L].tobytes(), L, opts) == G6.TX_REPLY:
            replies += 1
            assert act[i] == R, (i, hex(opts))
    assert replies > 100 and len(red) >= replies  # not vacuous: hundreds of the 4096 frames are answered
    assert (red == descs[act == R]).all()
    assert (CW.spec_classify_batch(umem, descs, opts, False)[0] == np.where(act == R, D, act)).all()


def test_dual_stack_batch_populates_every_class(batch7):
    """(DROP, PASS, REDIRECT) x (IPv4, IPv6, neither) under OPT_VLAN | OPT_IPV6: (REDIRECT, neither) cannot occur, the
    other eight do, so the GPU tests over this source see every outcome in both families."""
    umem, descs = batch7
    act, _ = CW.spec_classify_batch(umem, descs, 0x12, True)
    fam = np.array([CW.family(umem, d, 0x12) for d in descs])
    count = {(a, f): int(((act == a) & (fam == f)).sum()) for a in (D, P, R) for f in (4, 6, 0)}
    assert count.pop((R, 0)) == 0
    assert min(count.values()) >= 5, count
