"""xsk_gpu_echo_dev_indirect and xsk_gpu_ingress_dev_opts without a GPU: the ABI surface, the argument checks, the
launch geometry compiled for the host (tests/c/test_indirect_geometry.cpp), and the counter identities the header
states for the transform behind the filter, on the Python spec (tests/ingress_spec.py)."""
import errno
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import ingress_spec as IS
from tests.conftest import ROOT

EINVAL = -errno.EINVAL
MAX_BATCH = 0xFFFFFF00


def _decl(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xsk_gpu.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
    assert m, f"{name} is not declared"
    assert re.search(r"#define\s+XSK_GPU_ABI_VERSION\s+1\b", src)
    assert re.search(r"#define\s+XSK_GPU_OPT_MASK\s+0x17u\b", src)  # no new option bits
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_header_declares_and_library_exports_both_entry_points():
    import xsknet_amd as X
    assert _decl("xsk_gpu_echo_dev_indirect") == (
        "void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, const uint32_t* d_n, uint32_t n_max, "
        "uint32_t opts, uint8_t* d_verdicts, struct xsk_gpu_rec* d_recs, struct xsk_gpu_stats* d_stats, void* stream")
    assert _decl("xsk_gpu_ingress_dev_opts") == (
        "void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, uint32_t n, uint32_t opts, "
        "int target_bound, uint8_t* d_actions, struct xsk_gpu_desc* d_out, uint32_t* d_nout, uint8_t* d_verdicts, "
        "struct xsk_gpu_rec* d_recs, struct xsk_gpu_stats* d_stats, void* d_workspace, void* stream")
    out = subprocess.run(["nm", "-D", "--defined-only", X.LIB_PATH], capture_output=True, text=True, check=True)
    for name in ("xsk_gpu_echo_dev_indirect", "xsk_gpu_ingress_dev_opts"):
        assert re.search(r"\bT " + name + r"\b", out.stdout)
        assert hasattr(X.lib(), name) and name in X._SIGS
    assert callable(X.echo_dev_indirect) and callable(X.ingress_dev)


def test_indirect_argument_validation_needs_no_gpu():
    import xsknet_amd as X
    f = X.lib().xsk_gpu_echo_dev_indirect
    um, de, dn, ve, re_, st = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    for opts in (0, 0x7, 0x17):
        assert f(um, 4096, de, None, 64, opts, ve, re_, st, None) == EINVAL           # d_n NULL
        for mis in (1, 2, 3):
            assert f(um, 4096, de, dn + mis, 64, opts, ve, re_, st, None) == EINVAL   # d_n not 4-B aligned
        assert f(um, 4096, de + 8, dn, 64, opts, ve, re_, st, None) == EINVAL         # descriptors not 16-B aligned
        assert f(um, 4096, de, dn, 64, opts, ve, re_ + 8, st, None) == EINVAL         # records not 16-B aligned
        assert f(um + 4, 4096, de, dn, 64, opts, ve, re_, st, None) == EINVAL
        assert f(um, 4095, de, dn, 64, opts, ve, re_, st, None) == EINVAL
        assert f(None, 4096, de, dn, 64, opts, ve, re_, st, None) == EINVAL
        assert f(um, 4096, None, dn, 64, opts, ve, re_, st, None) == EINVAL
        assert f(um, 4096, de, dn, MAX_BATCH + 1, opts, ve, re_, st, None) == EINVAL  # > XSK_GPU_MAX_BATCH
        assert f(um, 4096, de, dn, 0xFFFFFFFF, opts, ve, re_, st, None) == EINVAL
        assert f(um, 4096, de, dn, 0, opts, ve, re_, st, None) == 0                    # n_max == 0: no launch
        assert f(um, 4096, de, dn, 0, opts, None, None, None, None) == 0
    for bad in (0x8, 0x20, 0x18):
        assert f(um, 4096, de, dn, 64, bad, ve, re_, st, None) == EINVAL, hex(bad)
        assert f(um, 4096, de, dn, 0, bad, ve, re_, st, None) == EINVAL, hex(bad)     # before the n_max == 0 shortcut
    assert f(um, 4096, de, None, 0, 0, ve, re_, st, None) == EINVAL                    # d_n is checked for n_max == 0 too


def test_ingress_argument_validation_needs_no_gpu():
    import xsknet_amd as X
    f = X.lib().xsk_gpu_ingress_dev_opts
    um, de, ac, out, nout, ve, re_, st, ws = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000,
                                              0x90000)
    for opts in (0, 0x13, 0x17):
        assert f(um, 4096, de, 64, opts, 1, ac, None, nout, ve, re_, st, ws, None) == EINVAL      # d_out required
        assert f(um, 4096, de, 64, opts, 1, ac, out, None, ve, re_, st, ws, None) == EINVAL       # d_nout required
        assert f(um, 4096, de, 64, opts, 1, ac, None, None, ve, re_, st, ws, None) == EINVAL
        assert f(um, 4096, de, 64, opts, 1, ac, out, nout + 2, ve, re_, st, ws, None) == EINVAL   # d_nout misaligned
        assert f(um, 4096, de, 64, opts, 1, ac, out + 8, nout, ve, re_, st, ws, None) == EINVAL   # d_out misaligned
        assert f(um, 4096, de + 8, 64, opts, 1, ac, out, nout, ve, re_, st, ws, None) == EINVAL   # d_descs misaligned
        assert f(um, 4096, de, 64, opts, 1, ac, out, nout, ve, re_ + 4, st, ws, None) == EINVAL   # d_recs misaligned
        assert f(um, 4096, de, 64, opts, 1, None, out, nout, ve, re_, st, ws, None) == EINVAL
        assert f(um, 4096, de, 64, opts, 1, ac, out, nout, ve, re_, st, None, None) == EINVAL
        assert f(None, 4096, de, 64, opts, 1, ac, out, nout, ve, re_, st, ws, None) == EINVAL
        assert f(um + 8, 4096, de, 64, opts, 1, ac, out, nout, ve, re_, st, ws, None) == EINVAL
        assert f(um, 4096, de, MAX_BATCH + 1, opts, 1, ac, out, nout, ve, re_, st, ws, None) == EINVAL
    for bad in (0x8, 0x20, 0x18):
        assert f(um, 4096, de, 64, bad, 1, ac, out, nout, ve, re_, st, ws, None) == EINVAL, hex(bad)
        assert f(um, 4096, de, 0, bad, 1, ac, out, nout, ve, re_, st, ws, None) == EINVAL, hex(bad)


def test_indirect_geometry_partitions_the_tiles_and_equals_the_direct_shares():
    """xsk_echo_geometry.h and xsk_echo_indirect.h on the host: n_max in {1, 64, 65, 1024, 1025, 16385, 2^21 + 64} x ncu
    in {1, 16, 256}, every n in {0, 1, 63, 64, 65, n_max - 1, n_max} and 1000 random ones each; then the small batches'
    sub-tiling for every n in 1..1024, tile in {0, 4, 8, 64} and forced grid in {0, 1, 3, 16}."""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "t")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-o", exe,
                        os.path.join(ROOT, "tests", "c", "test_indirect_geometry.cpp")], check=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "indirect geometry ok" in res.stdout


@pytest.mark.parametrize("opts", [0x13, 0x17])
def test_counters_behind_the_filter(opts):
    """The header's identities on mixed_batch6(4096, 2048, seed=9017): rx_packets == nout, rx_bytes == the redirected
    lengths, and -- nonzero opts -- the tx counters and every UMEM byte are the transform's over the whole batch."""
    umem, descs = IS.pipeline_batch()
    after, ref = IS.pipeline_ingress(opts, True)
    n, nout = len(descs), ref["nout"]
    assert 0 < nout < n                                       # a condition of the input
    assert int((ref["verdicts"] == IS.TX_REPLY).sum()) >= 1   # at least one reply
    red = ref["actions"] == IS.R
    assert (ref["out"] == descs[red]).all() and nout == int(red.sum())
    st = ref["stats"]
    assert st["rx_packets"] == nout
    assert st["rx_bytes"] == int(descs["len"][red].astype(np.int64).sum())
    assert st == IS.prefix_stats(ref["out"], ref["verdicts"], nout)
    whole = umem.copy()
    v_all, r_all, st_all = IS.spec_transform(whole, descs, opts)
    assert st["tx_packets"] == st_all["tx_packets"] > 0 and st["tx_bytes"] == st_all["tx_bytes"]
    assert (after == whole).all()
    assert (ref["verdicts"] == v_all[red]).all() and (ref["recs"] == r_all[red]).all()
    # without a bound socket nothing is redirected and nothing changes
    after0, ref0 = IS.pipeline_ingress(opts, False)
    assert ref0["nout"] == 0 and (after0 == umem).all() and not any(ref0["stats"].values())
    assert (ref0["actions"] == np.where(red, 1, ref["actions"])).all()


def test_reference_filter_hides_short_frames_the_reference_transform_answers():
    """opts == 0: the filter drops len < 34, the transform answers some frames of 20..33 bytes, so behind the filter
    the tx counters are NOT the transform's over the whole batch (the header says so).  One such frame by hand."""
    import oracle
    from tests.conftest import golden_frames
    v = next(g for g in golden_frames() if g["name"] == "echo_64")
    frame = np.frombuffer(bytes.fromhex(v["input"]), np.uint8)
    assert len(frame) >= 38
    umem = np.zeros(4096, np.uint8)
    umem[:len(frame)] = frame
    descs = np.zeros(1, oracle.DESC_DTYPE)
    descs[0] = (0, 33, 0)  # the frame's first 33 bytes; bytes up to 38 are in the UMEM behind them
    alone = umem.copy()
    v_alone, _, st_alone = IS.spec_transform(alone, descs, 0)
    assert v_alone[0] == IS.TX_REPLY and st_alone["tx_packets"] == 1
    behind = umem.copy()
    ref = IS.spec_ingress(behind, descs, 0, True)
    assert ref["nout"] == 0 and ref["actions"][0] == 1 and (behind == umem).all() and ref["stats"]["tx_packets"] == 0
