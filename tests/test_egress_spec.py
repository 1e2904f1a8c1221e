"""xsk_gpu_egress_dev without a GPU: the ABI surface, the argument checks (fabricated pointers, no device call
reached), the slot arithmetic of both kernel paths compiled for the host under AddressSanitizer
(tests/c/test_egress_slots.cpp), and the identities of the Python spec (tests/egress_spec.py), which is also compared
with a line-by-line restatement of xsk_gpu__rx_emit()'s loop written independently of it."""
import errno
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from tests import egress_spec as ES
from tests.conftest import ROOT

EINVAL = -errno.EINVAL
MAX_BATCH = 0xFFFFFF00


def _header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xsk_gpu.h")).read(), flags=re.S)
    assert re.search(r"#define\s+XSK_GPU_ABI_VERSION\s+1\b", src)
    assert re.search(r"#define\s+XSK_GPU_OPT_MASK\s+0x17u\b", src)  # additive: no new version, no new option bits
    return src


def _decl(ret, name):
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)", _header())
    assert m, f"{name} is not declared"
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_header_declares_and_library_exports_the_entry_points():
    import xsknet_amd as X
    assert _decl("int", "xsk_gpu_egress_dev") == (
        "const struct xsk_gpu_desc* d_descs, const uint8_t* d_verdicts, const uint32_t* d_n, uint32_t n_max, "
        "const uint32_t* d_tx_room, struct xsk_gpu_desc* d_tx, uint64_t* d_free, "
        "struct xsk_gpu_egress_counts* d_counts, struct xsk_gpu_stats* d_stats, void* d_workspace, void* stream")
    assert _decl("size_t", "xsk_gpu_egress_workspace_size") == "uint32_t n_max"
    m = re.search(r"struct\s+xsk_gpu_egress_counts\s*\{([^}]*)\}", _header())
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == \
        "uint32_t n; uint32_t n_tx; uint32_t n_tx_full; uint32_t n_free;"
    out = subprocess.run(["nm", "-D", "--defined-only", X.LIB_PATH], capture_output=True, text=True, check=True)
    for name in ("xsk_gpu_egress_dev", "xsk_gpu_egress_workspace_size"):
        assert re.search(r"\bT " + name + r"\b", out.stdout)
        assert hasattr(X.lib(), name) and name in X._SIGS
    # no new hook: everything else of the feature is static or in an anonymous namespace
    assert not [s for s in re.findall(r"\bT (\w+)", out.stdout) if "egress" in s and not s.startswith("xsk_gpu_egress_")]
    assert not re.search(r"\bT xsk_gpu__\w*egress", out.stdout)
    assert callable(X.egress_dev) and callable(X.egress_workspace_size)
    assert len(X._SIGS["xsk_gpu_egress_dev"][0]) == 11


def test_counts_struct_layout_matches_the_dtype():
    import xsknet_amd as X
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "xsk_gpu.h"
#define O(f) printf(#f " %zu\n", offsetof(struct xsk_gpu_egress_counts, f))
int main(void){ printf("size %zu\n", sizeof(struct xsk_gpu_egress_counts)); O(n); O(n_tx); O(n_tx_full); O(n_free); return 0; }
'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "p.c")
        open(c, "w").write(probe)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(td, "p"), c],
                       check=True)
        out = subprocess.run([os.path.join(td, "p")], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "size 16" and X.EGRESS_COUNTS_DTYPE.itemsize == 16
    offs = dict(line.split() for line in out[1:] if line)
    assert list(X.EGRESS_COUNTS_DTYPE.names) == ["n", "n_tx", "n_tx_full", "n_free"]
    for f in X.EGRESS_COUNTS_DTYPE.names:
        assert int(offs[f]) == X.EGRESS_COUNTS_DTYPE.fields[f][1], f
        assert X.EGRESS_COUNTS_DTYPE.fields[f][0] == np.dtype("<u4")
    assert X.EGRESS_COUNTS_DTYPE == ES.COUNTS_DTYPE


def test_workspace_size():
    import xsknet_amd as X
    ws = X.egress_workspace_size
    for n in (0, 1, 64, 1024):
        assert ws(n) == 0                      # the one-launch path takes none
    assert ws(1025) == 5 * 4                   # one uint32_t per 256-frame workgroup
    assert ws(1280) == 5 * 4 and ws(1281) == 6 * 4
    assert ws(262147) == 1025 * 4
    assert ws(MAX_BATCH) == ((MAX_BATCH + 255) // 256) * 4


def test_argument_validation_needs_no_gpu():
    import xsknet_amd as X
    f = X.lib().xsk_gpu_egress_dev
    de, ve, dn, room, tx, fr, co, st, ws = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000,
                                            0x90000)
    for n_max in (64, 1024, 1025, 4096):
        assert f(None, ve, dn, n_max, room, tx, fr, co, st, ws, None) == EINVAL          # d_descs NULL
        assert f(de, None, dn, n_max, room, tx, fr, co, st, ws, None) == EINVAL          # d_verdicts NULL
        assert f(de, ve, dn, n_max, room, None, fr, co, st, ws, None) == EINVAL          # d_tx NULL
        assert f(de, ve, dn, n_max, room, tx, None, co, st, ws, None) == EINVAL          # d_free NULL
        assert f(de, ve, dn, n_max, room, tx, fr, None, st, ws, None) == EINVAL          # d_counts NULL
        for mis in (1, 2, 4, 8):
            assert f(de + mis, ve, dn, n_max, room, tx, fr, co, st, ws, None) == EINVAL  # d_descs not 16-B aligned
            assert f(de, ve, dn, n_max, room, tx + mis, fr, co, st, ws, None) == EINVAL  # d_tx not 16-B aligned
        for mis in (1, 2, 4):
            assert f(de, ve, dn, n_max, room, tx, fr + mis, co, st, ws, None) == EINVAL  # d_free not 8-B aligned
            assert f(de, ve, dn, n_max, room, tx, fr, co, st + mis, ws, None) == EINVAL  # d_stats not 8-B aligned
        for mis in (1, 2, 3):
            assert f(de, ve, dn, n_max, room, tx, fr, co + mis, st, ws, None) == EINVAL  # d_counts not 4-B aligned
            assert f(de, ve, dn + mis, n_max, room, tx, fr, co, st, ws, None) == EINVAL  # d_n not 4-B aligned
            assert f(de, ve, dn, n_max, room + mis, tx, fr, co, st, ws, None) == EINVAL  # d_tx_room not 4-B aligned
            assert f(de, ve + mis, dn, n_max, room, de, fr, co, st, ws, None) == EINVAL  # (any verdict alignment: the
            #                                                                              refusal is d_tx == d_descs)
        assert f(de, ve, dn, n_max, room, de, fr, co, st, ws, None) == EINVAL            # d_tx == d_descs
        assert f(de, ve, None, n_max, None, de, fr, co, None, ws, None) == EINVAL
    for big in (MAX_BATCH + 1, 0xFFFFFFFF):
        assert f(de, ve, dn, big, room, tx, fr, co, st, ws, None) == EINVAL              # n_max > XSK_GPU_MAX_BATCH
    assert f(de, ve, dn, 1025, room, tx, fr, co, st, None, None) == EINVAL               # workspace required
    assert f(de, ve, dn, MAX_BATCH, room, tx, fr, co, st, None, None) == EINVAL
    # n_max == 1024 needs no workspace: with it NULL every OTHER rule is still what refuses the call (the success
    # path launches: tests/test_gpu_egress.py)
    assert f(de, ve, dn, 1024, room, de, fr, co, st, None, None) == EINVAL               # d_tx == d_descs
    assert f(de, ve, dn + 2, 1024, room, tx, fr, co, st, None, None) == EINVAL
    # the rules hold for an empty bound too (nothing is issued before them)
    assert f(None, ve, dn, 0, room, tx, fr, co, st, ws, None) == EINVAL
    assert f(de, ve, dn, 0, room, tx, fr, None, st, ws, None) == EINVAL
    assert f(de, ve, dn, 0, room, tx, fr, co + 2, st, ws, None) == EINVAL


def test_workspace_null_at_1024_is_not_what_refuses_the_call():
    """The host function's own text: the workspace rule compares n_max with the one-launch bound, XSK_GPU_LOWLAT_MAX
    (1024), and every rule stands in front of the first device call."""
    src = open(os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_egress.hip")).read()
    body = src[src.index("int xsk_gpu_egress_dev("):]
    assert re.search(r"!d_workspace\s*&&\s*n_max\s*>\s*kEgSmallMax", body)
    hdr = open(os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_egress.h")).read()
    assert re.search(r"kEgSmallMax\s*=\s*1024\b", hdr)
    first_device_call = min(body.index(t) for t in ("hipMemsetAsync", "<<<"))
    assert body.index("return -EINVAL") < first_device_call
    assert body.count("-EINVAL") == 1  # one block of checks, nothing refused later


def test_slot_arithmetic_on_the_host_under_address_sanitizer():
    """tests/c/test_egress_slots.cpp: xsk_egress.h's slot rule, grid, scan runs and workspace size, both paths replayed
    thread by thread into heap arrays of exactly n_tx and n_free entries (inputs of exactly n), against the sequential
    loop; eleven sizes, every count / room / pattern of its header comment."""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "t")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "c", "test_egress_slots.cpp")], check=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    assert "egress slots ok" in res.stdout


# ---- the spec ----------------------------------------------------------------------------------------------------

def rx_emit_restated(descs, verdict, n, ring_free):
    """xsk_gpu__rx_emit() (xsknet_amd/csrc/xsk_gpu_rx.c:32-66), line by line; `ring_free` is what xr_prod_free() would
    report.  Returns (tx entries, pool pushes, replied, tx_full, tx_packets delta against "every reply counted",
    tx_bytes delta)."""
    nrep = 0
    for i in range(n):
        nrep += 1 if verdict[i] == 0 else 0
    room, sent = 0, 0
    if nrep:
        room = ring_free
        if room > nrep:
            room = nrep
    ring, pool = [], []
    tx_bytes, tx_full = 0, 0
    all_reply_bytes = 0
    for i in range(n):
        if verdict[i] == 0:
            all_reply_bytes += int(descs[i]["len"])
        if verdict[i] == 0 and sent < room:
            ring.append((int(descs[i]["addr"]), int(descs[i]["len"]), 0))
            sent += 1
            tx_bytes += int(descs[i]["len"])
        else:
            if verdict[i] == 0:
                tx_full += 1
            pool.append(int(descs[i]["addr"]))
    # the transform counted every reply (tx_packets += nrep, tx_bytes += all_reply_bytes); rx_emit counts `sent`
    return ring, pool, sent, tx_full, sent - nrep, tx_bytes - all_reply_bytes


def _rooms(R):
    return [0, 1, 37, max(R - 1, 0), R, R + 1, ES.UNLIMITED]


SPEC_CASES = [(n_max, pat) for n_max in (1, 64, 65, 300, 1025) for pat in ES.PATTERNS]


@pytest.mark.parametrize("n_max,pattern", SPEC_CASES)
def test_spec_identities_and_the_rx_loop(n_max, pattern):
    descs = ES.random_descs(n_max, seed=n_max)
    verd = ES.verdict_pattern(pattern, n_max, seed=n_max)
    assert (descs["options"] != 0).all() and len(set(descs["addr"].tolist())) == n_max
    for n in sorted({0, 1, n_max - 1, n_max}):
        R = int((verd[:n] == 0).sum())
        for room in _rooms(R):
            tx, free, c, dp, db = ES.spec_egress(descs, verd, n, room)
            assert c["n"] == n and c["n_tx"] + c["n_free"] == n
            assert c["n_tx"] == min(R, room) and c["n_tx_full"] == R - c["n_tx"]
            assert len(tx) == c["n_tx"] and len(free) == c["n_free"]
            # tx followed by free, as address multisets, is the input
            assert sorted(tx["addr"].tolist() + free.tolist()) == sorted(descs["addr"][:n].tolist())
            assert (tx["options"] == 0).all()
            reply = verd[:n] == 0
            if room >= R:
                assert (free == descs["addr"][:n][~reply]).all() and dp == 0 and db == 0
                assert (tx["addr"] == descs["addr"][:n][reply]).all() and (tx["len"] == descs["len"][:n][reply]).all()
            # the host modes' loop
            ring, pool, sent, tx_full, dp2, db2 = rx_emit_restated(descs, verd, n, room)
            assert [tuple(int(x) for x in t) for t in tx.tolist()] == ring
            assert free.tolist() == pool
            assert (c["n_tx"], c["n_tx_full"]) == (sent, tx_full) and (dp, db) == (dp2, db2)
            assert dp == -c["n_tx_full"] and db <= 0


def test_spec_on_the_pipeline_batch():
    """Behind spec_ingress on the 4096-frame dual-stack batch: the replies are the verdict-0 entries of the compacted
    list, and with the ring cut the counters end at the frames submitted."""
    from tests import ingress_spec as IS
    _, ref = IS.pipeline_ingress(0x17, True)
    out, v, k = ref["out"], ref["verdicts"], ref["nout"]
    R = int((v == 0).sum())
    assert 1 < R < k
    tx, free, c, dp, db = ES.spec_egress(out, v, k, R // 2)
    assert c == dict(n=k, n_tx=R // 2, n_tx_full=R - R // 2, n_free=k - R // 2)
    st = ref["stats"]
    assert st["tx_packets"] + dp == R // 2 and st["tx_bytes"] + db == int(tx["len"].astype(np.int64).sum())
    assert np.ascontiguousarray(out).dtype == oracle.DESC_DTYPE
