"""xsk_gpu_egress_ports_dev without a GPU: the ABI surface, the argument checks (fabricated pointers, no device call
reached), the arithmetic of both kernel paths compiled for the host under AddressSanitizer
(tests/c/test_egress_ports.cpp), and the Python spec (tests/egress_ports_spec.py) against egress_spec.spec_egress
applied to each segment, the one-port identity and the offset rule."""
import errno
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import egress_ports_spec as EP
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
    assert _decl("int", "xsk_gpu_egress_ports_dev") == (
        "const struct xsk_gpu_desc* d_descs, const uint8_t* d_verdicts, const uint32_t* d_off, uint32_t n_ports, "
        "uint32_t n_max, const uint32_t* d_tx_room, struct xsk_gpu_desc* d_tx, uint64_t* d_free, "
        "struct xsk_gpu_egress_counts* d_counts, struct xsk_gpu_stats* d_stats, struct xsk_gpu_stats* d_port_stats, "
        "void* d_workspace, void* stream")
    assert _decl("size_t", "xsk_gpu_egress_ports_workspace_size") == "uint32_t n_max, uint32_t n_ports"
    out = subprocess.run(["nm", "-D", "--defined-only", X.LIB_PATH], capture_output=True, text=True, check=True)
    for name in ("xsk_gpu_egress_ports_dev", "xsk_gpu_egress_ports_workspace_size"):
        assert re.search(r"\bT " + name + r"\b", out.stdout)
        assert hasattr(X.lib(), name) and name in X._SIGS
    # no new hook: everything else of the feature is static or in an anonymous namespace
    assert not [s for s in re.findall(r"\bT (\w+)", out.stdout) if "egress" in s and not s.startswith("xsk_gpu_egress_")]
    assert not re.search(r"\bT xsk_gpu__\w*egress", out.stdout)
    assert callable(X.egress_ports_dev) and callable(X.egress_ports_workspace_size)
    assert "egress_ports_dev" in X.__all__ and "egress_ports_workspace_size" in X.__all__
    assert len(X._SIGS["xsk_gpu_egress_ports_dev"][0]) == 13
    assert len(X._SIGS["xsk_gpu_egress_ports_workspace_size"][0]) == 2


def test_the_three_not_built_remarks_point_to_the_call():
    hdr = open(os.path.join(ROOT, "include", "xsk_gpu.h")).read()
    steer = hdr[hdr.index("Steered ingress in one asynchronous call"):hdr.index("int xsk_gpu_ingress_steer_dev(")]
    assert "xsk_gpu_egress_ports_dev()" in steer and "Not built" not in steer and "follow-up" not in steer
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "xsk_gpu_egress_ports_dev" in text
        assert "an egress per port segment" not in text and "segmented egress is the follow-up" not in text


def test_workspace_size():
    import xsknet_amd as X
    ws = X.egress_ports_workspace_size
    for n in (0, 1, 64, 1024):
        for ports in (1, 8, 64):
            assert ws(n, ports) == 0                    # the one-launch path takes none
    # a word per 256-frame workgroup and per boundary, and a 32-B record of per-port counter sums per workgroup
    assert ws(1025, 1) == (5 + 2) * 4 + 5 * 32
    assert ws(1025, 64) == (5 + 65) * 4 + 5 * 32
    assert ws(1280, 8) == (5 + 9) * 4 + 5 * 32 and ws(1281, 8) == (6 + 9) * 4 + 6 * 32
    assert ws(262147, 8) == (1025 + 9) * 4 + 1025 * 32
    nwg = (MAX_BATCH + 255) // 256
    assert ws(MAX_BATCH, 64) == (nwg + 65) * 4 + nwg * 32


def test_argument_validation_needs_no_gpu():
    import xsknet_amd as X
    f = X.lib().xsk_gpu_egress_ports_dev
    de, ve, of, room, tx, fr, co, st, ps, ws = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000,
                                                0x90000, 0xA0000)
    for n_max in (64, 1024, 1025, 4096):
        for P in (1, 8, 64):
            assert f(None, ve, of, P, n_max, room, tx, fr, co, st, ps, ws, None) == EINVAL          # d_descs NULL
            assert f(de, None, of, P, n_max, room, tx, fr, co, st, ps, ws, None) == EINVAL          # d_verdicts NULL
            assert f(de, ve, None, P, n_max, room, tx, fr, co, st, ps, ws, None) == EINVAL          # d_off NULL
            assert f(de, ve, of, P, n_max, room, None, fr, co, st, ps, ws, None) == EINVAL          # d_tx NULL
            assert f(de, ve, of, P, n_max, room, tx, None, co, st, ps, ws, None) == EINVAL          # d_free NULL
            assert f(de, ve, of, P, n_max, room, tx, fr, None, st, ps, ws, None) == EINVAL          # d_counts NULL
            for mis in (1, 2, 4, 8):
                assert f(de + mis, ve, of, P, n_max, room, tx, fr, co, st, ps, ws, None) == EINVAL  # d_descs: 16 B
                assert f(de, ve, of, P, n_max, room, tx + mis, fr, co, st, ps, ws, None) == EINVAL  # d_tx: 16 B
            for mis in (1, 2, 4):
                assert f(de, ve, of, P, n_max, room, tx, fr + mis, co, st, ps, ws, None) == EINVAL  # d_free: 8 B
                assert f(de, ve, of, P, n_max, room, tx, fr, co, st + mis, ps, ws, None) == EINVAL  # d_stats: 8 B
                assert f(de, ve, of, P, n_max, room, tx, fr, co, st, ps + mis, ws, None) == EINVAL  # d_port_stats: 8 B
                assert f(de, ve, of, P, n_max, room, tx, fr, co, None, ps + mis, ws, None) == EINVAL
            for mis in (1, 2, 3):
                assert f(de, ve, of, P, n_max, room, tx, fr, co + mis, st, ps, ws, None) == EINVAL  # d_counts: 4 B
                assert f(de, ve, of + mis, P, n_max, room, tx, fr, co, st, ps, ws, None) == EINVAL  # d_off: 4 B
                assert f(de, ve, of, P, n_max, room + mis, tx, fr, co, st, ps, ws, None) == EINVAL  # d_tx_room: 4 B
                assert f(de, ve + mis, of, P, n_max, room, de, fr, co, st, ps, ws, None) == EINVAL  # (any verdict
                #                                                      alignment: the refusal is d_tx == d_descs)
            assert f(de, ve, of, P, n_max, room, de, fr, co, st, ps, ws, None) == EINVAL            # d_tx == d_descs
            assert f(de, ve, of, P, n_max, None, de, fr, co, None, None, ws, None) == EINVAL
        for P in (0, 65, 66, 0xFF, 0xFFFFFFFF):
            assert f(de, ve, of, P, n_max, room, tx, fr, co, st, ps, ws, None) == EINVAL            # n_ports
    for big in (MAX_BATCH + 1, 0xFFFFFFFF):
        assert f(de, ve, of, 8, big, room, tx, fr, co, st, ps, ws, None) == EINVAL      # n_max > XSK_GPU_MAX_BATCH
    assert f(de, ve, of, 8, 1025, room, tx, fr, co, st, ps, None, None) == EINVAL       # workspace required
    assert f(de, ve, of, 1, MAX_BATCH, room, tx, fr, co, st, ps, None, None) == EINVAL
    # n_max == 1024 needs no workspace: with it NULL every OTHER rule is still what refuses the call (the success
    # path launches: tests/test_gpu_egress_ports.py)
    assert f(de, ve, of, 8, 1024, room, de, fr, co, st, ps, None, None) == EINVAL       # d_tx == d_descs
    assert f(de, ve, of + 2, 8, 1024, room, tx, fr, co, st, ps, None, None) == EINVAL
    assert f(de, ve, of, 65, 1024, room, tx, fr, co, st, ps, None, None) == EINVAL
    # the rules hold for an empty bound too (nothing is issued before them; the success path reaches a memset)
    assert f(None, ve, of, 8, 0, room, tx, fr, co, st, ps, ws, None) == EINVAL
    assert f(de, ve, None, 8, 0, room, tx, fr, co, st, ps, ws, None) == EINVAL
    assert f(de, ve, of, 0, 0, room, tx, fr, co, st, ps, ws, None) == EINVAL
    assert f(de, ve, of, 8, 0, room, tx, fr, co + 2, st, ps, ws, None) == EINVAL


def test_every_rule_stands_in_front_of_the_first_device_call():
    src = open(os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_egress_ports.hip")).read()
    body = src[src.index("int xsk_gpu_egress_ports_dev("):]
    assert re.search(r"!d_workspace\s*&&\s*n_max\s*>\s*kEgSmallMax", body)
    first_device_call = min(body.index(t) for t in ("hipMemsetAsync", "<<<"))
    assert body.index("return -EINVAL") < first_device_call
    assert body.count("-EINVAL") == 1  # one block of checks, nothing refused later
    for word in ("hipMalloc", "Synchronize", "hipMemcpy"):  # allocates nothing, synchronises nothing, reads nothing
        assert word not in src


def test_arithmetic_on_the_host_under_address_sanitizer():
    """tests/c/test_egress_ports.cpp: xsk_egress_ports.h's offsets, owner search, per-port slot, boundary prefixes, grid
    and workspace size, both paths replayed thread by thread against a sequential loop per port; every store inside the
    owning port's list and every slot written once."""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "t")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "c", "test_egress_ports.cpp")], check=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    assert "egress ports ok" in res.stdout


# ---- the spec ----------------------------------------------------------------------------------------------------

def _rooms_for(kind, Rs):
    if kind == "null":
        return None
    if kind == "zero":
        return [0] * len(Rs)
    if kind == "R-1":
        return [max(R - 1, 0) for R in Rs]
    if kind == "R":
        return list(Rs)
    if kind == "R+1":
        return [R + 1 for R in Rs]
    assert kind == "mixed"
    return [(ES.UNLIMITED, 0, max(R - 1, 0), R // 2)[p % 4] for p, R in enumerate(Rs)]


ROOM_KINDS = ("null", "zero", "R-1", "R", "R+1", "mixed")
SPEC_CASES = [(n_max, ports, lay) for n_max in (1, 65, 300, 1025) for ports in (1, 8, 64) for lay in EP.LAYOUTS]


@pytest.mark.parametrize("n_max,n_ports,lay", SPEC_CASES)
def test_spec_is_spec_egress_on_each_segment(n_max, n_ports, lay):
    """Port p of the batch form == egress_spec.spec_egress over descs[o_p:], verd[o_p:] with n = n_p and the port's
    room, for every layout, room kind and reply pattern; the shared deltas are the sums."""
    descs = ES.random_descs(n_max, seed=n_max)
    off = EP.layout(lay, n_ports, n_max, seed=n_ports)
    # the offsets, restated: ascending, inside the bound, equal to the words where those are ascending and inside it
    o = EP.offsets(off, n_ports, n_max)
    assert all(0 <= a <= b <= n_max for a, b in zip(o, o[1:])) and len(o) == n_ports + 1
    if off == sorted(off) and off[-1] <= n_max:
        assert o == off
    for pat in ES.PATTERNS:
        verd = ES.verdict_pattern(pat, n_max, seed=n_max)
        Rs = [int((verd[o[p]:o[p + 1]] == 0).sum()) for p in range(n_ports)]
        for kind in ROOM_KINDS:
            rooms = _rooms_for(kind, Rs)
            sp = EP.spec_egress_ports(descs, verd, off, n_ports, n_max, rooms)
            assert sp["o"] == o
            dp = db = 0
            for p in range(n_ports):
                room = ES.UNLIMITED if rooms is None else rooms[p]
                tx, free, c, dp_p, db_p = ES.spec_egress(descs[o[p]:], verd[o[p]:], o[p + 1] - o[p], room)
                assert sp["counts"][p] == c, (p, sp["counts"][p], c)
                assert sp["tx"][p].tolist() == tx.tolist() and sp["free"][p].tolist() == free.tolist()
                assert sp["port_stats"][p] == dict(
                    rx_packets=c["n"], rx_bytes=int(descs["len"][o[p]:o[p + 1]].astype(np.int64).sum()),
                    tx_packets=c["n_tx"], tx_bytes=int(tx["len"].astype(np.int64).sum()))
                dp, db = dp + dp_p, db + db_p
            assert (sp["d_tx_packets"], sp["d_tx_bytes"]) == (dp, db)
            assert dp == -sum(c["n_tx_full"] for c in sp["counts"])
            # frames on no list appear nowhere; the listed ones exactly once
            listed = sorted(a for p in range(n_ports) for a in sp["tx"][p]["addr"].tolist() + sp["free"][p].tolist())
            assert listed == sorted(descs["addr"][o[0]:o[n_ports]].tolist())
            if kind == "mixed" and n_ports >= 8 and lay == "even" and pat == "random" and n_max >= 300:
                full = [c["n_tx_full"] > 0 for c in sp["counts"]]
                assert any(full) and not all(full)  # cut and uncut ports side by side: a condition of the input


@pytest.mark.parametrize("n_max", [1, 64, 65, 1024, 1025, 3000])
def test_one_port_identity(n_max):
    """n_ports == 1 and off = {0, k}: spec_egress(n = min(k, n_max)), for k above n_max too."""
    descs = ES.random_descs(n_max, seed=n_max)
    for pat in ("random", "all", "lane63"):
        verd = ES.verdict_pattern(pat, n_max, seed=n_max)
        for k in sorted({0, 1, n_max - 1, n_max, n_max + 5, 0xFFFFFFFF}):
            n = min(k, n_max)
            R = int((verd[:n] == 0).sum())
            for room in (None, 0, max(R - 1, 0), R, R + 1, R // 2):
                sp = EP.spec_egress_ports(descs, verd, [0, k], 1, n_max, None if room is None else [room])
                tx, free, c, dp, db = ES.spec_egress(descs, verd, n, ES.UNLIMITED if room is None else room)
                assert sp["o"] == [0, n] and sp["counts"] == [c]
                assert sp["tx"][0].tolist() == tx.tolist() and sp["free"][0].tolist() == free.tolist()
                assert (sp["d_tx_packets"], sp["d_tx_bytes"]) == (dp, db)


def test_offset_rule():
    """Words descending, equal, above n_max, and with d_off[0] > 0: the clamped running maximum."""
    n_max = 100
    assert EP.offsets([0, 10, 20, 100], 3, n_max) == [0, 10, 20, 100]            # what the steering call writes
    assert EP.offsets([50, 40, 30, 20], 3, n_max) == [50, 50, 50, 50]            # descending: every segment empty
    assert EP.offsets([0, 60, 30, 80], 3, n_max) == [0, 60, 60, 80]              # one word out of order: port 1 empty
    assert EP.offsets([7, 7, 7, 7], 3, n_max) == [7, 7, 7, 7]                    # equal
    assert EP.offsets([0, 50, 101, 70], 3, n_max) == [0, 50, 100, 100]           # above the bound, then below it
    assert EP.offsets([0, 0xFFFFFFFF, 5, 6], 3, n_max) == [0, 100, 100, 100]
    assert EP.offsets([200, 300, 400, 500], 3, n_max) == [100, 100, 100, 100]    # everything above: nothing listed
    assert EP.offsets([30, 40, 90, 95], 3, n_max) == [30, 40, 90, 95]            # d_off[0] > 0, d_off[3] < n_max
    descs = ES.random_descs(n_max, seed=3)
    verd = ES.verdict_pattern("alternating", n_max, seed=3)
    sp = EP.spec_egress_ports(descs, verd, [30, 40, 90, 95], 3, n_max, [2, 0, ES.UNLIMITED])
    assert [c["n"] for c in sp["counts"]] == [10, 50, 5]
    assert sp["counts"][0] == dict(n=10, n_tx=2, n_tx_full=3, n_free=8)
    assert sp["counts"][1] == dict(n=50, n_tx=0, n_tx_full=25, n_free=50)
    assert sp["counts"][2] == dict(n=5, n_tx=3, n_tx_full=0, n_free=2)
    assert sp["tx"][0]["addr"].tolist() == descs["addr"][[30, 32]].tolist()
    assert sp["free"][0].tolist() == descs["addr"][[31, 33, 34, 35, 36, 37, 38, 39]].tolist()
    assert sp["d_tx_packets"] == -28
    sp = EP.spec_egress_ports(descs, verd, [50, 40, 30, 20], 3, n_max)
    assert all(c == dict(n=0, n_tx=0, n_tx_full=0, n_free=0) for c in sp["counts"])
    assert all(len(t) == 0 for t in sp["tx"]) and all(len(f) == 0 for f in sp["free"])
    tx, free = EP.expected_arrays(sp, n_max)
    assert (tx == 0xEE).all() and (free == 0xEE).all()
