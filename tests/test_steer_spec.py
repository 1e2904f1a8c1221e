"""xsk_gpu_steer_dev without a GPU: the committed vectors against their generator, the identities of the Python spec
(tests/steer_spec.py), xsk_gpu_steer_table_prepare, the ABI surface, the argument checks of both device calls
(fabricated pointers, no device call reached), and xsk_steer.h compiled for the host under AddressSanitizer
(tests/c/test_steer.cpp)."""
import errno
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from tests import classify_wire as CW
from tests import steer_spec as SS
from tests.conftest import ROOT
from tests.v6_frames import mixed_batch6

GS = SS.GS
D, P, R = SS.XDP_DROP, SS.XDP_PASS, SS.XDP_REDIRECT
EINVAL, EEXIST = -errno.EINVAL, -errno.EEXIST
MAX_BATCH = 0xFFFFFF00


# ---- the fixture and the spec ------------------------------------------------------------------------------------

def test_fixture_is_what_the_generator_writes():
    doc = SS.golden()
    assert doc["frames"] == GS.vectors()
    assert doc["combos"] == [c[0] for c in GS.combos()] and len(doc["combos"]) == 8
    assert set(doc["frames"][0]["results"]) == {str(o) for o in GS.OPTION_WORDS} and 0 in GS.OPTION_WORDS
    names = [c["name"] for c in doc["frames"]]
    assert names[:len(CW.golden())] == [c["name"] for c in CW.golden()]  # the crafted frames of classify_wire.json
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "steer.json")) < 1 << 20


def _case(name):
    return next(c for c in SS.golden()["frames"] if c["name"] == name)


def test_fixture_pins_the_cases_the_spec_is_about():
    combos = SS.golden()["combos"]
    at = lambda c, opts, label: tuple(c["results"][str(opts)][combos.index(label)])  # noqa: E731
    # a table address, by family and tag depth; tags only under XSK_GPU_OPT_VLAN
    assert at(_case("steer_v4_table"), 0, "unicast/d0/b0") == (R, 2)
    assert at(_case("steer_v4_table"), 0x17, "wide/d255/b0") == (R, 1)
    assert at(_case("steer_v4_table"), 0x17, "wide/d255/b1") == (D, SS.PASS)      # port 1 unbound
    assert at(_case("steer_v6_table"), 0x17, "unicast/d255/b0") == (R, 2)
    assert at(_case("steer_v6_table"), 0x2, "unicast/d255/b0") == (P, SS.PASS)     # 0x86DD without OPT_IPV6
    assert at(_case("steer_v4_t2_table"), 0x12, "unicast/d255/b0") == (R, 2)
    assert at(_case("steer_v6_t1_table"), 0x12, "wide/d0/b0") == (R, 0)
    assert at(_case("steer_v4_t1_table"), 0x10, "unicast/d0/b0") == (P, SS.PASS)   # a tag without OPT_VLAN
    # not in the table: the default port, or the kernel stack
    assert at(_case("steer_v4_absent"), 0, "unicast/d0/b0") == (R, 0)
    assert at(_case("steer_v4_absent"), 0, "unicast/d255/b0") == (P, SS.PASS)
    for name in ("steer_v4_broadcast", "steer_v4_multicast", "steer_v6_multicast"):
        for o in (0x10, 0x17):
            assert at(_case(name), o, "unicast/d255/b0") == (P, SS.PASS), name
            assert at(_case(name), o, "unicast/d0/b0") == (R, 0), name
    assert at(_case("steer_v6_multicast"), 0x17, "wide/d255/b0") == (R, 40)        # a group in the table
    # the family is part of the key
    assert at(_case("steer_v4_prefix_of_v6_key"), 0x17, "wide/d255/b0") == (R, 5)
    assert at(_case("steer_v6_prefixed_by_v4_key"), 0x17, "wide/d255/b0") == (R, 6)
    assert at(_case("steer_v6_first_four_only"), 0x17, "wide/d255/b0") == (P, SS.PASS)
    # the destination as the frame's last bytes
    c = _case("steer_v4_dst_last_bytes")
    assert c["len"] == 34 and bytes.fromhex(c["frame"])[30:34] == GS.V4_OTHER
    for o in GS.OPTION_WORDS:
        assert at(c, o, "unicast/d255/b0") == (R, 2)
    assert at(_case("steer_v4_t2_dst_last_bytes"), 0x12, "unicast/d255/b0") == (R, 2)
    c = _case("steer_v6_dst_last_bytes")
    assert c["len"] == 14 + 40 and bytes.fromhex(c["frame"])[38:54] == GS.V6_OTHER
    assert at(c, 0x17, "unicast/d0/b0") == (D, SS.PASS)    # rule 5: the ICMPv6 header is cut, no lookup
    assert at(c, 0x2, "unicast/d0/b0") == (P, SS.PASS)     # rule 6
    assert at(_case("steer_v6_t2_dst_last_bytes"), 0x12, "wide/d0/b0") == (D, SS.PASS)


@functools.lru_cache(maxsize=None)
def _batch():
    umem, descs = mixed_batch6(600, 2048, seed=9400, offsets=True)
    descs = np.ascontiguousarray(descs, oracle.DESC_DTYPE)
    umem.setflags(write=False)
    return umem, descs


@pytest.mark.parametrize("bound", [True, False])
@pytest.mark.parametrize("opts", GS.OPTION_WORDS)
def test_degenerate_map_is_the_filter(opts, bound):
    """No table, default port 0, one port, *d_bound = target_bound: the actions and the list of the filter."""
    umem, descs = _batch()
    if opts == 0:  # the reference's traffic too: frames of 0 to 200 bytes
        um0 = np.zeros(2000 * 256, np.uint8)
        d0 = oracle.synth_batch(um0, 2000, 0, 256, seed=0x5EED57EE, mode=1, len_lo=0, len_hi=200)
        a_ref, r_ref = oracle.xdp_classify_batch(um0, d0, bound)
        got = SS.spec_steer_batch(um0, d0, 0, {}, 0, 1, int(bound))
        assert (got["actions"] == a_ref).all() and (got["out"] == r_ref).all() and got["off"][1] == len(r_ref)
        assert len(set(a_ref)) == (3 if bound else 2)
        a_ref, r_ref = oracle.xdp_classify_batch(umem, descs, bound)
    else:
        a_ref, r_ref = CW.spec_classify_batch(umem, descs, opts, bound)
    got = SS.spec_steer_batch(umem, descs, opts, {}, 0, 1, int(bound))
    assert (got["actions"] == a_ref).all()
    assert len(got["out"]) == len(r_ref) and (got["out"] == r_ref.view(oracle.DESC_DTYPE)).all()
    assert list(got["off"]) == [0, len(r_ref)]
    assert (got["ports"][a_ref == R] == 0).all() and (got["ports"][a_ref != R] == SS.PASS).all()


@pytest.mark.parametrize("n_ports,n_entries", [(1, 0), (3, 7), (64, 64), (64, 1024)])
@pytest.mark.parametrize("opts", [0, 0x17])
def test_offsets_partition_the_redirect_set_in_batch_order(opts, n_ports, n_entries):
    umem, descs = _batch()
    table = SS.sample_table(SS.destinations(umem, descs, opts), n_entries, n_ports, seed=n_entries)
    assert len(table) == n_entries
    for default_port, bound in ((0, SS.ALL_BOUND), (SS.PASS, SS.ALL_BOUND), (n_ports - 1, 0x5555555555555555)):
        ref = SS.spec_steer_batch(umem, descs, opts, table, default_port, n_ports, bound)
        off, red = ref["off"].astype(np.int64), ref["actions"] == R
        assert off[0] == 0 and (np.diff(off) >= 0).all() and off[n_ports] == red.sum() == len(ref["out"])
        assert (ref["ports"][~red] == SS.PASS).all() and (ref["ports"][red] < n_ports).all()
        assert sorted(ref["order"].tolist()) == np.nonzero(red)[0].tolist()
        for p in range(n_ports):
            seg = ref["order"][off[p]:off[p + 1]]
            assert (np.diff(seg) > 0).all() and (ref["ports"][seg] == p).all()
            assert (bound >> p) & 1 or len(seg) == 0
        # the same list from a stable sort of the REDIRECT frames by port
        idx = np.nonzero(red)[0]
        assert (ref["order"] == idx[np.argsort(ref["ports"][idx], kind="stable")]).all()
    if n_entries:  # a condition of the input: the table really spreads the frames
        ref = SS.spec_steer_batch(umem, descs, opts, table, 0, n_ports)
        assert len(set(ref["ports"][ref["actions"] == R].tolist())) > 1


@pytest.mark.parametrize("opts", [0, 0x10, 0x17])
def test_unicast_table_and_pass_leave_broadcast_and_multicast_to_the_stack(opts):
    umem, descs = _batch()
    umem = umem.copy()
    # some IPv4 echo requests to broadcast and multicast addresses among the random traffic
    bc = np.frombuffer(GS.W.build(daddr=GS.V4_BCAST), np.uint8)
    mc = np.frombuffer(GS.W.build(daddr=GS.V4_MCAST), np.uint8)
    descs = descs.copy()
    for i in range(0, 600, 50):
        f = bc if (i // 50) % 2 else mc
        a = int(descs[i]["addr"])
        umem[a:a + len(f)] = f
        descs[i]["len"] = len(f)
    keys = SS.destinations(umem, descs, opts)
    nonuni = [i for i, k in enumerate(keys) if k is not None and not SS.is_unicast(k)]
    assert len(nonuni) >= 12
    table = SS.sample_table(keys, 64, 8, seed=3, unicast_only=True)
    assert all(SS.is_unicast(k) for k in table)
    ref = SS.spec_steer_batch(umem, descs, opts, table, SS.PASS, 8)
    assert (ref["actions"][nonuni] == P).all() and (ref["actions"] == R).any()
    # with a default port they would be answered: this is the gap the PASS default closes
    ref0 = SS.spec_steer_batch(umem, descs, opts, table, 0, 8)
    assert (ref0["actions"][nonuni] == R).all()


# ---- xsk_gpu_steer_table_prepare ---------------------------------------------------------------------------------

def _key17(e):
    return bytes([int(e["family"])]) + e["addr"].tobytes()


def _random_entries(n, seed):
    rng = np.random.default_rng(seed)
    e = np.zeros(n, SS.ENTRY_DTYPE)
    fam = rng.choice([4, 6], n)
    e["family"] = fam
    e["port"] = rng.integers(0, 64, n)
    # few distinct leading bytes, so that the order is decided late in the key; a counter makes the keys distinct
    e["addr"][:, 0] = rng.integers(0, 3, n)
    cnt = np.arange(n, dtype=np.uint32)
    rng.shuffle(cnt)
    e["addr"][:, 2] = cnt >> 8
    e["addr"][:, 3] = cnt & 0xFF
    six = fam == 6
    e["addr"][six, 4:] = rng.integers(0, 256, (int(six.sum()), 12))
    return e


@pytest.mark.parametrize("n", [0, 1, 2, 1023, 1024])
def test_table_prepare_sorts_by_the_17_byte_key(n):
    import xsknet_amd as X
    assert X.STEER_ENTRY_DTYPE == SS.ENTRY_DTYPE
    e = _random_entries(n, seed=n)
    got = X.steer_table_prepare(e)
    want = sorted(range(n), key=lambda i: _key17(e[i]))
    assert got.tobytes() == e[want].tobytes()
    keys = [_key17(x) for x in got]
    assert all(a < b for a, b in zip(keys, keys[1:]))
    assert X.lib().xsk_gpu_steer_table_prepare(None, 0) == 0


def test_table_prepare_refuses():
    import xsknet_amd as X
    f = X.lib().xsk_gpu_steer_table_prepare
    good = _random_entries(8, seed=8)

    def rc(e):
        e = np.ascontiguousarray(e)
        before = e.tobytes()
        r = f(e.ctypes.data, len(e))
        return r, e.tobytes() == before

    assert rc(good.copy())[0] == 0
    assert f(_random_entries(1025, 1).ctypes.data, 1025) == EINVAL       # n > XSK_GPU_STEER_MAX_ENTRIES
    assert f(None, 1) == EINVAL
    for fam in (0, 5, 7, 255):
        e = good.copy()
        e[3]["family"] = fam
        assert rc(e) == (EINVAL, True), fam
    for k in range(4, 16):                                               # family 4: addr[4..16) zero
        e = good.copy()
        e[5]["family"] = 4
        e[5]["addr"][4:] = 0
        assert rc(e.copy())[0] == 0
        e[5]["addr"][k] = 1
        assert rc(e) == (EINVAL, True), k
    for port in (64, 65, 255):
        e = good.copy()
        e[0]["port"] = port
        assert rc(e) == (EINVAL, True), port
    e = good.copy()
    e[7]["port"] = 63
    assert rc(e)[0] == 0
    for k in range(6):
        e = good.copy()
        e[2]["pad"][k] = 1
        assert rc(e) == (EINVAL, True), k
    e = good.copy()                                                      # the same key twice, ports differ
    e[6] = e[1]
    e[6]["port"] = (int(e[1]["port"]) + 1) % 64
    assert rc(e)[0] == EEXIST
    e = _random_entries(1024, 2)
    e[1000]["addr"], e[1000]["family"] = e[17]["addr"], e[17]["family"]
    assert rc(e)[0] == EEXIST
    with pytest.raises(X.XskGpuError):
        X.steer_table_prepare(e)
    # the same address in both families is two keys
    e = np.zeros(2, SS.ENTRY_DTYPE)
    e["family"] = [6, 4]
    e["addr"][:, :4] = [10, 0, 0, 2]
    assert rc(e)[0] == 0 and list(e["family"]) == [4, 6]


# ---- the ABI surface ---------------------------------------------------------------------------------------------

def _header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xsk_gpu.h")).read(), flags=re.S)
    assert re.search(r"#define\s+XSK_GPU_ABI_VERSION\s+1\b", src)
    assert re.search(r"#define\s+XSK_GPU_OPT_MASK\s+0x17u\b", src)  # additive: no new version, no new option bits
    return src


def _decl(ret, name):
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)", _header())
    assert m, f"{name} is not declared"
    return re.sub(r"\s+", " ", m.group(1)).strip()


STEER_ARGS = ("const struct xsk_gpu_desc* d_descs, uint32_t n, uint32_t opts, const struct xsk_gpu_steer_entry* d_table, "
              "uint32_t n_entries, uint32_t default_port, uint32_t n_ports, const uint64_t* d_bound, uint8_t* d_actions, "
              "uint8_t* d_ports, struct xsk_gpu_desc* d_out, uint32_t* d_off, ")


def test_header_declares_and_library_exports_the_entry_points():
    import xsknet_amd as X
    h = _header()
    assert re.search(r"#define\s+XSK_GPU_STEER_MAX_PORTS\s+64u", h)
    assert re.search(r"#define\s+XSK_GPU_STEER_MAX_ENTRIES\s+1024u", h)
    assert re.search(r"#define\s+XSK_GPU_STEER_PASS\s+0xFFu", h)
    assert (X.STEER_MAX_PORTS, X.STEER_MAX_ENTRIES, X.STEER_PASS) == (64, 1024, 0xFF)
    assert _decl("int", "xsk_gpu_steer_table_prepare") == "struct xsk_gpu_steer_entry* entries, uint32_t n"
    assert _decl("size_t", "xsk_gpu_steer_workspace_size") == "uint32_t n, uint32_t n_ports"
    assert _decl("int", "xsk_gpu_steer_dev") == \
        "const void* d_umem, uint64_t umem_size, " + STEER_ARGS + "void* d_workspace, void* stream"
    assert _decl("int", "xsk_gpu_ingress_steer_dev") == \
        "void* d_umem, uint64_t umem_size, " + STEER_ARGS + \
        "uint8_t* d_verdicts, struct xsk_gpu_rec* d_recs, struct xsk_gpu_stats* d_stats, void* d_workspace, void* stream"
    out = subprocess.run(["nm", "-D", "--defined-only", X.LIB_PATH], capture_output=True, text=True, check=True)
    for name in ("xsk_gpu_steer_table_prepare", "xsk_gpu_steer_workspace_size", "xsk_gpu_steer_dev",
                 "xsk_gpu_ingress_steer_dev"):
        assert re.search(r"\bT " + name + r"\b", out.stdout)
        assert hasattr(X.lib(), name) and name in X._SIGS
    assert not re.search(r"\bT xsk_gpu__\w*steer", out.stdout)  # no new hook
    assert len(X._SIGS["xsk_gpu_steer_dev"][0]) == 16 and len(X._SIGS["xsk_gpu_ingress_steer_dev"][0]) == 19
    for f in (X.steer_table_prepare, X.steer_workspace_size, X.steer_dev, X.ingress_steer_dev):
        assert callable(f)


def test_entry_struct_layout_matches_the_dtype():
    import xsknet_amd as X
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "xsk_gpu.h"
#define O(f) printf(#f " %zu\n", offsetof(struct xsk_gpu_steer_entry, f))
int main(void){ printf("size %zu\n", sizeof(struct xsk_gpu_steer_entry)); O(addr); O(family); O(port); O(pad); return 0; }
'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "p.c")
        open(c, "w").write(probe)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(td, "p"), c],
                       check=True)
        out = subprocess.run([os.path.join(td, "p")], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "size 24" and X.STEER_ENTRY_DTYPE.itemsize == 24
    offs = dict(line.split() for line in out[1:] if line)
    for f in X.STEER_ENTRY_DTYPE.names:
        assert int(offs[f]) == X.STEER_ENTRY_DTYPE.fields[f][1], f


def test_workspace_size():
    import xsknet_amd as X
    ws = X.steer_workspace_size
    assert ws(1 << 20, 64) == 1 << 20          # 1 MiB at 1 M frames and 64 ports
    assert ws(1, 1) == 4 and ws(256, 1) == 4 and ws(257, 1) == 8
    assert ws(257, 3) == 24 and ws(4097, 64) == 17 * 64 * 4
    assert ws(0, 64) == 0
    assert ws(MAX_BATCH, 64) == ((MAX_BATCH + 255) // 256) * 64 * 4


def test_argument_validation_needs_no_gpu():
    """Every -EINVAL of include/xsk_gpu.h, for both calls, with pointers that belong to nobody: a device call that
    touched them, or any HIP call on a machine without a GPU, would not return -EINVAL."""
    import xsknet_amd as X
    um, de, ta, bo, ac, po, ou, of, ws, ve, re_, st = (0x10000 * k for k in range(1, 13))
    size = 1 << 20

    def steer(umem=um, usize=size, descs=de, n=300, opts=0x17, table=ta, n_entries=8, default=0, n_ports=4, bound=bo,
              actions=ac, ports=po, out=ou, off=of, w=ws):
        return X.lib().xsk_gpu_steer_dev(umem, usize, descs, n, opts, table, n_entries, default, n_ports, bound, actions,
                                         ports, out, off, w, None)

    def ingress(umem=um, usize=size, descs=de, n=300, opts=0x17, table=ta, n_entries=8, default=0, n_ports=4, bound=bo,
                actions=ac, ports=po, out=ou, off=of, w=ws, verd=ve, recs=re_, stats=st):
        return X.lib().xsk_gpu_ingress_steer_dev(umem, usize, descs, n, opts, table, n_entries, default, n_ports, bound,
                                                 actions, ports, out, off, verd, recs, stats, w, None)

    for f in (steer, ingress):
        for n in (300, 0):  # the rules hold for an empty batch too
            # the filter's rules
            assert f(n=n, opts=0x8) == EINVAL and f(n=n, opts=0x20) == EINVAL and f(n=n, opts=0x117) == EINVAL
            assert f(n=n, umem=None) == EINVAL
            assert f(n=n, descs=None) == EINVAL
            assert f(n=n, actions=None) == EINVAL
            assert f(n=n, w=None) == EINVAL
            for mis in (1, 2, 4, 8):
                assert f(n=n, descs=de + mis) == EINVAL
                assert f(n=n, out=ou + mis) == EINVAL
            # the map
            for bad in (0, 65, 0xFF, 0xFFFFFFFF):
                assert f(n=n, n_ports=bad, default=0) == EINVAL, bad
            for bad in (4, 5, 63, 64, 0xFE, 0x100, 0x1FF, 0xFFFFFFFF):
                assert f(n=n, default=bad) == EINVAL, bad
            assert f(n=n, n_ports=64, default=64) == EINVAL
            assert f(n=n, n_entries=1025) == EINVAL and f(n=n, n_entries=0xFFFFFFFF) == EINVAL
            assert f(n=n, table=None) == EINVAL
            for mis in (1, 2, 4):
                assert f(n=n, table=ta + mis) == EINVAL
                assert f(n=n, bound=bo + mis) == EINVAL
            for mis in (1, 2, 3):
                assert f(n=n, off=of + mis) == EINVAL
            assert f(n=n, ports=None) == EINVAL
            assert f(n=n, out=None) == EINVAL        # d_off without d_out
            assert f(n=n, off=None) == EINVAL        # d_out without d_off
        for big in (MAX_BATCH + 1, 0xFFFFFFFF):
            assert f(n=big) == EINVAL
    # both NULL is the actions-and-ports form of the filter, but not of the ingress call
    assert ingress(out=None, off=None) == EINVAL and ingress(n=0, out=None, off=None) == EINVAL
    # the transform's rules, in front of the filter's launches
    assert ingress(umem=um + 8) == EINVAL
    assert ingress(usize=size + 8) == EINVAL
    assert ingress(usize=1 << 48) == EINVAL
    for mis in (1, 2, 4, 8):
        assert ingress(recs=re_ + mis) == EINVAL
        assert ingress(n=0, recs=re_ + mis) == EINVAL


def test_the_checks_stand_in_front_of_the_first_device_call():
    src = open(os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_steer.hip")).read()
    launch = src[src.index("int steer_launch("):src.index("}  // namespace")]
    assert "-EINVAL" not in launch  # nothing is refused once launches have begun
    for name in ("int xsk_gpu_steer_dev(", "int xsk_gpu_ingress_steer_dev("):
        body = src[src.index(name):]
        assert body.index("return -EINVAL") < body.index("steer_launch(")
    body = src[src.index("int xsk_gpu_ingress_steer_dev("):]
    # the transform's arguments are checked by a call with a bound of 0 frames, which launches nothing
    m = re.search(r"xsk_gpu_echo_dev_indirect\(d_umem, umem_size, d_out, d_total, 0, opts", body)
    assert m and m.start() < body.index("steer_launch(")
    ind = open(os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_echo_indirect.hip")).read()
    ind = ind[ind.index("int xsk_gpu_echo_dev_indirect("):]
    assert ind.index("return -EINVAL") < ind.index("if (n_max == 0) return 0;") < ind.index("indirect_launch(")


def test_shared_header_on_the_host_under_address_sanitizer():
    """tests/c/test_steer.cpp: xsk_steer.h's decision on frames that end flush with their heap allocation, its search on
    tables of exactly n entries (0, 1, 2, 1023, 1024; prepared and not), and the three stages replayed lane by lane
    into a list of exactly the REDIRECT count, against a stable sort by port."""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "t")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "c", "test_steer.cpp")], check=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    assert "steer ok" in res.stdout
