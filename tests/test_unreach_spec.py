"""The port-unreachable responder without a GPU (xsk_gpu_unreach_dev, xsk_gpu_unreach_serve_dev; include/xsk_gpu.h
"Port-unreachable responder"): the two restatements of the rule (tests/unreach_spec.py, which parses, and
tests/golden/make_unreach_golden.py, which builds) held against each other and against errors written out by hand; the
properties of the errors; the serve loop's identities and its budget; the ABI surface and the export table; every
-EINVAL of the two calls with fabricated pointers (no device call reached); and xsk_unreach.h compiled for the host
under AddressSanitizer (tests/c/test_unreach.cpp)."""
import errno
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from tests import rx_dev_spec as RS
from tests import unreach_frames as UF
from tests import unreach_spec as US
from tests.conftest import ROOT
from tests.test_rx_dev_spec import MAX_BATCH, _bad_rings, _decl, _header, _ref, _ring, _struct
from tests.test_rx_steer_spec import _ports
from tests.test_tx_complete_rings_spec import _exports

EINVAL = -errno.EINVAL
NAMES = ("xsk_gpu_unreach_dev", "xsk_gpu_unreach_serve_dev")
SRC = os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_unreach.hip")
BIG = 1 << 62


def _same(got, frame, want):
    v, port, reply, rlen = got
    assert v == want["verdict"] and port == want["port"], (got[:2], want)
    assert ((reply + frame[rlen:]).hex() if reply is not None else None) == want.get("reply")
    assert rlen == want.get("reply_len", 0)


def _decide(frame, room, opts, open_ports=UF.OPEN):
    return US.decide(frame, opts, UF.table(), UF.N_PORTS, UF.BOUND, open_ports, BIG if room is None else room)


# ---- the two restatements ----------------------------------------------------------------------------------------

def test_the_golden_file_is_what_its_generator_writes():
    doc, G = UF.golden(), UF.G
    assert doc["opts"] == [0, 0x2, 0x10, 0x12, 0x17] and doc["n_ports"] == UF.N_PORTS and int(doc["bound"], 16) == UF.BOUND
    assert doc["open_ports"] == list(G.OPEN_PORTS)
    assert len(doc["cases"]) == 3 * len(G.CASES) and {c["tags"] for c in doc["cases"]} == {0, 1, 2}
    for c, (case, tags) in zip(doc["cases"], ((case, tags) for case in G.CASES for tags in G.TAGS)):
        name, family, (frame, reply), verdict, room = case
        f, r = frame(tags), G.room_of(reply, room, tags)
        assert c["name"] == name and c["frame"] == f.hex() and c["room"] == r
        for o in UF.OPTS:
            assert c["expect"]["0x%x" % o] == G.expect(family, verdict, reply, tags, o, f, r)
    assert [dict(family=e[0], addr=e[1].hex(), port=e[2], mac=e[3].hex()) for e in G.TABLE] == doc["table"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "unreach.json")) < 1 << 20


@pytest.mark.parametrize("opts", UF.OPTS)
def test_both_restatements_agree_on_every_golden_case(opts):
    seen = set()
    for frame, room, want in UF.golden_frames(opts):
        got = _decide(frame, room, opts)
        _same(got, frame, want)
        seen.add(got[0])
    # every verdict of the list call under the dual-stack option words; without XSK_GPU_OPT_IPV6 no IPv6 packet is looked at
    assert seen == (set(range(8)) if opts & US.OPT_IPV6 else set(range(8)) - {US.UNREACH6})


def test_every_rule_letter_has_a_case():
    names = {c[0] for c in UF.G.CASES}
    for need in ("udp4_cut_header", "udp4_version", "udp4_ihl_4", "udp4_cut_options", "tcp4",                      # 3a
                 "udp4_tl_short", "udp4_tl_overrun", "udp4_bad_header_sum",                                        # 3b
                 "udp4_later_fragment", "udp4_link_broadcast", "udp4_multicast", "udp4_source_zero",
                 "udp4_source_multicast", "udp4_source_loopback",                                                  # 3c
                 "udp4_stranger", "udp4_port_high", "udp4_port_unbound", "udp4_open_port", "udp4_one_byte_short",  # 3d-f
                 "udp4_probe", "udp4_ihl_15", "udp4_fits_to_the_byte", "udp4_padded", "udp4_empty",                # 3g
                 "udp6_cut_header", "udp6_version", "tcp6", "udp6_hop_by_hop",                                     # 4a
                 "udp6_pl_7", "udp6_pl_overrun", "udp6_zero_udp_sum",                                              # 4b
                 "udp6_link_multicast", "udp6_multicast", "udp6_source_unspecified", "udp6_source_multicast",      # 4c
                 "udp6_stranger", "udp6_port_unbound", "udp6_open_port", "udp6_one_byte_short",                    # 4d-e
                 "udp6_probe", "udp6_empty", "udp6_pl_1191", "udp6_pl_1192", "udp6_pl_1193", "udp6_padded",        # 4f
                 "tag_cut", "arp_request"):                                                                        # 2, 5
        assert need in names, need


def _batch(n, opts, seed):
    batch = UF.random_frames(n, opts, seed)
    umem, descs = UF.layout([f for f, _, _ in batch], [r for _, r, _ in batch])
    return batch, umem, descs


@pytest.mark.parametrize("opts,seed", [(0x17, 11), (0x12, 12), (0x17, 13)])
def test_both_restatements_agree_on_seeded_random_batches(opts, seed):
    batch, umem, descs = _batch(400, opts, seed)
    before = umem.copy()
    stats = dict.fromkeys(US.STATS_KEYS, 0)
    verdicts, ports, rlens = US.spec_unreach(umem, descs, len(descs), opts, UF.table(), UF.N_PORTS, UF.BOUND, UF.OPEN,
                                             UF.CHUNK, stats)
    UF.check_condition(verdicts)
    want_umem = before.copy()
    for i, (f, _, want) in enumerate(batch):
        assert (verdicts[i], ports[i], rlens[i]) == (want["verdict"], want["port"], want.get("reply_len")), i
        if "reply" in want:
            a = int(descs[i]["addr"])
            r = bytes.fromhex(want["reply"])
            want_umem[a:a + len(r)] = np.frombuffer(r, np.uint8)
    assert (umem == want_umem).all()  # the errors, and every byte between the frames as it was
    assert stats["seen"] == 400 and stats["unreach4"] == verdicts.count(US.UNREACH4) and stats["limited"] == 0
    assert stats["unreach6"] == verdicts.count(US.UNREACH6) and stats["reply_bytes"] == sum(r for r in rlens if r)


# ---- the errors ---------------------------------------------------------------------------------------------------

def _replies(kind):
    for opts in UF.OPTS:
        for frame, room, want in UF.golden_frames(opts):
            if want["verdict"] == kind:
                yield opts, frame, bytes.fromhex(want["reply"]), want["reply_len"]


def _l3(frame, opts):
    l3 = 14
    while opts & 2 and frame[l3 - 2:l3] in (b"\x81\x00", b"\x88\xa8"):
        l3 += 4
    return l3


def test_every_error_sums_to_ffff_by_the_oracles_sum():
    n4 = n6 = 0
    for opts, frame, reply, rlen in _replies(US.UNREACH4):
        l3 = _l3(frame, opts)
        buf = np.frombuffer(reply[l3:rlen], np.uint8).copy()
        assert oracle.fold_sum(buf, 0, 20) == 0xFFFF and oracle.fold_sum(buf, 20, len(buf)) == 0xFFFF
        q = rlen - l3 - 28
        assert reply[l3 + 28:rlen] == frame[l3:l3 + q] and q == 4 * (frame[l3] & 15) + 8
        assert reply[l3 + 12:l3 + 16] == frame[l3 + 16:l3 + 20] and reply[l3 + 16:l3 + 20] == frame[l3 + 12:l3 + 16]
        assert reply[rlen:] == frame[rlen:] and reply[12:l3] == frame[12:l3] and reply[:6] == frame[6:12]
        n4 += 1
    for opts, frame, reply, rlen in _replies(US.UNREACH6):
        l3 = _l3(frame, opts)
        q = rlen - l3 - 48
        src, dst, msg = reply[l3 + 8:l3 + 24], reply[l3 + 24:l3 + 40], reply[l3 + 40:rlen]
        buf = np.frombuffer(US.pseudo(src, dst, 8 + q) + msg + bytes(len(msg) & 1), np.uint8).copy()
        assert oracle.fold_sum(buf, 0, len(buf)) == 0xFFFF
        assert q == min(40 + int.from_bytes(frame[l3 + 4:l3 + 6], "big"), 1232) and rlen - l3 <= 1280
        assert msg[8:] == frame[l3:l3 + q] and src == frame[l3 + 24:l3 + 40] and dst == frame[l3 + 8:l3 + 24]
        assert reply[rlen:] == frame[rlen:] and reply[12:l3] == frame[12:l3] and reply[:6] == frame[6:12]
        n6 += 1
    assert n4 >= 30 and n6 >= 30


def test_an_error_fed_back_is_none():
    """ICMP and ICMPv6 are not UDP: no error is ever sent about an error (RFC 1122 §3.2.2, RFC 4443 §2.4(e))."""
    n = 0
    for kind in US.REPLIES:
        for opts, frame, reply, rlen in _replies(kind):
            for o in UF.OPTS:
                assert _decide(reply[:rlen], None, o)[0] == US.NONE
            n += 1
    assert n >= 60


def test_both_restatements_against_errors_written_out_by_hand():
    """Two errors as byte literals, worked out on paper.  192.0.2.77 (02:aa:bb:cc:dd:01) sends an empty datagram to
    192.0.2.1 port 33434 (0x829a), owned by 02:00:00:00:0a:03 on port 3.  The fresh header: 4500 + 0038 + 4000 + 4001 +
    c000 + 0201 + c000 + 024d = 24987 -> 4989 -> complement b676.  The message: 0303, the quoted header (it sums to ffff),
    9c40 + 829a + 0008 + 5cb4 = 17b96; 0303 + ffff + 17b96 = 27e98 -> 7e9a -> complement 8165.
    2001:db8::77 sends the same to 2001:db8::fe, owned by 02:00:00:00:06:fe on port 7.  Each address stands in the
    pseudo-header and in the quote: 2 x (2001 + 0db8 + 00fe + 2001 + 0db8 + 0077) = b9ce; 0038 + 003a = 0072; 0104; the
    quoted header's first words 60b5 + 4321 + 0008 + 113d = b51b; the datagram 9c40 + 829a + 0008 + 841c = 1a2fe; together
    3135d -> 1360 -> complement ec9f."""
    e4 = bytes.fromhex("02aabbccdd01" "020000000a03" "0800"
                       "4500" "0038" "0000" "4000" "40" "01" "b676" "c0000201" "c000024d"
                       "0303" "8165" "00000000"
                       "4510001cbeef40003911fe82c000024dc0000201" "9c40829a00085cb4")
    e6 = bytes.fromhex("02aabbccdd01" "0200000006fe" "86dd"
                       "60000000" "0038" "3a" "40"
                       "20010db80000000000000000000000fe" "20010db8000000000000000000000077"
                       "0104" "ec9f" "00000000"
                       "60b543210008113d" "20010db8000000000000000000000077" "20010db80000000000000000000000fe"
                       "9c40829a0008841c")
    by_name = {(c["name"], c["tags"]): c for c in UF.golden()["cases"]}
    for name, hand, verdict, port in (("udp4_empty", e4, US.UNREACH4, 3), ("udp6_empty", e6, US.UNREACH6, 7)):
        c = by_name[(name, 0)]
        want = c["expect"]["0x17"]
        assert want["reply"] == hand.hex() and want["verdict"] == verdict and want["port"] == port
        assert want["reply_len"] == len(hand) > len(c["frame"]) // 2  # the error is longer than the request
        assert _decide(bytes.fromhex(c["frame"]), None, 0x17) == (verdict, port, hand, len(hand))


def test_the_open_map_the_room_and_the_umems_end():
    by_name = {(c["name"], c["tags"]): c for c in UF.golden()["cases"]}
    f = bytes.fromhex(by_name[("udp4_probe", 0)]["frame"])
    assert _decide(f, None, 0)[0] == US.UNREACH4 and _decide(f, None, 0, None)[0] == US.UNREACH4
    assert _decide(f, None, 0, {33434})[0] == US.LEFT and _decide(f, None, 0, set(range(65536)))[0] == US.LEFT
    m = US.open_map({0, 7, 8, 65535})
    assert (m[0], m[1], m[8191], int(m.sum())) == (0x81, 1, 0x80, 0x81 + 1 + 0x80)
    R = 14 + 28 + 28
    assert _decide(f, R, 0)[0] == US.UNREACH4 and _decide(f, R - 1, 0)[0] == US.NO_ROOM
    # room_at: the chunk's end and the UMEM's end
    assert US.room_at(2048 + 5, 1 << 20, 2048) == 2043 and US.room_at(2048 + 5, 2048 + 60, 2048) == 55
    assert US.room_at(4096, 1 << 20, 4096) == 4096


# ---- the serve loop's own identities -------------------------------------------------------------------------------

def _serve_state(batch, n_ports, up_size=64, tx_size=8, rest_size=64, start=0xFFFFFFF0):
    umem, descs = UF.layout([f for f, _, _ in batch], [r for _, r, _ in batch])
    up = RS.RingState(np.zeros(up_size, oracle.DESC_DTYPE), start, start)
    up.produce(descs)
    txs = [RS.RingState(np.zeros(tx_size, oracle.DESC_DTYPE), start + p, start + p) for p in range(n_ports)]
    rest = RS.RingState(np.zeros(rest_size, oracle.DESC_DTYPE), 5, 5)
    return umem, descs, up, txs, rest


def test_the_serve_loop_is_the_list_rule_entry_by_entry_and_stops_without_losing_a_frame():
    batch = UF.random_frames(60, 0x17, 21)
    t = UF.table()
    umem, descs, up, txs, rest = _serve_state(batch, UF.N_PORTS, tx_size=64)
    ref = umem.copy()
    verdicts, ports, rlens = US.spec_unreach(ref, descs, 60, 0x17, t, UF.N_PORTS, UF.BOUND, UF.OPEN, UF.CHUNK)
    got = []
    res, left = US.spec_serve(umem, up, txs, rest, 1024, 0x17, t, UF.BOUND, UF.OPEN, UF.CHUNK, None, verdicts_out=got)
    assert got == verdicts and (umem == ref).all() and res["consumed"] == 60 and res["backlog"] == 0 and left is None
    assert res["rest"] == sum(r is None for r in rlens) and up.used() == 0 and res["limited"] == 0
    for p, tx in enumerate(txs):
        mine = [i for i in range(60) if ports[i] == p]
        assert tx.used() == len(mine)
        for k, i in enumerate(mine):  # batch order within a port; the error's descriptor
            e = tx.entries[tx.slot(tx.cons + k)]
            assert (int(e["addr"]), int(e["len"]), int(e["options"])) == (int(descs[i]["addr"]), rlens[i], 0)
    # a TX ring of two entries stops the call in the middle: the frames behind it are untouched
    umem, descs, up, txs, rest = _serve_state(batch, UF.N_PORTS, tx_size=2)
    before = umem.copy()
    res, _ = US.spec_serve(umem, up, txs, rest, 1024, 0x17, t, UF.BOUND, UF.OPEN, UF.CHUNK, None)
    c = res["consumed"]
    assert 0 < c < 60 and res["backlog"] == 60 - c and up.used() == 60 - c
    first_behind = int(descs[c]["addr"])
    assert (umem[first_behind:] == before[first_behind:]).all()
    assert ports[c] != US.NO_PORT and txs[ports[c]].free() == 0  # it stopped at an error whose ring is full


@pytest.mark.parametrize("seed", [31, 32])
def test_the_budget_limits_the_errors_and_every_verdict_occurs(seed):
    batch = UF.random_frames(400, 0x17, seed)
    t = UF.table()
    umem, descs, up, txs, rest = _serve_state(batch, UF.N_PORTS, up_size=512, tx_size=512, rest_size=512)
    ref = umem.copy()
    verdicts, ports, rlens = US.spec_unreach(ref, descs, 400, 0x17, t, UF.N_PORTS, UF.BOUND, UF.OPEN, UF.CHUNK)
    eligible = [i for i, v in enumerate(verdicts) if v in US.REPLIES]
    budget = len(eligible) - 7
    got = []
    stats = dict.fromkeys(US.STATS_KEYS, 0)
    res, left = US.spec_serve(umem, up, txs, rest, 1024, 0x17, t, UF.BOUND, UF.OPEN, UF.CHUNK, budget, stats, got)
    UF.check_condition(got, limited=True)
    assert left == 0 and res["limited"] == 7 == stats["limited"] and res["unreach4"] + res["unreach6"] == budget
    assert [i for i, v in enumerate(got) if v == US.LIMITED] == eligible[-7:]  # the last seven that were due
    for i in eligible[-7:]:  # a LIMITED frame is untouched and goes to rest whole
        a, n = int(descs[i]["addr"]), int(descs[i]["len"])
        assert bytes(umem[a:a + n]) == batch[i][0]
    assert res["rest"] == 400 - budget and stats["reply_bytes"] == sum(rlens[i] for i in eligible[:-7])
    # budget 0, a budget of exactly the eligible count, and more: the word afterwards
    for b, want_left, want_lim in ((0, 0, len(eligible)), (len(eligible), 0, 0), (len(eligible) + 5, 5, 0),
                                   (0xFFFFFFFF, 0xFFFFFFFF - len(eligible), 0)):
        umem, descs, up, txs, rest = _serve_state(batch, UF.N_PORTS, up_size=512, tx_size=512, rest_size=512)
        res, left = US.spec_serve(umem, up, txs, rest, 1024, 0x17, t, UF.BOUND, UF.OPEN, UF.CHUNK, b)
        assert (left, res["limited"]) == (want_left, want_lim) and res["consumed"] == 400
        if b == 0:
            assert (umem == _serve_state(batch, UF.N_PORTS)[0]).all() and res["rest"] == 400


# ---- the ABI surface ------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_entry_points():
    import xsknet_amd as X
    R, E = "const struct xsk_gpu_ring_dev*", "const struct xsk_gpu_neigh_entry*"
    assert _decl("int", "xsk_gpu_unreach_dev") == (
        "void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, const uint32_t* d_n, uint32_t n_max, "
        f"uint32_t opts, {E} d_table, uint32_t n_entries, uint32_t n_ports, const uint64_t* d_bound, "
        "const uint8_t* d_open, uint32_t chunk_size, uint8_t* d_uverdicts, uint8_t* d_uports, uint32_t* d_reply_len, "
        "struct xsk_gpu_unreach_stats* d_ustats, void* stream")
    assert _decl("int", "xsk_gpu_unreach_serve_dev") == (
        f"void* d_umem, uint64_t umem_size, {R} up, {R} tx , uint32_t n_ports, {R} rest, uint32_t max, uint32_t opts, "
        f"{E} d_table, uint32_t n_entries, const uint64_t* d_bound, const uint8_t* d_open, uint32_t chunk_size, "
        "uint32_t* d_budget, struct xsk_gpu_unreach_stats* d_ustats, struct xsk_gpu_unreach_result* d_res, void* stream")
    assert _struct("xsk_gpu_unreach_stats") == "uint64_t seen, unreach4, unreach6, reply_bytes, limited; uint64_t reserved[3];"
    for k, name in enumerate(X.UNREACH_VERDICTS):
        assert re.search(r"XSK_GPU_UNREACH_%s = %d\b" % (name, k), _header()) and getattr(X, "UNREACH_" + name) == k
        assert getattr(US, name) == k
    assert len(X.UNREACH_VERDICTS) == 9
    exported = _exports()
    for name in NAMES:
        assert name in exported and hasattr(X.lib(), name) and name in X._SIGS, name
    assert [len(X._SIGS[n][0]) for n in NAMES] == [17, 17]
    for f in ("UNREACH_STATS_DTYPE", "UNREACH_RESULT_DTYPE", "UNREACH_VERDICTS", "unreach_dev", "unreach_serve_dev"):
        assert f in X.__all__
    assert X.lib().xsk_gpu_abi_version() == 1 and re.search(r"#define\s+XSK_GPU_ABI_VERSION\s+1\b", _header())


def test_the_library_gained_exactly_the_two_names():
    src = open(SRC).read()
    pub = src[src.index('extern "C" {'):]
    assert sorted(re.findall(r"^(?:int|size_t) (\w+)\(", pub, re.M)) == sorted(NAMES)
    # nothing else of the feature is exported: no other "unreach", no ur_* helper
    assert sorted(s for s in _exports() if "unreach" in s.lower() or re.search(r"(^|_)ur_", s)) == sorted(NAMES)
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "xsk_unreach.o" in mk and "xsk_unreach.h" in mk and "xsk_unreach_device.h" in mk
    # the search is xsk_neigh.h's, shared through the header: no second text of it
    for name in ("xsk_unreach.h", "xsk_unreach.hip", "xsk_unreach_device.h"):
        code = open(os.path.join(ROOT, "xsknet_amd", "csrc", name)).read()
        assert "while (lo < hi)" not in code
    assert "ng_lookup(tab, n_entries, key)" in open(os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_unreach.h")).read()


def test_struct_layouts():
    import xsknet_amd as X
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "xsk_gpu.h"
#define O(s, f) printf(#s "." #f " %zu\n", offsetof(struct s, f))
int main(void){
 printf("sizes %zu %zu\n", sizeof(struct xsk_gpu_unreach_stats), sizeof(struct xsk_gpu_unreach_result));
 O(xsk_gpu_unreach_stats, seen); O(xsk_gpu_unreach_stats, unreach4); O(xsk_gpu_unreach_stats, unreach6);
 O(xsk_gpu_unreach_stats, reply_bytes); O(xsk_gpu_unreach_stats, limited); O(xsk_gpu_unreach_stats, reserved);
 O(xsk_gpu_unreach_result, consumed); O(xsk_gpu_unreach_result, unreach4); O(xsk_gpu_unreach_result, unreach6);
 O(xsk_gpu_unreach_result, rest); O(xsk_gpu_unreach_result, backlog); O(xsk_gpu_unreach_result, limited);
 O(xsk_gpu_unreach_result, reserved);
 return 0; }
'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "p.c")
        open(c, "w").write(probe)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(td, "p"), c], check=True)
        out = subprocess.run([os.path.join(td, "p")], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "sizes 64 32"
    offs = dict(line.split() for line in out[1:] if line)
    for dt, name in ((X.UNREACH_STATS_DTYPE, "xsk_gpu_unreach_stats"), (X.UNREACH_RESULT_DTYPE, "xsk_gpu_unreach_result")):
        for f in dt.names:
            assert int(offs[f"{name}.{f}"]) == dt.fields[f][1], (name, f)
    assert X.UNREACH_STATS_DTYPE.names[:5] == US.STATS_KEYS and X.UNREACH_RESULT_DTYPE.names[:6] == US.RESULT_KEYS


# ---- the argument rules ---------------------------------------------------------------------------------------------

BAD_CHUNKS = (0, 1, 1024, 2047, 2049, 3072, (1 << 20) + 1, 1 << 21, 0x80000000, 0xFFFFFFFF)


def test_argument_validation_of_the_list_call_needs_no_gpu():
    import xsknet_amd as X
    L = X.lib()
    um, de, dn, tb, bd, op, uv, upo, rl, st = (0x600000, 0x500000, 0x510000, 0x520000, 0x530000, 0x590000, 0x540000,
                                               0x550000, 0x560000, 0x570000)

    def call(um=um, de=de, dn=dn, n=64, opts=0, tb=tb, ne=4, np_=8, bd=bd, op=op, ch=2048, uv=uv, upo=upo, rl=rl, st=st):
        return L.xsk_gpu_unreach_dev(um, 1 << 20, de, dn, n, opts, tb, ne, np_, bd, op, ch, uv, upo, rl, st, None)

    for n in (0, 64, 1300):  # the empty call refuses alike
        assert call(n=n, um=None) == EINVAL and call(n=n, de=None) == EINVAL and call(n=n, uv=None) == EINVAL
        assert call(n=n, upo=None) == EINVAL
        for mis in (1, 2, 4, 8):
            assert call(n=n, de=de + mis) == EINVAL
        for mis in (1, 2, 4):
            assert call(n=n, tb=tb + mis) == EINVAL and call(n=n, bd=bd + mis) == EINVAL and call(n=n, st=st + mis) == EINVAL
        for mis in (1, 2, 3):
            assert call(n=n, dn=dn + mis) == EINVAL and call(n=n, rl=rl + mis) == EINVAL and call(n=n, op=op + mis) == EINVAL
        for opts in (0x8, 0x20, 0x1F, 0xFFFFFFFF):
            assert call(n=n, opts=opts) == EINVAL
        for np_ in (0, 65, 0xFFFFFFFF):
            assert call(n=n, np_=np_) == EINVAL
        assert call(n=n, ne=1025) == EINVAL and call(n=n, ne=0xFFFFFFFF) == EINVAL and call(n=n, tb=None) == EINVAL
        for ch in BAD_CHUNKS:
            assert call(n=n, ch=ch) == EINVAL, ch
    assert call(n=MAX_BATCH + 1) == EINVAL and call(n=0xFFFFFFFF) == EINVAL
    # n_max == 0 with valid arguments launches nothing; the optional arguments may be NULL; every chunk size of the range
    assert call(n=0) == 0 and call(n=0, dn=None, tb=None, ne=0, bd=None, op=None, rl=None, st=None) == 0
    for k in range(11, 21):
        assert call(n=0, ch=1 << k) == 0


def test_argument_validation_of_the_serve_call_needs_no_gpu():
    import xsknet_amd as X
    L = X.lib()
    up, rest = _ring(X, 0x100000), _ring(X, 0x200000)
    um, tb, bd, op, bu, st, res = 0x600000, 0x520000, 0x530000, 0x590000, 0x5A0000, 0x570000, 0x580000

    def call(um=um, up=up, tx=None, np_=3, rest=rest, mx=64, opts=0, tb=tb, ne=4, bd=bd, op=op, ch=2048, bu=bu, st=st,
             res=res):
        tx = _ports(X, max(min(np_, 64), 1)) if tx is None else tx
        return L.xsk_gpu_unreach_serve_dev(um, 1 << 20, _ref(up), tx if tx != 0 else None, np_, _ref(rest), mx, opts, tb,
                                           ne, bd, op, ch, bu, st, res, None)

    assert call(um=None) == EINVAL and call(tx=0) == EINVAL and call(rest=None) == EINVAL and call(up=None) == EINVAL
    for b in _bad_rings(X, 0x100000, 16):
        assert call(up=b) == EINVAL
        if b is not None:
            assert call(rest=b) == EINVAL
            for n, at in ((1, 0), (3, 2), (64, 63), (64, 31)):
                tx = _ports(X, n)
                tx[at] = b
                assert call(tx=tx, np_=n) == EINVAL
    # any two rings sharing an entry array or an index word
    for f in ("d_ring", "d_producer", "d_consumer"):
        for n, a, b in ((2, 0, 1), (64, 5, 63)):
            tx = _ports(X, n)
            setattr(tx[b], f, getattr(tx[a], f))
            assert call(tx=tx, np_=n) == EINVAL, f
        for other in (up, rest):
            tx = _ports(X, 64)
            setattr(tx[17], f, getattr(other, f))
            assert call(tx=tx, np_=64) == EINVAL, f
        s2 = _ring(X, 0x100000)
        setattr(s2, f, getattr(rest, f))
        assert call(up=s2) == EINVAL, f
    for mx in (0, 1025, MAX_BATCH, 0xFFFFFFFF):
        assert call(mx=mx) == EINVAL
    for np_ in (0, 65, 0xFFFFFFFF):
        assert call(np_=np_) == EINVAL
    for opts in (0x8, 0x20, 0xFFFFFFFF):
        assert call(opts=opts) == EINVAL
    assert call(ne=1025) == EINVAL and call(tb=None) == EINVAL
    for mis in (1, 2, 4):
        assert call(tb=tb + mis) == EINVAL and call(bd=bd + mis) == EINVAL and call(st=st + mis) == EINVAL
    for mis in (1, 2, 3):
        assert call(res=res + mis) == EINVAL and call(op=op + mis) == EINVAL and call(bu=bu + mis) == EINVAL
    for ch in BAD_CHUNKS:
        assert call(ch=ch) == EINVAL, ch


def test_every_rule_stands_in_front_of_the_first_device_call():
    """The host functions' own text: each device call returns -EINVAL from one block of checks before anything that
    launches, the files store through no inline assembly, hand out no slot by an atomic (the only atomics add to the
    counters) and read the index words and the budget through load_word."""
    code = re.sub(r"//[^\n]*", "", open(SRC).read())
    for name in ("xsk_unreach.h", "xsk_unreach_device.h"):
        more = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "xsknet_amd", "csrc", name)).read())
        assert "asm" not in more and "atomic" not in more.replace("__ATOMIC_ACQ_REL", "")
    assert "asm" not in code and "atomic_fetch" not in code and "hipMalloc" not in code and "hipMemcpy" not in code
    assert code.count("atomicAdd(") == 1 and "atomicAdd(reinterpret_cast<u64*>(ustats)" in code
    pub = code[code.index('extern "C" {'):]
    assert "<<<" not in pub
    for name in NAMES:
        body = pub[pub.index("int " + name + "("):]
        body = body[:body.index("\n}\n")]
        assert body.count("return -EINVAL") == 1 and body.index("return -EINVAL") < body.index("_launch("), name
    for word in ("r.cons", "r.prod", "A.d_budget"):
        assert f"load_word({word})" in code
    assert code.count("<<<") == 2  # one launch a call, no second


def test_the_rule_on_the_host_under_address_sanitizer():
    """tests/c/test_unreach.cpp: xsk_unreach.h's decision on frames in heap buffers of exactly len bytes, cut at every
    length; whole, at the end of a chunk-sized allocation where the error fits to the byte; both rewrites, the wave's
    replayed over 64 lanes; and the serve plan with its budget replayed lane by lane into rings of exactly their sizes.
    A stand-alone program: nothing loaded into Python runs under a sanitizer."""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "t")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "c", "test_unreach.cpp")], check=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    assert "unreach ok" in res.stdout
