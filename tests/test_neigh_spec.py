"""The neighbour responder without a GPU (xsk_gpu_neigh_table_prepare, xsk_gpu_neigh_dev, xsk_gpu_neigh_serve_dev;
include/xsk_gpu.h "Neighbour responder"): the two restatements of the rule (tests/neigh_spec.py, which parses, and
tests/golden/make_neigh_golden.py, which builds) held against each other and against replies written out by hand; the
properties of the replies; the ABI surface and the export table; every -EINVAL of the three calls with fabricated
pointers (no device call reached); the table's rules; and xsk_neigh.h compiled for the host under AddressSanitizer
(tests/c/test_neigh.cpp)."""
import ctypes as C
import errno
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from tests import neigh_frames as NF
from tests import neigh_spec as NS
from tests import rx_dev_spec as RS
from tests.conftest import ROOT
from tests.test_rx_dev_spec import MAX_BATCH, _bad_rings, _decl, _header, _ref, _ring, _struct
from tests.test_rx_steer_spec import _ports
from tests.test_tx_complete_rings_spec import _exports

EINVAL, EEXIST = -errno.EINVAL, -errno.EEXIST
NAMES = ("xsk_gpu_neigh_table_prepare", "xsk_gpu_neigh_dev", "xsk_gpu_neigh_serve_dev")
# substrings that existing tests reserve for existing exports
RESERVED = ("ring_dev", "rx_begin", "rx_end", "rx_step_dev", "tx_complete_dev", "rd_", "ring_ports", "rx_prepare", "rx_ports",
            "rx_step_steer", "rp_", "pass", "egress", "fused", "rx_loop", "complete_rings", "queues", "rx_queue")
SRC = os.path.join(ROOT, "xsknet_amd", "csrc", "xsk_neigh.hip")


def _same(got, want):
    v, port, reply, rlen = got
    assert v == want["verdict"] and port == want["port"], (got[:2], want)
    assert (reply.hex() if reply is not None else None) == want.get("reply")
    assert rlen == want.get("reply_len", 0)


# ---- the two restatements ----------------------------------------------------------------------------------------

def test_the_golden_file_is_what_its_generator_writes():
    doc = NF.golden()
    assert doc["opts"] == [0, 0x2, 0x10, 0x12, 0x17] and doc["n_ports"] == NF.N_PORTS and int(doc["bound"], 16) == NF.BOUND
    assert len(doc["cases"]) == 4 * len(NF.G.CASES) and {c["tags"] for c in doc["cases"]} == {0, 1, 2, 3}
    for c, (case, tags) in zip(doc["cases"], ((case, tags) for case in NF.G.CASES for tags in NF.G.TAGS)):
        name, family, (frame, reply), verdict = case
        f = frame(tags)
        assert c["name"] == name and c["frame"] == f.hex()
        for o in NF.OPTS:
            assert c["expect"]["0x%x" % o] == NF.G.expect(family, verdict, reply, tags, o, f)
    assert [dict(family=e[0], addr=e[1].hex(), port=e[2], mac=e[3].hex()) for e in NF.G.TABLE] == doc["table"]


@pytest.mark.parametrize("opts", NF.OPTS)
def test_both_restatements_agree_on_every_golden_case(opts):
    t = NF.table()
    seen = set()
    for frame, want in NF.golden_frames(opts):
        got = NS.decide(frame, opts, t, NF.N_PORTS, NF.BOUND)
        _same(got, want)
        seen.add(got[0])
    # every verdict under the dual-stack option words; without XSK_GPU_OPT_IPV6 no solicitation is looked at
    assert seen == (set(range(7)) if opts & NS.OPT_IPV6 else {NS.NONE, NS.ARP_REPLY, NS.MALFORMED, NS.UNKNOWN, NS.UNBOUND})


def test_every_rule_letter_has_a_case():
    names = {c[0] for c in NF.G.CASES}
    for need in ("arp_cut", "arp_htype", "arp_ptype", "arp_hlen", "arp_plen", "arp_is_reply", "arp_stranger",
                 "arp_port_high", "arp_port_unbound", "arp_request", "ns_cut_header", "ns_version", "ns_udp", "ns_cut_icmp",
                 "echo_request", "ns_hop_limit", "ns_code", "ns_pl_16", "ns_pl_overrun", "ns_target_multicast",
                 "ns_pl_not_8", "ns_pl_288", "ns_option_len_0", "ns_option_overrun", "ns_bad_sum", "ns_dad", "ns_no_option",
                 "ns_stranger", "ns_port_unbound", "ns_request", "tag_cut", "tcp4"):
        assert need in names, need


@pytest.mark.parametrize("opts,seed", [(0x17, 11), (0x12, 12), (0x17, 13)])
def test_both_restatements_agree_on_seeded_random_batches(opts, seed):
    batch = NF.random_frames(400, opts, seed)
    umem, descs = NF.layout([f for f, _ in batch])
    before = umem.copy()
    stats = dict.fromkeys(NS.STATS_KEYS, 0)
    verdicts, ports, rlens = NS.spec_neigh(umem, descs, len(descs), opts, NF.table(), NF.N_PORTS, NF.BOUND, stats)
    NF.check_condition(verdicts)
    want_umem = before.copy()
    for i, (f, want) in enumerate(batch):
        assert (verdicts[i], ports[i], rlens[i]) == (want["verdict"], want["port"], want.get("reply_len")), i
        if "reply" in want:
            a = int(descs[i]["addr"])
            want_umem[a:a + len(f)] = np.frombuffer(bytes.fromhex(want["reply"]), np.uint8)
    assert (umem == want_umem).all()  # the replies, and every byte between the frames as it was
    assert stats["seen"] == 400 and stats["arp_replies"] == verdicts.count(NS.ARP_REPLY)
    assert stats["na_replies"] == verdicts.count(NS.NA_REPLY) and stats["reply_bytes"] == sum(r for r in rlens if r)


# ---- the replies --------------------------------------------------------------------------------------------------

def _replies(kind):
    for opts in NF.OPTS:
        for frame, want in NF.golden_frames(opts):
            if want["verdict"] == kind:
                yield opts, frame, bytes.fromhex(want["reply"]), want["reply_len"]


def test_every_advertisement_sums_to_ffff_under_its_own_pseudo_header():
    n = 0
    for opts, frame, reply, rlen in _replies(NS.NA_REPLY):
        l3 = rlen - 72
        src, dst, msg = reply[l3 + 8:l3 + 24], reply[l3 + 24:l3 + 40], reply[l3 + 40:l3 + 72]
        buf = np.frombuffer(NS.pseudo(src, dst, 32) + msg, np.uint8).copy()
        assert oracle.fold_sum(buf, 0, len(buf)) == 0xFFFF
        assert reply[l3:l3 + 8] == bytes.fromhex("6000000000203aff") and msg[0] == 136 and msg[24:26] == b"\x02\x01"
        assert src == msg[8:24] == frame[l3 + 48:l3 + 64] and dst == frame[l3 + 8:l3 + 24]
        assert reply[rlen:] == frame[rlen:] and reply[12:l3] == frame[12:l3]
        n += 1
    assert n >= 15


def test_a_reply_fed_back_is_none():
    t = NF.table()
    n = 0
    for kind in (NS.ARP_REPLY, NS.NA_REPLY):
        for opts, frame, reply, rlen in _replies(kind):
            for o in NF.OPTS:
                assert NS.decide(reply, o, t, NF.N_PORTS, NF.BOUND)[0] == NS.NONE
                assert NS.decide(reply[:rlen], o, t, NF.N_PORTS, NF.BOUND)[0] == NS.NONE
            n += 1
    assert n >= 30


def test_both_restatements_against_replies_written_out_by_hand():
    """An ARP reply and a neighbour advertisement as byte literals, worked out on paper: 192.0.2.77 (02:aa:bb:cc:dd:01)
    asks for 192.0.2.1, owned by 02:00:00:00:0a:03 on port 3; 2001:db8::77 asks for 2001:db8::fe, owned by
    02:00:00:00:06:fe on port 7.  The advertisement's checksum: 3 x (2001 + 0db8) + 2 x 00fe + 0077 + 0020 + 003a + 8800 +
    6000 + 0201 + 0200 + 06fe = 17ef7 -> 7ef8 -> complement 8107."""
    arp = bytes.fromhex("02aabbccdd01" "020000000a03" "0806"
                        "0001" "0800" "06" "04" "0002"
                        "020000000a03" "c0000201" "02aabbccdd01" "c000024d")
    na = bytes.fromhex("02aabbccdd01" "0200000006fe" "86dd"
                       "60000000" "0020" "3a" "ff"
                       "20010db80000000000000000000000fe" "20010db8000000000000000000000077"
                       "8800" "8107" "60000000" "20010db80000000000000000000000fe" "0201" "0200000006fe")
    by_name = {(c["name"], c["tags"]): c for c in NF.golden()["cases"]}
    t = NF.table()
    for name, hand, verdict, port in (("arp_request", arp, NS.ARP_REPLY, 3), ("ns_request", na, NS.NA_REPLY, 7)):
        c = by_name[(name, 0)]
        want = c["expect"]["0x17"]
        assert want["reply"] == hand.hex() and want["verdict"] == verdict and want["port"] == port
        assert want["reply_len"] == len(hand)
        got = NS.decide(bytes.fromhex(c["frame"]), 0x17, t, NF.N_PORTS, NF.BOUND)
        assert got == (verdict, port, hand, len(hand))


# ---- the serve loop's own identities -------------------------------------------------------------------------------

def _serve_state(frames, n_ports, stack_size=64, tx_size=8, up_size=64, start=0xFFFFFFF0):
    umem, descs = NF.layout(frames)
    stack = RS.RingState(np.zeros(stack_size, oracle.DESC_DTYPE), start, start)
    stack.produce(descs)
    txs = [RS.RingState(np.zeros(tx_size, oracle.DESC_DTYPE), start + p, start + p) for p in range(n_ports)]
    up = RS.RingState(np.zeros(up_size, oracle.DESC_DTYPE), 5, 5)
    return umem, descs, stack, txs, up


def test_the_serve_loop_is_the_list_rule_entry_by_entry_and_stops_without_losing_a_frame():
    batch = NF.random_frames(60, 0x17, 21)
    frames = [f for f, _ in batch]
    t = NF.table()
    # room for everything: the frames and verdicts are the list call's
    umem, descs, stack, txs, up = _serve_state(frames, NF.N_PORTS, tx_size=64)
    ref = umem.copy()
    verdicts, ports, rlens = NS.spec_neigh(ref, descs, 60, 0x17, t, NF.N_PORTS, NF.BOUND)
    got = []
    res = NS.spec_serve(umem, stack, txs, up, 1024, 0x17, t, NF.BOUND, verdicts_out=got)
    assert got == verdicts and (umem == ref).all() and res["consumed"] == 60 and res["backlog"] == 0
    assert res["up"] == sum(r is None for r in rlens) and stack.used() == 0
    for p, tx in enumerate(txs):
        mine = [i for i in range(60) if ports[i] == p]
        assert tx.used() == len(mine)
        for k, i in enumerate(mine):  # batch order within a port; the reply's descriptor
            e = tx.entries[tx.slot(tx.cons + k)]
            assert (int(e["addr"]), int(e["len"]), int(e["options"])) == (int(descs[i]["addr"]), rlens[i], 0)
    # a TX ring of two entries stops the call in the middle: the frames behind it are untouched
    umem, descs, stack, txs, up = _serve_state(frames, NF.N_PORTS, tx_size=2)
    before = umem.copy()
    res = NS.spec_serve(umem, stack, txs, up, 1024, 0x17, t, NF.BOUND)
    c = res["consumed"]
    assert 0 < c < 60 and res["backlog"] == 60 - c and stack.used() == 60 - c
    first_behind = int(descs[c]["addr"])
    assert (umem[first_behind:] == before[first_behind:]).all()
    assert ports[c] != NS.NO_PORT and txs[ports[c]].free() == 0  # it stopped at a reply whose ring is full


# ---- the ABI surface ------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_entry_points():
    import xsknet_amd as X
    R, E = "const struct xsk_gpu_ring_dev*", "const struct xsk_gpu_neigh_entry*"
    assert _decl("int", "xsk_gpu_neigh_table_prepare") == "struct xsk_gpu_neigh_entry* entries, uint32_t n"
    assert _decl("int", "xsk_gpu_neigh_dev") == (
        "void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, const uint32_t* d_n, uint32_t n_max, "
        f"uint32_t opts, {E} d_table, uint32_t n_entries, uint32_t n_ports, const uint64_t* d_bound, "
        "uint8_t* d_nverdicts, uint8_t* d_nports, uint32_t* d_reply_len, struct xsk_gpu_neigh_stats* d_nstats, "
        "void* stream")
    assert _decl("int", "xsk_gpu_neigh_serve_dev") == (
        f"void* d_umem, uint64_t umem_size, {R} stack, {R} tx , uint32_t n_ports, {R} up, uint32_t max, uint32_t opts, "
        f"{E} d_table, uint32_t n_entries, const uint64_t* d_bound, struct xsk_gpu_neigh_stats* d_nstats, "
        "struct xsk_gpu_neigh_result* d_res, void* stream")
    assert _struct("xsk_gpu_neigh_entry") == "uint8_t addr[16]; uint8_t family; uint8_t port; uint8_t mac[6];"
    assert _struct("xsk_gpu_neigh_stats") == "uint64_t seen, arp_replies, na_replies, reply_bytes;"
    assert re.search(r"#define\s+XSK_GPU_NEIGH_MAX_ENTRIES\s+1024u\b", _header())
    for k, name in enumerate(X.NEIGH_VERDICTS):
        assert re.search(r"XSK_GPU_NEIGH_%s = %d\b" % (name, k), _header()) and getattr(X, "NEIGH_" + name) == k
        assert getattr(NS, name) == k
    exported = _exports()
    for name in NAMES:
        assert name in exported and hasattr(X.lib(), name) and name in X._SIGS, name
    assert [len(X._SIGS[n][0]) for n in NAMES] == [2, 15, 14]
    for f in ("NEIGH_ENTRY_DTYPE", "NEIGH_STATS_DTYPE", "NEIGH_RESULT_DTYPE", "NEIGH_MAX_ENTRIES", "neigh_table_prepare",
              "neigh_dev", "neigh_serve_dev"):
        assert f in X.__all__
    assert X.NEIGH_MAX_ENTRIES == 1024 and X.lib().xsk_gpu_abi_version() == 1


def test_the_library_gained_exactly_the_three_names():
    for name in NAMES:
        assert not [s for s in RESERVED if s in name], name
    src = open(SRC).read()
    pub = src[src.index('extern "C" {'):]
    assert sorted(re.findall(r"^(?:int|size_t) (\w+)\(", pub, re.M)) == sorted(NAMES)
    # nothing else of the feature is exported: no other "neigh", no ng_* helper (xsk_gpu_timing_* has an "ng_" of its own)
    assert sorted(s for s in _exports() if "neigh" in s.lower() or "ng_" in s.replace("timing_", "")) == sorted(NAMES)
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "xsk_neigh.o" in mk and "xsk_neigh.h" in mk


def test_struct_layouts():
    import xsknet_amd as X
    probe = r'''
#include <stdio.h>
#include <stddef.h>
#include "xsk_gpu.h"
#define O(s, f) printf(#s "." #f " %zu\n", offsetof(struct s, f))
int main(void){
 printf("sizes %zu %zu %zu\n", sizeof(struct xsk_gpu_neigh_entry), sizeof(struct xsk_gpu_neigh_stats), sizeof(struct xsk_gpu_neigh_result));
 O(xsk_gpu_neigh_entry, addr); O(xsk_gpu_neigh_entry, family); O(xsk_gpu_neigh_entry, port); O(xsk_gpu_neigh_entry, mac);
 O(xsk_gpu_neigh_stats, seen); O(xsk_gpu_neigh_stats, arp_replies); O(xsk_gpu_neigh_stats, na_replies); O(xsk_gpu_neigh_stats, reply_bytes);
 O(xsk_gpu_neigh_result, consumed); O(xsk_gpu_neigh_result, arp_replies); O(xsk_gpu_neigh_result, na_replies);
 O(xsk_gpu_neigh_result, up); O(xsk_gpu_neigh_result, backlog); O(xsk_gpu_neigh_result, reserved);
 return 0; }
'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "p.c")
        open(c, "w").write(probe)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(td, "p"), c], check=True)
        out = subprocess.run([os.path.join(td, "p")], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "sizes 24 32 32"
    offs = dict(line.split() for line in out[1:] if line)
    for dt, name in ((X.NEIGH_ENTRY_DTYPE, "xsk_gpu_neigh_entry"), (X.NEIGH_STATS_DTYPE, "xsk_gpu_neigh_stats"),
                     (X.NEIGH_RESULT_DTYPE, "xsk_gpu_neigh_result")):
        for f in dt.names:
            assert int(offs[f"{name}.{f}"]) == dt.fields[f][1], (name, f)
    assert X.NEIGH_STATS_DTYPE.names == NS.STATS_KEYS and X.NEIGH_RESULT_DTYPE.names[:5] == NS.RESULT_KEYS


# ---- the argument rules ---------------------------------------------------------------------------------------------

def test_argument_validation_of_the_list_call_needs_no_gpu():
    import xsknet_amd as X
    L = X.lib()
    um, de, dn, tb, bd, nv, npo, rl, st = (0x600000, 0x500000, 0x510000, 0x520000, 0x530000, 0x540000, 0x550000, 0x560000,
                                           0x570000)

    def call(um=um, de=de, dn=dn, n=64, opts=0, tb=tb, ne=4, np_=8, bd=bd, nv=nv, npo=npo, rl=rl, st=st):
        return L.xsk_gpu_neigh_dev(um, 1 << 20, de, dn, n, opts, tb, ne, np_, bd, nv, npo, rl, st, None)

    for n in (0, 64, 1300):  # the empty call refuses alike
        assert call(n=n, um=None) == EINVAL and call(n=n, de=None) == EINVAL and call(n=n, nv=None) == EINVAL
        assert call(n=n, npo=None) == EINVAL
        for mis in (1, 2, 4, 8):
            assert call(n=n, de=de + mis) == EINVAL
        for mis in (1, 2, 4):
            assert call(n=n, tb=tb + mis) == EINVAL and call(n=n, bd=bd + mis) == EINVAL and call(n=n, st=st + mis) == EINVAL
        for mis in (1, 2, 3):
            assert call(n=n, dn=dn + mis) == EINVAL and call(n=n, rl=rl + mis) == EINVAL
        for opts in (0x8, 0x20, 0x1F, 0xFFFFFFFF):
            assert call(n=n, opts=opts) == EINVAL
        for np_ in (0, 65, 0xFFFFFFFF):
            assert call(n=n, np_=np_) == EINVAL
        assert call(n=n, ne=1025) == EINVAL and call(n=n, ne=0xFFFFFFFF) == EINVAL and call(n=n, tb=None) == EINVAL
    assert call(n=MAX_BATCH + 1) == EINVAL and call(n=0xFFFFFFFF) == EINVAL
    # n_max == 0 with valid arguments launches nothing; the optional arguments may be NULL
    assert call(n=0) == 0 and call(n=0, dn=None, tb=None, ne=0, bd=None, rl=None, st=None) == 0


def test_argument_validation_of_the_serve_call_needs_no_gpu():
    import xsknet_amd as X
    L = X.lib()
    stack, up = _ring(X, 0x100000), _ring(X, 0x200000)
    um, tb, bd, st, res = 0x600000, 0x520000, 0x530000, 0x570000, 0x580000

    def call(um=um, stack=stack, tx=None, np_=3, up=up, mx=64, opts=0, tb=tb, ne=4, bd=bd, st=st, res=res):
        tx = _ports(X, max(min(np_, 64), 1)) if tx is None else tx
        return L.xsk_gpu_neigh_serve_dev(um, 1 << 20, _ref(stack), tx if tx != 0 else None, np_, _ref(up), mx, opts, tb,
                                         ne, bd, st, res, None)

    assert call(um=None) == EINVAL and call(tx=0) == EINVAL and call(up=None) == EINVAL and call(stack=None) == EINVAL
    for b in _bad_rings(X, 0x100000, 16):
        assert call(stack=b) == EINVAL
        if b is not None:
            assert call(up=b) == EINVAL
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
        for other in (stack, up):
            tx = _ports(X, 64)
            setattr(tx[17], f, getattr(other, f))
            assert call(tx=tx, np_=64) == EINVAL, f
        s2 = _ring(X, 0x100000)
        setattr(s2, f, getattr(up, f))
        assert call(stack=s2) == EINVAL, f
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
        assert call(res=res + mis) == EINVAL


def test_every_rule_stands_in_front_of_the_first_device_call():
    """The host functions' own text: each device call returns -EINVAL from one block of checks before anything that
    launches, the file stores through no inline assembly, hands out no slot by an atomic (its only atomics add to the
    counters) and reads the index words through load_word."""
    code = re.sub(r"//[^\n]*", "", open(SRC).read())
    assert "asm" not in code and "atomic_fetch" not in code and "hipMalloc" not in code and "hipMemcpy" not in code
    assert code.count("atomicAdd(") == 1 and "atomicAdd(reinterpret_cast<u64*>(nstats)" in code
    pub = code[code.index('extern "C" {'):]
    assert "<<<" not in pub
    for name in NAMES[1:]:
        body = pub[pub.index("int " + name + "("):]
        body = body[:body.index("\n}\n")]
        assert body.count("return -EINVAL") == 1 and body.index("return -EINVAL") < body.index("_launch("), name
    for word in ("r.cons", "r.prod"):
        assert f"load_word({word})" in code
    assert code.count("<<<") == 2  # one launch a call, no second


# ---- the table ------------------------------------------------------------------------------------------------------

def _entry(X, family, addr, port, mac):
    e = np.zeros(1, X.NEIGH_ENTRY_DTYPE)
    a = bytes(addr)
    e[0]["addr"][:len(a)] = np.frombuffer(a, np.uint8)
    e[0]["family"], e[0]["port"] = family, port
    e[0]["mac"] = np.frombuffer(bytes(mac), np.uint8)
    return e


def test_prepare_sorts_and_refuses_with_the_array_untouched():
    import xsknet_amd as X
    L = X.lib()
    good = np.concatenate([_entry(X, *e) for e in NF.G.TABLE])
    got = X.neigh_table_prepare(good)
    keys = [bytes([int(e["family"])]) + e["addr"].tobytes() for e in got]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert sorted(e.tobytes() for e in got) == sorted(e.tobytes() for e in good)
    assert NS.table_array(X, NF.table()).tobytes() == got.tobytes()
    assert L.xsk_gpu_neigh_table_prepare(None, 0) == 0 and L.xsk_gpu_neigh_table_prepare(None, 1) == EINVAL
    mac = bytes.fromhex("020000000001")
    v6 = bytes.fromhex("20010db8000000000000000000000001")
    bad = [_entry(X, 5, [10, 0, 0, 1], 0, mac), _entry(X, 0, [10, 0, 0, 1], 0, mac),
           _entry(X, 4, [10, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1], 0, mac), _entry(X, 4, [10, 0, 0, 1, 9], 0, mac),
           _entry(X, 4, [10, 0, 0, 1], 64, mac), _entry(X, 6, v6, 255, mac),
           _entry(X, 4, [10, 0, 0, 1], 0, bytes(6)), _entry(X, 4, [10, 0, 0, 1], 0, bytes.fromhex("010000000001")),
           _entry(X, 6, v6, 0, bytes.fromhex("ffffffffffff")),
           _entry(X, 6, bytes.fromhex("ff020000000000000000000000000001"), 0, mac), _entry(X, 6, bytes(16), 0, mac)]
    for b in bad:
        for at in (0, 3, len(good)):
            arr = np.concatenate([good[:at][::-1], b, good[at:][::-1]])  # unsorted: a sort would show
            before = arr.tobytes()
            assert L.xsk_gpu_neigh_table_prepare(arr.ctypes.data, len(arr)) == EINVAL
            assert arr.tobytes() == before
            with pytest.raises(X.XskGpuError):
                X.neigh_table_prepare(arr)
    # the all-zero IPv4 address is an address like any other
    assert L.xsk_gpu_neigh_table_prepare(_entry(X, 4, [0, 0, 0, 0], 0, mac).ctypes.data, 1) == 0
    big = np.concatenate([_entry(X, 4, [10, 0, i >> 8, i & 255], i & 63, mac) for i in range(1025)])
    before = big.tobytes()
    assert L.xsk_gpu_neigh_table_prepare(big.ctypes.data, 1025) == EINVAL and big.tobytes() == before
    assert L.xsk_gpu_neigh_table_prepare(big.ctypes.data, 1024) == 0
    # duplicates: the same key with another port and mac
    dup = np.concatenate([good[::-1], _entry(X, 4, NF.G.OWN4[1], 1, mac)])
    assert L.xsk_gpu_neigh_table_prepare(dup.ctypes.data, len(dup)) == EEXIST
    keys = [bytes([int(e["family"])]) + e["addr"].tobytes() for e in dup]
    assert keys == sorted(keys)


def test_the_rule_on_the_host_under_address_sanitizer():
    """tests/c/test_neigh.cpp: xsk_neigh.h's decision on frames in heap buffers of exactly len bytes, cut at every length,
    the lookup on tables of exactly n_entries entries (0, 1, 1023, 1024; garbage too), the rewrites, and the serve plan
    replayed lane by lane into rings of exactly their sizes.  A stand-alone program: nothing loaded into Python runs under
    a sanitizer."""
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "t")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "c", "test_neigh.cpp")], check=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    assert "neigh ok" in res.stdout
