"""The ICMPv6 echo spec (XSK_GPU_OPT_IPV6) without a GPU: the committed golden vectors are what the Python spec
generates, every reply's checksum is right by a from-scratch recompute, and the option mask of the C ABI."""
import errno
import json
import os
import struct

import numpy as np

from tests.conftest import ROOT
from tests.v6_frames import G6, mixed_batch6, spec_batch

GOLDEN = os.path.join(ROOT, "tests", "golden", "v6.json")


def test_golden_file_is_what_the_spec_generates(tmp_path, monkeypatch):
    monkeypatch.setattr(G6, "_HERE", str(tmp_path))
    G6.main()
    again = open(tmp_path / "v6.json").read()
    G6.main()
    assert open(tmp_path / "v6.json").read() == again  # deterministic
    assert again == open(GOLDEN).read()


def test_golden_covers_the_named_cases():
    cases = json.load(open(GOLDEN))
    seen = {}
    for c in cases:
        seen.setdefault(c["name"], set()).add(c["results"]["23"]["verdict"])
    every = set().union(*seen.values())
    assert every >= {G6.TX_REPLY, G6.DROP_SHORT, G6.DROP_NOT_IPV4, G6.DROP_NOT_ICMP, G6.DROP_NOT_ECHO, G6.DROP_BAD_IP,
                     G6.DROP_BAD_CSUM}
    for name in ("echo_62", "payload_1", "payload_2", "payload_1400", "vlan1", "vlan2_qinq"):
        assert G6.TX_REPLY in seen[name], name
    # without the option bit's path (an IPv4 frame) the results are wire mode's
    for c in cases:
        if c["name"] == "ipv4_plain":
            fr = bytes.fromhex(c["frame"])
            for o in range(0x10, 0x18):
                v, rec, out = G6.W.expect(fr, c["len"], o & 7)
                assert c["results"][str(o)] == {"verdict": v, "rec": rec, "out": out[:c["len"]].hex()}


def _verifies(frame: bytes, l3: int, end: int) -> bool:
    """RFC 4443 §2.3 from scratch: the pseudo-header of the frame's own addresses plus the message sums to 0xFFFF."""
    l4 = l3 + 40
    msg = frame[l4:end]
    ph = frame[l3 + 8:l3 + 40] + struct.pack("!I", len(msg)) + b"\0\0\0\x3a"
    data = ph + msg + (b"\0" if len(msg) % 2 else b"")
    s = sum(struct.unpack(f"!{len(data) // 2}H", data))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s == 0xFFFF


def _l3_of(frame: bytes, opts: int) -> int:
    l3, et, tags = 14, (frame[12] << 8) | frame[13], 0
    while (opts & G6.OPT_VLAN) and tags < 2 and et in (0x8100, 0x88A8):
        et = (frame[l3 + 2] << 8) | frame[l3 + 3]
        l3 += 4
        tags += 1
    return l3


def test_reply_checksum_verifies_iff_the_request_did():
    cases = json.load(open(GOLDEN))
    checked = bad = 0
    for c in cases:
        fr, L = bytes.fromhex(c["frame"]), c["len"]
        for o in range(0x10, 0x18):
            res = c["results"][str(o)]
            if res["verdict"] != G6.TX_REPLY or res["rec"]["eth_proto"] != 0x86DD:
                continue
            out = bytes.fromhex(res["out"])
            l3 = _l3_of(fr, o)
            end = l3 + 40 + ((fr[l3 + 4] << 8) | fr[l3 + 5]) if o & G6.OPT_STRICT else L
            before, after = _verifies(fr[:L], l3, end), _verifies(out, l3, end)
            assert before == after, (c["name"], L, o)
            assert before == bool(res["rec"]["flags"] & G6.F_ICMP_OK), (c["name"], L, o)
            assert out[l3 + 40] == 129 and out[l3 + 8:l3 + 24] == fr[l3 + 24:l3 + 40]
            checked += 1
            bad += not before
    assert checked >= 40 and bad >= 3  # replies to requests whose checksum was wrong (no VERIFY) are in the set


def test_random_replies_verify_too():
    """The same property over random traffic, and the mix the GPU tests rely on: >= 6 distinct verdicts at n = 3000."""
    umem, descs = mixed_batch6(3000, 2048, seed=3017, offsets=True)
    before = umem.copy()
    v, r, st = spec_batch(umem, descs, 0x17)
    assert len(np.unique(v)) >= 6, np.unique(v)
    six = np.nonzero((v == G6.TX_REPLY) & (r["eth_proto"] == 0x86DD))[0]
    assert len(six) >= 300
    for i in six:
        a, L = int(descs[i]["addr"]), int(descs[i]["len"])
        l3 = _l3_of(before[a:a + L].tobytes(), 0x17)
        end = l3 + 40 + ((int(before[a + l3 + 4]) << 8) | int(before[a + l3 + 5]))
        assert _verifies(umem[a:a + L].tobytes(), l3, end), i  # VERIFY on: every request verified
    assert st["tx_packets"] == int((v == G6.TX_REPLY).sum())
    # frames that are not replies are untouched, and so is every byte between the frames
    mask = np.zeros(umem.size, bool)
    for i in np.nonzero(v == G6.TX_REPLY)[0]:
        mask[int(descs[i]["addr"]):int(descs[i]["addr"]) + int(descs[i]["len"])] = True
    assert (umem[~mask] == before[~mask]).all()


def test_option_mask_of_the_abi():
    import xsknet_amd as X
    L = X.lib()
    assert (X.OPT_IPV6, X.OPT_MASK, X.OPT_ALL, X.F_IPV6) == (0x10, 0x17, 7, 0x10)
    for opts in (0x10, 0x17):
        assert L.xsk_gpu_echo_dev_opts(None, 0, None, 0, opts, None, None, None, None, None) == 0, opts
    for opts in (0x8, 0x18, 0x20):
        assert L.xsk_gpu_echo_dev_opts(None, 0, None, 0, opts, None, None, None, None, None) == -errno.EINVAL, opts
