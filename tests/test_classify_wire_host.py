"""The per-frame function of classify_wire_kernel (xsknet_amd/csrc/xsk_classify_wire.h) compiled for the host and run
under AddressSanitizer (tests/c/test_classify_wire.cpp, a stand-alone program): the actions of the Python spec, and no
read outside a UMEM that ends where the frame ends.  No GPU."""
import os
import struct
import subprocess
import tempfile

from tests import classify_wire as CW
from tests.conftest import ROOT
from tests.v6_frames import mixed_batch6


def _record(opts, bound, L, want, data: bytes) -> bytes:
    data = data[:L]
    return struct.pack("<5I", opts, int(bound), L, want, len(data)) + data


def test_host_build_matches_spec_and_reads_inside_the_frame():
    recs = []
    for v in CW.golden():
        f = bytes.fromhex(v["frame"])
        for opts in CW.GC.OPTION_WORDS:
            for bound in (True, False):
                want = v["results"][str(opts)]["bound" if bound else "unbound"]
                assert want == CW.GC.classify(f, v["len"], opts, bound)
                recs.append(_record(opts, bound, v["len"], want, f))
    umem, descs = mixed_batch6(1024, seed=11)
    for opts in (0x12, 0x17):
        act, _ = CW.spec_classify_batch(umem, descs, opts, True)
        for i in range(len(descs)):
            a, L = int(descs[i]["addr"]), int(descs[i]["len"])
            recs.append(_record(opts, True, L, int(act[i]), umem[a:a + L].tobytes()))
    # descriptors past XSK_GPU_MAX_LEN, with and without bytes behind them
    recs.append(_record(0x17, True, (1 << 30) + 1, CW.XDP_DROP, bytes.fromhex(CW.golden()[0]["frame"])))
    recs.append(_record(0x17, True, 0xFFFFFFFF, CW.XDP_DROP, b""))
    with tempfile.TemporaryDirectory() as td:
        exe, inp = os.path.join(td, "t"), os.path.join(td, "in.bin")
        with open(inp, "wb") as fh:
            fh.write(b"".join(recs))
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "c", "test_classify_wire.cpp")],
                       check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
        res = subprocess.run([exe, inp], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    assert f"classify wire ok: {len(recs)} records" in res.stdout
