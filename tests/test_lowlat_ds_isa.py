"""The dual-stack resident kernel's completion ordering and scalar loads, checked in the BUILT code object (no GPU).

resident_ds_kernel (xsk_lowlat.hip, the XSK_GPU_OPT_IPV6 instance of the LOWLAT doorbell kernel) runs its own copy of
lowlat_kernel's serving loop, so it is held to the same two properties as the two instances tests/test_lowlat_isa.py
checks, in the library as built:

    s_waitcnt vmcnt(0)          every wave: its own stores (the per-lane UMEM stores of wire_v6_phase among them) acked
    s_barrier                   the workgroup meets (no vector-memory op in between)
    buffer_wbl2 sc0 sc1         thread 0: system-scope release (L2 write-back)
    s_waitcnt vmcnt(0)          the write-back has completed
    global_store_dword ... sc0 sc1   bell->wg[g].done = seq

and: its only scalar loads come off the kernarg pointer or the GOT entry of the live counter (the acquire does not
invalidate the scalar data cache, so no batch data may come through it).
"""
import os
import re
import subprocess
import tempfile

import pytest

from tests.test_lowlat_isa import LIB, LLVM, VMEM, done_offset, gfx950_code_objects

pytestmark = pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-objdump"), reason="llvm-objdump not installed")


def ds_functions():
    """{symbol: [instruction lines]} of every dual-stack resident kernel in the library."""
    funcs = {}
    with tempfile.TemporaryDirectory() as td:
        for k, co in enumerate(gfx950_code_objects(LIB)):
            p = os.path.join(td, f"co{k}.o")
            open(p, "wb").write(co)
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", p], capture_output=True, text=True,
                                 check=True).stdout
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]{16} <(\S+)>:", line)
                if m:
                    cur = m.group(1) if "resident_ds_kernel" in m.group(1) else None
                    if cur:
                        funcs[cur] = []
                elif cur and line.startswith("\t"):
                    funcs[cur].append(line.split("//")[0].strip())
    return funcs


def the_kernel():
    funcs = ds_functions()
    assert len(funcs) == 1, sorted(funcs)  # exactly one dual-stack resident kernel
    (name, ins), = funcs.items()
    assert "lowlat_kernel" not in name and "echo_round_kernel" not in name, name  # outside the pinned set
    return name, ins


def test_ds_completion_waits_for_the_write_back():
    name, ins = the_kernel()
    off = done_offset()
    done = [i for i, s in enumerate(ins) if re.match(rf"global_store_dword \S+, \S+, .*offset:{off} sc0 sc1$", s)]
    # the cancelled-batch retirement (examine(): STOP seen with a batch not yet taken): `cancel` (offset + 8), the
    # write-back and a wait, then `done`
    cancel_re = re.compile(rf"global_store_dword \S+, \S+, .*offset:{off + 8} sc0 sc1$")
    retire = []
    for i in done:
        j = i - 1
        while j > i - 8 and not VMEM.match(ins[j]):
            j -= 1
        if cancel_re.match(ins[j]):
            between = ins[j + 1:i]
            assert "buffer_wbl2 sc0 sc1" in between and "s_waitcnt vmcnt(0)" in between, (name, between)
            retire.append(i)
    assert retire, (name, "no cancelled-batch retirement path")
    done = [i for i in done if i not in retire]
    assert len(done) == 1, (name, [ins[i] for i in done])  # the single completion store
    d = done[0]
    # back from it: a vmcnt(0) wait, before that the release write-back, no other vector-memory op in between
    j = d - 1
    saw_wait = False
    while not ins[j].startswith("buffer_wbl2"):
        assert not VMEM.match(ins[j]), (name, "a vector-memory op between the write-back and done", ins[j])
        saw_wait |= ins[j] == "s_waitcnt vmcnt(0)"
        j -= 1
        assert j > d - 64, (name, "no buffer_wbl2 before the done store")
    assert ins[j] == "buffer_wbl2 sc0 sc1", (name, ins[j])
    assert saw_wait, (name, "no s_waitcnt vmcnt(0) between buffer_wbl2 and the done store")
    # before the write-back: the workgroup barrier, reached by every wave only after its last vector-memory op has
    # been waited for
    k = j - 1
    while ins[k] != "s_barrier":
        assert not VMEM.match(ins[k]), (name, "a vector-memory op between the barrier and the write-back", ins[k])
        k -= 1
        assert k > j - 64, (name, "no s_barrier before the write-back")
    m = k - 1
    saw_wait = False
    while not VMEM.match(ins[m]):
        saw_wait |= bool(re.match(r"s_waitcnt vmcnt\(0\)", ins[m]))
        m -= 1
        assert m > k - 256, (name, "no vector-memory op before the barrier")
    assert saw_wait, (name, "the wave's last vector-memory op is not waited for before the barrier", ins[m])


def test_ds_scalar_loads_are_kernel_arguments_or_the_live_counter():
    name, ins = the_kernel()
    for i, s in enumerate(ins):
        if not (s.startswith("s_load") or s.startswith("s_buffer_load")):
            continue
        m = re.match(r"s_load_dword\w* s\[?[0-9:]+\]?, (s\[\d+:\d+\]), ", s)
        assert m, (name, s)
        if m.group(1) == "s[0:1]":
            continue  # kernarg segment
        base = m.group(1)
        lo = base[2:].split(":")[0]
        # the GOT entry: s_getpc_b64 base; s_add_u32 lo, lo, imm; s_addc_u32 hi, hi, 0; s_load base, base, 0x0
        assert ins[i - 3] == f"s_getpc_b64 {base}" and ins[i - 2].startswith(f"s_add_u32 s{lo}, s{lo}, "), \
            (name, ins[i - 4:i + 1])
