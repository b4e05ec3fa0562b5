"""What the decode attention's short latency chain rests on, read from the compiled code of its two bf16 one-row kernels
(attn_o_fused_kernel<false, 1> of attn_o_fused.hip and attn_decode_fused_kernel of attn_decode.hip; no GPU: hipcc cross-compiles gfx950).
Both instantiate body<> of attn_decode_body.h, whose head (slot | pos, then ONE batch of 6 RoPE operands + 8 K + 8 V rows) and merge
(2 statistics + 32 partial pairs requested before any wait) get their counted waits from hipcc's own wait insertion, helped by
branch-free loads on clamped indices and scheduling barriers.  A compiler that drains the counter again changes speed, not results:
no other test would notice.  This test looks for exactly that and for nothing else."""
import os
import re
import shutil
import subprocess

import pytest

from util import REPO

CSRC = os.path.join(REPO, "vision-zephyr_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = {"attn_o_fused": ("attn_o_fused.hip", r"_Z\w*attn_o_fused_kernelILb0ELi1EE\w*:"),
           "attn_decode": ("attn_decode.hip", r"_Z\w*attn_decode_fused_kernel\w*:")}
LOAD = re.compile(r"\b(global|buffer|flat|scratch)_load")
VMCNT = re.compile(r"s_waitcnt vmcnt\((\d+)\)")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    out = {}
    for name, (src, pat) in KERNELS.items():
        asm = str(tmp_path_factory.mktemp("attn_isa") / (name + ".s"))
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", src, "-o", asm],
                       check=True, cwd=CSRC, stderr=subprocess.DEVNULL)
        found = [fn for fn in re.split(r"\n(?=_Z\w+:)", open(asm).read()) if re.match(pat, fn) and "s_endpgm" in fn]
        assert len(found) == 1, (name, len(found))
        body, tail = found[0].rsplit("s_endpgm", 1)
        out[name] = (body.split("\n"), tail)
    return out


def _first(lines, pred, start=0):
    for i in range(start, len(lines)):
        if pred(lines[i]):
            return i
    raise AssertionError("pattern not found in the kernel's code")


@pytest.mark.parametrize("name", list(KERNELS))
def test_registers_and_scratch(kernels, name):
    """three workgroups per CU (every workgroup of the fused launch resident): 168 VGPRs or fewer, nothing spilled"""
    _, tail = kernels[name]
    num = lambda key: int(re.search(rf"; {key}: (\d+)", tail).group(1))  # noqa: E731
    assert num("NumVgprs") <= 168 and num("ScratchSize") == 0, (num("NumVgprs"), num("ScratchSize"))


@pytest.mark.parametrize("name", list(KERNELS))
def test_no_flat_load(kernels, name):
    lines, _ = kernels[name]
    assert not [ln for ln in lines if "flat_load" in ln]


@pytest.mark.parametrize("name", list(KERNELS))
def test_merge_is_one_batch(kernels, name):
    """after the ticket's atomic add: the first wait behind a partial-record load leaves 16 or more loads in flight, and no loop between
    the add and the merged store loads anything"""
    lines, _ = kernels[name]
    add = _first(lines, lambda ln: "global_atomic_add" in ln)
    part = _first(lines, lambda ln: "global_load_dwordx2" in ln and "sc1" in ln, add)
    wait = _first(lines, lambda ln: VMCNT.search(ln), part)
    assert int(VMCNT.search(lines[wait]).group(1)) >= 16, lines[wait]
    last_part = max(i for i in range(add, len(lines)) if "global_load_dwordx2" in lines[i] and "sc1" in lines[i])
    store = _first(lines, lambda ln: "global_store_dword" in ln, last_part)
    labels = {m.group(1): i for i in range(add, store) for m in [re.match(r"(\.LBB\d+_\d+):", lines[i])] if m}
    for i in range(add, store):
        m = re.search(r"s_cbranch_\w+ (\.LBB\d+_\d+)", lines[i]) or re.search(r"s_branch (\.LBB\d+_\d+)", lines[i])
        if m and m.group(1) in labels and labels[m.group(1)] < i:        # a backward branch: lines[label .. i] is a loop body
            loads = [ln for ln in lines[labels[m.group(1)]:i] if LOAD.search(ln)]
            assert not loads, loads[:3]


@pytest.mark.parametrize("name", list(KERNELS))
def test_head_is_two_round_trips(kernels, name):
    """between the wait for slot | pos and the first barrier of the attention, no wait that leaves fewer than 16 loads in flight: the
    RoPE waits for its operands with the 8 K and 8 V rows of the first chunk outstanding"""
    lines, _ = kernels[name]
    q = _first(lines, lambda ln: "global_load_ushort" in ln)               # the q pair: the attention's head
    # (the wait for slot | pos is the last one in front of it; attn_decode.hip reads the two with scalar loads: no vmcnt wait at all)
    slot_wait = max([i for i in range(q) if VMCNT.search(lines[i])], default=-1)
    barrier = _first(lines, lambda ln: "s_barrier" in ln, q)
    low = [ln for ln in lines[slot_wait + 1:barrier] if VMCNT.search(ln) and int(VMCNT.search(ln).group(1)) < 16]
    assert not low, low
