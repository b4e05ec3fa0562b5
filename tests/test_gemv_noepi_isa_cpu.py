"""The operand-free form of the decode GEMV (gemv_bf16_noepi_kernel: launches without bias and residual), read from the compiled code of
its batch-1 instantiations at K of one batch (no GPU: hipcc cross-compiles gfx950), by the method of test_gemv_isa_cpu.py: 4 and 8 waves
with the slot-by-slot refill (one unit per wave: QKV) and 8 waves with the refill in half batches (looping: gate|up, lm_head).

What the form is for is visible only here: no load of an epilogue operand, the stream's waits counted as in gemv_bf16_kernel, and no
wait between a unit's reduction and its stores that would sit out the loads of the wave's next unit.  A compiler that goes back to
draining changes no result, only the speed."""
import os
import re
import shutil
import subprocess

import pytest

from util import REPO

CSRC = os.path.join(REPO, "vision-zephyr_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FORMS = [(4, 1), (8, 1), (8, 4)]      # waves per workgroup, refill granularity
K_ONE = 1      # GEMV_K_ONE: K of exactly one batch (4096), the shape of QKV, gate|up and lm_head


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    asm = str(tmp_path_factory.mktemp("gemv_noepi_isa") / "gemv.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "gemv_audit.hip", "-o", asm],
                   check=True, cwd=CSRC, stderr=subprocess.DEVNULL)
    txt = open(asm).read()
    out = {}
    for fn in re.split(r"\n(?=_Z\w+:)", txt):
        # <MB 1, R 2, U 8, NT, NW, MODE, G>
        m = re.match(rf"_Z\w*gemv_bf16_noepi_kernelILi1ELi2ELi8ELb1ELi([48])ELi{K_ONE}ELi([14])EE\w*:", fn)
        if m and "s_endpgm" in fn:
            body, tail = fn.split("s_endpgm", 1)
            out[(int(m.group(1)), int(m.group(2)))] = (body, tail)
    assert sorted(out) == FORMS, sorted(out)
    return out


@pytest.mark.parametrize("nw,g", FORMS)
def test_registers_scratch_occupancy(kernels, nw, g):
    _, tail = kernels[(nw, g)]
    num = lambda key: int(re.search(rf"; {key}: (\d+)", tail).group(1))  # noqa: E731
    assert num("ScratchSize") == 0
    assert num("Occupancy") >= 5, (num("NumVgprs"), num("Occupancy"))


@pytest.mark.parametrize("nw,g", FORMS)
def test_no_operand_loads(kernels, nw, g):
    """x, norm_w and the weights are all 16-byte loads; bias (dword) and residual (ushort) are not requested at all"""
    body, _ = kernels[(nw, g)]
    for op in ("global_load_dword ", "global_load_ushort", "global_load_short"):
        assert op not in body, op
    assert "global_load_dwordx4" in body
    assert "flat_load" not in body      # a pending flat load makes every later wait a drain


@pytest.mark.parametrize("nw,g", FORMS)
def test_waits_are_counted(kernels, nw, g):
    """What test_gemv_isa_cpu.py demands of gemv_bf16_kernel: at least 24 waits that leave 8 or more loads in flight; slot by slot, 16 of
    them leave 14 or 15.  In half batches the ring runs down to 8 loads before the next 8 go out, and no wait of the refilling step
    leaves fewer."""
    body, _ = kernels[(nw, g)]
    waits = [int(n) for n in re.findall(r"s_waitcnt vmcnt\((\d+)\)", body)]
    assert sum(n >= 8 for n in waits) >= 24, sorted(waits)
    if g == 1:
        assert sum(n in (14, 15) for n in waits) >= 16, sorted(waits)


@pytest.mark.parametrize("nw,g", FORMS)
def test_no_drain_between_reduction_and_stores(kernels, nw, g):
    """From the first DPP add behind a unit's dot products to each of the unit's global stores there is no s_waitcnt vmcnt(N) with N < 8:
    the wave's next unit (16 loads) stays in flight under the reduction and the epilogue."""
    body, _ = kernels[(nw, g)]
    after_dots, in_unit_tail, low, stores = False, False, [], 0
    for line in body.split("\n"):
        line = line.strip()
        if line.startswith("v_dot2"):
            after_dots, in_unit_tail, low = True, False, []
        elif after_dots and line.startswith("v_add_f32_dpp"):
            after_dots, in_unit_tail = False, True
        elif in_unit_tail:
            m = re.match(r"s_waitcnt.*vmcnt\((\d+)\)", line)
            if m and int(m.group(1)) < 8:
                low.append(int(m.group(1)))
            if line.startswith("global_store"):
                stores += 1
                assert not low, f"vmcnt{low} between a unit's reduction and its store"
    assert stores >= 2      # the check saw the epilogue: a bf16 and an fp32 store at the least
