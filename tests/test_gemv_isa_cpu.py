"""What the decode GEMV's overlap rests on, read from the compiled code of its four batch-1 production instantiations (no GPU: hipcc
cross-compiles gfx950).  The kernel's counted waits come from hipcc's own wait insertion, helped by scheduling barriers, empty asm uses and an
occupancy hint (gemv.hip); a compiler that goes back to draining the counter, spilling or taking more registers would change no result and
no test - only the speed.  This test notices."""
import os
import re
import shutil
import subprocess

import pytest

from util import REPO

CSRC = os.path.join(REPO, "vision-zephyr_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    asm = str(tmp_path_factory.mktemp("gemv_isa") / "gemv.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "gemv_audit.hip", "-o", asm],
                   check=True, cwd=CSRC, stderr=subprocess.DEVNULL)
    txt = open(asm).read()
    out = {}
    for fn in re.split(r"\n(?=_Z\w+:)", txt):
        m = re.match(r"_Z\w*gemv_bf16_kernelILi1ELi2ELi8ELb1ELb([01])ELi([48])E\w*:", fn)
        if m and "s_endpgm" in fn:
            body, tail = fn.split("s_endpgm", 1)
            out[(m.group(1) == "1", int(m.group(2)))] = (body, tail)
    assert len(out) == 4, sorted(out)
    return out


@pytest.mark.parametrize("fp8,nw", [(False, 4), (False, 8), (True, 4), (True, 8)])
def test_registers_scratch_occupancy(kernels, fp8, nw):
    """as at the commit before the rolling refill: bf16 5 waves per SIMD, e4m3 4; nothing spilled"""
    _, tail = kernels[(fp8, nw)]
    num = lambda key: int(re.search(rf"; {key}: (\d+)", tail).group(1))  # noqa: E731
    assert num("ScratchSize") == 0
    assert num("Occupancy") >= (4 if fp8 else 5), (num("NumVgprs"), num("Occupancy"))


@pytest.mark.parametrize("fp8,nw", [(False, 4), (False, 8), (True, 4), (True, 8)])
def test_waits_are_counted(kernels, fp8, nw):
    """The two compiled forms of the step consume 8 slots each, every slot under its own wait: 15/14 behind a slot while the ring is
    refilled, 15 down to 0 where it drains - at least 24 waits that leave 8 or more loads in flight.  (The commit before had none above 2
    in the stream: one full drain per batch.)  The fused-norm staging waits with the first half batch of weights (8 loads) in flight."""
    body, _ = kernels[(fp8, nw)]
    waits = [int(n) for n in re.findall(r"s_waitcnt vmcnt\((\d+)\)", body)]
    assert sum(n >= 8 for n in waits) >= 24, sorted(waits)
    assert sum(n in (14, 15) for n in waits) >= 16, sorted(waits)
