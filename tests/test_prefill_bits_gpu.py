"""The rows-per-sample decoder stack (csrc/engine.hip: llm_rows_forward, behind vz_llm_prefill_rows and vz_llm_prefill_append) against
the commit before the two entry points shared one body: same bits, same arena mark, same launches.

tests/golden/prefill_parent_bits.npz was written by tools/dump_prefill_bits.py on that commit (its CASES are the list: plain and ragged
prefill, a prefill into the second cache row, the rotated-copy path, the fp8 MFMA route, an append on the fp8 engine - which keeps
the bf16 linears -, and the append's key-split, padded key-split and flash-per-run attention).  Every case reproduced bit for bit there,
so every case is held to equality: the SHA-256 of the logits, of the K and V the call wrote and of the K and V it had to keep, two
bit-pattern samples that size a mismatch, the digest of the inputs, the arena mark of vz_engine_ws_info, and the launches per profile
class."""
import os
import sys

import numpy as np
import pytest

from util import GOLDEN, REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import dump_prefill_bits as D  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def envs():
    e = D.Envs()
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "prefill_parent_bits.npz"))


def test_every_case_reproduced_on_the_parent_commit(golden):
    assert golden["nondet"].size == 0
    assert all(f"{name}.sha.logits_last" in golden.files for name in D.CASES)


@pytest.mark.parametrize("name", list(D.CASES))
def test_bits_peak_and_launches_equal_the_parent_commit(envs, golden, name):
    out = D.run_case(envs, name)
    got = D.digests(out)
    assert got["sha.inputs"] == str(golden[f"{name}.sha.inputs"]), f"{name}: the embeds or the weights differ from the recorded run (not a kernel difference)"
    assert out["untouched"], f"{name}: the call changed cache bits outside the slots it writes"
    for key in D.BIT_KEYS:
        want = golden[f"{name}.bits.{key}"]
        assert want.shape == got["bits." + key].shape, (name, key)
        n = int((want != got["bits." + key]).sum())
        assert n == 0, f"{name}.{key}: {n} of {want.size} values differ from the parent commit's bits"
    for key in D.SHA_KEYS:
        assert got["sha." + key] == str(golden[f"{name}.sha.{key}"]), f"{name}.{key}: not the parent commit's bits"
    assert got["peak"] == int(golden[f"{name}.peak"]), f"{name}: arena mark {got['peak']}, the parent commit's {int(golden[f'{name}.peak'])}"
    launches = D.count_launches(envs, name)
    assert launches == golden[f"{name}.launches"].tolist(), f"{name}: launches {dict(zip(D.CLASSES, launches))}, the parent commit's {golden[f'{name}.launches'].tolist()}"
