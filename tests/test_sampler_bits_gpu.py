"""The sampler and logits-processor entry points (csrc/engine.hip) against the commit before their parameters crossed the C ABI as one
record per family (vz_sample_params, vz_logits_proc_params): same tokens, same recorder rings, same processed logits, same graph captures.

tests/golden/sampler_parent_bits.npz was written by tools/dump_sampler_bits.py on that commit, through the Python helpers whose
signatures did not change (its CASES are the list: binding.sample, sample_rows, token_scores and logits_process at a vocabulary of the
kernels' staged form and one of their loop form; an engine under set_sampling with warpers, processors and the recorder, re-armed under
another seed and another temperature; under set_sampling_rows with a decode_set_row_sampling half way; and greedy with the recorder).
Every case reproduced bit for bit there, so every case is held to equality, with no tolerance: small results as bit patterns, score rows
by their SHA-256."""
import os
import sys

import numpy as np
import pytest

from util import GOLDEN, REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import dump_sampler_bits as D  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "sampler_parent_bits.npz"))


@pytest.fixture(scope="module")
def engine_cases():
    """the engine cases run once, in the order they were recorded in (the capture counts depend on it)"""
    return {name: D.digests(out) for name, out in D.run_engine_cases().items()}


def _equal_the_parent(golden, name, got):
    keys = sorted(k[len(name) + 1:] for k in golden.files if k.startswith(name + "."))
    assert keys and keys == sorted(got), (name, keys, sorted(got))
    for k in keys:
        want = golden[f"{name}.{k}"]
        if k.startswith("sha."):
            assert got[k] == str(want), f"{name}.{k}: not the parent commit's bits"
        else:
            assert want.shape == got[k].shape, (name, k, want.shape, got[k].shape)
            n = int((want != got[k]).sum())
            assert n == 0, f"{name}.{k}: {n} of {want.size} values differ from the parent commit's bits: {got[k].ravel()[:8]} vs {want.ravel()[:8]}"


def test_every_case_reproduced_on_the_parent_commit(golden):
    assert golden["nondet"].size == 0
    assert all(any(k.startswith(name + ".") for k in golden.files) for name in D.CASES)


@pytest.mark.parametrize("name", D.OP_CASES)
def test_ops_equal_the_parent_commit(golden, name):
    _equal_the_parent(golden, name, D.digests(D.run_op_case(name)))


@pytest.mark.parametrize("name", D.ENGINE_CASES)
def test_engine_equals_the_parent_commit(golden, engine_cases, name):
    _equal_the_parent(golden, name, engine_cases[name])
