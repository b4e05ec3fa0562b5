"""The warpers behind top-p without a GPU: tests/warpers_ref.py against HF's own classes, and the parsing of the four keywords
(vz_hip/sample_rows.py: parse_warpers, row_params, parse_request, RowParams.warp)."""
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "vision-zephyr_amd"))

import warpers_ref as WR  # noqa: E402
from vz_hip import sample_rows as SR  # noqa: E402

GEN = types.SimpleNamespace(top_k=50, top_p=1.0)


def _logits(V, seed, scale=2.5):
    return (np.random.default_rng(seed).standard_normal(V) * scale).astype(np.float32)


def _hf_chain(x, temperature, top_k, top_p, min_p, typical_p, eps, eta):
    torch = pytest.importorskip("torch")
    L = pytest.importorskip("transformers.generation.logits_process")
    s = torch.from_numpy(x.copy()).unsqueeze(0)
    ids = torch.zeros(1, 0, dtype=torch.long)
    chain = []
    if temperature != 1.0:
        chain.append(L.TemperatureLogitsWarper(temperature))
    if top_k:
        chain.append(L.TopKLogitsWarper(top_k=top_k))
    if top_p < 1.0:
        chain.append(L.TopPLogitsWarper(top_p=top_p))
    a, b, c, d = WR.on(min_p, typical_p, eps, eta)
    if a:
        chain.append(L.MinPLogitsWarper(min_p=min_p))
    if b:
        chain.append(L.TypicalLogitsWarper(mass=typical_p))
    if c:
        chain.append(L.EpsilonLogitsWarper(epsilon=eps))
    if d:
        chain.append(L.EtaLogitsWarper(epsilon=eta))
    for w in chain:
        s = w(ids, s)
    return s[0].numpy()


CASES = [
    # temperature, top_k, top_p, min_p, typical_p, epsilon, eta
    (1.0, 0, 1.0, 0.05, None, None, None),
    (0.7, 0, 1.0, None, 0.6, None, None),
    (1.0, 0, 1.0, None, None, 3e-3, None),
    (1.3, 0, 1.0, None, None, None, 2e-3),
    (0.8, 50, 0.9, 0.02, 0.8, 1e-3, 4e-3),
    (0.2, 50, 1.0, 0.1, 0.9, 0.02, 0.02),
    (1.0, 0, 0.95, 0.0, 0.2, None, 0.3),
    (1.0, 0, 1.0, 1.0, None, None, None),            # min_p = 1: only the maximum stays
    (1.0, 0, 1.0, None, None, 0.9, None),            # epsilon would drop everything: the largest score stays
    (1.0, 5, 1.0, None, 0.05, 0.5, 0.9),
    (1.0, 0, 1.0, None, 1.0, 0.0, 1.0),              # HF's off values: no class is built
]


@pytest.mark.parametrize("V", [64, 1000, 32001])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_restatement_equals_hf(case, V):
    T, k, p, mp, tp, eps, eta = CASES[case]
    for seed in range(3):
        x = _logits(V, 100 * case + seed)
        want = _hf_chain(x, T, k, p, mp, tp, eps, eta)
        got = WR.warp(x, T, k, p, mp, tp, eps, eta)
        assert np.array_equal(np.isneginf(got), np.isneginf(want)), (case, V, seed, int(np.isfinite(got).sum()), int(np.isfinite(want).sum()))
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))      # kept values: bitwise
        assert np.isfinite(got).sum() >= 1


def test_restatement_sees_earlier_drops():
    """a row that already holds -inf (a banned token in front of the warpers): entropy and softmax skip it, as HF's do"""
    x = _logits(500, 7)
    x[[3, 77, 400]] = -np.inf
    for T, k, p, mp, tp, eps, eta in CASES[:7]:
        want = _hf_chain(x, T, k, p, mp, tp, eps, eta)
        got = WR.warp(x, T, k, p, mp, tp, eps, eta)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_typical_can_drop_the_most_likely_token():
    x = _logits(1000, 11, scale=2.0)
    got = WR.warp(x, 1.0, 0, 1.0, None, 0.2, None, None)
    assert np.isneginf(got[int(np.argmax(x))]) and np.isfinite(got).sum() >= 1
    assert np.array_equal(got.view(np.uint32), _hf_chain(x, 1.0, 0, 1.0, None, 0.2, None, None).view(np.uint32))


def test_chosen_parameters_sit_between_tokens():
    """the GPU tests' parameter search: the chosen value separates the kept set from the rest by the margin it promises"""
    x = WR.warp(_logits(1000, 5), 1.0, 50, 1.0)
    mp = WR.choose_min_p(x)
    pr = WR._softmax(x).astype(np.float64)
    r = pr[np.isfinite(x)] / pr.max()
    assert mp is not None and np.all((r >= mp * 1.004) | (r <= mp / 1.004))
    eps = WR.choose_epsilon(x)
    q = pr[np.isfinite(x)]
    assert eps is not None and np.all((q >= eps * 1.004) | (q <= eps / 1.004))
    eta = WR.choose_eta(x)
    thr = float(WR.eta_threshold(x, eta))
    assert eta is not None and 0 < eta < 1 and np.all((q >= thr * 1.004) | (q <= thr / 1.004))
    tp = WR.choose_typical(x)
    assert tp is not None and 0 < tp < 1
    for name, kept in (("min_p", WR.min_p(x, mp)), ("epsilon", WR.epsilon(x, eps)), ("eta", WR.eta(x, eta)), ("typical", WR.typical(x, tp))):
        assert 1 <= np.isfinite(kept).sum() < np.isfinite(x).sum(), name


# ---- parsing ---------------------------------------------------------------------------------------------------------------------------------
def test_value_checks_follow_hf():
    for kw in (dict(min_p=-0.1), dict(min_p=1.5), dict(typical_p=0.0), dict(typical_p=-0.5)):
        with pytest.raises(ValueError):
            SR.parse_warpers(**kw)
    L = pytest.importorskip("transformers.generation.logits_process")
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            L.MinPLogitsWarper(min_p=bad)
    for bad in (0.0, -0.5):
        with pytest.raises(ValueError):
            L.TypicalLogitsWarper(mass=bad)


def test_off_values_arm_nothing():
    assert SR.parse_warpers() == {}
    assert SR.parse_warpers(typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=1.0) == {}
    assert SR.parse_warpers(typical_p=1.5, epsilon_cutoff=-1.0, eta_cutoff=2.0) == {}
    p = SR.row_params(True, 0.7, -1, None, 3, GEN, lambda: 0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
    assert p == SR.RowParams(True, 0.7, 50, 1.0, 3, 0) and p.warp is None
    assert SR.row_params(True, 0.7, -1, None, 3, GEN, lambda: 0, min_p=0.0).warp is None          # min_p = 0 drops nothing
    assert SR.GREEDY.warp is None


def test_greedy_ignores_the_warpers():
    assert SR.row_params(False, 1.0, -1, None, None, GEN, lambda: 0, min_p=0.3, typical_p=0.5) is SR.GREEDY
    assert SR.row_params(True, 0.0, -1, None, None, GEN, lambda: 0, min_p=7.0) is SR.GREEDY          # HF builds no warper: no check either
    assert SR.RowParams(False, min_p=0.3).warp is None


def test_row_params_and_requests_carry_the_warpers():
    p = SR.row_params(True, 0.5, 0, 0.9, 11, GEN, lambda: 0, min_p=0.05, typical_p=0.8, epsilon_cutoff=1e-3, eta_cutoff=2e-3)
    assert (p.min_p, p.typical_p, p.epsilon_cutoff, p.eta_cutoff) == (0.05, 0.8, 1e-3, 2e-3)
    assert p.warp == (0.05, 0.8, 1e-3, 2e-3) and p.at(5).warp == p.warp and p.at(5).counter == 5
    q = SR.parse_request({"do_sample": True, "temperature": 0.5, "seed": 4, "min_p": 0.1, "typical_p": 0.7}, GEN, lambda: 0)
    assert q == SR.RowParams(True, 0.5, 50, 1.0, 4, 0, min_p=0.1, typical_p=0.7) and q.warp == (0.1, 0.7, 0.0, 0.0)
    q = SR.parse_request({"do_sample": True, "epsilon_cutoff": 3e-4, "eta_cutoff": 6e-4, "seed": 1}, GEN, lambda: 0)
    assert q.warp == (0.0, 0.0, 3e-4, 6e-4)
    with pytest.raises(ValueError):
        SR.parse_request({"do_sample": True, "min_p": 2.0}, GEN, lambda: 0)
    assert SR.parse_request({"min_p": 0.1}, GEN, lambda: 0) is SR.GREEDY
