"""numpy restatement of HF's warpers behind top-p - MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper, EtaLogitsWarper
(hf:generation/logits_process.py), in the order of hf:generation/utils.py `_get_logits_processor` - chained behind
oracle/sampling_oracle.py's temperature / top-k / top-p.  TEST INFRASTRUCTURE ONLY.

Each warper sees the scores the one before it left, dropped tokens at -inf, so every softmax, entropy and maximum is taken over the set
kept so far.  All arithmetic in fp32, as HF's on fp32 scores.  tests/test_warpers_cpu.py pins `warp()` to HF's own classes (same kept
set, kept values equal bitwise); the GPU tests hold csrc/sampling.hip to it.

`choose_*` and `build_row` serve the GPU tests, which must choose every parameter away from any token: a float threshold decided in
another summation order may flip a token that sits on it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import sampling_oracle as SO  # noqa: E402

F = np.float32
NEG = F(-np.inf)


def _softmax(x):
    """fp32 softmax over the finite entries (exp(-inf) = 0)"""
    m = x.max()
    e = np.exp((x - m).astype(F), dtype=F)
    return (e / e.sum(dtype=F)).astype(F)


def _log_softmax(x):
    m = x.max()
    d = (x - m).astype(F)
    return (d - np.log(np.exp(d, dtype=F).sum(dtype=F), dtype=F)).astype(F)


def _entropy(x):
    """-sum p log p over the finite entries (HF: nansum / the clamped logits of torch.distributions.Categorical)"""
    lp = _log_softmax(x)
    fin = np.isfinite(lp)
    p = np.exp(lp[fin], dtype=F)
    return F(-(lp[fin] * p).sum(dtype=F))


def _keep_top(x, remove):
    """min_tokens_to_keep = 1: the largest score of the input set stays"""
    remove = remove & (x < x.max())
    return np.where(remove, NEG, x).astype(F)


def min_p(x, p):
    pr = _softmax(x)
    remove = pr < F(p) * pr.max()
    remove[int(np.argmax(pr))] = False
    return np.where(remove, NEG, x).astype(F)


def typical_shift(x):
    """the value TypicalLogitsWarper sorts by: |-log p_i - H| (inf for a dropped token)"""
    lp = _log_softmax(x)
    return np.abs((-lp) - _entropy(x)).astype(F)


def typical(x, mass):
    s = typical_shift(x)
    order = np.argsort(s, kind="stable")
    cum = np.cumsum(_softmax(x[order]), dtype=F)
    last = min(int((cum < F(mass)).sum()), x.shape[0] - 1)
    remove = s > s[order[last]]
    remove[order[0]] = False
    return np.where(remove, NEG, x).astype(F)


def epsilon(x, eps):
    return _keep_top(x, _softmax(x) < F(eps))


def eta_threshold(x, eta):
    return min(F(eta), F(np.sqrt(F(eta)) * np.exp(-_entropy(x), dtype=F)))


def eta(x, e):
    return _keep_top(x, _softmax(x) < eta_threshold(x, e))


def on(min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
    """which classes HF's generate would build"""
    return (min_p is not None, typical_p is not None and typical_p < 1.0, epsilon_cutoff is not None and 0.0 < epsilon_cutoff < 1.0,
            eta_cutoff is not None and 0.0 < eta_cutoff < 1.0)


def warp(logits, temperature, top_k=0, top_p=1.0, min_p_=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
    """fp32 logits [V] -> the scores the token is drawn from: tempered, the filtered entries at -inf"""
    x = SO.warp(np.asarray(logits, dtype=F), temperature, top_k, top_p).astype(F)
    a, b, c, d = on(min_p_, typical_p, epsilon_cutoff, eta_cutoff)
    if a:
        x = min_p(x, min_p_)
    if b:
        x = typical(x, typical_p)
    if c:
        x = epsilon(x, epsilon_cutoff)
    if d:
        x = eta(x, eta_cutoff)
    return x


def warp_params(logits, p):
    """`warp` by a vz_hip.sample_rows.RowParams (a greedy row: the logits as they are)"""
    if not p.sample:
        return np.asarray(logits, dtype=F)
    return warp(logits, p.temperature, p.top_k, p.top_p, p.min_p if p.min_p > 0 else None, p.typical_p, p.epsilon_cutoff, p.eta_cutoff)


def draw(logits, p, row=0):
    """the token csrc/sampling.hip draws for the RowParams p: the Gumbel race of oracle/sampling_oracle.py over the new kept set (the
    one-sequence kernel: row = its row; the per-row kernel: row 0); a greedy row: the first maximal index"""
    x = warp_params(logits, p)
    if not p.sample:
        return int(np.argmax(x))
    s = (x + SO.gumbel(x.shape[0], row, p.counter, p.seed)).astype(F)
    return int(np.argmax(np.where(np.isneginf(x), -np.inf, s)))


def lse(x):
    v = x[np.isfinite(x)].astype(np.float64)
    return float(v.max() + np.log(np.exp(v - v.max()).sum()))


# ---- parameters away from every token (the GPU tests' search) ----------------------------------------------------------------------------
def _gap_mid(vals, lo_rank, hi_rank, rel, most=False):
    """descending distinct decision values: the geometric midpoint of the first (most: the last) adjacent pair among ranks
    [lo_rank, hi_rank) that differs by at least `rel` (relative)"""
    v = np.sort(np.unique(vals[np.isfinite(vals) & (vals > 0)]).astype(np.float64))[::-1]
    ranks = range(lo_rank, min(hi_rank, len(v) - 1))
    for i in (reversed(ranks) if most else ranks):
        if v[i] >= (1.0 + rel) * v[i + 1] and v[i] < 0.98:
            return float(np.sqrt(v[i] * v[i + 1]))
    return None


def choose_min_p(x, rank=4, most=False):
    """x = the scores min_p sees: a min_p between two tokens' p_i / p_max at least 1 % apart, more than `rank` tokens kept (most: as
    many of the top 64 as possible)"""
    pr = _softmax(x).astype(np.float64)
    return _gap_mid(pr / pr.max(), rank, 64, 0.01, most)


def choose_epsilon(x, rank=4, most=False):
    return _gap_mid(_softmax(x), rank, 64, 0.01, most)


def choose_eta(x, rank=4, most=False):
    """eta with min(eta, sqrt(eta) * exp(-H)) between two tokens' probabilities: the decision value of token i in terms of eta is
    max(p_i, (p_i * exp(H))^2) (the smallest eta that drops it); the midpoint between two of those at least 1 % apart - both branches of
    the minimum then keep their distance to every token"""
    pr = _softmax(x).astype(np.float64)
    eh = float(np.exp(np.float64(_entropy(x))))
    return _gap_mid(np.maximum(pr, (pr * eh) ** 2), rank, 64, 0.03, most)


def choose_typical(x, rank=2, drop_top=False, most=False):
    """a typical_p at the midpoint between two adjacent cumulative masses (tokens ascending in the shifted value) whose token holds at
    least 1 % of the mass, with the neighbouring shifted values at least 1e-3 apart; drop_top: one that leaves out the most likely token"""
    s = typical_shift(x).astype(np.float64)
    order = np.argsort(s, kind="stable")
    pr = _softmax(x).astype(np.float64)[order]
    cum = np.cumsum(pr)
    ss = s[order]
    n = int(np.isfinite(x).sum())
    top_at = int(np.nonzero(order == int(np.argmax(x)))[0][0])
    ranks = range(rank, min(64, n - 1))
    for j in (reversed(ranks) if most else ranks):
        # mass in (cum[j-1], cum[j]) makes token j the last one kept
        if pr[j] >= 0.01 and ss[j] - ss[j - 1] >= 1e-3 and ss[j + 1] - ss[j] >= 1e-3 and cum[j] < 0.999 and (not drop_top or top_at > j):
            return float(0.5 * (cum[j - 1] + cum[j]))
    return None


# the GPU tests' rows: (temperatures to try, top_k, top_p, which warpers) per case
CASES = {
    "min_p": ((1.0, 0.7), 0, 1.0, "m"),
    "typical": ((0.35, 0.25, 0.5), 0, 1.0, "t"),
    "epsilon": ((1.0, 0.7), 0, 1.0, "e"),
    "eta": ((1.0, 0.7), 0, 1.0, "h"),
    "all": ((0.8, 0.6, 1.0), 50, 0.9, "mteh"),                 # all four behind top-k 50 / top-p 0.9
    "no_top_k": ((0.5, 0.4), 0, 0.95, "mteh"),                 # top-k off
    "typical_drops_top": ((0.6, 0.5, 0.7, 0.8, 0.4), 0, 1.0, "T"),
    "epsilon_keeps_one": ((1.0,), 0, 1.0, "E"),                # epsilon would drop everything: the fallback keeps the maximum
    "greedy": ((1.0,), 0, 1.0, ""),
}


def build_row(case, V, seed, scale=2.5):
    """(fp32 logits [V], RowParams) of one test row: random normal logits, the case's warpers with every parameter chosen away from any
    token (searched over seeds seed, seed + 1, ... and the case's temperatures); the row's Philox seed and counter follow `seed`"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vision-zephyr_amd"))
    from vz_hip.sample_rows import GREEDY, RowParams
    temps, top_k, top_p, which = CASES[case]
    for s in range(seed, seed + 200):
        logits = (np.random.default_rng(s).standard_normal(V) * scale).astype(F)
        if which == "":
            return logits, GREEDY.at(seed % 3)
        for T in temps:
            x = SO.warp(logits, T, top_k, top_p).astype(F)
            kw, ok = {}, True
            most = len(which) > 1          # a chain: every warper drops little, so that the next one still has a choice
            for c in which:
                r = 1 if most else 4
                if c == "m":
                    v = choose_min_p(x, r, most)
                    kw["min_p"], x = v, (min_p(x, v) if v else x)
                elif c in "tT":
                    v = choose_typical(x, min(r, 2), c == "T", most)
                    kw["typical_p"], x = v, (typical(x, v) if v else x)
                elif c == "e":
                    v = choose_epsilon(x, r, most)
                    kw["epsilon_cutoff"], x = v, (epsilon(x, v) if v else x)
                elif c == "E":
                    v = 0.9 if float(_softmax(x).max()) < 0.5 else None
                    kw["epsilon_cutoff"], x = v, (epsilon(x, v) if v else x)
                elif c == "h":
                    v = choose_eta(x, r, most)
                    kw["eta_cutoff"], x = v, (eta(x, v) if v else x)
                if v is None:
                    ok = False
                    break
            if ok:
                return logits, RowParams(True, T, top_k, top_p, 0x5EED_0000_0000 + 7919 * seed, (0, 1, 77)[seed % 3], **kw)
    raise AssertionError(f"no row for case {case} at V = {V} from seed {seed}")
