"""tests/seq_bias_ref.py against HF's SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor plus the four existing processors, bit for
bit, and vz_hip.logits_proc.parse on the two keywords.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seq_bias_ref as R  # noqa: E402
from vz_hip import logits_proc as LP  # noqa: E402

V = 97


def _rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, V, generator=g) * 3).float()
    x[:, 3] = 0.0
    x[:, 5] = -1.5
    x[:, 7] = float("-inf")
    return x


def _hf_chain(kw, eos):
    from transformers.generation import logits_process as L
    chain = []
    if kw.get("sequence_bias") is not None:
        chain.append(L.SequenceBiasLogitsProcessor(sequence_bias=kw["sequence_bias"]))
    if kw.get("repetition_penalty") is not None:
        chain.append(L.RepetitionPenaltyLogitsProcessor(penalty=kw["repetition_penalty"]))
    if kw.get("no_repeat_ngram_size"):
        chain.append(L.NoRepeatNGramLogitsProcessor(kw["no_repeat_ngram_size"]))
    if kw.get("bad_words_ids") is not None:
        chain.append(L.NoBadWordsLogitsProcessor(kw["bad_words_ids"], torch.tensor(eos) if eos else None))
    if kw.get("min_new_tokens"):
        chain.append(L.MinNewTokensLengthLogitsProcessor(0, kw["min_new_tokens"], list(eos), device="cpu"))
    if kw.get("suppress_tokens"):
        chain.append(L.SuppressTokensLogitsProcessor(list(kw["suppress_tokens"]), device="cpu"))
    return chain


EOS = [90]
CASES = [
    dict(sequence_bias={(20,): 2.5}),
    dict(sequence_bias={(20, 21): -3.0, (20,): 1.5, (33, 40, 41): 4.0}),
    dict(sequence_bias=[[[20, 21], 2.0], [[22, 21], 0.7], [[21], -0.3]]),                      # two sequences and a one-id sequence bias id 21
    dict(sequence_bias={(40, 41, 50, 60): 5.0, (60,): float("-inf")}),
    dict(bad_words_ids=[[20], [20, 21], [33, 40, 41], [90]]),                                  # [90] equals the eos id: dropped
    dict(bad_words_ids=[[21], [60, 70]], sequence_bias={(21,): 9.0, (50, 70): 1.0}),
    # bias on ids the penalty also touches, either sign (5 is negative, 3 is zero, 33 random), and everything else at once
    dict(sequence_bias={(5,): 4.0, (3,): -2.0, (33,): 6.0, (20, 5): -9.5, (11, 33): -20.0}, repetition_penalty=1.3),
    dict(sequence_bias={(5,): 4.0, (3,): -2.0, (33,): -6.0}, repetition_penalty=0.7, no_repeat_ngram_size=2, bad_words_ids=[[40, 41], [22]],
         min_new_tokens=301, suppress_tokens=[11, 50]),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_reference_equals_hf_processors_bitwise(case):
    kw = CASES[case]
    cfg = LP.parse(eos=EOS, vocab=V, **kw)
    rng = np.random.default_rng(7 + case)
    alphabet = np.array([0, 3, 5, 11, 20, 21, 22, 33, 40, 41, 50, 60, 70, 90, V - 1])
    hists = [[], [20], [21], [33, 40], [20, 21], [7, 22], [40, 41, 50], [33, 40, 41], [5, 40, 41, 50], [3, 33, 11], [60, 20]]
    hists += [alphabet[rng.integers(0, len(alphabet), size=n)].tolist() for n in (1, 2, 3, 4, 5, 300)]
    hists += [h + [20] for h in hists[-3:]] + [h + [40, 41] for h in hists[-3:]]          # longer than every sequence, ending in a prefix
    x = _rows(len(hists), seed=case)
    chain = _hf_chain(kw, EOS)
    for r, hist in enumerate(hists):
        want = x[r:r + 1].clone()
        for p in chain:
            want = p(torch.tensor([hist], dtype=torch.long), want)
        got = R.process(x[r].numpy(), hist, cfg)
        assert got.dtype == np.float32
        assert np.array_equal(got.view(np.int32), want[0].numpy().view(np.int32)), (case, hist, np.nonzero(got.view(np.int32) != want[0].numpy().view(np.int32)))


def test_length_quirk_and_order():
    """a 2-id sequence does not act on a history of 1 id even though its prefix is there (HF compares len(sequence) with the ids generated);
    biases on one id add up in the table's order: the one-id sequence first"""
    cfg = LP.parse(sequence_bias={(20, 21): 1e8, (21,): 1.0, (22, 21): -1e8}, vocab=V)
    assert [k for k, _, _ in cfg.seq] == [(21,), (20, 21), (22, 21)]
    assert not R.acts((20, 21), [20]) and R.acts((20, 21), [5, 20]) and R.acts((21,), [])
    assert R.bias_row(V, [20], cfg)[21] == np.float32(1.0)
    assert R.bias_row(V, [5, 20], cfg)[21] == np.float32(np.float32(1.0) + np.float32(1e8))


def test_parse():
    assert LP.parse() is None and LP.parse(eos=[2]) is None
    c = LP.parse(bad_words_ids=[[5, 6], [2], [7]], eos=[2])
    assert c.seq == (((5, 6), float("-inf"), True), ((7,), float("-inf"), True)) and c.penalty == 1.0
    t = c.seq_table()
    assert len(t) == 2 * LP.SEQ_STRIDE and t[:6] == [2, 1, 0, 0, 5, 6] and t[12:17] == [1, 1, 0, 0, 7]
    c = LP.parse(sequence_bias=[[[5, 6], 2.0]], repetition_penalty=1.2)
    assert c.seq == (((5, 6), 2.0, False),) and c.seq_table()[:6] == [2, 0, 0x40000000, 0, 5, 6]
    assert str(LP.ProcConfig(penalty=1.3)) == "ProcConfig(penalty=1.3, ngram=0, min_new=0, eos=(), suppress=())"
    for bad in ({}, [], "x", {5: 1.0}, {(5,): 1}, {(): 1.0}, {(-1,): 1.0}, [[[5], 1]], [[[0], 1.0]], [[5, 1.0]]):
        with pytest.raises(ValueError):
            LP.parse(sequence_bias=bad)
    for bad in ([], "x", [5], [[-1]], [[1.5]], [[]]):
        with pytest.raises(ValueError):
            LP.parse(bad_words_ids=bad, eos=[2])
    assert LP.parse(bad_words_ids=[[2]], eos=[2]) is None          # only the eos id: nothing is left, as in HF's class
    with pytest.raises(ValueError, match="vocabulary size"):
        LP.parse(bad_words_ids=[[5, 97]], vocab=97)
    with pytest.raises(ValueError, match="vocabulary size"):
        LP.parse(sequence_bias={(97,): 1.0}, vocab=97)
    # the limits hold 32 sequences of 8 ids and more; beyond them: NotImplementedError
    many = LP.parse(bad_words_ids=[[i + 1] * 8 for i in range(32)], sequence_bias={(i + 1, 3): 1.0 for i in range(32)})
    assert len(many.seq) == 64 and len(many.seq_table()) == 64 * LP.SEQ_STRIDE
    with pytest.raises(NotImplementedError):
        LP.parse(bad_words_ids=[[i + 1] for i in range(65)])
    with pytest.raises(NotImplementedError):
        LP.parse(sequence_bias={tuple(range(1, 10)): 1.0})


def test_hf_refuses_the_same():
    from transformers.generation import logits_process as L
    for bad in ({}, [], {5: 1.0}, {(5,): 1}, {(): 1.0}, {(-1,): 1.0}, [[[5], 1]], [[[0], 1.0]]):
        with pytest.raises(ValueError):
            L.SequenceBiasLogitsProcessor(sequence_bias=bad)
    for bad in ([], "x", [5], [[-1]], [[1.5]]):
        with pytest.raises(ValueError):
            L.NoBadWordsLogitsProcessor(bad, torch.tensor([2]))
    assert L.NoBadWordsLogitsProcessor([[2]], torch.tensor([2])).sequence_bias == {}


def test_stream_requests_refuse_the_keywords():
    import types
    from vz_hip import sample_rows as SR
    gen = types.SimpleNamespace(top_k=50, top_p=1.0)
    for k, v in (("bad_words_ids", [[5]]), ("sequence_bias", {(5,): 1.0})):
        with pytest.raises(NotImplementedError):
            SR.parse_request({k: v}, gen, lambda: 0)
