"""Beam search with logits processors, per-step scores and beam_indices, pinned against transformers itself (no GPU).

A tiny seeded fp32 MistralForCausalLM generates with `generate(inputs_embeds=..., num_beams=k, <processors>, output_scores=True,
output_logits=True, return_dict_in_generate=True)`.  The same model's per-step logits drive the host restatement of what the device
does (csrc/beam.hip, csrc/logits_proc.hip): torch log_softmax, HF's own processor objects on every running beam's replayed ids,
`select_reference` on the rows as they are, `BeamReplay` with its parent chains.  Equal: `sequences`, `sequences_scores` (1e-6, as
tests/test_beam_cpu.py), `beam_indices`, every processed row (HF's `scores[t]`) and `compute_transition_scores(..., beam_indices)`.

The processors have to bite for any of that to mean something: a strong one-id `sequence_bias` makes the tiny model repeat a token,
and the test counts the steps at which the repetition penalty, the n-gram ban and a two-id bad word (the first two ids of the best hypothesis
of the run without it) each change a top-K candidate; a count of 0 fails."""
import pytest
import torch

transformers = pytest.importorskip("transformers")

from beam_proc_util import BITERS, step  # noqa: E402
from test_beam_cpu import V, _model, _prompts  # noqa: E402
from vz_hip import beam as BM  # noqa: E402
from vz_hip import scores as SC  # noqa: E402

BIAS_TOKEN = 17
BIAS = {(BIAS_TOKEN,): 6.0}


def _hf(m, emb, mask, nb, eos, nrs, max_new, kw):
    return m.generate(inputs_embeds=emb, attention_mask=mask, num_beams=nb, do_sample=False, eos_token_id=eos, pad_token_id=0,
                      num_return_sequences=nrs, max_new_tokens=max_new, return_dict_in_generate=True, output_scores=True,
                      output_logits=True, **kw)


def _restate(out, Bsz, nb, eos, nrs, max_new, kw, bites):
    """-> (sequences, sequences_scores, beam_indices, scores tuple) of the restatement, fed HF's raw logits step by step"""
    replays = [BM.BeamReplay(nb, eos, max_new, 1.0, False) for _ in range(Bsz)]
    rows_all = []
    for t, lg in enumerate(out.logits):
        rows_t = torch.zeros(Bsz * nb, V)
        for b, r in enumerate(replays):
            if r.done:
                continue
            if t == 0:          # HF's num_beams rows of a prompt are identical here; the device has one and replicates it
                lp = torch.log_softmax(lg[b * nb:b * nb + 1].float(), dim=-1)
                rows, cs, ct, cp, *_ = step(kw, eos, [[]], lp, None, 1, nb, bites)
                rows = rows.expand(nb, V)
            else:
                lp = torch.log_softmax(lg[b * nb:(b + 1) * nb].float(), dim=-1)
                rows, cs, ct, cp, *_ = step(kw, eos, r.running, lp, r.running_scores, nb, nb, bites)
            assert torch.equal(rows, out.scores[t][b * nb:(b + 1) * nb]), f"step {t}, prompt {b}: the processed rows are not HF's scores"
            rows_t[b * nb:(b + 1) * nb] = rows
            r.step(cs, ct, cp)
        rows_all.append(rows_t)
        if all(r.done for r in replays):
            assert t == len(out.logits) - 1, "the replay stopped before HF did"
    assert all(r.done for r in replays), "HF stopped before the replay did"
    hyps = [h for r in replays for h in r.best(nrs)]
    n = max(len(tk) for tk, _ in hyps)
    seqs = torch.full((Bsz * nrs, n), BM.fill_value(0, eos), dtype=torch.long)
    for i, (tk, _) in enumerate(hyps):
        seqs[i, :len(tk)] = torch.tensor(tk, dtype=torch.long)
    idx = BM.flat_beam_indices([r.best_indices(nrs) for r in replays], nb)
    return seqs, torch.tensor([sc for _, sc in hyps], dtype=torch.float32), idx, tuple(rows_all)


def _keywords(m, emb, mask, nb, eos, max_new):
    """the bias alone first; then every processor but the bad word; the bad word = the first two ids of that run's best hypothesis"""
    plain = _hf(m, emb, mask, nb, eos, 1, max_new, dict(sequence_bias=BIAS))
    best = plain.sequences[0].tolist()
    assert best.count(BIAS_TOKEN) >= 2, "the bias does not make the model repeat its token"
    kw = dict(sequence_bias=BIAS, repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3, suppress_tokens=[best[0]])
    kw["bad_words_ids"] = [_hf(m, emb, mask, nb, eos, 1, max_new, kw).sequences[0].tolist()[:2]]
    return kw


def _check(m, lens, seed, nb, eos, nrs, max_new):
    emb, mask = _prompts(m, lens, seed=seed)
    kw = _keywords(m, emb, mask, nb, eos, max_new)
    out = _hf(m, emb, mask, nb, eos, nrs, max_new, kw)
    bites = {}
    seqs, sc, idx, rows = _restate(out, len(lens), nb, eos, nrs, max_new, kw, bites)
    assert seqs.tolist() == out.sequences.tolist()
    assert torch.allclose(sc, out.sequences_scores.float(), rtol=0, atol=1e-6)
    assert idx.tolist() == out.beam_indices.tolist()
    want = m.compute_transition_scores(out.sequences, out.scores, out.beam_indices)
    assert torch.equal(SC.beam_transition_scores(seqs, rows, idx, vocab_size=V), want)
    assert torch.equal(SC.beam_transition_scores(out.sequences, out.scores, out.beam_indices, vocab_size=V), want)
    return out, bites


@pytest.mark.parametrize("nb", [2, 4])
@pytest.mark.parametrize("nrs", [1, None])
def test_restatement_matches_hf_with_every_processor_biting(nb, nrs):
    m = _model()
    out, bites = _check(m, [9, 5], 3, nb, [5], nb if nrs is None else nrs, 14)
    assert set(bites) == set(BITERS) and all(v >= 1 for v in bites.values()), f"a processor never changed a candidate: {bites}"
    assert tuple(out.scores[0].shape) == (2 * nb, V) and tuple(out.beam_indices.shape) == tuple(out.sequences.shape)


def test_an_eos_ends_a_hypothesis_before_the_length_limit():
    m = _model()
    out, _ = _check(m, [9, 5], 3, 4, [5, 9], 2, 16)
    lens = (out.beam_indices >= 0).sum(-1)
    assert int(lens.min()) < 16 and bool(((out.sequences == 5) | (out.sequences == 9)).any()), "no hypothesis ended on an eos id"
    assert bool((out.beam_indices[lens < lens.max()] == -1).any())


def test_transition_scores_with_beam_indices_equal_hf():
    from transformers import GenerationMixin
    T, rows, nb, Vv = 6, 3, 4, 50
    g = torch.Generator().manual_seed(11)
    scores = tuple(torch.randn(rows * nb, Vv, generator=g) * 3 for _ in range(T))
    seq = torch.randint(0, Vv, (rows, T + 3), generator=g)          # HF takes the last (longest hypothesis) columns
    idx = torch.randint(0, rows * nb, (rows, T), generator=g, dtype=torch.int32)
    idx[0, 4:] = -1
    idx[2, 2:] = -1                                                  # the longest hypothesis has 5 tokens: the result is cut to it

    class _M(GenerationMixin):
        class config:
            vocab_size = Vv
            is_encoder_decoder = False

            @staticmethod
            def get_text_config(decoder=False):
                return _M.config

    for normalize in (False, True):
        want = GenerationMixin.compute_transition_scores(_M(), seq, scores, idx, normalize_logits=normalize)
        got = SC.beam_transition_scores(seq, scores, idx, normalize_logits=normalize)
        assert tuple(got.shape) == (rows, T) and torch.equal(got, want)
    idx[1, 5:] = -1
    want = GenerationMixin.compute_transition_scores(_M(), seq, scores, idx)
    assert tuple(want.shape) == (rows, 5) and torch.equal(SC.beam_transition_scores(seq, scores, idx), want)
    assert float(want[2, 3]) == 0.0 and float(want[0, 4]) == 0.0


def test_flat_beam_indices():
    idx = BM.flat_beam_indices([[[0, 1, 1], [0]], [[0, 3], [0, 2, 2]]], 4)
    assert idx.dtype == torch.int32 and idx.tolist() == [[0, 1, 1], [0, -1, -1], [4, 7, -1], [4, 6, 6]]


def test_the_guards_that_remain():
    assert SC.check_outputs(True, True, True, False, num_beams=4, beam_extended=True) == SC.SCORE_WARPED | SC.SCORE_RAW
    assert SC.check_outputs(False, True, True, False, num_beams=4, beam_extended=True) == 0
    with pytest.raises(NotImplementedError, match="output_logprobs"):
        SC.check_outputs(True, False, False, True, num_beams=4, beam_extended=True)
    # without the opt-in the earlier refusals stand, and the form without beams refuses beam_indices
    with pytest.raises(NotImplementedError, match="beam_extended"):
        SC.check_outputs(True, True, False, False, num_beams=4)
    with pytest.raises(NotImplementedError, match="beam_transition_scores"):
        SC.transition_scores(torch.zeros(1, 2, dtype=torch.long), (torch.zeros(1, 4),) * 2, beam_indices=torch.zeros(1, 2, dtype=torch.long))
