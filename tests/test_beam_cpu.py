"""Beam-search semantics pinned against transformers itself (no GPU): a tiny seeded fp32 MistralForCausalLM generates with
`generate(inputs_embeds=..., num_beams=k, do_sample=False)`, and the same model's per-step logits drive vz_hip/beam.py - the torch
restatement of the device selection (csrc/beam.hip) plus the host replay of its records.  Same `sequences`, `sequences_scores`
within 1e-6."""
import pytest
import torch

transformers = pytest.importorskip("transformers")

from vz_hip import beam as BM  # noqa: E402

V = 128


def _model(seed=0):
    cfg = transformers.MistralConfig(vocab_size=V, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                                     num_key_value_heads=2, head_dim=16, max_position_embeddings=256, sliding_window=None,
                                     pad_token_id=0, eos_token_id=5, bos_token_id=1)
    torch.manual_seed(seed)
    m = transformers.MistralForCausalLM(cfg).float().eval()
    with torch.no_grad():          # sharper logits than the default init, so that eos ids win now and then
        m.lm_head.weight.mul_(8.0)
    return m


def _hf(m, emb, mask, nb, eos, lp, es, nrs, max_new):
    return m.generate(inputs_embeds=emb, attention_mask=mask, num_beams=nb, do_sample=False, eos_token_id=eos, pad_token_id=0,
                      length_penalty=lp, early_stopping=es, num_return_sequences=nrs, max_new_tokens=max_new,
                      return_dict_in_generate=True, output_scores=True, output_logits=True)


def _replay(out, Bsz, nb, eos, lp, es, nrs, max_new):
    """drive the restated select + replay with the logits HF's own loop computed (step t, row b * nb + j = running beam j of
    prompt b); the running beams the replay chooses must be HF's for the rows to line up."""
    replays = [BM.BeamReplay(nb, eos, max_new, lp, es) for _ in range(Bsz)]
    for t, lg in enumerate(out.logits):
        if t == 0:     # the first step considers beam 0 only (HF: running scores [0, -1e9, ...]); the device takes it from one row
            cs, ct, cp, *_ = BM.select_reference(lg[::nb].float(), None, 1, nb, eos)
            scores = None
        else:
            cs, ct, cp, *_ = BM.select_reference(lg.float(), scores, nb, nb, eos)
        nxt = []
        for b in range(Bsz):
            if not replays[b].done:
                replays[b].step(cs[b], ct[b], cp[b])
            nxt.append(replays[b].running_scores)
        scores = torch.cat(nxt)
        if all(r.done for r in replays):
            assert t == len(out.logits) - 1, "the replay stopped before HF did"
    assert all(r.done for r in replays), "HF stopped before the replay did"
    hyps = [h for r in replays for h in r.best(nrs)]
    n = max(len(tk) for tk, _ in hyps)
    seqs = torch.full((Bsz * nrs, n), BM.fill_value(0, eos), dtype=torch.long)
    for i, (tk, _) in enumerate(hyps):
        seqs[i, :len(tk)] = torch.tensor(tk, dtype=torch.long)
    return seqs, torch.tensor([sc for _, sc in hyps], dtype=torch.float32)


def _prompts(m, lens, seed=1):
    g = torch.Generator().manual_seed(seed)
    S = max(lens)
    ids = torch.randint(6, V, (len(lens), S), generator=g)
    mask = torch.zeros(len(lens), S, dtype=torch.long)
    for b, L in enumerate(lens):       # left padding, as HF's decoder-only generate expects
        mask[b, S - L:] = 1
    with torch.no_grad():
        emb = m.get_input_embeddings()(ids)
    return emb, mask


@pytest.mark.parametrize("nb", [2, 4])
@pytest.mark.parametrize("lp", [1.0, 0.0, 2.0])
@pytest.mark.parametrize("es", [False, True, "never"])
def test_beam_replay_matches_hf(nb, lp, es):
    m = _model()
    emb, mask = _prompts(m, [7])
    out = _hf(m, emb, mask, nb, [5], lp, es, 1, 12)
    seqs, sc = _replay(out, 1, nb, [5], lp, es, 1, 12)
    assert seqs.tolist() == out.sequences.tolist()
    assert torch.allclose(sc, out.sequences_scores.float(), rtol=0, atol=1e-6)


@pytest.mark.parametrize("eos", [[5], [5, 9]])
@pytest.mark.parametrize("nrs", [1, 2])
def test_beam_replay_batch_eos_and_returns(eos, nrs):
    m = _model()
    emb, mask = _prompts(m, [9, 5], seed=3)
    out = _hf(m, emb, mask, 4, eos, 1.0, False, nrs, 16)
    seqs, sc = _replay(out, 2, 4, eos, 1.0, False, nrs, 16)
    assert seqs.tolist() == out.sequences.tolist()
    assert torch.allclose(sc, out.sequences_scores.float(), rtol=0, atol=1e-6)


def test_an_eos_is_hit_before_the_length_limit():
    """the parametrised cases above are only worth something if eos ids actually end hypotheses early"""
    m = _model()
    hit = 0
    for seed in (1, 3):
        emb, mask = _prompts(m, [7] if seed == 1 else [9, 5], seed=seed)
        out = _hf(m, emb, mask, 4, [5, 9], 1.0, False, 2, 16)
        hit += int(((out.sequences == 5) | (out.sequences == 9)).any())
    assert hit >= 1


def test_select_reference_ties_go_to_the_smaller_flat_index():
    lg = torch.zeros(2, 8)                                   # two beams, every candidate equal
    vals, tok, par, nt, ns, npar = BM.select_reference(lg, torch.zeros(2), 2, 2, eos=[0])
    K = BM.beam_k(2, 1)
    assert tok[0].tolist() == list(range(K)) and par[0].tolist() == [0] * K
    assert nt.tolist() == [1, 2] and npar.tolist() == [0, 0]     # token 0 is eos: the first two others run on


def test_fill_value_follows_hf():
    assert BM.fill_value(0, [5]) == 5
    assert BM.fill_value(None, [5, 7]) == 5
    assert BM.fill_value(3, [5]) == 3
    assert BM.fill_value(3, []) == -1
