"""tests/logits_proc_ref.py against HF's own processor classes (bit for bit) and against MistralForCausalLM.generate from
inputs_embeds (ids), and vz_hip.logits_proc.parse.  No GPU."""
import numpy as np
import pytest
import torch

import logits_proc_ref as R
from vz_hip import logits_proc as LP

V = 97


def _rows(n, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, V, generator=g) * 3).float()
    x[:, 3] = 0.0                       # exact zero, a negative, -inf: the alphabet below reaches all three
    x[:, 5] = -1.5
    x[:, 7] = float("-inf")
    x[:, 11] = -0.0
    return x


def _hf_chain(cfg):
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor, SuppressTokensLogitsProcessor)
    chain = []
    if cfg.penalty != 1.0:
        chain.append(RepetitionPenaltyLogitsProcessor(penalty=cfg.penalty))
    if cfg.ngram > 0:
        chain.append(NoRepeatNGramLogitsProcessor(cfg.ngram))
    if cfg.min_new > 0:
        chain.append(MinNewTokensLengthLogitsProcessor(0, cfg.min_new, list(cfg.eos), device="cpu"))
    if cfg.suppress:
        chain.append(SuppressTokensLogitsProcessor(list(cfg.suppress), device="cpu"))
    return chain


@pytest.mark.parametrize("cfg", [
    LP.ProcConfig(penalty=1.3), LP.ProcConfig(penalty=0.7), LP.ProcConfig(ngram=1), LP.ProcConfig(ngram=2), LP.ProcConfig(ngram=3),
    LP.ProcConfig(ngram=8), LP.ProcConfig(min_new=4, eos=(5, 90)), LP.ProcConfig(suppress=(0, 7, 96)),
    LP.ProcConfig(penalty=1.3, ngram=2, min_new=301, eos=(3,), suppress=(11, 20)),
], ids=str)
def test_reference_equals_hf_processors_bitwise(cfg):
    rng = np.random.default_rng(7)
    alphabet = np.array([0, 3, 5, 7, 11, 20, 21, 22, 33, 40, 41, 50, 60, 70, 90, V - 1])
    g = max(cfg.ngram, 2)
    lens = [0, 1, g - 1, g, 300]
    x = _rows(len(lens), V, seed=1)
    for r, n in enumerate(lens):
        hist = alphabet[rng.integers(0, 16, size=n)].tolist()
        ids = torch.tensor([hist], dtype=torch.long)
        want = x[r:r + 1].clone()
        for p in _hf_chain(cfg):
            want = p(ids, want)
        got = R.process(x[r].numpy(), hist, cfg)
        assert got.dtype == np.float32
        assert np.array_equal(got.view(np.int32), want[0].numpy().view(np.int32)), (cfg, n)


@pytest.fixture(scope="module")
def tiny():
    from transformers import MistralConfig, MistralForCausalLM
    torch.manual_seed(0)
    cfg = MistralConfig(vocab_size=V, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                        num_key_value_heads=2, max_position_embeddings=128, sliding_window=None, bos_token_id=None, eos_token_id=None,
                        pad_token_id=None)
    m = MistralForCausalLM(cfg).float().eval()
    prompt = torch.randn(1, 7, 64)
    return m, prompt


def _hf_ids(tiny, **kw):
    m, prompt = tiny
    with torch.no_grad():
        out = m.generate(inputs_embeds=prompt, attention_mask=torch.ones(1, 7, dtype=torch.long), max_new_tokens=24, do_sample=False,
                         pad_token_id=0, **kw)
    return out[0].tolist()


def _ref_ids(tiny, cfg, eos=()):
    m, prompt = tiny
    emb = m.get_input_embeddings()

    def logits_fn(out):
        with torch.no_grad():
            x = prompt if not out else torch.cat([prompt, emb(torch.tensor([out]))], 1)
            return m(inputs_embeds=x).logits[0, -1].float().numpy()
    return R.generate(logits_fn, cfg, 24, eos)


def test_reference_loop_equals_hf_generate(tiny):
    plain = _hf_ids(tiny)
    assert len(plain) == 24 and plain == _ref_ids(tiny, None)
    t0, t1 = plain[0], plain[1]
    cases = [
        (dict(repetition_penalty=1.3), ()),
        (dict(no_repeat_ngram_size=2), ()),
        (dict(min_new_tokens=8), (t1,)),
        (dict(suppress_tokens=[t0]), ()),
        (dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=8, suppress_tokens=[t0]), (t1,)),
    ]
    for kw, eos in cases:
        cfg = LP.parse(kw.get("repetition_penalty"), kw.get("no_repeat_ngram_size"), kw.get("min_new_tokens"), kw.get("suppress_tokens"), eos)
        assert cfg is not None
        hf = _hf_ids(tiny, **kw, **(dict(eos_token_id=list(eos)) if eos else {}))
        mine = _ref_ids(tiny, cfg, eos)
        assert hf == mine, (kw, hf, mine)
        base = plain if not eos else plain[:plain.index(eos[0]) + 1]       # the plain run with this eos stops at its first occurrence
        assert hf != base, (kw, "does not change this model's plain run")


def test_parse():
    assert LP.parse() is None
    assert LP.parse(None, None, None, None, None) is None
    assert LP.parse(1.0, 0, 0, [], [2]) is None
    assert LP.parse(1.0, 0, 5, [], []) is None                  # no eos id: HF adds no min-new-tokens processor
    c = LP.parse(1.2, 3, 5, [7, 7, 9], [2])
    assert (c.penalty, c.ngram, c.min_new, c.eos, c.suppress) == (1.2, 3, 5, (2,), (7, 9))
    assert LP.parse(1.2, 0, 0, None, [2]).eos == ()             # eos ids only travel with min_new_tokens
    for bad in (0.0, -1.0, 2, "1.2"):
        with pytest.raises(ValueError):
            LP.parse(repetition_penalty=bad)
    with pytest.raises(ValueError):
        LP.parse(no_repeat_ngram_size=-1)
    with pytest.raises(ValueError):
        LP.parse(min_new_tokens=-1, eos=[2])
    with pytest.raises(NotImplementedError):
        LP.parse(no_repeat_ngram_size=9)
    with pytest.raises(NotImplementedError):
        LP.parse(suppress_tokens=list(range(17)))
    with pytest.raises(NotImplementedError):
        LP.parse(min_new_tokens=3, eos=[1, 2, 3, 4, 5])
    assert LP.parse(1.2, eos=[1, 2, 3, 4, 5]) is not None       # five eos ids without min_new_tokens are fine
    assert LP.parse(no_repeat_ngram_size=8).ngram == 8 and len(LP.parse(suppress_tokens=list(range(16))).suppress) == 16
