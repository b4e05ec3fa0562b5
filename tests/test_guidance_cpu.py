"""Classifier-free guidance on the CPU: the reference combine (tests/cfg_ref.py) against HF's own processor class
bit for bit, the two-branch scheme against HF's `generate(guidance_scale=..., negative_prompt_ids=...)` on a tiny fp32 Mistral, the
checks of the call's keywords (vz_hip/guidance.py), the row layout of a guided chunk against a toy engine whose cache rows hold token
histories, and the position of the guidance arming in the arming scope (vz_hip/decode_loop.py)."""
import types

import pytest
import torch

import cfg_ref
from vz_hip import decode_loop as DL
from vz_hip import guidance as GD

V = 128
SCALE = 1.7


# ---- the combine against HF's class -------------------------------------------------------------------------------------------
class _Out(dict):
    logits = None


@pytest.mark.parametrize("s", [1.5, 0.5, 3.0, -0.75])
def test_reference_combine_equals_hf_class_bits(s):
    transformers = pytest.importorskip("transformers")
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor as HFGuidance
    g = torch.Generator().manual_seed(int(s * 100) + 7)
    cond = torch.randn(3, 1000, generator=g) * 3
    preset = torch.randn(3, 4, 1000, generator=g) * 3          # what the stub model answers: [rows, positions, V]
    cond[1, 17] = -float("inf")

    def stub(input_ids, attention_mask=None, use_cache=None, past_key_values=None):
        o = _Out()
        o.logits = preset
        return o

    neg = torch.randint(0, 1000, (3, 4), generator=g)
    got = HFGuidance(s, stub, unconditional_ids=neg)(torch.zeros(3, 1, dtype=torch.long), cond.clone())
    want = cfg_ref.combine(cond, preset[:, -1], s)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert want[1, 17] == (-float("inf") if s > 0 else float("inf"))
    del transformers


# ---- the scheme against HF's generate ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    transformers = pytest.importorskip("transformers")
    cfg = transformers.MistralConfig(vocab_size=V, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                                     num_key_value_heads=2, head_dim=16, max_position_embeddings=256, sliding_window=None,
                                     pad_token_id=0, eos_token_id=5, bos_token_id=1)
    torch.manual_seed(0)
    m = transformers.MistralForCausalLM(cfg).float().eval()
    with torch.no_grad():
        m.lm_head.weight.mul_(8.0)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(6, V, (2, 9), generator=g)
    neg = torch.randint(6, V, (2, 7), generator=g)
    mask = torch.ones(2, 7, dtype=torch.long)
    mask[1, :3] = 0                                              # negative prompts of 7 and 4 ids, left-padded as HF's generate expects
    return types.SimpleNamespace(tf=transformers, m=m, ids=ids, neg=neg, mask=mask)


def _hf_generate(t, from_embeds, guided, max_new, **kw):
    src = {"inputs_embeds": t.m.get_input_embeddings()(t.ids)} if from_embeds else {"input_ids": t.ids}
    if guided:
        kw.update(guidance_scale=SCALE, negative_prompt_ids=t.neg, negative_prompt_attention_mask=t.mask)
    with torch.no_grad():
        out = t.m.generate(**src, attention_mask=torch.ones_like(t.ids), do_sample=False, max_new_tokens=max_new, eos_token_id=V + 7,
                           pad_token_id=0, **kw)      # (an eos id outside the vocabulary: no row ever ends)
    return out if from_embeds else out[:, t.ids.shape[1]:]


@pytest.mark.parametrize("from_embeds", [False, True])
@pytest.mark.parametrize("with_proc", [False, True])
def test_pair_loop_equals_hf_generate(tiny, from_embeds, with_proc):
    t, max_new = tiny, 10
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2) if with_proc else {}
    want = _hf_generate(t, from_embeds, True, max_new, **kw)
    LP = t.tf.generation.logits_process
    procs = (LP.RepetitionPenaltyLogitsProcessor(1.3), LP.NoRepeatNGramLogitsProcessor(2)) if with_proc else ()
    src = {"inputs_embeds": t.m.get_input_embeddings()(t.ids)} if from_embeds else {"input_ids": t.ids}
    got = cfg_ref.pair_loop(t.m, SCALE, t.neg, t.mask, max_new, processors=procs, **src)
    assert got.tolist() == want.tolist()
    plain = _hf_generate(t, from_embeds, False, max_new, **kw)
    assert any(g[:6] != p[:6] for g, p in zip(got.tolist(), plain.tolist())), "guidance did not change the ids: the case shows nothing"


# ---- the call's keywords ---------------------------------------------------------------------------------------------------------
def test_parse_off_values():
    neg = torch.ones(2, 3, dtype=torch.long)
    gen = types.SimpleNamespace()
    assert GD.parse(None, None, None, None, 2, gen) is None
    assert GD.parse(None, neg, None, None, 2, gen) is None               # negative ids without a scale: ignored, as in HF
    assert GD.parse(1, neg, None, None, 2, gen) is None and GD.parse(1.0, neg, None, None, 2, gen) is None
    assert GD.parse(None, neg, None, None, 2, types.SimpleNamespace(guidance_scale=None)) is None
    assert GD.parse(None, neg, None, None, 2, types.SimpleNamespace(guidance_scale=1.0)) is None


def test_parse_takes_scales_and_the_config_default():
    neg = torch.ones(2, 3, dtype=torch.long)
    for s in (1.5, 0.5, 3, -1.0, 0.0):
        scale, ids, mask = GD.parse(s, neg, None, None, 2, None)
        assert scale == float(s) and isinstance(scale, float) and torch.equal(ids, neg) and mask is None
    scale, _, mask = GD.parse(None, neg.tolist(), torch.ones(2, 3), None, 2, types.SimpleNamespace(guidance_scale=2.5))
    assert scale == 2.5 and tuple(mask.shape) == (2, 3)
    assert GD.parse(1.5, neg, None, None, 2, types.SimpleNamespace(guidance_scale=2.5))[0] == 1.5      # the keyword wins


def test_parse_refusals():
    neg = torch.ones(2, 3, dtype=torch.long)
    with pytest.raises(ValueError, match="no last prompt id to fall back on"):
        GD.parse(1.5, None, None, None, 2, None)
    with pytest.raises(ValueError, match="one row per prompt"):
        GD.parse(1.5, neg, None, None, 3, None)
    with pytest.raises(ValueError, match="one row per prompt"):
        GD.parse(1.5, neg[0], None, None, 1, None)
    with pytest.raises(ValueError, match="does not match"):
        GD.parse(1.5, neg, torch.ones(2, 4), None, 2, None)
    with pytest.raises(ValueError, match="finite"):
        GD.parse(float("nan"), neg, None, None, 2, None)
    with pytest.raises(ValueError, match="finite"):
        GD.parse(float("inf"), neg, None, None, 2, None)
    sent = neg.clone()
    sent[1, 1] = -200
    with pytest.raises(ValueError, match="image sentinels"):
        GD.parse(1.5, sent, None, None, 2, None, image_token_index=-200)
    assert GD.parse(1.5, sent, None, object(), 2, None, image_token_index=-200) is not None      # with images: the splice takes them


def test_prompts_per_chunk():
    assert [GD.prompts_per_chunk(mb) for mb in (2, 3, 4, 9, 64, 200)] == [1, 1, 2, 4, 32, 32]
    assert GD.prompts_per_chunk(8, 2) == 2 and GD.prompts_per_chunk(9, 4) == 1 and GD.prompts_per_chunk(64, 3) == 10
    with pytest.raises(ValueError, match="two KV-cache rows"):
        GD.prompts_per_chunk(1)
    with pytest.raises(ValueError, match="num_return_sequences = 3"):
        GD.prompts_per_chunk(4, 3)


# ---- the row layout of a guided chunk ---------------------------------------------------------------------------------------------
class PairEngine:
    """cache row r holds the ids of the sequence prefilled (or moved) into it; rows of a running batch may only be touched while parked"""

    def __init__(self, max_batch):
        self.max_batch, self.rows, self.dec_B, self.parked, self.log = max_batch, [None] * max_batch, 0, True, []

    def _fill(self, row0, emb, seqlens, position_ids):
        assert row0 + emb.shape[0] <= self.max_batch
        logits = torch.zeros(emb.shape[0], 8)
        for j, L in enumerate(seqlens):
            assert position_ids is None or position_ids.shape[1] >= L
            self.rows[row0 + j] = [int(v) for v in emb[j, :L, 0].tolist()]
            logits[j, 0] = float(sum(self.rows[row0 + j]))
        return logits

    def prefill(self, emb, seqlens, position_ids=None, all_logits=False, last_logits=True):
        self.log.append(("prefill", emb.shape[0]))
        return None, self._fill(0, emb, seqlens, position_ids)

    def prefill_rows(self, row0, emb, seqlens, position_ids=None):
        self.log.append(("prefill_rows", row0, emb.shape[0]))
        return self._fill(row0, emb, seqlens, position_ids)

    def decode_begin(self, first, next_pos, ctx_len):
        assert all(c == 0 for c in ctx_len) and all(p == 0 for p in next_pos)
        self.dec_B = len(ctx_len)
        self.log.append(("park", self.dec_B))

    def kv_move_rows(self, src, dst, lens):
        assert len(set(dst)) == len(dst) and not set(dst) & set(src) and all(d < self.dec_B for d in dst)
        for s_, d_, n in zip(src, dst, lens):
            assert n == len(self.rows[s_])
            self.rows[d_] = list(self.rows[s_][:n])
        self.log.append(("move", len(dst)))


def _seqs(lens, base):
    emb = torch.zeros(len(lens), max(lens), 1)
    for i, L in enumerate(lens):
        emb[i, :L, 0] = torch.arange(L) + base * (i + 1)
    return emb


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("with_pos", [False, True])
def test_pair_prefill_layout(G, n, with_pos):
    lens, nlens = [5, 9, 7][:G], [4, 2, 6][:G]
    emb, nemb = _seqs(lens, 100), _seqs(nlens, 1000)
    pos = (torch.arange(max(lens)) + 3).repeat(G, 1) if with_pos else None          # (a spliced prompt's positions: shifted)
    npos = (torch.arange(max(nlens)) * 2).repeat(G, 1) if with_pos else None
    neg = GD.Negative(SCALE, nemb, nlens, npos)
    eng = PairEngine(2 * G * n + 1)
    last, last_u, next_pos, ctx_len = DL.pair_prefill(eng, emb, lens, pos, neg, n)
    R = G * n
    assert len(next_pos) == len(ctx_len) == 2 * R and eng.rows[2 * R] is None
    for r in range(2 * R):          # conditional rows [0, R): prompt r // n; unconditional rows [R, 2R): negative prompt (r - R) // n
        g, e, L, p = (r // n, emb, lens, pos) if r < R else ((r - R) // n, nemb, nlens, npos)
        assert eng.rows[r] == [int(v) for v in e[g, :L[g], 0].tolist()]
        assert ctx_len[r] == L[g] and next_pos[r] == (L[g] if p is None else int(p[g, L[g] - 1]) + 1)
    assert last.shape == last_u.shape == (G, 8)
    assert last[:, 0].tolist() == [float(sum(eng.rows[g * n])) for g in range(G)]
    assert last_u[:, 0].tolist() == [float(sum(eng.rows[R + g * n])) for g in range(G)]
    if n == 1:                      # one prefill for the prompts, one into the rows behind them for the negative prompts
        assert eng.log == [("prefill", G), ("prefill_rows", G, G)]
    else:                           # every sequence prefilled once, then spread
        assert eng.log[0] == ("park", 2 * R) and eng.log[-1] == ("move", 2 * G * (n - 1))
        assert sorted(c[1] for c in eng.log[1:-1]) == sorted([g * n for g in range(G)] + [R + g * n for g in range(G)])


def test_negative_rows_slices_a_chunk():
    neg = GD.Negative(SCALE, _seqs([4, 2, 6], 10), [4, 2, 6], torch.arange(6).repeat(3, 1))
    part = neg.rows(1, 3)
    assert part.scale == SCALE and part.seqlens == [2, 6] and torch.equal(part.embeds, neg.embeds[1:3]) and part.position_ids.shape == (2, 6)
    assert part.config(2) == GD.GuidanceConfig(SCALE, 2)


# ---- the arming scope ---------------------------------------------------------------------------------------------------------------
class RecordingEngine:
    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        return lambda *args: self.log.append((name,) + args)


def test_guidance_arms_behind_the_processors_and_in_front_of_the_tail():
    eng, cfg = RecordingEngine(), GD.GuidanceConfig(SCALE, 2)
    first = torch.tensor([5, 6], dtype=torch.int32)
    with DL.armed(eng, proc="PROC", sampling_rows=["ROW0", "ROW1"], scores=(4, 2, True, False), stop="PLAN", guidance=cfg) as begin:
        begin(first, [3, 4, 7, 8], [3, 4, 7, 8])
    names = [c[0] for c in eng.log]
    assert names == ["set_logits_proc", "set_guidance", "set_sampling_rows", "set_scores", "set_stop", "decode_begin", "stop_rows",
                     "set_stop", "set_scores", "set_sampling_rows", "set_guidance", "set_logits_proc"]
    assert eng.log[1] == ("set_guidance", cfg) and eng.log[-2] == ("set_guidance", None)
    ids, next_pos, ctx_len = eng.log[5][1:]
    assert ids.tolist() == [5, 6, 5, 6] and next_pos == [3, 4, 7, 8] and ctx_len == [3, 4, 7, 8]      # each first token to both rows of its pair
    assert eng.log[6][1] == 0 and eng.log[6][2].tolist() == [5, 6]                                       # the matcher watches the conditional rows


def test_guidance_alone_and_plain_call():
    eng = RecordingEngine()
    with DL.armed(eng, sampling=(True, 0.8, 50, 1.0, 3, 1), guidance=GD.GuidanceConfig(0.5, 1)) as begin:
        begin(torch.tensor([9], dtype=torch.int32), [4, 2], [4, 2])
    assert [c[0] for c in eng.log] == ["set_guidance", "set_sampling", "decode_begin", "set_sampling", "set_guidance"]
    eng = RecordingEngine()
    with DL.armed(eng) as begin:
        begin(torch.tensor([1]), [2], [2])
    assert [c[0] for c in eng.log] == ["decode_begin"] and eng.log[0][1].tolist() == [1]


def test_first_tokens_combines_in_front_of_the_processors(monkeypatch):
    from vz_hip import binding as B
    from vz_hip.sample_rows import GREEDY
    calls = []

    def fake_combine(cond, uncond, s):
        calls.append("combine")
        cond.copy_(cfg_ref.combine(cond, uncond, s))
        return cond

    def fake_proc(logits, proc):
        calls.append("proc")
        logits[:, 3] = -float("inf")

    monkeypatch.setattr(B, "cfg_combine", fake_combine)
    monkeypatch.setattr(B, "logits_process", fake_proc)
    monkeypatch.setattr(B, "argmax", lambda lg: lg.argmax(-1).to(torch.int32))
    g = torch.Generator().manual_seed(5)
    cond, uncond = torch.randn(2, 16, generator=g), torch.randn(2, 16, generator=g)
    want = cfg_ref.combine(cond, uncond, SCALE)
    want[:, 3] = -float("inf")
    first, first_cpu, blk = DL.first_tokens(cond.clone(), [GREEDY] * 2, proc="PROC", uncond=(uncond, SCALE))
    assert calls == ["combine", "proc"] and first_cpu.tolist() == want.argmax(-1).tolist() and blk is None
