"""Classifier-free guidance on the device (csrc/guidance.hip): cfg_combine_kernel against float64, and generate() with
`guidance_scale` + `negative_prompt_ids` against a host loop over un-armed engine calls - prefill of both branches, then eager steps
of the same 2G rows with their raw logits handed back, the combine at op level, the processors on the host (tests/logits_proc_ref.py), the
first maximum (or a one-row draw of the sampler) as the token, and that token fed to both rows.  The loop is the reference; every case
first shows that its ids leave the plain run's within eight tokens, so a call that ignores the keywords cannot pass."""
import numpy as np
import pytest
import torch

import logits_proc_ref as R
from util import record

pytestmark = pytest.mark.gpu

NEW = 32
S = 1.5
TEMP, SEED = 0.8, 1000


# ---- kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", [1, 3, 32])
@pytest.mark.parametrize("V", [1000, 32000, 32001, 32002])
def test_combine_kernel_against_float64(pairs, V):
    _check_combine(pairs, V)


@pytest.mark.parametrize("V", [32768, 32769, 33000])
def test_combine_kernel_beyond_the_register_path(V):
    """rows of more than 32768 columns are swept from memory instead of held in registers: the last width of the one path, the first of the
    other, and a width whose quads run into a second batch"""
    _check_combine(2, V)


def _check_combine(pairs, V):
    from vz_hip import binding as B
    g = torch.Generator().manual_seed(pairs * 100003 + V)
    cond = (torch.randn(pairs, V, generator=g) * 3).float()
    uncond = (torch.randn(pairs, V, generator=g) * 3).float()
    cond[pairs - 1, V // 3] = float("-inf")
    cond[0, V - 1] = float("-inf")
    lc = torch.log_softmax(cond.double(), -1)
    lu = torch.log_softmax(uncond.double(), -1)
    hole = torch.isinf(cond)
    for s in (1.5, 0.5, 3.0):
        c, u = cond.cuda(), uncond.cuda()
        out = B.cfg_combine(c, u, s)
        assert out.data_ptr() == c.data_ptr()
        got = c.cpu()
        assert torch.equal(u.cpu(), uncond), "the unconditional rows were written"
        assert bool((got[hole] == float("-inf")).all()) and int(torch.isinf(got).sum()) == int(hole.sum()) and not bool(torch.isnan(got).any())
        ref = s * (lc - lu) + lu
        # 2e-6 relative on each log-prob row (the bound tests/test_beam_proc_gpu.py holds such rows to), carried through s * lc + (1 - s) * lu
        # (|s| + |1 - s| <= 2|s| + 1), + the fp32 rounding of the result
        bound = (2 * abs(s) + 1) * 2e-6 * torch.maximum(lc.abs(), lu.abs()) + 1e-7 * ref.abs()
        err = (got.double() - ref).abs()
        ok = ~hole
        worst = float((err[ok] / bound[ok]).max())
        record("cfg_combine", pairs=pairs, V=V, scale=s, max_abs_err=float(err[ok].max()), max_err_over_bound=worst)
        print(f"cfg_combine pairs={pairs} V={V} s={s}: max |err| {float(err[ok].max()):.3e}, max err / bound {worst:.3f}")
        assert bool((err[ok] <= bound[ok]).all()), (pairs, V, s, worst)
        c2 = cond.cuda()
        B.cfg_combine(c2, u, s)
        assert torch.equal(c2.cpu().view(torch.int32), got.view(torch.int32)), "a second call gives other bits"
        both = torch.cat([cond, uncond]).cuda()          # one [2G, V] buffer, as the decode step holds the rows
        B.cfg_combine(both[:pairs], both[pairs:], s)
        assert torch.equal(both[:pairs].cpu().view(torch.int32), got.view(torch.int32)), "one buffer and two buffers give other bits"
        assert torch.equal(both[pairs:].cpu(), uncond)


# ---- generate ------------------------------------------------------------------------------------------------------------------------
def _hf_config():
    from vz_hip import synth
    from vis_zephyr.model import VisZephyrConfig
    cfg = synth.ArchConfig(n_layers=2)
    hf = VisZephyrConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=2, num_attention_heads=32,
                         num_key_value_heads=8, vocab_size=cfg.vocab, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    return cfg, hf


@pytest.fixture(scope="module")
def model():
    """the 2-layer synthetic model of tests/test_sampling_gpu.py with 4 cache rows"""
    from vis_zephyr.model import VisZephyrForCausalLM
    return VisZephyrForCausalLM.from_synthetic(_hf_config()[1], seed=0, max_batch=4, max_ctx=256, max_tiles=1, max_text=32)


def _ids(n, seed):
    from vz_hip import synth
    return synth.synth_ids(n, 32000, image_pos=-1, seed=seed)


@pytest.fixture(scope="module")
def prompt():
    return _ids(12, 21).unsqueeze(0)


@pytest.fixture(scope="module")
def negative():
    return _ids(5, 91).unsqueeze(0)


def _padded(rows):
    L = max(r.numel() for r in rows)
    ids = torch.full((len(rows), L), 5, dtype=torch.long)
    mask = torch.zeros(len(rows), L, dtype=torch.long)
    for b, r in enumerate(rows):
        ids[b, :r.numel()] = r
        mask[b, :r.numel()] = 1
    return ids, mask


def _host_loop(model, ids, lens, neg, nlens, s, cfg=None, max_new=NEW, draw=None, n=1, keep=None):
    """The reference: ids [G * n][max_new] of the G prompts `ids` (right-padded to `lens`) under guidance against `neg` (`nlens`), from
    un-armed engine calls.  Rows as a guided chunk lays them out: conditional rows [0, G * n), unconditional rows behind them.  cfg: a
    vz_hip.logits_proc config applied on the host; draw = (temperature, top_k, top_p, seeds per row): row r's token by a one-row call of
    the sampler under seeds[r] with the draw counter = the token's index (else the first maximum); n: rows per prompt, each sequence
    prefilled once and its KV copied; keep: a dict that receives "raw" / "scores" = per step the conditional rows' logits as the lm_head
    left them / after the combine and the processors."""
    from vz_hip import binding as B
    eng = model.engine
    G, Rn = ids.shape[0], ids.shape[0] * n
    emb, nemb = (x if x.is_floating_point() else model.get_model().embed_tokens(x.to(model.device)) for x in (ids, neg))      # (ids, or embeddings [G, S, H])
    if n == 1:
        _, last = eng.prefill(emb, lens, None, all_logits=False, last_logits=True)
        last_u = eng.prefill_rows(G, nemb, nlens)
    else:
        eng.decode_begin(torch.zeros(2 * Rn, dtype=torch.int32), [0] * (2 * Rn), [0] * (2 * Rn))
        last = torch.cat([eng.prefill_rows(g * n, emb[g:g + 1, :lens[g]], [lens[g]]) for g in range(G)]).contiguous()
        last_u = torch.cat([eng.prefill_rows(Rn + g * n, nemb[g:g + 1, :nlens[g]], [nlens[g]]) for g in range(G)]).contiguous()
        src = [q * n for q in range(2 * G) for _ in range(1, n)]
        dst = [q * n + j for q in range(2 * G) for j in range(1, n)]
        eng.kv_move_rows(src, dst, [(lens + nlens)[d // n] for d in dst])
    ctx = [lens[r // n] for r in range(Rn)] + [nlens[r // n] for r in range(Rn)]
    out = [[] for _ in range(Rn)]
    if keep is not None:
        keep["raw"], keep["scores"] = [], []

    def choose(cond, uncond, t):          # cond / uncond: device rows [Rn, V] of the conditional / unconditional branch
        raw = cond.clone()
        B.cfg_combine(cond, uncond, s)
        x = cond.cpu().numpy()
        if cfg is not None:
            x = np.stack([R.process(x[r], out[r], cfg) for r in range(Rn)])
        if keep is not None:
            keep["raw"].append(raw.cpu())
            keep["scores"].append(torch.from_numpy(x.copy()))
        for r in range(Rn):
            if draw is None:
                tok = int(np.argmax(x[r]))          # first maximal index, as the argmax kernel
            else:
                tok = int(B.sample(torch.from_numpy(x[r:r + 1].copy()).cuda(), draw[0], draw[1], draw[2], draw[3][r], t)[0])
            out[r].append(tok)
        return [o[-1] for o in out]

    rep = (lambda x: x.repeat_interleave(n, dim=0).contiguous()) if n > 1 else (lambda x: x)
    toks = choose(rep(last), rep(last_u), 0)
    for t in range(1, max_new):
        at = [c + t - 1 for c in ctx]
        eng.decode_begin(torch.tensor(toks + toks, dtype=torch.int32), at, at)
        _, lg = eng.decode_steps(1, return_logits=True)
        toks = choose(lg[0, :Rn], lg[0, Rn:], t)
    return out


def _differ_early(a, b):
    return a[:8] != b[:8]


@pytest.fixture(scope="module")
def plain(model, prompt):
    return model.generate(input_ids=prompt, do_sample=False, max_new_tokens=NEW, eos_token_id=[])[0].tolist()


@pytest.fixture(scope="module")
def guided(model, prompt, negative, plain):
    """the reference ids of the one-prompt greedy case (+ its rows), computed once and shared"""
    keep = {}
    ids = _host_loop(model, prompt, [12], negative, [5], S, keep=keep)[0]
    assert len(ids) == NEW and _differ_early(ids, plain), f"guidance does not change the plain run {plain}: {ids}"
    return ids, keep


class _Streamer:
    def __init__(self):
        self.puts, self.ended = [], False

    def put(self, v):
        self.puts.append(v.reshape(-1).tolist())

    def end(self):
        self.ended = True


def _kw(prompt, negative, **more):
    return dict(input_ids=prompt, do_sample=False, max_new_tokens=NEW, eos_token_id=[], guidance_scale=S, negative_prompt_ids=negative, **more)


def test_greedy_equals_host_loop(model, prompt, negative, plain, guided):
    want = guided[0]
    got = model.generate(**_kw(prompt, negative))[0].tolist()
    print("plain", plain, "reference", want, "generate", got)
    assert got == want and got != plain


def test_processors_behind_the_combine(model, prompt, negative, plain, guided):
    from vz_hip import logits_proc as LP
    kw = dict(repetition_penalty=1.3, suppress_tokens=[guided[0][0], guided[0][3]])
    cfg = LP.parse(1.3, None, None, kw["suppress_tokens"], [])
    want = _host_loop(model, prompt, [12], negative, [5], S, cfg)[0]
    assert _differ_early(want, plain) and want != guided[0] and want[0] != guided[0][0]
    assert model.generate(**_kw(prompt, negative, **kw))[0].tolist() == want


def test_batched_equals_host_loop(model):
    rows, negs = [_ids(12, 30), _ids(9, 31)], [_ids(5, 92), _ids(9, 93)]
    ids, mask = _padded(rows)
    neg, nmask = _padded(negs)
    base = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, max_new_tokens=NEW, eos_token_id=[]).tolist()
    want = _host_loop(model, ids, [12, 9], neg, [5, 9], S)
    for b in range(2):
        assert _differ_early(want[b], base[b]), (b, want[b], base[b])
    got = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, max_new_tokens=NEW, eos_token_id=[], guidance_scale=S,
                         negative_prompt_ids=neg, negative_prompt_attention_mask=nmask).tolist()
    assert got == want


def test_streamer_and_host_criterion(model, prompt, negative, plain, guided):
    want = guided[0]
    assert _differ_early(want, plain)
    st, seen = _Streamer(), []
    got = model.generate(**_kw(prompt, negative, streamer=st, stopping_criteria=[lambda i, sc, **k: seen.append(i.shape[1]) or False]))[0].tolist()
    assert got == want and st.ended and st.puts[0] == [] and [p[0] for p in st.puts[1:]] == want
    assert seen == list(range(1, NEW + 1))


def test_prompt_lookup_takes_the_guided_path(model, prompt, negative, plain, guided):
    assert _differ_early(guided[0], plain)
    assert model.generate(**_kw(prompt, negative, prompt_lookup_num_tokens=3))[0].tolist() == guided[0]


def test_negative_images_are_spliced_like_images(model):
    """the degraded-image contrast: a negative prompt with an image sentinel of its own and another tile, spliced by
    prepare_inputs_labels_for_multimodal as the prompt is; the reference loop runs on the two spliced embeddings, so a negative branch
    that dropped or misplaced the visual tokens would leave it"""
    from vz_hip import synth
    ids = synth.synth_ids(12, 32000, image_pos=3, seed=21).unsqueeze(0)
    nids = synth.synth_ids(9, 32000, image_pos=5, seed=95).unsqueeze(0)
    tiles, worse = synth.synth_tiles(1, seed=1), synth.synth_tiles(1, seed=2)
    splice = lambda x, im: model.prepare_inputs_labels_for_multimodal(x.to(model.device), None, None, None, None, [im], None)[4]      # noqa: E731
    emb, nemb = splice(ids, tiles), splice(nids, worse)
    assert emb.shape[1] > 12 and emb.shape[1] - nemb.shape[1] == 3
    kw = dict(input_ids=ids, images=[tiles], do_sample=False, max_new_tokens=NEW, eos_token_id=[])
    base = model.generate(**kw)[0].tolist()
    want = _host_loop(model, emb, [emb.shape[1]], nemb, [nemb.shape[1]], S)[0]
    assert _differ_early(want, base)
    assert model.generate(guidance_scale=S, negative_prompt_ids=nids, negative_images=[worse], **kw)[0].tolist() == want
    with pytest.raises(ValueError, match="image sentinels"):
        model.generate(guidance_scale=S, negative_prompt_ids=nids, **kw)


# ---- sampled ---------------------------------------------------------------------------------------------------------------------------
def test_sampled_equals_host_loop(model, prompt, negative):
    kw = dict(input_ids=prompt, do_sample=True, temperature=TEMP, seed=SEED, max_new_tokens=NEW, eos_token_id=[])
    base = model.generate(**kw)[0].tolist()
    want = _host_loop(model, prompt, [12], negative, [5], S, draw=(TEMP, 50, 1.0, [SEED]))[0]          # (top_k: the generation config's 50)
    assert _differ_early(want, base)
    assert model.generate(guidance_scale=S, negative_prompt_ids=negative, **kw)[0].tolist() == want


def test_return_sequences_rows_follow_their_own_seeds(model, prompt, negative):
    """row j of the prompt draws under seed + j with its own counter: the ids that seed gives the row alone (one-row draws in the loop,
    which steps the same four rows as the call, so that both run the same kernels)"""
    want = _host_loop(model, prompt, [12], negative, [5], S, draw=(TEMP, 50, 1.0, [SEED, SEED + 1]), n=2)
    assert want[0] != want[1]
    got = model.generate(input_ids=prompt, do_sample=True, temperature=TEMP, seed=SEED, max_new_tokens=NEW, eos_token_id=[], guidance_scale=S,
                         negative_prompt_ids=negative, num_return_sequences=2).tolist()
    assert got == want


# ---- scores ----------------------------------------------------------------------------------------------------------------------------
def test_scores_and_logits_rows(model, prompt, negative, guided):
    want, keep = guided
    out = model.generate(**_kw(prompt, negative, return_dict_in_generate=True, output_scores=True, output_logits=True))
    assert out.sequences[0].tolist() == want and len(out.scores) == len(out.logits) == NEW
    V = keep["raw"][0].shape[1]
    for t in range(NEW):
        assert tuple(out.logits[t].shape) == tuple(out.scores[t].shape) == (1, V)
        assert torch.equal(out.logits[t].cpu().view(torch.int32), keep["raw"][t].view(torch.int32)), f"raw conditional logits of step {t}"
        assert torch.equal(out.scores[t].cpu().view(torch.int32), keep["scores"][t].view(torch.int32)), f"combined scores of step {t}"


def test_scores_shapes_batched(model):
    rows, negs = [_ids(12, 30), _ids(9, 31)], [_ids(5, 92), _ids(9, 93)]
    ids, mask = _padded(rows)
    neg, nmask = _padded(negs)
    keep = {}
    want = _host_loop(model, ids, [12, 9], neg, [5, 9], S, max_new=6, keep=keep)
    out = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, max_new_tokens=6, eos_token_id=[], guidance_scale=S,
                         negative_prompt_ids=neg, negative_prompt_attention_mask=nmask, return_dict_in_generate=True, output_scores=True,
                         output_logits=True)
    assert out.sequences.tolist() == want
    for t in range(6):
        assert tuple(out.scores[t].shape) == tuple(out.logits[t].shape) == (2, keep["raw"][0].shape[1])
        assert torch.equal(out.logits[t].cpu().view(torch.int32), keep["raw"][t].view(torch.int32))
        assert torch.equal(out.scores[t].cpu().view(torch.int32), keep["scores"][t].view(torch.int32))


# ---- state -----------------------------------------------------------------------------------------------------------------------------
def test_state_between_calls(model, prompt, negative, plain, guided):
    eng = model.engine
    pk = dict(input_ids=prompt, do_sample=False, max_new_tokens=NEW, eos_token_id=[])
    assert model.generate(**pk)[0].tolist() == plain
    info0 = eng.decode_info()
    assert model.generate(**_kw(prompt, negative))[0].tolist() == guided[0]
    c1 = eng.decode_info()[1]
    other = _host_loop(model, prompt, [12], negative, [5], 0.5)[0]
    assert other != guided[0]
    assert model.generate(**{**_kw(prompt, negative), "guidance_scale": 0.5})[0].tolist() == other
    c2 = eng.decode_info()[1]
    assert c2 > c1, "another guidance scale must capture the step again"
    # off again: the plain ids and the plain step's context splits
    assert model.generate(**pk)[0].tolist() == plain
    assert eng.decode_info()[0] == info0[0]
    assert model.generate(guidance_scale=1.0, negative_prompt_ids=negative, **pk)[0].tolist() == plain          # 1 = off
    # the graph key of a step with the mode off is the key it had before the mode was ever armed: the same plain call into the same
    # buffer replays the captured step (generate() itself hands every call a fresh buffer, which is part of the key)
    from vz_hip.guidance import GuidanceConfig
    buf = torch.empty(1, 2, dtype=torch.int32, device=model.device)
    first = torch.tensor([plain[0]], dtype=torch.int32)
    eng.decode_begin(first, [12], [12])
    a = eng.decode_steps(2, out=buf).cpu().tolist()
    c3 = eng.decode_info()[1]
    eng.set_guidance(GuidanceConfig(3.0, 2))
    eng.set_guidance(None)
    eng.decode_begin(first, [12], [12])
    assert eng.decode_steps(2, out=buf).cpu().tolist() == a and eng.decode_info()[1] == c3


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(model, prompt, negative):
    from vz_hip.guidance import GuidanceConfig
    with pytest.raises(NotImplementedError, match="num_beams"):
        model.generate(**_kw(prompt, negative, num_beams=2))
    with pytest.raises(ValueError, match="no last prompt id"):
        model.generate(input_ids=prompt, guidance_scale=S, max_new_tokens=4)
    with pytest.raises(ValueError, match="one row per prompt"):
        model.generate(**{**_kw(prompt, negative), "negative_prompt_ids": negative.repeat(2, 1)})
    with pytest.raises(NotImplementedError, match="generate_stream"):
        list(model.generate_stream([{"input_ids": prompt, "guidance_scale": S, "negative_prompt_ids": negative}], max_new_tokens=4))
    with pytest.raises(NotImplementedError, match="generate_stream"):
        list(model.generate_stream([{"input_ids": prompt, "negative_prompt_ids": negative}], max_new_tokens=4))
    # the engine checks what it is armed with itself
    eng = model.engine
    emb = model.get_model().embed_tokens(prompt.to(model.device).repeat(3, 1))
    eng.prefill(emb, [12] * 3)
    first = torch.tensor([7, 7, 7], dtype=torch.int32)
    try:
        with pytest.raises(ValueError):
            eng.set_guidance(GuidanceConfig(S, 3))          # 6 rows: the engine has 4
        with pytest.raises(ValueError):
            eng.set_guidance(GuidanceConfig(float("nan"), 1))
        eng.set_guidance(GuidanceConfig(S, 1))
        eng.decode_begin(first, [12] * 3, [12] * 3)
        with pytest.raises(ValueError, match="2 x 1 rows"):
            eng.decode_steps(1)
        eng.decode_begin(first[:2], [12] * 2, [12] * 2)
        eng.set_beam(True, 2, 1, [], [12], torch.zeros(2, device=model.device), torch.empty(1, 1, 4, 3, dtype=torch.int32, device=model.device))
        try:
            with pytest.raises(NotImplementedError, match="guidance"):
                eng.decode_steps(1)
        finally:
            eng.set_beam(False)
        eng.decode_begin(first[:2], [12, 13], [12, 13])
        eng.set_spec(True, D=1, history=prompt[0].tolist() + [7], budget=4)
        try:
            with pytest.raises(NotImplementedError, match="guidance"):
                eng.decode_steps(1)
        finally:
            eng.set_spec(False)
    finally:
        eng.set_guidance(None)
    eng.decode_begin(first[:2], [12] * 2, [12] * 2)
    assert tuple(eng.decode_steps(2).shape) == (2, 2)          # off: a plain two-row step again
