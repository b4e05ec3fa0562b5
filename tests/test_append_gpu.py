"""Append prefill through the layers: `Engine.prefill_append`, `forward(past_key_values=...)` with >= 4 new tokens and
`generate(past_key_values=...)` on a 2-layer full-width synthetic model (max_batch 2, max_ctx 512).

Tolerance of "continued vs full": the two are two bf16 evaluation orders of the same arithmetic - 3e-2 max-norm / 1e-2 relative L2, what
tests/test_stages_gpu.py::test_forward_loss_on_device_and_cache_continuation holds the continued forward to."""
import pytest
import torch

from util import check_close, record

pytestmark = pytest.mark.gpu

MAX_TOL, L2_TOL = 3e-2, 1e-2
IMG = -200


@pytest.fixture(scope="module")
def env():
    from vz_hip import synth
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    cfg = synth.ArchConfig(n_layers=2)
    hf = VisZephyrConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=cfg.n_layers,
                         num_attention_heads=cfg.n_heads, num_key_value_heads=cfg.n_kv_heads, vocab_size=cfg.vocab,
                         rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta, sliding_window=cfg.sliding_window,
                         eos_token_id=2, pad_token_id=2, bos_token_id=1)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    model = VisZephyrForCausalLM.from_synthetic(hf, seed=0, max_batch=2, max_ctx=512, max_tiles=1, max_text=64)
    ids = synth.synth_ids(400, cfg.vocab, image_pos=-1, seed=77).unsqueeze(0).cuda()
    return dict(cfg=cfg, model=model, synth=synth, ids=ids, cache={})


def _full(env, n):
    """logits of one plain forward over the first n ids (computed once per length)"""
    if n not in env["cache"]:
        env["cache"][n] = env["model"](input_ids=env["ids"][:, :n]).logits[0].clone()
    return env["cache"][n]


# ---- engine -------------------------------------------------------------------------------------------------------------------------
def test_engine_prefill_append_matches_one_prefill(env):
    model, ids = env["model"], env["ids"]
    eng = model.engine
    P, T = 37, 20
    emb = model.get_model().embed_tokens(ids[:, :P + T])
    la_full, ll_full = eng.prefill(emb, [P + T], all_logits=True, last_logits=True)
    kv_full = eng.kv_cache()[:, :, 0, :, :P + T].clone()
    eng.prefill(emb[:, :P], [P], all_logits=False, last_logits=True)
    kv_head = eng.kv_cache()[:, :, 0, :, :P].clone()
    la, ll = eng.prefill_append(0, emb[:, P:], [T], [P], all_logits=True, last_logits=True)
    kv = eng.kv_cache()[:, :, 0]
    assert la.shape == (1, T, env["cfg"].vocab) and ll.shape == (1, env["cfg"].vocab)
    check_close("prefill_append logits", la[0], la_full[0, P:], MAX_TOL, L2_TOL)
    check_close("prefill_append last logits", ll[0], ll_full[0], MAX_TOL, L2_TOL)
    assert torch.equal(kv[:, :, :, :P], kv_head), "the append rewrote cached slots"
    check_close("prefill_append K of the new slots", kv[:, 0, :, P:P + T], kv_full[:, 0, :, P:], MAX_TOL, L2_TOL)
    check_close("prefill_append V of the new slots", kv[:, 1, :, P:P + T], kv_full[:, 1, :, P:], MAX_TOL, L2_TOL)


def test_engine_prefill_append_argument_checks(env):
    model, ids = env["model"], env["ids"]
    eng = model.engine
    emb = model.get_model().embed_tokens(ids[:, :8])
    eng.prefill(emb, [8], all_logits=False, last_logits=True)
    for new, past in (([0], [8]), ([9], [8]), ([8], [-1]), ([8], [505])):
        with pytest.raises(ValueError):
            eng.prefill_append(0, emb, new, past)
    with pytest.raises(ValueError):
        eng.prefill_append(2, emb, [8], [8])


# ---- forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [5, 40, 300])          # 300: above the row count at which the append runs the flash kernel with q_pos0
def test_forward_append_matches_full_forward(env, T):
    model, ids = env["model"], env["ids"]
    P = 37
    full = _full(env, P + T)
    head = model(input_ids=ids[:, :P])
    step = model(input_ids=ids[:, P:P + T], past_key_values=head.past_key_values)
    assert step.logits.shape == (1, T, env["cfg"].vocab) and step.past_key_values.lengths == [P + T]
    check_close(f"forward append T={T}", step.logits[0], full[P:], MAX_TOL, L2_TOL)
    # and the handle it returns continues: one more token by a decode step
    last = model(input_ids=ids[:, P + T:P + T + 1], past_key_values=step.past_key_values)
    check_close(f"forward append T={T}, then one token", last.logits[0, 0], _full(env, P + T + 1)[P + T], MAX_TOL, L2_TOL)
    with pytest.raises(ValueError):
        model(input_ids=ids[:, :4], past_key_values=head.past_key_values)          # stale


@pytest.mark.parametrize("T", [6, 260])              # 260: one flash launch per run of rows with equal past
def test_forward_append_rows_of_different_cached_length(env, T):
    model, synth, cfg = env["model"], env["synth"], env["cfg"]
    lens = (37, 20)
    rows = [synth.synth_ids(lens[b] + T, cfg.vocab, image_pos=-1, seed=90 + b).cuda() for b in range(2)]
    alone = [model(input_ids=rows[b].unsqueeze(0)).logits[0].clone() for b in range(2)]
    ids = torch.full((2, max(lens)), 2, dtype=torch.long, device="cuda")
    mask = torch.zeros(2, max(lens), dtype=torch.long, device="cuda")
    for b in range(2):
        ids[b, :lens[b]] = rows[b][:lens[b]]
        mask[b, :lens[b]] = 1
    head = model(input_ids=ids, attention_mask=mask)
    assert head.past_key_values.lengths == list(lens)
    step = model(input_ids=torch.stack([rows[b][lens[b]:] for b in range(2)]), past_key_values=head.past_key_values)
    assert step.past_key_values.lengths == [l + T for l in lens]
    for b in range(2):
        check_close(f"forward append, row {b} of lengths {lens}", step.logits[b], alone[b][lens[b]:], MAX_TOL, L2_TOL)


def test_forward_below_append_min_new_is_the_decode_path_bit_for_bit(env):
    model, ids = env["model"], env["ids"]
    P = 37
    head = model(input_ids=ids[:, :P])
    three = model(input_ids=ids[:, P:P + 3], past_key_values=head.past_key_values).logits.clone()
    pkv = model(input_ids=ids[:, :P]).past_key_values
    for t in range(3):
        one = model(input_ids=ids[:, P + t:P + t + 1], past_key_values=pkv)
        assert torch.equal(one.logits[0, 0], three[0, t]), t
        pkv = one.past_key_values


def test_forward_append_max_ctx_overflow(env):
    model, ids = env["model"], env["ids"]
    head = model(input_ids=ids[:, :37])
    with pytest.raises(ValueError, match="max_ctx"):
        model(input_ids=torch.cat([ids] * 2, 1)[:, :480], past_key_values=head.past_key_values)


# ---- generate -----------------------------------------------------------------------------------------------------------------------
def _near_tie(row, tok) -> bool:
    """`tok` is the row's argmax, or within a few bf16-band errors of it (the criterion of
    tests/test_stages_gpu.py::test_continuous_batching_default_knobs_near_tie; 2e-2 = the bf16 band of this 2-layer model's logits)"""
    row = row.double().cpu()
    return float(row.max() - row[tok]) < 4.0 * 2e-2 * float(row.pow(2).mean().sqrt())


def _turn1(env, n_new=8):
    model, synth, cfg = env["model"], env["synth"], env["cfg"]
    tiles = synth.synth_tiles(1, seed=1)
    ids1 = synth.synth_ids(16, cfg.vocab, image_pos=3, seed=2).unsqueeze(0)
    out = model.generate(input_ids=ids1, images=[tiles], do_sample=False, max_new_tokens=n_new, eos_token_id=None, return_dict_in_generate=True)
    new = synth.synth_ids(12, cfg.vocab, image_pos=-1, seed=3).unsqueeze(0)
    conv = torch.cat([ids1, out.sequences.cpu(), new], 1)
    return out, ids1, tiles, new, conv


def test_generate_continues_on_the_returned_handle(env):
    model, cfg = env["model"], env["cfg"]
    out1, ids1, tiles, new, conv = _turn1(env)
    e1 = out1.sequences[0].tolist()
    h = out1.past_key_values
    S1 = 15 + cfg.qf_queries                                   # the spliced prompt: 16 ids, one of them 32 visual tokens
    # bookkeeping: the prompt positions + every emitted token but the last; the ids as given + the emitted ids but the last
    assert h.lengths == [S1 + 7] and h.next_pos == [S1 + 7] and h.ids == [ids1[0].tolist() + e1[:-1]]
    n2 = 6
    out2 = model.generate(input_ids=conv, images=[tiles], past_key_values=h, do_sample=False, max_new_tokens=n2, eos_token_id=None,
                          return_dict_in_generate=True)
    got = out2.sequences[0].tolist()
    h2 = out2.past_key_values
    fed = e1[-1:] + new[0].tolist()
    assert h2.lengths == [S1 + 7 + len(fed) + n2 - 1] and h2.ids == [conv[0].tolist() + got[:-1]]
    # the reference: the same position sequence - turn 1's spliced embeddings, then the embeddings of every id fed since - through
    # plain forwards that build their cache from scratch; greedy ids may differ only behind a near-tie of the reference's own logits
    # (tests/test_stages_gpu.py::test_continuous_batching_default_knobs_near_tie's criterion)
    (_, _, _, _, emb1, _) = model.prepare_inputs_labels_for_multimodal(ids1.to(model.device), None, None, None, None, [tiles], None)
    assert emb1.shape[1] == S1
    want = []
    for t in range(n2):
        tail = torch.tensor([e1[:-1] + fed + want], dtype=torch.long, device=model.device)
        row = model(inputs_embeds=torch.cat([emb1, model.get_model().embed_tokens(tail)], 1)).logits[0, -1].double().cpu()
        if got[t] != int(row.argmax()):
            gap = float(row.max() - row[got[t]])
            tol = 4.0 * 2e-2 * float(row.pow(2).mean().sqrt())
            record("generate append near-tie", step=t, gap=gap, tolerance=tol)
            assert gap < tol, f"turn 2 leaves the from-scratch ids at step {t} with a logit gap {gap:.3e} (tolerance {tol:.3e})"
            break
        want.append(got[t])


def test_generate_sampled_continuation_is_reproducible(env):
    model = env["model"]
    runs = []
    for _ in range(2):
        out1, _, _, _, conv = _turn1(env)
        runs.append(model.generate(input_ids=conv, past_key_values=out1.past_key_values, do_sample=True, temperature=0.8, top_p=0.9, seed=5,
                                   max_new_tokens=6, eos_token_id=None)[0].tolist())
    assert runs[0] == runs[1] and len(runs[0]) == 6


def test_generate_batch_continues_rows_of_different_length(env):
    model, synth, cfg = env["model"], env["synth"], env["cfg"]
    lens = (14, 9)
    rows = [synth.synth_ids(lens[b], cfg.vocab, image_pos=-1, seed=40 + b) for b in range(2)]
    ids = torch.full((2, max(lens)), 2, dtype=torch.long)
    mask = torch.zeros(2, max(lens), dtype=torch.long)
    for b in range(2):
        ids[b, :lens[b]] = rows[b]
        mask[b, :lens[b]] = 1
    out1 = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, max_new_tokens=5, eos_token_id=None, return_dict_in_generate=True)
    h = out1.past_key_values
    assert h.lengths == [l + 4 for l in lens]
    add = [synth.synth_ids(n, cfg.vocab, image_pos=-1, seed=50 + n).tolist() for n in (7, 4)]
    conv = [rows[b].tolist() + out1.sequences[b].tolist() + add[b] for b in range(2)]
    L = max(len(c) for c in conv)
    ids2 = torch.full((2, L), 2, dtype=torch.long)
    mask2 = torch.zeros(2, L, dtype=torch.long)
    for b in range(2):                                          # left-padded this time: the planner drops the pads
        ids2[b, L - len(conv[b]):] = torch.tensor(conv[b])
        mask2[b, L - len(conv[b]):] = 1
    # a sampled batch loops its sequences through cache row 0: it cannot continue two kept rows, says so, and leaves the handle live
    with pytest.raises(NotImplementedError, match="one sequence at a time"):
        model.generate(input_ids=ids2, attention_mask=mask2, past_key_values=h, do_sample=True, max_new_tokens=1)
    got = model.generate(input_ids=ids2, attention_mask=mask2, past_key_values=h, do_sample=False, max_new_tokens=1, eos_token_id=None)
    for b in range(2):                                          # the first token of each row against that row's own full forward
        assert _near_tie(model(input_ids=torch.tensor([conv[b]], device=model.device)).logits[0, -1], int(got[b, 0])), b


def test_generate_handle_refusals(env):
    model, cfg = env["model"], env["cfg"]
    out1, ids1, tiles, new, conv = _turn1(env, n_new=3)
    h = out1.past_key_values
    changed = conv.clone()
    changed[0, 5] += 1
    with pytest.raises(ValueError, match="index 5"):
        model.generate(input_ids=changed, past_key_values=h, max_new_tokens=2)
    with_img = conv.clone()
    with_img[0, -2] = IMG
    with pytest.raises(NotImplementedError, match="image"):
        model.generate(input_ids=with_img, past_key_values=h, max_new_tokens=2)
    with pytest.raises(NotImplementedError, match="no new id"):
        model.generate(input_ids=conv[:, :16 + 2], past_key_values=h, max_new_tokens=2)
    # the refused combinations, each naming itself; none of them consumes the handle
    with pytest.raises(NotImplementedError, match="num_beams"):
        model.generate(input_ids=conv, past_key_values=h, num_beams=2, max_new_tokens=2)
    with pytest.raises(NotImplementedError, match="guidance"):
        model.generate(input_ids=conv, past_key_values=h, guidance_scale=1.5, negative_prompt_ids=env["ids"][:, :4].cpu(), max_new_tokens=2)
    with pytest.raises(NotImplementedError, match="num_return_sequences"):
        model.generate(input_ids=conv, past_key_values=h, do_sample=True, num_return_sequences=2, max_new_tokens=2)
    with pytest.raises(NotImplementedError, match="max_batch"):
        model.generate(input_ids=torch.cat([conv] * 3), past_key_values=h, max_new_tokens=2)
    # a handle of forward() knows positions, not ids: the caller's ids must reach past them
    fw = model(input_ids=env["ids"][:, :20])
    with pytest.raises(ValueError, match="holds 20"):
        model.generate(input_ids=env["ids"][:, :12], past_key_values=fw.past_key_values, max_new_tokens=2)
    got = model.generate(input_ids=env["ids"][:, :26], past_key_values=fw.past_key_values, do_sample=False, max_new_tokens=2, eos_token_id=None)
    assert got.shape == (1, 2) and _near_tie(_full(env, 26)[-1], int(got[0, 0]))
    # ... and that call made every earlier handle stale
    with pytest.raises(ValueError, match="stale"):
        model.generate(input_ids=conv, past_key_values=h, max_new_tokens=2)


def test_refused_continued_calls_leave_the_handle_live(env):
    model = env["model"]
    out1, _, _, _, conv = _turn1(env, n_new=3)
    h = out1.past_key_values
    with pytest.raises(ValueError, match="max_ctx"):
        model.generate(input_ids=conv, past_key_values=h, max_new_tokens=600)
    with pytest.raises(NotImplementedError, match="num_beams"):
        model.generate(input_ids=conv, past_key_values=h, num_beams=3, max_new_tokens=2)
    with pytest.raises(ValueError, match="tokenizer"):
        model.generate(input_ids=conv, past_key_values=h, stop_strings=["x"], max_new_tokens=2)
    assert model.generate(input_ids=conv, past_key_values=h, do_sample=False, max_new_tokens=2, eos_token_id=None).shape == (1, 2)


def _continued(env, **kw):
    """turn 1 again (a handle serves one call), then the continued greedy call with `kw`"""
    out1, ids1, _, new, conv = _turn1(env, n_new=3)
    kw.setdefault("eos_token_id", None)
    return model_generate(env, conv, out1.past_key_values, **kw), ids1, new, conv


def model_generate(env, conv, handle, **kw):
    return env["model"].generate(input_ids=conv, past_key_values=handle, do_sample=False, **kw)


def test_continued_call_processors_see_the_cached_ids(env):
    """repetition_penalty on a continued call penalises ids that occur only in the cached part - at the first token (chosen outside the
    step) and in the steps (the engine's seeded history) - and min_new_tokens still counts the new tokens from 0"""
    p, eos = 1.5, 777
    out, ids1, new, conv = _continued(env, max_new_tokens=4, repetition_penalty=p, min_new_tokens=2, eos_token_id=[eos],
                                      return_dict_in_generate=True, output_scores=True, output_logits=True)
    cached_only = [t for t in ids1[0].tolist() if t >= 0 and t not in new[0].tolist()][:4]
    fed = set(conv[0].tolist())
    outside = next(t for t in range(1000, 2000) if t not in fed and t != eos and t not in out.sequences[0].tolist())
    assert len(out.scores) >= 3 and cached_only
    for step in range(3):
        raw, got = out.logits[step][0].float().cpu(), out.scores[step][0].float().cpu()
        for t in cached_only:
            want = raw[t] * p if raw[t] < 0 else raw[t] / p
            assert got[t] == want, (step, t, float(raw[t]), float(got[t]))
        assert got[outside] == raw[outside], step
        assert (got[eos] == float("-inf")) == (step < 2), (step, float(got[eos]))


def test_continued_call_stop_string_across_the_boundary(env):
    """a stop string that begins in the last cached id and ends in the first new token stops the call at that token, on the device and
    on the host; one inside the new tokens stops where it always did"""
    import stop_ref as R
    wide = R.fixed_width_tokenizer(env["cfg"].vocab)
    free, _, new, conv = _continued(env, max_new_tokens=6)
    free = free[0].tolist()
    across = wide.text([int(conv[0, -1]), free[0]])
    assert _continued(env, max_new_tokens=6, stop_strings=[across], tokenizer=wide)[0][0].tolist() == free[:1]
    assert _continued(env, max_new_tokens=6, stop_strings=[across], tokenizer=wide, device_stop=False)[0][0].tolist() == free[:1]
    inside = wide.text(free[1:3])
    assert _continued(env, max_new_tokens=6, stop_strings=[inside], tokenizer=wide)[0][0].tolist() == free[:3]
    # the same string on a fresh call over the suffix alone does not see the cached id: it runs to the end
    plain = env["model"].generate(input_ids=new, do_sample=False, max_new_tokens=6, eos_token_id=None)[0].tolist()
    got = env["model"].generate(input_ids=new, do_sample=False, max_new_tokens=6, eos_token_id=None,
                                stop_strings=[wide.text([int(new[0, -1]), plain[0]])], tokenizer=wide)[0].tolist()
    assert got == plain


def test_plain_paths_unchanged_by_an_append_call(env):
    model, ids = env["model"], env["ids"]
    prompt = ids[:, :30].cpu()

    def plain():
        return (model.generate(input_ids=prompt, do_sample=False, max_new_tokens=6, eos_token_id=None).clone(),
                model(input_ids=ids[:, :45]).logits.clone())

    g0, f0 = plain()
    head = model(input_ids=ids[:, :37])
    model(input_ids=ids[:, 37:60], past_key_values=head.past_key_values)
    out1, _, _, _, conv = _turn1(env, n_new=3)
    model.generate(input_ids=conv, past_key_values=out1.past_key_values, do_sample=False, max_new_tokens=3, eos_token_id=None)
    g1, f1 = plain()
    assert torch.equal(g0, g1) and torch.equal(f0, f1)
