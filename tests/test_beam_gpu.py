"""Beam search on the MI355X (csrc/beam.hip + vz_hip/beam.py + VisZephyrForCausalLM.generate(num_beams > 1)).

1. vz_op_beam_select against the fp64 restatement (random logits, eos ids, -inf, exact ties);
2. the KV reorder against a torch gather of the cache, bit for bit;
3. generate(num_beams=4) against a host-driven beam search on the same engine (eager decode steps with their logits, the torch
   selection, kv_move_rows through spare rows, the same replay) - text-only and multimodal prompts;
4. the beam tail replayed from the decode graph equals the eager steps;
5. batches (a prompt's beams do not depend on the other prompt of its chunk), num_return_sequences, an eos hit mid-chunk;
6. num_beams=1 is the greedy path; the refused arguments raise.
"""
import os

import pytest
import torch

from util import record

pytestmark = pytest.mark.gpu

NB_ROWS = 16


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
    model = VisZephyrForCausalLM.from_synthetic(hf, seed=0, max_batch=NB_ROWS, max_ctx=256, max_tiles=1, max_text=64)
    torch.cuda.synchronize()
    return dict(cfg=cfg, model=model, synth=synth)


# ---- 1. the selection op ----------------------------------------------------------------------------------------------------
def _check_select(logits, scores, nb_in, nb_out, eos, name):
    from vz_hip import beam as BM
    from vz_hip import binding as B
    rec, nt, ns, npar = B.beam_select(logits, scores, nb_in, nb_out, eos)
    s, t, p = BM.decode_records(rec)
    rows, V = logits.shape
    G, K = rows // nb_in, BM.beam_k(nb_out, len(eos))
    lp = torch.log_softmax(logits.double(), -1)
    if scores is not None:
        lp = lp + scores.double()[:, None]
    flat = lp.reshape(G, nb_in * V).cpu()
    vals, idx = torch.sort(flat, dim=1, descending=True, stable=True)
    near = 0
    for g in range(G):
        ref_t, ref_p = (idx[g, :K] % V), (idx[g, :K] // V)
        bad = (ref_t != t[g]) | (ref_p != p[g])
        if bool(bad.any()):
            # only a candidate whose fp64 neighbour (or the K boundary) lies within 1e-5 may move
            for i in torch.nonzero(bad).view(-1).tolist():
                gap = min(float(vals[g, i] - vals[g, i + 1]), float(vals[g, i - 1] - vals[g, i]) if i > 0 else float("inf"))
                assert gap < 1e-5, f"{name}: group {g} candidate {i}: {t[g, i].item()}/{p[g, i].item()} vs {ref_t[i].item()}/{ref_p[i].item()} (gap {gap:.3e})"
                near += 1
        ref_s = flat[g].gather(0, (p[g] * V + t[g]))          # the device's own candidates, scored in fp64
        fin = torch.isfinite(ref_s)
        rel = ((s[g].double()[fin] - ref_s[fin]).abs() / ref_s[fin].abs().clamp_min(1e-30)).max().item() if bool(fin.any()) else 0.0
        assert rel <= 2e-6, f"{name}: group {g} scores rel err {rel:.3e}"
        assert bool((s[g][~fin] == ref_s[~fin].float()).all())
        assert bool((s[g][:-1] >= s[g][1:]).all()), f"{name}: candidates not sorted"
        # the next running beams: the first nb_out candidates that are not eos, in order
        keep = [i for i in range(K) if int(t[g, i]) not in eos][:nb_out]
        assert nt.view(G, nb_out)[g].cpu().tolist() == [int(t[g, i]) for i in keep]
        assert npar.view(G, nb_out)[g].cpu().tolist() == [int(p[g, i]) for i in keep]
        assert ns.view(G, nb_out)[g].cpu().tolist() == [float(s[g, i]) for i in keep]
    return s, t, p, near


@pytest.mark.parametrize("V", [32000, 32002, 1000])
@pytest.mark.parametrize("nb", [2, 4, 8, 16])
def test_beam_select_matches_fp64(env, V, nb):
    g = torch.Generator(device="cuda").manual_seed(V + nb)
    G = 2
    logits = (torch.randn(G * nb, V, device="cuda", generator=g) * 3.0).contiguous()
    scores = -torch.rand(G * nb, device="cuda", generator=g) * 20.0
    near = 0
    _, t, _, n0 = _check_select(logits, scores, nb, nb, [], f"V{V} nb{nb}")
    near += n0
    # eos ids: the best candidate of group 0 (inside the top nb) and its (K-1)-th (outside)
    eos = [int(t[0, 0]), int(t[0, 2 * nb - 1])]
    _, t2, _, n1 = _check_select(logits, scores, nb, nb, eos, f"V{V} nb{nb} eos")
    near += n1
    # the first step: one row per prompt
    _, _, p3, n2 = _check_select(logits[:G].contiguous(), None, 1, nb, eos[:1], f"V{V} nb{nb} first")
    assert int(p3.max()) == 0
    near += n2
    record("beam_select", V=V, nb=nb, near_ties=near)


def test_beam_select_inf_and_ties(env):
    V, nb = 32000, 4
    lg = torch.randn(2 * nb, V, device="cuda")
    lg[0, V // 2:] = -float("inf")                 # rows containing -inf
    lg[3, ::3] = -float("inf")
    _check_select(lg.contiguous(), torch.zeros(2 * nb, device="cuda") - 3.0, nb, nb, [7], "inf")
    # exact ties: every logit of group 1 equal and equal running scores -> the smallest flat indices, beam 0 first
    from vz_hip import beam as BM
    from vz_hip import binding as B
    lg = torch.zeros(2 * nb, V, device="cuda")
    rec, nt, _, npar = B.beam_select(lg, torch.full((2 * nb,), -1.0, device="cuda"), nb, nb, [1])
    s, t, p = BM.decode_records(rec)
    K = BM.beam_k(nb, 1)
    assert t[1].tolist() == list(range(K)) and p[1].tolist() == [0] * K
    assert nt.view(2, nb)[1].tolist() == [0, 2, 3, 4]          # token 1 is eos
    # ties across beams: token 5 of beams 1 and 3 equal and best -> beam 1 first
    lg = torch.zeros(nb, V, device="cuda")
    lg[1, 5] = lg[3, 5] = 10.0
    rec, _, _, _ = B.beam_select(lg, torch.zeros(nb, device="cuda"), nb, nb, [])
    s, t, p = BM.decode_records(rec)
    assert (t[0, :2].tolist(), p[0, :2].tolist()) == ([5, 5], [1, 3])


# ---- 2. the KV reorder ------------------------------------------------------------------------------------------------------
def test_kv_beam_reorder_is_a_gather(env):
    model = env["model"]
    eng, cfg = model.engine, env["cfg"]
    nb, G = 4, 3
    R = nb * G
    eng.decode_begin(torch.zeros(NB_ROWS, dtype=torch.int32), [0] * NB_ROWS, [0] * NB_ROWS)
    ids = torch.randint(3, cfg.vocab, (NB_ROWS, 40), generator=torch.Generator().manual_seed(5))
    eng.prefill_rows(0, eng.embed_tokens(ids.cuda()), [40] * NB_ROWS)        # distinct contents in every row
    base, end = [10, 3, 20], [37, 40, 21]
    parents = [[1, 2, 3, 0],          # a 4-cycle
               [2, 2, 2, 1],          # one parent, several children
               [0, 1, 2, 3]]          # identity
    before = eng.kv_cache().clone()
    eng.kv_beam_reorder(nb, G, base, end, torch.tensor(sum(parents, []), dtype=torch.int32))
    after = eng.kv_cache()
    want = before.clone()
    for g in range(G):
        for j in range(nb):
            want[:, :, g * nb + j, :, base[g]:end[g]] = before[:, :, g * nb + parents[g][j], :, base[g]:end[g]]
    assert torch.equal(after.view(torch.int16), want.view(torch.int16))
    assert torch.equal(after[:, :, R:].view(torch.int16), before[:, :, R:].view(torch.int16))       # rows outside the groups
    for g in range(G):
        assert torch.equal(after[:, :, g * nb:(g + 1) * nb, :, :base[g]].view(torch.int16),
                           before[:, :, g * nb:(g + 1) * nb, :, :base[g]].view(torch.int16))        # [0, base) untouched


# ---- 3. end to end against a host-driven beam search ------------------------------------------------------------------------
def _host_beam(model, emb, nb, eos, max_new, lp=1.0, es=False):
    """the same beam search driven from the host: eager decode steps (their logits), the torch selection, the KV reorder by
    kv_move_rows through spare rows, the same replay.  Returns (hypotheses, smallest fp32 gap met at a selection, steps at which
    an eos candidate finished a hypothesis before the length limit)."""
    from vz_hip import beam as BM
    eng = model.engine
    S, R = emb.shape[1], nb
    park = lambda: eng.decode_begin(torch.zeros(R, dtype=torch.int32), [0] * R, [0] * R)   # noqa: E731
    park()
    last = eng.prefill_rows(0, emb, [S])
    rep = BM.BeamReplay(nb, eos, max_new, lp, es)
    min_gap = [float("inf")]
    eos_steps = []

    def select(lg, sc, nb_in):
        cs, ct, cp, nt, ns, npar = BM.select_reference(lg, sc, nb_in, nb, eos)
        lp_all = torch.log_softmax(lg.float(), -1) + (0 if sc is None else sc[:, None])
        top = torch.sort(lp_all.reshape(-1), descending=True)[0][:cs.shape[1] + 1]
        min_gap[0] = min(min_gap[0], float((top[:-1] - top[1:]).min()))
        if rep.cur_len + 1 < max_new and any(int(t) in eos for t in ct[0, :nb].tolist()):
            eos_steps.append(rep.cur_len)
        rep.step(cs[0].cpu(), ct[0].cpu(), cp[0].cpu())
        return nt, ns, npar

    nt, ns, npar = select(last, None, 1)
    if not rep.done:
        eng.kv_move_rows([0] * (R - 1), list(range(1, R)), [S] * (R - 1))
    L = S
    while not rep.done:
        eng.decode_begin(nt.to(torch.int32), [L] * R, [L] * R)
        _, lg = eng.decode_steps(1, return_logits=True)
        L += 1
        nt, ns2, npar = select(lg[0], ns, nb)
        ns = ns2
        if rep.done:
            break
        park()
        ch = [j for j in range(R) if int(npar[j]) != j]
        if ch:
            eng.kv_move_rows([int(npar[j]) for j in ch], [R + i for i in range(len(ch))], [L] * len(ch))
            eng.kv_move_rows([R + i for i in range(len(ch))], ch, [L] * len(ch))
    return rep.best(nb), min_gap[0], eos_steps


def _compare(name, got, hyps, fill, gap):
    toks, sc = hyps[0]
    row = got.sequences[0].tolist()
    want = toks + [fill] * (len(row) - len(toks))
    if row != want:
        assert gap < 1e-4, f"{name}: {row} vs host {want} (smallest selection gap {gap:.3e})"
        record("beam_e2e_near_tie", case=name, gap=gap)
        return
    assert abs(float(got.sequences_scores[0]) - sc) <= 1e-4
    record("beam_e2e", case=name, gap=gap, n=len(toks))


def test_generate_beam_matches_host_driven_text_and_multimodal(env):
    model, cfg, S = env["model"], env["cfg"], env["synth"]
    from vz_hip import beam as BM
    ids = S.synth_ids(24, cfg.vocab, image_pos=-1, seed=11).unsqueeze(0)
    got = model.generate(input_ids=ids, num_beams=4, max_new_tokens=20, eos_token_id=None, return_dict_in_generate=True)
    hyps, gap, _ = _host_beam(model, model.engine.embed_tokens(ids.cuda()), 4, [2], 20)
    _compare("text", got, hyps, BM.fill_value(2, [2]), gap)
    tiles = S.synth_tiles(1, seed=1)
    ids = S.synth_ids(16, cfg.vocab, image_pos=3, seed=2).unsqueeze(0)
    got = model.generate(input_ids=ids, images=[tiles], num_beams=4, max_new_tokens=16, return_dict_in_generate=True)
    emb = model.prepare_inputs_labels_for_multimodal(ids.cuda(), None, None, None, None, [tiles], None)[4]
    hyps, gap, _ = _host_beam(model, emb, 4, [2], 16)
    _compare("multimodal", got, hyps, BM.fill_value(2, [2]), gap)


# ---- 4. graph replay == eager ---------------------------------------------------------------------------------------------
def test_beam_graph_equals_eager(env):
    model, cfg, S = env["model"], env["cfg"], env["synth"]
    ids = S.synth_ids(20, cfg.vocab, image_pos=-1, seed=4).unsqueeze(0)
    kw = dict(input_ids=ids, num_beams=4, max_new_tokens=24, sync_every=8, return_dict_in_generate=True)
    graph = model.generate(**kw)
    assert model.engine.decode_mode()[0]
    os.environ["VZ_NO_GRAPH"] = "1"
    try:
        eager = model.generate(**kw)
    finally:
        del os.environ["VZ_NO_GRAPH"]
    assert graph.sequences.tolist() == eager.sequences.tolist()
    assert graph.sequences_scores.tolist() == eager.sequences_scores.tolist()


# ---- 5. batches, num_return_sequences, eos ------------------------------------------------------------------------------------
def test_beam_batches_and_returns(env):
    from vz_hip import binding as B
    model, cfg, S = env["model"], env["cfg"], env["synth"]
    a = S.synth_ids(22, cfg.vocab, image_pos=-1, seed=21)
    b = S.synth_ids(15, cfg.vocab, image_pos=-1, seed=22)
    def batch(p, q):           # left padding + mask, as a tokenizer with padding_side="left" gives it
        n = max(len(p), len(q))
        ids = torch.full((2, n), 2, dtype=torch.long)
        mask = torch.zeros(2, n, dtype=torch.long)
        for r, x in enumerate((p, q)):
            ids[r, n - len(x):] = x
            mask[r, n - len(x):] = 1
        return ids, mask
    with B.tuned(splitk_mid=0):
        kw = dict(num_beams=4, max_new_tokens=12, return_dict_in_generate=True)
        ab = model.generate(input_ids=batch(a, b)[0], attention_mask=batch(a, b)[1], **kw)
        aa = model.generate(input_ids=batch(a, a)[0], attention_mask=batch(a, a)[1], **kw)
        bb = model.generate(input_ids=batch(b, b)[0], attention_mask=batch(b, b)[1], **kw)
    # 8 rows in every call: each prompt's beams are what that prompt gives next to itself
    assert ab.sequences[0].tolist() == aa.sequences[0].tolist() and ab.sequences[1].tolist() == bb.sequences[0].tolist()
    assert ab.sequences_scores.tolist() == [aa.sequences_scores[0].item(), bb.sequences_scores[0].item()]
    two = model.generate(input_ids=a.unsqueeze(0), num_beams=4, max_new_tokens=12, num_return_sequences=2, return_dict_in_generate=True)
    one = model.generate(input_ids=a.unsqueeze(0), num_beams=4, max_new_tokens=12, return_dict_in_generate=True)
    assert two.sequences.shape[0] == 2 and float(two.sequences_scores[0]) >= float(two.sequences_scores[1])
    assert two.sequences[0].tolist() == one.sequences[0].tolist()


def test_beam_eos_hit_mid_chunk(env):
    from vz_hip import beam as BM
    model, cfg, S = env["model"], env["cfg"], env["synth"]
    ids = S.synth_ids(18, cfg.vocab, image_pos=-1, seed=31).unsqueeze(0)
    free = model.generate(input_ids=ids, num_beams=4, max_new_tokens=20, eos_token_id=[], return_dict_in_generate=True)
    e = int(free.sequences[0, 5])                      # taken at step 5 of the free run: inside the first 16-step chunk
    got = model.generate(input_ids=ids, num_beams=4, max_new_tokens=20, eos_token_id=e, pad_token_id=0, return_dict_in_generate=True)
    hyps, gap, eos_steps = _host_beam(model, model.engine.embed_tokens(ids.cuda()), 4, [e], 20)
    # the eos id finished a hypothesis inside the first 16-step chunk (not on its last step): the replay took it mid-chunk
    assert any(1 <= st <= 15 for st in eos_steps), eos_steps
    _compare("eos", got, hyps, BM.fill_value(0, [e]), gap)
    record("beam_eos", eos_steps=eos_steps, best_len=len(hyps[0][0]))


# ---- 6. guards ------------------------------------------------------------------------------------------------------------------
def test_beam_guards(env):
    model, cfg, S = env["model"], env["cfg"], env["synth"]
    ids = S.synth_ids(12, cfg.vocab, image_pos=-1, seed=41).unsqueeze(0)
    assert model.generate(input_ids=ids, num_beams=1, max_new_tokens=6).tolist() == model.generate(input_ids=ids, max_new_tokens=6).tolist()
    with pytest.raises(NotImplementedError):
        model.generate(input_ids=ids, num_beams=2, do_sample=True, max_new_tokens=4)
    with pytest.raises(ValueError):
        model.generate(input_ids=ids, num_beams=2, streamer=object(), max_new_tokens=4)
    with pytest.raises(NotImplementedError):
        model.generate(input_ids=ids, num_beams=2, stopping_criteria=[lambda *a: False], max_new_tokens=4)
    with pytest.raises(ValueError):
        model.generate(input_ids=ids, num_beams=2, num_return_sequences=3, max_new_tokens=4)
    with pytest.raises((ValueError, NotImplementedError)):
        model.generate(input_ids=ids, num_beams=NB_ROWS + 1, max_new_tokens=4)
    eng = model.engine
    eng.tp_size = 2
    try:
        with pytest.raises(NotImplementedError):
            model.generate(input_ids=ids, num_beams=2, max_new_tokens=4)
    finally:
        eng.tp_size = 1
