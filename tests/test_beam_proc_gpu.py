"""Beam search with logits processors, per-step scores and beam_indices on the MI355X (csrc/beam.hip, csrc/logits_proc.hip,
vz_hip/beam.py, VisZephyrForCausalLM.generate(num_beams > 1, <processor keywords>, output_scores=, output_logits=)).

1. the log-prob rows op against fp64 log_softmax; log-prob rows + select-on-rows == the fused select, bit for bit;
2. log-prob rows -> processors -> select-on-rows against HF's processor objects on the device's own rows + `select_reference`;
3. the history reorder against a torch gather (a cycle, one parent with several children, the identity; rows outside untouched);
4. generate() against a host-driven loop (eager steps, torch log_softmax, HF's processors on each beam's replayed ids, the torch
   selection, kv_move_rows, the same replay) - text and multimodal, every processor biting;
5. the captured step == the eager step, sync_every 1 == 8, a processor parameter is part of the graph key;
6. 5 prompts x 4 beams on 16 cache rows (chunks of 4 and 1 prompts), num_return_sequences=2, zeros behind a prompt's end;
7. with no processors and no outputs asked the beam step is the fused step: same ids and score bits, no extra capture.
"""
import os

import pytest
import torch

from beam_proc_util import BITERS, hf_chain, process, step
from util import record

pytestmark = pytest.mark.gpu

NB_ROWS = 16
EOS = 2
BIAS_TOKEN, BIAS_NEXT = 1234, 4321
PENALTY = 1.3


@pytest.fixture(scope="module")
def env():
    from vz_hip import synth
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    cfg = synth.ArchConfig(n_layers=2)
    hf = VisZephyrConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=cfg.n_layers,
                         num_attention_heads=cfg.n_heads, num_key_value_heads=cfg.n_kv_heads, vocab_size=cfg.vocab,
                         rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta, sliding_window=cfg.sliding_window,
                         eos_token_id=EOS, pad_token_id=EOS, bos_token_id=1)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    model = VisZephyrForCausalLM.from_synthetic(hf, seed=0, max_batch=NB_ROWS, max_ctx=256, max_tiles=1, max_text=64)
    torch.cuda.synchronize()
    return dict(cfg=cfg, model=model, synth=synth)


def _with_inf(logits):
    if logits.shape[0] >= 8:
        logits[0, logits.shape[1] // 2:] = -float("inf")          # half a row
        logits[3, ::3] = -float("inf")                            # every third entry
    else:
        logits[0, ::3] = -float("inf")
    return logits.contiguous()


# ---- 1. log-prob rows; select-on-rows == the fused select ----------------------------------------------------------------------
@pytest.mark.parametrize("V", [32000, 32002, 1000])
@pytest.mark.parametrize("rows", [1, 8, 16])
def test_logprob_rows_match_fp64_and_select_on_rows_is_the_fused_select(V, rows):
    from vz_hip import binding as B
    g = torch.Generator(device="cuda").manual_seed(V + rows)
    logits = _with_inf(torch.randn(rows, V, device="cuda", generator=g) * 3.0)
    lp = B.beam_logprob_rows(logits)
    ref = torch.log_softmax(logits.double(), -1)
    fin = torch.isfinite(ref)
    assert bool((lp[~fin] == -float("inf")).all()) and bool(torch.isfinite(lp[fin]).all())
    rel = float(((lp.double()[fin] - ref[fin]).abs() / ref[fin].abs().clamp_min(1e-30)).max())
    record("beam_logprob_rows", V=V, rows=rows, rel=rel)
    assert rel <= 2e-6, f"log-prob rows rel err {rel:.3e}"
    inplace = logits.clone()
    assert B.beam_logprob_rows(inplace, out=inplace) is inplace and torch.equal(inplace.view(torch.int32), lp.view(torch.int32))
    scores = -torch.rand(rows, device="cuda", generator=g) * 20.0
    first = torch.topk(logits[0], 3)[1].tolist()
    for nb in (2, 4, 16):
        for eos in ([], [first[0], first[2]]):
            cases = [(logits[:1].contiguous(), lp[:1].contiguous(), None, 1)]          # the first step: nb_in = 1
            if rows % nb == 0:
                cases.append((logits, lp, scores, nb))
            for lg, rw, sc, nb_in in cases:
                fused = B.beam_select(lg, sc, nb_in, nb, eos)
                split = B.beam_select(rw, sc, nb_in, nb, eos, on_rows=True)
                for a, b, what in zip(fused, split, ("records", "next tokens", "next scores", "next parents")):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"V{V} rows{rows} nb{nb} nb_in{nb_in} eos{eos}: {what} differ"


# ---- 2. log-prob rows -> processors -> select-on-rows -------------------------------------------------------------------------
def _select_rows_check(rows, scores, nb_in, nb_out, eos, got, name):
    """the device's candidates `got` = (records, next tokens, scores, parents) against the fp64 order of rows + scores: identical except
    where the fp64 gap to a neighbour is under 1e-5 (tests/test_beam_gpu.py's rule); returns the near ties"""
    from vz_hip import beam as BM
    s, t, p = BM.decode_records(got[0])
    n, V = rows.shape
    G, K = n // nb_in, BM.beam_k(nb_out, len(eos))
    flat = (rows.double() + (0 if scores is None else scores.double()[:, None])).reshape(G, nb_in * V).cpu()
    vals, idx = torch.sort(flat, dim=1, descending=True, stable=True)
    near = 0
    for g in range(G):
        ref_t, ref_p = idx[g, :K] % V, idx[g, :K] // V
        for i in torch.nonzero((ref_t != t[g]) | (ref_p != p[g])).view(-1).tolist():
            gap = min(float(vals[g, i] - vals[g, i + 1]), float(vals[g, i - 1] - vals[g, i]) if i > 0 else float("inf"))
            assert gap < 1e-5, f"{name}: group {g} candidate {i}: {t[g, i].item()}/{p[g, i].item()} vs {ref_t[i].item()}/{ref_p[i].item()} (gap {gap:.3e})"
            near += 1
        keep = [i for i in range(K) if int(t[g, i]) not in eos][:nb_out]
        assert got[1].view(G, nb_out)[g].cpu().tolist() == [int(t[g, i]) for i in keep]
        assert got[3].view(G, nb_out)[g].cpu().tolist() == [int(p[g, i]) for i in keep]
    return near


def test_processed_selection_matches_hf_processors():
    from vz_hip import binding as B
    from vz_hip import logits_proc as LP
    V, nb, G, stride = 32000, 4, 2, 64
    R = nb * G
    g = torch.Generator(device="cuda").manual_seed(77)
    logits = _with_inf(torch.randn(R, V, device="cuda", generator=g) * 3.0)
    scores = -torch.rand(R, device="cuda", generator=g) * 20.0
    lens = [0, 1, 7, stride, 7, stride, 1, 0]
    hist = torch.randint(10, 40, (R, stride), device="cuda", generator=g, dtype=torch.int32)       # a small alphabet: n-grams repeat
    hist_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    eos = [EOS, 11]
    kw = dict(sequence_bias={(12,): 4.0, (int(hist[2, 6]), 13): -3.0, (int(hist[3, stride - 1]), 14): 2.5}, repetition_penalty=PENALTY,
              no_repeat_ngram_size=2, bad_words_ids=[[15], [int(hist[4, 5]), int(hist[4, 6]), 16]], min_new_tokens=3, suppress_tokens=[17, 18])
    cfg = LP.parse(kw["repetition_penalty"], kw["no_repeat_ngram_size"], kw["min_new_tokens"], kw["suppress_tokens"], eos,
                   kw["sequence_bias"], kw["bad_words_ids"], V)
    lp = B.beam_logprob_rows(logits)
    rows = B.logits_process(lp.clone(), cfg, hist, hist_len)
    chain = hf_chain(kw, eos, "cuda")
    want = torch.cat([process(chain, [hist[r, :lens[r]].tolist()], lp[r:r + 1]) for r in range(R)], 0)
    assert torch.equal(rows.view(torch.int32), want.view(torch.int32)), "the processed rows are not HF's, bit for bit"
    changed = (rows.view(torch.int32) != lp.view(torch.int32)).sum(1).tolist()
    assert all(c >= 3 for c in changed), f"processors that change nothing prove nothing: {changed}"
    near = _select_rows_check(rows, scores, nb, nb, eos, B.beam_select(rows, scores, nb, nb, eos, on_rows=True), "processed")
    near += _select_rows_check(rows[:G].contiguous(), None, 1, nb, eos, B.beam_select(rows[:G].contiguous(), None, 1, nb, eos, on_rows=True), "processed first")
    record("beam_proc_select", near_ties=near, changed=changed)


# ---- 3. the history reorder ---------------------------------------------------------------------------------------------------
def test_hist_beam_reorder_is_a_gather():
    from vz_hip import binding as B
    nb, G, stride = 4, 3, 1100                                   # (one history longer than the kernel's 512-id piece)
    g = torch.Generator().manual_seed(9)
    hist = torch.randint(0, 32000, (NB_ROWS, stride), generator=g, dtype=torch.int32).cuda()
    lens = torch.tensor([5, 1030, 0, 17, 3, 9, 40, 1, 6, 2, 8, 4, 11, 12, 13, 14], dtype=torch.int32).cuda()
    parents = [[1, 2, 3, 0],          # a 4-cycle
               [2, 2, 2, 1],          # one parent with three children
               [0, 1, 2, 3]]          # identity
    before, before_len = hist.clone(), lens.clone()
    B.hist_beam_reorder(lens, hist, nb, G, torch.tensor(sum(parents, []), dtype=torch.int32).cuda())
    for grp in range(G):
        for j in range(nb):
            src = grp * nb + parents[grp][j]
            n = int(before_len[src])
            assert int(lens[grp * nb + j]) == n
            assert torch.equal(hist[grp * nb + j, :n], before[src, :n]), f"group {grp} row {j}"
    assert torch.equal(hist[8:], before[8:]) and torch.equal(lens[8:], before_len[8:])          # the identity group and the rows outside


# ---- 4. end to end against a host-driven loop ------------------------------------------------------------------------------------
def _host_beam(model, emb, nb, eos, max_new, kw, bites=None):
    """the same beam search driven from the host.  Returns (replay, smallest fp32 gap met at a selection, the processed rows of every
    step [nb, V])."""
    from vz_hip import beam as BM
    eng = model.engine
    S, R = emb.shape[1], nb
    park = lambda: eng.decode_begin(torch.zeros(R, dtype=torch.int32), [0] * R, [0] * R)   # noqa: E731
    park()
    last = eng.prefill_rows(0, emb, [S])
    rep = BM.BeamReplay(nb, eos, max_new, 1.0, False)
    min_gap, all_rows = [float("inf")], []

    def select(lg, ids, sc, nb_in):
        rows, cs, ct, cp, nt, ns, npar = step(kw, eos, ids, torch.log_softmax(lg.float(), -1), sc, nb_in, nb, bites)
        tot = rows + (0 if sc is None else sc[:, None])
        top = torch.sort(tot.reshape(-1), descending=True)[0][:cs.numel() + 1]
        min_gap[0] = min(min_gap[0], float((top[:-1] - top[1:]).min()))
        all_rows.append(rows.expand(nb, -1).clone())
        rep.step(cs.cpu(), ct.cpu(), cp.cpu())
        return nt, ns, npar

    nt, ns, npar = select(last, [[]], None, 1)
    if not rep.done:
        eng.kv_move_rows([0] * (R - 1), list(range(1, R)), [S] * (R - 1))
    L = S
    while not rep.done:
        eng.decode_begin(nt.to(torch.int32), [L] * R, [L] * R)
        _, lg = eng.decode_steps(1, return_logits=True)
        L += 1
        nt, ns, npar = select(lg[0], rep.running, ns, nb)
        if rep.done:
            break
        park()
        ch = [j for j in range(R) if int(npar[j]) != j]
        if ch:
            eng.kv_move_rows([int(npar[j]) for j in ch], [R + i for i in range(len(ch))], [L] * len(ch))
            eng.kv_move_rows([R + i for i in range(len(ch))], ch, [L] * len(ch))
    return rep, min_gap[0], all_rows


def _rows_close(a, b, tol=1e-4):
    fin = torch.isfinite(b)
    return bool((torch.isfinite(a) == fin).all()) and bool(((a[fin] - b[fin]).abs() <= tol).all()) and bool((a[~fin] == b[~fin]).all())


def _e2e(name, model, gen_kw, emb, nb, max_new):
    """generate() with the biases alone, then with every processor, against the host-driven loop.  The biases make the processors
    bite: the bias on T outweighs the model (T repeats), the bias on X behind T is a little smaller, so X follows T only once the
    penalty has shrunk T's score; the bad word = two adjacent ids of the bias run's best hypothesis (T, T); and the n-gram ban meets
    the pair (T, X) a second time."""
    from vz_hip import beam as BM
    bias = {(BIAS_TOKEN,): 40.0, (BIAS_TOKEN, BIAS_NEXT): 36.0}
    run = lambda **kw: model.generate(num_beams=nb, max_new_tokens=max_new, return_dict_in_generate=True, output_scores=True, beam_extended=True,
                                      **gen_kw, **kw)   # noqa: E731
    plain = run(sequence_bias=bias)
    best = plain.sequences[0].tolist()
    assert best.count(BIAS_TOKEN) >= 2, f"{name}: the bias does not make the model repeat its token: {best}"
    i = best.index(BIAS_TOKEN)
    kw = dict(sequence_bias=bias, repetition_penalty=PENALTY, no_repeat_ngram_size=2, bad_words_ids=[best[i:i + 2]], min_new_tokens=3)
    got = run(**kw)
    bites = {}
    rep, gap, rows = _host_beam(model, emb, nb, [EOS], max_new, kw, bites)
    record("beam_proc_e2e", case=name, gap=gap, bites=bites, steps=len(rows), best=rep.best(1)[0][0], bias_run=best, got=got.sequences[0].tolist())
    assert set(bites) == set(BITERS) and all(v >= 1 for v in bites.values()), f"{name}: a processor never changed a candidate: {bites}"
    toks, sc = rep.best(1)[0]
    row = got.sequences[0].tolist()
    want = toks + [BM.fill_value(EOS, [EOS])] * (len(row) - len(toks))
    if row != want or len(got.scores) != len(rows):
        assert gap < 1e-4, f"{name}: {row} vs host {want} (smallest selection gap {gap:.3e})"
        record("beam_proc_e2e_near_tie", case=name, gap=gap)
        return
    assert abs(float(got.sequences_scores[0]) - sc) <= 1e-4
    assert got.beam_indices.tolist() == BM.flat_beam_indices([rep.best_indices(1)], nb).tolist()
    assert tuple(got.scores[0].shape) == (nb, model.config.vocab_size)
    bad = [t for t in range(len(rows)) if not _rows_close(got.scores[t], rows[t])]
    assert not bad or gap < 1e-4, f"{name}: scores rows of steps {bad} are not the host loop's (smallest selection gap {gap:.3e})"
    tr = model.compute_transition_scores(got.sequences, got.scores, got.beam_indices)
    n = len(toks)
    assert abs(float(tr[0, :n].sum()) - sc * n) <= 1e-3 * n, "the transition scores do not add up to the hypothesis' score"


def test_generate_matches_host_driven_loop_text(env):
    model, cfg, S = env["model"], env["cfg"], env["synth"]
    ids = S.synth_ids(24, cfg.vocab, image_pos=-1, seed=11).unsqueeze(0)
    _e2e("text", model, dict(input_ids=ids), model.engine.embed_tokens(ids.cuda()), 4, 20)


def test_generate_matches_host_driven_loop_multimodal(env):
    model, cfg, S = env["model"], env["cfg"], env["synth"]
    tiles = S.synth_tiles(1, seed=1)
    ids = S.synth_ids(16, cfg.vocab, image_pos=3, seed=2).unsqueeze(0)
    emb = model.prepare_inputs_labels_for_multimodal(ids.cuda(), None, None, None, None, [tiles], None)[4]
    _e2e("multimodal", model, dict(input_ids=ids, images=[tiles]), emb, 4, 20)


# ---- 5. graph == eager; the graph key ----------------------------------------------------------------------------------------------
def _same(a, b):
    assert a.sequences.tolist() == b.sequences.tolist()
    assert torch.equal(a.sequences_scores.view(torch.int32), b.sequences_scores.view(torch.int32))
    assert a.beam_indices.tolist() == b.beam_indices.tolist()
    assert len(a.scores) == len(b.scores) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a.scores, b.scores))
    assert len(a.logits) == len(b.logits) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a.logits, b.logits))


def test_graph_equals_eager_and_parameters_are_part_of_the_graph_key(env):
    model, cfg, S = env["model"], env["cfg"], env["synth"]
    eng = model.engine
    ids = S.synth_ids(20, cfg.vocab, image_pos=-1, seed=4).unsqueeze(0)
    kw = dict(input_ids=ids, num_beams=4, max_new_tokens=20, return_dict_in_generate=True, output_scores=True, output_logits=True, beam_extended=True,
              sequence_bias={(BIAS_TOKEN,): 14.0}, no_repeat_ngram_size=2, min_new_tokens=2)
    graph = model.generate(sync_every=8, repetition_penalty=PENALTY, **kw)
    assert eng.decode_mode()[0]
    c0 = eng.decode_info()[1]
    _same(graph, model.generate(sync_every=1, repetition_penalty=PENALTY, **kw))
    os.environ["VZ_NO_GRAPH"] = "1"
    try:
        eager = model.generate(sync_every=8, repetition_penalty=PENALTY, **kw)
    finally:
        del os.environ["VZ_NO_GRAPH"]
    _same(graph, eager)
    c1 = eng.decode_info()[1]
    other = model.generate(sync_every=8, repetition_penalty=1.9, **kw)
    assert eng.decode_info()[1] > c1 >= c0, "another penalty must capture the step again"
    assert any(not torch.equal(x, y) for x, y in zip(graph.scores, other.scores)), "another penalty must change the processed rows"


# ---- 6. batches in chunks ----------------------------------------------------------------------------------------------------------
def _min_gap(out, nb, eos, max_new):
    """the smallest gap between neighbours among the K + 1 best candidates at any step of a one-prompt run, from its own score rows"""
    from vz_hip import beam as BM
    rep, gap = BM.BeamReplay(nb, eos, max_new, 1.0, False), float("inf")
    for t, rows in enumerate(out.scores):
        rows, sc, nb_in = (rows[:1], None, 1) if t == 0 else (rows, rep.running_scores.to(rows.device), nb)
        cs, ct, cp, *_ = BM.select_reference(rows, sc, nb_in, nb, eos, on_rows=True)
        tot = (rows + (0 if sc is None else sc[:, None])).reshape(-1)
        top = torch.sort(tot, descending=True)[0][:cs.shape[1] + 1]
        gap = min(gap, float((top[:-1] - top[1:]).min()))
        rep.step(cs[0].cpu(), ct[0].cpu(), cp[0].cpu())
    return gap


def test_batches_in_chunks_global_rows_and_zeros_behind_a_prompts_end(env):
    from vz_hip import binding as B
    model, cfg, S = env["model"], env["cfg"], env["synth"]
    nb, nrs, max_new = 4, 2, 14
    lens = [22, 15, 19, 12, 17]
    prompts = [S.synth_ids(n, cfg.vocab, image_pos=-1, seed=60 + i) for i, n in enumerate(lens)]
    n = max(lens)
    ids, mask = torch.full((5, n), EOS, dtype=torch.long), torch.zeros(5, n, dtype=torch.long)
    for r, x in enumerate(prompts):          # left padding + mask, as a tokenizer with padding_side="left" gives it
        ids[r, n - len(x):] = x
        mask[r, n - len(x):] = 1
    # a bias on the eos id ends hypotheses early, min_new_tokens holds it back for the first steps; how early depends on the prompt: the
    # bias lifts the eos id (log-prob about -11 in this model) to just above the model's best tokens (about -6), not far beyond them
    kw = dict(num_beams=nb, num_return_sequences=nrs, max_new_tokens=max_new, return_dict_in_generate=True, output_scores=True, beam_extended=True,
              output_logits=True, sequence_bias={(EOS,): 5.0}, min_new_tokens=3, repetition_penalty=PENALTY, sync_every=4)
    with B.tuned(splitk_mid=0):          # one kernel route for every row count (tests/test_beam_gpu.py::test_beam_batches_and_returns)
        batch = model.generate(input_ids=ids, attention_mask=mask, **kw)
        singles = [model.generate(input_ids=p.unsqueeze(0), **kw) for p in prompts]
    steps = [len(s.scores) for s in singles]
    record("beam_proc_batch", steps=steps, lens=[int((s.beam_indices[0] >= 0).sum()) for s in singles])
    assert len(set(steps)) > 1, f"the searches all took the same number of steps, the zeros rule is not exercised: {steps}"
    assert len(batch.scores) == len(batch.logits) == max(steps) and tuple(batch.scores[0].shape) == (5 * nb, cfg.vocab)
    assert batch.sequences.shape[0] == 5 * nrs == batch.beam_indices.shape[0]
    assert any(int(s.sequences[0, 0]) != EOS and EOS in s.sequences[0].tolist()[3:] for s in singles), "no eos id ended a best hypothesis behind min_new_tokens"
    assert all(EOS not in s.sequences[0].tolist()[:3] for s in singles), "min_new_tokens did not hold the eos id back"
    for b, one in enumerate(singles):
        gap = _min_gap(one, nb, [EOS], max_new)
        w = one.sequences.shape[1]
        same = batch.sequences[b * nrs:(b + 1) * nrs, :w].tolist() == one.sequences.tolist() and \
            bool((batch.sequences[b * nrs:(b + 1) * nrs, w:] == EOS).all())
        if not same:
            assert gap < 1e-4, f"prompt {b}: {batch.sequences[b * nrs:(b + 1) * nrs].tolist()} vs alone {one.sequences.tolist()} (gap {gap:.3e})"
            record("beam_proc_batch_near_tie", prompt=b, gap=gap)
            continue
        assert torch.allclose(batch.sequences_scores[b * nrs:(b + 1) * nrs], one.sequences_scores, rtol=0, atol=1e-4)
        idx = batch.beam_indices[b * nrs:(b + 1) * nrs, :w]
        assert torch.equal(idx, torch.where(one.beam_indices >= 0, one.beam_indices + b * nb, one.beam_indices)), f"prompt {b}: beam_indices are not global rows"
        assert bool((batch.beam_indices[b * nrs:(b + 1) * nrs, w:] == -1).all())
        for t in range(len(batch.scores)):
            for full, alone in ((batch.scores, one.scores), (batch.logits, one.logits)):
                mine = full[t][b * nb:(b + 1) * nb]
                if t < steps[b]:
                    assert _rows_close(mine, alone[t]) or gap < 1e-4, f"prompt {b} step {t}: rows differ from the prompt's own run"
                else:
                    assert not bool(mine.any()), f"prompt {b} step {t}: rows behind the prompt's end are not zeros"


# ---- 7. nothing changed when nothing is asked ------------------------------------------------------------------------------------
def test_plain_beam_step_is_the_fused_step(env):
    """generate(num_beams=4) == a host-driven loop through the op-level fused select on eager logits, bit for bit; an armed call in
    between leaves nothing behind: the plain call after it captures the plain step and gives the same bits."""
    from vz_hip import beam as BM
    from vz_hip import binding as B
    model, cfg, S = env["model"], env["cfg"], env["synth"]
    eng = model.engine
    nb, max_new = 4, 16
    ids = S.synth_ids(21, cfg.vocab, image_pos=-1, seed=8).unsqueeze(0)
    kw = dict(input_ids=ids, num_beams=nb, max_new_tokens=max_new, return_dict_in_generate=True)
    plain = model.generate(**kw)
    c0 = eng.decode_info()[1]
    again = model.generate(**kw)
    c1 = eng.decode_info()[1]
    armed = model.generate(repetition_penalty=PENALTY, output_scores=True, beam_extended=True, **kw)
    assert armed.scores is not None and plain.scores is None and plain.logits is None
    c2 = eng.decode_info()[1]
    after = model.generate(**kw)
    # 15 steps in one chunk: a call captures its step at most once (its history buffer is part of the key), armed call in between or not
    assert c1 - c0 <= 1 and eng.decode_info()[1] - c2 <= 1, "a plain beam call captured more than its one step"
    for x in (again, after):
        assert x.sequences.tolist() == plain.sequences.tolist()
        assert torch.equal(x.sequences_scores.view(torch.int32), plain.sequences_scores.view(torch.int32))
    # the op-level fused path on eager steps
    emb = eng.embed_tokens(ids.cuda())
    S0, R = emb.shape[1], nb
    park = lambda: eng.decode_begin(torch.zeros(R, dtype=torch.int32), [0] * R, [0] * R)   # noqa: E731
    park()
    rep = BM.BeamReplay(nb, [EOS], max_new, 1.0, False)
    rec, nt, ns, npar = B.beam_select(eng.prefill_rows(0, emb, [S0]), None, 1, nb, [EOS])
    rep.step(*[x[0] for x in BM.decode_records(rec)])
    eng.kv_move_rows([0] * (R - 1), list(range(1, R)), [S0] * (R - 1))
    L = S0
    while not rep.done:
        eng.decode_begin(nt, [L] * R, [L] * R)
        _, lg = eng.decode_steps(1, return_logits=True)
        L += 1
        rec, nt, ns, npar = B.beam_select(lg[0].contiguous(), ns, nb, nb, [EOS])
        rep.step(*[x[0] for x in BM.decode_records(rec)])
        if rep.done:
            break
        park()
        eng.kv_beam_reorder(nb, 1, [S0], [L], npar)
    toks, sc = rep.best(1)[0]
    assert plain.sequences[0].tolist()[:len(toks)] == toks
    assert float(plain.sequences_scores[0]) == float(torch.tensor(sc, dtype=torch.float32))
    assert plain.beam_indices.tolist() == BM.flat_beam_indices([rep.best_indices(1)], nb).tolist()


def test_the_guards_that_remain(env):
    model, cfg, S = env["model"], env["cfg"], env["synth"]
    ids = S.synth_ids(12, cfg.vocab, image_pos=-1, seed=41).unsqueeze(0)
    kw = dict(input_ids=ids, num_beams=2, max_new_tokens=4)
    with pytest.raises(NotImplementedError, match="output_logprobs"):
        model.generate(return_dict_in_generate=True, output_logprobs=True, beam_extended=True, **kw)
    with pytest.raises(NotImplementedError, match="beam sampling"):
        model.generate(do_sample=True, repetition_penalty=1.2, beam_extended=True, **kw)
    with pytest.raises(NotImplementedError, match="stopping_criteria"):
        model.generate(stopping_criteria=[lambda *a: False], no_repeat_ngram_size=2, beam_extended=True, **kw)
    # the surface is opt-in: without the flag the earlier refusals stand, and the flag alone changes nothing
    with pytest.raises(NotImplementedError, match="beam_extended"):
        model.generate(repetition_penalty=1.2, **kw)
    with pytest.raises(NotImplementedError, match="beam_extended"):
        model.generate(return_dict_in_generate=True, output_scores=True, **kw)
    assert model.generate(beam_extended=True, **kw).tolist() == model.generate(**kw).tolist()
    # the engine refuses the processors together with the speculative tail only; the row recorder refuses more steps than its rings hold
    from vz_hip import binding as B
    eng = model.engine
    with pytest.raises(ValueError):
        B.check(eng.lib.vz_llm_decode_beam_rows(eng.h, B.ptr(torch.empty(4, device="cuda")), None, 0))
    B.check(eng.lib.vz_llm_decode_beam_rows(eng.h, None, None, 0))
