"""Prompt-lookup speculative decoding of a SAMPLED sequence on the device (csrc/sampling.hip: spec_sample_kernel in front of csrc/spec.hip:
spec_tail_kernel): row i of a verify step behind w generated ids draws with Philox stream-row word 0 and draw counter w + 1 + i - the
draw that position has in a one-row step - so the ids are a function of (seed, logits) and not of the drafts."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from test_spec_gpu import _expect, _text_prompt
from util import errs, record

pytestmark = pytest.mark.gpu

SEED = 0x0123_4567_89AB_CDEF


def _pars():
    from vz_hip.sample_rows import RowParams
    return [RowParams(True, 0.7, 50, 0.9, SEED, 0), RowParams(True, 1.0, 0, 1.0, SEED + 1, 0), RowParams(True, 0.9, 0, 1.0, SEED + 2, 0, min_p=0.02)]


@pytest.fixture(scope="module")
def B():
    from vz_hip import binding
    binding.load_library()
    return binding


@pytest.fixture(scope="module")
def env():
    """ONE pair of 2-layer synthetic models (bf16 and e4m3 weights) with 8 cache rows for the whole module (tests/test_spec_gpu.py's)."""
    from vz_hip import synth
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    cfg = synth.ArchConfig(n_layers=2)

    def make(fp8):
        hf = VisZephyrConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=cfg.n_layers,
                             num_attention_heads=cfg.n_heads, num_key_value_heads=cfg.n_kv_heads, vocab_size=cfg.vocab,
                             rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta, sliding_window=cfg.sliding_window,
                             eos_token_id=2, pad_token_id=2, bos_token_id=1)
        hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
        hf.mm_patch_merge_type = "flat"
        hf.mm_hidden_size = 5120
        hf.mm_vision_select_layer = "-2,-5,-8,-11,6"
        hf.mm_vision_select_feature = "patch"
        return VisZephyrForCausalLM.from_synthetic(hf, seed=0, max_batch=8, max_ctx=512, max_tiles=4, max_text=64, weight_fp8=fp8)

    return dict(cfg=cfg, synth=synth, bf16=make(False), fp8=make(True))


# ------------------------------------------------------------------------------------------------
# 1: the op - draws and acceptance on constructed logits
# ------------------------------------------------------------------------------------------------
def op_logits(R, cols, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(R, cols, generator=g) * 3.0).float()


def oracle_draw(x, par, counter):
    """(the oracle's token for stream-row word 0 and `counter`, its race margin, the tokens kept with the cut moved a hair inwards or
    None when the record has no cumulative / relative cut): tests/test_sampling_gpu.py's terms; the min_p record goes through
    tests/warpers_ref.py, which puts HF's MinPLogitsWarper behind the oracle's warp."""
    from oracle import sampling_oracle as S
    if par.min_p > 0:
        import warpers_ref as WR
        sc = WR.warp(x, par.temperature, par.top_k, par.top_p, par.min_p)
        s = np.where(np.isneginf(sc), -np.inf, (sc + S.gumbel(sc.shape[0], 0, counter, par.seed)).astype(np.float32))
        two = np.partition(s, -2)[-2:]
        strict = np.isfinite(WR.warp(x, par.temperature, par.top_k, par.top_p, par.min_p * (1.0 + 1e-4)))
        return int(np.argmax(s)), float(two[1] - two[0]), strict
    want, margin = S.draw(x, par.temperature, par.top_k, par.top_p, par.seed, counter, row=0, return_margin=True)
    strict = np.isfinite(S.warp(x, par.temperature, par.top_k, max(1e-6, par.top_p - 1e-5))) if par.top_p < 1.0 else None
    return want, margin, strict


OP_SHAPES = [(R, cols) for cols in (1000, 32000, 40000) for R in (2, 4, 8)]           # 40000 columns: the loop form
OP_WRITES = (0, 5)


def _accept(B, x, par, drafts, *, w=0, budget=100, eos=(), pos0=40, slot0=30, done=0, hist_len=5):
    R = x.shape[0]
    state = torch.zeros(4, R, dtype=torch.int32)
    state[0] = torch.tensor([11] + list(drafts))
    state[1] = pos0 + torch.arange(R)
    state[2] = slot0 + torch.arange(R)
    state[3] = state[2] + 1
    state = state.cuda()
    ctl = torch.zeros(B.SPEC_CTL_WORDS, dtype=torch.int32)
    ctl[B.SPEC_CTL_WRITE], ctl[B.SPEC_CTL_HIST], ctl[B.SPEC_CTL_DONE], ctl[B.SPEC_CTL_DRAFTED] = w, hist_len, done, len(drafts)
    ctl = ctl.cuda()
    out = torch.full((budget + 8,), -7, dtype=torch.int32, device="cuda")
    hist = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    stats = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    B.spec_accept(x, state, ctl, out, budget, hist, eos, stats, max_ctx=4096, rope_max=8192, sample=par)
    return state.cpu(), ctl.cpu().tolist(), out.cpu().tolist(), hist.cpu().tolist(), stats.cpu().tolist()


def _one_row_draws(B, x, par, w):
    return [int(B.sample_rows(x[i:i + 1], [par.at(w + 1 + i)])[0]) for i in range(x.shape[0])]


def test_spec_sample_draws_are_the_one_row_draws(B):
    """the R ids in the control words == vz_op_sample_rows on ONE row at a time with counter WRITE + 1 + i, exactly; and == the numpy
    oracle's draw(row=0, counter=WRITE + 1 + i) but for a race margin < 1e-3 or a token on the boundary of a cut, on at most 2 % of
    the draws (on the CPU the oracle's own margins of these seeds fall below 1e-3 on 1 of the 252 draws, and no drawn token sits on a
    cut's boundary: the cap of 5 leaves room for that one)."""
    checked = excused = 0
    for R, cols in OP_SHAPES:
        x = op_logits(R, cols, seed=cols + R)
        xd = x.cuda()
        for w in OP_WRITES:
            for par in _pars():
                ctl = _accept(B, xd, par, [0] * (R - 1), w=w)[1]
                got = ctl[B.SPEC_CTL_IDS:B.SPEC_CTL_IDS + R]
                assert got == _one_row_draws(B, xd, par, w), (R, cols, w, par)
                for i in range(R):
                    want, margin, strict = oracle_draw(x[i].numpy(), par, w + 1 + i)
                    checked += 1
                    if got[i] != want:
                        assert margin < 1e-3 or (strict is not None and (not strict[got[i]] or not strict[want])), (R, cols, w, i, got[i], want, margin)
                        excused += 1
    record("spec sample op draws", checked=checked, excused=excused)
    assert checked == 252 and excused <= 0.02 * checked, f"{excused} of {checked} draws differ from the oracle"


def test_spec_accept_sampled_cases(B):
    """tests/test_spec_gpu.py::test_spec_accept_cases with the draws in the place of the argmax ids: drafts built from the draws to match
    exactly a = 0..D of them"""
    par = _pars()[0]
    R, cols = 4, 1000
    D = R - 1
    x = op_logits(R, cols, seed=77).cuda()
    g = _one_row_draws(B, x, par, 0)
    assert len(set(g)) == R and cols - 1 not in g, g          # (another seed if this ever fires)
    wrong = lambda t: (t + 1) % cols                          # noqa: E731
    for a in range(D + 1):
        st = _accept(B, x, par, g[:a] + [wrong(t) for t in g[a:D]])
        _expect(*st, emitted=g[:a + 1], drafted=D, R=R)
        assert st[1][B.SPEC_CTL_IDS:B.SPEC_CTL_IDS + R] == g  # the draws do not depend on the drafts
    # a guess that is right AFTER a wrong one does not count
    _expect(*_accept(B, x, par, [g[0], wrong(g[1]), g[2]]), emitted=g[:2], drafted=D, R=R)
    # eos inside the accepted run: emitted, nothing behind it, done; eos as the row's own draw after a wrong guess
    _expect(*_accept(B, x, par, g[:D], eos=[g[1], cols - 1]), emitted=g[:2], drafted=D, R=R, done=1)
    _expect(*_accept(B, x, par, [wrong(g[0]), g[1], g[2]], eos=[g[0]]), emitted=g[:1], drafted=D, R=R, done=1)
    # budget clamp inside the run; the counters follow the write index
    g8, g6 = _one_row_draws(B, x, par, 8), _one_row_draws(B, x, par, 6)
    assert g8 != g and g6 != g
    _expect(*_accept(B, x, par, g8[:D], w=8, budget=10), emitted=g8[:2], w=8, drafted=D, R=R, done=1)
    _expect(*_accept(B, x, par, g6[:D], w=6, budget=10), emitted=g6, w=6, drafted=D, R=R, done=1)
    # R = 2 and R = 8
    x2, x8 = op_logits(2, cols, seed=78).cuda(), op_logits(8, cols, seed=79).cuda()
    g2, g8r = _one_row_draws(B, x2, par, 0), _one_row_draws(B, x8, par, 0)
    _expect(*_accept(B, x2, par, g2[:1]), emitted=g2, drafted=1, R=2)
    assert g8r[4] != 0
    _expect(*_accept(B, x8, par, g8r[:4] + [0] + g8r[5:7]), emitted=g8r[:5], drafted=7, R=8)
    # once done, a step emits nothing and moves nothing
    state, ctl, out, hist, stats = _accept(B, x, par, g[:D], done=1, w=3)
    assert ctl[0] == 3 and ctl[2] == 1 and ctl[4] == 1 and stats == [0, 0, 0] and out[:8] == [-7] * 8
    assert state[1].tolist() == [40, 41, 42, 43] and state[2].tolist() == [30, 31, 32, 33] and int(state[0, 0]) == 11


# ------------------------------------------------------------------------------------------------
# engine-level helpers
# ------------------------------------------------------------------------------------------------
def _spec_run(eng, S, first, history, D, n_new, par, source=0, stream=None, eos=(), chunk=4, logits=True, info=None):
    """sampled verify steps on the prompt already prefilled into cache row 0 (S positions): (ids incl. `first`, per-id logits or None,
    records); `info` collects decode_info() = (context splits, graphs captured) after every call."""
    R = D + 1
    eng.decode_begin(torch.tensor([first] + [0] * D, dtype=torch.int32), [S + i for i in range(R)], [S + i for i in range(R)])
    eng.set_spec(True, D=D, max_ngram=2, history=list(history) + [first], eos=eos, budget=n_new - 1, source=source, stream=stream, sample=par)
    ids, lgs = [first], []
    try:
        while True:
            n0 = len(eng.spec_state()["records"])
            if logits:
                got, lg = eng.decode_steps(chunk, return_logits=True)
            else:
                got, lg = eng.decode_steps(chunk), None
            eng.check_async()
            if info is not None:
                info.append(eng.decode_info())
            st = eng.spec_state()
            if logits:
                for s, r in enumerate(st["records"][n0:]):
                    lgs += [lg[s, j].clone() for j in range(r[2])]
            ids += got.tolist()
            if st["done"]:
                break
        return ids, lgs, [r for r in st["records"] if r[2] > 0]
    finally:
        eng.set_spec(False)


def _first(B, last, par):
    """token 0 of a sampled sequence: one draw on the prefill logits with counter 0"""
    return int(B.sample(last, par.temperature, par.top_k, par.top_p, par.seed, 0, par.warp)[0])


def _replay(B, ids, lgs, par):
    """every emitted id t is the one-row draw on the logits row it was chosen from, counter t, same record - exactly"""
    assert len(lgs) == len(ids) - 1
    for t in range(1, len(ids)):
        assert int(B.sample_rows(lgs[t - 1].view(1, -1), [par.at(t)])[0]) == ids[t], f"id {t} is not the draw of counter {t} on its logits row"


N_NEW = 40


@pytest.fixture(scope="module")
def runs(env, B):
    """per (weights, D): the 60-position prompt prefilled once, then five runs of 40 ids under one record - n-gram drafts, the true
    continuation and always-wrong drafts as eager steps (with logits), the true continuation and n-gram drafts as graph replays"""
    cache = {}

    def get(which, D):
        if (which, D) not in cache:
            eng, V, par = env[which].engine, env["cfg"].vocab, _pars()[0]
            pat = _text_prompt(env, 12, 17).tolist()
            prompt = [1] + pat * 4 + pat[:11]             # 60 positions: + 40 new ids + 7 slots stays inside one 128-key bucket
            S = len(prompt)
            assert S == 60
            _, last = eng.prefill(eng.embed_tokens(torch.tensor([prompt])), [S], all_logits=False, last_logits=True)
            first = _first(B, last, par)
            a = _spec_run(eng, S, first, prompt, D, N_NEW, par, source=0)
            b = _spec_run(eng, S, first, prompt, D, N_NEW, par, source=1, stream=a[0][1:])
            c = _spec_run(eng, S, first, prompt, D, N_NEW, par, source=1, stream=[(t + 1) % V for t in a[0][1:]])
            gb = _spec_run(eng, S, first, prompt, D, N_NEW, par, source=1, stream=a[0][1:], logits=False)
            graph = eng.decode_mode()[0]
            ga = _spec_run(eng, S, first, prompt, D, N_NEW, par, source=0, logits=False)
            cache[(which, D)] = dict(par=par, a=a, b=b, c=c, gb=gb, ga=ga, graph=graph)
        return cache[(which, D)]

    return get


CASES = [("bf16", 3), ("bf16", 7), ("fp8", 3), ("fp8", 7)]


# ------------------------------------------------------------------------------------------------
# 2: the output does not depend on the drafts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,D", CASES)
def test_sampled_output_is_independent_of_the_drafts(runs, which, D):
    r = runs(which, D)
    (ids_a, lg_a, rec_a), (ids_b, lg_b, rec_b), (ids_c, lg_c, rec_c) = r["a"], r["b"], r["c"]
    record(f"spec sample T2 {which} D{D}", steps=[len(rec_a), len(rec_b), len(rec_c)], accepted_ngram=sum(x[1] for x in rec_a))
    assert len(ids_a) == N_NEW and len(lg_a) == N_NEW - 1
    assert ids_b == ids_a, "the true continuation as drafts changes the ids: a row's counter or stream-row word is off"
    assert ids_c == ids_a
    for t in range(N_NEW - 1):
        assert torch.equal(lg_a[t], lg_b[t]) and torch.equal(lg_a[t], lg_c[t]), f"logits of id {t + 1} depend on the drafts"
    assert all(x[1] == D and x[2] == D + 1 for x in rec_b[:-1]) and len(rec_b) == -(-(N_NEW - 1) // (D + 1))
    assert all(x[1] == 0 and x[2] == 1 for x in rec_c) and len(rec_c) == N_NEW - 1
    # graph replay = eager
    assert r["graph"], "the verify steps did not run as a captured graph"
    assert r["gb"][0] == ids_a and r["gb"][2] == rec_b
    assert r["ga"][0] == ids_a and r["ga"][2] == rec_a


# ------------------------------------------------------------------------------------------------
# 3: replay - every id is the one-row draw of its counter on its logits row
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,D", CASES)
def test_sampled_ids_replay_as_one_row_draws(runs, B, which, D):
    r = runs(which, D)
    _replay(B, r["b"][0], r["b"][1], r["par"])


# ------------------------------------------------------------------------------------------------
# 4: the record is part of what a captured step froze
# ------------------------------------------------------------------------------------------------
def test_sampling_record_is_live_in_the_graph(env, B):
    """every buffer is held here and the mode is armed through the C ABI, so nothing but the record differs between two arms: the same
    record replays the captured graph, another temperature or seed captures again and draws by the NEW record"""
    eng, lib, par = env["bf16"].engine, B.lib(), _pars()[0]
    D, budget, W = 3, 16, B.SPEC_CTL_WORDS
    pat = _text_prompt(env, 12, 41).tolist()
    prompt = [1] + pat * 3 + pat[:4]
    S = len(prompt)
    _, last = eng.prefill(eng.embed_tokens(torch.tensor([prompt])), [S], all_logits=False, last_logits=True)
    hist = torch.zeros(S + 1 + budget, dtype=torch.int32, device=eng.device)
    buf = torch.zeros(W + 4 * budget + 1, dtype=torch.int32, device=eng.device)       # control words | out [budget] | stats [budget][3]
    out, stats = buf[W:], buf[W + budget:]

    def run(p):
        first = _first(B, last, p)
        hist.copy_(torch.tensor(prompt + [first] + [0] * budget, dtype=torch.int32))
        eng.decode_begin(torch.tensor([first] + [0] * D, dtype=torch.int32), [S + i for i in range(D + 1)], [S + i for i in range(D + 1)])
        ea = (C.c_int * 4)(0, 0, 0, 0)
        B.check(lib.vz_llm_decode_spec(eng.h, 1, D, 2, B.ptr(hist), S + 1, hist.numel(), ea, 0, B.ptr(out), budget, B.ptr(buf), B.ptr(stats),
                                       budget, 0, None, 0, eng._s()))
        B.check(lib.vz_llm_decode_spec_sampling(eng.h, B.sample_params([p])))
        try:
            B.check(lib.vz_llm_decode_steps(eng.h, budget, B.ptr(out), None, eng._s()))          # a step emits >= 1 id: done within `budget` steps
            eng.check_async()
            host = buf.cpu()
        finally:
            eng.set_spec(False)
        assert eng.decode_mode()[0] and int(host[B.SPEC_CTL_DONE]) == 1
        return [first] + host[W:W + int(host[B.SPEC_CTL_WRITE])].tolist(), eng.decode_info()[1]

    ids1, cap1 = run(par)
    ids2, cap2 = run(par)
    assert len(ids1) == budget + 1 and ids2 == ids1
    assert cap2 == cap1, "a second call with the same record captured a new graph"
    cap = cap2
    for p2 in (dataclasses.replace(par, temperature=1.5), dataclasses.replace(par, seed=SEED + 99)):
        ids_g, cap_g = run(p2)
        assert cap_g == cap + 1, "a changed record replayed the graph captured with the old one"
        cap = cap_g
        ids_e, lg_e, _ = _spec_run(eng, S, ids_g[0], prompt, D, budget + 1, p2, source=0)      # eager steps: the logits rows of the same ids
        assert ids_e == ids_g
        _replay(B, ids_e, lg_e, p2)
        assert ids_g != ids1
    # a NULL record behind the arming: argmax verify again
    first = _first(B, last, par)
    eng.decode_begin(torch.tensor([first] + [0] * D, dtype=torch.int32), [S + i for i in range(D + 1)], [S + i for i in range(D + 1)])
    eng.set_spec(True, D=D, history=prompt + [first], budget=4, source=0, sample=par)
    try:
        B.check(lib.vz_llm_decode_spec_sampling(eng.h, None))
        got, lg = eng.decode_steps(1, return_logits=True)
        assert int(got[0]) == int(lg[0, 0].argmax())
    finally:
        eng.set_spec(False)


# ------------------------------------------------------------------------------------------------
# 5: a context-bucket crossing with the mode on
# ------------------------------------------------------------------------------------------------
def test_sampled_bucket_crossing_eager_equals_graph(env, B):
    """the 60 + 64 case of tests/test_spec_gpu.py::test_generate_prompt_lookup_edges: the graph is captured again in the middle and the
    steps behind it merge two splits"""
    eng, par = env["bf16"].engine, _pars()[0]
    pat = _text_prompt(env, 24, 29).tolist()
    long_ids = [1] + (pat * 3)[:59]
    S = len(long_ids)
    _, last = eng.prefill(eng.embed_tokens(torch.tensor([long_ids])), [S], all_logits=False, last_logits=True)
    first = _first(B, last, par)
    info_e, info_g = [], []
    ids_e, lg_e, rec_e = _spec_run(eng, S, first, long_ids, 7, 64, par, source=0, logits=True, info=info_e)
    ids_g, _, rec_g = _spec_run(eng, S, first, long_ids, 7, 64, par, source=0, logits=False, info=info_g)
    assert eng.decode_mode()[0]
    assert len(ids_e) == 64 and ids_g == ids_e and rec_g == rec_e
    for info in (info_e, info_g):
        assert sorted(set(ns for ns, _ in info)) == [1, 2], info
    _replay(B, ids_e, lg_e, par)


# ------------------------------------------------------------------------------------------------
# 6: generate(do_sample=True, prompt_lookup_num_tokens=...)
# ------------------------------------------------------------------------------------------------
def _equal_or_near_tie(name, model, B, emb, history, kw, plain, got, D, par):
    """all ids equal, or at the FIRST differing index j the race on the plain call's own logits row j (counter j) is a near-tie: its
    margin is below 4 x the two routes' relative-L2 difference on that row x the row's rms (the tolerance of
    tests/test_spec_gpu.py::test_generate_with_prompt_lookup_matches_plain_greedy) / T - the race runs on logits / T"""
    from oracle import sampling_oracle as S
    f = next((t for t in range(min(len(plain), len(got))) if plain[t] != got[t]), -1)
    if f < 0:
        assert len(plain) == len(got)
        record(name, diverged=-1)
        return
    assert f > 0, "the first id is one draw on the same prefill logits"
    out = model.generate(return_dict_in_generate=True, output_logits=True, **kw)
    assert out.sequences[0].tolist() == plain
    p = out.logits[f][0].float().cpu()
    _, margin = S.draw(p.numpy(), par.temperature, par.top_k, par.top_p, par.seed, f, return_margin=True)
    eng, n = model.engine, emb.shape[1]
    eng.prefill(emb, [n], all_logits=False, last_logits=True)
    ids_f, lgs, _ = _spec_run(eng, n, plain[0], history, D, f + 1, par, source=1, stream=plain[1:])
    assert ids_f == got[:f + 1], "generate() and the forced verify steps disagree on the same prefix"
    q = lgs[f - 1].float().cpu()
    e = errs(q, p)[1]
    tol = 4.0 * e * float(p.double().pow(2).mean().sqrt()) / par.temperature
    record(name, diverged=f, margin=margin, tolerance=tol, step_rel_l2=e)
    assert margin < tol, f"{name}: id {f}: {got[f]} vs plain {plain[f]}: race margin {margin:.3e} exceeds 4 x error x rms / T = {tol:.3e}"


def _always_wrong(env, B, eng, emb, history, D, n_new, par):
    n = emb.shape[1]
    _, last = eng.prefill(emb, [n], all_logits=False, last_logits=True)
    first = _first(B, last, par)
    # (the drafts must be wrong whatever is drawn: a stream cannot know the ids in advance, so it is built from a first run)
    ids, _, _ = _spec_run(eng, n, first, history, D, n_new, par, source=0, logits=False)
    V = env["cfg"].vocab
    ids_w, _, rec_w = _spec_run(eng, n, first, history, D, n_new, par, source=1, stream=[(t + 1) % V for t in ids[1:]], logits=False)
    assert all(x[1] == 0 for x in rec_w)
    return ids_w


def test_generate_sampled_with_prompt_lookup(env, B):
    from vz_hip.sample_rows import RowParams
    model, cfg, S_ = env["bf16"], env["cfg"], env["synth"]
    seed = 4242
    par = RowParams(True, 0.7, 0, 1.0, seed, 0)               # top-k and top-p off: no kept-set boundary can flip between the two routes
    pat = _text_prompt(env, 24, 23).tolist()
    ids = torch.tensor([[1] + pat * 3 + pat[:7]])
    kw = dict(input_ids=ids, do_sample=True, seed=seed, temperature=0.7, top_k=0, top_p=1.0, max_new_tokens=40, eos_token_id=None, pad_token_id=2)
    plain = model.generate(**kw)[0].tolist()
    t = {}
    got = model.generate(prompt_lookup_num_tokens=7, timing=t, **kw)[0].tolist()
    assert t["spec"]["used"] is True and t["spec"]["sampled"] is True and t["spec"]["D"] == 7 and t["spec"]["tokens"] == len(got) == 40
    record("spec sample T6 text", **t["spec"])
    emb = model.engine.embed_tokens(ids)
    assert got == _always_wrong(env, B, model.engine, emb, ids[0].tolist(), 7, 40, par)
    _equal_or_near_tie("spec sample T6 text near-tie", model, B, emb, ids[0].tolist(), kw, plain, got, 7, par)
    # multimodal: the history carries -1 where the 96 visual tokens sit
    tiles = S_.synth_tiles(3, seed=1)
    mm = S_.synth_ids(32, cfg.vocab, image_pos=5, seed=2)
    mm[20:32] = mm[6:18]                                     # some text that repeats
    mm = mm.unsqueeze(0)
    kw = dict(input_ids=mm, images=[tiles], do_sample=True, seed=seed, temperature=0.7, top_k=0, top_p=1.0, max_new_tokens=24, eos_token_id=None,
              pad_token_id=2)
    plain = model.generate(**kw)[0].tolist()
    t = {}
    got = model.generate(prompt_lookup_num_tokens=7, timing=t, **kw)[0].tolist()
    assert t["spec"]["used"] is True and t["spec"]["sampled"] is True and len(got) == 24
    emb = model.prepare_inputs_labels_for_multimodal(mm, None, None, None, None, [tiles])[4]
    hist = model._spec_history(mm, None, [tiles], emb.shape[1])
    assert len(hist) == 31 + 96 and hist[5:101] == [-1] * 96
    assert got == _always_wrong(env, B, model.engine, emb, hist, 7, 24, par)
    _equal_or_near_tie("spec sample T6 multimodal near-tie", model, B, emb, hist, kw, plain, got, 7, par)


# ------------------------------------------------------------------------------------------------
# 7: calls the mode does not cover run what they ran
# ------------------------------------------------------------------------------------------------
class _Streamer:
    def put(self, v):
        pass

    def end(self):
        pass


def test_uncovered_sampled_calls_keep_their_route(env):
    model = env["bf16"]
    pat = _text_prompt(env, 24, 29).tolist()
    ids = torch.tensor([[1] + pat * 2 + pat[:9]])
    base = dict(input_ids=ids, do_sample=True, seed=77, temperature=0.7, top_k=50, top_p=0.9, max_new_tokens=10, eos_token_id=None, pad_token_id=2)
    cases = {
        "a processor keyword": lambda: dict(repetition_penalty=1.3),
        "a streamer": lambda: dict(streamer=_Streamer()),
        "stopping_criteria": lambda: dict(stopping_criteria=[lambda i, s, **k: False]),
        "two sequences": lambda: dict(input_ids=torch.cat([ids, ids])),
        "num_return_sequences": lambda: dict(num_return_sequences=2),
        "output_scores": lambda: dict(return_dict_in_generate=True, output_scores=True),
    }
    for name, more in cases.items():
        want = model.generate(**{**base, **more()})
        t = {}
        got = model.generate(prompt_lookup_num_tokens=7, timing=t, **{**base, **more()})
        assert "spec" not in t, name
        if name == "output_scores":
            want, got = want.sequences, got.sequences
        assert torch.equal(got, want), name
    t = {}
    model.generate(prompt_lookup_num_tokens=7, timing=t, **base)
    assert t["spec"]["used"] and t["spec"]["sampled"]           # (the same call with none of them does take the mode)
