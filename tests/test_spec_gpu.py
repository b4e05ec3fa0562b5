"""Prompt-lookup speculative decoding on the device (csrc/spec.hip): the draft and accept kernels against the Python rule, the verify
attention against the fp64 reference, verify steps against the prefill under teacher forcing, independence of the output from the
drafts, and `generate(prompt_lookup_num_tokens=...)` against plain greedy `generate`."""
import random

import pytest
import torch

from test_ops_gpu import BF16_L2, BF16_MAX, _rand, _ref_attention
from test_spec_cpu import random_cases
from util import check_close, errs, record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from vz_hip import binding
    binding.load_library()
    return binding


@pytest.fixture(scope="module")
def env():
    """ONE pair of 2-layer synthetic models (bf16 and e4m3 weights) with 8 cache rows for the whole module."""
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
# T1: the draft kernel == lookup_draft
# ------------------------------------------------------------------------------------------------
def test_spec_draft_matches_lookup_draft(B):
    from vz_hip import spec
    cases = list(random_cases(150, seed=3))
    rng = random.Random(5)
    for L in (127, 256, 257, 1000, 4096):                 # histories up to a whole context, with sentinel runs and rare repeats
        for vocab in (7, 300):
            seq = [rng.randrange(vocab) for _ in range(L)]
            a = rng.randrange(0, L // 2)
            seq[a:a + L // 5] = [-1] * (L // 5)
            cases.append((seq, rng.randint(1, 7), rng.randint(1, 4), [rng.randrange(vocab)]))
            cases.append((seq[:-3] + seq[L // 2:L // 2 + 3], 7, 3, []))          # a 3-gram that does occur earlier (unless it holds a sentinel)
    cases += [([1, 2, 3, 9, 1, 2, 4, 1, 2], 3, 2, []), ([1, 2, 3, 7, 2], 2, 4, []), ([1, 2, 3, 4], 5, 3, []), ([5], 3, 2, []),
              ([1, 2, 3, 0, 8, 1, 2], 4, 2, [0]), ([1, 2, 0, 8, 1, 2, 5, 1, 2], 4, 2, [0]), ([4, -1, -1, 6, 4], 3, 1, []),
              ([4, 5, -1, 6, 4], 3, 1, []), ([-1, 7, -1, 7], 3, 2, []), ([-1, -1, 3, -1], 3, 2, [])]
    hits = 0
    for seq, k, n, eos in cases:
        want = spec.lookup_draft(seq, k, n, eos)
        got = B.spec_draft(torch.tensor(seq, dtype=torch.int32, device="cuda"), k, n, eos)
        assert got == want, (len(seq), k, n, eos, got, want)
        hits += bool(want)
    assert hits > 60


# ------------------------------------------------------------------------------------------------
# T2: argmax + acceptance on constructed logits
# ------------------------------------------------------------------------------------------------
def _accept(B, g, drafts, *, w=0, budget=100, eos=(), pos0=40, slot0=30, ties=None, done=0, hist_len=5, drafted=None):
    R, V = len(g), 1000
    logits = _rand((R, V), 1.0, 7)
    for i, t in enumerate(g):
        logits[i, t] = 50.0
    for (i, t) in (ties or []):
        logits[i, t] = 50.0
    state = torch.zeros(4, R, dtype=torch.int32)
    state[0] = torch.tensor([11] + list(drafts))
    state[1] = pos0 + torch.arange(R)
    state[2] = slot0 + torch.arange(R)
    state[3] = state[2] + 1
    state = state.cuda()
    ctl = torch.zeros(B.SPEC_CTL_WORDS, dtype=torch.int32)
    ctl[B.SPEC_CTL_WRITE], ctl[B.SPEC_CTL_HIST], ctl[B.SPEC_CTL_DONE] = w, hist_len, done
    ctl[B.SPEC_CTL_DRAFTED] = len(drafts) if drafted is None else drafted
    ctl = ctl.cuda()
    out = torch.full((budget + 8,), -7, dtype=torch.int32, device="cuda")
    hist = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    stats = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    B.spec_accept(logits, state, ctl, out, budget, hist, eos, stats, max_ctx=4096, rope_max=8192)
    return state.cpu(), ctl.cpu().tolist(), out.cpu().tolist(), hist.cpu().tolist(), stats.cpu().tolist()


def _expect(state, ctl, out, hist, stats, *, emitted, w=0, pos0=40, slot0=30, hist_len=5, done=0, drafted=None, R=None):
    n = len(emitted)
    assert out[w:w + n] == emitted and out[w + n] == -7 and (w == 0 or out[w - 1] == -7)
    assert hist[hist_len:hist_len + n] == emitted and hist[hist_len + n] == -7
    assert ctl[0] == w + n and ctl[1] == hist_len + n and ctl[2] == done and ctl[4] == 1
    assert stats == [drafted, max(0, n - 1), n]
    if n:
        assert int(state[0, 0]) == emitted[-1]
    assert state[1].tolist() == [pos0 + n + i for i in range(R)]
    assert state[2].tolist() == [slot0 + n + i for i in range(R)]
    assert state[3].tolist() == [slot0 + n + i + 1 for i in range(R)]


def test_spec_accept_cases(B):
    g = [100, 200, 300, 400]
    # a = 0: the first guess is wrong - one id, the model's own
    _expect(*_accept(B, g, [101, 300, 400]), emitted=[100], drafted=3, R=4)
    # partial: two guesses right, the third wrong
    _expect(*_accept(B, g, [100, 200, 999]), emitted=[100, 200, 300], drafted=3, R=4)
    # a guess that is right AFTER a wrong one does not count
    _expect(*_accept(B, g, [100, 999, 300]), emitted=[100, 200], drafted=3, R=4)
    # full: D accepted, D + 1 emitted; a padded slot that happens to be right is accepted like any guess
    _expect(*_accept(B, g, [100, 200, 300], drafted=1), emitted=[100, 200, 300, 400], drafted=1, R=4)
    # eos inside the accepted run: emitted, nothing behind it, done
    _expect(*_accept(B, g, [100, 200, 300], eos=[200, 5]), emitted=[100, 200], drafted=3, R=4, done=1)
    # eos as the model's own id after a wrong guess
    _expect(*_accept(B, g, [7, 200, 300], eos=[100]), emitted=[100], drafted=3, R=4, done=1)
    # budget clamp inside the run (write index 8 of 10), done when it is reached
    _expect(*_accept(B, g, [100, 200, 300], w=8, budget=10), emitted=[100, 200], w=8, drafted=3, R=4, done=1)
    _expect(*_accept(B, g, [100, 200, 300], w=6, budget=10), emitted=[100, 200, 300, 400], w=6, drafted=3, R=4, done=1)
    # an exact tie resolves to the first maximal index, as the argmax op does: row 1 ties 150 with 200 -> 150
    st = _accept(B, g, [100, 150, 300], ties=[(1, 150)])
    _expect(*st, emitted=[100, 150, 300, 400], drafted=3, R=4)
    assert st[1][B.SPEC_CTL_IDS:B.SPEC_CTL_IDS + 4] == [100, 150, 300, 400]
    lg = _rand((4, 1000), 1.0, 7)
    lg[1, 200] = lg[1, 150] = 50.0
    assert int(B.argmax(lg)[1]) == 150
    # R = 2 and R = 8
    _expect(*_accept(B, [5, 6], [5]), emitted=[5, 6], drafted=1, R=2)
    _expect(*_accept(B, list(range(10, 18)), list(range(10, 14)) + [0, 15, 16]), emitted=[10, 11, 12, 13, 14], drafted=7, R=8)
    # once done, a step emits nothing and moves nothing
    state, ctl, out, hist, stats = _accept(B, g, [100, 200, 300], done=1, w=3)
    assert ctl[0] == 3 and ctl[2] == 1 and ctl[4] == 1 and stats == [0, 0, 0] and out[:8] == [-7] * 8
    assert state[1].tolist() == [40, 41, 42, 43] and state[2].tolist() == [30, 31, 32, 33] and int(state[0, 0]) == 11


# ------------------------------------------------------------------------------------------------
# T3: the verify attention
# ------------------------------------------------------------------------------------------------
def _tables(D, n):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))
    fr = torch.arange(n, dtype=torch.float32).unsqueeze(-1) * inv
    return fr.cos().cuda().contiguous(), fr.sin().cuda().contiguous()


@pytest.mark.parametrize("ctx,nsplit,window", [(1, 4, 0), (77, 8, 0), (1500, 16, 0), (700, 8, 256), (2047, 16, 4096)])
@pytest.mark.parametrize("R", [2, 4, 8])
def test_attention_verify(B, R, ctx, nsplit, window):
    """row i of a verify step = position ctx - 1 + i of the sequence: sees keys [.., ctx - 1 + i] of the cache row after the append."""
    Hq, Hkv, D, max_ctx = 32, 8, 128, 2048 + 24
    kc = _rand((Hkv, max_ctx, D), 1.0, 60).bfloat16()
    vc = _rand((Hkv, max_ctx, D), 1.0, 61).bfloat16()
    cos, sin = _tables(D, max_ctx + 16)
    ticket = None
    for rep in range(2):                                   # twice on the same ticket buffer, the second step R slots further
        L = ctx - 1 + rep * R
        slot = (L + torch.arange(R, dtype=torch.int32)).cuda()
        pos = slot + 5
        qkv = _rand((R, (Hq + 2 * Hkv) * D), 1.0, 62 + rep).bfloat16()
        kc1, vc1 = kc.clone(), vc.clone()
        q = B.rope_kv(qkv, cos, sin, pos, slot, kc1.unsqueeze(0), vc1.unsqueeze(0), 1, R, Hq, Hkv, D)       # the existing RoPE + append
        kc2, vc2 = kc.clone(), vc.clone()
        out, ticket = B.attention_verify(qkv, kc2, vc2, cos, sin, pos, slot, Hq, D ** -0.5, nsplit, L + R, window, ticket)
        assert torch.equal(kc1, kc2) and torch.equal(vc1, vc2), "cache append differs"
        assert int(ticket.abs().sum()) == 0, "ticket not reset by the last arriver"
        for i in range(R):
            n = L + i + 1
            lo = max(0, n - window) if window > 0 else 0
            ref = _ref_attention(q[i:i + 1].unsqueeze(1), kc2[:, lo:n].permute(1, 0, 2).unsqueeze(0), vc2[:, lo:n].permute(1, 0, 2).unsqueeze(0),
                                 D ** -0.5, False, 0, 0, None)
            check_close(f"verify attention R{R} ctx{ctx} rep{rep} row{i}", out[i], ref[0, 0], BF16_MAX, BF16_L2)
        # causality among the new rows: large values in the inputs of rows > i leave row i's output bit-identical
        for i in (0, R // 2):
            if i == R - 1:
                continue
            bad = qkv.clone()
            bad[i + 1:] = 1.0e4
            kc3, vc3 = kc.clone(), vc.clone()
            out3, ticket = B.attention_verify(bad, kc3, vc3, cos, sin, pos, slot, Hq, D ** -0.5, nsplit, L + R, window, ticket)
            assert torch.equal(out3[:i + 1], out[:i + 1]), f"row <= {i} sees a later row"
        kc, vc = kc2, vc2


# ------------------------------------------------------------------------------------------------
# engine-level helpers
# ------------------------------------------------------------------------------------------------
def _spec_run(eng, S, first, history, D, n_new, source=0, stream=None, eos=(), chunk=4, logits=True, info=None):
    """verify steps on the prompt already prefilled into cache row 0 (S positions): (ids incl. `first`, per-id logits or None, records);
    `info` collects decode_info() = (context splits, graphs captured) after every call."""
    R = D + 1
    eng.decode_begin(torch.tensor([first] + [0] * D, dtype=torch.int32), [S + i for i in range(R)], [S + i for i in range(R)])
    eng.set_spec(True, D=D, max_ngram=2, history=list(history) + [first], eos=eos, budget=n_new - 1, source=source, stream=stream)
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


def _text_prompt(env, n, seed):
    return env["synth"].synth_ids(n, env["cfg"].vocab, image_pos=-1, seed=seed)


# ------------------------------------------------------------------------------------------------
# T4: teacher forcing - every row of a verify step against the prefill logits at its position
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["bf16", "fp8"])
@pytest.mark.parametrize("R", [2, 4, 8])
def test_verify_step_matches_prefill(env, which, R):
    eng = env[which].engine
    S = 37
    ids = _text_prompt(env, S + R, 13)
    emb = eng.embed_tokens(ids.unsqueeze(0))
    full, _ = eng.prefill(emb, [S + R], all_logits=True, last_logits=False)
    eng.prefill(emb[:, :S].contiguous(), [S], all_logits=False, last_logits=True)
    eng.decode_begin(torch.tensor([int(ids[S])] + [0] * (R - 1), dtype=torch.int32), [S + i for i in range(R)], [S + i for i in range(R)])
    eng.set_spec(True, D=R - 1, history=ids[:S + 1].tolist(), budget=64, source=1, stream=ids[S + 1:].tolist())      # drafts = the true next ids
    try:
        _, lg = eng.decode_steps(1, return_logits=True)
        eng.check_async()
    finally:
        eng.set_spec(False)
    for i in range(R):
        check_close(f"{which} R{R} verify row {i} vs prefill", lg[0, i], full[0, S + i], 3e-2, 1e-2)


# ------------------------------------------------------------------------------------------------
# T5: the output does not depend on the drafts
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,D", [("bf16", 3), ("bf16", 7), ("fp8", 3), ("fp8", 7)])
def test_output_is_independent_of_the_drafts(env, which, D):
    eng = env[which].engine
    V = env["cfg"].vocab
    pat = _text_prompt(env, 12, 17).tolist()
    prompt = [1] + pat * 3 + pat[:5]                      # 42 positions: + 48 new ids stays inside one 128-key bucket
    S, n_new = len(prompt), 48
    emb = eng.embed_tokens(torch.tensor([prompt]))
    _, last = eng.prefill(emb, [S], all_logits=False, last_logits=True)
    first = int(last[0].argmax())
    ids_a, lg_a, rec_a = _spec_run(eng, S, first, prompt, D, n_new, source=0)                              # n-gram drafts
    assert len(ids_a) == n_new and len(lg_a) == n_new - 1
    ids_b, lg_b, rec_b = _spec_run(eng, S, first, prompt, D, n_new, source=1, stream=ids_a[1:])            # the true continuation
    ids_c, lg_c, rec_c = _spec_run(eng, S, first, prompt, D, n_new, source=1, stream=[(t + 1) % V for t in ids_a[1:]])    # always wrong
    record(f"spec T5 {which} D{D}", steps=[len(rec_a), len(rec_b), len(rec_c)], accepted_ngram=sum(r[1] for r in rec_a))
    assert ids_b == ids_a and ids_c == ids_a
    for t in range(n_new - 1):
        assert torch.equal(lg_a[t], lg_b[t]) and torch.equal(lg_a[t], lg_c[t]), f"logits of id {t + 1} depend on the drafts"
        assert int(lg_a[t].argmax()) == ids_a[t + 1]
    # the true continuation accepts D in every full step, always-wrong accepts nothing and emits one id per step
    assert all(r[1] == D and r[2] == D + 1 for r in rec_b[:-1]) and len(rec_b) == -(-(n_new - 1) // (D + 1))
    assert all(r[1] == 0 and r[2] == 1 for r in rec_c) and len(rec_c) == n_new - 1
    # graph replay = eager
    ids_g, _, rec_g = _spec_run(eng, S, first, prompt, D, n_new, source=1, stream=ids_a[1:], logits=False)
    assert eng.decode_mode()[0], "the verify steps did not run as a captured graph"
    assert ids_g == ids_a and rec_g == rec_b
    ids_h, _, _ = _spec_run(eng, S, first, prompt, D, n_new, source=0, logits=False)
    assert ids_h == ids_a
    # the n-gram rule inside the graph: with a history that CONTAINS the continuation (the ids of run a in front of the first id) the
    # drafts are right most of the time, and every step's record is what the Python rule gives for the history at that step
    from vz_hip import spec
    eng.decode_begin(torch.tensor([first] + [0] * D, dtype=torch.int32), [S + i for i in range(D + 1)], [S + i for i in range(D + 1)])
    eng.set_spec(True, D=D, max_ngram=2, history=ids_a + [first], budget=n_new - 1, source=0)
    try:
        ids_d = [first]
        while not eng.spec_state()["done"]:
            ids_d += eng.decode_steps(3).tolist()
        rec_d = [r for r in eng.spec_state()["records"] if r[2] > 0]
    finally:
        eng.set_spec(False)
    assert ids_d == ids_a
    hist, w = ids_a + [first], 0
    for r in rec_d:
        d = spec.lookup_draft(hist, D, 2)
        pad = d + [0] * (D - len(d))
        acc = 0
        while acc < D and 1 + w + acc < n_new and pad[acc] == ids_a[1 + w + acc]:
            acc += 1
        n = min(acc + 1, n_new - 1 - w)
        assert r == [len(d), n - 1, n], (w, r, d)
        hist += ids_a[1 + w:1 + w + n]
        w += n
    assert w == n_new - 1 and sum(r[1] for r in rec_d) >= 20


# ------------------------------------------------------------------------------------------------
# T6: generate(prompt_lookup_num_tokens=...) against plain greedy generate
# ------------------------------------------------------------------------------------------------
def _near_tie_or_equal(name, model, emb, history, plain, spec_ids, D):
    """equal up to the first divergence; there the plain logits' gap between the two choices must be below 4 x the step's relative-L2
    difference (R-row route vs 1-row route, same prefix) x the logit rms - the criterion of test_depth32_gpu.py / test_stages_gpu.py."""
    f = next((t for t in range(min(len(plain), len(spec_ids))) if plain[t] != spec_ids[t]), -1)
    if f < 0:
        assert len(plain) == len(spec_ids)
        record(name, diverged=-1)
        return
    assert f > 0, "the first id comes from the same prefill"
    eng, S = model.engine, emb.shape[1]
    eng.prefill(emb, [S], all_logits=False, last_logits=True)
    eng.decode_begin(torch.tensor([plain[0]], dtype=torch.int32), [S], [S])
    got, lg = eng.decode_steps(f, return_logits=True)
    assert got[0].tolist() == plain[1:f + 1]
    p = lg[f - 1, 0].float().cpu()
    _, lgs, _ = _spec_run(eng, S, plain[0], history, D, f + 1, source=1, stream=plain[1:])
    q = lgs[f - 1].float().cpu()
    e = errs(q, p)[1]
    gap = float(p[plain[f]] - p[spec_ids[f]])
    tol = 4.0 * e * float(p.double().pow(2).mean().sqrt())
    record(name, diverged=f, gap=gap, tolerance=tol, step_rel_l2=e)
    assert int(q.argmax()) == spec_ids[f], "generate() and the forced verify step disagree on the same prefix"
    assert gap < tol, f"{name}: step {f}: id {spec_ids[f]} vs plain {plain[f]}: gap {gap:.3e} exceeds 4 x error x rms = {tol:.3e}"


def test_generate_with_prompt_lookup_matches_plain_greedy(env):
    model, cfg, S_ = env["bf16"], env["cfg"], env["synth"]
    pat = _text_prompt(env, 24, 23).tolist()
    ids = torch.tensor([[1] + pat * 3 + pat[:7]])
    plain = model.generate(input_ids=ids, do_sample=False, max_new_tokens=40, eos_token_id=None, pad_token_id=2)
    t = {}
    got = model.generate(input_ids=ids, do_sample=False, max_new_tokens=40, eos_token_id=None, pad_token_id=2, prompt_lookup_num_tokens=7, timing=t)
    assert t["spec"]["used"] is True and t["spec"]["D"] == 7 and t["spec"]["tokens"] == got.shape[1] == 40
    assert t["spec"]["steps"] >= 1 and t["spec"]["drafted"] >= t["spec"]["accepted"]
    record("spec T6 text", **t["spec"])
    _near_tie_or_equal("spec T6 text near-tie", model, model.engine.embed_tokens(ids), ids[0].tolist(), plain[0].tolist(), got[0].tolist(), 7)
    # multimodal: the history carries -1 where the 96 visual tokens sit
    tiles = S_.synth_tiles(3, seed=1)
    mm = S_.synth_ids(32, cfg.vocab, image_pos=5, seed=2)
    mm[20:32] = mm[6:18]                                     # some text that repeats
    mm = mm.unsqueeze(0)
    plain = model.generate(input_ids=mm, images=[tiles], do_sample=False, max_new_tokens=24, eos_token_id=None, pad_token_id=2)
    t = {}
    got = model.generate(input_ids=mm, images=[tiles], do_sample=False, max_new_tokens=24, eos_token_id=None, pad_token_id=2,
                         prompt_lookup_num_tokens=4, max_matching_ngram_size=3, timing=t)
    assert t["spec"]["used"] is True and t["spec"]["D"] == 4 and got.shape == (1, 24)
    emb = model.prepare_inputs_labels_for_multimodal(mm, None, None, None, None, [tiles])[4]
    hist = model._spec_history(mm, None, [tiles], emb.shape[1])
    assert len(hist) == 31 + 96 and hist[5:101] == [-1] * 96
    _near_tie_or_equal("spec T6 multimodal near-tie", model, emb, hist, plain[0].tolist(), got[0].tolist(), 4)


# ------------------------------------------------------------------------------------------------
# T7: edges
# ------------------------------------------------------------------------------------------------
def test_generate_prompt_lookup_edges(env):
    model = env["bf16"]
    eng = model.engine
    pat = _text_prompt(env, 24, 29).tolist()
    ids = torch.tensor([[1] + pat * 2 + pat[:9]])
    kw = dict(do_sample=False, pad_token_id=2)
    before = model.generate(input_ids=ids, max_new_tokens=30, eos_token_id=None, **kw)
    ref = model.generate(input_ids=ids, max_new_tokens=30, eos_token_id=None, prompt_lookup_num_tokens=7, **kw)[0].tolist()
    # eos in the middle of the output ends it there (inclusive), wherever in a step's run it falls
    for cut in (3, 10, 17):
        eos = ref[cut]
        n = ref.index(eos) + 1
        got = model.generate(input_ids=ids, max_new_tokens=30, eos_token_id=[eos, 0], prompt_lookup_num_tokens=7, **kw)[0].tolist()
        assert got == ref[:n], (cut, got, ref)
    # max_new_tokens reached in the middle of a run: a prefix of the longer generation
    for n in (1, 2, 5, 13):
        got = model.generate(input_ids=ids, max_new_tokens=n, eos_token_id=None, prompt_lookup_num_tokens=7, **kw)[0].tolist()
        assert got == ref[:n]
    # calls the mode does not cover behave as without the kwarg
    two = torch.cat([ids, ids])
    assert torch.equal(model.generate(input_ids=two, max_new_tokens=6, eos_token_id=None, prompt_lookup_num_tokens=7, **kw),
                       model.generate(input_ids=two, max_new_tokens=6, eos_token_id=None, **kw))
    t = {}
    model.generate(input_ids=ids, max_new_tokens=4, eos_token_id=None, num_beams=2, prompt_lookup_num_tokens=7, timing=t, **kw)
    assert "spec" not in t
    # a left-padded prompt: the history follows the caller's mask
    pad = torch.cat([torch.full((1, 3), 2, dtype=torch.long), ids], 1)
    mask = torch.cat([torch.zeros(1, 3, dtype=torch.long), torch.ones_like(ids)], 1)
    t = {}
    got = model.generate(input_ids=pad, attention_mask=mask, max_new_tokens=30, eos_token_id=None, prompt_lookup_num_tokens=7, timing=t, **kw)
    assert t["spec"]["used"] and got[0].tolist() == ref
    # more eos ids than the device tail takes: today's path, no error
    t = {}
    got = model.generate(input_ids=ids, max_new_tokens=5, eos_token_id=[0, 3, 4, 5, 6], prompt_lookup_num_tokens=7, timing=t, **kw)
    assert "spec" not in t and got.shape[1] <= 5
    # a generation that crosses a context bucket with the mode on.  60 positions + 64 ids, calls of 4 steps: the host's worst-case bound is
    # min(61 + 3 x 8, 124) + 7 = 92 keys for the first call (one 128-key chunk: 1 split) and 124 + 7 = 131 from the third call on (2 splits):
    # the graph is captured again in the middle, and the steps behind it merge two splits on the same ticket / partial buffers.
    long_ids = [1] + (pat * 3)[:59]
    S = len(long_ids)
    emb = eng.embed_tokens(torch.tensor([long_ids]))
    _, last = eng.prefill(emb, [S], all_logits=False, last_logits=True)
    first = int(last[0].argmax())
    V = env["cfg"].vocab
    info_e, info_g = [], []
    cap0 = eng.decode_info()[1]
    ids_e, lg_e, rec_e = _spec_run(eng, S, first, long_ids, 7, 64, source=0, logits=True, info=info_e)
    assert eng.decode_info()[1] == cap0                               # (eager steps capture nothing)
    ids_g, _, rec_g = _spec_run(eng, S, first, long_ids, 7, 64, source=0, logits=False, info=info_g)
    assert ids_g == ids_e and rec_g == rec_e and len(ids_e) == 64
    assert len(rec_e) >= 12, "the drafts were accepted too often for this run to reach the second bucket"
    for info in (info_e, info_g):
        assert [ns for ns, _ in info][:2] == [1, 1] and info[-1][0] == 2 and sorted(set(ns for ns, _ in info)) == [1, 2], info
    caps = [c for _, c in info_g]
    first2 = next(i for i, (ns, _) in enumerate(info_g) if ns == 2)
    assert caps[0] == cap0 + 1 and caps[first2] == caps[first2 - 1] + 1 and caps[-1] == cap0 + 2, info_g      # one capture per bucket
    assert eng.decode_mode()[0]
    # the same ids and bits whatever the drafts, across the bucket change too (a split stays 128 keys)
    ids_w, lg_w, rec_w = _spec_run(eng, S, first, long_ids, 7, 64, source=1, stream=[(t_ + 1) % V for t_ in ids_e[1:]], info=[])
    ids_t, lg_t, rec_t = _spec_run(eng, S, first, long_ids, 7, 64, source=1, stream=ids_e[1:])
    assert ids_w == ids_e and ids_t == ids_e and len(rec_w) == 63 and len(rec_t) == 8
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(lg_e, lg_w, lg_t))
    # a plain generate right after returns to the 1-row path, bit-identically to before
    after = model.generate(input_ids=ids, max_new_tokens=30, eos_token_id=None, **kw)
    assert torch.equal(after, before)


# ------------------------------------------------------------------------------------------------
# T8: the decode graph's key - whatever a captured step froze makes the next call capture again
# ------------------------------------------------------------------------------------------------
def test_knob_change_captures_again(env, B):
    """a captured step froze the routes the vz_tune_set knobs chose: the first decode_steps after a knob change captures again,
    even into the same output buffer, and then runs what an eager step runs under that knob."""
    eng = env["bf16"].engine
    S = 40
    emb = eng.embed_tokens(_text_prompt(env, S, 31).unsqueeze(0))
    _, last = eng.prefill(emb, [S], all_logits=False, last_logits=True)
    first = last[0].argmax().to(torch.int32).view(1)
    buf = torch.empty(1, 4, dtype=torch.int32, device=eng.device)
    cap = lambda: eng.decode_info()[1]        # noqa: E731
    eng.decode_begin(first, [S], [S])
    eng.decode_steps(1)                       # whatever graph an earlier test left is replaced by one of another shape
    c0 = cap()
    eng.decode_steps(4, out=buf)
    c1 = cap()
    eng.decode_steps(4, out=buf)
    assert (c1, cap()) == (c0 + 1, c0 + 1)
    with B.tuned(skinny_mode=0):
        eng.decode_begin(first, [S], [S])
        eng.decode_steps(4, out=buf)
        assert eng.decode_mode()[0] and cap() == c0 + 2, "the knob change did not make the next call capture again"
        eng.decode_begin(first, [S], [S])
        eager, _ = eng.decode_steps(4, return_logits=True)
        assert torch.equal(buf, eager)


def test_colliding_eos_sets_capture_again(env, B):
    """the speculative tail's eos ids are kernel arguments: two eos sets that differ only in ids >= 65536 / their order run on two
    graphs.  Every buffer is held here and the mode is armed through the C ABI, so nothing else differs between the two arms."""
    import ctypes as C
    eng, lib = env["bf16"].engine, B.lib()
    D, budget, W = 3, 16, B.SPEC_CTL_WORDS
    prompt = [1] + _text_prompt(env, 40, 37).tolist()
    S = len(prompt)
    _, last = eng.prefill(eng.embed_tokens(torch.tensor([prompt])), [S], all_logits=False, last_logits=True)
    first = int(last[0].argmax())
    first_ids = torch.tensor([first] + [0] * D, dtype=torch.int32)
    hist0 = torch.tensor(prompt + [first] + [0] * budget, dtype=torch.int32).to(eng.device)
    hist = hist0.clone()
    buf = torch.zeros(W + 4 * budget + 1, dtype=torch.int32, device=eng.device)       # control words | out [budget] | stats [budget][3]
    out, stats = buf[W:], buf[W + budget:]

    def run(eos):
        hist.copy_(hist0)
        eng.decode_begin(first_ids, [S + i for i in range(D + 1)], [S + i for i in range(D + 1)])
        ea = (C.c_int * 4)(*(list(eos) + [0] * (4 - len(eos))))
        B.check(lib.vz_llm_decode_spec(eng.h, 1, D, 2, B.ptr(hist), S + 1, hist.numel(), ea, len(eos), B.ptr(out), budget, B.ptr(buf), B.ptr(stats),
                                       budget, 0, None, 0, eng._s()))
        try:
            B.check(lib.vz_llm_decode_steps(eng.h, 2, B.ptr(out), None, eng._s()))
            eng.check_async()
            host = buf.cpu()
        finally:
            eng.set_spec(False)
        assert eng.decode_mode()[0]
        return host[W:W + int(host[B.SPEC_CTL_WRITE])].tolist(), eng.decode_info()[1]

    free, _ = run(())
    assert 2 <= len(free) <= 2 * (D + 1) and 0 not in free and 1 not in free, free       # (another prompt seed if this ever fires)
    a = next(t for t in range(2, env["cfg"].vocab) if t not in free)
    ids1, cap1 = run((a, 0x10000, 0))
    ids2, cap2 = run((a, 0, 1))
    assert ids1 == free and ids2 == free
    assert cap2 == cap1 + 1, "a different eos set replayed the graph captured with the other one"
