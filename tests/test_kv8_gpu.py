"""The opt-in e4m3 KV mirror through the engine and generate(): a 2-layer full-width synthetic model, max_batch 6,
max_ctx 256, once built with `kv_fp8=True` and once without.  The mirror is a pure function of the bf16 cache, so every writer is held to
`quantize_kv(bf16 cache)` byte for byte; the decode step is held to the oracle fed the engine's own dequantised mirror."""
import pytest
import torch

import kv8_ref as R
from util import band_tol, errs, record

pytestmark = pytest.mark.gpu


def _build(**kw):
    from vz_hip import synth
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    cfg = synth.ArchConfig(n_layers=2)
    hf = VisZephyrConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=2, num_attention_heads=32,
                         num_key_value_heads=8, vocab_size=cfg.vocab, rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta,
                         sliding_window=cfg.sliding_window, eos_token_id=2, pad_token_id=2)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    return cfg, VisZephyrForCausalLM.from_synthetic(hf, seed=0, max_batch=6, max_ctx=256, max_tiles=1, max_text=32, **kw)


@pytest.fixture(scope="module")
def env():
    from oracle import vz_oracle as O
    from vz_hip import synth
    cfg, plain = _build()
    _, model = _build(kv_fp8=True)
    sd = {k: v.cpu() for k, v in synth.iter_state_dict(cfg, 0, device=model.device)}
    torch.cuda.synchronize()
    return dict(cfg=cfg, plain=plain, model=model, sd=sd, O=O, synth=synth)


def band(name, hip, o_bf16, o_fp32):
    """hold the HIP result to the measured bf16 band (tests/test_stages_gpu.py: its module docstring and its band())"""
    e_or = errs(o_bf16, o_fp32)[1]
    mx_hip, e_hip = errs(hip, o_fp32)
    mx_x, e_x = errs(hip, o_bf16)
    record(name, e_oracle_bf16_vs_fp32=e_or, e_hip_vs_fp32=e_hip, e_hip_vs_bf16=e_x, max_hip_vs_fp32=mx_hip)
    assert torch.isfinite(hip.float()).all(), f"{name}: non-finite"
    assert e_hip <= band_tol(e_or), f"{name}: hip vs fp32 {e_hip:.3e} outside the bf16 band (oracle-bf16 vs fp32 {e_or:.3e})"
    assert e_x <= 2.2 * e_or + 5e-4, f"{name}: hip vs oracle-bf16 {e_x:.3e} (band {e_or:.3e})"


def _bits(t):
    """the tensor's bits (uninitialised cache slots may hold NaN, which compares unequal to itself)"""
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _prompt(env, n, seed):
    return env["synth"].synth_ids(n, env["cfg"].vocab, image_pos=-1, seed=seed).unsqueeze(0)


def _check_mirror(eng, at_least=None):
    """Every slot any writer has covered since the mirror was enabled - enabling zeroes the scales, a written row's scale is a power of
    two - holds quantize_kv of the bf16 cache's same slot, bytes and scales, every layer, K and V, every KV head; the covered slots of a
    cache row are a prefix [0, L) and `at_least` = {row: slots it must cover}.  Returns the rows' L."""
    kv = eng.kv_cache()
    q, sc = eng.kv8_mirror()
    lens = []
    for row in range(eng.max_batch):
        covered = sc[0, 0, row, 0] != 0
        L = int(covered.sum())
        assert bool(covered[:L].all()), f"row {row}: covered slots are not a prefix"
        assert L >= (at_least or {}).get(row, 0), f"row {row}: mirror covers {L} slots, expected at least {(at_least or {}).get(row, 0)}"
        lens.append(L)
        assert bool((sc[:, :, row, :, L:] == 0).all()), f"row {row}: a layer or head covers more than {L} slots"
        if L:
            want_q, want_s = R.quantize_kv(kv[:, :, row, :, :L])
            assert torch.equal(sc[:, :, row, :, :L], want_s), f"row {row}: scales of [0, {L})"
            assert torch.equal(q[:, :, row, :, :L], want_q), f"row {row}: bytes of [0, {L})"
    return lens


def test_off_is_off(env):
    """a model built without the keyword has no mirror, and a kv_fp8 engine switched off again runs the same call the same way: ids, key
    splits and graph captures"""
    plain, model = env["plain"], env["model"]
    assert plain.engine.kv_fp8 is False and model.engine.kv_fp8 is True
    with pytest.raises(RuntimeError):
        plain.engine.kv8_mirror()
    ids = _prompt(env, 40, 3)
    kw = dict(do_sample=False, max_new_tokens=24, eos_token_id=None)

    def call(m):
        c0 = m.engine.decode_info()[1]
        out = m.generate(input_ids=ids.to(m.device), **kw)
        ns, c1 = m.engine.decode_info()
        return out[0].tolist(), ns, c1 - c0, m.engine.persist_mode()

    want = call(plain)
    model.engine.set_kv_fp8(False)
    try:
        assert model.engine.kv_fp8 is False
        with pytest.raises(RuntimeError):
            model.engine.kv8_mirror()
        assert call(model) == want
    finally:
        model.engine.set_kv_fp8(True)


def test_prefill_leaves_bf16_untouched(env):
    """prefill logits and the bf16 cache of the kv_fp8 engine are the plain engine's bits; the mirror is quantize_kv of the cache over [0, S)"""
    plain, model = env["plain"].engine, env["model"].engine
    S, lens = 37, [37, 20]
    ids = torch.cat([_prompt(env, S, 5), _prompt(env, S, 6)], 0)
    got = []
    for eng in (plain, model):
        emb = eng.embed_tokens(ids.to(eng.device))
        full, last = eng.prefill(emb, lens, all_logits=True, last_logits=True)
        got.append((full.clone(), last.clone(), eng.kv_cache()))
    for b, n in enumerate(lens):
        assert torch.equal(got[0][0][b, :n], got[1][0][b, :n]) and torch.equal(got[0][1][b], got[1][1][b])
        assert torch.equal(got[0][2][:, :, b, :, :n], got[1][2][:, :, b, :, :n])
    covered = _check_mirror(model, {0: 37, 1: 20})
    assert covered[0] == 37 and covered[1] == 20
    # an append prefill rebuilds the row from slot 0: [0, past + new)
    emb = model.embed_tokens(_prompt(env, 6, 7).to(model.device))
    model.prefill_append(1, emb, [6], [20])
    assert _check_mirror(model, {1: 26})[1] == 26


def test_decode_step_reads_the_mirror(env):
    """teacher forcing as in tests/test_stages_gpu.py::test_decode_matches_prefill_logits, 3 steps behind a prefill of 33 tokens: each
    step's logits sit in the bf16 band around the oracle whose KV cache is the engine's OWN dequantised mirror (two bf16-close K tensors
    quantise to different e4m3 codes on a few percent of the elements - far outside a bf16 band - so the oracle does not quantise for
    itself).  Control: the same logits are farther from the oracle fed the unquantised bf16 cache."""
    cfg, eng, O, sd = env["cfg"], env["model"].engine, env["O"], env["sd"]
    ids = env["synth"].synth_ids(40, cfg.vocab, image_pos=-1, seed=9)
    S0 = 33
    eng.prefill(eng.embed_tokens(ids).unsqueeze(0)[:, :S0].contiguous(), [S0], all_logits=False, last_logits=True)
    for t in range(3):
        n = S0 + t
        q, sc = eng.kv8_mirror()
        kv = eng.kv_cache()
        deq = R.dequant(q[:, :, 0, :, :n], sc[:, :, 0, :, :n]).cpu()            # [layer][K|V][kv head][n][128]
        mirror = O.KVCache([deq[i, 0].permute(1, 0, 2).unsqueeze(0) for i in range(cfg.n_layers)],
                           [deq[i, 1].permute(1, 0, 2).unsqueeze(0) for i in range(cfg.n_layers)], torch.ones(1, n, dtype=torch.bool))
        unq = kv[:, :, 0, :, :n].float().cpu()
        plain = O.KVCache([unq[i, 0].permute(1, 0, 2).unsqueeze(0) for i in range(cfg.n_layers)],
                          [unq[i, 1].permute(1, 0, 2).unsqueeze(0) for i in range(cfg.n_layers)], torch.ones(1, n, dtype=torch.bool))
        tok = ids[n:n + 1].view(1, 1)
        o16, _ = O.llm_forward(cfg, sd, O.embed_tokens(sd, tok, O.BF16), cache=mirror, P=O.BF16)
        o32, _ = O.llm_forward(cfg, sd, O.embed_tokens(sd, tok, O.FP32), cache=mirror, P=O.FP32)
        p32, _ = O.llm_forward(cfg, sd, O.embed_tokens(sd, tok, O.FP32), cache=plain, P=O.FP32)
        eng.decode_begin(ids[n:n + 1].to(torch.int32), [n], [n])
        _, lg = eng.decode_steps(1, return_logits=True)
        e_mirror, e_plain = errs(lg[0, 0], o32[0, 0])[1], errs(lg[0, 0], p32[0, 0])[1]
        record(f"kv8 decode step {t}", e_vs_mirror_oracle=e_mirror, e_vs_unquantised_oracle=e_plain)
        print(f"kv8 decode step {t}: rel-L2 vs mirror-fed oracle {e_mirror:.3e}, vs bf16-cache-fed oracle {e_plain:.3e}")
        band(f"kv8 decode step {t} logits", lg[0, 0], o16[0, 0], o32[0, 0])
        assert e_plain > e_mirror, f"step {t}: the kernel does not read the mirror ({e_plain:.3e} vs {e_mirror:.3e})"
        # the step appended slot n to both caches
        kv1 = eng.kv_cache()
        q1, sc1 = eng.kv8_mirror()
        want_q, want_s = R.quantize_kv(kv1[:, :, 0, :, n])
        assert torch.equal(q1[:, :, 0, :, n], want_q) and torch.equal(sc1[:, :, 0, :, n], want_s)
        assert torch.equal(kv1[:, :, 0, :, :n], kv[:, :, 0, :, :n]) and torch.equal(q1[:, :, 0, :, :n], q[:, :, 0, :, :n])
    _check_mirror(eng, {0: S0 + 3})


def test_every_writer_keeps_the_mirror_exact(env):
    model = env["model"]
    eng = model.engine
    eng.set_kv_fp8(True)                  # start from an empty mirror: what is covered below was covered by these calls
    # continuous batching: 5 requests through 2 rows, admitted together through the spare rows (kv_move_rows + set_row)
    lens, budgets = [9, 30, 17, 12, 25], [5, 14, 9, 3, 11]
    reqs = [{"input_ids": _prompt(env, n, 70 + i), "max_new_tokens": bud} for i, (n, bud) in enumerate(zip(lens, budgets))]
    got = dict(model.generate_stream(reqs, eos_token_id=None, rows=2, sync_every=4))
    assert sorted(got) == list(range(5)) and all(got[i].numel() == budgets[i] for i in range(5))
    covered = _check_mirror(eng)
    assert covered[0] > 0 and covered[1] > 0 and covered[2] > 0, "the admissions did not go through the spare rows"
    # sampled, 3 samples of one prompt: the prompt's KV reaches rows 1 and 2 by copy
    ids = _prompt(env, 21, 80).to(model.device)
    out = model.generate(input_ids=ids, do_sample=True, temperature=0.9, top_p=0.95, seed=11, num_return_sequences=3, max_new_tokens=9, eos_token_id=None)
    assert tuple(out.shape) == (3, 9)
    _check_mirror(eng, {r: 21 + 8 for r in range(3)})
    # guided: the prompts' rows and the negative prompts' rows
    neg = _prompt(env, 7, 81).to(model.device)
    out = model.generate(input_ids=ids, do_sample=False, max_new_tokens=8, eos_token_id=[], guidance_scale=1.5, negative_prompt_ids=neg)
    assert tuple(out.shape) == (1, 8)
    _check_mirror(eng, {0: 21 + 7, 1: 7 + 7})
    # a call that keeps its cache, and the call that continues on it (append prefill + plain steps)
    first = model.generate(input_ids=ids, do_sample=False, max_new_tokens=6, eos_token_id=None, return_dict_in_generate=True)
    _check_mirror(eng, {0: 21 + 5})
    conv = torch.cat([ids, first.sequences.to(model.device), _prompt(env, 5, 82).to(model.device)], 1)
    second = model.generate(input_ids=conv, past_key_values=first.past_key_values, do_sample=False, max_new_tokens=5, eos_token_id=None,
                            return_dict_in_generate=True)
    L = second.past_key_values.lengths[0]
    assert L >= conv.shape[1] + 4
    assert _check_mirror(eng, {0: L})[0] >= L
    # forward() and forward(past_key_values=): a prefill, then 5 more tokens behind the kept cache
    head = model(input_ids=ids[:, :16])
    step = model(input_ids=ids[:, 16:], past_key_values=head.past_key_values)
    assert step.past_key_values.lengths == [21]
    _check_mirror(eng, {0: 21})


def test_stream_yields_the_static_batch_ids(env):
    """with the kernel routes pinned as tests/test_stages_gpu.py::test_continuous_batching_matches_static_batches pins them, generate_stream on
    the kv_fp8 engine yields the ids the static batched call yields (contexts of at most one 128-key chunk: one key split whatever the batch)"""
    from vz_hip import binding as B
    model = env["model"]
    lens, budgets = [9, 30, 17, 44, 12, 25], [5, 21, 9, 30, 1, 18]
    reqs = [{"input_ids": _prompt(env, n, 90 + i), "max_new_tokens": bud} for i, (n, bud) in enumerate(zip(lens, budgets))]
    with B.tuned(gemm256_streamk=0, splitk_mid=0):
        want = {}
        for i, r in enumerate(reqs):
            two = torch.cat([r["input_ids"], r["input_ids"]], 0).to(model.device)
            out = model.generate(input_ids=two, do_sample=False, max_new_tokens=budgets[i], eos_token_id=None, pad_token_id=0)
            assert torch.equal(out[0], out[1])
            want[i] = out[0].tolist()
        for admit in (0, None):
            got = dict(model.generate_stream(reqs, eos_token_id=None, rows=3, sync_every=4, admit=admit))
            assert {i: t.tolist() for i, t in got.items()} == want, f"admit={admit}"


def test_refusals_and_state(env):
    model = env["model"]
    eng = model.engine
    ids = _prompt(env, 24, 95).to(model.device)
    with pytest.raises(NotImplementedError):
        model.generate(input_ids=ids, num_beams=2, max_new_tokens=4)
    with pytest.raises(NotImplementedError):
        model.generate(input_ids=ids, do_sample=True, num_return_sequences=2, share_prompt_kv=True, max_new_tokens=4)
    with pytest.raises(NotImplementedError):
        eng.kv_beam_reorder(2, 1, [0], [4], torch.zeros(2, dtype=torch.int32))
    kw = dict(do_sample=False, max_new_tokens=12, eos_token_id=None)
    rep = torch.cat([ids[:, :8]] * 3, 1)                       # a prompt that repeats itself: prompt lookup would find drafts
    assert model.generate(input_ids=rep, prompt_lookup_num_tokens=3, **kw).tolist() == model.generate(input_ids=rep, **kw).tolist()
    # a row that was not prefilled since the mirror was enabled has no mirror to decode from
    eng.set_kv_fp8(True)
    with pytest.raises(RuntimeError):
        eng.decode_begin(torch.tensor([5], dtype=torch.int32), [10], [10])
    eng.decode_begin(torch.tensor([5], dtype=torch.int32), [0], [0])          # parked: nothing cached, nothing to mirror
    with pytest.raises(RuntimeError):
        eng.decode_set_row(0, 5, 10, 10)
    # a parked row steps 300 times - more than max_ctx: the step's tail saturates its slot at the row's last one - without leaving its
    # cache row: the neighbouring row's caches stay as they are, and what it appended to its own row is mirrored exactly
    eng.prefill_rows(1, eng.embed_tokens(_prompt(env, 40, 96).to(eng.device)), [40])
    kv0 = eng.kv_cache()
    q0, s0 = eng.kv8_mirror()
    eng.decode_begin(torch.tensor([5], dtype=torch.int32), [0], [0])
    for _ in range(3):
        eng.decode_steps(100)
    torch.cuda.synchronize()
    kv1 = eng.kv_cache()
    q1, s1 = eng.kv8_mirror()
    assert _same(kv1[:, :, 1:], kv0[:, :, 1:]) and _same(q1[:, :, 1:], q0[:, :, 1:]) and _same(s1[:, :, 1:], s0[:, :, 1:])
    assert _check_mirror(eng, {0: 1, 1: 40})[1] == 40
