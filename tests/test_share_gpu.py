"""`generate(num_return_sequences=n, share_prompt_kv=True)` and the armed decode step under it (csrc/attn_shared.hip)
on the 2-layer synthetic model of tests/test_sample_rows_gpu.py: the armed step against the copy route on teacher-forced tokens, the
generate route's ids, that nothing is copied, that nothing stays armed, and what is refused.

Tolerance of "armed vs copy route": the two are two bf16 evaluation orders of the same arithmetic - 3e-2 max-norm / 1e-2 relative L2, what
tests/test_append_gpu.py holds two routes of this model to."""
import pytest
import torch

from test_append_gpu import _near_tie
from test_sample_rows_gpu import _prompt, model, pinned_routes  # noqa: F401  (the fixtures of that file)
from util import check_close

pytestmark = pytest.mark.gpu

MAX_TOL, L2_TOL = 3e-2, 1e-2


def _teacher_forced(model, prompts, n, steps, share, seed):
    """[steps, rows, V] logits of `steps` eager steps over the G * n rows of the prompts (id tensors [1, L]), every row fed its own fixed
    token script through decode_set_row - the shape of tests/test_sample_rows_gpu.py::_host_steps - on the copy route or armed"""
    from vz_hip import decode_loop as DL
    from vz_hip import share as SH
    eng = model.engine
    G, lens = len(prompts), [p.shape[1] for p in prompts]
    R = G * n
    ids = torch.full((G, max(lens)), 2, dtype=torch.long)
    for g, p in enumerate(prompts):
        ids[g, :lens[g]] = p[0]
    g_ = torch.Generator().manual_seed(seed)
    script = torch.randint(3, 32000, (R, steps + 1), generator=g_)          # a different token per (row, step)
    assert len({tuple(r) for r in script.tolist()}) == R
    emb = eng.embed_tokens(ids.to(model.device))
    DL.fan_prefill(eng, emb, lens, None, n)
    next_pos, ctx = (DL.fan_share if share else DL.fan_spread)(eng, lens, None, n)
    out = []
    with DL.armed(eng, share=SH.plan(lens, n, steps + 1, eng.max_ctx, 4096, eng.max_batch) if share else None) as begin:
        begin(script[:, 0].to(torch.int32), next_pos, ctx)
        for t in range(steps):
            _, lg = eng.decode_steps(1, return_logits=True)
            out.append(lg[0].float().cpu())
            for r in range(R):
                eng.decode_set_row(r, int(script[r, t + 1]), next_pos[r] + t + 1, ctx[r] + t + 1)
    return torch.stack(out)


def _foreign_kv(model, n, G):
    """every cache row filled with another prompt's KV by the copy route: a prefix read from a row's OWN slots would now be wrong"""
    from vz_hip import decode_loop as DL
    eng = model.engine
    other = _prompt(60, 999)
    DL.fan_prefill(eng, eng.embed_tokens(other.to(model.device).repeat(G, 1)), [60] * G, None, n)
    DL.fan_spread(eng, [60] * G, None, n)


@pytest.mark.parametrize("lens,n", [((40,), 4), ((40, 23), 3)], ids=["1x4", "2x3"])
def test_armed_step_equals_copy_route(model, pinned_routes, lens, n):
    prompts = [_prompt(L, 300 + L) for L in lens]
    want = _teacher_forced(model, prompts, n, 8, False, seed=n)
    _foreign_kv(model, n, len(lens))
    got = _teacher_forced(model, prompts, n, 8, True, seed=n)
    assert got.shape == want.shape == (8, len(lens) * n, 32000)
    for t in range(8):
        for r in range(len(lens) * n):          # every (row, step), no exemptions
            check_close(f"share step {t} row {r} ({len(lens)}x{n})", got[t, r], want[t, r], MAX_TOL, L2_TOL)


def _assert_greedy_or_near_tie(model, ids, got):
    """every token of `got` is the argmax - or a near-tie of it - of the plain forward's logits on the prompt and the tokens before it"""
    fed = ids.to(model.device)
    for t, tok in enumerate(got):
        row = model(input_ids=fed).logits[0, -1]
        assert _near_tie(row, int(tok)), (t, int(tok), int(row.argmax()))
        fed = torch.cat([fed, torch.tensor([[int(tok)]], device=model.device)], 1)


def test_generate_top_k_1_is_greedy(model, pinned_routes):
    ids = [_prompt(21, 90), _prompt(33, 91)]
    kw = dict(do_sample=True, top_k=1, temperature=0.9, seed=7, max_new_tokens=6, eos_token_id=[])
    for p in ids:
        out = model.generate(input_ids=p, num_return_sequences=4, share_prompt_kv=True, **kw)
        assert tuple(out.shape) == (4, 6) and out.dtype == torch.long
        assert all(torch.equal(out[0], out[j]) for j in range(1, 4)), out.tolist()
        greedy = model.generate(input_ids=p, do_sample=False, max_new_tokens=6, eos_token_id=[])[0]
        if not torch.equal(out[0], greedy):
            _assert_greedy_or_near_tie(model, p, out[0].tolist())
    # two prompts of different length, three rows each: HF's order, a prompt's samples adjacent
    both = torch.full((2, 33), 2, dtype=torch.long)
    mask = torch.zeros(2, 33, dtype=torch.long)
    for b, p in enumerate(ids):
        both[b, :p.shape[1]] = p[0]
        mask[b, :p.shape[1]] = 1
    out = model.generate(input_ids=both, attention_mask=mask, num_return_sequences=3, share_prompt_kv=True, **kw)
    assert tuple(out.shape) == (6, 6)
    for b, p in enumerate(ids):
        assert all(torch.equal(out[3 * b], out[3 * b + j]) for j in range(1, 3)), out.tolist()
        _assert_greedy_or_near_tie(model, p, out[3 * b].tolist())


def test_generate_sampled_is_reproducible_and_copies_nothing(model, pinned_routes, monkeypatch):
    ids = _prompt(21, 90)
    kw = dict(do_sample=True, temperature=0.9, top_p=0.95, seed=4242, max_new_tokens=10, eos_token_id=[])

    def no_copy(*a, **k):
        raise AssertionError("kv_move_rows called on the shared route")
    monkeypatch.setattr(model.engine, "kv_move_rows", no_copy)
    a = model.generate(input_ids=ids, num_return_sequences=4, share_prompt_kv=True, **kw)
    b = model.generate(input_ids=ids, num_return_sequences=4, share_prompt_kv=True, **kw)
    assert tuple(a.shape) == (4, 10) and a.dtype == torch.long and torch.equal(a, b)
    assert len({tuple(r) for r in a.tolist()}) > 1          # (four seeds at temperature 0.9: not one sequence four times)
    # with output_scores the recorder sits behind the armed attention as behind the plain one
    out = model.generate(input_ids=ids, num_return_sequences=4, share_prompt_kv=True, return_dict_in_generate=True, output_logprobs=True, **kw)
    assert torch.equal(out.sequences, a) and tuple(out.token_logprobs.shape) == (4, 10) and bool(torch.isfinite(out.token_logprobs).all())


def test_nothing_stays_armed(model, pinned_routes, monkeypatch):
    eng = model.engine
    ids = _prompt(21, 90)
    kw = dict(do_sample=True, temperature=0.9, top_p=0.95, seed=4242, max_new_tokens=8, eos_token_id=[])
    plain = lambda: model.generate(input_ids=ids, do_sample=False, max_new_tokens=8, eos_token_id=[])          # noqa: E731
    copy = lambda: model.generate(input_ids=ids, num_return_sequences=4, **kw)                                   # noqa: E731
    plain0, copy0 = plain(), copy()
    model.generate(input_ids=ids, num_return_sequences=4, share_prompt_kv=True, **kw)
    assert torch.equal(plain(), plain0) and torch.equal(copy(), copy0)
    # a shared call that dies in its first chunk of steps
    real = eng.decode_steps
    with monkeypatch.context() as m:
        def boom(*a, **k):
            raise RuntimeError("decode_steps failed")
        m.setattr(eng, "decode_steps", boom)
        with pytest.raises(RuntimeError, match="decode_steps failed"):
            model.generate(input_ids=ids, num_return_sequences=4, share_prompt_kv=True, **kw)
    assert eng.decode_steps == real
    assert torch.equal(plain(), plain0) and torch.equal(copy(), copy0)
    # ... and a batch of another shape begins: the engine refuses that only while a plan is armed
    eng.decode_begin(torch.zeros(5, dtype=torch.int32), [0] * 5, [0] * 5)


def test_refusals_come_before_the_cache_is_touched(model, monkeypatch):
    eng = model.engine
    ids = _prompt(21, 90)

    def touched(*a, **k):
        raise AssertionError("the engine was used by a refused call")
    with monkeypatch.context() as m:
        for name in ("prefill", "prefill_rows", "prefill_append", "decode_begin", "decode_steps", "kv_move_rows", "set_share"):
            m.setattr(eng, name, touched)
        kw = dict(input_ids=ids, do_sample=True, num_return_sequences=4, share_prompt_kv=True, max_new_tokens=4)
        for bad in (dict(num_beams=2, do_sample=False), dict(guidance_scale=1.5, negative_prompt_ids=ids), dict(past_key_values=object()),
                    dict(prompt_lookup_num_tokens=3), dict(num_return_sequences=1), dict(num_return_sequences=None)):
            with pytest.raises(NotImplementedError, match="share_prompt_kv"):
                model.generate(**{**kw, **bad})
        m.setattr(eng, "tp_size", 2)
        with pytest.raises(NotImplementedError, match="tensor-parallel"):
            model.generate(**kw)


def test_engine_refusals_while_armed(model):
    """what would write into the shared slots, and what the armed step does not run with"""
    from vz_hip import decode_loop as DL
    from vz_hip import share as SH
    from vz_hip.guidance import GuidanceConfig
    eng = model.engine
    ids = _prompt(40, 340)
    DL.fan_prefill(eng, eng.embed_tokens(ids.to(model.device)), [40], None, 3)
    next_pos, ctx = DL.fan_share(eng, [40], None, 3)
    first = torch.tensor([5, 6, 7], dtype=torch.int32)
    with DL.armed(eng, share=SH.plan([40], 3, 8, eng.max_ctx, 4096, eng.max_batch)) as begin:
        with pytest.raises(ValueError, match="decode_begin"):
            eng.decode_begin(torch.zeros(4, dtype=torch.int32), [40] * 4, [40] * 4)          # B != groups * n
        begin(first, next_pos, ctx)
        with pytest.raises(ValueError, match="decode_set_row"):
            eng.decode_set_row(1, 5, 0, 0)                                                     # parks a row
        with pytest.raises(ValueError, match="decode_set_row"):
            eng.decode_set_row(1, 5, 39, 39)                                                   # a context shorter than the shared slots
        with pytest.raises(ValueError, match="kv_move_rows"):
            eng.kv_move_rows([4], [0], [10])                                                   # into the group's first row
        eng.set_guidance(GuidanceConfig(1.5, 1))
        try:
            with pytest.raises(NotImplementedError, match="decode_share"):
                eng.decode_steps(1)                                                            # guidance with the armed step
        finally:
            eng.set_guidance(None)
        assert tuple(eng.decode_steps(2).shape) == (3, 2)                                      # and the armed batch itself still steps
    for bad in (SH.Plan(1, [40, 40, 40]), SH.Plan(65, [40]), SH.Plan(4, [40, 40]), SH.Plan(3, [0]), SH.Plan(3, [eng.max_ctx + 1])):
        with pytest.raises(ValueError, match="decode_share"):
            eng.set_share(bad)
    eng.set_share(None)
