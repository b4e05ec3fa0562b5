"""The per-row step tail (csrc/sampling.hip: sample_rows_kernel) and what is built on it: the op against the one-row calls of the existing
kernels bit for bit and against oracle/sampling_oracle.py, the tail inside the decode step against a host-driven loop, generate_stream with
per-request sampling, and generate(do_sample=True, num_return_sequences=n)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NEG = float("-inf")


def _logits(rows, V, seed, scale=2.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, V, generator=g) * scale).float()


def _params(rows, seed, greedy=()):
    """random per-row parameters: T in [0.1, 1.3], top_k in {0, 5, 50}, top_p in {0.3, 0.9, 1.0}, distinct seeds, counters in {0, 1, 77}"""
    from vz_hip.sample_rows import GREEDY, RowParams
    rng = np.random.RandomState(seed)
    out = []
    for r in range(rows):
        p = RowParams(True, float(rng.uniform(0.1, 1.3)), int(rng.choice([0, 5, 50])), float(rng.choice([0.3, 0.9, 1.0])),
                      0x1234_5678_0000_0000 + 7919 * r + seed, int(rng.choice([0, 1, 77])))
        out.append(GREEDY.at(p.counter) if r in greedy else p)
    return out


def _pick(B, row_logits, p, counter):
    """the row's token by the EXISTING kernels called on that row alone (so the sampler's Philox row word is 0): int32 [1] on the device"""
    if not p.sample:
        return B.argmax(row_logits)
    return B.sample(row_logits, p.temperature, p.top_k, p.top_p, p.seed, counter)


# ---- 1. the op against the existing kernels, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1000, 32000, 32001, 40000])          # 40000 > 32768: the loop form
@pytest.mark.parametrize("R", [1, 3, 64])
def test_op_equals_one_row_calls(R, V):
    from vz_hip import binding as B
    from vz_hip.sample_rows import GREEDY, RowParams
    x = _logits(R, V, seed=V + R)
    if R == 1:
        tables = [_params(1, 3), [GREEDY]]
    elif R == 3:
        tables = [_params(3, 5, greedy=(0,))]
        x[0, 7] = x[0, V - 3] = x[0].max() + 1.0                     # greedy row, exact tie at the maximum: the first index wins
        x[2, 11] += 200.0                                            # sampled row whose kept set is one token
        tables[0][2] = RowParams(True, 0.7, 5, 0.3, tables[0][2].seed, 1)
    else:
        tables = [_params(64, 9, greedy=(0, 1, 2, 5, 40))]
        t = tables[0]
        x[0, 7] = x[0, V - 3] = x[0].max() + 1.0                     # greedy: exact tie at the maximum
        x[1] = NEG                                                   # greedy: a row of -inf
        x[5, ::3] = NEG                                              # greedy: -inf among the values
        x[3] = NEG                                                   # sampled: a row of -inf
        x[4, 11] += 200.0                                            # sampled: the kept set is one token
        t[4] = RowParams(True, 0.7, 5, 0.3, t[4].seed, 1)
        x[6, 20] = x[6, 900] = x[6].max() + 0.5                      # sampled: exact tie at the maximum
        assert all(p.sample for p in (t[3], t[4], t[6])) and sum(not p.sample for p in t) >= 3
    xd = x.cuda()
    for params in tables:
        got = B.sample_rows(xd, params)
        want = torch.cat([_pick(B, xd[r:r + 1], params[r], params[r].counter) for r in range(R)])
        assert torch.equal(got, want), (got.tolist(), want.tolist())
        if R == 3:
            assert int(got[0]) == 7 and int(got[2]) == 11
        if R == 64:
            assert int(got[0]) == 7 and int(got[1]) == 0 and int(got[4]) == 11
            # draws do not depend on the row a request sits in: rows and table entries permuted together permute the ids
            perm = torch.randperm(R, generator=torch.Generator().manual_seed(1))
            got_p = B.sample_rows(xd[perm.cuda()].contiguous(), [params[int(i)] for i in perm])
            assert torch.equal(got_p, got[perm.cuda()])


def test_op_refuses_bad_entries():
    from vz_hip import binding as B
    from vz_hip.sample_rows import RowParams
    x = _logits(2, 1000, 1).cuda()
    ok = RowParams(True, 0.7, 50, 0.9, 1, 0)
    for bad in (RowParams(True, 0.0, 50, 0.9, 1, 0), RowParams(True, 0.7, -1, 0.9, 1, 0), RowParams(True, 0.7, 50, 0.0, 1, 0),
                RowParams(True, 0.7, 50, 1.5, 1, 0), RowParams(True, 0.7, 50, 0.9, 1, -1)):
        with pytest.raises(ValueError):
            B.sample_rows(x, [ok, bad])


# ---- 2. the op against the oracle ----------------------------------------------------------------------------------------------------
# per-row parameter sets (the cases of tests/test_sampling_gpu.py::test_draw_equals_oracle), row r takes set r % 6 and counter (0, 1, 77)[r % 3]
_ORACLE_SETS = [(0.2, 50, 1.0), (0.7, 0, 0.9), (1.0, 20, 0.5), (0.1, 50, 0.95), (1.3, 0, 1.0), (0.7, 5, 0.3)]


def _oracle_case(V):
    from vz_hip.sample_rows import RowParams
    rows = 24
    x = _logits(rows, V, seed=V + 1)
    params = [RowParams(True, *_ORACLE_SETS[r % 6], 0x0BAD_5EED_0000_0000 + 104729 * r + V, (0, 1, 77)[r % 3]) for r in range(rows)]
    return x, params


@pytest.mark.parametrize("V", [1000, 32000, 32001])
def test_op_equals_oracle(V):
    """the allowance of tests/test_sampling_gpu.py::test_draw_equals_oracle, with the oracle's row word 0 for every row.  The seeds were kept
    after running the oracle alone on these inputs: the smallest gap between the two best race scores is 7.0e-3 (V = 32000), far from the
    1e-3 near-tie allowance, and no drawn token is a top-p boundary token."""
    from oracle import sampling_oracle as S
    from vz_hip import binding as B
    x, params = _oracle_case(V)
    got = B.sample_rows(x.cuda(), params).cpu().tolist()
    bad = 0
    for r, p in enumerate(params):
        xr = x[r].numpy()
        T, k, tp = p.temperature, p.top_k, p.top_p
        want, margin = S.draw(xr, T, k, tp, p.seed, p.counter, row=0, return_margin=True)
        loose = np.isfinite(S.warp(xr, T, k, min(1.0, tp + 1e-5))) if tp < 1.0 else np.isfinite(S.warp(xr, T, k, tp))
        assert loose[got[r]], f"row {r}: drew token {got[r]}, which the warpers filter"
        if got[r] != want:
            strict = np.isfinite(S.warp(xr, T, k, max(1e-6, tp - 1e-5)))
            assert margin < 1e-3 or not strict[got[r]] or not strict[want], (r, got[r], want, margin)
            bad += 1
    assert bad <= 2, f"{bad} of {len(params)} draws differ from the oracle"


# ---- the model the step-tail, stream and generate tests share ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from vz_hip import synth
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    cfg = synth.ArchConfig(n_layers=2)
    hf = VisZephyrConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=2, num_attention_heads=32,
                         num_key_value_heads=8, vocab_size=cfg.vocab, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    return VisZephyrForCausalLM.from_synthetic(hf, seed=0, max_batch=6, max_ctx=256, max_tiles=1, max_text=32)


@pytest.fixture()
def pinned_routes():
    """whole tiles only and no row-count-dependent K slices: rows of different batches get the same bits (the setup of
    tests/test_stages_gpu.py::test_continuous_batching_matches_static_batches)"""
    from vz_hip import binding as B
    with B.tuned(gemm256_streamk=0, splitk_mid=0):
        yield


def _prompt(n, seed):
    from vz_hip import synth
    return synth.synth_ids(n, 32000, image_pos=-1, seed=seed).unsqueeze(0)


def _host_steps(eng, first, next_pos, ctx, params, steps, switch=None):
    """The host-driven loop: eager steps with the logits handed back, every row's token chosen on the host side of the API with the one-row
    calls of the existing kernels, the counters counted up here, and the rows armed again with the chosen tokens.  params[r].counter = the
    draw counter of row r's first step; switch = {step: {row: params}} re-arms a row from that step on.  Returns [rows][steps] ids."""
    from vz_hip import binding as B
    R = len(params)
    params = list(params)
    ctr = [p.counter for p in params]
    eng.set_sampling_rows(None)
    eng.decode_begin(first, next_pos, ctx)
    out = [[] for _ in range(R)]
    for t in range(steps):
        for r, p in (switch or {}).get(t, {}).items():
            params[r], ctr[r] = p, p.counter
        _, lg = eng.decode_steps(1, return_logits=True)
        toks = torch.cat([_pick(B, lg[0, r:r + 1].contiguous(), params[r], ctr[r]) for r in range(R)]).tolist()
        for r in range(R):
            out[r].append(int(toks[r]))
            ctr[r] += 1
            eng.decode_set_row(r, toks[r], next_pos[r] + t + 1, ctx[r] + t + 1)
    return out


def _host_generate(model, ids, params, max_new):
    """`max_new` tokens of the prompt `ids` [1, L] in every row of a len(params)-row batch, row r by params[r], with the host-driven loop:
    the first token from the prefill logits with counter 0, the steps from counter 1."""
    from vz_hip import binding as B
    eng = model.engine
    R, L = len(params), ids.shape[1]
    emb = eng.embed_tokens(ids.to(model.device).repeat(R, 1))
    _, last = eng.prefill(emb, [L] * R)
    first = torch.cat([_pick(B, last[r:r + 1].contiguous(), params[r], 0) for r in range(R)])
    rest = _host_steps(eng, first, [L] * R, [L] * R, [p.at(1) for p in params], max_new - 1) if max_new > 1 else [[] for _ in range(R)]
    return [[int(first[r])] + rest[r] for r in range(R)]


# ---- 3. the step tail ----------------------------------------------------------------------------------------------------------------
def test_step_tail_equals_host_loop(model):
    from vz_hip import binding as B
    from vz_hip.sample_rows import GREEDY, RowParams
    eng = model.engine
    lens = [9, 30, 17]
    S = max(lens)
    ids = torch.full((3, S), 2, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = _prompt(n, 80 + b)[0]
    _, last = eng.prefill(eng.embed_tokens(ids.to(model.device)), lens)
    first = B.argmax(last)
    params = [RowParams(True, 0.9, 50, 0.95, 4242, 1), GREEDY.at(5), RowParams(True, 0.4, 5, 1.0, 77, 77)]
    other = RowParams(True, 1.2, 0, 0.9, 31337, 3)
    want = _host_steps(eng, first, lens, lens, params, 6)
    want_sw = _host_steps(eng, first, lens, lens, params, 6, switch={3: {1: other}})

    def run(n_calls, rearm=None):
        buf = torch.empty(3, 6 // n_calls, dtype=torch.int32, device=model.device)
        eng.set_sampling_rows(params)
        try:
            eng.decode_begin(first, lens, lens)
            parts, caps = [], []
            for c in range(n_calls):
                if c and rearm is not None:
                    eng.decode_set_row_sampling(*rearm)
                parts.append(eng.decode_steps(6 // n_calls, out=buf).cpu().clone())
                caps.append(eng.decode_info()[1])
            return torch.cat(parts, 1).tolist(), caps
        finally:
            eng.set_sampling_rows(None)

    got, _ = run(1)
    assert got == want, (got, want)
    os.environ["VZ_NO_GRAPH"] = "1"
    try:
        eager, _ = run(1)
    finally:
        del os.environ["VZ_NO_GRAPH"]
    assert eager == got
    # re-arming one row between two replays: that row follows its new parameters, the others do not move, nothing is captured again
    halves, caps = run(2)
    assert halves == got and caps[1] == caps[0]
    sw, caps = run(2, rearm=(1, other))
    assert sw == want_sw and caps[1] == caps[0], (sw, want_sw, caps)
    assert sw[0] == got[0] and sw[2] == got[2] and sw[1][:3] == got[1][:3]
    # the tail refuses the company the issue names
    eng.set_sampling_rows(params)
    try:
        eng.decode_begin(first, lens, lens)
        eng.set_beam(True, 3, 1, [], lens[:1], torch.zeros(3, device=model.device), torch.empty(1, 1, 6, 3, dtype=torch.int32, device=model.device))
        with pytest.raises(ValueError, match="per-row tail"):
            eng.decode_steps(1)
    finally:
        eng.set_beam(False)
        eng.set_sampling_rows(None)
    # and with it off the greedy step is what it was
    eng.decode_begin(first, lens, lens)
    g = eng.decode_steps(2).cpu().tolist()
    assert g[1] == want[1][:2]


# ---- 4. generate_stream ----------------------------------------------------------------------------------------------------------------
def test_stream_sampled_requests(model, pinned_routes):
    from vz_hip.sample_rows import GREEDY, parse_request
    lens = [9, 30, 17, 44, 12, 25]
    budgets = [5, 12, 9, 11, 7, 10]
    samp = [dict(do_sample=True, temperature=0.9, top_p=0.95, seed=11), None, dict(do_sample=True, temperature=0.3, top_k=5, seed=12),
            dict(do_sample=True, temperature=1.2, top_k=0, top_p=0.9, seed=13), None, dict(do_sample=True, temperature=0.7, seed=14)]
    reqs = []
    for i, (n, bud) in enumerate(zip(lens, budgets)):
        reqs.append({"input_ids": _prompt(n, 70 + i), "max_new_tokens": bud, **(samp[i] or {})})
    pars = [parse_request(r, model.generation_config, None) for r in reqs]
    assert [p.sample for p in pars] == [True, False, True, True, False, True] and pars[0].top_k == 50 and pars[3].top_k == 0

    def alone(i, p):     # the same request as row 0 of a 2-row batch (same kernels as the stream's rows)
        two = _host_generate(model, reqs[i]["input_ids"], [p, p], budgets[i])
        assert two[0] == two[1]
        return two[0]

    free_run = [alone(i, pars[i]) for i in range(len(reqs))]
    assert len({tuple(f) for f in free_run}) == len(reqs)
    # an eos that a sampled request emits mid-chunk (sync_every = 4: its 7th or 8th token) and that is nobody's first token
    firsts = {f[0] for f in free_run}
    eos = next(free_run[i][k] for i in (3, 5, 2) for k in (6, 7) if free_run[i][k] not in firsts)
    for admit in (0, None):
        got = dict(model.generate_stream(reqs, eos_token_id=[eos], rows=3, sync_every=4, admit=admit))
        assert sorted(got) == list(range(len(reqs)))
        for i, want in enumerate(free_run):
            want = want[: want.index(eos) + 1] if eos in want else want
            assert got[i].tolist() == want, f"admit={admit} request {i}: {got[i].tolist()} vs {want}"
        assert any(eos in f[:-1] for f in free_run), "the eos ended no request early"
    # a stream whose requests are all greedy: the greedy tokens, by the code it always ran
    plain = [{"input_ids": r["input_ids"], "max_new_tokens": r["max_new_tokens"]} for r in reqs]
    greedy_run = [alone(i, GREEDY) for i in range(len(reqs))]
    got = dict(model.generate_stream(plain, eos_token_id=None, rows=3, sync_every=4))
    assert [got[i].tolist() for i in range(len(reqs))] == greedy_run
    assert greedy_run[1] == free_run[1] and greedy_run[4] == free_run[4]
    with pytest.raises(NotImplementedError):
        next(model.generate_stream([{**reqs[0], "repetition_penalty": 1.2}], rows=3))


# ---- 5. num_return_sequences -------------------------------------------------------------------------------------------------------------
def test_num_return_sequences(model, pinned_routes):
    from vz_hip.sample_rows import RowParams
    ids = _prompt(21, 90)
    s = 4242
    kw = dict(do_sample=True, temperature=0.9, top_p=0.95, seed=s, max_new_tokens=10, eos_token_id=[])
    out = model.generate(input_ids=ids, num_return_sequences=4, **kw)
    assert tuple(out.shape) == (4, 10) and out.dtype == torch.long
    assert len({tuple(r) for r in out.tolist()}) > 1, "the four samples are all equal"
    want = _host_generate(model, ids, [RowParams(True, 0.9, 50, 0.95, s + j, 0) for j in range(4)], 10)
    assert out.tolist() == want, (out.tolist(), want)
    # two prompts of different length, n = 2: prompt-major, rows b * 2 + j under seed s + b * 2 + j
    ids2 = _prompt(13, 91)
    both = torch.full((2, 21), 2, dtype=torch.long)
    both[0], both[1, :13] = ids[0], ids2[0]
    mask = torch.zeros(2, 21, dtype=torch.long)
    mask[0], mask[1, :13] = 1, 1
    out2 = model.generate(input_ids=both, attention_mask=mask, num_return_sequences=2, **kw)
    assert tuple(out2.shape) == (4, 10)
    a = model.generate(input_ids=ids, num_return_sequences=2, **kw)
    b = model.generate(input_ids=ids2, num_return_sequences=2, **{**kw, "seed": s + 2})
    assert out2[:2].tolist() == a.tolist() == want[:2] and out2[2:].tolist() == b.tolist()
    # logits processors work: a suppressed token never appears
    t = int(out[0, 0])
    sup = model.generate(input_ids=ids, num_return_sequences=4, suppress_tokens=[t], **kw)
    assert tuple(sup.shape) == (4, 10) and not bool((sup == t).any()) and bool((out == t).any())
    with pytest.raises(ValueError, match="Greedy methods without beam search"):
        model.generate(input_ids=ids, do_sample=False, num_return_sequences=2, max_new_tokens=4)

    class _St:
        def put(self, v):
            pass

        def end(self):
            pass
    with pytest.raises(NotImplementedError):
        model.generate(input_ids=ids, num_return_sequences=2, streamer=_St(), **kw)
    with pytest.raises(ValueError):
        model.generate(input_ids=ids, num_return_sequences=7, **kw)          # the engine has 6 cache rows
    # n = 1 is the code it always was
    one = model.generate(input_ids=ids, **kw)
    assert tuple(one.shape) == (1, 10) and model.generate(input_ids=ids, num_return_sequences=1, **kw).tolist() == one.tolist()
