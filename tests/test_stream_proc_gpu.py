"""Per-request logits processors and stop sequences in the serving loop: the per-row processor launch inside the decode
step - graph replay against eager steps and against a host loop over the call-level kernel, re-arming without a capture - and
generate_stream(per_request=True) against generate() run alone with each request's own keywords.  Kernel routes are pinned where rows of
different batches are compared, as in tests/test_sample_rows_gpu.py::test_stream_sampled_requests."""
import os

import pytest
import torch

import stop_ref as SRF

pytestmark = pytest.mark.gpu

LENS3 = [9, 30, 17]


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
    """whole tiles only and no row-count-dependent K slices (tests/test_sample_rows_gpu.py's pins) - and one decode route for every row
    count (skinny_mode 0: the GEMV up to 8 rows).  By default a 2-row linear takes the GEMV and a 3-row one the MFMA weight stream, two
    orders of the same bf16 sums, so a 3-row stream and its 2-row reference agree only up to near-ties - and a request's own processors
    steer it off its free run into one.  Measured: generate(bad_words_ids=) as a 2-row against a 3-row batch parts at token 5, the two
    best logits 4.8478 / 4.8462 against 4.8388 / 4.8459 (max |difference| of the row 0.0199); with this knob the rows' logits are equal
    bit for bit at 2 and 3 rows (the 2-row rows also on the weight stream, knob value 7, are not: 0.0198)."""
    from vz_hip import binding as B
    with B.tuned(gemm256_streamk=0, splitk_mid=0, skinny_mode=0):
        yield


def _prompt(n, seed):
    from vz_hip import synth
    return synth.synth_ids(n, 32000, image_pos=-1, seed=seed).unsqueeze(0)


@pytest.fixture(scope="module")
def three(model):
    """three prompts prefilled together: (first tokens on the device, their plain greedy run of 6 steps)"""
    from vz_hip import binding as B
    eng = model.engine
    ids = torch.full((3, max(LENS3)), 2, dtype=torch.long)
    for b, n in enumerate(LENS3):
        ids[b, :n] = _prompt(n, 80 + b)[0]
    _, last = eng.prefill(eng.embed_tokens(ids.to(model.device)), LENS3)
    first = B.argmax(last)
    eng.decode_begin(first, LENS3, LENS3)
    return first, eng.decode_steps(6).cpu().tolist()


def _process(B, row, cfg, hist):
    """the call-level kernel on one logits row [1, V] with the row's own config and history (a host list)"""
    h = torch.zeros(1, 64, dtype=torch.int32)
    h[0, :len(hist)] = torch.tensor(hist, dtype=torch.int32)
    return B.logits_process(row, cfg, h.to(row.device), torch.tensor([len(hist)], dtype=torch.int32, device=row.device))


# ---- 1. with both modes off the step is what it was (runs first: before anything in this module arms either mode) ------------------------
def test_off_is_the_plain_step(model, three):
    from vz_hip import binding as B
    from vz_hip.logits_proc import ProcConfig
    eng = model.engine
    first, plain = three

    def run():
        eng.prof_enable(True, B.K_OTHER)
        try:
            eng.prof_read()
            eng.decode_begin(first, LENS3, LENS3)
            ids = eng.decode_steps(2).cpu().tolist()
            return ids, eng.prof_read()[0]
        finally:
            eng.prof_enable(False)

    ids0, n0 = run()
    assert [r[:2] for r in plain] == ids0 and n0 > 0 and n0 % 2 == 0
    eng.set_logits_proc_rows(True)
    eng.set_stop_row_seqs(True)
    try:
        eng.decode_begin(first, LENS3, LENS3)
        eng.decode_set_row_logits_proc(0, ProcConfig(suppress=(plain[0][0],)))
        eng.decode_set_row_stop_seqs(0, [[plain[0][1]]])
        eng.stop_rows(0, first)
        _, n_on = run()
        assert n_on == n0 + 2, (n0, n_on)          # the matcher's own scope, one per step; the processor launch sits in the tail's scope
    finally:
        eng.set_stop_row_seqs(False)
        eng.set_logits_proc_rows(False)
    ids1, n1 = run()
    assert ids1 == ids0 and n1 == n0, (n0, n1)


# ---- 2. the step tail ------------------------------------------------------------------------------------------------------------------
def _host_steps(eng, first, cfgs, steps, switch=None):
    """eager steps with the raw logits handed back; every armed row's logits go through the call-level kernel with the row's own config and
    history (its input token appended first, as the step does), the argmax picks, and the rows are armed again with the chosen tokens.
    switch = {step: {row: cfg}} re-arms a row from that step on: its history restarts empty."""
    from vz_hip import binding as B
    cfgs, cur = list(cfgs), first.tolist()
    hist = [[] for _ in cfgs]
    out = [[] for _ in cfgs]
    eng.decode_begin(first, LENS3, LENS3)
    for t in range(steps):
        for r, c in (switch or {}).get(t, {}).items():
            cfgs[r], hist[r] = c, []
        _, lg = eng.decode_steps(1, return_logits=True)
        for r, cfg in enumerate(cfgs):
            row = lg[0, r:r + 1].contiguous()
            if cfg is not None:
                hist[r].append(cur[r])
                _process(B, row, cfg, hist[r])
            cur[r] = int(B.argmax(row))
            out[r].append(cur[r])
            eng.decode_set_row(r, cur[r], LENS3[r] + t + 1, LENS3[r] + t + 1)
    return out


def test_step_tail_equals_host_loop(model, three):
    from vz_hip.logits_proc import ProcConfig
    eng = model.engine
    first, plain = three
    A = ProcConfig(penalty=1.3, suppress=(plain[0][1],))
    Bc = ProcConfig(penalty=1.5, ngram=2, suppress=(plain[2][0],), seq=(((plain[2][2],), float("-inf"), True),))
    other = ProcConfig(ngram=1, suppress=(plain[1][3],))
    cfgs = [A, None, Bc]
    want = _host_steps(eng, first, cfgs, 6)
    want_sw = _host_steps(eng, first, cfgs, 6, switch={3: {1: other}})
    want_off = _host_steps(eng, first, cfgs, 6, switch={3: {0: None}})
    assert want[1] == plain[1] and want[0] != plain[0] and want[2] != plain[2], "the records do not act"

    def run(n_calls, rearm=None, records=cfgs):
        buf = torch.empty(3, 6 // n_calls, dtype=torch.int32, device=model.device)
        eng.set_logits_proc_rows(True)
        try:
            eng.decode_begin(first, LENS3, LENS3)
            for r, c in enumerate(records):
                if c is not None:
                    eng.decode_set_row_logits_proc(r, c)
            parts, caps = [], []
            for c in range(n_calls):
                if c and rearm is not None:
                    eng.decode_set_row_logits_proc(*rearm)
                parts.append(eng.decode_steps(6 // n_calls, out=buf).cpu().clone())
                caps.append(eng.decode_info()[1])
            return torch.cat(parts, 1).tolist(), caps
        finally:
            eng.set_logits_proc_rows(False)

    got, _ = run(1)
    assert got == want, (got, want)
    os.environ["VZ_NO_GRAPH"] = "1"
    try:
        eager, _ = run(1)
    finally:
        del os.environ["VZ_NO_GRAPH"]
    assert eager == got
    halves, caps = run(2)
    assert halves == got and caps[1] == caps[0]
    # re-arming row 1 between two replays: only row 1 moves, from that step on, and nothing is captured again
    sw, caps = run(2, rearm=(1, other))
    assert sw == want_sw and caps[1] == caps[0], (sw, want_sw, caps)
    assert sw[0] == got[0] and sw[2] == got[2] and sw[1][:3] == got[1][:3] and sw[1][3] != got[1][3]
    # deactivating a row: plain greedy steps from there on; every record inactive: the plain run
    off, caps = run(2, rearm=(0, None))
    assert off == want_off and caps[1] == caps[0] and off[0][:3] == got[0][:3]
    idle, _ = run(1, records=[None, None, None])
    assert idle == plain


def test_refusals(model, three):
    from vz_hip.logits_proc import ProcConfig
    eng = model.engine
    first, _ = three
    cfg = ProcConfig(penalty=1.2)
    # the call-level processors and the per-row mode together, whichever is armed second
    eng.set_logits_proc(cfg)
    try:
        with pytest.raises(ValueError, match="one of the two forms"):
            eng.set_logits_proc_rows(True)
    finally:
        eng.set_logits_proc(None)
    eng.set_logits_proc_rows(True)
    try:
        with pytest.raises(ValueError, match="one of the two forms"):
            eng.set_logits_proc(cfg)
        with pytest.raises(ValueError):
            eng.decode_set_row_logits_proc(0, ProcConfig(ngram=9))
        with pytest.raises(ValueError):
            eng.decode_set_row_logits_proc(6, cfg)
        # with the beam tail decode_steps refuses, as it does for the per-row sampling tail
        eng.decode_begin(first, LENS3, LENS3)
        eng.set_beam(True, 3, 1, [], LENS3[:1], torch.zeros(3, device=model.device), torch.empty(1, 1, 6, 3, dtype=torch.int32, device=model.device))
        with pytest.raises(ValueError, match="per-row logits processors"):
            eng.decode_steps(1)
    finally:
        eng.set_beam(False)
        eng.set_logits_proc_rows(False)
    with pytest.raises(ValueError, match="per-row logits processors are off"):
        eng.decode_set_row_logits_proc(0, cfg)
    # the per-row stop sequences: the call's and the row's share 16; the call-level set cannot change under the armed mode
    eng.set_stop_row_seqs(True)
    try:
        eng.decode_set_row_stop_seqs(0, [[t] for t in range(16)])
        with pytest.raises(ValueError):
            eng.decode_set_row_stop_seqs(0, [[t] for t in range(17)])
        with pytest.raises(ValueError, match="per-row stop sequences are armed"):
            eng.set_stop(None)
    finally:
        eng.set_stop_row_seqs(False)
    with pytest.raises(ValueError, match="per-row stop sequences are off"):
        eng.decode_set_row_stop_seqs(0, [[5]])


# ---- 3. generate_stream ------------------------------------------------------------------------------------------------------------------
def _alone(model, ids, budget, **kw):
    """generate() on the request alone, as row 0 of a 2-row batch (the kernels the stream's rows run on)"""
    out = model.generate(input_ids=ids.repeat(2, 1), do_sample=False, max_new_tokens=budget, eos_token_id=[], **kw)
    assert torch.equal(out[0], out[1])
    return out[0].tolist()


def _host_generate(model, ids, p, cfg, max_new):
    """the sampled request alone in both rows of a 2-row batch by a host-driven loop: raw logits back, the call-level processor kernel on each
    row with its history, the one-row sampler with the request's seed and draw counter t"""
    from vz_hip import binding as B
    eng = model.engine
    L = ids.shape[1]
    _, last = eng.prefill(eng.embed_tokens(ids.to(model.device).repeat(2, 1)), [L, L])
    out = [[], []]

    def choose(lg, t):
        for r in range(2):
            row = lg[r:r + 1].contiguous().clone()
            if cfg is not None:
                _process(B, row, cfg, out[r])
            tok = B.sample(row, p.temperature, p.top_k, p.top_p, p.seed, t) if p.sample else B.argmax(row)
            out[r].append(int(tok))
        return [out[0][-1], out[1][-1]]

    toks = choose(last, 0)
    for t in range(1, max_new):
        eng.decode_begin(torch.tensor(toks, dtype=torch.int32), [L + t - 1] * 2, [L + t - 1] * 2)
        _, lg = eng.decode_steps(1, return_logits=True)
        toks = choose(lg[0], t)
    assert out[0] == out[1]
    return out[0]


def test_stream_with_per_request_keys(model, pinned_routes):
    """Six requests, each with its own keys, against generate() run alone with those keys as row 0 of a 2-row batch.
    The routes are pinned so that the stream's 3 rows and the 2-row references run one decode route (the `pinned_routes` fixture says why):
    every list is compared for equality."""
    from vz_hip import logits_proc as LP
    from vz_hip.sample_rows import parse_request
    lens = [9, 30, 17, 44, 12, 25]
    budgets = [8, 10, 9, 11, 10, 8]
    prompts = [_prompt(n, 70 + i) for i, n in enumerate(lens)]
    samp = dict(do_sample=True, temperature=0.9, top_p=0.95, seed=21)
    par4 = parse_request(samp, model.generation_config, None)
    free = [_alone(model, prompts[i], budgets[i]) if i != 4 else _host_generate(model, prompts[4], par4, None, budgets[4]) for i in range(6)]
    x = next(t for t in range(1000, 32000) if t not in free[2])
    pair = [free[3][4], free[3][5]]
    own = [dict(suppress_tokens=[free[0][1]]), dict(bad_words_ids=[[free[1][2], free[1][3]]]), dict(sequence_bias={(x,): 1e4}),
           dict(stop_token_sequences=[pair]), dict(repetition_penalty=1.3, no_repeat_ngram_size=2, **samp), {}]
    reqs = [{"input_ids": prompts[i], "max_new_tokens": budgets[i], **own[i]} for i in range(6)]
    cfg4 = LP.parse(repetition_penalty=1.3, no_repeat_ngram_size=2, eos=[], vocab=32000)
    want = [_alone(model, prompts[0], budgets[0], suppress_tokens=[free[0][1]]),
            _alone(model, prompts[1], budgets[1], bad_words_ids=[[free[1][2], free[1][3]]]),
            _alone(model, prompts[2], budgets[2], sequence_bias={(x,): 1e4}),
            _alone(model, prompts[3], budgets[3], stopping_criteria=[SRF.keyword_criterion([pair], 0)]),
            _host_generate(model, prompts[4], par4, cfg4, budgets[4]),
            free[5]]
    print("free", free, "want", want)
    # every key acts where it must: token 1; token 3; every token x; cut inclusive at token 5; no bigram twice
    assert want[0][0] == free[0][0] and want[0][1] != free[0][1] and free[0][1] not in want[0]
    assert want[1][:3] == free[1][:3] and want[1][3] != free[1][3]
    assert want[2] == [x] * budgets[2]
    assert want[3] == free[3][:6] and len(free[3]) > 6
    # (the sampled request: whether a penalty on the few ids seen so far turns a Gumbel race cannot be said in advance - it is held to
    # its own reference below, which runs the processors on the host side of the API)
    assert len(set(zip(want[4], want[4][1:]))) == len(want[4]) - 1
    for admit in (0, None):
        got = {i: t.tolist() for i, t in model.generate_stream(reqs, eos_token_id=[], rows=3, sync_every=4, admit=admit, per_request=True)}
        assert sorted(got) == list(range(6))
        for i in range(6):
            assert got[i] == want[i], f"admit={admit} request {i}: {got[i]} vs {want[i]}"
    # both modes are off again behind the call
    assert _alone(model, prompts[5], budgets[5]) == free[5]


def test_flag_on_without_keys_is_flag_off(model, pinned_routes):
    lens = [9, 30, 17, 44, 12, 25]
    reqs = [{"input_ids": _prompt(n, 70 + i), "max_new_tokens": 7 + i % 3} for i, n in enumerate(lens)]
    off = {i: t.tolist() for i, t in model.generate_stream(reqs, eos_token_id=[], rows=3, sync_every=4)}
    on = {i: t.tolist() for i, t in model.generate_stream(reqs, eos_token_id=[], rows=3, sync_every=4, per_request=True)}
    assert on == off and sorted(on) == list(range(6))
    for key, val in (("repetition_penalty", 1.2), ("stop_token_sequences", [[5, 6]])):
        with pytest.raises(NotImplementedError):
            next(model.generate_stream([{**reqs[0], key: val}], rows=3))
    # a request's stop sequences beside the call's: together at most 16, refused before the request runs
    with pytest.raises(ValueError, match="at most 16"):
        next(model.generate_stream([{**reqs[0], "stop_token_sequences": [[5, 6]] * 3}], rows=3, per_request=True, stop_token_sequences=[[7, 8]] * 14))
