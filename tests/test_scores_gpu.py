"""The step recorder (csrc/sampling.hip: token_scores_kernel) and what is built on it: the op against float64 and oracle/sampling_oracle.py,
the recorder inside the decode step against the op on the logits of a host-driven loop bit for bit, generate()'s score outputs,
generate_stream's per-request log-probs, and what the engine refuses.

Tolerance on lse and lse_kept: 2e-5 + 2^-22 * max|x| (x / T for the kept sum).  The kernel adds at most 64 (a thread's stride-1024
elements of a row of up to 65536) + 6 (wave) + 16 (wave partials) positive fp32 terms in sequence: relative error <= 86 * 2^-24 ~ 5e-6 of
the sum, i.e. 5e-6 absolute in its log; expf / logf add a few ulp each, the rounding of x - m a relative 2e-6 or less on the terms that
matter, and the final m + log(sum) rounds to one ulp of a result bounded by max|x| + log V."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NEG = float("-inf")
_ORACLE_SETS = [(0.2, 50, 1.0), (0.7, 0, 0.9), (1.0, 20, 0.5), (0.1, 50, 0.95), (1.3, 0, 1.0), (0.7, 5, 0.3)]


def _logits(rows, V, seed, scale=2.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, V, generator=g) * scale).float()


def _par(s):
    from vz_hip.sample_rows import GREEDY, RowParams
    return GREEDY if s is None else RowParams(True, s[0], s[1], s[2], 0, 0)


def _tol(x):
    f = np.abs(x[np.isfinite(x)])
    return 2e-5 + 2.0 ** -22 * (float(f.max()) if f.size else 0.0)


def _lse64(v):
    v = v.astype(np.float64)
    v = v[np.isfinite(v)]
    if v.size == 0:
        return NEG
    m = v.max()
    return float(m + np.log(np.exp(v - m).sum()))


def _check(x, sets, toks):
    """B.token_scores(x, toks, sets, warped=True) against float64 and the oracle's kept set.  Returns the tokens whose membership differs
    from the oracle's (allowed at the top-p boundary only: inside the symmetric difference of warp(p - 1e-5) and warp(p + 1e-5), at most one
    per row; such a row skips the lse_kept comparison)."""
    from oracle import sampling_oracle as S
    from vz_hip import binding as B
    from vz_hip import scores as SC
    R, V = x.shape
    rec, warped = B.token_scores(x.cuda(), torch.tensor(toks, dtype=torch.int32).cuda(), [_par(s) for s in sets], warped=True)
    xt, lse, lk, nk = (t.cpu().numpy() for t in SC.unpack(rec))
    warped = warped.cpu().numpy()
    assert not np.isnan(lse).any() and not np.isnan(lk).any()
    used = 0
    for r in range(R):
        xr = x[r].numpy()
        # x_tok: the logit as it stands, exact; NaN outside the vocabulary
        if 0 <= toks[r] < V:
            assert xt[r] == xr[toks[r]] or (np.isnan(xr[toks[r]]) and np.isnan(xt[r])), (r, xt[r], xr[toks[r]])
        else:
            assert np.isnan(xt[r]), (r, toks[r], xt[r])
        want = _lse64(xr)
        print(f"row {r} set {sets[r]}: lse {lse[r]!r} vs {want!r} (tol {_tol(xr):.2e}); lse_kept {lk[r]!r}, n_kept {nk[r]}")
        assert (lse[r] == NEG) if want == NEG else abs(float(lse[r]) - want) <= _tol(xr), (r, lse[r], want)
        if sets[r] is None:          # greedy: the row itself, lse again, every column
            assert np.array_equal(warped[r], xr) and lk[r] == lse[r] and nk[r] == V
            continue
        if not np.isfinite(xr).any():          # a sampled row of -inf: nothing has mass
            assert lk[r] == NEG and nk[r] == 0 and np.all(warped[r] == NEG)
            continue
        T, k, p = sets[r]
        xT = (xr / np.float32(T)).astype(np.float32)          # the sampler's fp32 division
        kept = np.isfinite(warped[r])
        assert int(kept.sum()) == nk[r], (r, int(kept.sum()), nk[r])          # the finite pattern and the record agree
        assert np.array_equal(warped[r][kept], xT[kept]) and np.all(warped[r][~kept] == NEG)
        ref = np.isfinite(S.warp(xr, T, k, p))
        diff = np.nonzero(kept != ref)[0]
        if diff.size:
            lo = np.isfinite(S.warp(xr, T, k, max(1e-6, p - 1e-5)))
            hi = np.isfinite(S.warp(xr, T, k, min(1.0, p + 1e-5)))
            assert p < 1.0 and diff.size <= 1 and np.all(lo[diff] != hi[diff]), f"row {r}: kept set differs from the oracle's at {diff.tolist()}"
            used += int(diff.size)
            continue
        want = _lse64(xT[ref])
        assert (lk[r] == NEG) if want == NEG else abs(float(lk[r]) - want) <= _tol(xT), (r, lk[r], want)
    return used


# ---- 1. the op against float64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1000, 32000, 32001, 40000])          # fewer columns than threads; ragged last batch; 40000 > 32768: the loop form
@pytest.mark.parametrize("R", [1, 3, 64])
def test_op_equals_float64(R, V):
    from vz_hip import binding as B
    from vz_hip import scores as SC
    x = _logits(R, V, seed=V + R)
    g = np.random.RandomState(V + R)
    sets = [None if r % 7 == 6 else _ORACLE_SETS[r % 7] for r in range(R)]          # the six sets, every seventh row greedy
    toks = [int(x[r].argmax()) if r % 2 == 0 else int(g.randint(V)) for r in range(R)]
    if R == 1:
        sets = [_ORACLE_SETS[1]]
        assert _check(x, [None], toks) == 0          # the same row, greedy
    if R == 3:
        sets = [None, _ORACLE_SETS[5], _ORACLE_SETS[2]]
        x[1, 11] += 200.0                            # (0.7, 5, 0.3) and a +200 outlier: the kept set is one token
        toks[1], toks[2] = 11, V - 1                 # a chosen id equal to cols - 1
    if R == 64:
        o = torch.argsort(x[8], descending=True)
        x[8, o[50]] = x[8, o[49]]                    # set 0 (top_k 50): an exact tie at the k-th value, both stay
        sets[8] = _ORACLE_SETS[0]
        x[9, 11] += 200.0
        sets[9], toks[9] = _ORACLE_SETS[5], 11
        x[10] = NEG                                  # a row of -inf, sampled and greedy
        x[11] = NEG
        sets[10], sets[11] = _ORACLE_SETS[1], None
        x[12, ::3] = NEG                             # -inf scattered in a row, sampled and greedy
        x[13, ::3] = NEG
        sets[12], sets[13], toks[12], toks[13] = _ORACLE_SETS[2], None, 1, 3
        toks[14] = V - 1
        toks[15], toks[16] = V, -1                   # outside [0, cols): NaN, nothing is read
    used = _check(x, sets, toks)
    assert used <= 3, f"{used} boundary tokens"
    rec = B.token_scores(x.cuda(), torch.tensor(toks, dtype=torch.int32).cuda(), [_par(s) for s in sets])
    xt, lse, lk, nk = (t.cpu() for t in SC.unpack(rec))
    if R == 3:
        assert int(nk[1]) == 1 and float(lk[1]) == float(xt[1] / torch.tensor(0.7, dtype=torch.float32))          # exactly x_tok / T
    if R == 64:
        assert int(nk[8]) == 51 and int(nk[9]) == 1 and float(lk[9]) == float(xt[9] / torch.tensor(0.7, dtype=torch.float32))
        assert float(lse[10]) == NEG and float(lk[10]) == NEG and int(nk[10]) == 0 and float(lse[11]) == NEG and float(lk[11]) == NEG
        assert bool(torch.isnan(xt[15])) and bool(torch.isnan(xt[16])) and float(xt[14]) == float(x[14, V - 1])
    # a second run gives the same bits, and so does the launch without the warped rows
    again = B.token_scores(x.cuda(), torch.tensor(toks, dtype=torch.int32).cuda(), [_par(s) for s in sets], warped=True)[0]
    assert torch.equal(again.view(torch.int32), rec.view(torch.int32))


# ---- 2. the kept set at the top-p boundary -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1000, 32000, 32001, 40000])
def test_kept_set_is_the_samplers(V):
    """x = randn(24, V, seed = V + 1) * 2.5, row r by set r % 6 (the inputs of tests/test_sample_rows_gpu.py::test_op_equals_oracle): the
    oracle alone has 0 / 2 / 0 / 1 tokens in all whose membership differs between warp(p - 1e-5) and warp(p + 1e-5), never two in a row -
    only those may differ, at most 3 per case."""
    x = _logits(24, V, seed=V + 1)
    sets = [_ORACLE_SETS[r % 6] for r in range(24)]
    used = _check(x, sets, [int(x[r].argmax()) for r in range(24)])
    print(f"V = {V}: {used} boundary tokens differ from the oracle")
    assert used <= 3


def test_op_refuses_bad_arguments():
    from vz_hip import binding as B
    from vz_hip.sample_rows import RowParams
    x = _logits(2, 1000, 1).cuda()
    ids = torch.zeros(2, dtype=torch.int32).cuda()
    for bad in (RowParams(True, 0.0, 50, 0.9, 0, 0), RowParams(True, 0.7, -1, 0.9, 0, 0), RowParams(True, 0.7, 50, 1.5, 0, 0)):
        with pytest.raises(ValueError):
            B.token_scores(x, ids, [RowParams(True, 0.7, 50, 0.9, 0, 0), bad])


# ---- the model the step, generate and stream tests share -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    """the 2-layer synthetic model of tests/test_sample_rows_gpu.py"""
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
    """whole tiles only and no row-count-dependent K slices: rows of different batches get the same bits (the setup of the stream tests)"""
    from vz_hip import binding as B
    with B.tuned(gemm256_streamk=0, splitk_mid=0):
        yield


def _prompt(n, seed):
    from vz_hip import synth
    return synth.synth_ids(n, 32000, image_pos=-1, seed=seed).unsqueeze(0)


def _padded(lens, seed0):
    S = max(lens)
    ids = torch.full((len(lens), S), 2, dtype=torch.long)
    mask = torch.zeros(len(lens), S, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = _prompt(n, seed0 + b)[0]
        mask[b, :n] = 1
    return ids, mask


# ---- 3. in the step, bit for bit -----------------------------------------------------------------------------------------------------
LENS = [9, 30, 17, 12, 25, 21]
STEPS, CAP = 12, 5


@pytest.fixture(scope="module")
def armed_rows(model):
    """the six rows' prefill, once: (first tokens, on the device)"""
    from vz_hip import binding as B
    eng = model.engine
    ids, _ = _padded(LENS, 80)
    _, last = eng.prefill(eng.embed_tokens(ids.to(model.device)), LENS)
    return B.argmax(last)


@pytest.mark.parametrize("mode", ["rows", "sampler", "proc"])
def test_step_records_equal_host_loop(model, armed_rows, mode):
    """12 steps of 6 rows with a ring of 5 steps (calls of 5, 5 and 2 steps: the ring wraps twice): the records, the warped rows and the
    raw rows of the replayed graph equal the op applied to the logits of a host-driven eager loop over the same tokens."""
    from vz_hip import binding as B
    from vz_hip import logits_proc as LP
    from vz_hip.sample_rows import GREEDY, RowParams
    eng = model.engine
    first = armed_rows
    cfg = None
    if mode == "rows":          # mixed greedy and sampled rows through the per-row table
        params = [RowParams(True, 0.9, 50, 0.95, 4242, 1), GREEDY.at(5), RowParams(True, 0.4, 5, 1.0, 77, 77), RowParams(True, 1.2, 0, 0.9, 31337, 3),
                  GREEDY.at(1), RowParams(True, 0.7, 20, 0.9, 5, 1)]
    elif mode == "sampler":     # the single-sampler tail: every row by the same parameters, taken by value
        params = [RowParams(True, 0.8, 40, 0.9, 99, 1)] * 6
    else:                       # greedy behind the logits processors
        params = [GREEDY] * 6
        cfg = LP.parse(1.3, 2, None, None, [])

    def arm(scores):
        if mode == "rows":
            eng.set_sampling_rows(params)
        if mode == "sampler":
            eng.set_sampling(True, 0.8, 40, 0.9, 99, first_counter=1)
        if cfg is not None:
            eng.set_logits_proc(cfg)
        eng.set_scores(*((CAP, 6, True, True) if scores else (None,)))
        eng.decode_begin(first, LENS, LENS)

    def disarm():
        eng.set_scores(None)
        eng.set_logits_proc(None)
        eng.set_sampling(False)
        eng.set_sampling_rows(None)

    try:
        arm(True)
        with pytest.raises(ValueError, match="cap_steps"):
            eng.decode_steps(CAP + 1)
        arm(True)
        ids, rec, warped, raw = [], [], [], []
        for n in (5, 5, 2):
            ids.append(eng.decode_steps(n).clone())
            r, w, x = eng.scores_steps(n)
            rec.append(r), warped.append(w), raw.append(x)
        assert eng.decode_mode()[0], "the scored steps did not run as a replayed graph"
        ids, rec, warped, raw = torch.cat(ids, 1), torch.cat(rec, 0), torch.cat(warped, 0), torch.cat(raw, 0)
        assert tuple(rec.shape) == (STEPS, 6, 4) and tuple(warped.shape) == (STEPS, 6, eng.cfg.vocab)
        arm(False)          # the recorder changes no id
        assert torch.equal(eng.decode_steps(STEPS), ids)
    finally:
        disarm()
    # the host-driven loop: eager steps with the raw logits handed back, the rows re-armed with the graph's tokens
    eng.decode_begin(first, LENS, LENS)
    hist = torch.zeros(6, STEPS + 1, dtype=torch.int32, device=model.device)
    hist[:, 0] = first
    differ = 0
    for t in range(STEPS):
        _, lg = eng.decode_steps(1, return_logits=True)
        x = lg[0].clone()
        if cfg is not None:          # the ids generated so far, the step's input token included
            B.logits_process(x, cfg, hist, torch.full((6,), t + 1, dtype=torch.int32, device=model.device))
            differ += int((x != lg[0]).sum())
        toks = ids[:, t].contiguous()
        want_rec, want_w = B.token_scores(x, toks, params, warped=True)
        assert torch.equal(rec[t].view(torch.int32), want_rec.view(torch.int32)), (mode, t, rec[t].tolist(), want_rec.tolist())
        assert torch.equal(warped[t], want_w), (mode, t)
        assert torch.equal(raw[t], lg[0]), (mode, t)
        hist[:, t + 1] = toks
        for r in range(6):
            eng.decode_set_row(r, int(toks[r]), LENS[r] + t + 1, LENS[r] + t + 1)
    if cfg is not None:
        assert differ > 0, "the processors changed no logit: the case shows nothing"


def test_recorder_refuses_the_beam_tail(model, armed_rows):
    eng = model.engine
    try:
        eng.set_scores(4, 3)
        eng.decode_begin(armed_rows[:3], LENS[:3], LENS[:3])
        eng.set_beam(True, 3, 1, [], LENS[:1], torch.zeros(3, device=model.device), torch.empty(1, 1, 6, 3, dtype=torch.int32, device=model.device))
        with pytest.raises(ValueError, match="step recorder"):
            eng.decode_steps(1)
    finally:
        eng.set_beam(False)
        eng.set_scores(None)


# ---- 4. generate() ---------------------------------------------------------------------------------------------------------------------
def _check_output(model, out, plain, T_div, eos):
    """the checks every scored generate() call shares; T_div = the temperature the rows were drawn at (1 = greedy)"""
    from vz_hip import scores as SC
    seq = out.sequences
    assert torch.equal(seq, plain)
    Bn, T = seq.shape
    assert len(out.scores) == T and len(out.logits) == T and tuple(out.scores[0].shape) == (Bn, model.engine.cfg.vocab)
    assert tuple(out.token_logprobs.shape) == (Bn, T) and out.token_logprobs.dtype == torch.float32
    mask = SC.behind_eos(seq, eos).cpu()
    lp, lpw = out.token_logprobs.cpu(), out.token_logprobs_warped.cpu()
    assert not bool(lp[mask].any()) and not bool(lpw[mask].any())
    hf = model.compute_transition_scores(seq, out.scores, normalize_logits=True).cpu()
    for t in range(T):
        sc, lg = out.scores[t].cpu().double(), out.logits[t].cpu().double()
        for b in range(Bn):
            if mask[b, t]:
                continue
            tok = int(seq[b, t])
            assert bool(torch.isfinite(sc[b, tok])), f"token {tok} of row {b} step {t} is filtered in its scores row"
            own = float(torch.log_softmax(lg[b], 0)[tok])          # the model's own distribution (no processors here: logits = the processed row)
            tol = 2e-5 + 2.0 ** -22 * float(lg[b].abs().max())
            assert abs(float(lp[b, t]) - own) <= tol, (b, t, float(lp[b, t]), own, tol)
            fin = sc[b][torch.isfinite(sc[b])]
            tolw = 2e-5 + 2.0 ** -22 * float(fin.abs().max())
            assert abs(float(lpw[b, t]) - float(torch.log_softmax(sc[b], 0)[tok])) <= tolw
            assert abs(float(lpw[b, t]) - float(hf[b, t])) <= tolw, (b, t, float(lpw[b, t]), float(hf[b, t]))
            if T_div == 1.0:
                assert torch.equal(out.scores[t][b], out.logits[t][b]) and float(lp[b, t]) == float(lpw[b, t])
    return mask


def test_generate_greedy_batch(model):
    ids, mask = _padded([9, 30, 17], 60)
    kw = dict(input_ids=ids, attention_mask=mask, do_sample=False, max_new_tokens=10, sync_every=4)
    free = model.generate(eos_token_id=[], **kw)
    eos = int(free[1, 3])          # a token row 1 emits mid-run
    plain = model.generate(eos_token_id=[eos], **kw)
    assert eos in plain[1].tolist() and plain.shape[1] > 4
    out = model.generate(eos_token_id=[eos], return_dict_in_generate=True, output_scores=True, output_logits=True, output_logprobs=True, **kw)
    from transformers.generation.utils import GenerateDecoderOnlyOutput
    assert isinstance(out, GenerateDecoderOnlyOutput)
    m = _check_output(model, out, plain, 1.0, {eos})
    assert bool(m[1].any()), "no position behind an eos in the batch"
    # as in HF: without return_dict_in_generate the keywords return the tensor; return_dict_in_generate alone returns the object
    assert torch.equal(model.generate(eos_token_id=[eos], output_scores=True, output_logprobs=True, **kw), plain)
    bare = model.generate(eos_token_id=[eos], return_dict_in_generate=True, **kw)
    assert torch.equal(bare.sequences, plain) and bare.scores is None and bare.token_logprobs is None
    # the cheap form: log-probs only, the same bits
    cheap = model.generate(eos_token_id=[eos], return_dict_in_generate=True, output_logprobs=True, **kw)
    assert cheap.scores is None and cheap.logits is None and torch.equal(cheap.token_logprobs, out.token_logprobs)


def test_generate_sampled_n(model, pinned_routes):
    ids = _prompt(21, 90)
    kw = dict(input_ids=ids, do_sample=True, temperature=0.7, top_k=20, top_p=0.9, seed=4242, num_return_sequences=3, max_new_tokens=9, eos_token_id=[],
              sync_every=4)
    plain = model.generate(**kw)
    out = model.generate(return_dict_in_generate=True, output_scores=True, output_logits=True, output_logprobs=True, **kw)
    assert tuple(plain.shape) == (3, 9)
    _check_output(model, out, plain, 0.7, set())
    assert all(int(torch.isfinite(s).sum(1).max()) <= 20 for s in out.scores)
    # the serial sampled loop (two prompts, one sequence each): row b is the single call under seed + b
    two, m2 = _padded([21, 13], 90)
    kw2 = dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.9, seed=7, max_new_tokens=6, eos_token_id=[], return_dict_in_generate=True, output_logprobs=True)
    both = model.generate(input_ids=two, attention_mask=m2, **kw2)
    a = model.generate(input_ids=two[0:1], **kw2)
    b = model.generate(input_ids=two[1:2, :13], **{**kw2, "seed": 8})
    assert torch.equal(both.sequences, torch.cat([a.sequences, b.sequences])) and tuple(both.token_logprobs.shape) == (2, 6)
    assert torch.equal(both.token_logprobs, torch.cat([a.token_logprobs, b.token_logprobs]))
    assert torch.equal(both.token_logprobs_warped, torch.cat([a.token_logprobs_warped, b.token_logprobs_warped]))


@pytest.mark.parametrize("sample", [False, True])
def test_streamer_path_gives_the_same_records(model, sample):
    """_generate_one with a stopping criterion (one step in flight, the token ring; the records in a device ring of max_new slots, read
    once at the end) against the same call without one"""
    ids = _prompt(17, 33)
    kw = dict(input_ids=ids, max_new_tokens=11, eos_token_id=[], sync_every=4, return_dict_in_generate=True, output_scores=True, output_logits=True,
              output_logprobs=True, repetition_penalty=1.2)
    if sample:
        kw.update(do_sample=True, temperature=0.8, top_k=30, top_p=0.95, seed=5)
    calls = []

    def crit(seq, scores):
        calls.append(seq.shape[1])
        return len(calls) >= 8          # stops after the eighth token

    a = model.generate(**kw)
    b = model.generate(stopping_criteria=[crit], **kw)
    assert calls == list(range(1, 9)) and tuple(b.sequences.shape) == (1, 8) and torch.equal(b.sequences, a.sequences[:, :8])
    assert torch.equal(b.token_logprobs, a.token_logprobs[:, :8]) and torch.equal(b.token_logprobs_warped, a.token_logprobs_warped[:, :8])
    assert len(b.scores) == 8 and all(torch.equal(b.scores[t], a.scores[t]) and torch.equal(b.logits[t], a.logits[t]) for t in range(8))
    # the records see the processed logits, `logits` the unprocessed ones: the penalty moves the logits of the ids generated so far
    t0 = int(a.sequences[0, 0])
    assert float(a.scores[1][0, t0]) != float(a.logits[1][0, t0]) or sample
    if not sample:
        x = a.logits[1][0, t0]
        assert float(a.scores[1][0, t0]) == float(x / 1.2 if x > 0 else x * 1.2)
    assert bool((a.token_logprobs < 0).all())


def test_recorder_off_is_free(model, armed_rows):
    eng = model.engine
    ids = _prompt(14, 41)
    kw = dict(input_ids=ids, do_sample=False, max_new_tokens=8, eos_token_id=[])
    before = model.generate(**kw)
    scored = model.generate(return_dict_in_generate=True, output_scores=True, output_logprobs=True, **kw)
    assert torch.equal(scored.sequences, before)
    assert torch.equal(model.generate(**kw), before) and torch.equal(model.generate(**kw), before)
    # the graph key: the same steps into the same buffer - armed captures once, back to the unscored key once more, then nothing
    buf = torch.empty(3, 4, dtype=torch.int32, device=model.device)

    def steps():
        eng.decode_begin(armed_rows[:3], LENS[:3], LENS[:3])
        out = eng.decode_steps(4, out=buf).clone()
        return out, eng.decode_info()[1]

    plain, c0 = steps()
    same, c1 = steps()
    assert c1 == c0 and torch.equal(same, plain)
    try:
        eng.set_scores(4, 3)
        on, c2 = steps()
        on2, c3 = steps()
    finally:
        eng.set_scores(None)
    off, c4 = steps()
    off2, c5 = steps()
    assert (c2, c3, c4, c5) == (c0 + 1, c0 + 1, c0 + 2, c0 + 2), (c0, c1, c2, c3, c4, c5)
    assert all(torch.equal(t, plain) for t in (on, on2, off, off2))


def test_generate_beams_and_prompt_lookup(model):
    from transformers.generation.utils import GenerateBeamDecoderOnlyOutput
    ids = _prompt(19, 52)
    kw = dict(input_ids=ids, num_beams=3, max_new_tokens=8, eos_token_id=[])
    plain = model.generate(**kw)
    out = model.generate(return_dict_in_generate=True, **kw)
    assert isinstance(out, GenerateBeamDecoderOnlyOutput) and torch.equal(out.sequences, plain)
    # sequences_scores = what the host-side beam bookkeeping holds at the end (vz_hip.beam.BeamReplay.best: HF's finished hypotheses, best
    # first), captured during the call: two prompts, the two best of three beams each, prompt-major
    from vz_hip import beam as BM
    finals, best = [], BM.BeamReplay.best

    def capture(self, n):
        finals.append(best(self, n))
        return finals[-1]

    two, mask = _padded([19, 11], 52)
    BM.BeamReplay.best = capture
    try:
        got = model.generate(input_ids=two, attention_mask=mask, num_beams=3, num_return_sequences=2, max_new_tokens=8, eos_token_id=[],
                             return_dict_in_generate=True)
        one = model.generate(return_dict_in_generate=True, **kw)
    finally:
        BM.BeamReplay.best = best
    assert len(finals) == 3 and [len(f) for f in finals] == [2, 2, 1]
    hyps = finals[0] + finals[1]
    assert tuple(got.sequences.shape) == (4, 8) and got.sequences_scores.dtype == torch.float32
    assert got.sequences.tolist() == [t for t, _ in hyps], "sequences are not the finished hypotheses, prompt-major and best first"
    assert got.sequences_scores.cpu().tolist() == [float(torch.tensor(sc, dtype=torch.float32)) for _, sc in hyps]
    assert all(hyps[i][1] >= hyps[i + 1][1] for i in (0, 2))
    assert one.sequences.tolist() == [finals[2][0][0]] == plain.tolist() and float(one.sequences_scores[0]) == float(torch.tensor(finals[2][0][1]))
    assert torch.equal(one.sequences_scores, out.sequences_scores)
    for k in ("output_scores", "output_logits", "output_logprobs"):
        with pytest.raises(NotImplementedError):
            model.generate(return_dict_in_generate=True, **{k: True}, **kw)
    # prompt lookup: with a score output the call takes the plain greedy path - the same ids
    rep = torch.cat([ids, ids], 1)
    kw = dict(input_ids=rep, do_sample=False, max_new_tokens=8, eos_token_id=[], prompt_lookup_num_tokens=4)
    spec = model.generate(**kw)
    out = model.generate(return_dict_in_generate=True, output_logprobs=True, **kw)
    assert torch.equal(out.sequences, spec) and tuple(out.token_logprobs.shape) == (1, 8) and bool((out.token_logprobs < 0).all())


# ---- 5. generate_stream ----------------------------------------------------------------------------------------------------------------
def test_stream_logprobs(model, pinned_routes):
    """four requests on 2 rows, two of them with logprobs=True (one greedy, one sampled): those yield 3-tuples whose log-probs equal
    generate(..., output_logprobs=True) of the same request alone bit for bit, the others the 2-tuples with the ids of a call in which
    nobody asks.  admit = 0: every request is prefilled alone, as generate() prefills it (a prefill shared by several admissions takes
    other GEMM kernels for its rows: equally accurate, other bits); the 1-row and the 2-row decode steps give a row the same bits."""
    lens, budgets = [9, 30, 17, 12], [7, 10, 6, 9]
    samp = [None, dict(do_sample=True, temperature=0.9, top_p=0.95, seed=11), dict(do_sample=True, temperature=0.5, top_k=5, seed=12), None]
    reqs = [{"input_ids": _prompt(n, 70 + i), "max_new_tokens": b, **(samp[i] or {})} for i, (n, b) in enumerate(zip(lens, budgets))]
    nobody = {i: v for i, *v in model.generate_stream(reqs, eos_token_id=[], rows=2, sync_every=4, admit=0)}
    assert all(len(v) == 1 for v in nobody.values())
    flagged = [dict(r, logprobs=(i in (0, 1))) for i, r in enumerate(reqs)]
    got = {i: v for i, *v in model.generate_stream(flagged, eos_token_id=[], rows=2, sync_every=4, admit=0)}
    assert sorted(got) == [0, 1, 2, 3]
    for i in range(4):
        assert len(got[i]) == (2 if i in (0, 1) else 1), f"request {i}: a {1 + len(got[i])}-tuple"
        assert torch.equal(got[i][0], nobody[i][0]) and got[i][0].numel() == budgets[i]
    common = dict(eos_token_id=[], return_dict_in_generate=True, output_logprobs=True)
    a = model.generate(input_ids=reqs[0]["input_ids"], max_new_tokens=budgets[0], **common)
    b = model.generate(input_ids=reqs[1]["input_ids"], max_new_tokens=budgets[1], **samp[1], **common)
    for i, alone in ((0, a), (1, b)):
        ids, lp = got[i]
        assert lp.dtype == torch.float32 and tuple(lp.shape) == (budgets[i],)
        assert ids.tolist() == alone.sequences[0].tolist()
        assert torch.equal(lp, alone.token_logprobs[0].cpu()), (i, lp.tolist(), alone.token_logprobs[0].tolist())
