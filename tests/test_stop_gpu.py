"""The stop matcher (csrc/stop.hip: stop_match_kernel) and what is built on it: the operator against HF's `StopStringCriteria` and this
package's `KeywordsStoppingCriteria` run on the CPU over the same id streams ("the first index at which the criterion returns True on the
prefix" is the expected `at`; every comparison is between integers), the matcher inside the decode step, and generate() /
generate_stream with stop strings and keyword stops decided on the device."""
import numpy as np
import pytest
import torch

import stop_ref as R

pytestmark = pytest.mark.gpu


def _hf(tok, strings):
    from transformers.generation.stopping_criteria import StopStringCriteria
    return StopStringCriteria(tok, strings)


def _run_op(plan, streams, per):
    """streams [rows, T] (long, host) through vz_op_stop_match, one id per row per call, `per` rows per launch: at after every step [T, rows]"""
    from vz_hip import binding as B
    rows, T = streams.shape
    tabs = B.StopTables(plan, "cuda")
    state = B.stop_state(rows, "cuda")
    dev = streams.to(torch.int32).cuda()
    ats = []
    for t in range(T):
        col = dev[:, t].contiguous()
        for r0 in range(0, rows, per):
            B.stop_match(state[r0:r0 + per], col[r0:r0 + per], tabs, reset=(t == 0))
        ats.append(state[:, 1].clone())
    assert state[:, 0].tolist() == [min(T, int(a) + 1) if a >= 0 else T for a in ats[-1].tolist()]      # a stopped row counts no further
    return torch.stack(ats).cpu().to(torch.long)


def _expect(first, T):
    """first hits [rows] -> what `at` shows after every step [T, rows]: -1 until the hit, then the hit for good (sticky)"""
    t = torch.arange(T).view(T, 1)
    return torch.where((first.view(1, -1) >= 0) & (first.view(1, -1) <= t), first.view(1, -1).expand(T, -1), torch.full((T, first.numel()), -1))


# ---- 1. the operator against HF ---------------------------------------------------------------------------------------------------------
SCRIPTED = {("<|", "user", "|>"): 2, ("<", "|", "u", "s", "e", "r", "|", ">"): 7, ("<", "|user|", ">\n"): 2, ("<|", "us", "e", "r|>x"): 3,
            ("<", "/", "s", ">"): 3, ("</", "s>"): 1, ("</s>",): 0, ("ab", "ab", "ab"): 2, ("aba", "bab"): 1, ("aa", "bab", "ab"): 2,
            ("ab", "ab", "abc"): 2, ("abcdef",): 0}
NEAR = [("ab", "ab", "x", "ab"), ("<|", "user", "|", "x", ">"), ("</", "x", "s>"), ("ab", "ab", "a"), ("<", "|", "u", "s", "e", "r", "|", "y", ">")]


@pytest.fixture(scope="module")
def small():
    """the stand-in tokenizer, HF's criterion over it, the plan, and the scripted + random id streams with HF's own first hits"""
    from vz_hip import stop as ST
    tok = R.small_tokenizer()
    crit = _hf(tok, R.STOPS)
    plan, host = ST.parse(R.STOPS, tok, None)
    assert host is None
    pad = tok.vocab["y"]
    rows, want = [], []
    for toks, hit in SCRIPTED.items():
        rows.append(tok.ids("x", "yz", *toks))
        want.append(hit + 2)
    for toks in NEAR:
        rows.append(tok.ids("x", "yz", *toks))
        want.append(-1)
    rows.append(tok.ids("x", "yz") + [999] + tok.ids("</s>"))                 # an id outside the vocabulary in front of a stop: still stops
    want.append(3)
    rows.append(tok.ids("x", "yz", "</") + [999] + tok.ids("s>"))             # ... between the two halves of one: does not
    want.append(-1)
    T = max(len(r) for r in rows) + 2
    scripted = torch.tensor([r + [pad] * (T - len(r)) for r in rows], dtype=torch.long)
    rng = np.random.RandomState(1)
    quiet, V = np.array(tok.ids(*R.QUIET)), len(R.VOCAB)
    rnd = np.empty((96, 40), dtype=np.int64)
    rnd[:32] = quiet[rng.randint(0, len(quiet), (32, 40))]
    rnd[32:64] = rng.randint(0, V, (32, 40))
    mix = rng.rand(32, 40) < 0.07
    rnd[64:] = np.where(mix, rng.randint(0, V, (32, 40)), quiet[rng.randint(0, len(quiet), (32, 40))])
    rnd = torch.from_numpy(rnd)
    return dict(tok=tok, crit=crit, plan=plan, scripted=scripted, scripted_want=torch.tensor(want), random=rnd,
                scripted_hf=R.first_hits_batch(crit, scripted), random_hf=R.first_hits_batch(crit, rnd))


def test_inputs_exercise_every_stop_string(small):
    """on HF's own result: the scripted rows hit where the table says, enough random rows stop and enough never do, and every stop string
    fires somewhere - otherwise the inputs are wrong, not the kernel"""
    assert torch.equal(small["scripted_hf"], small["scripted_want"])
    hf = small["random_hf"]
    print("random rows stopped per third:", [int((hf[i:i + 32] >= 0).sum()) for i in (0, 32, 64)])
    total = hf.numel() + small["scripted_hf"].numel()
    stopped = int((hf >= 0).sum()) + int((small["scripted_hf"] >= 0).sum())
    assert stopped >= total / 4 and total - stopped >= total / 4
    fired = set()
    singles = {s: _hf(small["tok"], [s]) for s in R.STOPS}
    for streams, hits in ((small["scripted"], small["scripted_hf"]), (small["random"], hf)):
        for row, h in zip(streams.tolist(), hits.tolist()):
            if h >= 0:
                fired |= {s for s, c in singles.items() if bool(c(torch.tensor([row[:h + 1]]), None).all())}
    assert fired == set(R.STOPS), fired


@pytest.mark.parametrize("per", [1, 5])
@pytest.mark.parametrize("which", ["scripted", "random"])
def test_op_equals_hf(small, which, per):
    streams, want = small[which], small[which + "_hf"]
    got = _run_op(small["plan"], streams, per)
    exp = _expect(want, streams.shape[1])
    bad = (got != exp).any(dim=0).nonzero().view(-1).tolist()
    assert not bad, [(r, streams[r].tolist(), got[:, r].tolist(), int(want[r])) for r in bad[:3]]


# ---- 2. id sequences ----------------------------------------------------------------------------------------------------------------------
def test_id_sequences(small):
    from vis_zephyr.model.mm_utils import KeywordsStoppingCriteria
    from vz_hip import stop as ST
    tok = small["tok"]
    x, y, z, ab = tok.ids("x", "y", "z", "ab")
    k2 = KeywordsStoppingCriteria(["xy"], tok, torch.zeros(1, 3, dtype=torch.long))          # two ids, start_length 3
    k1 = KeywordsStoppingCriteria(["ab"], tok, torch.zeros(1, 0, dtype=torch.long))          # one id
    for crit, rows in ((k2, [[z, z, x, y, z, z, z, z],          # the keyword at generated indices 2..3: not yet comparable, no stop
                             [z, z, z, x, y, z, x, y],          # at 3..4: stops at 4
                             [x, y, x, y, x, y, z, z]]),        # ... the first occurrence that is comparable: 4..5
                       (k1, [[z, z, ab, z, ab, z, z, z], [ab, z, z, z, z, z, z, z], [z, z, z, z, z, z, z, z]])):
        plan, host = ST.parse(None, None, [crit])
        assert host is None
        streams = torch.tensor(rows, dtype=torch.long)
        want = torch.tensor([R.first_hit(crit, r) for r in rows])
        assert want.tolist() == ([-1, 4, 5] if crit is k2 else [2, 0, -1])
        assert torch.equal(_run_op(plan, streams, 5), _expect(want, streams.shape[1]))


def test_both_rules_the_earlier_hit_wins(small):
    from vis_zephyr.model.mm_utils import KeywordsStoppingCriteria
    from vz_hip import stop as ST
    tok = small["tok"]
    kw = KeywordsStoppingCriteria(["yz"], tok, torch.zeros(1, 0, dtype=torch.long))
    plan, host = ST.parse(["abc"], tok, [kw])
    assert host is None and plan.n_str == 1 and len(plan.seqs) == 1
    rows = [tok.ids("x", "x", "yz", "x", "a", "bc", "x"), tok.ids("x", "ab", "cd", "x", "x", "yz", "x"), tok.ids("x", "x", "x", "x", "x", "x", "x")]
    both = lambda ids, scores: bool(kw(ids, scores)) or bool(_hf(tok, ["abc"])(ids, scores).all())      # noqa: E731
    want = torch.tensor([R.first_hit(both, r) for r in rows])
    assert want.tolist() == [2, 2, -1]
    assert torch.equal(_run_op(plan, torch.tensor(rows), 1), _expect(want, 7))


def test_sixteen_sequences_of_thirty_two_ids():
    from vz_hip import stop as ST
    g = torch.Generator().manual_seed(3)
    seqs = torch.randint(5, 32000, (16, 32), generator=g)
    crit = R.keyword_criterion(seqs.tolist(), 0)
    plan, host = ST.parse(None, None, [crit])
    assert host is None and len(plan.seqs) == 16
    rows = []
    for k in range(16):                       # row k: k + 1 quiet ids, then sequence k
        rows.append([3] * (k + 1) + seqs[k].tolist() + [3] * (17 - k))
    near = [3] * 4 + seqs[5].tolist() + [3] * 14
    near[4] = 4                               # the oldest id of the sequence is another one: the whole comparison runs and fails
    rows.append(near)
    share = seqs[7].tolist()
    rows.append([3] * 2 + share[:31] + [int(seqs[9, 31])] + [3] * 16)          # sequence 7 with the newest id of sequence 9: neither
    streams = torch.tensor(rows, dtype=torch.long)
    want = torch.tensor([R.first_hit(crit, r) for r in rows])
    assert want.tolist() == [k + 32 for k in range(16)] + [-1, -1]
    assert torch.equal(_run_op(plan, streams, 5), _expect(want, streams.shape[1]))


# ---- 3. the window ------------------------------------------------------------------------------------------------------------------------
def test_window_of_sixty_four_tokens():
    """a 64-character stop string matched by 64 one-character tokens (a 64-token walk over 63 staged table rows), by two 32-character
    tokens, and by a row whose 70 generated tokens wrap the ring; one wrong character at the far end of the window never matches"""
    from vz_hip import stop as ST
    rng = np.random.RandomState(7)
    s = "".join(rng.permutation(list("abcdefgh" * 8)))
    tok = R.SelfTokenizer(["abcdef", "x"] + list("abcdefgh") + [s[:32], s[32:]])
    crit = _hf(tok, [s])
    plan, host = ST.parse([s], tok, None)
    assert host is None and plan.window == 64 and plan.max_pos <= ST.MAX_POS
    x = tok.vocab["x"]
    chars = tok.ids(*s)
    wrong = list(chars)
    wrong[0] = tok.vocab["a" if s[0] != "a" else "b"]
    rows = [chars + [x] * 6, tok.ids(s[:32], s[32:]) + [x] * 68, [x] * 6 + chars, wrong + [x] * 6, [x] * 3 + tok.ids(s[:32]) + chars[32:] + [x] * 34,
            chars[:32] + tok.ids(s[32:]) + [x] * 37]
    streams = torch.tensor(rows, dtype=torch.long)
    want = R.first_hits_batch(crit, streams)
    assert want.tolist() == [63, 1, 69, -1, 35, 32]
    assert torch.equal(_run_op(plan, streams, 5), _expect(want, 70))


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def wide():
    """the stand-in tokenizer sized to the fixture's vocabulary: token i decodes to a unique 7-character string"""
    return R.fixed_width_tokenizer(32000)


@pytest.fixture()
def pinned_routes():
    """whole tiles only and no row-count-dependent K slices: rows of different batches get the same bits (the setup of
    tests/test_stages_gpu.py::test_continuous_batching_matches_static_batches)"""
    from vz_hip import binding as B
    with B.tuned(gemm256_streamk=0, splitk_mid=0):
        yield


@pytest.fixture()
def armed(model, monkeypatch):
    """the plans Engine.set_stop was armed with during the test (the route a call took)"""
    seen = []
    real = model.engine.set_stop

    def spy(plan=None):
        if plan is not None:
            seen.append(plan)
        return real(plan)

    monkeypatch.setattr(model.engine, "set_stop", spy)
    return seen


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


def _cut(free, crit, pad):
    """the no-stop rows `free` [rows, T], each cut at HF's first hit on the CPU (inclusive) and padded; the call ends with the last row"""
    rows = free.tolist()
    hits = [R.first_hit(crit, r) for r in rows]
    T = max(h + 1 if h >= 0 else len(r) for h, r in zip(hits, rows))
    out = torch.full((len(rows), T), pad, dtype=torch.long)
    for b, (h, r) in enumerate(zip(hits, rows)):
        keep = r[:h + 1] if h >= 0 else r
        out[b, :min(T, len(keep))] = torch.tensor(keep[:T])
    return out, hits


def test_generate_stop_strings_one_sequence(model, wide, armed):
    """(a) and (b): one greedy sequence stops on a string of its own text, on the device, through HF's keywords and through a
    KeywordsStoppingCriteria; the host path gives the same ids.  On the parent commit the first call returns all 24 tokens."""
    from vis_zephyr.model.mm_utils import KeywordsStoppingCriteria
    ids = _prompt(14, 41)
    kw = dict(input_ids=ids, do_sample=False, max_new_tokens=24, eos_token_id=[])
    free = model.generate(**kw)[0].tolist()
    assert len(free) == 24 and not armed
    s = wide.text(free[9:11])
    crit = _hf(wide, [s])
    hit = R.first_hit(crit, free)
    print("tokens", free, "stop string", repr(s), "HF's first hit", hit)
    assert hit == 10
    got = model.generate(stop_strings=[s], tokenizer=wide, **kw)
    assert got[0].tolist() == free[:11] and len(armed) == 1 and armed[0].n_str == 1
    host = model.generate(stopping_criteria=[crit], device_stop=False, **kw)
    assert torch.equal(host, got) and len(armed) == 1
    assert torch.equal(model.generate(stopping_criteria=[crit], **kw), got) and len(armed) == 2           # HF's criterion object: its tables
    assert torch.equal(model.generate(stop_strings=s, tokenizer=wide, sync_every=3, **kw), got)              # a sync in front of the hit
    with pytest.raises(ValueError, match="tokenizer"):
        model.generate(stop_strings=[s], **kw)
    # (b) the reference's criterion, no streamer: the keyword's ids, compared from start_length on
    for start in (0, 10):
        kc = KeywordsStoppingCriteria([s], wide, torch.zeros(1, start, dtype=torch.long))
        want = R.first_hit(kc, free)
        assert want == (10 if start == 0 else -1) and kc.keyword_ids[0].tolist() == free[9:11]
        n0 = len(armed)
        got = model.generate(stopping_criteria=[kc], **kw)
        assert got[0].tolist() == (free[:want + 1] if want >= 0 else free) and len(armed) == n0 + 1 and armed[-1].seqs == [(free[9:11], start)]
    # the first token stops
    first = wide.text(free[:1])
    assert model.generate(stop_strings=[first], tokenizer=wide, **kw)[0].tolist() == free[:1]
    # prompt lookup with a device stop: the plain greedy path, the same ids
    assert model.generate(stop_strings=[s], tokenizer=wide, prompt_lookup_num_tokens=4, **kw)[0].tolist() == free[:11]
    # the log-probs behind a stop are handled as behind eos
    a = model.generate(return_dict_in_generate=True, output_logprobs=True, **kw)
    b = model.generate(return_dict_in_generate=True, output_logprobs=True, stop_strings=[s], tokenizer=wide, **kw)
    assert b.sequences[0].tolist() == free[:11] and torch.equal(b.token_logprobs, a.token_logprobs[:, :11])


def test_generate_batch_stops_per_row(model, wide, pinned_routes, armed):
    """(c): three prompts of different lengths decode together; every row is cut at HF's first hit and padded, the call ends once all
    rows are done"""
    ids, mask = _padded([9, 30, 17], 60)
    kw = dict(input_ids=ids, attention_mask=mask, do_sample=False, max_new_tokens=24, eos_token_id=[], sync_every=4)
    free = model.generate(**kw).cpu()
    assert tuple(free.shape) == (3, 24)
    stops = [wide.text(free[0, 5:7].tolist()), wide.text(free[1, 12:14].tolist()), wide.text(free[2, 8:9].tolist())]
    crit = _hf(wide, stops)
    want, hits = _cut(free, crit, 2)
    print("first hits", hits)
    assert all(0 <= h < 23 for h in hits) and want.shape[1] == max(hits) + 1
    got = model.generate(stop_strings=stops, tokenizer=wide, **kw)
    assert torch.equal(got.cpu(), want) and len(armed) == 1
    # one row never stops: the batch runs to the token budget, the other rows show pads behind their stops
    crit2 = _hf(wide, stops[:2])
    want2, hits2 = _cut(free, crit2, 2)
    if hits2[2] < 0:
        assert want2.shape[1] == 24
    assert torch.equal(model.generate(stop_strings=stops[:2], tokenizer=wide, **kw).cpu(), want2)
    # positions behind a stop: log-probs as behind eos
    a = model.generate(return_dict_in_generate=True, output_logprobs=True, **kw)
    b = model.generate(return_dict_in_generate=True, output_logprobs=True, stop_strings=stops, tokenizer=wide, **kw)
    T = want.shape[1]
    for r, h in enumerate(hits):
        assert torch.equal(b.token_logprobs[r, :h + 1], a.token_logprobs[r, :h + 1]) and not bool(b.token_logprobs[r, h + 1:T].any())


def test_generate_samples_with_stops(model, wide, armed):
    """(d): num_return_sequences with a stop no longer raises; every sample is cut at its own first hit"""
    ids = _prompt(14, 43)
    kw = dict(input_ids=ids, do_sample=True, temperature=0.8, top_k=20, num_return_sequences=3, seed=1234, max_new_tokens=20, eos_token_id=[],
              sync_every=4)
    free = model.generate(**kw).cpu()
    assert tuple(free.shape) == (3, 20)
    stops = [wide.text(free[r, 4 + 3 * r:6 + 3 * r].tolist()) for r in range(3)]
    want, hits = _cut(free, _hf(wide, stops), 2)
    assert all(0 <= h < 19 for h in hits)
    got = model.generate(stop_strings=stops, tokenizer=wide, **kw)
    assert torch.equal(got.cpu(), want) and len(armed) == 1
    kc = R.keyword_criterion([free[0, 4:6].tolist()], 0)
    want, _ = _cut(free, kc, 2)
    assert torch.equal(model.generate(stopping_criteria=[kc], **kw).cpu(), want)
    with pytest.raises(NotImplementedError):
        model.generate(stopping_criteria=[kc, lambda i, s: False], **kw)


def test_generate_stream_with_call_level_stops(model, wide, pinned_routes):
    """(e): five requests on two rows; each yielded sequence equals that request's no-stop sequence cut at its first hit"""
    reqs = [dict(input_ids=_prompt(n, 70 + i), max_new_tokens=m) for i, (n, m) in enumerate([(9, 14), (21, 9), (13, 16), (30, 12), (17, 10)])]
    free = {i: t.tolist() for i, t in model.generate_stream(reqs, eos_token_id=[], rows=2, sync_every=4)}
    assert sorted(free) == list(range(5))
    stops = [wide.text(free[0][5:7]), wide.text(free[2][0:1]), wide.text(free[4][7:9])]
    seq = free[3][3:6]
    crit = _hf(wide, stops)
    ks = R.keyword_criterion([seq], 0)
    both = lambda ids, scores: bool(ks(ids, scores)) or bool(crit(ids, scores).all())      # noqa: E731
    got = {i: t.tolist() for i, t in model.generate_stream(reqs, eos_token_id=[], rows=2, sync_every=4, stop_strings=stops, tokenizer=wide,
                                                           stop_token_sequences=[seq])}
    hits = {i: R.first_hit(both, free[i]) for i in range(5)}
    print("first hits", hits)
    assert hits[0] >= 0 and hits[2] == 0 and hits[3] >= 0 and hits[4] >= 0
    for i in range(5):
        assert got[i] == (free[i][:hits[i] + 1] if hits[i] >= 0 else free[i]), (i, got[i], free[i], hits[i])
    # the matcher is off again behind the call
    kw = dict(input_ids=reqs[0]["input_ids"], do_sample=False, max_new_tokens=14, eos_token_id=[])
    assert len(model.generate(**kw)[0]) == 14
    # a stop set the device cannot take raises before anything runs: never a stream without its stops
    with pytest.raises(ValueError):
        next(model.generate_stream(reqs, eos_token_id=[], rows=2, stop_token_sequences=[[5, 6]] * 17))
    with pytest.raises(NotImplementedError):
        next(model.generate_stream(reqs, eos_token_id=[], rows=2, stop_strings=["<00001>" * 10], tokenizer=wide))
    with pytest.raises(NotImplementedError):
        next(model.generate_stream(reqs, eos_token_id=[], rows=2, stop_strings=["<00001>" * 10], tokenizer=wide, stop_token_sequences=[[5, 6]]))


def test_unknown_criterion_and_streamer_keep_the_host_path(model, wide, armed):
    """(f) a lambda next to a keyword criterion: the host path, the lambda called once per token; (g) with a streamer nothing changes"""
    ids = _prompt(14, 41)
    kw = dict(input_ids=ids, do_sample=False, max_new_tokens=16, eos_token_id=[])
    free = model.generate(**kw)[0].tolist()
    kc = R.keyword_criterion([free[6:8]], 0)
    calls = []

    def lam(ids, scores, **k):
        calls.append(ids.shape[1])
        return False

    got = model.generate(stopping_criteria=[kc, lam], **kw)[0].tolist()
    assert got == free[:8] and calls == list(range(1, 9)) and not armed

    class Streamer:
        def __init__(self):
            self.got, self.ended = [], False

        def put(self, t):
            self.got += t.view(-1).tolist()

        def end(self):
            self.ended = True

    st = Streamer()
    got = model.generate(stopping_criteria=[kc], streamer=st, **kw)[0].tolist()
    assert got == free[:8] and st.got == free[:8] and st.ended and not armed
    st = Streamer()
    got = model.generate(stop_strings=[wide.text(free[6:8])], tokenizer=wide, streamer=st, **kw)[0].tolist()
    assert got == free[:8] and st.got == free[:8] and not armed          # stop strings with a streamer: HF's criterion on the host


# ---- 5. graph and off-state ---------------------------------------------------------------------------------------------------------------
def test_matcher_in_the_graph_and_off_state(model, small):
    from vz_hip import binding as B
    from vz_hip import stop as ST
    eng = model.engine
    lens = [9, 30, 17]
    ids, _ = _padded(lens, 80)
    _, last = eng.prefill(eng.embed_tokens(ids.to(model.device)), lens)
    first = B.argmax(last)
    buf = torch.empty(3, 4, dtype=torch.int32, device=model.device)

    def steps(stop=False):
        eng.decode_begin(first, lens, lens)
        if stop:
            eng.stop_rows(0, first)
        out = eng.decode_steps(4, out=buf).clone()
        return out, eng.decode_info()[1]

    plain, c0 = steps()
    same, c1 = steps()
    assert c1 == c0 and torch.equal(same, plain)
    # a plan that stops row 1 at its third token (index 2) and row 2 at its first
    plan = ST.Plan(seqs=[([int(plain[1, 0]), int(plain[1, 1])], 0), ([int(first[2])], 0)])
    try:
        eng.set_stop(plan)
        on, c2 = steps(True)
        at = eng.stop_at(0, 3).tolist()
        on2, c3 = steps(True)
    finally:
        eng.set_stop(None)
    off, c4 = steps()
    off2, c5 = steps()
    assert (c2, c3, c4, c5) == (c0 + 1, c0 + 1, c0 + 2, c0 + 2), (c0, c1, c2, c3, c4, c5)
    assert all(torch.equal(t, plain) for t in (on, on2, off, off2))          # arming the matcher changes no id
    want = [R.first_hit(R.keyword_criterion([s for s, _ in plan.seqs], 0), [int(first[r])] + plain[r].tolist()) for r in range(3)]
    assert at == want and at[1] == 2 and at[2] == 0, (at, want)
    # launches per step: the matcher is one more, and with it off the count is the plain one
    def launches(stop):
        eng.prof_enable(True, B.K_OTHER)
        try:
            eng.prof_read()
            steps(stop)
            return eng.prof_read()[0]
        finally:
            eng.prof_enable(False)

    n_plain = launches(False)
    try:
        eng.set_stop(plan)
        n_on = launches(True)
    finally:
        eng.set_stop(None)
    assert n_plain % 4 == 0 and n_on == n_plain + 4 and launches(False) == n_plain, (n_plain, n_on)
    # a stop set outside the limits is an argument error
    with pytest.raises(ValueError):
        eng.set_stop(ST.Plan(seqs=[([], 0)]))          # a sequence without ids
