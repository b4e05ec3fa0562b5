"""Host logic of `VisZephyrForCausalLM.generate_stream` (continuous batching with single and batched admissions) on the CPU: the
engine is replaced by a toy whose next token depends on the WHOLE history held in a KV-cache row, so a request admitted into the
wrong row, moved with the wrong length, armed with the wrong position or decoded past its budget changes its tokens.  (The same
loop against the real engine: tests/test_stages_gpu.py::test_continuous_batching_matches_static_batches.)"""
import types

import pytest
import torch

V = 251           # toy vocabulary: every id is exact in bf16


def next_token(history):
    return (sum((i + 1) * t for i, t in enumerate(history)) * 31 + 7 * len(history) + 3) % V


def solo(prompt, budget, eos):
    hist, out = list(prompt), []
    while len(out) < budget:
        t = next_token(hist)
        out.append(t)
        hist.append(t)
        if t in eos:
            break
    return out


def mix(h, seed, counter):
    """the toy's draw: the token a sampled row emits where a greedy one emits h (h: a function of the whole history)"""
    return (h * 17 + seed * 13 + counter * 29 + 5) % V


def toy_lp(h, t):
    """the toy's log-prob of token t behind a history that hashes to h: a multiple of 1/8, exact in fp32"""
    return -float((h * 7 + t * 3) % 97) / 8.0


def shift_of(cfg):
    """what a row's processor record does in the toy: it moves the chosen candidate by a request-specific amount"""
    return 0 if cfg is None else int(round(cfg.penalty * 10))


class ToyEngine:
    """the engine surface generate_stream touches; cache row r holds the token history of the sequence living there.  The step's modes
    are modelled as far as the host loop can get them wrong: the per-row tail (a row's token is a function of history, seed and draw
    counter), the per-row processor records (a record moves the row's token), the stop matcher (per row the index of the generated
    token at which a stop sequence first held) and the step recorder.  Stale per-row state is KEPT across parking, so a row that is
    re-armed without its writes decodes something else.  fail = (prefix, k): the k-th call of a method so named raises."""
    tp_size = 1

    def __init__(self, max_batch, max_ctx=512, fail=None, async_after=None):
        self.max_batch, self.max_ctx = max_batch, max_ctx
        self.rows = [None] * max_batch          # history per cache row
        self.cur = [None] * max_batch           # armed input token per decode row (None = parked)
        self.dec_B = 0
        self.prefill_shapes, self.moves = [], []
        self.log = []                           # (name, armed?) of every set_* call, in order
        self.samp = self.proc = self.stop = self.row_seqs = self.score = None      # modes: None = off
        self.samp_rows, self.records, self.own_seqs = {}, {}, {}                     # per-row state (survives disarming: read by the tests)
        self.watch, self.at = {}, [-1] * max_batch
        self.stage, self.want_stage = {}, {}    # per row: the writes since its decode_set_row, and the ones its admission owes
        self.sample_flags = {}                  # per row: the sample flag of every tail entry written
        self.writes = {"proc": 0, "seqs": 0, "park_proc": 0, "admit": 0, "park": 0}
        self.armed_at = {}                      # mode -> (requests prefilled so far, size of the last prefill) when it came on
        self.chunks, self.checks, self.async_after = 0, 0, async_after
        if fail is not None:
            count = [0]
            for name in [n for n in dir(self) if n.startswith(fail[0]) and not n.startswith("_") and callable(getattr(self, n))]:
                def failing(*a, _f=getattr(self, name), _n=name, **kw):
                    count[0] += 1
                    if count[0] == fail[1]:
                        raise RuntimeError(f"{_n} failed")
                    return _f(*a, **kw)
                setattr(self, name, failing)

    def embed_tokens(self, ids):
        return ids.to(torch.bfloat16).unsqueeze(-1)

    def prefill_rows(self, row0, emb, seqlens, position_ids=None):
        k = emb.shape[0]
        assert row0 + k <= self.max_batch
        self.prefill_shapes.append((row0, k, emb.shape[1]))
        logits = torch.full((k, V), -1.0)
        for j in range(k):
            assert self.cur[row0 + j] is None if row0 + j < self.dec_B else True, "prefill into a row that is decoding"
            hist = [int(v) for v in emb[j, :seqlens[j], 0].float().tolist()]
            self.rows[row0 + j] = hist
            logits[j, next_token(hist)] = 1.0
        return logits

    def kv_move_rows(self, src, dst, lens):
        assert len(set(dst)) == len(dst) and not set(dst) & set(src)
        for s_, d_, n in zip(src, dst, lens):
            assert s_ >= self.dec_B and d_ < self.dec_B and self.cur[d_] is None
            self.rows[d_] = list(self.rows[s_][:n])
        self.moves.append((tuple(src), tuple(dst), tuple(lens)))

    def decode_begin(self, first_ids, next_pos, ctx_len):
        self.dec_B = len(next_pos)
        assert all(c == 0 for c in ctx_len)
        self.cur = [None] * self.max_batch

    def decode_set_row(self, row, token, next_pos, ctx_len):
        assert row < self.dec_B
        if ctx_len == 0:
            self.cur[row] = None
            self.writes["park"] += 1
            return
        assert len(self.rows[row]) == ctx_len == next_pos, "armed with a context that is not the prefilled one"
        self.cur[row] = token
        self.writes["admit"] += 1
        self.stage[row] = ["row"]
        self.want_stage[row] = ["row"] + ["proc"] * (self.proc is not None) + ["seqs"] * (self.row_seqs is not None) \
            + ["stop_rows"] * (self.stop is not None or self.row_seqs is not None) + ["sampling"] * (self.samp is not None)

    def decode_steps(self, n):
        out = torch.zeros(self.dec_B, n, dtype=torch.int32)
        assert self.score is None or (n <= self.score["cap"] and self.score["rows"] == self.dec_B)
        for s_ in range(n):
            lps = [0.0] * self.dec_B
            for r in range(self.dec_B):
                if self.cur[r] is None:
                    continue
                assert self.stage.get(r) == self.want_stage.get(r), f"row {r}: admission wrote {self.stage[r]}, the engine needs {self.want_stage[r]}"
                self.rows[r].append(self.cur[r])
                assert len(self.rows[r]) < self.max_ctx
                h = (next_token(self.rows[r]) + (shift_of(self.records.get(r)) if self.proc is not None else 0)) % V
                p = self.samp_rows.get(r) if self.samp is not None else None
                if p is not None and p.sample:
                    self.cur[r] = mix(h, p.seed, p.counter)
                    self.samp_rows[r] = p.at(p.counter + 1)
                else:
                    self.cur[r] = h
                out[r, s_] = self.cur[r]
                lps[r] = toy_lp(h, self.cur[r])
                if self.stop is not None or self.row_seqs is not None:
                    self._match(r, self.cur[r])
            if self.score is not None:
                self.score["steps"].append(lps)
        self.chunks += 1
        return out

    def _armed_when(self, name, on):
        if on:
            self.armed_at[name] = (sum(k for _, k, _ in self.prefill_shapes), self.prefill_shapes[-1][1] if self.prefill_shapes else 0)

    def check_async(self):
        self.checks += 1
        if self.async_after is not None and self.chunks >= self.async_after:
            raise RuntimeError("vz_hip: a bounded device-side wait expired (toy); outputs since the last check are invalid")

    # ---- the per-row tail ----
    def set_sampling_rows(self, params=None):
        assert params is None or params == []
        self.log.append(("set_sampling_rows", params is not None))
        self.samp = None if params is None else True
        self._armed_when("set_sampling_rows", params is not None)

    def decode_set_row_sampling(self, row, p):
        assert self.samp is not None and p.counter == 1, "a row's second token is draw 1 of its request's stream"
        self.stage[row].append("sampling")
        self.samp_rows[row] = p
        self.sample_flags.setdefault(row, []).append(p.sample)

    # ---- the per-row processor records ----
    def set_logits_proc_rows(self, on):
        self.log.append(("set_logits_proc_rows", bool(on)))
        self.proc = True if on else None

    def decode_set_row_logits_proc(self, row, cfg=None):
        assert self.proc is not None
        if self.cur[row] is None:               # behind the parking of the row
            assert cfg is None
            self.writes["park_proc"] += 1
        else:
            self.stage[row].append("proc")
            self.writes["proc"] += 1
        self.records[row] = cfg

    # ---- the stop matcher ----
    def set_stop(self, plan=None):
        assert self.row_seqs is None, "the library refuses the matcher's entry point while the per-row sequences are armed"
        self.log.append(("set_stop", plan is not None))
        self.stop = None if plan is None else [[int(t) for t in ids] for ids, _ in plan.seqs]

    def set_stop_row_seqs(self, on):
        self.log.append(("set_stop_row_seqs", bool(on)))
        self.row_seqs = True if on else None

    def decode_set_row_stop_seqs(self, row, seqs=()):
        assert self.row_seqs is not None
        self.stage[row].append("seqs")
        self.writes["seqs"] += 1
        self.own_seqs[row] = [[int(t) for t in s_] for s_ in seqs]

    def stop_rows(self, row0, first_ids):
        assert self.stop is not None or self.row_seqs is not None
        for j, t in enumerate(first_ids.tolist()):
            self.stage[row0 + j].append("stop_rows")
            self.watch[row0 + j], self.at[row0 + j] = [], -1
            self._match(row0 + j, int(t))

    def _match(self, row, t):
        if row not in self.watch:
            return
        g = self.watch[row]
        g.append(t)
        seqs = (self.stop or []) + (self.own_seqs.get(row, []) if self.row_seqs is not None else [])
        if self.at[row] < 0 and any(g[-len(s_):] == s_ for s_ in seqs):
            self.at[row] = len(g) - 1

    def stop_at(self, row0, rows):
        return torch.tensor(self.at[row0:row0 + rows], dtype=torch.int32)

    # ---- the step recorder ----
    def set_scores(self, cap_steps=None, rows=1, warped=False, raw=False):
        self.log.append(("set_scores", cap_steps is not None))
        self.score = None if cap_steps is None else {"cap": int(cap_steps), "rows": int(rows), "steps": []}
        self._armed_when("set_scores", cap_steps is not None)

    def scores_steps(self, n, first=None):
        assert self.score is not None and first is None and n <= len(self.score["steps"])
        rec = torch.zeros(n, self.score["rows"], 4)
        rec[..., 0] = torch.tensor(self.score["steps"][-n:])
        return rec, None, None


def _patch_binding(monkeypatch):
    """binding's first-token entry points on toy logits, whose argmax is the hash of the row's history"""
    from vz_hip import binding as B

    def sample_rows(logits, params):
        assert all(p.counter == 0 for p in params), "a first token is draw 0"
        return torch.tensor([mix(h, p.seed, 0) if p.sample else h for h, p in zip(logits.argmax(-1).tolist(), params)], dtype=torch.int32)

    def token_scores(logits, ids, params, warped=False):
        rec = torch.zeros(logits.shape[0], 4)
        rec[:, 0] = torch.tensor([toy_lp(h, t) for h, t in zip(logits.argmax(-1).tolist(), ids.tolist())])
        return rec

    def logits_process_rows(logits, cfgs):
        for j, (h, c) in enumerate(zip(logits.argmax(-1).tolist(), cfgs)):
            if c is not None:
                logits[j, h], logits[j, (h + shift_of(c)) % V] = -1.0, 1.0

    monkeypatch.setattr(B, "argmax", lambda logits: logits.argmax(-1).to(torch.int32))
    monkeypatch.setattr(B, "sample_rows", sample_rows)
    monkeypatch.setattr(B, "token_scores", token_scores)
    monkeypatch.setattr(B, "logits_process_rows", logits_process_rows)


@pytest.fixture()
def stream_gen(monkeypatch):
    """the generator itself: generate_stream on a stand-in model around a toy engine"""
    from vis_zephyr.model import VisZephyrForCausalLM
    _patch_binding(monkeypatch)

    def run(eng, reqs, **kw):
        me = types.SimpleNamespace(_kv_epoch=0, _ensure_ready=lambda: None, engine=eng, device=torch.device("cpu"),
                                   generation_config=types.SimpleNamespace(eos_token_id=None, top_k=50, top_p=1.0),
                                   config=types.SimpleNamespace(vocab_size=V), prepare_inputs_labels_for_multimodal=None)
        return VisZephyrForCausalLM.generate_stream.__wrapped__(me, reqs, **kw)
    return run


@pytest.fixture()
def stream(stream_gen):
    return lambda eng, reqs, **kw: dict(stream_gen(eng, reqs, **kw))


def _requests(n, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(3, 40, (n,), generator=g).tolist()
    budgets = torch.randint(1, 30, (n,), generator=g).tolist()
    budgets[2] = 1                                                  # finishes on its first token: never takes a row
    prompts = [torch.randint(1, V, (L,), generator=g) for L in lens]
    return [{"input_ids": p.unsqueeze(0), "max_new_tokens": b} for p, b in zip(prompts, budgets)], prompts, budgets


@pytest.mark.parametrize("rows,max_batch,admit,sync_every", [(3, 3, None, 4), (3, 6, None, 4), (3, 6, 2, 16), (3, 6, 0, 1), (1, 4, None, 8),
                                                              (8, 24, None, 4), (5, 7, None, 3)])
def test_stream_equals_solo_generation(stream, rows, max_batch, admit, sync_every):
    reqs, prompts, budgets = _requests(23, seed=rows * 100 + max_batch)
    # an eos id that some sequences emit mid-way and (so that both endings are exercised) that ends request 5 at its first token
    eos = {next_token(prompts[5].tolist()), solo(prompts[7].tolist(), budgets[7] + 3, set())[min(2, budgets[7] - 1)]}
    eng = ToyEngine(max_batch)
    got = stream(eng, reqs, eos_token_id=sorted(eos), rows=rows, sync_every=sync_every, admit=admit)
    assert sorted(got) == list(range(len(reqs)))
    for i, (p, b) in enumerate(zip(prompts, budgets)):
        assert got[i].tolist() == solo(p.tolist(), b, eos), f"request {i}"
    spare = max_batch - rows
    width = min(spare, 16) if admit is None else admit
    if width >= 2 and rows >= 2:
        assert eng.moves, "no batched admission happened"
        assert all(r0 == rows and k <= width for r0, k, _ in eng.prefill_shapes if k > 1)     # groups live in the spare rows only
    elif width < 2:
        assert not eng.moves and all(k == 1 and r0 < rows for r0, k, _ in eng.prefill_shapes)


def test_stream_argument_checks(stream):
    reqs, _, _ = _requests(4, seed=1)
    with pytest.raises(ValueError):
        stream(ToyEngine(4), reqs, rows=5)
    with pytest.raises(ValueError):
        stream(ToyEngine(6), reqs, rows=4, admit=3)                 # two spare rows only
    long = [{"input_ids": torch.ones(1, 500, dtype=torch.long), "max_new_tokens": 20}]
    with pytest.raises(ValueError):
        stream(ToyEngine(2), long, rows=1)                          # prompt + budget beyond max_ctx


class ToyBatchEngine(ToyEngine):
    """+ the static-batch surface of `_generate_batched`: one right-padded prefill, decode_begin with the first tokens"""

    def prefill(self, embeds, seqlens, position_ids=None, all_logits=False, last_logits=True):
        assert not all_logits and last_logits and embeds.shape[0] <= min(self.max_batch, 64)
        self.dec_B = 0
        return None, self.prefill_rows(0, embeds, seqlens)

    def decode_begin(self, first_ids, next_pos, ctx_len):
        self.dec_B = len(next_pos)
        for b in range(self.dec_B):
            assert len(self.rows[b]) == ctx_len[b] == next_pos[b]
        self.cur = [int(t) for t in first_ids.tolist()] + [None] * (self.max_batch - self.dec_B)


@pytest.mark.parametrize("n_seq,max_batch,sync_every,max_new", [(5, 8, 4, 24), (5, 2, 16, 24), (3, 4, 1, 9), (1, 1, 16, 5), (4, 4, 5, 1)])
def test_static_batches_eos_and_padding_equal_solo_generation(monkeypatch, n_seq, max_batch, sync_every, max_new):
    """`_generate_batched`: rows that emitted eos show the pad token from then on, the batch stops at the first step after which
    every row is done, batches beyond the engine's rows run in parts - every row equals the sequence generated alone."""
    from vis_zephyr.model import VisZephyrForCausalLM
    from vz_hip import binding as B
    monkeypatch.setattr(B, "argmax", lambda logits: logits.argmax(-1).to(torch.int32))
    g = torch.Generator().manual_seed(n_seq * 10 + max_batch)
    lens = torch.randint(2, 30, (n_seq,), generator=g).tolist()
    prompts = [torch.randint(1, V, (L,), generator=g).tolist() for L in lens]
    free = [solo(p, max_new, set()) for p in prompts]
    eos = {free[0][min(3, max_new - 1)]} | ({free[-1][0]} if n_seq > 2 else set())     # one ends mid-way, one on its first token
    S = max(lens)
    emb = torch.zeros(n_seq, S, 1, dtype=torch.bfloat16)
    for i, p in enumerate(prompts):
        emb[i, :len(p), 0] = torch.tensor(p, dtype=torch.bfloat16)
    eng = ToyBatchEngine(max_batch)
    me = types.SimpleNamespace(engine=eng, device=torch.device("cpu"))
    me._generate_batched = types.MethodType(VisZephyrForCausalLM._generate_batched, me)
    PAD = 250
    out = me._generate_batched(emb, lens, None, max_new, eos, PAD, sync_every)
    want = [solo(p, max_new, eos) for p in prompts]
    cap = min(max_batch, 64)
    for i0 in range(0, n_seq, cap):              # each part stops when ITS rows are done; the rest of the row is padding
        n_part = max(len(w) for w in want[i0:i0 + cap])
        for i in range(i0, min(n_seq, i0 + cap)):
            row = out[i].tolist()
            assert row[:len(want[i])] == want[i], f"row {i}"
            assert all(t == PAD for t in row[len(want[i]):]) and len(row) >= n_part
    assert out.shape[1] == max(len(w) for w in want)


# ---- the stream's modes: sampled rows, log-probs, call-level stops, per_request, and what it leaves armed ----

def reference(prompt, budget, eos, seed=None, shift=0, stops=()):
    """one request generated alone under the toy's rules: (ids, log-probs, how it ended).  "first": eos or budget at its first token (it
    never takes a row); "eos" / "budget" / "stop" later - a stop also when the first token is one (the row is taken, then cut)."""
    hist, out, lps = list(prompt), [], []
    while True:
        h = (next_token(hist) + shift) % V
        t = h if seed is None else mix(h, seed, len(out))
        out.append(t)
        lps.append(toy_lp(h, t))
        hist.append(t)
        if t in eos or len(out) >= budget:
            return out, lps, "first" if len(out) == 1 else ("eos" if t in eos else "budget")
        if any(out[-len(s_):] == list(s_) for s_ in stops):
            return out, lps, "stop"


ROUTES = [(3, 6, None, 4), (1, 4, None, 8), (5, 7, None, 3), (2, 2, None, 5), (4, 8, 2, 16)]      # rows, max_batch, admit, sync_every
LONG = (9, 11, 13, 15, 17)          # requests with room for a stop in the middle


def _scenario(n=24, seed=7, sampled=(), logprobs=(), call_stops=False, own=False):
    """requests, what each yields alone, and the call's keywords.  call_stops: a one-id stop out of request 9, a two-id one out of
    request 11, request 13's first token.  own: requests 3, 8 and 17 carry a processor key, 15 and 17 stop sequences of their own."""
    reqs, prompts, budgets = _requests(n, seed)
    for i in LONG:
        budgets[i] = reqs[i]["max_new_tokens"] = 12
    for i in sampled:
        reqs[i].update(do_sample=True, temperature=0.7, seed=1000 + i)
    for i in logprobs:
        reqs[i]["logprobs"] = True
    penalty = {3: 1.4, 8: 1.1, 17: 1.3} if own else {}
    for i, p in penalty.items():
        reqs[i]["repetition_penalty"] = p
    how = [dict(seed=1000 + i if i in sampled else None, shift=int(round(penalty.get(i, 0) * 10))) for i in range(n)]
    free = [reference(prompts[i].tolist(), max(budgets[i], 8), set(), **how[i])[0] for i in range(n)]
    eos = {free[5][0], free[7][min(2, budgets[7] - 1)]}         # ends request 5 at its first token and request 7 mid-way
    stops = [[free[9][3]], free[11][1:3], [free[13][0]]] if call_stops else []
    mine = {15: [[free[15][4]]], 17: [free[17][2:4]]} if own else {}
    for i, seqs in mine.items():
        reqs[i]["stop_token_sequences"] = seqs
    expect = [reference(prompts[i].tolist(), budgets[i], eos, stops=stops + mine.get(i, []), **how[i]) for i in range(n)]
    kw = dict(eos_token_id=sorted(eos))
    if call_stops:
        kw["stop_token_sequences"] = stops
    if own:
        kw["per_request"] = True
    return types.SimpleNamespace(reqs=reqs, expect=expect, kw=kw, logprobs=set(logprobs))


def _route_kw(route):
    return dict(rows=route[0], admit=route[2], sync_every=route[3])


def _check_results(results, sc):
    """every request once, with the ids (and, where it asked, the log-probs - and only there) that it gets alone"""
    assert sorted(r[0] for r in results) == list(range(len(sc.reqs)))
    for r in results:
        ids, lps, _ = sc.expect[r[0]]
        assert r[1].tolist() == ids, f"request {r[0]}"
        assert (len(r) == 3) == (r[0] in sc.logprobs), f"request {r[0]}"
        if len(r) == 3:
            assert r[2].dtype == torch.float32 and r[2].tolist() == lps, f"request {r[0]}"


def _check_modes(eng, armed):
    """the modes in `armed` came on in that order, each once, and each went off once (in which order: test_leaving_the_stream_*)"""
    assert [name for name, on in eng.log if on] == armed
    assert sorted(name for name, on in eng.log if not on) == sorted(armed)


@pytest.mark.parametrize("route", ROUTES)
def test_sampled_and_greedy_requests_share_the_batch(stream_gen, route):
    sampled = (4, 5, 6, 10, 12, 13, 16, 19, 22)
    sc = _scenario(sampled=sampled)
    eng = ToyEngine(route[1])
    _check_results(list(stream_gen(eng, sc.reqs, **sc.kw, **_route_kw(route))), sc)
    _check_modes(eng, ["set_sampling_rows"])                    # once ...
    prefilled, last = eng.armed_at["set_sampling_rows"]
    assert prefilled - last <= sampled[0] < prefilled           # ... by the admission that brought the first sampled request
    # a sampled request's row was handed to a greedy one, which the ids above show to have decoded greedily
    assert any(True in f and False in f[f.index(True):] for f in eng.sample_flags.values())
    greedy = _scenario()
    eng = ToyEngine(route[1])
    _check_results(list(stream_gen(eng, greedy.reqs, **greedy.kw, **_route_kw(route))), greedy)
    assert eng.log == [] and not eng.sample_flags               # no request samples: the per-row tail is never armed


@pytest.mark.parametrize("route", ROUTES)
def test_logprobs_of_flagged_requests(stream_gen, route):
    """the log-prob of every token is the toy's for that history and that token: across chunk boundaries, a stop's cut, admissions"""
    logprobs = (2, 3, 7, 9, 11, 13, 14, 20)
    sc = _scenario(sampled=(6, 11, 14), logprobs=logprobs, call_stops=True)
    assert sc.expect[2][2] == "first" and {sc.expect[i][2] for i in (9, 11, 13)} == {"stop"}
    eng = ToyEngine(route[1])
    _check_results(list(stream_gen(eng, sc.reqs, **sc.kw, **_route_kw(route))), sc)
    assert [name for name, on in eng.log if on][:1] == ["set_stop"]
    assert [name for name, on in eng.log].count("set_scores") == 2                 # on once, off once
    prefilled, last = eng.armed_at["set_scores"]
    assert prefilled - last <= logprobs[0] < prefilled


@pytest.mark.parametrize("route", ROUTES)
def test_call_level_stops(stream_gen, route):
    sc = _scenario(call_stops=True)
    ends = [e[2] for e in sc.expect]
    assert {"first", "eos", "budget", "stop"} <= set(ends)
    assert sc.expect[13][2] == "stop" and len(sc.expect[13][0]) == 1              # its first token already stops it
    assert sc.expect[9][2] == "stop" and len(sc.expect[9][0]) == 4 and sc.expect[11][2] == "stop" and len(sc.expect[11][0]) == 3
    eng = ToyEngine(route[1])
    _check_results(list(stream_gen(eng, sc.reqs, **sc.kw, **_route_kw(route))), sc)
    _check_modes(eng, ["set_stop"])
    took_a_row = len(ends) - ends.count("first")
    assert eng.writes["admit"] == eng.writes["park"] == took_a_row                # every stopped row was parked, and refilled


@pytest.mark.parametrize("route", ROUTES)
def test_per_request_records_and_stop_sequences(stream_gen, route):
    """the order of an admission's writes is asserted by the toy's decode_steps (`want_stage`)"""
    sc = _scenario(sampled=(4, 8, 15, 21), logprobs=(3, 17), call_stops=True, own=True)
    ends = [e[2] for e in sc.expect]
    assert ends[15] == "stop" and len(sc.expect[15][0]) == 5 and ends[17] == "stop" and ends.count("first") >= 2
    eng = ToyEngine(route[1])
    _check_results(list(stream_gen(eng, sc.reqs, **sc.kw, **_route_kw(route))), sc)
    assert [name for name, on in eng.log if on][:3] == ["set_stop", "set_logits_proc_rows", "set_stop_row_seqs"]
    took_a_row = len(ends) - ends.count("first")
    assert eng.writes == {"admit": took_a_row, "proc": took_a_row, "seqs": took_a_row, "park": took_a_row, "park_proc": took_a_row}
    assert all(cfg is None for cfg in eng.records.values())                       # every parked row's record is inactive


@pytest.mark.parametrize("route", ROUTES[:3])
def test_per_request_without_keys_is_the_plain_stream(stream_gen, route):
    sc = _scenario(sampled=(4, 8), logprobs=(3, 17), call_stops=True)
    plain = list(stream_gen(ToyEngine(route[1]), sc.reqs, **sc.kw, **_route_kw(route)))
    eng = ToyEngine(route[1])
    flagged = list(stream_gen(eng, sc.reqs, per_request=True, **sc.kw, **_route_kw(route)))
    _check_results(flagged, sc)
    assert [[t.tolist() if torch.is_tensor(t) else t for t in r] for r in flagged] == [[t.tolist() if torch.is_tensor(t) else t for t in r] for r in plain]
    assert all(cfg is None for cfg in eng.records.values())


MODES = {"eager": dict(call_stops=True, own=True), "lazy": dict(sampled=(0, 1, 8), logprobs=(4, 9)),
         "all": dict(call_stops=True, own=True, sampled=(0, 1, 8), logprobs=(4, 9))}
ARMED = {"eager": ["set_stop", "set_logits_proc_rows", "set_stop_row_seqs"], "lazy": ["set_sampling_rows", "set_scores"]}
ARMED["all"] = ARMED["eager"] + ARMED["lazy"]


def _assert_disarmed(eng):
    """what was armed is disarmed exactly once, last first; nothing else is"""
    armed = [name for name, on in eng.log if on]
    assert len(set(armed)) == len(armed)
    assert eng.log == [(name, True) for name in armed] + [(name, False) for name in reversed(armed)]
    return armed


@pytest.mark.parametrize("modes", list(MODES))
@pytest.mark.parametrize("how", ["exhausted", "closed", "embed"])
def test_leaving_the_stream_disarms_what_it_armed(stream_gen, modes, how):
    sc = _scenario(**MODES[modes])
    if how == "embed":
        sc.reqs[6] = {"input_ids": torch.ones(1, 500, dtype=torch.long), "max_new_tokens": 20}      # prompt + budget beyond max_ctx
    eng = ToyEngine(6)
    gen = stream_gen(eng, sc.reqs, rows=3, sync_every=4, **sc.kw)
    if how == "exhausted":
        assert len(list(gen)) == len(sc.reqs)
    elif how == "closed":
        next(gen)
        gen.close()
    else:
        with pytest.raises(ValueError, match="exceeds the engine's max_ctx"):
            list(gen)
    armed = _assert_disarmed(eng)
    assert armed == ARMED[modes] if how == "exhausted" else armed and armed == ARMED[modes][:len(armed)]      # (a lazy mode may not have come on yet)


@pytest.mark.parametrize("modes", list(MODES))
@pytest.mark.parametrize("fail", [("decode_steps", 2), ("prefill_rows", 3), ("set_", 3), ("set_", 2)])
def test_leaving_the_stream_after_a_failed_engine_call(stream_gen, modes, fail):
    if fail[0] == "set_" and fail[1] > len(ARMED[modes]):
        fail = None                          # fewer armings than that: the call would be a disarming
    sc = _scenario(**MODES[modes])
    eng = ToyEngine(6, fail=fail)
    gen = stream_gen(eng, sc.reqs, rows=3, sync_every=4, **sc.kw)
    if fail is None:
        list(gen)
    else:
        with pytest.raises(RuntimeError, match="failed"):
            list(gen)
    armed = _assert_disarmed(eng)
    if fail is None or fail[0] == "set_":
        assert armed == (ARMED[modes] if fail is None else ARMED[modes][:fail[1] - 1])       # the arming that raised is not disarmed
    else:
        assert armed and armed == ARMED[modes][:len(armed)]


def test_expired_device_wait_raises_out_of_the_stream(stream_gen):
    """`check_async` behind every chunk's readback: nothing of the chunk whose check fails is yielded"""
    sc = _scenario(sampled=(0, 1, 8), logprobs=(4, 9), call_stops=True)
    clean = ToyEngine(6)
    before = [r[0] for r in stream_gen(clean, sc.reqs, rows=3, sync_every=4, **sc.kw) if clean.chunks < 2]
    assert clean.checks == clean.chunks > 2
    eng, got = ToyEngine(6, async_after=2), []
    with pytest.raises(RuntimeError, match="device-side wait expired"):
        for r in stream_gen(eng, sc.reqs, rows=3, sync_every=4, **sc.kw):
            got.append(r[0])
    assert got == before and eng.chunks == 2
    _assert_disarmed(eng)


@pytest.mark.parametrize("ids,budget,chunk,at,keep,done", [
    ([5], 4, [6, 7, 8, 9], -1, 3, True),           # budget inside the chunk
    ([5], 5, [6, 7, 8, 9], -1, 4, True),           # ... at its end
    ([5], 9, [6, 7, 8, 9], -1, 4, False),          # ... beyond it
    ([5], 9, [6, 1, 8, 9], -1, 2, True),           # eos, no matcher
    ([5], 9, [6, 1, 8, 9], 3, 2, True),            # eos before `at`
    ([5], 9, [6, 7, 8, 1], 2, 2, True),            # eos after `at`: the stop ends the row, inclusive of token 2
    ([5, 6, 7], 9, [8, 9], 1, 0, True),            # `at` in an earlier chunk: the row is at its cut, nothing is kept
    ([5], 9, [6, 7], 0, 0, True),                  # the first token already stopped it
    ([5, 6], 9, [7, 8, 9], 4, 3, True),            # `at` is the chunk's last token
    ([5, 6], 9, [7, 8, 9], 7, 3, False),           # `at` beyond what the row holds (it cannot be: the row keeps going)
    ([5], 2, [6, 7], 3, 1, True),                  # budget before `at`
])
def test_row_end_within_a_chunk(ids, budget, chunk, at, keep, done):
    from vz_hip import stream as S
    assert S.row_end(ids, budget, chunk, at, eos={1, 2}) == (keep, done)
