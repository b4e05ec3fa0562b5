"""Prompt-lookup speculative decoding of a SAMPLED sequence, host side (vz_hip/spec.py): the prefix count against HF's expression, the
chunked loop with sampled verify steps on a fake engine whose draws follow the counter rule (row i of a step behind w generated ids
draws at counter w + 1 + i, stream-row word 0), and the eligibility rule."""
import random

import numpy as np
import pytest
import torch

from oracle import sampling_oracle as SO
from vz_hip import spec
from vz_hip.sample_rows import RowParams

V = 50
PAR = RowParams(True, 0.7, 10, 0.9, 0x5EED_1234_ABCD, 0)


def test_accept_count_is_hfs_prefix_count():
    """hf:generation/utils.py `_assisted_decoding`: n_matches = ((~(candidate_new_tokens == selected_tokens[:, :-1])).cumsum(-1) < 1).sum()"""
    rng = random.Random(11)
    some = 0
    for _ in range(500):
        L = rng.randint(1, 7)
        cand = torch.tensor([[rng.randrange(4) for _ in range(L)]])
        sel = torch.tensor([[rng.randrange(4) for _ in range(L + 1)]])
        if rng.random() < 0.5:                               # a matching prefix of random length, so long runs occur too
            n = rng.randint(0, L)
            sel[0, :n] = cand[0, :n]
        want = int(((~(cand == sel[:, :-1])).cumsum(-1) < 1).sum())
        assert spec.accept_count(cand[0].tolist(), sel[0].tolist()) == want
        some += want > 0
    assert some > 150


# ------------------------------------------------------------------------------------------------
# a sampled fake engine
# ------------------------------------------------------------------------------------------------
_TABLE = np.random.default_rng(7).normal(0.0, 2.0, size=(V, V, V)).astype(np.float32)


def model_logits(prev2, prev1):
    """the 'model': logits [50] as a function of the last two ids"""
    return _TABLE[prev2 % V, prev1 % V]


def draw_at(prev2, prev1, par, counter):
    return SO.draw(model_logits(prev2, prev1), par.temperature, par.top_k, par.top_p, par.seed, counter)


def reference(prompt, par, n):
    """the sequential loop: token t of the generated sequence is drawn with counter t"""
    seq = list(prompt)
    out = []
    for t in range(n):
        tok = draw_at(seq[-2], seq[-1], par, t)
        out.append(tok)
        seq.append(tok)
    return out


class FakeEngine:
    """The device semantics of a sampled verify step in Python (csrc/spec.hip: spec_tail_kernel behind csrc/sampling.hip:
    spec_sample_kernel), with the engine's interface as vz_hip.spec.decode uses it.  Row i of a step behind w generated ids draws with
    counter w + 1 + i.  (An engine with every row on counter w + 1, and one whose counters follow steps instead of ids, were each run
    through these tests once while they were written: both fail test_sampled_loop_equals_the_sequential_draws.)"""

    def __init__(self, prompt, max_ctx=4096):
        self.prompt, self.max_ctx = list(prompt), max_ctx
        self.on, self.par, self.calls = False, None, []

    def decode_begin(self, first, next_pos, ctx_len):
        self.R = len(next_pos)
        assert list(ctx_len) == [ctx_len[0] + i for i in range(self.R)] and list(next_pos) == [next_pos[0] + i for i in range(self.R)]
        self.first = int(first[0])

    def set_spec(self, on, D=0, max_ngram=2, history=(), eos=(), budget=0, source=0, stream=None, sample=None):
        self.on = on
        if not on:
            self.par = None
            return
        assert D == self.R - 1 and list(history) == self.prompt + [self.first]
        assert sample is not None and sample.sample, "the sampled loop arms the verify steps with its record"
        self.par = sample
        self.hist, self.eos, self.budget, self.ngram = list(history), set(eos), budget, max_ngram
        self.source, self.stream = source, list(stream or [])
        self.w, self.done, self.records, self.steps = 0, budget == 0, [], 0
        self._draft()

    def _draft(self):
        D = self.R - 1
        if self.source == 1:
            self.draft = [(self.stream[self.w + j] if self.w + j < len(self.stream) else 0) for j in range(D)]
            self.drafted = D
        else:
            d = spec.lookup_draft(self.hist, D, self.ngram, self.eos)
            self.drafted = len(d)
            self.draft = (d + [0] * D)[:D]

    def decode_steps(self, n):
        assert self.on
        self.calls.append(n)
        out = []
        D = self.R - 1
        for _ in range(n):
            if self.done:
                self.records.append([0, 0, 0])
                self.steps += 1
                continue
            # row i is fed [.., cur, draft_0 .. draft_(i-1)] and draws with its own counter
            fed = self.hist + self.draft
            L = len(self.hist)
            g = [draw_at(fed[L + i - 2], fed[L + i - 1], self.par, self.w + 1 + i) for i in range(self.R)]
            a = spec.accept_count(self.draft, g)
            emit = []
            for j in range(a + 1):
                if self.w + len(emit) >= self.budget:
                    break
                emit.append(g[j])
                if g[j] in self.eos:
                    self.done = True
                    break
            self.w += len(emit)
            self.done = self.done or self.w >= self.budget
            self.hist += emit
            out += emit
            self.records.append([self.drafted, max(0, len(emit) - 1), len(emit)])
            self.steps += 1
            self._draft()
        return torch.tensor(out, dtype=torch.int32)

    def check_async(self):
        pass

    def spec_state(self):
        return {"done": self.done, "steps": len(self.records), "tokens": self.w, "records": self.records, "D": self.R - 1}


PROMPT = [3, 9, 14, 27, 31, 8] * 4


def _run(D, max_new, eos=(), source=0, stream=None, par=PAR, sync_every=4, **eng_kw):
    eng = FakeEngine(PROMPT, **eng_kw)
    first = draw_at(PROMPT[-2], PROMPT[-1], par, 0)
    rep = {}
    out = spec.decode(eng, first, len(PROMPT), len(PROMPT), PROMPT, D, max_new, eos, 2, sync_every, source=source, stream=stream, report=rep,
                      sample=par)
    assert eng.on is False and eng.par is None                          # the mode is off again afterwards
    return out, rep, eng


@pytest.fixture(scope="module")
def ref():
    return reference(PROMPT, PAR, 48)


@pytest.mark.parametrize("D", [1, 3, 7])
def test_sampled_loop_equals_the_sequential_draws(ref, D):
    n = 40
    wrong = [(t + 1) % V for t in ref[1:]]
    out_n, rep_n, _ = _run(D, n)                                        # n-gram drafts
    out_t, rep_t, eng_t = _run(D, n, source=1, stream=ref[1:])          # the true continuation
    out_w, rep_w, eng_w = _run(D, n, source=1, stream=wrong)            # always wrong
    assert out_n == ref[:n] and out_t == ref[:n] and out_w == ref[:n]
    for rep in (rep_n, rep_t, rep_w):
        assert rep["used"] and rep["sampled"] is True and rep["D"] == D and rep["tokens"] == n
    full = [r for r in eng_t.records if r[2] > 0]
    assert all(r[1] == D and r[2] == D + 1 for r in full[:-1]) and len(full) == -(-(n - 1) // (D + 1))
    assert all(r[1] == 0 and r[2] == 1 for r in eng_w.records if r[2] > 0) and rep_w["steps"] == n - 1
    assert rep_t["accepted"] == sum(r[1] for r in full)


@pytest.mark.parametrize("D", [1, 3, 7])
@pytest.mark.parametrize("max_new", [1, 2, 5, 13])
def test_budget_cuts_a_run(ref, D, max_new):
    for kw in (dict(), dict(source=1, stream=ref[1:])):
        out, rep, _ = _run(D, max_new, **kw)
        assert out == ref[:max_new] and rep["tokens"] == max_new


@pytest.mark.parametrize("D", [1, 3, 7])
def test_eos_inside_an_accepted_run(ref, D):
    for cut in (2, 6, 11):                                              # with the true continuation every id but a step's first is an accepted guess
        eos = ref[cut]
        n = ref.index(eos) + 1
        for kw in (dict(), dict(source=1, stream=ref[1:])):
            out, _, _ = _run(D, 40, eos=[eos], **kw)
            assert out == ref[:n], (cut, kw)


def test_draft_slots_sampled():
    ok = dict(n_seq=1, num_beams=1, streamer=None, stopping_criteria=None, tp_size=1, max_batch=8, prompt_len=100, max_new=128, max_ctx=4096)
    for k, kw in ((10, {}), (3, {}), (10, {"max_batch": 4}), (10, {"prompt_len": 4096 - 128 - 7}), (10, {"n_eos": 4})):
        want = spec.draft_slots(k, 2, greedy=True, **{**ok, **kw})
        assert want > 0 and spec.draft_slots(k, 2, greedy=False, sampled=True, **{**ok, **kw}) == want
    assert spec.draft_slots(10, 2, greedy=False, **ok) == 0 and spec.draft_slots(10, 2, greedy=False, sampled=False, **ok) == 0
    for change in ({"n_seq": 2}, {"num_beams": 4}, {"streamer": object()}, {"stopping_criteria": [object()]}, {"max_batch": 1}, {"tp_size": 2},
                   {"prompt_len": 4096 - 128 - 6}, {"n_eos": 5}, {"heads_per_kv": 8}):
        assert spec.draft_slots(10, 2, greedy=False, sampled=True, **{**ok, **change}) == 0, change
    assert spec.draft_slots(None, 2, greedy=False, sampled=True, **ok) == 0 and spec.draft_slots(10, 5, greedy=False, sampled=True, **ok) == 0
