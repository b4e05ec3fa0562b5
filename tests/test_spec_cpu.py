"""Prompt-lookup speculative decoding, host side (vz_hip/spec.py): the draft rule against the installed HF class, the history of a
spliced prompt, the eligibility rule and the chunked loop's bookkeeping on a fake engine."""
import random

import pytest
import torch

from vz_hip import spec


def _hf_candidates(seq, k, n, eos):
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    gen = PromptLookupCandidateGenerator(eos_token_id=torch.tensor(eos, dtype=torch.long) if eos else None, num_output_tokens=k,
                                         max_matching_ngram_size=n, max_length=10 ** 6)
    ids = torch.tensor([seq], dtype=torch.long)
    cand, _ = gen.get_candidates(ids)
    return cand[0, len(seq):].tolist()


def random_cases(n_cases, seed=0, max_len=60):
    rng = random.Random(seed)
    for _ in range(n_cases):
        L = rng.randint(2, max_len)
        vocab = rng.choice([3, 5, 12])
        seq = [rng.randrange(vocab) for _ in range(L)]
        eos = [rng.randrange(vocab)] if rng.random() < 0.5 else []
        yield seq, rng.randint(1, 7), rng.randint(1, 4), eos


def test_lookup_draft_matches_hf_prompt_lookup():
    """C1: the plain restatement == PromptLookupCandidateGenerator.get_candidates on 2000 seeded random sequences."""
    bad = 0
    some = 0
    for seq, k, n, eos in random_cases(2000):
        want = _hf_candidates(seq, k, n, eos)
        got = spec.lookup_draft(seq, k, n, eos)
        bad += got != want
        some += bool(want)
    assert bad == 0
    assert some > 500           # the cases do exercise matches


def test_lookup_draft_hand_cases():
    # leftmost occurrence wins, up to k ids follow
    assert spec.lookup_draft([1, 2, 3, 9, 1, 2, 4, 1, 2], 3, 2) == [3, 9, 1]
    # n falls back from max to 1: no earlier [7, 2], but an earlier [2]
    assert spec.lookup_draft([1, 2, 3, 7, 2], 2, 2) == [3, 7]
    assert spec.lookup_draft([1, 2, 3, 7, 2], 2, 4) == [3, 7]
    # nothing repeats
    assert spec.lookup_draft([1, 2, 3, 4], 5, 3) == []
    # the only occurrence is the tail itself: no continuation
    assert spec.lookup_draft([5], 3, 2) == []
    # eos crops the proposal in front of it; cropped to nothing = no draft (no second match is tried, as in HF)
    assert spec.lookup_draft([1, 2, 3, 0, 8, 1, 2], 4, 2, eos=[0]) == [3]
    assert spec.lookup_draft([1, 2, 0, 8, 1, 2, 5, 1, 2], 4, 2, eos=[0]) == []
    # -1 sentinels never match (neither in the window nor as the tail) and crop a proposal
    assert spec.lookup_draft([4, -1, -1, 6, 4], 3, 1) == []
    assert spec.lookup_draft([4, 5, -1, 6, 4], 3, 1) == [5]
    assert spec.lookup_draft([-1, -1, 3, -1], 3, 2) == []
    assert spec.lookup_draft([-1, 7, -1, 7], 3, 2) == []          # [-1, 7] must not match itself through the sentinel


def test_spliced_history():
    IMG = -200
    h = spec.spliced_history([1, 5, IMG, 6, 7], [3], IMG, 32)
    assert len(h) == 4 + 96 and h[:2] == [1, 5] and h[2:98] == [-1] * 96 and h[98:] == [6, 7]
    assert spec.spliced_history([1, IMG, 2, IMG, 3], [1, 2], IMG, 32, max_len=40) == [1] + [-1] * 32 + [2] + [-1] * 6
    assert spec.spliced_history([1, 2, 3], [], IMG) == [1, 2, 3]
    with pytest.raises(IndexError):
        spec.spliced_history([IMG, IMG], [1], IMG)


def test_draft_slots_eligibility():
    """C2: calls the mode does not cover take today's path (0 slots)."""
    ok = dict(n_seq=1, greedy=True, num_beams=1, streamer=None, stopping_criteria=None, tp_size=1, max_batch=8, prompt_len=100, max_new=128,
              max_ctx=4096)
    assert spec.draft_slots(10, 2, **ok) == 7
    assert spec.draft_slots(3, 2, **ok) == 3
    assert spec.draft_slots(10, 2, **{**ok, "max_batch": 4}) == 3
    assert spec.draft_slots(None, 2, **ok) == 0
    assert spec.draft_slots(0, 2, **ok) == 0
    for change in ({"greedy": False}, {"n_seq": 2}, {"num_beams": 4}, {"streamer": object()}, {"stopping_criteria": [object()]},
                   {"max_batch": 1}, {"tp_size": 2}, {"prompt_len": 4096 - 128 - 6}):
        assert spec.draft_slots(10, 2, **{**ok, **change}) == 0, change
    assert spec.draft_slots(10, 2, **{**ok, "prompt_len": 4096 - 128 - 7}) == 7
    assert spec.draft_slots(10, 5, **ok) == 0 and spec.draft_slots(10, 0, **ok) == 0
    # what the device tail / verify attention do not take stays on today's path too: > 4 eos ids, a GQA ratio other than 4
    assert spec.draft_slots(10, 2, n_eos=4, **ok) == 7 and spec.draft_slots(10, 2, n_eos=5, **ok) == 0
    assert spec.draft_slots(10, 2, heads_per_kv=8, **ok) == 0


class FakeEngine:
    """The device semantics of a verify step in Python, for a 'model' whose greedy continuation is a fixed id sequence `truth`
    (truth[t] = the t-th generated id).  Keeps the engine's interface as vz_hip.spec.decode uses it."""

    def __init__(self, truth, max_ctx):
        self.truth, self.max_ctx = list(truth), max_ctx
        self.calls, self.on = [], False
        self.max_slot = -1

    def decode_begin(self, first, next_pos, ctx_len):
        self.R = len(next_pos)
        assert list(ctx_len) == [ctx_len[0] + i for i in range(self.R)] and list(next_pos) == [next_pos[0] + i for i in range(self.R)]
        assert int(first[0]) == self.truth[0]
        self.L = ctx_len[0]

    def set_spec(self, on, D=0, max_ngram=2, history=(), eos=(), budget=0, source=0, stream=None):
        self.on = on
        if not on:
            return
        assert D == self.R - 1 and len(history) == self.L + 1
        self.hist, self.eos, self.budget, self.ngram = list(history), set(eos), budget, max_ngram
        self.w, self.done, self.records = 0, budget == 0, []
        self.draft = spec.lookup_draft(self.hist, D, max_ngram, eos)

    def decode_steps(self, n):
        assert self.on
        self.calls.append(n)
        out = []
        D = self.R - 1
        for _ in range(n):
            if self.done:
                self.records.append([0, 0, 0])
                continue
            self.max_slot = max(self.max_slot, self.L + self.R - 1)
            assert self.L + self.R - 1 < self.max_ctx                  # no row ever writes a slot outside the cache
            draft = (self.draft + [0] * D)[:D]
            g = [self.truth[self.w + 1 + i] if self.w + 1 + i < len(self.truth) else 10 ** 6 for i in range(self.R)]
            a = 0
            while a < D and draft[a] == g[a]:
                a += 1
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
            self.L += len(emit)
            self.hist += emit
            out += emit
            self.records.append([len(self.draft), max(0, len(emit) - 1), len(emit)])
            self.draft = spec.lookup_draft(self.hist, D, self.ngram, self.eos)
        return torch.tensor(out, dtype=torch.int32)

    def check_async(self):
        pass

    def spec_state(self):
        return {"done": self.done, "steps": len(self.records), "tokens": self.w, "records": self.records, "D": self.R - 1}


def _run(truth, prompt, D, max_new, eos=(), max_ctx=4096, sync_every=4, ngram=2):
    eng = FakeEngine(truth, max_ctx)
    rep = {}
    out = spec.decode(eng, truth[0], len(prompt), len(prompt), prompt, D, max_new, eos, ngram, sync_every, report=rep)
    assert eng.on is False                                             # the mode is always switched off again
    return out, rep, eng


def test_loop_accepts_repeats_and_reports():
    prompt = [3, 4, 5, 6, 7, 8, 9, 10] * 3
    truth = ([3, 4, 5, 6, 7, 8, 9, 10] * 8)[:50]
    out, rep, eng = _run(truth, prompt, D=7, max_new=40)
    assert out == truth[:40]
    assert rep["used"] and rep["D"] == 7 and rep["tokens"] == 40
    assert rep["steps"] < 12 and rep["accepted"] >= 25                 # the repeated pattern is drafted and accepted
    assert sum(eng.calls) <= 39                                        # never more steps than ids to go


def test_loop_truncates_at_eos_and_budget_inside_an_accepted_run():
    prompt = [3, 4, 5, 6, 7, 8, 9, 10] * 3
    truth = [3, 4, 5, 6, 2, 8, 9, 10, 3, 4, 5, 6, 7, 8]
    out, rep, _ = _run(truth, prompt, D=7, max_new=12, eos=[2])
    assert out == [3, 4, 5, 6, 2]                                      # eos was a wrong guess here (the draft said 7): emitted by the model, ends the run
    truth2 = ([3, 4, 5, 6, 7, 8, 9, 10] * 4)
    out, rep, _ = _run(truth2, prompt, D=7, max_new=12, eos=[8])
    assert out == [3, 4, 5, 6, 7, 8]                                   # eos accepted mid-run: nothing behind it
    out, rep, _ = _run(truth2, prompt, D=7, max_new=11)
    assert out == truth2[:11] and rep["tokens"] == 11                  # budget reached mid-run
    out, rep, _ = _run(truth2, prompt, D=7, max_new=1)
    assert out == truth2[:1] and rep["steps"] == 0
    out, rep, _ = _run([8] + truth2, prompt, D=3, max_new=9, eos=[8])
    assert out == [8]                                                  # the first token already ends it


def test_loop_never_lets_a_slot_reach_max_ctx():
    prompt = [3, 4, 5, 6] * 10
    truth = [3, 4, 5, 6] * 40
    for D in (1, 3, 7):
        max_ctx = len(prompt) + 64 + D                                 # the tightest cache draft_slots admits
        assert spec.draft_slots(D, 2, n_seq=1, greedy=True, num_beams=1, streamer=None, stopping_criteria=None, tp_size=1, max_batch=8,
                                prompt_len=len(prompt), max_new=64, max_ctx=max_ctx) == D
        out, rep, eng = _run(truth, prompt, D=D, max_new=64, max_ctx=max_ctx, sync_every=16)
        assert out == truth[:64] and eng.max_slot <= max_ctx - 1
        with pytest.raises(ValueError):
            _run(truth, prompt, D=D, max_new=64, max_ctx=max_ctx - 1)
