"""The pieces every host route of `generate()` shares (vz_hip/decode_loop.py) on the CPU, against the toy engine of
tests/test_stream_host_cpu.py: the row loop for one row and with device-decided stops, the arming scope's order, the fan-out of a
prompt over n cache rows, and running a route in parts."""
import itertools
import types

import pytest
import torch

from test_stream_host_cpu import ToyBatchEngine, ToyEngine, V, next_token, solo
from vz_hip import decode_loop as DL

PAD = 250


def _prompt(seed, L=7, distinct=12):
    """a prompt whose first `distinct` free-running tokens are all different (so "the eos id" names one position)"""
    for s in range(seed, seed + 1000):
        p = torch.randint(1, V, (L,), generator=torch.Generator().manual_seed(s)).tolist()
        free = solo(p, distinct, set())
        if len(set(free)) == distinct and PAD not in free:
            return p, free
    raise AssertionError("no such prompt")


class LoopEngine(ToyBatchEngine):
    """+ what the row loop touches: the sizes of the decode_steps calls, a stop matcher that reports a fixed index per row, a recorder"""

    def __init__(self, max_batch, at=None):
        super().__init__(max_batch)
        self.at, self.step_calls = at, []

    def decode_steps(self, n):
        self.step_calls.append(n)
        return super().decode_steps(n)

    def stop_at(self, row0, rows):
        return torch.tensor(self.at[row0:row0 + rows], dtype=torch.int32)

    def scores_steps(self, n):
        return torch.zeros(n, self.dec_B, 4), None, None


def _armed_rows(eng, prompts):
    """the prompts prefilled into rows 0.., their first tokens armed: what a route has done when it enters the row loop"""
    S = max(len(p) for p in prompts)
    emb = torch.zeros(len(prompts), S, 1, dtype=torch.bfloat16)
    for i, p in enumerate(prompts):
        emb[i, :len(p), 0] = torch.tensor(p, dtype=torch.bfloat16)
    lens = [len(p) for p in prompts]
    first = eng.prefill(emb, lens)[1].argmax(-1).to(torch.int32)
    eng.decode_begin(first, lens, lens)
    return first.to(torch.long)


@pytest.mark.parametrize("case", ["first", "mid", "chunk_end", "none", "stop_first", "stop_mid"])
@pytest.mark.parametrize("max_new", [1, 2, 9])
@pytest.mark.parametrize("sync_every", [1, 4, 16])
def test_row_loop_one_row_equals_solo(sync_every, max_new, case):
    prompt, free = _prompt(3)
    at = {"first": 0, "mid": 2, "chunk_end": min(sync_every, 8), "none": None, "stop_first": 0, "stop_mid": 2}[case]      # chunk 1 = the tokens 1 .. sync_every
    stop = case.startswith("stop")            # the row ends at token `at` because the matcher says so, not because of what the token is
    eos = set() if at is None or stop else {free[at]}
    eng = LoopEngine(1, at=[at])
    out = DL.decode_rows(eng, _armed_rows(eng, [prompt]), max_new, eos, PAD, sync_every, None, stop)
    want = solo(prompt, max_new, {free[at]} if stop else eos)
    assert out.shape[0] == 1 and out[0].tolist() == want
    if at is None:        # nothing to look at: one chunk
        assert eng.step_calls == ([max_new - 1] if max_new > 1 else [])
    else:                 # sync_every-sized chunks up to the one that holds the row's last token
        steps = len(want) - 1
        full, rest = divmod(max_new - 1, sync_every)
        assert eng.step_calls == ([sync_every] * full + ([rest] if rest else []))[:-(-steps // sync_every)]


def test_row_loop_stops_per_row():
    (p0, f0), (p1, f1), (p2, f2) = _prompt(11), _prompt(2000, L=4), _prompt(4000, L=9)
    eos = {f2[9]}
    assert eos.isdisjoint(f0[:1] + f1[:7] + f2[:9])           # rows 0 and 1 end by their stop, row 2 by eos at its token 9
    eng = LoopEngine(3, at=[0, 6, -1])                          # stopped on token 0 | mid-way through chunk 2 (tokens 5..8) | never
    from vz_hip import scores as SC
    blk = SC.Sink(1).block(3)
    out = DL.decode_rows(eng, _armed_rows(eng, [p0, p1, p2]), 20, eos, PAD, 4, blk, True)
    kept = [1, 7, 10]
    assert out.shape == (3, 10)                                 # cut inside chunk 3 (tokens 9..12), after the step that finished row 2
    for row, f, k in zip(out.tolist(), (f0, f1, f2), kept):
        assert row[:k] == f[:k] and all(t == PAD for t in row[k:])
    assert blk.ends.tolist() == kept
    assert eng.step_calls == [4, 4, 4] and sum(c.shape[0] for c in blk.rec) == 12


class RecordingEngine:
    """records every method called on it; `fail` = (name, k): the k-th call of that name (or of any `set_*` for name "set_") raises"""

    def __init__(self, fail=None):
        self.log, self.fail, self.count = [], fail, 0

    def __getattr__(self, name):
        def call(*args):
            self.log.append((name,) + args)
            if self.fail is not None and name.startswith(self.fail[0]):
                self.count += 1
                if self.count == self.fail[1]:
                    raise RuntimeError(f"{name} failed")
        return call


ORDER = [("proc", "set_logits_proc"), ("sampling_rows", "set_sampling_rows"), ("scores", "set_scores"), ("stop", "set_stop")]
ASKED = {"proc": "PROC", "sampling_rows": ["ROW0", "ROW1"], "scores": (4, 2, True, False), "stop": "PLAN"}
SUBSETS = [s for k in range(5) for s in itertools.combinations(range(4), k)]


def _on(key, name):
    return (name,) + (ASKED[key] if key == "scores" else (ASKED[key],))


@pytest.mark.parametrize("subset", SUBSETS)
@pytest.mark.parametrize("fail", [None, ("decode_steps", 1), ("set_", 3)])
def test_arming_scope_order(subset, fail):
    asked = [ORDER[i] for i in subset]
    if fail == ("set_", 3) and len(asked) < 3:
        fail = None                          # fewer than three armings: the third `set_*` call would be a disarming
    eng = RecordingEngine(fail)
    first = torch.tensor([5, 6], dtype=torch.int32)

    def run():
        with DL.armed(eng, **{key: ASKED[key] for key, _ in asked}) as begin:
            begin(first, [3, 4], [3, 4])
            eng.decode_steps(1)

    raises = fail is not None
    if raises:
        with pytest.raises(RuntimeError):
            run()
    else:
        run()
    in_entry = raises and fail[0] == "set_"
    on = [_on(key, name) for key, name in asked]
    armed = asked[:2] if in_entry else asked
    body = [] if in_entry else [("decode_begin", first, [3, 4], [3, 4])] + ([("stop_rows", 0, first)] if ("stop", "set_stop") in asked else []) \
        + [("decode_steps", 1)]
    off = [(name, None) for _, name in reversed(armed)]
    assert eng.log == (on[:3] if in_entry else on) + body + off          # the documented order in, the armed set in reverse out, nothing else


def test_plain_call_touches_no_filter():
    eng = RecordingEngine()
    with DL.armed(eng) as begin:
        begin(torch.tensor([1]), [2], [2])
    assert [c[0] for c in eng.log] == ["decode_begin"]


class FanEngine(ToyEngine):
    """+ the fan-out surface: a prompt's KV copied from its first row into parked rows of the batch, then the real decode_begin"""
    tp_size = 1

    def __init__(self, max_batch):
        super().__init__(max_batch)
        self.begins, self.tables = [], []

    def kv_move_rows(self, src, dst, lens):
        for s_, d_, n in zip(src, dst, lens):
            assert self.cur[d_] is None and d_ < self.dec_B
            self.rows[d_] = list(self.rows[s_][:n])
        self.moves.append((tuple(src), tuple(dst), tuple(lens)))

    def decode_begin(self, first_ids, next_pos, ctx_len):
        if all(c == 0 for c in ctx_len):
            return super().decode_begin(first_ids, next_pos, ctx_len)      # every row parked
        self.begins.append((list(next_pos), list(ctx_len)))
        for b in range(len(ctx_len)):
            assert len(self.rows[b]) == ctx_len[b], "armed with a context that is not the prompt's"
        self.cur = [int(t) for t in first_ids.tolist()] + [None] * (self.max_batch - len(ctx_len))

    def set_sampling_rows(self, params):
        self.tables.append(params)


def _embeds(prompts):
    emb = torch.zeros(len(prompts), max(len(p) for p in prompts), 1, dtype=torch.bfloat16)
    for i, p in enumerate(prompts):
        emb[i, :len(p), 0] = torch.tensor(p, dtype=torch.bfloat16)
    return emb


@pytest.mark.parametrize("with_pos", [False, True])
def test_fan_out_rows_moves_and_positions(with_pos):
    prompts = [_prompt(1, L=5)[0], _prompt(50, L=9)[0]]
    lens, n = [5, 9], 3
    pos = torch.stack([torch.arange(9) + 10 * (g + 1) for g in range(2)]) if with_pos else None
    eng = FanEngine(6)
    last = DL.fan_prefill(eng, _embeds(prompts), lens, pos, n)
    assert eng.prefill_shapes == [(0, 1, 5), (3, 1, 9)] and eng.dec_B == 6 and not eng.moves
    assert last.shape == (2, V) and last.argmax(-1).tolist() == [next_token(p) for p in prompts]
    next_pos, ctx_len = DL.fan_spread(eng, lens, pos, n)
    assert eng.moves == [((0, 0, 3, 3), (1, 2, 4, 5), (5, 5, 9, 9))]
    assert ctx_len == [5, 5, 5, 9, 9, 9]
    assert next_pos == ([15, 15, 15, 29, 29, 29] if with_pos else ctx_len)
    assert [eng.rows[r] for r in range(6)] == [prompts[0]] * 3 + [prompts[1]] * 3


def test_samples_in_parts_draw_their_own_seeds(monkeypatch):
    """5 prompts x 3 samples on 6 cache rows: parts of 2 prompts, and row j of prompt b draws under row_seed(seed, b, n, j) whichever
    part it lands in; the first part stamps the timing."""
    from vis_zephyr.model import VisZephyrForCausalLM
    from vz_hip import binding as B
    from vz_hip import sample_rows as SR
    drawn = []

    def sample_rows(logits, params):
        drawn.append([p.seed for p in params])
        assert all(p.sample and p.counter == 0 for p in params)
        return logits.argmax(-1).to(torch.int32)
    monkeypatch.setattr(B, "sample_rows", sample_rows)
    prompts = [_prompt(100 * i, L=3 + i)[0] for i in range(5)]
    lens, n, seed, max_new = [len(p) for p in prompts], 3, 1000, 6
    eng = FanEngine(6)
    me = types.SimpleNamespace(engine=eng, device=torch.device("cpu"))
    me._generate_samples = types.MethodType(VisZephyrForCausalLM._generate_samples, me)
    timing = {}
    out = me._generate_samples(_embeds(prompts), lens, None, n, max_new, 0.7, 50, 1.0, seed, set(), PAD, 4, timing)
    want = [[SR.row_seed(seed, b, n, j) for b in part for j in range(n)] for part in ([0, 1], [2, 3], [4])]
    assert drawn == want
    assert [[p.seed for p in t] for t in eng.tables if t is not None] == want and all(p.counter == 1 for t in eng.tables if t for p in t)
    assert eng.tables[1::2] == [None] * 3                         # every part disarmed its table
    assert [c for _, c in eng.begins] == [[3, 3, 3, 4, 4, 4], [5, 5, 5, 6, 6, 6], [7, 7, 7]]
    assert out.shape == (15, max_new) and "t_first_token" in timing
    for b, p in enumerate(prompts):                               # the toy "sampler" is the argmax: every sample is the solo sequence
        for j in range(n):
            assert out[b * n + j].tolist() == solo(p, max_new, set())


def test_parts_pad_and_stamp_once():
    widths, stamps = {0: 3, 2: 5, 4: 2}, []

    def route(lo, hi, tm):
        stamps.append(tm)
        if tm is not None:
            tm["t_first_token"] = tm.get("t_first_token", 0) + 1
        return torch.full((hi - lo, widths[lo]), lo + 1, dtype=torch.long)
    timing = {}
    out = DL.run_parts(route, 5, 2, PAD, torch.device("cpu"), timing)
    assert stamps == [timing, None, None] and timing == {"t_first_token": 1}
    assert out.tolist() == [[1, 1, 1, PAD, PAD]] * 2 + [[3] * 5] * 2 + [[5, 5, PAD, PAD, PAD]]
    one = torch.arange(6).view(2, 3)
    assert DL.run_parts(lambda lo, hi, tm: one, 2, 2, PAD, torch.device("cpu")) is one      # within capacity: the route's own tensor


def test_batch_beyond_the_cache_rows_stamps_the_first_token(monkeypatch):
    from vis_zephyr.model import VisZephyrForCausalLM
    from vz_hip import binding as B
    monkeypatch.setattr(B, "argmax", lambda logits: logits.argmax(-1).to(torch.int32))
    prompts = [_prompt(10 * i, L=4 + i)[0] for i in range(5)]
    eng = ToyBatchEngine(2)
    me = types.SimpleNamespace(engine=eng, device=torch.device("cpu"))
    me._generate_batched = types.MethodType(VisZephyrForCausalLM._generate_batched, me)
    timing = {}
    out = me._generate_batched(_embeds(prompts), [len(p) for p in prompts], None, 5, set(), PAD, 4, timing)
    assert "t_first_token" in timing and out.tolist() == [solo(p, 5, set()) for p in prompts]


def test_call_defaults_keep_the_callers_eos_order():
    gen = types.SimpleNamespace(eos_token_id=[9, 2], pad_token_id=None)
    d = DL.resolve_defaults(gen, None, None, 30, 12)
    assert (d.eos_list, d.eos, d.max_new, d.pad, d.fill) == ([9, 2], {2, 9}, 18, None, 2)
    d = DL.resolve_defaults(gen, 7, 4, 30, 12, 0)
    assert (d.eos_list, d.max_new, d.pad, d.fill) == ([7], 4, 0, 0)
    d = DL.resolve_defaults(types.SimpleNamespace(eos_token_id=None))
    assert (d.eos_list, d.eos, d.max_new, d.fill) == ([], set(), 20, 0)
