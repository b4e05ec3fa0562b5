#!/usr/bin/env python
"""What the stop matcher costs per decode step, and what it buys: 32-layer synthetic Zephyr-7B, 64-id prompts.
    python tools/bench_stop.py [layers] [rounds]
Part 1, at 1 row and at 64 rows, alternating in one process (a) the matcher off, (b) `armed`: one stop string and one id sequence that
nothing the model emits can end - the common step, (c) `walk`: a table in which every token decodes to "a" and the stop string is "b" +
16 x "a", so every step stages 16 table rows and walks them without ever stopping, (d) `heads`: 16 id sequences of 32 ids whose newest id
is one row 0 emits (on 16 of the 63 steps a head matches and the 31 older ids of the sequence are fetched and compared; none matches).  Every window is 63 graph steps ended by a device
synchronise, behind an untimed window of the same leg that takes the graph capture; per leg the best and the median of `rounds` windows, the legs taken in turn inside every round so that drift hits them
alike; the spread of (a) is the run-to-run yardstick.  Part 2, the case the matcher exists for: 16 prompts, a KeywordsStoppingCriteria
that never fires, no streamer, 128 new tokens - items/s of the whole generate() call (prefill included) - and what arming costs the
host: `Engine.set_stop` with a new stop set and with the one the engine holds already.  On a tree without the
matcher (the parent commit) only leg (a) runs and part 2 takes the sequential host path.  Under `rocprofv3 --kernel-trace --stats` the
kernel of interest is stop_match_kernel (all legs together; run them apart with VZ_BENCH_STOP_LEGS=armed / walk / heads)."""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-zephyr_amd"))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from vz_hip import binding as Bd, synth  # noqa: E402

layers = int(sys.argv[1]) if len(sys.argv) > 1 else 32
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n_steps = 63
only = [s for s in os.environ.get("VZ_BENCH_STOP_LEGS", "").split(",") if s]


def build(max_batch):
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    hf = VisZephyrConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=layers, num_attention_heads=32,
                         num_key_value_heads=8, vocab_size=32000, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2,
                         bos_token_id=1)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    hf.mm_hidden_size = 5120
    return VisZephyrForCausalLM.from_synthetic(hf, seed=0, device="cuda:0", max_batch=max_batch, max_ctx=512, max_tiles=1, max_text=64)


class _Tok:
    """tokens decode to themselves (what tests/stop_ref.py uses): enough of a tokenizer for HF's StopStringCriteria constructor"""
    bos_token_id = None

    def __init__(self, tokens):
        self.tokens, self.vocab = list(tokens), {t: i for i, t in enumerate(tokens)}

    def get_vocab(self):
        return dict(self.vocab)

    def __call__(self, text, **kw):
        return {"input_ids": [self.vocab[text]]}

    def _convert_id_to_token(self, i):
        return self.tokens[i]

    def convert_tokens_to_string(self, tokens):
        return "".join(tokens)


def plans():
    from transformers.generation.stopping_criteria import StopStringCriteria
    from vz_hip import stop as ST
    # the common step: token i decodes to "<%05d>"; a two-token stop string no greedy run here emits, an id sequence that ends past the vocabulary
    wide = _Tok(["abcdef"] + ["<%05d>" % i for i in range(1, 32000)])
    quiet, _ = ST.parse(["<00007><00008>"], wide, None, token_sequences=[[5, 6, 40000]])
    # every step walks: the table row of "a" for every id, stop string "b" + 16 x "a"
    c = StopStringCriteria(_Tok(["abcdef", "a", "b"]), ["b" + "a" * 16])
    tabs = ST._string_tables(c)
    tabs["emb"] = torch.cat([c.embedding_vec[1:2].expand(32000, -1), c.embedding_vec[-1:]]).to(torch.int32).contiguous()
    return quiet, ST.Plan(**tabs)


model = build(64)
eng = model.engine
HAVE = hasattr(eng, "set_stop")
LEGS = [("off", None)]
if HAVE:
    quiet, walk = plans()

    def heads(ref):                      # built from the ids the `off` leg produced: row 0's tokens of steps 2, 5, 8, ... as the sequences' heads
        from vz_hip import stop as ST
        return ST.Plan(seqs=[([40000] * 31 + [int(ref[0, 2 + 3 * k])], 0) for k in range(16)])

    LEGS += [("armed", quiet), ("walk", walk), ("heads", heads)]
if only:
    LEGS = [leg for leg in LEGS if leg[0] == "off" or leg[0] in only]

for B in (1, 64):
    ids = torch.stack([synth.synth_ids(64, 32000, image_pos=-1, seed=10 + b) for b in range(B)]).cuda()
    _, last = eng.prefill(eng.embed_tokens(ids), [64] * B)
    first = Bd.argmax(last)
    out = torch.empty(B, n_steps, dtype=torch.int32, device="cuda:0")
    ts = {name: [] for name, _ in LEGS}
    ref = None
    for r in range(rounds + 1):          # round 0 warms every leg up (its graph capture)
        for name, plan in LEGS:
            if callable(plan):
                plan = plan(ref)
            if plan is not None:
                eng.set_stop(plan)
            try:
                # a leg that follows another one captures its graph again (the engine holds one): an untimed window first, so that the
                # timed one only replays - on every leg, and on the parent, alike
                for timed in (False, True):
                    eng.decode_begin(first, [64] * B, [64] * B)
                    if plan is not None:
                        eng.stop_rows(0, first)
                    if not timed:
                        eng.decode_steps(n_steps, out=out)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.decode_steps(n_steps, out=out)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / n_steps * 1e3
                if plan is not None:
                    assert eng.stop_at(0, B).tolist() == [-1] * B, f"{name}: a row stopped"
            finally:
                if plan is not None:
                    eng.set_stop(None)
            ref = out.clone() if ref is None else ref
            assert torch.equal(out, ref), f"{name}: the ids moved"
            if r:
                ts[name].append(dt)
    for name, _ in LEGS:
        v = sorted(ts[name])
        print(f"rows {B:2d} {name:6s}: best {v[0]:.4f} ms/step, median {v[len(v) // 2]:.4f}, worst {v[-1]:.4f} ({B / v[0] * 1e3:8.1f} tokens/s on the best)",
              flush=True)
    a = sorted(ts["off"])
    for name, _ in LEGS[1:]:
        v = sorted(ts[name])
        print(f"rows {B:2d} {name:6s} - off: {(v[0] - a[0]) * 1e3:+.1f} us/step on the best, {(v[len(v) // 2] - a[len(a) // 2]) * 1e3:+.1f} us on the median; "
              f"spread of off (worst - best) {(a[-1] - a[0]) * 1e3:.1f} us", flush=True)

# ---- part 2: 16 prompts with a keyword criterion, no streamer ------------------------------------------------------------------------------
if not only:
    from vis_zephyr.model.mm_utils import KeywordsStoppingCriteria
    ids = torch.stack([synth.synth_ids(64, 32000, image_pos=-1, seed=100 + b) for b in range(16)])

    class _Kw:                           # the keyword's ids: a pair no greedy run of this model ends in (checked below: every row runs to 128)
        bos_token_id = None

        def __call__(self, text):
            from types import SimpleNamespace
            return SimpleNamespace(input_ids=[31999, 31998])

    crit = KeywordsStoppingCriteria(["</s>"], _Kw(), torch.zeros(1, 0, dtype=torch.long))
    for r in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = model.generate(input_ids=ids, do_sample=False, max_new_tokens=128, eos_token_id=[], stopping_criteria=[crit])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert tuple(got.shape) == (16, 128)
        print(f"16 prompts x 128 new tokens, KeywordsStoppingCriteria, no streamer, run {r}: {dt:.3f} s = {16 / dt:.2f} items/s, "
              f"{16 * 128 / dt:.0f} tokens/s ({'device matcher, one batch' if HAVE else 'host path, one sequence at a time'})", flush=True)
    if HAVE:
        ts = []
        for plan in (quiet, walk, walk, walk, quiet, quiet):          # (tables of 32001 x 3 and 32001 x 17 words)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.set_stop(plan)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            eng.set_stop(None)
        print("Engine.set_stop, host ms per call (armed set, walk set x 3, armed set x 2; a repeated set uploads nothing): " +
              " ".join(f"{t:.3f}" for t in ts), flush=True)
