#!/usr/bin/env python
"""Prompt-lookup speculative decoding: what a verify step of R = D + 1 rows costs against the plain 1-row step and against the batched
greedy step of R independent rows (the code path that existed before), on a 32-layer synthetic Zephyr-7B with a text prompt of S = 2048
ids, eos off, bf16 and e4m3 weights in ONE process.

Per (weights, D): N verify steps at acceptance 1 emit T = N * (D + 1) ids, so every variant decodes over the same context range - a call
of T ids that warms up and captures the graph, then a timed call over the next T ids (device events around the call; plain / batched /
acceptance 0: T steps, acceptance 1: N steps).  Drafts come from an id stream (draft source 1): all wrong for acceptance 0 - whose output
is the true continuation that acceptance 1 is then fed with.  The variants alternate and the whole series runs `--series` times.  The
decode attention's split count is pinned (knob 10 = 32, the partition every context above 2048 keys gets anyway) so that no call has to
capture a second graph inside its timed part.
    python tools/bench_spec.py [--D 1,3,7] [--steps 100] [--series 2] [--layers 32] [--out profiles/spec_bench.json]

--sample: the sampled mode instead (temperature 0.7, top-k 50, top-p 0.9, one seed), same model and protocol.  Per (weights, D): the
plain SAMPLED 1-row step (`set_sampling`), the greedy verify step, and the sampled verify step at acceptance 0 (an id stream that is
always wrong: the ids of a first run + 1) and at acceptance 1 (the ids of that run fed back as the stream, same seed)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-zephyr_amd"))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from vz_hip import binding as B  # noqa: E402
from vz_hip import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--D", default="1,3,7")
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--series", type=int, default=2)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--S", type=int, default=2048)
ap.add_argument("--weights", default="bf16,e4m3")
ap.add_argument("--out", default="")
ap.add_argument("--sample", action="store_true", help="the sampled legs: plain sampled step, greedy verify, sampled verify at acceptance 0 / 1")
a = ap.parse_args()

from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM  # noqa: E402
DS = [int(v) for v in a.D.split(",")]
N = a.steps
MAX_CTX = 4096
assert a.S + 2 * N * (max(DS) + 1) + max(DS) + 1 <= MAX_CTX, "two calls of N * (D + 1) ids must fit the cache"
B.tune("attn_nsplit", 32)


def make(fp8):
    hf = VisZephyrConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=a.layers, num_attention_heads=32, num_key_value_heads=8,
                         vocab_size=32000, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2, bos_token_id=1)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    hf.mm_hidden_size = 5120
    return VisZephyrForCausalLM.from_synthetic(hf, seed=0, device="cuda:0", max_batch=8, max_ctx=MAX_CTX, max_tiles=1, max_text=64,
                                               weight_fp8=fp8).engine


ids = synth.synth_ids(a.S, 32000, image_pos=-1, seed=7).unsqueeze(0)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def prefill(eng, rows, sample=None):
    emb = eng.embed_tokens(ids.expand(rows, -1).contiguous())
    _, last = eng.prefill(emb, [a.S] * rows, all_logits=False, last_logits=True)
    if sample is not None:          # token 0 of a sampled sequence: one draw with counter 0
        return int(B.sample(last[0:1].contiguous(), sample.temperature, sample.top_k, sample.top_p, sample.seed, 0, sample.warp)[0])
    return int(last[0].argmax())


def greedy_rows(eng, rows, T):
    """the plain tail: `rows` independent copies of the prompt, T steps to warm up, T steps timed"""
    first = prefill(eng, rows)
    eng.decode_begin(torch.tensor([first] * rows, dtype=torch.int32), [a.S] * rows, [a.S] * rows)
    eng.decode_steps(T)
    ms, _ = timed(lambda: eng.decode_steps(T))
    eng.check_async()
    return ms / T


def sampled_row(eng, T, par):
    """the plain SAMPLED tail on one row: T steps to warm up, T steps timed"""
    first = prefill(eng, 1, par)
    eng.set_sampling(True, par.temperature, par.top_k, par.top_p, par.seed, 1, par.warp)
    try:
        eng.decode_begin(torch.tensor([first], dtype=torch.int32), [a.S], [a.S])
        eng.decode_steps(T)
        ms, _ = timed(lambda: eng.decode_steps(T))
        eng.check_async()
        return ms / T
    finally:
        eng.set_sampling(False)


def verify(eng, D, n, stream, budget, sample=None):
    """verify steps fed from `stream`: n steps to warm up, n steps timed -> (ms per step, ids of both calls, ids per timed step);
    sample (vz_hip.sample_rows.RowParams): sampled verify steps"""
    first = prefill(eng, 1, sample)
    R = D + 1
    eng.decode_begin(torch.tensor([first] + [0] * D, dtype=torch.int32), [a.S + i for i in range(R)], [a.S + i for i in range(R)])
    eng.set_spec(True, D=D, history=[first], budget=budget, source=1, stream=stream, sample=sample)
    try:
        warm = eng.decode_steps(n).tolist()
        ms, got = timed(lambda: eng.decode_steps(n))
        eng.check_async()
        return ms / n, warm + got.tolist(), got.numel() / n
    finally:
        eng.set_spec(False)


engines = {w: make(w == "e4m3") for w in a.weights.split(",")}
rows = []
for series in range(a.series):
    for w, eng in engines.items():
        for D in DS:
            R, T = D + 1, N * (D + 1)
            if a.sample:
                from vz_hip.sample_rows import RowParams
                par = RowParams(True, 0.7, 50, 0.9, 1234, 0)
                plain = sampled_row(eng, T, par)
                greedy0, _, _ = verify(eng, D, T, [0] * (2 * T), 2 * T)
                _, truth, _ = verify(eng, D, T, [0] * (2 * T), 2 * T, par)         # a first run: the ids of this seed
                acc0, ids0, per0 = verify(eng, D, T, [(t + 1) % eng.cfg.vocab for t in truth], 2 * T, par)
                acc1, ids1, per1 = verify(eng, D, N, truth, 2 * T, par)
                r = dict(series=series, weights=w, D=D, rows=R, sampled=True, steps_timed=dict(plain=T, greedy_verify=T, accept0=T, accept1=N),
                         plain_sampled_ms=round(plain, 4), greedy_verify_ms=round(greedy0, 4), verify_accept0_ms=round(acc0, 4),
                         verify_accept1_ms=round(acc1, 4), ids_per_step_accept0=round(per0, 3), ids_per_step_accept1=round(per1, 3),
                         same_ids=ids0 == truth and ids1 == truth[:len(ids1)], sampled_over_greedy_verify=round(acc0 / greedy0, 4),
                         accept1_over_accept0=round(acc1 / acc0, 4), plain_tok_s=round(1e3 / plain, 1), accept0_tok_s=round(1e3 * per0 / acc0, 1),
                         accept1_tok_s=round(1e3 * per1 / acc1, 1), break_even_ids_per_step=round(max(acc0, acc1) / plain, 4))
                rows.append(r)
                print(json.dumps(r), flush=True)
                continue
            plain = greedy_rows(eng, 1, T)
            batched = greedy_rows(eng, R, T)
            acc0, truth, per0 = verify(eng, D, T, [0] * (2 * T), 2 * T)            # id 0 is never the argmax here: every guess is wrong
            acc1, ids1, per1 = verify(eng, D, N, truth, 2 * T)
            r = dict(series=series, weights=w, D=D, rows=R, steps_timed=dict(plain=T, batched=T, accept0=T, accept1=N),
                     plain_ms=round(plain, 4), batched_ms=round(batched, 4), verify_accept0_ms=round(acc0, 4), verify_accept1_ms=round(acc1, 4),
                     ids_per_step_accept0=round(per0, 3), ids_per_step_accept1=round(per1, 3), same_ids=ids1 == truth[:len(ids1)],
                     plain_tok_s=round(1e3 / plain, 1), accept0_tok_s=round(1e3 * per0 / acc0, 1), accept1_tok_s=round(1e3 * per1 / acc1, 1),
                     verify_over_batched=round(acc1 / batched, 4), verify_over_plain=round(acc1 / plain, 4),
                     break_even_ids_per_step=round(max(acc0, acc1) / plain, 4))
            rows.append(r)
            print(json.dumps(r), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(layers=a.layers, S=a.S, steps=N, series=a.series, note="ms per step from device events around the timed call",
                       rows=rows), f, indent=1)
