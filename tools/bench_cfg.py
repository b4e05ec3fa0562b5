#!/usr/bin/env python
"""The guided decode step (classifier-free guidance) against the plain steps it is made of: 32-layer synthetic
Zephyr-7B, one text prompt of S = 2048 ids, a 64-id negative prompt, 128 new tokens, eos disabled (every step runs).  ms per step =
(end - first token on the host) / 127.  Legs: the guided step (2 rows per weight sweep + combine + follow), the plain greedy 2-row step
of the same tree with the prompt in both rows (rows2) and with the prompt and the negative prompt as its two rows (rows2_short: the guided
step's own contexts, without guidance), the plain 1-row step (twice that = what two model calls per token cost).
    python tools/bench_cfg.py [--layers 32] [--reps 3] [--scale 1.5] [--out FILE]
    python tools/bench_cfg.py --only guided --new 24      (a short guided run alone: the leg to put under a kernel trace)"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-zephyr_amd"))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from vz_hip import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--S", type=int, default=2048)
ap.add_argument("--neg", type=int, default=64)
ap.add_argument("--new", type=int, default=128)
ap.add_argument("--scale", type=float, default=1.5)
ap.add_argument("--only", default="", help="guided | rows2 | rows2_short | rows1: that leg alone")
ap.add_argument("--out", default="")
a = ap.parse_args()

from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM  # noqa: E402
hf = VisZephyrConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=a.layers, num_attention_heads=32, num_key_value_heads=8,
                     vocab_size=32000, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2, bos_token_id=1)
hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
hf.mm_patch_merge_type = "flat"
hf.mm_hidden_size = 5120
model = VisZephyrForCausalLM.from_synthetic(hf, seed=0, device="cuda:0", max_batch=2, max_ctx=a.S + a.new + 16, max_tiles=1, max_text=64)
ids = synth.synth_ids(a.S, 32000, image_pos=-1, seed=7).unsqueeze(0).cuda()
neg = synth.synth_ids(a.neg, 32000, image_pos=-1, seed=8).unsqueeze(0).cuda()


def per_step(**kw):
    runs = []
    for _ in range(a.reps + 1):                   # the first run captures the graph
        tm = {}
        model.generate(max_new_tokens=a.new, eos_token_id=[], pad_token_id=2, do_sample=False, timing=tm, **kw)
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - tm["t_first_token"]) / (a.new - 1) * 1e3)
    return min(runs[1:] or runs), runs[1:] or runs


LEGS = {"guided": dict(input_ids=ids, guidance_scale=a.scale, negative_prompt_ids=neg),
        "rows2": dict(input_ids=ids.expand(2, -1).contiguous()),
        "rows2_short": dict(input_ids=torch.cat([ids, torch.nn.functional.pad(neg, (0, a.S - a.neg), value=2)]),
                            attention_mask=(torch.arange(a.S, device="cuda")[None, :] < torch.tensor([[a.S], [a.neg]], device="cuda")).long()),
        "rows1": dict(input_ids=ids)}
r = dict(layers=a.layers, S=a.S, negative=a.neg, new_tokens=a.new, scale=a.scale)
for leg in ([a.only] if a.only else list(LEGS)):
    best, runs = per_step(**LEGS[leg])
    r[f"{leg}_ms_per_step"] = round(best, 4)
    r[f"{leg}_runs_ms"] = [round(v, 4) for v in runs]
if not a.only:
    r["guided_minus_rows2_us"] = round((r["guided_ms_per_step"] - r["rows2_ms_per_step"]) * 1e3, 1)
    r["guided_minus_rows2_short_us"] = round((r["guided_ms_per_step"] - r["rows2_short_ms_per_step"]) * 1e3, 1)
    r["two_calls_ms_per_step"] = round(2 * r["rows1_ms_per_step"], 4)
    r["guided_over_two_calls"] = round(r["guided_ms_per_step"] / r["two_calls_ms_per_step"], 4)
print(json.dumps(r), flush=True)
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1)
