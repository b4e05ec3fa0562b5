#!/usr/bin/env python
"""Beam-search decode step against the greedy step at the same row count: 32-layer synthetic Zephyr-7B, one text prompt of
S = 2048 ids (configs[2]-shaped), 128 new tokens, eos disabled (every step runs).  ms per step = (end - first step on the host) / 127.
    python tools/bench_beam.py [--nb 1,2,4,8] [--layers 32] [--reps 2] [--legs proc,rows] [--no-greedy]
--legs adds beam legs beside the plain one: `proc` = logits processors armed (repetition_penalty 1.2 +
no_repeat_ngram_size 3: log-prob rows, the processor kernel, the select on rows, the history reorder), `rows` = the processed rows
recorded (output_scores: log-prob rows, one copy of [nb, V] per step into the ring, the select on rows; the host drains the ring at
every sync, which is part of the figure)."""
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
ap.add_argument("--nb", default="1,2,4,8")
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--S", type=int, default=2048)
ap.add_argument("--new", type=int, default=128)
ap.add_argument("--out", default="")
ap.add_argument("--legs", default="")
ap.add_argument("--no-greedy", action="store_true")
a = ap.parse_args()

from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM  # noqa: E402
hf = VisZephyrConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=a.layers, num_attention_heads=32, num_key_value_heads=8,
                     vocab_size=32000, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2, bos_token_id=1)
hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
hf.mm_patch_merge_type = "flat"
hf.mm_hidden_size = 5120
NBS = [int(v) for v in a.nb.split(",")]
model = VisZephyrForCausalLM.from_synthetic(hf, seed=0, device="cuda:0", max_batch=max(NBS), max_ctx=a.S + a.new + 16, max_tiles=1,
                                            max_text=64)
ids = synth.synth_ids(a.S, 32000, image_pos=-1, seed=7).unsqueeze(0).cuda()


def per_step(**kw):
    best = 1e9
    for _ in range(a.reps + 1):                   # the first run captures the graph
        tm = {}
        out = model.generate(max_new_tokens=a.new, eos_token_id=[], pad_token_id=2, timing=tm, **kw)
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - tm["t_first_token"]) / (a.new - 1))
    return best * 1e3, out


LEGS = {"proc": dict(repetition_penalty=1.2, no_repeat_ngram_size=3, beam_extended=True),
        "rows": dict(return_dict_in_generate=True, output_scores=True, beam_extended=True)}
rows = []
for nb in NBS:
    r = dict(nb=nb)
    if not a.no_greedy:
        greedy, _ = per_step(input_ids=ids.expand(nb, -1).contiguous(), do_sample=False)
        r.update(greedy_ms_per_step=round(greedy, 4))
    if nb > 1:
        beam, out = per_step(input_ids=ids, num_beams=nb)
        assert out.shape == (1, a.new)
        r.update(beam_ms_per_step=round(beam, 4))
        if not a.no_greedy:
            r.update(beam_over_greedy=round(beam / greedy, 4))
        for leg in [v for v in a.legs.split(",") if v]:
            ms, _ = per_step(input_ids=ids, num_beams=nb, **LEGS[leg])
            r.update({f"beam_{leg}_ms_per_step": round(ms, 4), f"beam_{leg}_added_us": round((ms - beam) * 1e3, 1)})
    rows.append(r)
    print(json.dumps(r), flush=True)
if a.out:
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(layers=a.layers, S=a.S, new_tokens=a.new, rows=rows), f, indent=1)
