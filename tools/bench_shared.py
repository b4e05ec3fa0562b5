#!/usr/bin/env python
"""`generate(do_sample=True, num_return_sequences=n, share_prompt_kv=True)` against the copy route: synthetic
Zephyr-7B, G text prompts of S ids, n samples each, eos disabled.  Two numbers per shape and arm:
  start_ms     wall time of a call with max_new_tokens = 2: prefill, first tokens, the copy route's KV copies (or none), one step, readback
  ms_per_step  (wall of a call with 2 + K tokens - start) / K
One process measures one tree: --tree names a checkout (default: this one) whose vz_hip / vis_zephyr / built library are used, so the
same tool times the parent commit's step, built side by side, from this tree's tools/.  --share 1 passes share_prompt_kv=True.
    python tools/bench_shared.py --share 1 [--layers 32] [--shapes 4x16x2048,1x64x2048,8x2x200] [--steps 32] [--reps 3]
    python tools/bench_shared.py --alternate PARENT_TREE [--rounds 3]     (this tree armed and PARENT_TREE's copy route, in turn, a fresh
                                                                           process each, same device, plus this tree's copy route once;
                                                                           prints every run and the medians)
    python tools/bench_shared.py --share 1 --trace-leg 4x16x2048          (one short call alone: the leg to put under a kernel trace)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=HERE)
ap.add_argument("--share", type=int, default=0)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--shapes", default="4x16x2048,1x64x2048,8x2x200")
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--alternate", default="", help="a second checkout: its copy route against this tree's armed route, in turn")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--trace-leg", default="", help="GxNxS: one warm-up call and one 9-token call of that shape, nothing else")
a = ap.parse_args()

if a.alternate:
    runs = {"share": [], "copy_here": [], "copy_parent": []}
    arms = [("share", HERE, 1), ("copy_parent", a.alternate, 0), ("copy_here", HERE, 0)]
    for rnd in range(a.rounds):
        for name, tree, share in (arms if rnd == 0 else arms[:2]):      # this tree's copy route once: the trace shows it is the parent's step
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--share", str(share), "--layers", str(a.layers),
                                  "--shapes", a.shapes, "--steps", str(a.steps), "--reps", str(a.reps)], capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                sys.exit(f"{name} (round {rnd}) failed with exit {out.returncode}:\n{out.stderr[-2000:]}")
            r = json.loads(out.stdout.strip().splitlines()[-1])
            runs[name].append(r)
            print(f"round {rnd} {name}: {json.dumps(r['shapes'])}", flush=True)
    print(f"\nlayers {a.layers}, {a.steps} steps per timed call, {a.reps} calls per process (min), {a.rounds} processes per arm - copy_here one (median [min .. max])")
    print(f"{'shape GxNxS':>12} {'arm':>12} {'ms/step':>26} {'start ms (2 tokens)':>30}")
    for shape in a.shapes.split(","):
        for name in runs:
            st = [r["shapes"][shape]["ms_per_step"] for r in runs[name]]
            s0 = [r["shapes"][shape]["start_ms"] for r in runs[name]]
            f = lambda v: f"{statistics.median(v):9.3f} [{min(v):8.3f} .. {max(v):8.3f}]"      # noqa: E731
            print(f"{shape:>12} {name:>12} {f(st)} {f(s0)}")
    sys.exit(0)

sys.path.insert(0, os.path.join(a.tree, "vision-zephyr_amd"))
sys.path.insert(0, a.tree)
import torch  # noqa: E402

from vz_hip import synth  # noqa: E402
from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM  # noqa: E402

shapes = [tuple(int(v) for v in s.split("x")) for s in (a.trace_leg or a.shapes).split(",")]
new_max = 2 + a.steps
hf = VisZephyrConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=a.layers, num_attention_heads=32, num_key_value_heads=8,
                     vocab_size=32000, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2, bos_token_id=1)
hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
hf.mm_patch_merge_type = "flat"
hf.mm_hidden_size = 5120
model = VisZephyrForCausalLM.from_synthetic(hf, seed=0, device="cuda:0", max_batch=max(g * n for g, n, _ in shapes),
                                            max_ctx=max(s for _, _, s in shapes) + new_max + 16, max_tiles=1, max_text=64)
extra = dict(share_prompt_kv=True) if a.share else {}


def wall(ids, n, new):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.generate(input_ids=ids, do_sample=True, temperature=0.9, top_p=0.95, seed=11, num_return_sequences=n, max_new_tokens=new,
                         eos_token_id=[], pad_token_id=2, **extra)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (ids.shape[0] * n, new)
    return (time.perf_counter() - t0) * 1e3


res = {}
for g, n, s in shapes:
    ids = torch.stack([synth.synth_ids(s, 32000, image_pos=-1, seed=7 + i) for i in range(g)]).cuda()
    if a.trace_leg:
        wall(ids, n, 9)
        wall(ids, n, 9)
        continue
    wall(ids, n, new_max)                                             # (captures the step's graph)
    start = min(wall(ids, n, 2) for _ in range(a.reps))
    full = min(wall(ids, n, new_max) for _ in range(a.reps))
    res[f"{g}x{n}x{s}"] = dict(start_ms=round(start, 3), ms_per_step=round((full - start) / a.steps, 4))
print(json.dumps(dict(tree=a.tree, share=a.share, layers=a.layers, steps=a.steps, shapes=res)), flush=True)
