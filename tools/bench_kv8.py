#!/usr/bin/env python
"""The decode step with the e4m3 KV mirror on (`kv_fp8=True`) against the plain step: synthetic Zephyr-7B, B rows of
different text prompts of S ids each, greedy, the captured step replayed.  Per shape BxS: the B rows are prefilled once (groups of 4 rows),
then one warm-up call (captures the step's graph) and min over --reps of
  ms_per_step  wall of K replayed steps / K (decode_steps(K) between two device synchronisations; decode_begin, which restarts every call at
               context S, is outside the timed span)
One process measures one arm of one tree: --tree names a checkout (default: this one) whose vz_hip / vis_zephyr / built library are used,
so the same tool times or traces the parent commit's step (plain arm only: it has no keyword).
    python tools/bench_kv8.py --kv-fp8 1 [--layers 32] [--shapes 64x2048,16x2048,64x200,1x2048] [--steps 32] [--reps 3]
    python tools/bench_kv8.py --alternate [--rounds 3]      (a kv_fp8 engine and a plain engine in turn, a fresh process each under its
                                                             own time limit, same device; prints every run and the medians; stops at the
                                                             first process that fails)
    python tools/bench_kv8.py --kv-fp8 1 --trace-leg 64x2048   (the prefill and two 9-step calls alone: the leg to put under a kernel trace)"""
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
ap.add_argument("--kv-fp8", type=int, default=0)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--shapes", default="64x2048,16x2048,64x200,1x2048")
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--alternate", action="store_true", help="both arms in turn, a fresh process each")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--limit", type=int, default=240, help="seconds one process of --alternate may take")
ap.add_argument("--trace-leg", default="", help="BxS: the prefill and two 9-step calls of that shape, nothing else")
a = ap.parse_args()

if a.alternate:
    runs = {"kv_fp8": [], "plain": []}
    for rnd in range(a.rounds):
        for name, on in (("kv_fp8", 1), ("plain", 0)):
            out = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--kv-fp8", str(on), "--layers", str(a.layers),
                                  "--shapes", a.shapes, "--steps", str(a.steps), "--reps", str(a.reps)], capture_output=True, text=True)
            if out.returncode != 0:
                sys.exit(f"{name} (round {rnd}) failed with exit {out.returncode}; nothing more is started:\n{out.stderr[-2000:]}")
            r = json.loads(out.stdout.strip().splitlines()[-1])
            runs[name].append(r)
            print(f"round {rnd} {name}: {json.dumps(r['shapes'])}", flush=True)
    print(f"\nlayers {a.layers}, {a.steps} steps per timed call, {a.reps} calls per process (min), {a.rounds} processes per arm (median [min .. max])")
    print(f"{'shape BxS':>12} {'arm':>8} {'ms/step':>30}   kv_fp8 / plain")
    for shape in a.shapes.split(","):
        med = {}
        for name in runs:
            st = [r["shapes"][shape]["ms_per_step"] for r in runs[name]]
            med[name] = statistics.median(st)
            print(f"{shape:>12} {name:>8} {med[name]:9.4f} [{min(st):8.4f} .. {max(st):8.4f}]" + (f"   {med['kv_fp8'] / med['plain']:.3f}" if name == "plain" else ""))
    sys.exit(0)

sys.path.insert(0, os.path.join(a.tree, "vision-zephyr_amd"))
sys.path.insert(0, a.tree)
import torch  # noqa: E402

from vz_hip import synth  # noqa: E402
from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM  # noqa: E402

shapes = [tuple(int(v) for v in s.split("x")) for s in (a.trace_leg or a.shapes).split(",")]
hf = VisZephyrConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=a.layers, num_attention_heads=32, num_key_value_heads=8,
                     vocab_size=32000, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2, bos_token_id=1)
hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
hf.mm_patch_merge_type = "flat"
hf.mm_hidden_size = 5120
max_batch, max_ctx = max(b for b, _ in shapes), max(s for _, s in shapes) + a.steps + 16
model = VisZephyrForCausalLM.from_synthetic(hf, seed=0, device="cuda:0", max_batch=max_batch, max_ctx=max_ctx, max_tiles=1, max_text=64, **(dict(kv_fp8=True) if a.kv_fp8 else {}))
eng = model.engine


def wall(first, B, S, n):
    eng.decode_begin(first, [S] * B, [S] * B)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.decode_steps(n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


res = {}
for B, S in shapes:
    first = []
    for b0 in range(0, B, 4):
        n = min(4, B - b0)
        ids = torch.stack([synth.synth_ids(S, 32000, image_pos=-1, seed=7 + b0 + i) for i in range(n)]).cuda()
        first.append(eng.prefill_rows(b0, eng.embed_tokens(ids), [S] * n).argmax(-1).to(torch.int32))
    first = torch.cat(first)
    if a.trace_leg:
        wall(first, B, S, 9)
        wall(first, B, S, 9)
        continue
    wall(first, B, S, a.steps)                                         # (captures the step's graph)
    full = min(wall(first, B, S, a.steps) for _ in range(a.reps))
    res[f"{B}x{S}"] = dict(ms_per_step=round(full / a.steps, 4), splits=eng.decode_info()[0])
mem = {}
if a.kv_fp8:
    from vz_hip import kv8  # noqa: E402
    mem = dict(cache_bytes=kv8.cache_bytes(eng.cfg, max_batch, max_ctx), mirror_bytes=kv8.mirror_bytes(eng.cfg, max_batch, max_ctx))
print(json.dumps(dict(tree=a.tree, kv_fp8=a.kv_fp8, layers=a.layers, steps=a.steps, shapes=res, **mem)), flush=True)
