#!/usr/bin/env python
"""Batched greedy decode throughput: B text-only prompts of 64 ids, 64 new tokens each, Zephyr-7B shape.
    python tools/bench_batched.py [layers] [fp8]
    python tools/bench_batched.py [layers] --sample      the per-row sampling tail: step time at 16 and 64 rows with
                                                         every row sampling (T 0.7, top_k 50, top_p 0.9) next to the greedy step at the same rows
Under `rocprofv3 --kernel-trace --stats` the --sample leg's kernels of interest are sample_rows_kernel and argmax_kernel."""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-zephyr_amd"))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from bench import build_model  # noqa: E402
from vz_hip import synth  # noqa: E402

SAMPLE = "--sample" in sys.argv
sys.argv = [a for a in sys.argv if a != "--sample"]
layers = int(sys.argv[1]) if len(sys.argv) > 1 else 32
import bench  # noqa: E402


FP8 = len(sys.argv) > 2 and sys.argv[2] == "fp8"


def build(max_batch):
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    hf = VisZephyrConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=layers, num_attention_heads=32,
                         num_key_value_heads=8, vocab_size=32000, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2,
                         bos_token_id=1)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    hf.mm_hidden_size = 5120
    return VisZephyrForCausalLM.from_synthetic(hf, seed=0, device="cuda:0", max_batch=max_batch, max_ctx=512, max_tiles=1, max_text=64,
                                               weight_fp8=FP8)


model = build(64)
from vz_hip import binding as _B  # noqa: E402
_B.tune_from_args(os.environ.get("VZ_TUNE", ""))       # experiments: "knob=value,..." (names or numbers)
ROWS = [int(v) for v in os.environ.get("VZ_ROWS", "16,64" if SAMPLE else "1,2,4,8,16,32,48,64").split(",")]
n_new = 64


def step_ms(B, params, reps=5):
    """ms per decode step of B rows behind 64-id prompts: n_new - 1 graph steps per window, ended by a device synchronise; (best, median) of
    `reps` windows after a warm-up window.  params = the per-row table (vz_hip.sample_rows.RowParams per row), None = the greedy tail."""
    from vz_hip import binding as Bd
    eng = model.engine
    ids = torch.stack([synth.synth_ids(64, 32000, image_pos=-1, seed=10 + b) for b in range(B)]).cuda()
    _, last = eng.prefill(eng.embed_tokens(ids), [64] * B)
    first = Bd.argmax(last)
    out = torch.empty(B, n_new - 1, dtype=torch.int32, device="cuda:0")
    ts = []
    eng.set_sampling_rows(params)
    try:
        for _ in range(reps + 1):
            eng.decode_begin(first, [64] * B, [64] * B)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.decode_steps(n_new - 1, out=out)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / (n_new - 1) * 1e3)
    finally:
        eng.set_sampling_rows(None)
    ts = sorted(ts[1:])
    return ts[0], ts[len(ts) // 2]


if SAMPLE:
    from vz_hip.sample_rows import RowParams
    for B in ROWS:
        g = step_ms(B, None)
        sm = step_ms(B, [RowParams(True, 0.7, 50, 0.9, 1000 + r, 1) for r in range(B)])
        g2 = step_ms(B, None)
        print(f"rows {B}: greedy step {g[0]:.4f} ms (median {g[1]:.4f}; again {g2[0]:.4f} / {g2[1]:.4f}), per-row sampled step {sm[0]:.4f} ms "
              f"(median {sm[1]:.4f}): {(sm[0] / min(g[0], g2[0]) - 1) * 100:+.2f} % on the best, {B / sm[0] * 1e3:.0f} sampled tokens/s", flush=True)
    sys.exit(0)
for B in ROWS:
    ids = torch.stack([synth.synth_ids(64, 32000, image_pos=-1, seed=10 + b) for b in range(B)]).cuda()
    model.generate(input_ids=ids, do_sample=False, max_new_tokens=n_new, eos_token_id=None, pad_token_id=2)
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(3):
        tm = {}
        t0 = time.perf_counter()
        out = model.generate(input_ids=ids, do_sample=False, max_new_tokens=n_new, eos_token_id=None, pad_token_id=2, timing=tm)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        best = min(best, t1 - tm.get("t_first_token", t0))
    assert tuple(out.shape) == (B, n_new)
    print(f"{'fp8 ' if FP8 else ''}batch {B}: {B * (n_new - 1) / best:8.1f} decode tokens/s total ({(n_new - 1) / best:7.1f} per sequence), {best / (n_new - 1) * 1e3:6.3f} ms per step", flush=True)
