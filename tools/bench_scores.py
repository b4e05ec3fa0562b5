#!/usr/bin/env python
"""What the step recorder costs per decode step: 32-layer synthetic Zephyr-7B, 64-id prompts, at 1 row and at 64 rows,
alternating in one process (a) the recorder off, (b) VZ_SCORE_REC, (c) VZ_SCORE_REC | VZ_SCORE_WARPED.
    python tools/bench_scores.py [layers] [rounds]
Every window is 63 graph steps (rings of 63 steps) ended by a device synchronise; per leg the best and the median of `rounds` windows,
the legs taken in turn inside every round so that drift hits them alike; the spread of (a) is the run-to-run yardstick.  On a tree
without the recorder (the parent commit) only leg (a) runs.  Under `rocprofv3 --kernel-trace --stats` the kernels of interest are
token_scores_kernel and argmax_kernel."""
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


def build(max_batch):
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    hf = VisZephyrConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=layers, num_attention_heads=32,
                         num_key_value_heads=8, vocab_size=32000, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2,
                         bos_token_id=1)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    hf.mm_hidden_size = 5120
    return VisZephyrForCausalLM.from_synthetic(hf, seed=0, device="cuda:0", max_batch=max_batch, max_ctx=512, max_tiles=1, max_text=64)


model = build(64)
eng = model.engine
HAVE = hasattr(eng, "set_scores")
LEGS = [("off", None)] + ([("rec", dict(warped=False)), ("rec+warped", dict(warped=True))] if HAVE else [])

for B in (1, 64):
    ids = torch.stack([synth.synth_ids(64, 32000, image_pos=-1, seed=10 + b) for b in range(B)]).cuda()
    _, last = eng.prefill(eng.embed_tokens(ids), [64] * B)
    first = Bd.argmax(last)
    out = torch.empty(B, n_steps, dtype=torch.int32, device="cuda:0")
    ts = {name: [] for name, _ in LEGS}
    ref = None
    for r in range(rounds + 1):          # round 0 warms every leg up (its graph capture)
        for name, kw in LEGS:
            if kw is not None:
                eng.set_scores(n_steps, B, **kw)
            try:
                eng.decode_begin(first, [64] * B, [64] * B)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.decode_steps(n_steps, out=out)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / n_steps * 1e3
            finally:
                if kw is not None:
                    eng.set_scores(None)
            ref = out.clone() if ref is None else ref
            assert torch.equal(out, ref), f"{name}: the ids moved"
            if r:
                ts[name].append(dt)
    for name, _ in LEGS:
        v = sorted(ts[name])
        print(f"rows {B:2d} {name:11s}: best {v[0]:.4f} ms/step, median {v[len(v) // 2]:.4f}, worst {v[-1]:.4f} ({B / v[0] * 1e3:8.1f} tokens/s on the best)",
              flush=True)
    if HAVE:
        a = sorted(ts["off"])
        for name in ("rec", "rec+warped"):
            v = sorted(ts[name])
            print(f"rows {B:2d} {name:11s} - off: {(v[0] - a[0]) * 1e3:+.1f} us/step on the best, {(v[len(v) // 2] - a[len(a) // 2]) * 1e3:+.1f} us on the median; "
                  f"spread of off (worst - best) {(a[-1] - a[0]) * 1e3:.1f} us", flush=True)
