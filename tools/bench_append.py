#!/usr/bin/env python
"""Append prefill: what putting T new tokens behind a cached context of P positions costs, on the 32-layer synthetic
Zephyr-7B, against the two things a caller could do before -

  append    one `Engine.prefill_append` of T rows behind P cached positions (what forward(past_key_values=...) and a continued generate() run)
  decode    T decode steps on the same cache (what forward(past_key_values=...) ran before; graph replays of `decode_steps`, the cheapest form)
  prefill   one `Engine.prefill` of P + T positions (what a new generate() turn costs the language model; CLIP and the Q-Former come on top)

- and, per layer, the append attention (`vz_op_attention_append`) against `vz_op_attention` with q_pos0 = P at the same shapes.  Every
figure is the median of `--reps` device-event timings after `--warmup` untimed calls; the op timings cover `--launches` back-to-back launches
each (a single launch is a few microseconds).  `--ops-only` runs the two attention ops alone: under `rocprofv3 --kernel-trace --stats`
their kernels' own durations are in the trace (attn_append_kernel + attn_append_combine against flash_attn2_kernel).
    python tools/bench_append.py [--T 4,16,64,128,256] [--P 2048] [--layers 32] [--reps 9] [--out profiles/append.json] [--ops-only]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-zephyr_amd"))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from vz_hip import binding as B  # noqa: E402
from vz_hip import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--T", default="4,16,64,128,256")
ap.add_argument("--P", type=int, default=2048)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--flash-min-t", type=int, default=-1, help="knob 36 (append_flash_min_t): rows per sample above which the append runs the flash kernel")
ap.add_argument("--ops-only", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()
TS = [int(v) for v in a.T.split(",")]
P = a.P
MAX_CTX = P + max(TS) + 64
HQ, HKV, D = 32, 8, 128
if not torch.cuda.is_available():
    raise SystemExit("bench_append: needs the GPU (no timing is taken on a CPU)")
B.load_library()
if a.flash_min_t >= 0:
    B.tune("append_flash_min_t", a.flash_min_t)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def median_ms(fn, reps=None, warmup=None):
    for _ in range(a.warmup if warmup is None else warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(timed(fn) for _ in range(a.reps if reps is None else reps))


def bench_ops():
    """per launch, microseconds: the append attention against the flash kernel with a scalar q_pos0, one layer's shapes"""
    g = torch.Generator(device="cpu").manual_seed(0)
    kc = torch.randn(1, HKV, MAX_CTX, D, generator=g).bfloat16().cuda()
    vc = torch.randn(1, HKV, MAX_CTX, D, generator=g).bfloat16().cuda()
    rows = []
    for T in TS:
        q = torch.randn(1, T, HQ, D, generator=g).bfloat16().cuda()
        past = torch.tensor([P], dtype=torch.int32, device="cuda")
        new = torch.tensor([T], dtype=torch.int32, device="cuda")
        k1 = kc[0, :, :P + T].permute(1, 0, 2).unsqueeze(0)
        v1 = vc[0, :, :P + T].permute(1, 0, 2).unsqueeze(0)
        out = torch.empty(1, T, HQ, D, dtype=torch.bfloat16, device="cuda")

        def run_new():
            for _ in range(a.launches):
                B.attention_append(q, kc, vc, past, new, D ** -0.5, P + T, window=4096, out=out)

        def run_old():
            for _ in range(a.launches):
                B.attention(q, k1, v1, D ** -0.5, True, P, 4096)

        o_new = B.attention_append(q, kc, vc, past, new, D ** -0.5, P + T, window=4096).float()
        o_old = B.attention(q, k1, v1, D ** -0.5, True, P, 4096).float()
        r = dict(kind="attention op", T=T, P=P, append_us=round(1e3 * median_ms(run_new) / a.launches, 2),
                 flash_q_pos0_us=round(1e3 * median_ms(run_old) / a.launches, 2),
                 max_abs_diff=float((o_new - o_old).abs().max()))
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def bench_engine():
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    hf = VisZephyrConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=a.layers, num_attention_heads=HQ, num_key_value_heads=HKV,
                         vocab_size=32000, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2, bos_token_id=1)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    hf.mm_hidden_size = 5120
    eng = VisZephyrForCausalLM.from_synthetic(hf, seed=0, device="cuda:0", max_batch=1, max_ctx=MAX_CTX, max_tiles=1, max_text=64).engine
    ids = synth.synth_ids(P + max(TS), 32000, image_pos=-1, seed=7).unsqueeze(0)
    emb = eng.embed_tokens(ids)
    rows = []
    for T in TS:
        eng.prefill(emb[:, :P], [P], all_logits=False, last_logits=True)
        new = emb[:, P:P + T].contiguous()
        t_app = median_ms(lambda: eng.prefill_append(0, new, [T], [P], all_logits=True, last_logits=False))
        first = torch.tensor([int(ids[0, P])], dtype=torch.int32)

        def decode():
            eng.decode_begin(first, [P], [P])
            eng.decode_steps(T)

        t_dec = median_ms(decode, reps=min(a.reps, 5), warmup=1)
        eng.check_async()
        t_full = median_ms(lambda: eng.prefill(emb[:, :P + T], [P + T], all_logits=False, last_logits=True), reps=min(a.reps, 5), warmup=1)
        r = dict(kind="engine", layers=a.layers, T=T, P=P, append_ms=round(t_app, 3), decode_steps_ms=round(t_dec, 3),
                 full_prefill_ms=round(t_full, 3), decode_over_append=round(t_dec / t_app, 2), prefill_over_append=round(t_full / t_app, 2))
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


rows = bench_ops()
if not a.ops_only:
    rows += bench_engine()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(P=P, layers=a.layers, reps=a.reps, launches=a.launches,
                       note="medians of device-event timings; op rows in microseconds per launch, engine rows in milliseconds per call", rows=rows), f, indent=1)
