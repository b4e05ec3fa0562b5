#!/usr/bin/env python
"""Stage-2 LoRA finetune micro-batch at the shape of ref:script/finetune.sh: 4 samples per micro-batch, anyres grid
[[336,672],[672,336]] = 3 tiles per image, model_max_length 1024 -> 929 ids + 96 visual rows = S 1024, all 32 Zephyr layers.

    python tools/bench_stage2.py [layers] [iters]

Times forward + backward of one micro-batch (the optimiser step is timed apart: it runs once per 4 micro-batches) through
Stage2Trainer (r 128, alpha 256, dropout 0.05) and through Stage1Trainer on the same batch; prints one JSON line with ms per
micro-batch, the ratio (the LoRA share), the algorithmic TFLOP/s of the Stage-2 micro-batch and the peak device memory."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-zephyr_amd"))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from vz_hip import synth  # noqa: E402
from vz_hip import lora as L  # noqa: E402
from vz_hip.train import Stage1Trainer, Stage2Trainer  # noqa: E402
from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM  # noqa: E402

nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
layers = nums[0] if nums else 32
iters = nums[1] if len(nums) > 1 else 3
Bn, N_TILES, N_IDS, R = 4, 3, 929, 128
S = N_IDS - 1 + 32 * N_TILES

hf = VisZephyrConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=layers, num_attention_heads=32, num_key_value_heads=8,
                     vocab_size=32000, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2, bos_token_id=1)
hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
hf.mm_patch_merge_type = "flat"
model = VisZephyrForCausalLM.from_synthetic(hf, seed=0, device="cuda:0", max_batch=Bn, max_ctx=S + 8, max_tiles=N_TILES * Bn,
                                            max_text=N_IDS + 8)
ids = torch.stack([synth.synth_ids(N_IDS, 32000, image_pos=1, seed=100 + b) for b in range(Bn)])
labels = ids.clone()
labels[:, :2] = -100
labels[ids == -200] = -100
tiles = [synth.synth_tiles(N_TILES, seed=300 + b).bfloat16() for b in range(Bn)]
mask = torch.ones_like(ids)


def timed(tr):
    tr.zero_grad()
    tr.forward_backward(ids, mask, labels, tiles)          # warm-up: arena, kernels
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = tr.forward_backward(ids, mask, labels, tiles)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.optimizer_step(0.0)                                 # lr 0: the masters stay, so both trainers see the same weights
    torch.cuda.synchronize()
    return min(ts) * 1e3, (time.perf_counter() - t0) * 1e3, loss


t1 = Stage1Trainer(model)
ms1, adam1, loss1 = timed(t1)
t1.close()
del t1
torch.cuda.empty_cache()
t2 = Stage2Trainer(model, r=R, alpha=256, dropout=0.05, seed=1)
t2.init_lora(torch.Generator().manual_seed(0))
ms2, adam2, loss2 = timed(t2)
peak = torch.cuda.max_memory_allocated()
free, total = torch.cuda.mem_get_info()
a = model.arch
rows = Bn * S
per_layer_w = ((a.n_heads + 2 * a.n_kv_heads) * a.head_dim + a.hidden + 3 * a.inter) * a.hidden
lora_w = sum(R * sum(L.module_dims(a, m)) for m in L.MODULES)            # r (in + out) per module
f_clip, f_qf = 381.9e9 * Bn * N_TILES, 8 * 59.4e9 * Bn * N_TILES
f_lin = 2 * rows * (layers * per_layer_w + a.vocab * a.hidden)
f_att = Bn * layers * 4 * S * S * a.hidden / 2
f_stage1 = f_clip + 3 * f_qf + 2 * f_lin + 3.5 * f_att
f_lora = 3 * 2 * rows * layers * lora_w                                   # forward + input gradient + weight gradients
print(json.dumps({"layers": layers, "samples": Bn, "tiles_per_sample": N_TILES, "S": S, "r": R,
                  "stage1_ms_per_microbatch": round(ms1, 2), "stage2_ms_per_microbatch": round(ms2, 2), "ratio": round(ms2 / ms1, 4),
                  "stage2_adamw_ms": round(adam2, 2), "stage1_adamw_ms": round(adam1, 2),
                  "stage2_tflops": round((f_stage1 + f_lora) / (ms2 * 1e-3) / 1e12, 1), "stage1_tflops": round(f_stage1 / (ms1 * 1e-3) / 1e12, 1),
                  "lora_params": layers * lora_w, "peak_alloc_gb_torch": round(peak / 2**30, 2),
                  "device_used_gb": round((total - free) / 2**30, 2), "loss_stage1": loss1, "loss_stage2": loss2}))
t2.close()
