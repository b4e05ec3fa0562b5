"""Host-side pieces of the Stage-2 LoRA finetune step (importable without a GPU).

What the reference trains in Stage 2 (`ref:script/finetune.sh`; `ref:vis_zephyr/train/train.py:224-243` `find_all_linear_names` keeps
every decoder linear - `mm_projector`, `vision_tower` and `lm_head` excluded; `:933-951` peft `LoraConfig(r=128, lora_alpha=256,
lora_dropout=0.05, bias="none", task_type="CAUSAL_LM")`):

    y = W x + scaling * B (A dropout(x)),   A [r, in] (kaiming_uniform_(a=sqrt(5))), B [out, r] (zeros), scaling = alpha / r

with one nn.Dropout per adapted module.  This module holds:
  * the name maps: peft's saved keys (`base_model.model.model.layers.{i}.self_attn.q_proj.lora_A.weight`) <-> the trainer's tensor
    names (`lora.{i}.q.A`), and the module shapes;
  * `dropout_keep`, the numpy restatement of the device's dropout mask (csrc/lora.hip): Philox4x32-10 with key = seed and
    counter = (column / 4, sample * row_stride + position, layer * 7 + module, optimiser step), word column % 4, kept when the
    word >= floor(p * 2^32);
  * peft's initial values and the adapter files (`adapter_config.json`, `adapter_model.safetensors`, `non_lora_trainables.bin`)
    that `vz_hip.weights.load_lora` / `load_pretrained_model(..., model_name="...lora...")` read back.
"""
from __future__ import annotations

import json
import math
import os
from typing import Dict, Iterable, Optional, Tuple

import numpy as np
import torch

MODULES = ("q", "k", "v", "o", "gate", "up", "down")                      # the engine's order; tag = layer * 7 + index
PEFT_MODULE = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj",
               "gate": "mlp.gate_proj", "up": "mlp.up_proj", "down": "mlp.down_proj"}
TARGET_MODULES = sorted(PEFT_MODULE[m].split(".")[1] for m in MODULES)
PEFT_PREFIX = "base_model.model."
FINETUNE_LR = 2e-4          # ref:script/finetune.sh --learning_rate, no --mm_projector_lr: one AdamW group for the factors and the projector


def module_dims(cfg, mod: str) -> Tuple[int, int]:
    """(in, out) of an adapted Zephyr linear; cfg = vz_hip.synth.ArchConfig (or anything with its field names)"""
    H, A, KV, I = cfg.hidden, cfg.n_heads * cfg.head_dim, cfg.n_kv_heads * cfg.head_dim, cfg.inter
    return {"q": (H, A), "k": (H, KV), "v": (H, KV), "o": (A, H), "gate": (H, I), "up": (H, I), "down": (I, H)}[mod]


def engine_name(layer: int, mod: str, ab: str) -> str:
    return f"lora.{layer}.{mod}.{ab}"


def peft_key(layer: int, mod: str, ab: str) -> str:
    """the key peft's `save_pretrained` writes (adapter name stripped)"""
    return f"{PEFT_PREFIX}model.layers.{layer}.{PEFT_MODULE[mod]}.lora_{ab}.weight"


def reference_weight_key(layer: int, mod: str) -> str:
    """the frozen weight an adapter is merged into (`vz_hip.weights.load_lora`'s keys)"""
    return f"model.layers.{layer}.{PEFT_MODULE[mod]}.weight"


def names(n_layers: int) -> Iterable[Tuple[int, str, str]]:
    for i in range(n_layers):
        for mod in MODULES:
            for ab in ("A", "B"):
                yield i, mod, ab


def peft_to_engine(n_layers: int) -> Dict[str, str]:
    return {peft_key(i, m, ab): engine_name(i, m, ab) for i, m, ab in names(n_layers)}


def shape(cfg, name: str, r: int) -> Tuple[int, int]:
    _, _, mod, ab = name.split(".")
    fin, fout = module_dims(cfg, mod)
    return (r, fin) if ab == "A" else (fout, r)


# ---- the dropout mask (numpy restatement of csrc/lora.hip) ----
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 on broadcastable uint32 counters; returns the four output words (uint64 arrays holding uint32 values)"""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in (c0, c1, c2, c3)]
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def threshold(p: float) -> int:
    """a word below it drops the element; p travels as fp32 through the C ABI"""
    return int(math.floor(float(np.float32(p)) * 4294967296.0))


def factor(scaling: float, p: float) -> np.float32:
    """the kept elements' multiplier scaling / (1 - p), as the device computes it (fp64, rounded to fp32)"""
    return np.float32(float(np.float32(scaling)) / (1.0 - float(np.float32(p))))


def dropout_keep(seed: int, step: int, tag: int, rows: int, cols: int, S: int, sample_base: int, row_stride: int, p: float) -> np.ndarray:
    """bool [rows, cols]: which elements of the input of module `tag` (= layer * 7 + module index) survive, for the rows
    b * S + t of a micro-batch whose first sample is sample `sample_base` of the optimiser batch"""
    assert cols % 4 == 0 and row_stride >= S
    r = np.arange(rows, dtype=np.int64)
    c1 = ((sample_base + r // S) * row_stride + r % S).astype(np.uint64)
    g = np.arange(cols // 4, dtype=np.uint64)
    w = philox4x32_10(g[None, :], c1[:, None], tag, step, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    words = np.stack(w, -1).reshape(rows, cols)
    return words >= np.uint64(threshold(p))


def dropout_apply(x: torch.Tensor, keep: np.ndarray, scaling: float, p: float) -> torch.Tensor:
    """the device's output values: bf16(keep * x * scaling / (1 - p)) with one fp32 multiply (x bf16 or fp32 holding bf16 values)"""
    y = x.float() * torch.from_numpy(np.asarray(factor(scaling, p))).float()
    return torch.where(torch.from_numpy(keep), y, torch.zeros_like(y)).to(torch.bfloat16)


# ---- peft's initial values and the adapter files ----
def init_factors(cfg, r: int, generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
    """{engine name: fp32 tensor} as peft's `reset_lora_parameters(init_lora_weights=True)` draws them: A <- kaiming_uniform_(a=sqrt(5)),
    B <- 0; layers in order, q k v o gate up down within a layer"""
    out = {}
    for i, mod, ab in names(cfg.n_layers):
        t = torch.empty(shape(cfg, engine_name(i, mod, ab), r), dtype=torch.float32)
        if ab == "A":
            torch.nn.init.kaiming_uniform_(t, a=math.sqrt(5), generator=generator)
        else:
            t.zero_()
        out[engine_name(i, mod, ab)] = t
    return out


def adapter_config(r: int, alpha: float, dropout: float, base_model: Optional[str] = None) -> dict:
    return {"peft_type": "LORA", "task_type": "CAUSAL_LM", "r": int(r), "lora_alpha": alpha, "lora_dropout": float(dropout),
            "target_modules": list(TARGET_MODULES), "bias": "none", "fan_in_fan_out": False, "inference_mode": True,
            "init_lora_weights": True, "modules_to_save": None, "base_model_name_or_path": base_model}


def write_adapter(directory: str, r: int, alpha: float, dropout: float, factors: Dict[str, torch.Tensor],
                  projector: Dict[str, torch.Tensor], dtype: torch.dtype = torch.bfloat16, base_model: Optional[str] = None) -> str:
    """the reference's Stage-2 output directory (ref:vis_zephyr/train/train.py:1037-1046): `adapter_config.json` +
    `adapter_model.safetensors` (peft keys, `factors` = {peft key: tensor}) and `non_lora_trainables.bin` (the projector under
    `base_model.model.model.mm_projector.*`; `projector` keys with or without that prefix)"""
    from safetensors.torch import save_file
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "adapter_config.json"), "w") as f:
        json.dump(adapter_config(r, alpha, dropout, base_model), f, indent=2)
    save_file({k: v.detach().to("cpu", dtype).contiguous() for k, v in factors.items()}, os.path.join(directory, "adapter_model.safetensors"))
    proj = {}
    for k, v in projector.items():
        k = k if k.startswith(PEFT_PREFIX) else PEFT_PREFIX + k
        proj[k] = v.detach().to("cpu", dtype).contiguous()
    torch.save(proj, os.path.join(directory, "non_lora_trainables.bin"))
    return directory


def read_adapter(directory: str) -> Tuple[dict, Dict[str, torch.Tensor]]:
    """(adapter_config, {peft key: tensor}) of a saved adapter"""
    from .weights import _iter_file
    cfg = json.load(open(os.path.join(directory, "adapter_config.json")))
    files = [f for f in (os.path.join(directory, "adapter_model.safetensors"), os.path.join(directory, "adapter_model.bin")) if os.path.exists(f)]
    if not files:
        raise FileNotFoundError(f"no adapter_model.* in {directory}")
    return cfg, dict(_iter_file(files[0]))
