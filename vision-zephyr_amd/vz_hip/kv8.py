"""Opt-in e4m3 mirror of the KV cache for the decode attention (csrc/attn_decode_kv8.hip): beside the bf16 cache, which
prefill writes and the prefill attentions read, every cache row is kept as OCP e4m3 bytes with one fp32 power-of-two scale per (cache row,
KV head, slot), for K (after RoPE) and for V - each 128-value row quantised as `quant.quantize_rows` quantises a weight row - and the decode
step streams that copy: half the bytes per key.  This module holds the host arithmetic - the layout, what the mirror costs, what is
refused; `Engine(kv_fp8=True)` / `Engine.set_kv_fp8` switch it, `binding.attention_decode_kv8` and `binding.kv8_mirror_rows` are the ops
on their own."""
from typing import Tuple

from .binding import attention_decode_kv8, kv8_mirror_rows  # noqa: F401  (the ops belong to this feature's surface)

ROW = 128              # values per quantised row = head_dim
MAX_ROWS = 64          # rows of a decode batch the kernel takes
MAX_SPLITS = 32        # key splits per (row, KV head) the kernel's merge holds


def mirror_shape(cfg, max_batch: int, max_ctx: int, tp_size: int = 1) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """(shape of the mirror's bytes, shape of its fp32 scales): [layer][K|V][row][kv head][slot][128] and [layer][K|V][row][kv head][slot]"""
    if cfg.head_dim != ROW:
        raise ValueError(f"kv_fp8: head_dim {cfg.head_dim}, the mirror's rows are {ROW} values")
    if max_batch < 1 or max_ctx < 1 or cfg.n_kv_heads % tp_size:
        raise ValueError(f"kv_fp8: max_batch {max_batch} >= 1, max_ctx {max_ctx} >= 1 and tp_size {tp_size} dividing {cfg.n_kv_heads} KV heads expected")
    lead = (cfg.n_layers, 2, int(max_batch), cfg.n_kv_heads // tp_size, int(max_ctx))
    return lead + (ROW,), lead


def row_offset(cfg, max_batch: int, max_ctx: int, layer: int, half: int, row: int, head: int, slot: int) -> int:
    """index of the (layer, K|V, cache row, KV head, slot) row in the flat scale table; its bytes start at 128 times that - which is also
    the element offset of the same row in the bf16 cache"""
    (L, two, R, H, S, _), _ = mirror_shape(cfg, max_batch, max_ctx)
    if not (0 <= layer < L and 0 <= half < two and 0 <= row < R and 0 <= head < H and 0 <= slot < S):
        raise ValueError(f"kv_fp8: (layer {layer}, half {half}, row {row}, head {head}, slot {slot}) outside {(L, two, R, H, S)}")
    return (((layer * two + half) * R + row) * H + head) * S + slot


def mirror_bytes(cfg, max_batch: int, max_ctx: int, tp_size: int = 1) -> int:
    """device bytes the mirror takes: 1 byte per cache element + 4 bytes per 128 of them, next to the bf16 cache's 2 bytes per element
    (+50 % KV memory, + 1/64 for the scales)"""
    q, s = mirror_shape(cfg, max_batch, max_ctx, tp_size)
    rows = 1
    for d in s:
        rows *= d
    return rows * ROW + rows * 4


def cache_bytes(cfg, max_batch: int, max_ctx: int, tp_size: int = 1) -> int:
    """device bytes of the bf16 cache the mirror sits beside"""
    q, _ = mirror_shape(cfg, max_batch, max_ctx, tp_size)
    n = 2
    for d in q:
        n *= d
    return n


def check_engine(tp_size: int):
    """what no kv_fp8 engine is built for"""
    if tp_size > 1:
        raise NotImplementedError("kv_fp8 on a tensor-parallel engine is not built")


def check_call(num_beams, share_prompt_kv: bool):
    """`generate()` on a kv_fp8 model: what the route does not build raises NotImplementedError here, before anything runs.  Their
    attention reads the bf16 cache, and their KV writes would leave the mirror stale.  (prompt_lookup_num_tokens is not refused: it is
    without effect and the call takes the plain path - `lookup_effective`.)"""
    if (num_beams or 1) != 1:
        raise NotImplementedError("kv_fp8 with num_beams > 1 is not built (the beam step reorders the bf16 cache only)")
    if share_prompt_kv:
        raise NotImplementedError("kv_fp8 with share_prompt_kv is not built (the shared-prefix attention reads the bf16 cache)")


def lookup_effective(kv_fp8: bool, prompt_lookup_num_tokens):
    """prompt_lookup_num_tokens as the call runs it: the verify attention reads the bf16 cache, so on a kv_fp8 model the call is the plain one"""
    return None if kv_fp8 else prompt_lookup_num_tokens
