"""Shared prompt KV for `generate(num_return_sequences=n, share_prompt_kv=True)` (csrc/attn_shared.hip): the n
sampled rows of a prompt read the prompt's K / V from the one cache row it was prefilled into, as one stacked pass per step, instead of
each streaming its own copy.  This module holds the host arithmetic - what is shared, what is refused; `Engine.set_share` arms a plan,
`decode_loop.armed(share=)` scopes it, `binding.attention_shared` is the op on its own."""
from dataclasses import dataclass
from typing import List, Sequence

from .binding import attention_shared, attention_shared_ws_floats  # noqa: F401  (the op belongs to this feature's surface)

MAX_ROWS = 64          # rows of a decode batch the engine takes
MAX_N = 64             # rows per group the kernels take


@dataclass(frozen=True)
class Plan:
    """n adjacent rows per group; shared[g] leading cache slots of group g live in cache row g * n only"""
    n: int
    shared: List[int]

    @property
    def rows(self) -> int:
        return self.n * len(self.shared)


def plan(seqlens: Sequence[int], n: int, max_new: int, max_ctx: int, window: int = 0, max_batch: int = MAX_ROWS) -> Plan:
    """The `shared` table of one decode batch: every prompt's whole prefill, `seqlens[g]` slots, is what its n rows share.
    ValueError: what no engine takes (n < 2 rows per group, an empty prompt, a prompt + max_new beyond the cache, more rows than the
    batch holds); NotImplementedError: what this route does not build (more than 64 rows per group)."""
    n, max_new, max_ctx = int(n), int(max_new), int(max_ctx)
    seqlens = [int(s) for s in seqlens]
    if n < 2:
        raise ValueError(f"share_prompt_kv: {n} row(s) per prompt share nothing (num_return_sequences >= 2 expected)")
    if n > MAX_N:
        raise NotImplementedError(f"share_prompt_kv: {n} rows per prompt, the shared-prefix attention takes 2..{MAX_N}")
    if not seqlens:
        raise ValueError("share_prompt_kv: no prompt")
    if len(seqlens) * n > min(int(max_batch), MAX_ROWS):
        raise ValueError(f"share_prompt_kv: {len(seqlens)} prompts x {n} rows exceed the {min(int(max_batch), MAX_ROWS)} rows of a decode batch")
    if max_new < 1 or int(window) < 0:
        raise ValueError(f"share_prompt_kv: max_new {max_new} >= 1 and window {window} >= 0 expected")
    for g, s in enumerate(seqlens):
        if s < 1:
            raise ValueError(f"share_prompt_kv: prompt {g} is empty")
        if s + max_new > max_ctx:
            raise ValueError(f"share_prompt_kv: prompt {g} ({s}) + max_new_tokens ({max_new}) exceeds max_ctx ({max_ctx})")
    return Plan(n, seqlens)


def check_call(num_return_sequences, num_beams, guidance: bool, past_key_values: bool, prompt_lookup, tp_size: int):
    """`generate(share_prompt_kv=True)`: what the route does not build raises NotImplementedError here, before anything runs"""
    if (num_beams or 1) != 1:
        raise NotImplementedError("share_prompt_kv with num_beams > 1 is not built (the beams' rows still take the prompt's KV by copy)")
    if guidance:
        raise NotImplementedError("share_prompt_kv with guidance_scale is not built")
    if past_key_values:
        raise NotImplementedError("share_prompt_kv with past_key_values is not built")
    if prompt_lookup:
        raise NotImplementedError("share_prompt_kv with prompt_lookup_num_tokens is not built")
    if tp_size > 1:
        raise NotImplementedError("share_prompt_kv on a tensor-parallel engine is not built")
    if (num_return_sequences or 1) == 1:
        raise NotImplementedError("share_prompt_kv with num_return_sequences == 1: one row per prompt shares nothing")
