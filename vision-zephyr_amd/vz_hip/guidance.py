"""Classifier-free guidance in `generate()`: HF's `guidance_scale` + `negative_prompt_ids`
(hf:generation/logits_process.py UnbatchedClassifierFreeGuidanceLogitsProcessor) with the two branches as two rows of one weight sweep.
The checks of the call's keywords, the unconditional branch of a call, and the row layout of a guided chunk: G prompts of n rows each are
the conditional rows [0, G * n), their negative prompts the unconditional rows [G * n, 2 * G * n) in the same order."""
import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

ROW_CAP = 64          # rows that decode together (vz_llm_decode_begin)


@dataclass(frozen=True)
class GuidanceConfig:
    """what `Engine.set_guidance` arms: the scale, and the pairs of the next decode batch (its first `pairs` rows are the conditional ones)"""
    scale: float
    pairs: int


def parse(guidance_scale, negative_prompt_ids, negative_prompt_attention_mask, negative_images, n_prompts: int, gen_config=None,
          image_token_index: Optional[int] = None) -> Optional[Tuple[float, torch.Tensor, Optional[torch.Tensor]]]:
    """The guidance keywords of a generate() call over `n_prompts` prompts: None = off (scale None or 1: every route is what it is without
    them), else (scale, negative ids LongTensor [n_prompts, L], their attention mask or None).  The scale defaults to the generation
    config's when it has one; any other finite float is taken, scales in (0, 1) included."""
    if guidance_scale is None:
        guidance_scale = getattr(gen_config, "guidance_scale", None)
    if guidance_scale is None or guidance_scale == 1:
        return None
    scale = float(guidance_scale)
    if not math.isfinite(scale):
        raise ValueError(f"`guidance_scale` has to be a finite float, but is {guidance_scale}")
    if negative_prompt_ids is None:
        raise ValueError("`guidance_scale` needs `negative_prompt_ids`: generation starts from embeddings here, so there is no last prompt id "
                         "to fall back on for the unconditional branch (HF's own fallback is empty in that case)")
    ids = torch.as_tensor(negative_prompt_ids).to(torch.long)
    if ids.dim() != 2 or ids.shape[0] != n_prompts or ids.shape[1] < 1:
        raise ValueError(f"`negative_prompt_ids` has to be [{n_prompts}, L] (one row per prompt), but is {list(ids.shape)}")
    mask = negative_prompt_attention_mask
    if mask is not None:
        mask = torch.as_tensor(mask)
        if tuple(mask.shape) != tuple(ids.shape):
            raise ValueError(f"`negative_prompt_attention_mask` {list(mask.shape)} does not match `negative_prompt_ids` {list(ids.shape)}")
    if negative_images is None and image_token_index is not None and bool((ids == image_token_index).any()):
        raise ValueError("`negative_prompt_ids` holds image sentinels but no `negative_images` were given: the unconditional branch is text "
                         "only unless its images are named")
    return scale, ids, mask


@dataclass
class Negative:
    """the unconditional branch of a call: the scale and the negative prompts' embeddings, right-padded, one row per prompt"""
    scale: float
    embeds: torch.Tensor                       # [Bsz, L, H]
    seqlens: List[int]
    position_ids: Optional[torch.Tensor]       # [Bsz, L] or None

    def rows(self, lo: int, hi: int) -> "Negative":
        return Negative(self.scale, self.embeds[lo:hi], self.seqlens[lo:hi], None if self.position_ids is None else self.position_ids[lo:hi])

    def config(self, pairs: int) -> GuidanceConfig:
        return GuidanceConfig(self.scale, int(pairs))


def prompts_per_chunk(row_capacity: int, n: int = 1) -> int:
    """prompts that decode together under guidance when each takes n rows per branch: 2 * chunk * n <= min(max_batch, 64)"""
    cap = min(int(row_capacity), ROW_CAP)
    if cap < 2:
        raise ValueError(f"guidance needs two KV-cache rows per sequence (the prompt's and the negative prompt's): max_batch = {row_capacity}")
    if 2 * n > cap:
        raise ValueError(f"num_return_sequences = {n} with guidance exceeds the {cap} rows that decode together: every sample needs two KV-cache rows")
    return cap // (2 * int(n))


@dataclass(frozen=True)
class PairLayout:
    """A guided chunk of G prompts x n rows.  cond_first / uncond_first: the cache row each prompt / negative prompt is prefilled into;
    src / dst / lens: the cache moves that spread a prefilled row over its other n - 1 rows; next_pos / ctx_len: what `decode_begin`
    takes for all 2 * G * n rows."""
    pairs: int
    cond_first: List[int]
    uncond_first: List[int]
    src: List[int]
    dst: List[int]
    lens: List[int]
    next_pos: List[int]
    ctx_len: List[int]


def pair_layout(seqlens, neg_seqlens, position_ids=None, neg_position_ids=None, n: int = 1) -> PairLayout:
    G, R = len(seqlens), len(seqlens) * n
    assert len(neg_seqlens) == G
    first = [g * n for g in range(G)] + [R + g * n for g in range(G)]
    lens_of = [int(v) for v in seqlens] + [int(v) for v in neg_seqlens]              # by prefilled sequence: G prompts, G negative prompts
    src = [first[q] for q in range(2 * G) for _ in range(1, n)]
    dst = [first[q] + j for q in range(2 * G) for j in range(1, n)]
    ctx_len = [lens_of[r // n] for r in range(2 * R)]

    def nxt(r):
        q = r // n
        pid = position_ids if q < G else neg_position_ids
        return ctx_len[r] if pid is None else int(pid[q % G, ctx_len[r] - 1]) + 1
    return PairLayout(R, first[:G], first[G:], src, dst, [lens_of[d // n] for d in dst], [nxt(r) for r in range(2 * R)], ctx_len)
