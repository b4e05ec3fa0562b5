"""Prompt-lookup speculative decoding for greedy and sampled `generate` (HF: `prompt_lookup_num_tokens`, `max_matching_ngram_size`).

The device side is csrc/spec.hip: a verify step runs the last emitted token plus D guessed continuations of ONE sequence as D + 1 rows,
keeps the longest prefix of guesses that equals the argmax the model produces anyway - in a sampled call: the draw each position would
have had anyway, the counter-based sampler's token t of the sequence (csrc/sampling.hip: spec_sample_kernel) - and drafts the next
guesses from the ids already in the context - all inside the per-token graph.  This module holds the host side: the draft rule in plain Python (the reference the
device kernel is tested against), the history of a spliced multimodal prompt, the eligibility rule and the chunked loop.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

MAX_DRAFT = 7          # R = D + 1 rows stay inside the <= 8-row decode routes
NO_ID = -1             # history entry of a position that holds no text id (a visual token): never matches, ends a proposal


def lookup_draft(history: Sequence[int], k: int, max_ngram: int = 2, eos: Sequence[int] = ()) -> List[int]:
    """hf:generation/candidate_generator.py PromptLookupCandidateGenerator.get_candidates, restated: for n = min(max_ngram, len - 1)
    down to 1 take the LEFTMOST earlier occurrence of the last n ids whose continuation is non-empty, propose the up to k ids that
    follow it, crop the proposal in front of the first eos id (and in front of NO_ID); no match or an empty proposal = []."""
    h = list(history)
    L = len(h)
    for n in range(min(max_ngram, L - 1), 0, -1):
        tail = h[L - n:]
        if any(t < 0 for t in tail):
            continue
        for idx in range(0, L - n):                      # idx + n < L: something follows the window
            if h[idx:idx + n] == tail:
                out = []
                for t in h[idx + n:min(idx + n + k, L)]:
                    if t < 0 or t in eos:
                        break
                    out.append(t)
                return out
    return []


def spliced_history(input_ids: Sequence[int], tiles_per_image: Sequence[int], image_token: int, tokens_per_tile: int = 32,
                    max_len: Optional[int] = None) -> List[int]:
    """one id per position of the spliced sequence `prepare_inputs_labels_for_multimodal` builds ('flat' merge): the text id where the
    position holds a text embedding, NO_ID x (tiles x tokens_per_tile) where an image sentinel was replaced, cut at max_len as there."""
    out: List[int] = []
    img = 0
    for t in input_ids:
        t = int(t)
        if t == image_token:
            if img >= len(tiles_per_image):
                raise IndexError("more image sentinels than images")
            out.extend([NO_ID] * (int(tiles_per_image[img]) * tokens_per_tile))
            img += 1
        else:
            out.append(t)
    return out if max_len is None else out[:max_len]


def accept_count(draft: Sequence[int], chosen: Sequence[int]) -> int:
    """hf:generation/utils.py `_assisted_decoding`, n_matches: the longest prefix of `draft` that equals the ids the model chose at those
    positions (`chosen` holds one more: the id behind the last guess)."""
    a = 0
    while a < len(draft) and int(draft[a]) == int(chosen[a]):
        a += 1
    return a


def draft_slots(k, max_ngram, *, n_seq: int, greedy: bool, num_beams: int, streamer, stopping_criteria, tp_size: int, max_batch: int,
                prompt_len: int, max_new: int, max_ctx: int, n_eos: int = 0, heads_per_kv: int = 4, sampled: bool = False) -> int:
    """D, the draft slots a `generate(prompt_lookup_num_tokens=k)` call runs with, or 0 = the call takes the plain path (the kwarg is
    without effect, as before): one sequence - greedy, or sampled when the caller runs sampled verify steps (`sampled`) - no beams /
    streamer / stopping criteria / tensor parallelism, an engine with >= 2 rows, n-gram size 1..4, at most 4 eos ids and 4 query heads
    per KV head (what the device tail / the verify attention take) and prompt + max_new_tokens + D inside the cache."""
    if k is None or int(k) < 1 or n_seq != 1 or not (greedy or sampled) or num_beams != 1 or streamer is not None or stopping_criteria is not None:
        return 0
    if tp_size != 1 or not 1 <= int(max_ngram) <= 4 or n_eos > 4 or heads_per_kv != 4:
        return 0
    D = min(int(k), MAX_DRAFT, max_batch - 1)
    if D < 1 or prompt_len + max_new + D > max_ctx:
        return 0
    return D


def decode(eng, first_tok: int, next_pos: int, ctx_len: int, history: Sequence[int], D: int, max_new: int, eos: Sequence[int] = (),
           max_ngram: int = 2, sync_every: int = 16, source: int = 0, stream: Optional[Sequence[int]] = None,
           report: Optional[dict] = None, sample=None) -> List[int]:
    """The decode loop behind `generate(prompt_lookup_num_tokens=...)`: `first_tok` came from the prefill of `ctx_len` positions
    (`history`: one id each); chunks of `sync_every` verify steps, one readback per chunk.  Returns the generated ids, `first_tok`
    included, at most `max_new`, ending with the first eos id.  `report` receives {used, D, steps, drafted, accepted, tokens}.
    `sample` (a sampled vz_hip.sample_rows.RowParams: temperature, top_k, top_p, seed, warpers): `first_tok` was drawn with counter 0
    and every verify step draws its rows - row i of a step behind w generated ids at counter w + 1 + i - instead of taking their
    argmax; the report then also carries "sampled": True."""
    import torch
    out = [int(first_tok)]
    eos = set(int(t) for t in eos)
    sampled = sample is not None and bool(sample.sample)
    if report is not None:
        report.update({"used": True, "D": D, "steps": 0, "drafted": 0, "accepted": 0, "tokens": 1})
        if sampled:
            report["sampled"] = True
    if out[0] in eos or max_new <= 1:
        return out
    if len(history) != ctx_len:
        raise ValueError(f"history holds {len(history)} ids, the prompt {ctx_len} positions")
    if ctx_len + max_new + D > eng.max_ctx:
        raise ValueError(f"prompt ({ctx_len}) + max_new_tokens ({max_new}) + draft slots ({D}) exceed the engine's max_ctx ({eng.max_ctx})")
    R = D + 1
    first = torch.tensor([out[0]] + [0] * D, dtype=torch.int32)
    eng.decode_begin(first, [next_pos + i for i in range(R)], [ctx_len + i for i in range(R)])
    eng.set_spec(True, D=D, max_ngram=max_ngram, history=list(history) + [out[0]], eos=sorted(eos), budget=max_new - 1, source=source,
                 stream=stream, **({"sample": sample} if sampled else {}))
    try:
        stop = False
        while not stop and len(out) < max_new:
            n = max(1, min(int(sync_every), max_new - len(out)))       # a step emits at least one id: never more steps than ids to go
            ids = eng.decode_steps(n).tolist()
            eng.check_async()                                          # a bounded device-side wait that expired = invalid ids: fail loudly
            for t in ids:
                out.append(int(t))
                if int(t) in eos or len(out) >= max_new:
                    stop = True
                    break
            st = eng.spec_state()
            stop = stop or st["done"] or not ids
        if report is not None:
            rec = [r for r in eng.spec_state()["records"] if r[2] > 0]           # (steps behind the eos / the budget emit nothing)
            report.update({"steps": len(rec), "drafted": sum(r[0] for r in rec), "accepted": sum(r[1] for r in rec), "tokens": len(out)})
        return out
    finally:
        eng.set_spec(False)
