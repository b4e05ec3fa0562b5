"""Continuing on the kept KV cache: what a cache handle remembers after a `generate()` call and how the next
call's `input_ids` - HF's contract: the whole conversation so far - are cut into the cached part and the new suffix that
`Engine.prefill_append` puts behind it.  Host only: needs no GPU to import or test."""
from dataclasses import dataclass
from typing import List, Optional, Sequence, Set

APPEND_MIN_NEW = 4      # forward(past_key_values=...): fewer new tokens than this run as decode steps, as they always did


@dataclass(frozen=True)
class Plan:
    """per cache row: the cached positions the row keeps, the rotary position of the first new token, the new ids"""
    past: List[int]
    next_pos: List[int]
    suffix: List[List[int]]
    history: Optional[List[List[int]]] = None      # every id the row has been fed once the suffix is appended: the caller's ids as given

    @property
    def new_lens(self) -> List[int]:
        return [len(s) for s in self.suffix]

    @property
    def width(self) -> int:
        return max(self.new_lens)


def masked_rows(input_ids, attention_mask=None) -> List[List[int]]:
    """the ids of each row of a [B, L] batch (nested lists or a tensor) with the masked-out (left or right pad) columns dropped"""
    rows = input_ids.tolist() if hasattr(input_ids, "tolist") else [list(r) for r in input_ids]
    if attention_mask is None:
        return [[int(t) for t in r] for r in rows]
    mask = attention_mask.tolist() if hasattr(attention_mask, "tolist") else [list(r) for r in attention_mask]
    if len(mask) != len(rows) or any(len(m) != len(r) for m, r in zip(mask, rows)):
        raise ValueError("attention_mask and input_ids differ in shape")
    return [[int(t) for t, m in zip(r, mk) if m] for r, mk in zip(rows, mask)]


def plan(rows: Sequence[Sequence[int]], lengths: Sequence[int], ids: Optional[Sequence[Sequence[int]]],
         next_pos: Optional[Sequence[int]], image_token: int) -> Plan:
    """rows: the caller's ids per cache row, pads dropped.  lengths / ids / next_pos: what the handle holds - cached positions per row,
    the ids those positions stand for (None: a handle of forward(), which never saw ids) and the next rotary position (None: the
    cached length).  With remembered ids a row must begin with them (ValueError names the first differing index) and the rest is the
    suffix; without, the handle cannot tell how many positions the caller's ids stand for (an image is one id and many positions), so
    the suffix is whatever lies behind the first `lengths[b]` ids - which the row must have (ValueError).  NotImplementedError: an
    empty suffix (nothing to compute the next token from) or an image sentinel in it (an image cannot be spliced behind a cache)."""
    if len(rows) != len(lengths):
        raise ValueError(f"past_key_values: {len(rows)} rows of input_ids for a cache of {len(lengths)} rows")
    suffix = []
    for b, row in enumerate(rows):
        row = [int(t) for t in row]
        if ids is not None:
            known = [int(t) for t in ids[b]]
            diff = next((i for i, (x, y) in enumerate(zip(row, known)) if x != y), None)
            if diff is None and len(row) < len(known):
                diff = len(row)
            if diff is not None:
                raise ValueError(f"past_key_values: row {b} of input_ids leaves the cached conversation at index {diff} "
                                 f"(the cache holds {len(known)} ids; pass the whole conversation so far)")
            new = row[len(known):]
        else:
            if len(row) < int(lengths[b]):
                raise ValueError(f"past_key_values: row {b} has {len(row)} ids, the cache of a forward() call holds {int(lengths[b])} "
                                 "positions and no ids: input_ids must be as long as the cache plus the new part")
            new = row[int(lengths[b]):]
        if not new:
            raise NotImplementedError(f"past_key_values: row {b} of input_ids adds no new id behind the cache")
        if image_token in new:
            raise NotImplementedError(f"past_key_values: row {b} has an image among its new ids; an image cannot be spliced behind a cache")
        suffix.append(new)
    past = [int(v) for v in lengths]
    return Plan(past, past if next_pos is None else [int(v) for v in next_pos], suffix, [[int(t) for t in r] for r in rows])


def emitted_counts(seqs: Sequence[Sequence[int]], eos: Set[int], fill: Optional[int] = None) -> List[int]:
    """how many ids each row of a generate() result really emitted: up to and including its first eos id; else, with `fill` (a batch
    whose rows can end on a stop condition and show the fill id behind it), without the trailing fill ids but at least one; else the
    row's width.  Counting one id too few only makes the next call compute it again."""
    out = []
    for row in seqs:
        row = [int(t) for t in row]
        n = next((i + 1 for i, t in enumerate(row) if t in eos), None)
        if n is None:
            n = len(row)
            if fill is not None:
                while n > 1 and row[n - 1] == fill:
                    n -= 1
        out.append(n)
    return out


def after_generate(prompt_ids: Sequence[Sequence[int]], prompt_positions: Sequence[int], next_pos: Sequence[int],
                   emitted: Sequence[Sequence[int]]):
    """What the cache holds after a generate() call, as HF leaves its cache: every prompt position plus every emitted token but the last
    (the last one was chosen, never fed).  prompt_ids: the ids as the caller gave them (an image is one id here and many positions
    there); prompt_positions / next_pos: cached positions and next rotary position in front of the first emitted token; emitted: the
    ids each row really emitted (`emitted_counts`).  Returns (lengths, next_pos, ids) per row."""
    fed = [max(0, len(e) - 1) for e in emitted]
    lengths = [int(p) + f for p, f in zip(prompt_positions, fed)]
    pos = [int(p) + f for p, f in zip(next_pos, fed)]
    ids = [[int(t) for t in p] + [int(t) for t in e[:f]] for p, e, f in zip(prompt_ids, emitted, fed)]
    return lengths, pos, ids
