"""What every host route of `generate()` shares: the call's defaults, the first token, the scope that arms the
engine's step filters, the chunked row loop, the fan-out of one prompt over n cache rows, and running a route in parts.  The engine is
whatever object has the `vz_hip.Engine` methods a call needs - a toy on the CPU will do."""
import time
from contextlib import contextmanager
from dataclasses import dataclass
from typing import List, Optional, Set

import torch

from . import binding as B


@dataclass(frozen=True)
class CallDefaults:
    """eos: the ids in the caller's order and as a set; pad: the caller's or the generation config's (may be None); fill: what pads a row"""
    eos_list: List[int]
    eos: Set[int]
    max_new: int
    pad: Optional[int]
    fill: int


def resolve_defaults(gen, eos_token_id=None, max_new_tokens=None, max_length=None, prompt_len: int = 0, pad_token_id=None) -> CallDefaults:
    """HF's defaults of a generate call against the generation config `gen`: eos ids from the config when not named, 20 new tokens unless
    `max_length` (which counts the prompt) says otherwise, the pad id from the config, else the smallest eos id, else 0."""
    if eos_token_id is None:
        eos_token_id = gen.eos_token_id
    eos = [] if eos_token_id is None else ([int(eos_token_id)] if isinstance(eos_token_id, int) else [int(t) for t in eos_token_id])
    if max_new_tokens is None:
        max_new_tokens = 20 if max_length is None else max(1, max_length - prompt_len)
    if pad_token_id is None:
        pad_token_id = getattr(gen, "pad_token_id", None)
    return CallDefaults(eos, set(eos), int(max_new_tokens), pad_token_id, pad_token_id if pad_token_id is not None else min(eos, default=0))


def prefill_or_append(eng, embeds, seqlens, position_ids=None, app=None):
    """The prompts into cache rows 0 .. (`Engine.prefill`) or, continuing on a kept cache (app: vz_hip.append.Plan), the new suffixes
    behind what the rows hold (`Engine.prefill_append`): (last-position logits [B, V], next_pos, ctx_len) as `begin` takes them."""
    Bsz = embeds.shape[0]
    if app is None:
        _, last = eng.prefill(embeds, seqlens, position_ids, all_logits=False, last_logits=True)
        next_pos = [int(seqlens[b]) if position_ids is None else int(position_ids[b, seqlens[b] - 1]) + 1 for b in range(Bsz)]
        return last, next_pos, list(seqlens)
    _, last = eng.prefill_append(0, embeds, seqlens, app.past, position_ids, all_logits=False, last_logits=True)
    return last, [app.next_pos[b] + int(seqlens[b]) for b in range(Bsz)], [app.past[b] + int(seqlens[b]) for b in range(Bsz)]


def first_tokens(last, params, proc=None, sink=None, timing=None, draw=None, uncond=None, history=None):
    """The first token of every row, chosen on the prefill logits `last` [prompts, V] (processed in place by `proc`, whose first step
    sees an empty history): (first - device, first - host, the sink's block of these rows or None).  uncond = (the negative prompts'
    prefill logits [prompts, V], guidance scale): `last` becomes HF's guided scores in front of `proc` (B.cfg_combine; the sink's raw
    rows stay the conditional logits).  params: one
    vz_hip.sample_rows.RowParams per row; with n times as many rows as prompts each prompt's logits row serves its n adjacent rows.
    The choice is B.argmax when no row samples, else B.sample_rows; draw = (temperature, top_k, top_p, seed[, warp]): the serial sampled
    sequence's B.sample(..., seed, 0[, warp]) instead (`params` then only describes the row to the sink).  timing: stamped once the host
    holds the tokens.  history (a call that continues on a kept cache): per row the ids fed so far - `proc` then sees them as HF's
    processors see a prompt's ids, while min_new_tokens, which counts generated ids, runs over an empty history in a pass of its own
    (it only writes -inf, so the two passes commute)."""
    keep_raw = sink is not None and sink.raw
    raw = last.clone() if keep_raw and (proc is not None or uncond is not None) else last
    if uncond is not None:
        B.cfg_combine(last, uncond[0], uncond[1])
    if proc is not None and history is None:
        B.logits_process(last, proc)
    elif proc is not None:
        import dataclasses
        seen = dataclasses.replace(proc, min_new=0, eos=())
        if seen.penalty != 1.0 or seen.ngram or seen.suppress or seen.seq:
            width = max(1, max(len(h) for h in history))
            hist = torch.zeros(len(history), width, dtype=torch.int32)
            for r, h in enumerate(history):
                hist[r, :len(h)] = torch.tensor([int(t) for t in h], dtype=torch.int32)
            B.logits_process(last, seen, hist.to(last.device), torch.tensor([len(h) for h in history], dtype=torch.int32, device=last.device))
        if proc.min_new > 0:
            B.logits_process(last, type(proc)(min_new=proc.min_new, eos=proc.eos))
    n = len(params) // last.shape[0]
    if n > 1:                                                    # a prompt's one logits row, once per sample
        last, raw = last.repeat_interleave(n, dim=0).contiguous(), raw.repeat_interleave(n, dim=0) if keep_raw else None
    if draw is not None:
        first = B.sample(last, *draw[:4], 0, *draw[4:])
    else:
        first = B.sample_rows(last, params) if any(p.sample for p in params) else B.argmax(last)
    blk = None
    if sink is not None:
        blk = sink.block(len(params), params[0].temperature)
        r = B.token_scores(last, first, params, warped=sink.warped)
        rec, w = r if sink.warped else (r, None)
        blk.add(rec.unsqueeze(0), None if w is None else w.unsqueeze(0), raw.unsqueeze(0) if keep_raw else None)
    first_cpu = first.cpu().to(torch.long)
    if timing is not None:
        timing["t_first_token"] = time.perf_counter()
    return first, first_cpu, blk


def chunk_recorder(sink, rows: int, sync_every: int, max_new: int):
    """`armed`'s `scores` for a route that reads the recorder once per chunk of its row loop; None without a sink"""
    return None if sink is None else (max(1, min(sync_every, max_new - 1)), rows, sink.warped, sink.raw)


class arming:
    """The scope every decode route arms the engine's step modes through: `arm(name, args, off)` calls `eng.name(*args)` at any time inside
    it and, once that call has returned, owes `eng.name(*off)`; on the way out, whatever happened, exactly what was armed is disarmed, last
    first.  `has(name)`: is that mode armed by now?"""

    def __init__(self, eng):
        self.eng, self.undo = eng, []

    def arm(self, name, args, off):
        getattr(self.eng, name)(*args)
        self.undo.append((name, off))

    def has(self, name) -> bool:
        return any(n == name for n, _ in self.undo)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for name, off in reversed(self.undo):
            getattr(self.eng, name)(*off)


@contextmanager
def armed(eng, proc=None, sampling=None, sampling_rows=None, ring=None, scores=None, stop=None, beam=None, beam_rows=None, guidance=None,
          history=None, share=None):
    """Arms what the call asked for in the one order the engine requires - logits processors, classifier-free guidance (`guidance`: a
    vz_hip.guidance.GuidanceConfig; `begin` then takes the first tokens of the conditional rows and the positions of all 2 * pairs rows,
    and hands each first token to both rows of its pair), the step's tail (`sampling`: the arguments
    of `set_sampling`, or `sampling_rows`: the per-row table), the host token ring, the step recorder (`scores`: the arguments of
    `set_scores`), the stop matcher, the beam tail's row recorder (`beam_rows`: the arguments of `set_beam_rows`), the beam tail (`beam`:
    the arguments of `set_beam`), the shared-prefix attention (`share`: a vz_hip.share.Plan - the batch `begin` starts is its groups x n
    rows) - all in front of the batch's `decode_begin`,
    and yields `begin(first, next_pos, ctx_len)`: `decode_begin`, then the matcher takes the rows' first tokens.  On the way out,
    whatever happened (a failed arming included), exactly what was armed is disarmed, last first.  None = not asked for: not called.
    history (a call that continues on a kept cache): per row the ids fed before the first token - the processors' histories and the stop
    matcher's rings start from them (`Engine.seed_history`)."""
    def begin(first, next_pos, ctx_len):
        eng.decode_begin(first if guidance is None else torch.cat([first, first]), next_pos, ctx_len)
        if stop is not None:
            eng.stop_rows(0, first)

    with arming(eng) as scope:
        arm = scope.arm
        if proc is not None:
            arm("set_logits_proc", (proc,), (None,))
            if history is not None:
                eng.seed_history(history, proc=True)
        if guidance is not None:
            arm("set_guidance", (guidance,), (None,))
        if sampling is not None:
            arm("set_sampling", sampling, (False,))
        if sampling_rows is not None:
            arm("set_sampling_rows", (sampling_rows,), (None,))
        if ring is not None:
            arm("set_ring", (ring,), (None,))
        if scores is not None:
            arm("set_scores", scores, (None,))
        if stop is not None:
            arm("set_stop", (stop,), (None,))
            if history is not None:
                eng.seed_history(history, stop=True)
        if beam_rows is not None:
            arm("set_beam_rows", beam_rows, (None,))
        if beam is not None:
            arm("set_beam", beam, (False,))
        if share is not None:
            arm("set_share", (share,), (None,))
        yield begin


def decode_rows(eng, first_cpu, max_new, eos, pad_token_id, sync_every, blk=None, stop: bool = False) -> torch.Tensor:
    """the steps of a batch `begin` has armed with the rows' first tokens `first_cpu` (host): [rows, <= max_new] new tokens,
    `sync_every` steps per host sync (host tensor), a row showing `pad_token_id` behind its eos, until every row is done - one row
    comes back cut at its last token.  Without eos ids, stop or blk there is nothing to look at: one chunk of max_new - 1 steps.
    blk (vz_hip.scores block; the engine's step recorder is armed for `sync_every` steps): every chunk's records are added to it.
    stop: the engine's stop matcher watches the rows (`Engine.set_stop`, `stop_rows`): the token at which a row's stop condition first
    held ends the row as an eos does - the indices ride with each chunk's ids."""
    Bsz = first_cpu.numel()
    cols = [first_cpu.view(Bsz, 1)]
    eos_t = torch.tensor(sorted(eos), dtype=torch.long)
    done = torch.isin(first_cpu, eos_t) if eos else torch.zeros(Bsz, dtype=torch.bool)
    if stop:
        done = done | (eng.stop_at(0, Bsz).cpu() == 0)
    remaining = max_new - 1
    seen = 1                                                         # generated tokens per row in front of the next chunk
    finished = bool(done.all())
    while remaining > 0 and not finished:
        n = min(sync_every, remaining) if (eos or stop or blk is not None) else remaining
        chunk = eng.decode_steps(n)
        at = eng.stop_at(0, Bsz) if stop else None
        chunk = chunk.cpu()                                          # [B, n]: the only host sync of the chunk
        eng.check_async()                                            # a bounded device-side wait that expired = invalid ids: fail loudly
        if blk is not None:
            blk.add(*eng.scores_steps(n))
        remaining -= n
        if Bsz == 1 and (eos or stop):                               # one row: a plain walk over the chunk's ids, no tensor op per chunk
            a = int(at[0]) - seen if stop else -1
            end = next((i for i, t in enumerate(chunk[0].tolist()) if t in eos or i == a), None)
            seen += n
            if end is not None:
                chunk, finished = chunk[:, :end + 1], True
        elif eos or stop:
            chunk = chunk.to(torch.long)
            hit = torch.isin(chunk, eos_t) if eos else torch.zeros_like(chunk, dtype=torch.bool)      # eos emitted at (row, step)
            if stop:                                                 # ... or the row's stop condition first held at that token
                hit = hit | (at.cpu().to(torch.long).view(Bsz, 1) == seen + torch.arange(n, dtype=torch.long).view(1, n))
            seen += n
            # a row is finished after its first eos (inclusive): later steps show the pad token
            after = (torch.cumsum(hit.to(torch.int32), dim=1) - hit.to(torch.int32)) > 0
            chunk = torch.where(done.view(Bsz, 1) | after, torch.full_like(chunk, pad_token_id), chunk)
            done_at = done.view(Bsz, 1) | (torch.cumsum(hit.to(torch.int32), dim=1) > 0)      # state after each step
            all_done = done_at.all(dim=0)
            if bool(all_done.any()):                                 # stop at the first step after which every row is done
                chunk = chunk[:, : int(torch.nonzero(all_done)[0]) + 1]
            done = done_at[:, chunk.shape[1] - 1]
            finished = bool(done.all())
        cols.append(chunk)
    out = torch.cat(cols, dim=1)                                     # (int32 chunks widen to the first tokens' int64)
    if stop and blk is not None:
        at = eng.stop_at(0, Bsz).cpu().to(torch.long)
        blk.ends = torch.where((at >= 0) & (at < out.shape[1]), at + 1, torch.full_like(at, out.shape[1]))
    return out


def fan_prefill(eng, embeds, seqlens, position_ids, n: int) -> torch.Tensor:
    """First half of giving each of G prompts n cache rows: every one of the G * n rows parked (the cache moves of `fan_spread` may
    only touch parked rows), then one prefill per prompt into its first row g * n.  Returns the prompts' last-position logits [G, V];
    the caller chooses the rows' first tokens on them before it spreads."""
    R = embeds.shape[0] * n
    eng.decode_begin(torch.zeros(R, dtype=torch.int32), [0] * R, [0] * R)
    last = []
    for g in range(embeds.shape[0]):
        Sg = int(seqlens[g])
        last.append(eng.prefill_rows(g * n, embeds[g:g + 1, :Sg], [Sg], None if position_ids is None else position_ids[g:g + 1, :Sg]))
    return torch.cat(last, 0).contiguous()


def fan_spread(eng, seqlens, position_ids, n: int):
    """Second half: each prompt's KV from its first row into its other n - 1 rows.  Returns (next_pos, ctx_len) per row for `begin`."""
    G = len(seqlens)
    src = [g * n for g in range(G) for _ in range(1, n)]
    dst = [g * n + j for g in range(G) for j in range(1, n)]
    eng.kv_move_rows(src, dst, [seqlens[d // n] for d in dst])
    ctx_len = [int(seqlens[r // n]) for r in range(G * n)]
    next_pos = list(ctx_len) if position_ids is None else [int(position_ids[r // n, ctx_len[r] - 1]) + 1 for r in range(G * n)]
    return next_pos, ctx_len


def fan_share(eng, seqlens, position_ids, n: int):
    """`fan_spread` without the copies: the prompt's KV stays in its first row alone and the rows of a prompt read it from there
    (`armed(share=)`).  Returns (next_pos, ctx_len) per row for `begin` - every row appends behind the prompt in
    its own cache row."""
    G = len(seqlens)
    ctx_len = [int(seqlens[r // n]) for r in range(G * n)]
    next_pos = list(ctx_len) if position_ids is None else [int(position_ids[r // n, ctx_len[r] - 1]) + 1 for r in range(G * n)]
    return next_pos, ctx_len


def pair_prefill(eng, embeds, seqlens, position_ids, neg, n: int = 1):
    """A guided chunk (vz_hip.guidance): the G prompts `embeds` into the conditional rows, their negative prompts
    `neg` (vz_hip.guidance.Negative of the same G prompts) into the unconditional rows behind them, each sequence prefilled once and,
    with n > 1, its KV spread over its n rows.  Returns (the prompts' last-position logits [G, V], the negative prompts' [G, V],
    next_pos, ctx_len of all 2 * G * n rows for `begin`).  The first tokens are chosen on the two logits blocks; with n > 1 the rows stay
    parked until `begin`, as in `fan_prefill`."""
    from .guidance import pair_layout
    G = embeds.shape[0]
    lay = pair_layout(seqlens, neg.seqlens, position_ids, neg.position_ids, n)
    if n == 1:
        _, last = eng.prefill(embeds, seqlens, position_ids, all_logits=False, last_logits=True)
        last_u = eng.prefill_rows(G, neg.embeds, neg.seqlens, neg.position_ids)
        return last, last_u, lay.next_pos, lay.ctx_len
    R = 2 * lay.pairs
    eng.decode_begin(torch.zeros(R, dtype=torch.int32), [0] * R, [0] * R)          # every row parked: the cache moves below touch parked rows only
    last, last_u = [], []
    for g in range(G):
        Sg, Ng = int(seqlens[g]), int(neg.seqlens[g])
        last.append(eng.prefill_rows(lay.cond_first[g], embeds[g:g + 1, :Sg], [Sg], None if position_ids is None else position_ids[g:g + 1, :Sg]))
        last_u.append(eng.prefill_rows(lay.uncond_first[g], neg.embeds[g:g + 1, :Ng], [Ng],
                                       None if neg.position_ids is None else neg.position_ids[g:g + 1, :Ng]))
    eng.kv_move_rows(lay.src, lay.dst, lay.lens)
    return torch.cat(last, 0).contiguous(), torch.cat(last_u, 0).contiguous(), lay.next_pos, lay.ctx_len


def pad_parts(parts, fill, device) -> torch.Tensor:
    """[rows_i, T_i] id tensors one under the other: LongTensor [sum rows_i, max T_i] on `device`, `fill` behind a part's width"""
    if len(parts) == 1:
        return parts[0].to(device)
    out = torch.full((sum(p.shape[0] for p in parts), max(p.shape[1] for p in parts)), fill, dtype=torch.long, device=device)
    r = 0
    for p in parts:
        out[r:r + p.shape[0], :p.shape[1]] = p
        r += p.shape[0]
    return out


def run_parts(route, n_prompts: int, cap: int, fill, device, timing=None) -> torch.Tensor:
    """`route(lo, hi, timing)` -> [rows, T] over the prompts [lo, hi), at most `cap` at a time and in order (so a sink's blocks are in
    row order), padded into one tensor.  The first part stamps `timing`; the later ones get None."""
    return pad_parts([route(lo, min(n_prompts, lo + cap), timing if lo == 0 else None) for lo in range(0, n_prompts, cap)], fill, device)
