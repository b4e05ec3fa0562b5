"""Per-token scores and log-probs of a generation (csrc/sampling.hip: token_scores_kernel): the host side of the step
recorder - what a generate() call asks for, the records of its chunks and rings put together as [rows, T], the positions behind a row's
eos masked, HF's `compute_transition_scores`, and the output objects.  Needs no GPU.

A record is four 32-bit words per (step, row) about the token the step's tail chose: x_tok (its logit after the processors, before
temperature), lse (log-partition of the whole row at temperature 1), lse_kept (log-partition of x / T over the sampler's kept set; a
greedy row: lse), n_kept (int32, size of that set)."""
from dataclasses import dataclass
from typing import List, Mapping, Optional, Sequence

import torch

SCORE_REC, SCORE_WARPED, SCORE_RAW = 1, 2, 4


def check_outputs(return_dict_in_generate, output_scores, output_logits, output_logprobs, num_beams: int = 1, beam_extended: bool = False) -> int:
    """the recorder flags a generate() call needs: 0 = none (every path runs as without the keywords).  As in HF, `output_scores` /
    `output_logits` / `output_logprobs` without `return_dict_in_generate` return the plain tensor, so nothing is recorded for them.
    With num_beams > 1 the keywords are refused unless the call opts in (`beam_extended=True`): then `output_scores` / `output_logits`
    give the flags of the rows the beam tail's own recorder keeps (csrc/beam.hip; no per-token records), and `output_logprobs` stays
    refused - a beam step has no single chosen row to speak of."""
    asked = [k for k, v in (("output_scores", output_scores), ("output_logits", output_logits), ("output_logprobs", output_logprobs)) if v]
    if num_beams != 1 and asked and not beam_extended:
        raise NotImplementedError(f"`{asked[0]}` with num_beams > 1 needs `beam_extended=True` (without it beam search returns `sequences`, "
                                  "`sequences_scores` and `beam_indices`)")
    if num_beams != 1 and output_logprobs:
        raise NotImplementedError("`output_logprobs` with num_beams > 1 is not built (a beam step has no single chosen row to speak of; "
                                  "`output_scores` with `compute_transition_scores(..., beam_indices)` gives the tokens' scores)")
    if not return_dict_in_generate or not asked:
        return 0
    if num_beams != 1:
        return (SCORE_WARPED if output_scores else 0) | (SCORE_RAW if output_logits else 0)
    return SCORE_REC | (SCORE_WARPED if output_scores else 0) | (SCORE_RAW if output_logits else 0)


def wants_logprobs(req: Mapping) -> bool:
    """does a `generate_stream` request ask for its tokens' log-probs (`logprobs=True`)?"""
    v = req.get("logprobs", False)
    if v is None:
        return False
    if not isinstance(v, (bool, int)) or int(v) not in (0, 1):
        raise ValueError(f"`logprobs` in a request has to be True or False, but is {v!r} (top-n alternatives are not built)")
    return bool(v)


def unpack(rec: torch.Tensor):
    """records fp32 [..., 4] -> (x_tok, lse, lse_kept fp32 [...], n_kept int32 [...])"""
    rec = rec.contiguous()
    return rec[..., 0], rec[..., 1], rec[..., 2], rec.view(torch.int32)[..., 3]


def ring_order(ring: torch.Tensor, count: int, n: int, first: Optional[int] = None) -> torch.Tensor:
    """ring [cap, ...] written at slot (step mod cap) by `count` steps so far -> the n steps from step `first` (default: the last n) in
    step order, [n, ...]"""
    cap = ring.shape[0]
    first = count - n if first is None else int(first)
    if n < 0 or first < 0 or first + n > count or first < count - cap:
        raise ValueError(f"steps [{first}, {first + n}) are not held by a ring of {cap} slots after {count} steps")
    idx = torch.tensor([(first + i) % cap for i in range(n)], dtype=torch.long, device=ring.device)
    return ring.index_select(0, idx)


def assemble(chunks: Sequence[torch.Tensor], T: Optional[int] = None) -> torch.Tensor:
    """chunks of steps [n_i, rows, ...] (unequal n_i) -> [rows, T, ...]: concatenated in step order, cut to T steps or zero-padded to them"""
    x = torch.cat([c for c in chunks if c.shape[0]], 0) if any(c.shape[0] for c in chunks) else chunks[0]
    if T is not None:
        if x.shape[0] > T:
            x = x[:T]
        elif x.shape[0] < T:
            x = torch.cat([x, x.new_zeros((T - x.shape[0],) + tuple(x.shape[1:]))], 0)
    return x.transpose(0, 1).contiguous()


def behind_eos(ids: torch.Tensor, eos) -> torch.Tensor:
    """ids [rows, T] -> bool [rows, T]: True strictly behind the row's first eos (the positions generate() shows pads in)"""
    eos = sorted(eos or [])
    if not eos:
        return torch.zeros_like(ids, dtype=torch.bool)
    hit = torch.isin(ids, torch.tensor(eos, dtype=ids.dtype, device=ids.device)).to(torch.int32)
    return (torch.cumsum(hit, dim=1) - hit) > 0


def logprobs(rec: torch.Tensor, temperature, mask: Optional[torch.Tensor] = None):
    """records [rows, T, 4], the rows' temperatures (float or [rows]; 1 for a greedy row) -> (token_logprobs = x_tok - lse,
    token_logprobs_warped = x_tok / T - lse_kept), fp32 [rows, T], 0.0 where `mask`"""
    x, lse, lse_kept, _ = unpack(rec)
    T = torch.as_tensor(temperature, dtype=torch.float32, device=rec.device).reshape(-1, 1)
    lp, lpw = x - lse, x / T - lse_kept
    if mask is not None:
        zero = torch.zeros((), dtype=torch.float32, device=rec.device)
        lp, lpw = torch.where(mask, zero, lp), torch.where(mask, zero, lpw)
    return lp, lpw


def transition_scores(sequences: torch.Tensor, scores, beam_indices=None, normalize_logits: bool = False) -> torch.Tensor:
    """HF's `GenerationMixin.compute_transition_scores` without beams (the same tensor operations in the same order, so the same fp32
    bits): the score of each generated token, [rows, len(scores)]; with `normalize_logits` the log-softmax of each step's row first."""
    if beam_indices is not None:
        raise NotImplementedError("`transition_scores` is the form without beams: with `beam_indices` use `beam_transition_scores`")
    n = len(scores)
    vocab = scores[0].shape[-1]
    beam_indices = torch.arange(scores[0].shape[0], device=sequences.device).view(-1, 1).expand(-1, n)
    s = torch.stack(tuple(scores)).reshape(n, -1).transpose(0, 1)
    if normalize_logits:
        s = s.reshape(-1, vocab, s.shape[-1])
        s = torch.nn.functional.log_softmax(s, dim=1)
        s = s.reshape(-1, s.shape[-1])
    cut = sequences.shape[-1] - n
    indices = sequences[:, cut:] + beam_indices * vocab
    return s.gather(0, indices)


def beam_transition_scores(sequences: torch.Tensor, scores, beam_indices=None, normalize_logits: bool = False, vocab_size: Optional[int] = None) -> torch.Tensor:
    """HF's `GenerationMixin.compute_transition_scores` with `beam_indices` (the same tensor operations in the same order, so the same fp32 bits): the score
    of each generated token, [rows, len(scores)]; with `normalize_logits` the log-softmax of each step's row first.  `beam_indices`
    (beam search: the flattened row of `scores[t]` that produced token t of a hypothesis, -1 behind its end): the result is cut to the
    longest hypothesis and 0 behind a hypothesis' end.  vocab_size: the model's (HF reads its config); default = the rows' width."""
    n = len(scores)
    vocab = scores[0].shape[-1] if vocab_size is None else int(vocab_size)
    if beam_indices is None:
        beam_indices = torch.arange(scores[0].shape[0]).view(-1, 1).to(sequences.device)
        beam_indices = beam_indices.expand(-1, n)
    s = torch.stack(tuple(scores)).reshape(n, -1).transpose(0, 1)
    if normalize_logits:
        s = s.reshape(-1, vocab, s.shape[-1])
        s = torch.nn.functional.log_softmax(s, dim=1)
        s = s.reshape(-1, s.shape[-1])
    mask = beam_indices < 0
    longest = (1 - mask.long()).sum(-1).max()
    beam_indices = beam_indices.clone()[:, :longest]
    mask = mask[:, :longest]
    beam_indices[mask] = 0
    cut = sequences.shape[-1] - longest
    indices = sequences[:, cut:] + beam_indices * vocab
    out = s.gather(0, indices)
    out[mask] = 0
    return out


# ---- what a generate() call collects --------------------------------------------------------------------------------------------------
class _Block:
    """the rows that decoded together: their first token's record (from the prefill logits) and the chunks of their steps"""

    def __init__(self, rows: int, temperature):
        self.rows, self.temperature = rows, temperature
        self.rec, self.warped, self.raw = [], [], []
        self.ends = None         # LongTensor [rows]: tokens a row kept when a device-side stop ended it (vz_hip.stop), else None

    def add(self, rec, warped=None, raw=None):
        """steps [n, rows, 4] (+ [n, rows, V] rows), on any device"""
        self.rec.append(rec)
        if warped is not None:
            self.warped.append(warped)
        if raw is not None:
            self.raw.append(raw)


class Sink:
    """collects the records of one generate() call, block of rows by block of rows, and puts them together"""

    def __init__(self, what: int):
        self.what = int(what)
        self.blocks: List[_Block] = []

    @property
    def warped(self) -> bool:
        return bool(self.what & SCORE_WARPED)

    @property
    def raw(self) -> bool:
        return bool(self.what & SCORE_RAW)

    def block(self, rows: int, temperature=1.0) -> _Block:
        b = _Block(rows, temperature)
        self.blocks.append(b)
        return b

    def finish(self, ids: torch.Tensor, eos) -> dict:
        """ids [rows, T] as generate() returns them -> token_logprobs / token_logprobs_warped [rows, T] (0.0 behind a row's eos and behind
        the end of a row that decoded alone and stopped early) and the tuples scores / logits of T tensors [rows, V] (None when not
        recorded; a row's entries behind its eos are what its parked row produced, behind the end of a row that decoded alone zeros)."""
        T = ids.shape[1]
        dev = ids.device
        assert sum(b.rows for b in self.blocks) == ids.shape[0]
        rec = torch.cat([assemble([c.to(dev) for c in b.rec], T) for b in self.blocks], 0)
        temps = torch.cat([torch.as_tensor(b.temperature, dtype=torch.float32).reshape(-1).expand(b.rows) for b in self.blocks]).to(dev)
        steps = torch.cat([torch.full((b.rows,), sum(c.shape[0] for c in b.rec), dtype=torch.long) for b in self.blocks]).to(dev)
        mask = behind_eos(ids, eos) | (torch.arange(T, device=dev).view(1, T) >= steps.view(-1, 1))
        if any(b.ends is not None for b in self.blocks):          # positions behind a stop string / keyword stop: as behind eos
            ends = torch.cat([torch.full((b.rows,), T, dtype=torch.long) if b.ends is None else b.ends.to(torch.long).cpu() for b in self.blocks]).to(dev)
            mask = mask | (torch.arange(T, device=dev).view(1, T) >= ends.view(-1, 1))
        lp, lpw = logprobs(rec, temps, mask)
        out = {"token_logprobs": lp, "token_logprobs_warped": lpw, "scores": None, "logits": None}
        for key, on, pick in (("scores", self.warped, lambda b: b.warped), ("logits", self.raw, lambda b: b.raw)):
            if on:
                full = torch.cat([assemble([c.to(dev) for c in pick(b)], T) for b in self.blocks], 0)      # [rows, T, V]
                out[key] = tuple(full[:, t].contiguous() for t in range(T))
        return out


def output_classes():
    """(GenerateDecoderOnlyOutput with the two log-prob fields, GenerateBeamDecoderOnlyOutput) - HF's own output objects"""
    from transformers.generation.utils import GenerateBeamDecoderOnlyOutput, GenerateDecoderOnlyOutput
    global _SCORED
    if _SCORED is None:
        @dataclass
        class GenerateScoredDecoderOnlyOutput(GenerateDecoderOnlyOutput):
            """`token_logprobs` [rows, T]: log-prob of each generated token under the model's own distribution (after the logits
            processors, temperature 1); `token_logprobs_warped` [rows, T]: under the distribution it was drawn from (temperature, top-k,
            top-p, min_p, typical_p and the epsilon / eta cutoffs applied) = compute_transition_scores(sequences, scores, normalize_logits=True).  Both 0.0 behind a row's eos."""
            token_logprobs: Optional[torch.FloatTensor] = None
            token_logprobs_warped: Optional[torch.FloatTensor] = None
        _SCORED = GenerateScoredDecoderOnlyOutput
    return _SCORED, GenerateBeamDecoderOnlyOutput


_SCORED = None
