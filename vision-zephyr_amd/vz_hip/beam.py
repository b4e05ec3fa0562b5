"""Beam search bookkeeping on the host (hf:generation/utils.py `_beam_search`, do_sample=False).

The device (csrc/beam.hip) chooses the running beams of every step and appends one record per prompt and step: the top K
candidates {score, token, parent beam} in order, K = max(2, 1 + n_eos) * num_beams.  HF's choice of the running beams never
depends on the finished hypotheses, so the host can keep those by REPLAYING the records afterwards, a chunk of steps at a time,
and stop at the step where HF stops (the device may have run past it; those steps are discarded).

`select_reference` restates the device selection in torch (the tests' oracle); `BeamReplay` restates
`_get_running_beams_for_next_iteration`, `_update_finished_beams`, `_check_early_stop_heuristic` and
`_beam_search_has_unfinished_sequences` for one prompt with the same fp32 tensor arithmetic.  It also keeps, per running beam and
per finished hypothesis, the chain of parent beams its tokens were chosen from - HF's `beam_indices`, here as beam numbers inside the
prompt (`best_indices`); `flat_beam_indices` turns them into HF's flattened rows `prompt * num_beams + beam`.

With logits processors (csrc/logits_proc.hip) or recorded rows the selection runs on rows that are scores already - HF's
`logits_processor(ids, log_softmax(logits))` - so `select_reference(..., on_rows=True)` adds the running scores and normalises nothing.

Ties: torch.topk leaves the order of equal values unspecified.  Here, as on the device, equal scores go to the smaller flat index
beam * V + token (candidates), and to the earlier entry (running beams, finished hypotheses: a stable sort).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch


def beam_k(num_beams: int, n_eos: int) -> int:
    """candidates kept per prompt and step (HF's `beams_to_keep`)."""
    return max(2, 1 + n_eos) * num_beams


def select_reference(logits: torch.Tensor, scores: Optional[torch.Tensor], nb_in: int, nb_out: int, eos: Sequence[int] = (),
                     on_rows: bool = False):
    """torch restatement of the device selection on fp32 logits [groups * nb_in, V] and running scores [groups * nb_in] (None = 0).
    on_rows: the rows are scores already (processed log-prob rows) and are taken as they are.
    Returns (cand_scores fp32 [groups, K], cand_tokens int64 [groups, K], cand_parents int64 [groups, K],
    next_tokens, next_scores, next_parents [groups * nb_out])."""
    rows, V = logits.shape
    groups = rows // nb_in
    lp = logits.float() if on_rows else torch.log_softmax(logits.float(), dim=-1)
    if scores is not None:
        lp = lp + scores.to(lp.device, torch.float32)[:, None]
    flat = lp.reshape(groups, nb_in * V)
    K = beam_k(nb_out, len(eos))
    vals, idx = torch.sort(flat, dim=1, descending=True, stable=True)      # equal scores: smaller flat index first
    vals, idx = vals[:, :K], idx[:, :K]
    tok, par = idx % V, idx // V
    eos_t = torch.tensor(list(eos), dtype=torch.int64, device=idx.device)
    is_eos = torch.isin(tok, eos_t) if len(eos) else torch.zeros_like(tok, dtype=torch.bool)
    nt, ns, npar = [], [], []
    for g in range(groups):
        keep = torch.nonzero(~is_eos[g]).view(-1)[:nb_out]
        nt.append(tok[g, keep]); ns.append(vals[g, keep]); npar.append(par[g, keep])
    return vals, tok, par, torch.cat(nt), torch.cat(ns), torch.cat(npar)


def decode_records(rec: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """device records int32 [..., K, 3] -> (scores fp32, tokens int64, parents int64) on the host."""
    rec = rec.cpu()
    return rec[..., 0].contiguous().view(torch.float32), rec[..., 1].long(), rec[..., 2].long()


def _stable_topk(x: torch.Tensor, k: int) -> torch.Tensor:
    return torch.sort(x, descending=True, stable=True)[1][:k]


class BeamReplay:
    """HF's beam bookkeeping for ONE prompt, fed the K sorted candidates of every step in order.

    max_length counts generated tokens (a decoder-only model generating from inputs_embeds: HF's decoder prompt length is 0)."""

    def __init__(self, num_beams: int, eos: Sequence[int], max_length: int, length_penalty: float = 1.0, early_stopping=False):
        self.nb, self.eos = int(num_beams), [int(t) for t in eos]
        self.max_length, self.length_penalty, self.early_stopping = int(max_length), float(length_penalty), early_stopping
        self.running: List[List[int]] = [[] for _ in range(self.nb)]
        self.running_scores = torch.zeros(self.nb, dtype=torch.float32)
        self.running_scores[1:] = -1e9
        self.finished: List[List[int]] = [[] for _ in range(self.nb)]
        # HF's running_beam_indices / beam_indices: the parent beam (inside the prompt) of every token of a running beam / a hypothesis,
        # as a chain (rest, parent) from the last token back, None = empty - one cell per candidate and step, unrolled by `best_indices`
        self.running_idx: list = [None] * self.nb
        self.finished_idx: list = [None] * self.nb
        self.beam_scores = torch.full((self.nb,), -1e9, dtype=torch.float32)
        self.is_sent_finished = torch.zeros(self.nb, dtype=torch.bool)
        self.heuristic_unsatisfied = True
        self.cur_len = 0
        self.done = False

    def step(self, scores: torch.Tensor, tokens: torch.Tensor, parents: torch.Tensor) -> bool:
        """one step's K candidates (sorted as the device sorts them); returns True once HF's loop would have ended."""
        assert not self.done
        nb, K = self.nb, int(scores.numel())
        scores = scores.to(torch.float32)
        toks, pars = [int(t) for t in tokens], [int(p) for p in parents]
        topk_seqs = [self.running[p] + [t] for t, p in zip(toks, pars)]
        topk_idx = [(self.running_idx[p], p) for p in pars]
        hits = torch.tensor([t in self.eos for t in toks], dtype=torch.bool)
        if self.cur_len + 1 >= self.max_length:                       # MaxLengthCriteria: every candidate stops
            hits[:] = True
        # _get_running_beams_for_next_iteration
        run_lp = scores + hits.to(torch.float32) * -1.0e9
        nxt = _stable_topk(run_lp, nb)
        self.running = [topk_seqs[i] for i in nxt.tolist()]
        self.running_idx = [topk_idx[i] for i in nxt.tolist()]
        self.running_scores = run_lp[nxt]
        # _update_finished_beams
        top_mask = torch.zeros(K, dtype=torch.bool)
        top_mask[:nb] = True
        did = hits & top_mask
        lp = scores / ((self.cur_len + 1) ** self.length_penalty)
        full = bool(self.is_sent_finished.all()) and (self.early_stopping is True)
        lp = lp + torch.tensor(float(full)) * -1.0e9
        lp = lp + torch.tensor(float(not self.heuristic_unsatisfied)) * -1.0e9
        lp = lp + (~did).to(torch.float32) * -1.0e9
        merged_scores = torch.cat([self.beam_scores, lp])
        merged_seqs = self.finished + topk_seqs
        merged_idx = self.finished_idx + topk_idx
        merged_fin = torch.cat([self.is_sent_finished, did])
        sel = _stable_topk(merged_scores, nb)
        self.finished = [merged_seqs[i] for i in sel.tolist()]
        self.finished_idx = [merged_idx[i] for i in sel.tolist()]
        self.beam_scores = merged_scores[sel]
        self.is_sent_finished = merged_fin[sel]
        self.cur_len += 1
        # _check_early_stop_heuristic
        if self.early_stopping == "never" and self.length_penalty > 0.0:
            best_len = self.max_length
        else:
            best_len = self.cur_len
        best = self.running_scores[:1] / (best_len ** self.length_penalty)
        worst = torch.where(self.is_sent_finished, torch.min(self.beam_scores), torch.tensor(-1.0e9))
        self.heuristic_unsatisfied = self.heuristic_unsatisfied and bool(torch.any(best > worst))
        # _beam_search_has_unfinished_sequences
        exists_open = not (bool(self.is_sent_finished.all()) and self.early_stopping is True)
        valid = not bool(hits.all())
        self.done = not (self.heuristic_unsatisfied and exists_open and valid)
        return self.done

    def best(self, n: int) -> List[Tuple[List[int], float]]:
        """the n best hypotheses (tokens, sequences_score), best first."""
        return [(list(self.finished[i]), float(self.beam_scores[i])) for i in range(n)]

    def best_indices(self, n: int) -> List[List[int]]:
        """the parent beam of every token of the n best hypotheses (beam numbers inside the prompt), as long as the hypothesis"""
        out = []
        for i in range(n):
            chain, cell = [], self.finished_idx[i]
            while cell is not None:
                cell, p = cell
                chain.append(p)
            out.append(chain[::-1])
        return out


def flat_beam_indices(chains: Sequence[Sequence[Sequence[int]]], num_beams: int) -> torch.Tensor:
    """HF's `beam_indices` [prompts * n, longest hypothesis] int32 from every prompt's `BeamReplay.best_indices(n)`: the flattened row
    prompt * num_beams + beam whose `scores[t]` row produced token t, -1 behind a hypothesis' end."""
    rows = [[b * num_beams + p for p in chain] for b, per in enumerate(chains) for chain in per]
    width = max((len(r) for r in rows), default=0)
    out = torch.full((len(rows), width), -1, dtype=torch.int32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.tensor(r, dtype=torch.int32)
    return out


def fill_value(pad_token_id, eos: Sequence[int]) -> int:
    """what HF's beam output holds past the end of a shorter hypothesis: `pad_token_id or eos_token_id[0]` with eos ids, else -1
    (a pad id of 0 gives way to the first eos id; HF sets pad = eos[0] when no pad id is configured)."""
    if not len(eos):
        return -1
    return int(pad_token_id) if pad_token_id else int(eos[0])
