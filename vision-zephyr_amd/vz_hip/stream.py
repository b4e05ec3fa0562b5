"""The scheduler of `generate_stream` (continuous batching; DESIGN.md section 4, "SURVEY config 5 in miniature", and section 6i):
requests are admitted into free cache rows, the rows step together, and at every host sync the rows that ended are yielded and parked.
Everything here needs only the engine - whatever
object has the `vz_hip.Engine` methods the loop calls, a toy on the CPU will do - the call's parsed values and a callback that embeds one
request.  The step modes are armed through `decode_loop.arming`: the call's up front, the per-row tail and the step recorder at the
first request that needs them."""
from dataclasses import dataclass
from typing import Callable, List, Optional

import torch

from . import binding as B
from . import decode_loop as DL
from . import logits_proc as LP
from . import sample_rows as SR
from . import scores as SC
from . import stop as ST


@dataclass
class Request:
    """one request as parsed at its admission"""
    index: int
    emb: Optional[torch.Tensor]          # [1, S, H]; dropped once the prefill has read it
    S: int                               # prompt length in embeddings
    budget: int                          # new tokens at the most
    params: SR.RowParams
    wants: bool                          # logprobs=True
    proc: Optional[LP.ProcConfig]        # per_request: its own processors (None: an inactive record)
    stops: List[List[int]]               # per_request: its own stop sequences


@dataclass
class Row:
    """the occupant of a live cache row"""
    req: Request
    ids: List[int]
    lps: Optional[List[float]]           # the log-prob of every id, for a request that wants them

    def result(self):
        ids = torch.tensor(self.ids, dtype=torch.long)
        return (self.req.index, ids) if self.lps is None else (self.req.index, ids, torch.tensor(self.lps, dtype=torch.float32))


def row_end(ids, budget: int, chunk, at: int, eos):
    """A row that holds `ids` and has just stepped through `chunk`: (how many of the chunk's tokens it keeps, is it finished).  It ends,
    inclusively, at an eos id, at its budget, or at generated token `at` - the index at which the matcher saw a stop condition first hold,
    -1 for none; a row already at that token keeps nothing."""
    cut = at + 1 if at >= 0 else budget
    keep = 0
    for t in chunk:
        if len(ids) + keep >= cut:
            break
        keep += 1
        if t in eos or len(ids) + keep >= budget:
            break
    last = chunk[keep - 1] if keep else ids[-1]
    return keep, last in eos or len(ids) + keep >= min(budget, cut)


def first_tokens(logits, group):
    """one launch and one readback for an admission: argmax, or each row by its own parameters, behind each row's own processors over an
    empty history (in place): (ids, their log-probs or None when no request of the group wants them)"""
    if any(q.proc is not None for q in group):
        B.logits_process_rows(logits, [q.proc for q in group])
    params = [q.params for q in group]
    ids = B.sample_rows(logits, params) if any(p.sample for p in params) else B.argmax(logits)
    if not any(q.wants for q in group):
        return ids.tolist(), None
    x, lse, _, _ = SC.unpack(B.token_scores(logits, ids, params))
    return ids.tolist(), (x - lse).tolist()


class Stream:
    """one call's state: what it armed (`scope`), who lives in which cache row (`slots`), and the three steps of its loop"""

    def __init__(self, eng, scope, embed: Callable, gen, vocab: Optional[int], eos, max_new: int, stop=None, per_request: bool = False, rows=None,
                 admit=None, sync_every: int = 16, draw_seed=lambda: int(torch.randint(0, 2 ** 62, (1,)).item())):
        n_rows = min(eng.max_batch, 64) if rows is None else int(rows)
        if not 1 <= n_rows <= min(eng.max_batch, 64):
            raise ValueError(f"rows must be in [1, {min(eng.max_batch, 64)}]")
        spare = eng.max_batch - n_rows
        width = min(spare, 16) if admit is None else int(admit)
        if not 0 <= width <= min(spare, 16):
            raise ValueError(f"admit must be in [0, {min(spare, 16)}] (max_batch {eng.max_batch} - rows {n_rows} spare cache rows)")
        self.eng, self.scope, self.embed, self.gen, self.vocab, self.eos, self.max_new = eng, scope, embed, gen, vocab, eos, max_new
        self.per_request, self.sync_every, self.draw_seed, self.n_rows, self.width = per_request, sync_every, draw_seed, n_rows, width
        self.watched = stop is not None or per_request     # the stop matcher runs: rows are watched from their admission on
        self.n_call = len(stop.seqs) if stop is not None else 0
        self.slots: List[Optional[Row]] = [None] * n_rows
        self.exhausted = False
        eng.decode_begin(torch.zeros(n_rows, dtype=torch.int32), [0] * n_rows, [0] * n_rows)       # every row parked
        if stop is not None:
            scope.arm("set_stop", (stop,), (None,))         # no row is watched until a request lands in it (stop_rows)
        if per_request:                                     # every record inactive, every row's stop sequences the call's
            scope.arm("set_logits_proc_rows", (True,), (False,))
            scope.arm("set_stop_row_seqs", (True,), (False,))

    def parse(self, idx: int, req) -> Request:
        emb = self.embed(idx, req)
        S, budget = emb.shape[1], int(req.get("max_new_tokens", self.max_new))
        if S + budget > self.eng.max_ctx:
            raise ValueError(f"request {idx}: prompt ({S}) + max_new_tokens ({budget}) exceeds the engine's max_ctx ({self.eng.max_ctx})")
        proc, stops = (LP.parse_request(req, sorted(self.eos), self.vocab), ST.parse_row_sequences(req.get("stop_token_sequences"), self.n_call)) \
            if self.per_request else (None, [])
        return Request(idx, emb, S, budget, SR.parse_request(req, self.gen, self.draw_seed, self.per_request), SC.wants_logprobs(req), proc, stops)

    def prefill(self, group: List[Request], row: int):
        """a single request straight into its free row; a group right-padded into the spare rows behind the batch: the last-position logits"""
        if len(group) == 1:
            logits = self.eng.prefill_rows(row, group[0].emb, [group[0].S])
        else:
            pad = torch.zeros(len(group), max(q.S for q in group), group[0].emb.shape[-1], dtype=torch.bfloat16, device=group[0].emb.device)
            for j, q in enumerate(group):
                pad[j, :q.S] = q.emb[0]
            logits = self.eng.prefill_rows(self.n_rows, pad, [q.S for q in group])
        for q in group:
            q.emb = None
        return logits

    def start(self, r: int):
        """the per-row writes of an admission, in the order the engine's entry points ask for"""
        eng, row = self.eng, self.slots[r]
        eng.decode_set_row(r, row.ids[0], row.req.S, row.req.S)
        if self.per_request:                                # the row's own record (its history restarts empty) and stop sequences
            eng.decode_set_row_logits_proc(r, row.req.proc)
            eng.decode_set_row_stop_seqs(r, row.req.stops)
        if self.watched:                                    # the row starts clean and its first token goes through the matcher
            eng.stop_rows(r, torch.tensor([row.ids[0]], dtype=torch.int32))
        if self.scope.has("set_sampling_rows"):             # the row's second token is draw 1 of the request's own stream
            eng.decode_set_row_sampling(r, row.req.params.at(1))

    def admit(self, it):
        """fills the free rows from `it`, one request or (with spare rows) one group per prefill; yields what ended at its first token"""
        while not self.exhausted:
            free = [r for r, row in enumerate(self.slots) if row is None]
            if not free:
                break
            group: List[Request] = []
            while len(group) < (min(len(free), self.width) if self.width >= 2 else 1):
                try:
                    group.append(self.parse(*next(it)))
                except StopIteration:
                    self.exhausted = True
                    break
            if not group:
                break
            firsts, lp0 = first_tokens(self.prefill(group, free[0]), group)
            if not self.scope.has("set_scores") and any(q.wants for q in group):
                self.scope.arm("set_scores", (max(1, int(self.sync_every)), self.n_rows), (None,))      # records only; restarts the ring between two chunks
            if not self.scope.has("set_sampling_rows") and any(q.params.sample for q in group):
                # the table the running batch uploaded holds every row greedy: rows keep their ids when the tail changes under them
                self.scope.arm("set_sampling_rows", ([],), (None,))
            src, dst = [], []                               # a group's KV: from the spare row of its prefill to the free row it takes
            for j, q in enumerate(group):
                row = Row(q, [int(firsts[j])], [lp0[j]] if q.wants else None)
                if row.ids[0] in self.eos or q.budget <= 1:
                    yield row.result()                      # (ended at its first token: nothing to write)
                    continue
                src.append(self.n_rows + j)
                dst.append(free.pop(0))
                self.slots[dst[-1]] = row
            if len(group) > 1 and dst:
                self.eng.kv_move_rows(src, dst, [self.slots[r].req.S for r in dst])
            for r in dst:
                self.start(r)

    def step(self):
        """one chunk of the live rows: (ids [rows][n], per row the matcher's index or None, log-probs [rows][n] or None) on the host"""
        eng = self.eng
        n = min([self.sync_every] + [row.req.budget - len(row.ids) for row in self.slots if row is not None])
        chunk = eng.decode_steps(n)
        at = eng.stop_at(0, self.n_rows) if self.watched else None
        chunk = chunk.cpu()                                 # [rows, n]; the only host sync of the chunk
        eng.check_async()                                   # a bounded device-side wait that expired = invalid ids: fail loudly
        lps = None
        if self.scope.has("set_scores"):
            x, lse, _, _ = SC.unpack(eng.scores_steps(n)[0].cpu())      # [n, rows]
            lps = (x - lse).transpose(0, 1).tolist()
        return chunk.tolist(), None if at is None else at.tolist(), lps

    def harvest(self, chunk, at, lps):
        """per live row what it keeps of the chunk; a finished one is yielded and its row parked until the next request arrives"""
        for r, row in enumerate(self.slots):
            if row is None:
                continue
            keep, done = row_end(row.ids, row.req.budget, chunk[r], -1 if at is None else at[r], self.eos)
            row.ids.extend(chunk[r][:keep])
            if row.lps is not None:
                row.lps.extend(lps[r][:keep])
            if done:
                yield row.result()
                self.eng.decode_set_row(r, 0, 0, 0)
                if self.per_request:
                    self.eng.decode_set_row_logits_proc(r, None)      # a parked row costs the step one record read
                self.slots[r] = None


def run(eng, requests, embed, **call):
    """the generator behind `generate_stream`: `embed(index, request)` -> the request's embeddings [1, S, H]; `call`: `Stream`'s keywords"""
    with DL.arming(eng) as scope:
        s = Stream(eng, scope, embed, **call)
        it = iter(enumerate(requests))
        while True:
            yield from s.admit(it)
            if all(row is None for row in s.slots):
                return
            yield from s.harvest(*s.step())
