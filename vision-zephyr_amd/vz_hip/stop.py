"""Stop strings and keyword stops of generate(), matched on the device (csrc/stop.hip: stop_match_kernel).

`parse` turns what a caller asks for - HF's `stop_strings=` / `tokenizer=` keywords, instances of HF's `StopStringCriteria` and of this
package's `KeywordsStoppingCriteria` in `stopping_criteria` - into a `Plan` the engine arms behind the step's tail
(`Engine.set_stop`), or leaves everything on the host when the device cannot take all of it.  The vocabulary preprocessing is HF's:
the plan carries the tables `StopStringCriteria.__init__` builds, verbatim."""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import torch

W = 64                       # ids the device keeps per row = the longest window (VZ_STOP_W)
ROW = 2 + W                  # ints of a row's state: n | at | ring (VZ_STOP_ROW)
MAX_STR, MAX_POS, MAX_END = 8, 16, 8
MAX_SEQ, MAX_SEQ_LEN = 16, 32
SEQ_STRIDE = 2 + MAX_SEQ_LEN
UNARMED = -2

NO_TOKENIZER = ("There are one or more stop strings, either in the arguments to `generate` or in the model's generation config, but we could "
                "not locate a tokenizer. When generating with stop strings, you must pass the model's tokenizer to the `tokenizer` argument "
                "of `generate`.")


@dataclass
class Plan:
    """what the matcher is armed with.  Stop strings: HF's tables (`emb` = embedding_vec int32 [V + 2, vec], `target` = target_lens,
    `max_pos` = max_valid_positions, `max_end` = max_valid_end_lens, `window` = maximum_token_len); `seqs`: (ids, start) pairs."""
    emb: Optional[torch.Tensor] = None
    target: Optional[torch.Tensor] = None
    n_str: int = 0
    max_pos: int = 0
    max_end: int = 0
    window: int = 0
    seqs: List[Tuple[List[int], int]] = field(default_factory=list)

    @property
    def vec(self) -> int:
        return 0 if self.emb is None else int(self.emb.shape[1])

    def seq_table(self) -> torch.Tensor:
        """int32 [n_seq, SEQ_STRIDE] = [len, start, the ids newest first] (what the kernel reads: a sequence's head is its last id)"""
        t = torch.zeros(max(1, len(self.seqs)), SEQ_STRIDE, dtype=torch.int32)
        for k, (ids, start) in enumerate(self.seqs):
            t[k, 0], t[k, 1] = len(ids), int(start)
            t[k, 2:2 + len(ids)] = torch.tensor(list(reversed(ids)), dtype=torch.int32)
        return t


def parse_row_sequences(token_sequences, n_call: int = 0) -> List[List[int]]:
    """the `stop_token_sequences` of one `generate_stream(per_request=True)` request, checked as `parse` checks the call-level ones (1..32
    ids each); with the call's own `n_call` sequences, which the matcher copies in front of every row's, they must fit MAX_SEQ:
    ValueError otherwise.  None / empty: []."""
    out = []
    for ids in token_sequences or []:
        ids = [int(t) for t in ids]
        if not 1 <= len(ids) <= MAX_SEQ_LEN:
            raise ValueError(f"a stop token sequence holds 1..{MAX_SEQ_LEN} ids, got {len(ids)}")
        out.append(ids)
    if int(n_call) + len(out) > MAX_SEQ:
        raise ValueError(f"at most {MAX_SEQ} stop token sequences for a request, the call's own included: got {n_call} + {len(out)}")
    return out


def row_seq_table(seqs: Sequence[Sequence[int]]) -> torch.Tensor:
    """a request's own sequences as the matcher's per-row table takes them (Plan.seq_table's entries, start 0)"""
    return Plan(seqs=[(list(ids), 0) for ids in seqs]).seq_table()


def _string_tables(crit) -> Optional[dict]:
    """HF's StopStringCriteria -> its tables, or None beyond the matcher's limits"""
    emb = crit.embedding_vec.detach().to("cpu", torch.int32).contiguous()
    n, mp, me, win = int(crit.num_stop_strings), int(crit.max_valid_positions), int(crit.max_valid_end_lens), int(crit.maximum_token_len)
    if not (1 <= n <= MAX_STR and 1 <= mp <= MAX_POS and 1 <= me <= MAX_END and 1 <= win <= W):
        return None
    if emb.dim() != 2 or emb.shape[1] != n * (mp + me) + 1:
        return None
    return dict(emb=emb, target=crit.target_lens.detach().to("cpu", torch.int32).contiguous(), n_str=n, max_pos=mp, max_end=me, window=win)


def _keyword_seqs(crit) -> Optional[List[Tuple[List[int], int]]]:
    out = []
    for kid in crit.keyword_ids:
        ids = [int(t) for t in torch.as_tensor(kid).reshape(-1).tolist()]
        if not 1 <= len(ids) <= MAX_SEQ_LEN:
            return None
        out.append((ids, int(crit.start_length)))
    return out


def as_list(stopping_criteria) -> list:
    if stopping_criteria is None:
        return []
    return list(stopping_criteria) if isinstance(stopping_criteria, (list, tuple)) else [stopping_criteria]


def parse(stop_strings=None, tokenizer=None, stopping_criteria=None, generation_config=None, device_stop: bool = True,
          token_sequences: Optional[Sequence[Sequence[int]]] = None):
    """-> (plan | None, host_criteria | None).  Either the device takes every stop condition of the call (plan, None) or none of them
    (None, the criteria the host calls once per token; None when nothing is asked).  The device takes `stop_strings` (a str or a list;
    default `generation_config.stop_strings`; without `tokenizer`: ValueError, as in HF), instances of HF's `StopStringCriteria` and of
    `vis_zephyr.model.mm_utils.KeywordsStoppingCriteria` (id sequences with their `start_length`) and `token_sequences` (id lists, start
    0) - one set of stop strings, within the matcher's limits (8 strings, maximum_token_len <= 64, max_valid_positions <= 16,
    max_valid_end_lens <= 8; 16 id sequences of <= 32 ids).  Any other criterion in the list (a subclass of the two classes included), a
    second set of stop strings, a limit exceeded or `device_stop=False` leaves the whole list on the host; stop strings given by keyword
    then join it as a `StopStringCriteria`, so they are never dropped.  `token_sequences` have no host form: more than 16 of them, one
    that is empty or longer than 32 ids: ValueError; in a call whose other conditions stay on the host: NotImplementedError."""
    crits = as_list(stopping_criteria)
    if stop_strings is None and generation_config is not None:
        stop_strings = getattr(generation_config, "stop_strings", None)
    if isinstance(stop_strings, str):
        stop_strings = [stop_strings]
    stop_strings = list(stop_strings) if stop_strings else None
    if stop_strings is not None and tokenizer is None:
        raise ValueError(NO_TOKENIZER)
    seqs0 = []
    for ids in token_sequences or []:
        ids = [int(t) for t in ids]
        if not 1 <= len(ids) <= MAX_SEQ_LEN:
            raise ValueError(f"a stop token sequence holds 1..{MAX_SEQ_LEN} ids, got {len(ids)}")
        seqs0.append((ids, 0))
    if len(seqs0) > MAX_SEQ:
        raise ValueError(f"at most {MAX_SEQ} stop token sequences, got {len(seqs0)}")
    if stop_strings is None and not crits and not seqs0:
        return None, None
    from transformers.generation.stopping_criteria import StopStringCriteria
    from vis_zephyr.model.mm_utils import KeywordsStoppingCriteria
    kw_crit = StopStringCriteria(tokenizer, stop_strings) if stop_strings is not None else None

    def host():
        if seqs0:                            # id lists have no host criterion to fall back to: never dropped without a word
            raise NotImplementedError("`token_sequences` together with stop conditions the device matcher cannot take (vz_hip.stop.parse)")
        every = crits + ([kw_crit] if kw_crit is not None else [])
        return None, (every or None)

    if not device_stop:
        return host()
    strings = [kw_crit] if kw_crit is not None else []
    seqs = list(seqs0)
    for c in crits:
        # the classes themselves only: a subclass may override __call__, and the device computes the base class's rule
        if type(c) is StopStringCriteria:
            strings.append(c)
        elif type(c) is KeywordsStoppingCriteria:
            s = _keyword_seqs(c)
            if s is None:
                return host()
            seqs += s
        else:
            return host()                    # a criterion the device does not know: the whole list stays on the host
    if len(strings) > 1 or len(seqs) > MAX_SEQ:
        return host()
    tabs = {}
    if strings:
        tabs = _string_tables(strings[0])
        if tabs is None:
            return host()
    if not strings and not seqs:
        return host()
    return Plan(seqs=seqs, **tabs), None

