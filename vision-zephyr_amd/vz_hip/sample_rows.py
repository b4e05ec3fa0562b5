"""Per-row sampling of a decode batch (csrc/sampling.hip: sample_rows_kernel): what a `generate_stream` request
and `generate(do_sample=True, num_return_sequences=n)` ask for, checked and turned into one table entry per decode row.  Needs no GPU."""
from dataclasses import dataclass, replace
from typing import Callable, Mapping, Optional

ROW_CAP = 64                     # rows one decode batch holds at the most
UNBUILT_REQUEST_KEYS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens", "sequence_bias", "bad_words_ids")


@dataclass(frozen=True)
class RowParams:
    """one row's entry of the per-row table; `counter` = the draw counter of the row's next token"""
    sample: bool = False
    temperature: float = 1.0
    top_k: int = 0               # 0 = no top-k filter
    top_p: float = 1.0           # 1 = no top-p filter
    seed: int = 0
    counter: int = 0
    # HF's warpers behind top-p (csrc/sampling.hip step 3b), each at its "off" value
    min_p: float = 0.0           # 0 = nothing dropped
    typical_p: float = 1.0       # >= 1 = off
    epsilon_cutoff: float = 0.0  # outside (0, 1) = off
    eta_cutoff: float = 0.0      # outside (0, 1) = off

    def at(self, counter: int) -> "RowParams":
        return replace(self, counter=int(counter))

    @property
    def warp(self):
        """(min_p, typical_p, epsilon_cutoff, eta_cutoff) with 0 for whatever is off - the kernels' column - or None when all are"""
        off = lambda v: v <= 0.0 or v >= 1.0      # noqa: E731  (HF's off values of a cutoff; a NaN is not one: the entry points refuse it)
        w = (0.0 if self.min_p <= 0.0 else self.min_p, 0.0 if self.typical_p >= 1.0 else self.typical_p,
             0.0 if off(self.epsilon_cutoff) else self.epsilon_cutoff, 0.0 if off(self.eta_cutoff) else self.eta_cutoff)
        return w if self.sample and any(w) else None


GREEDY = RowParams()


def parse_warpers(min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> dict:
    """The four warper keywords as RowParams fields, checked where HF checks them (hf:generation/logits_process.py, the constructors
    of MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper, EtaLogitsWarper - same ValueError conditions) and only when HF's
    `_get_logits_processor` would build the class: None, typical_p >= 1 and a cutoff outside (0, 1) arm nothing."""
    out = {}
    if min_p is not None:
        if not (0 <= min_p <= 1.0):
            raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {min_p}")
        out["min_p"] = float(min_p)
    if typical_p is not None and typical_p < 1.0:
        typical_p = float(typical_p)
        if not (typical_p > 0 and typical_p < 1):
            raise ValueError(f"`typical_p` has to be a float > 0 and < 1, but is {typical_p}")
        out["typical_p"] = typical_p
    if epsilon_cutoff is not None and 0.0 < epsilon_cutoff < 1.0:
        out["epsilon_cutoff"] = float(epsilon_cutoff)
    if eta_cutoff is not None and 0.0 < eta_cutoff < 1.0:
        out["eta_cutoff"] = float(eta_cutoff)
    return out


def row_params(do_sample, temperature, top_k, top_p, seed: Optional[int], gen, draw_seed: Callable[[], int], min_p=None, typical_p=None,
               epsilon_cutoff=None, eta_cutoff=None) -> RowParams:
    """`generate`'s reading of its sampling keywords: greedy unless do_sample with a temperature > 0; top_k = -1 (not named) takes the
    generation config's (`gen.top_k`), None / 0 = no filter; top_p None takes `gen.top_p`; a sampled row without a seed draws one.
    A greedy row reads neither `gen` nor a seed, and ignores the warpers as HF does (they are not even checked: HF builds none)."""
    if (not do_sample) or temperature is None or temperature <= 0:
        return GREEDY
    warp = parse_warpers(min_p, typical_p, epsilon_cutoff, eta_cutoff)
    if top_k == -1:
        top_k = gen.top_k
    top_k = int(top_k or 0)
    if top_p is None:
        top_p = gen.top_p
    top_p = float(1.0 if top_p is None else top_p)
    if top_k < 0:
        raise ValueError(f"`top_k` has to be a non-negative integer, but is {top_k}")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"`top_p` has to be a float > 0 and <= 1, but is {top_p}")
    return RowParams(True, float(temperature), top_k, top_p, int(draw_seed() if seed is None else seed), 0, **warp)


def parse_request(req: Mapping, gen, draw_seed: Callable[[], int], per_request: bool = False) -> RowParams:
    """the sampling parameters of one `generate_stream` request (keys do_sample, temperature, top_p, top_k, seed, min_p, typical_p,
    epsilon_cutoff, eta_cutoff; defaults as `generate`'s, `gen` = the model's generation config).
    Logits processors and stop sequences per request need the stream's `per_request=True` (the per-row tables of DESIGN.md section 6m;
    vz_hip.logits_proc.parse_request and vz_hip.stop.parse_row_sequences read those keys): without it a request that names one raises,
    it is never dropped."""
    for k in () if per_request else UNBUILT_REQUEST_KEYS:
        if req.get(k) is not None:
            raise NotImplementedError(f"generate_stream: `{k}` in a request is not built (logits processors run over a whole batch: generate())")
    if not per_request and req.get("stop_token_sequences") is not None:
        raise NotImplementedError("generate_stream: `stop_token_sequences` in a request needs per_request=True (without it the stop set is the call's)")
    return row_params(req.get("do_sample", False), req.get("temperature", 1.0), req.get("top_k", -1), req.get("top_p"), req.get("seed"),
                      gen, draw_seed, req.get("min_p"), req.get("typical_p"), req.get("epsilon_cutoff"), req.get("eta_cutoff"))


def row_seed(seed: int, prompt: int, n: int, j: int) -> int:
    """seed of sample j of prompt `prompt` when every prompt returns n sequences (n = 1: seed + prompt, the sequential batch's rule)"""
    return int(seed) + int(prompt) * int(n) + int(j)


def check_return_sequences(n, greedy: bool, row_capacity: int, streamer=None, stopping_criteria=None) -> int:
    """`num_return_sequences` of a generate() call without beams: the checked n.  n = 1 is every existing path, untouched."""
    if n is None:
        return 1
    if not isinstance(n, int) or isinstance(n, bool) or n < 1:
        raise ValueError(f"`num_return_sequences` has to be a strictly positive integer, but is {n}")
    if n == 1:
        return 1
    if greedy:
        raise ValueError(f"Greedy methods without beam search do not support `num_return_sequences` different than 1 (got {n}).")
    if streamer is not None or stopping_criteria is not None:
        raise NotImplementedError("a streamer or stopping_criteria with num_return_sequences > 1 is not built")
    cap = min(int(row_capacity), ROW_CAP)
    if n > cap:
        raise ValueError(f"num_return_sequences = {n} exceeds the {cap} rows that decode together (min(max_batch, {ROW_CAP})): every sample needs a KV-cache row")
    return n


def prompts_per_chunk(n: int, row_capacity: int) -> int:
    """prompts that decode together when each takes n rows: chunk * n <= min(max_batch, 64)"""
    return max(1, min(int(row_capacity), ROW_CAP) // int(n))
