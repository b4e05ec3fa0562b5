"""HF's logits processors for generate(): the keywords `repetition_penalty`, `no_repeat_ngram_size`, `min_new_tokens` and
`suppress_tokens` checked as HF checks them and packed for the device-side filter (csrc/logits_proc.hip).
Needs no GPU."""
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

MAX_NGRAM, MAX_SUPPRESS, MAX_EOS = 8, 16, 4


@dataclass(frozen=True)
class ProcConfig:
    penalty: float = 1.0                   # 1 = off
    ngram: int = 0                         # 0 = off
    min_new: int = 0                       # the eos ids are -inf while fewer ids were generated; 0 = off
    eos: Tuple[int, ...] = ()              # only kept with min_new > 0
    suppress: Tuple[int, ...] = ()


def parse(repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None, suppress_tokens=None,
          eos: Optional[Sequence[int]] = None) -> Optional[ProcConfig]:
    """None when nothing is active, else the config.  ValueError where HF's processors raise one, NotImplementedError beyond
    what the kernel takes by value."""
    penalty = 1.0
    if repetition_penalty is not None:
        # hf:RepetitionPenaltyLogitsProcessor: "`penalty` has to be a strictly positive float"
        if not isinstance(repetition_penalty, float) or not repetition_penalty > 0:
            raise ValueError(f"`repetition_penalty` has to be a strictly positive float, but is {repetition_penalty}")
        penalty = repetition_penalty
    ngram = 0
    if no_repeat_ngram_size is not None:
        if not isinstance(no_repeat_ngram_size, int) or isinstance(no_repeat_ngram_size, bool) or no_repeat_ngram_size < 0:
            raise ValueError(f"`no_repeat_ngram_size` has to be a non-negative integer, but is {no_repeat_ngram_size}")
        ngram = no_repeat_ngram_size
    min_new = 0
    if min_new_tokens is not None:
        if not isinstance(min_new_tokens, int) or isinstance(min_new_tokens, bool) or min_new_tokens < 0:
            raise ValueError(f"`min_new_tokens` has to be a non-negative integer, but is {min_new_tokens}")
        min_new = min_new_tokens
    suppress = tuple(dict.fromkeys(int(t) for t in (suppress_tokens or ())))
    eos_ids = tuple(dict.fromkeys(int(t) for t in (eos or ())))
    if not eos_ids:                        # HF adds the min-new-tokens processor only when there is an eos id
        min_new = 0
    if ngram > MAX_NGRAM:
        raise NotImplementedError(f"no_repeat_ngram_size {ngram} > {MAX_NGRAM} is not built")
    if len(suppress) > MAX_SUPPRESS:
        raise NotImplementedError(f"{len(suppress)} suppress_tokens, more than {MAX_SUPPRESS} are not built")
    if min_new > 0 and len(eos_ids) > MAX_EOS:
        raise NotImplementedError(f"min_new_tokens with {len(eos_ids)} eos ids, more than {MAX_EOS} are not built")
    if penalty == 1.0 and ngram == 0 and min_new == 0 and not suppress:
        return None
    return ProcConfig(float(penalty), ngram, min_new, eos_ids if min_new > 0 else (), suppress)
