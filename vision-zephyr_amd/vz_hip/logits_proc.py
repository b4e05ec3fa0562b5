"""HF's logits processors for generate(): the keywords `repetition_penalty`, `no_repeat_ngram_size`, `min_new_tokens`,
`suppress_tokens`, `sequence_bias` and `bad_words_ids` checked as HF checks them and packed for the device-side filter
(csrc/logits_proc.hip, DESIGN.md sections 6e and 6j).  Needs no GPU."""
import struct
from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple

MAX_NGRAM, MAX_SUPPRESS, MAX_EOS = 8, 16, 4
MAX_SEQ, MAX_SEQ_IDS, SEQ_STRIDE = 64, 8, 12          # the id-sequence table of sequence_bias / bad_words_ids (csrc/vz_common.h: ProcArgs)


@dataclass(frozen=True)
class ProcConfig:
    penalty: float = 1.0                   # 1 = off
    ngram: int = 0                         # 0 = off
    min_new: int = 0                       # the eos ids are -inf while fewer ids were generated; 0 = off
    eos: Tuple[int, ...] = ()              # only kept with min_new > 0
    suppress: Tuple[int, ...] = ()
    # sequence_bias / bad_words_ids: (ids, bias, bad) in the table's order - the one-id sequences, then the longer
    # ones, each group in HF's dict order (the order its biases add up in), then the bad words (bad = True: banned, the bias is not read)
    seq: Tuple[Tuple[Tuple[int, ...], float, bool], ...] = field(default=(), repr=False)

    def seq_table(self):
        """the table as the C entry points take it: SEQ_STRIDE ints per sequence = [len | bad | bias, fp32 bits | 0 | ids, 0-padded]"""
        out = []
        for ids, bias, bad in self.seq:
            bits = struct.unpack("<i", struct.pack("<f", float(bias)))[0]
            out += [len(ids), int(bad), 0 if bad else bits, 0] + list(ids) + [0] * (MAX_SEQ_IDS - len(ids))
        return out


# vz_proc_row (include/viszephyr.h): one row's record of the per-row table, 32 little-endian 32-bit words by byte offset -
#   0 repetition_penalty (fp32) | 4 no_repeat_ngram | 8 min_new_tokens | 12 n_eos | 16 eos[4] | 32 n_suppress | 36 suppress[16] |
#   100 n_seq | 104 active | 108 reserved[5]
ROW_RECORD_BYTES = 128
REQUEST_KEYS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens", "sequence_bias", "bad_words_ids")


def pack_row(cfg: Optional[ProcConfig]) -> bytes:
    """the vz_proc_row record of a config as the device table holds it (unused list slots -1); None: an inactive record, all zeros"""
    if cfg is None:
        return bytes(ROW_RECORD_BYTES)
    pad = lambda ids, n: (list(ids) + [-1] * n)[:n]      # noqa: E731  (a list beyond its slots keeps its count: the entry points refuse the record)
    rec = struct.pack("<f3i4ii16i2i5i", float(cfg.penalty), int(cfg.ngram), int(cfg.min_new), len(cfg.eos), *pad(cfg.eos, MAX_EOS),
                      len(cfg.suppress), *pad(cfg.suppress, MAX_SUPPRESS), len(cfg.seq), 1, 0, 0, 0, 0, 0)
    assert len(rec) == ROW_RECORD_BYTES
    return rec


def pack_row_seqs(cfg: Optional[ProcConfig]) -> list:
    """what a row's region of the per-row sequence table [max_batch][MAX_SEQ][SEQ_STRIDE] starts with: the config's own table"""
    return [] if cfg is None else cfg.seq_table()


def parse_request(req, eos: Optional[Sequence[int]] = None, vocab: Optional[int] = None) -> Optional[ProcConfig]:
    """the processor keys of one `generate_stream(per_request=True)` request (REQUEST_KEYS, read as `generate` reads its keywords) with the
    call's eos ids and the model's vocabulary: `parse`'s config, None for a request that names none of them"""
    return parse(req.get("repetition_penalty"), req.get("no_repeat_ngram_size"), req.get("min_new_tokens"), req.get("suppress_tokens"),
                 eos, req.get("sequence_bias"), req.get("bad_words_ids"), vocab)


def _check_sequence_bias(sequence_bias) -> dict:
    """hf:SequenceBiasLogitsProcessor._validate_arguments and _convert_list_arguments_into_dict: {tuple of ids: bias}"""
    sb = sequence_bias
    if not isinstance(sb, dict) and not isinstance(sb, list) or len(sb) == 0:
        raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sb}.")
    is_id = lambda t: isinstance(t, int) and not isinstance(t, bool) or type(t).__module__ == "numpy" and "int" in type(t).__name__      # noqa: E731
    if isinstance(sb, dict):
        if any(not isinstance(k, tuple) for k in sb):
            raise ValueError(f"`sequence_bias` has to be a dict with tuples as keys, but is {sb}.")
        if any(any((not is_id(t) or t < 0) for t in k) or len(k) == 0 for k in sb):
            raise ValueError(f"Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is {sb}.")
        if any(not isinstance(b, float) for b in sb.values()):
            raise ValueError(f"`sequence_bias` has to be a dict with floats as values, but is {sb}.")
        return {tuple(int(t) for t in k): float(b) for k, b in sb.items()}
    ok = lambda q: (isinstance(q, (list, tuple)) and len(q) == 2 and isinstance(q[0], list) and len(q[0]) > 0      # noqa: E731
                    and all(is_id(t) and t > 0 for t in q[0]) and isinstance(q[1], float))
    if any(not ok(q) for q in sb):
        raise ValueError(f"Each element in `sequence_bias` has to be a non-empty list of lists of positive integers and float, but is {sb}.")
    return {tuple(int(t) for t in q[0]): float(q[1]) for q in sb}


def _check_bad_words(bad_words_ids, eos_ids) -> list:
    """hf:NoBadWordsLogitsProcessor: the checked sequences without the one-id sequences that equal an eos id (possibly none)"""
    bw = bad_words_ids
    if not isinstance(bw, list) or len(bw) == 0:
        raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bw}.")
    if any(not isinstance(w, list) for w in bw):
        raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bw}.")
    if any(any((not isinstance(t, int) or isinstance(t, bool) or t < 0) for t in w) for w in bw):
        raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bw}.")
    if any(len(w) == 0 for w in bw):          # (HF builds the class and fails with an IndexError at its first step)
        raise ValueError(f"Each list in `bad_words_ids` has to be a non-empty list of positive integers, but is {bw}.")
    return list(dict.fromkeys(tuple(w) for w in bw if all(w != [e] for e in eos_ids)))      # (nothing left: HF's class then adds zeros)


def parse(repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None, suppress_tokens=None,
          eos: Optional[Sequence[int]] = None, sequence_bias=None, bad_words_ids=None, vocab: Optional[int] = None) -> Optional[ProcConfig]:
    """None when nothing is active, else the config.  ValueError where HF's processors raise one (vocab given: also for a biased or bad
    id >= vocab, which HF finds at its first step), NotImplementedError beyond what the kernel takes: more than MAX_SEQ sequences in
    `sequence_bias` and `bad_words_ids` together, or one of more than MAX_SEQ_IDS ids."""
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
    seq = []
    if sequence_bias is not None:
        sb = _check_sequence_bias(sequence_bias)
        seq += [(k, b, False) for k, b in sb.items() if len(k) == 1] + [(k, b, False) for k, b in sb.items() if len(k) > 1]
    if bad_words_ids is not None:
        seq += [(k, float("-inf"), True) for k in _check_bad_words(bad_words_ids, eos_ids)]
    if vocab is not None:
        beyond = [t for k, _, _ in seq for t in k if t >= vocab]
        if beyond:
            raise ValueError(f"The model vocabulary size is {vocab}, but the following tokens were being biased: {beyond}")
    if len(seq) > MAX_SEQ:
        raise NotImplementedError(f"{len(seq)} sequences in sequence_bias and bad_words_ids, more than {MAX_SEQ} are not built")
    if any(len(k) > MAX_SEQ_IDS for k, _, _ in seq):
        raise NotImplementedError(f"a sequence of more than {MAX_SEQ_IDS} ids in sequence_bias / bad_words_ids is not built")
    if penalty == 1.0 and ngram == 0 and min_new == 0 and not suppress and not seq:
        return None
    return ProcConfig(float(penalty), ngram, min_new, eos_ids if min_new > 0 else (), suppress, tuple(seq))
