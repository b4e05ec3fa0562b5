"""numpy restatement of HF's SequenceBiasLogitsProcessor and NoBadWordsLogitsProcessor, put into the chain of tests/logits_proc_ref.py
at HF's positions (hf:generation/utils.py `_get_logits_processor`): sequence bias, repetition penalty, no-repeat-n-gram, bad words,
min-new-tokens, suppress-tokens.  TEST INFRASTRUCTURE ONLY.  The history is the ids generated so far.

cfg = vz_hip.logits_proc.ProcConfig: cfg.seq holds (ids, bias, bad) - the one-id bias sequences, the longer ones (each group in HF's
dict order), then the bad words."""
import numpy as np

import logits_proc_ref as LPR


def acts(ids, history):
    """HF's rule, quirk included: a one-id sequence always; a longer one when the history ends in its first len - 1 ids - and is at least
    len ids long (HF skips a sequence while len(sequence) > ids generated)"""
    L = len(ids)
    if L == 1:
        return True
    h = [int(t) for t in history]
    return len(h) >= L and h[len(h) - (L - 1):] == [int(t) for t in ids[:-1]]


def bias_row(V, history, cfg):
    """the row HF adds to the scores: zeros, + the one-id biases, + every acting longer sequence's bias on its last id, in order (fp32)"""
    b = np.zeros(V, dtype=np.float32)
    for ids, bias, bad in cfg.seq:
        if not bad and 0 <= ids[-1] < V and acts(ids, history):
            b[ids[-1]] = np.float32(b[ids[-1]] + np.float32(bias))
    return b


def process(logits_fp32, history, cfg):
    """one row through the six processors -> new fp32 logits [V].  Ids outside [0, V) are ignored."""
    x = np.array(logits_fp32, dtype=np.float32, copy=True)
    V = x.shape[0]
    if any(not bad for _, _, bad in cfg.seq):
        with np.errstate(invalid="ignore"):
            x = (x + bias_row(V, history, cfg)).astype(np.float32)
    x = LPR.process(x, history, cfg)          # penalty, n-gram ban, min-new-tokens, suppress-tokens: the last three only write -inf,
    for ids, _, bad in cfg.seq:               # so the bad words' -inf may follow them
        if bad and 0 <= ids[-1] < V and acts(ids, history):
            x[ids[-1]] = np.float32(-np.inf)
    return x


def generate(logits_fn, cfg, max_new, eos=()):
    """tests/logits_proc_ref.py's greedy loop with the six processors"""
    out = []
    eos = set(int(t) for t in eos)
    for _ in range(max_new):
        x = process(np.asarray(logits_fn(list(out)), dtype=np.float32), out, cfg)
        tok = int(np.argmax(x))
        out.append(tok)
        if tok in eos:
            break
    return out
