"""numpy restatement of the four HF logits processors generate() honours (csrc/logits_proc.hip is checked against it, and it against
HF's own classes in test_logits_proc_cpu.py), in HF's order: repetition penalty, no-repeat-n-gram, min-new-tokens (prompt length to
skip = 0), suppress-tokens.  The history is the ids generated so far - the reference generates from inputs_embeds, so HF's processors
never see the prompt."""
import numpy as np


def banned_ngram_tokens(history, g):
    """ids that would complete an n-gram of size g already in `history` (hf:_calc_banned_ngram_tokens)."""
    h = [int(t) for t in history]
    n = len(h)
    if g <= 0 or n + 1 < g:
        return set()
    tail = h[n - g + 1:] if g > 1 else []
    return {h[i + g - 1] for i in range(n - g + 1) if h[i:i + g - 1] == tail}


def process(logits_fp32, history, cfg):
    """one row: fp32 logits [V], history = ids generated so far, cfg with .penalty .ngram .min_new .eos .suppress -> new fp32 logits [V].
    Ids outside [0, V) are ignored."""
    x = np.array(logits_fp32, dtype=np.float32, copy=True)
    V = x.shape[0]
    h = [int(t) for t in history]
    ok = lambda ids: sorted({int(t) for t in ids if 0 <= int(t) < V})      # noqa: E731
    if cfg.penalty != 1.0:
        idx = np.array(ok(h), dtype=np.int64)            # once per distinct token: HF gathers, then scatters
        if idx.size:
            p = np.float32(cfg.penalty)
            v = x[idx]
            with np.errstate(invalid="ignore"):
                x[idx] = np.where(v < 0, v * p, v / p).astype(np.float32)
    ninf = np.float32(-np.inf)
    for t in ok(banned_ngram_tokens(h, cfg.ngram)):
        x[t] = ninf
    if len(h) < cfg.min_new:
        for t in ok(cfg.eos):
            x[t] = ninf
    for t in ok(cfg.suppress):
        x[t] = ninf
    return x


def generate(logits_fn, cfg, max_new, eos=()):
    """greedy loop: logits_fn(ids generated so far) -> fp32 logits [V] of the next position; stops after an eos id (inclusive).
    Ties go to the smallest index."""
    out = []
    eos = set(int(t) for t in eos)
    for _ in range(max_new):
        x = np.asarray(logits_fn(list(out)), dtype=np.float32)
        if cfg is not None:
            x = process(x, out, cfg)
        tok = int(np.argmax(x))
        out.append(tok)
        if tok in eos:
            break
    return out
