"""What tests/test_beam_proc_cpu.py and tests/test_beam_proc_gpu.py share: HF's own logits-processor objects in the order of
`_get_logits_processor`, one beam step of the host restatement (processors on log-prob rows, then `select_reference` on the rows as
they are), and the count of steps at which a processor changed a top-K candidate."""
import torch

from vz_hip import beam as BM

BITERS = ("repetition_penalty", "no_repeat_ngram_size", "bad_words_ids")


def hf_chain(kw, eos, device="cpu"):
    """HF's processor objects for generate()'s keywords `kw`, in HF's order"""
    from transformers.generation import logits_process as L
    chain = L.LogitsProcessorList()
    if kw.get("sequence_bias"):
        chain.append(L.SequenceBiasLogitsProcessor(sequence_bias=kw["sequence_bias"]))
    if kw.get("repetition_penalty") is not None:
        chain.append(L.RepetitionPenaltyLogitsProcessor(penalty=kw["repetition_penalty"]))
    if kw.get("no_repeat_ngram_size"):
        chain.append(L.NoRepeatNGramLogitsProcessor(kw["no_repeat_ngram_size"]))
    if kw.get("bad_words_ids"):
        chain.append(L.NoBadWordsLogitsProcessor(kw["bad_words_ids"], torch.tensor(list(eos)) if eos else None))
    if kw.get("min_new_tokens") and eos:
        chain.append(L.MinNewTokensLengthLogitsProcessor(0, kw["min_new_tokens"], list(eos), device=device))
    if kw.get("suppress_tokens"):
        chain.append(L.SuppressTokensLogitsProcessor(list(kw["suppress_tokens"]), device=device))
    return chain


def process(chain, ids, lp):
    """HF's processors on a copy of the log-prob rows lp fp32 [n, V]; ids = the n rows' generated ids (lists of one length)"""
    t = torch.tensor(ids, dtype=torch.long, device=lp.device).view(len(ids), -1)
    return chain(t, lp.clone())


def step(kw, eos, ids, lp, scores, nb_in, nb, bites=None):
    """one prompt's beam step: (processed rows, K candidate scores, tokens, parents, next tokens, scores, parents).  bites: a dict that
    counts, per processor of BITERS in kw, the steps at which leaving it out changes a (token, parent) of the K candidates."""
    rows = process(hf_chain(kw, eos, lp.device.type), ids, lp)
    cs, ct, cp, nt, ns, npar = BM.select_reference(rows, scores, nb_in, nb, eos, on_rows=True)
    if bites is not None:
        for k in BITERS:
            if kw.get(k) is None:
                continue
            less = {a: b for a, b in kw.items() if a != k}
            _, t2, p2, *_ = BM.select_reference(process(hf_chain(less, eos, lp.device.type), ids, lp), scores, nb_in, nb, eos, on_rows=True)
            bites[k] = bites.get(k, 0) + int(t2.tolist() != ct.tolist() or p2.tolist() != cp.tolist())
    return rows, cs[0], ct[0], cp[0], nt, ns, npar
