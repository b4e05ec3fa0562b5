"""Classifier-free guidance as HF defines it (hf:generation/logits_process.py UnbatchedClassifierFreeGuidanceLogitsProcessor), restated
in torch: the combine of a pair of logits rows, and the two-branch greedy loop over an HF causal LM that `generate(guidance_scale=s,
negative_prompt_ids=...)` is held to in tests/test_guidance_cpu.py.  Nothing here touches the device."""
import torch


def combine(cond, uncond, s):
    """HF's guided scores of logits rows [rows, V]: s * (lc - lu) + lu over the two log-softmax rows, in the inputs' precision"""
    lc = torch.nn.functional.log_softmax(cond, dim=-1)
    lu = torch.nn.functional.log_softmax(uncond, dim=-1)
    return s * (lc - lu) + lu


@torch.no_grad()
def pair_loop(model, s, neg_ids, neg_mask, max_new, input_ids=None, inputs_embeds=None, processors=()):
    """Greedy ids [Bsz, max_new] of the two-branch scheme: the conditional branch is the prompt (ids, or embeddings: the processors then
    see the generated ids only, as HF's do), the unconditional branch `neg_ids` (left-padded by `neg_mask`) followed by the generated
    tokens, each branch with its own cache; every step combines the two last-position rows, runs `processors` (HF LogitsProcessor
    objects, in order) on the result and feeds the argmax to both branches.  The model is called as HF's generate and HF's processor
    call it: the conditional branch with positions from its (all-ones) mask, the unconditional branch with the mask only."""
    Bsz = (input_ids if input_ids is not None else inputs_embeds).shape[0]
    seq = input_ids.clone() if input_ids is not None else torch.empty(Bsz, 0, dtype=torch.long)
    c = model(input_ids=input_ids, inputs_embeds=inputs_embeds, use_cache=True)
    u = model(neg_ids, attention_mask=neg_mask, use_cache=True)
    mask_u = neg_mask
    out = []
    for _ in range(max_new):
        scores = combine(c.logits[:, -1].float(), u.logits[:, -1].float(), s)
        for p in processors:
            scores = p(seq, scores)
        tok = scores.argmax(-1)
        out.append(tok)
        seq = torch.cat([seq, tok[:, None]], dim=1)
        if len(out) == max_new:
            break
        mask_u = torch.cat([mask_u, torch.ones_like(tok[:, None])], dim=1)
        c = model(tok[:, None], past_key_values=c.past_key_values, use_cache=True)
        u = model(tok[:, None], attention_mask=mask_u, past_key_values=u.past_key_values, use_cache=True)
    return torch.stack(out, dim=1)
