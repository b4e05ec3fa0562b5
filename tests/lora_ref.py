"""Torch restatement of the Stage-2 LoRA step for the tests (no GPU): the Zephyr forward of oracle/vz_oracle.py with peft's branch
y = W x + scaling * B (A dropout(x)) on its seven linears, the Stage-1 loss around it, and autograd for the gradients of the factors
and the projector.  The dropout masks are injected (vz_hip/lora.py::dropout_keep), so the restatement computes the function the
device computes for those masks.  tests/test_lora_cpu.py pins it against transformers' MistralForCausalLM with a peft-equivalent
wrapper; tests/test_lora_train_gpu.py holds the HIP step to it."""
import torch
import torch.nn.functional as F

from oracle import vz_oracle as O
from vz_hip import lora as L


def masks_for(cfg, B, S, p, seed, step=0, sample_base=0, row_stride=None, dtype=torch.float32):
    """{(layer, module): float mask [B, S, in]} of the device's dropout for a batch of B samples of S spliced rows"""
    out = {}
    row_stride = S if row_stride is None else row_stride
    for i in range(cfg.n_layers):
        for j, mod in enumerate(L.MODULES):
            fin, _ = L.module_dims(cfg, mod)
            keep = L.dropout_keep(seed, step, i * 7 + j, B * S, fin, S, sample_base, row_stride, p)
            out[(i, mod)] = torch.from_numpy(keep).to(dtype).view(B, S, fin)
    return out


def llm_forward(cfg, sd, inputs_embeds, lora, scaling, p=0.0, masks=None, attention_mask=None, position_ids=None, P=O.FP32):
    """vz_oracle.llm_forward (no cache) with the LoRA branch.  lora = {(layer, module): (A, B)}; masks as masks_for (None: p = 0).
    With P = BF16 every branch output is rounded where the HIP path stores it: drop(x) * scaling / (1 - p), u, and the sum into
    the frozen projection's (rounded) output."""
    B_, S, H = inputs_embeds.shape
    if attention_mask is None:
        attention_mask = torch.ones(B_, S, dtype=torch.bool)
    attention_mask = attention_mask.bool()
    if position_ids is None:
        position_ids = torch.arange(S).unsqueeze(0).expand(B_, S)
    cos, sin = O.rope_tables(cfg, position_ids)
    cos, sin = cos.unsqueeze(2), sin.unsqueeze(2)
    qpos, kpos = torch.arange(S).view(1, 1, S, 1), torch.arange(S).view(1, 1, 1, S)
    keep = (kpos <= qpos) & (kpos > qpos - cfg.sliding_window) & attention_mask.view(B_, 1, 1, S)
    keep = keep | ~keep.any(-1, keepdim=True)
    nh, nkv, hd = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
    fac = scaling / (1.0 - p)

    def lin(i, mod, x, w):
        A, Bm = lora[(i, mod)]
        xd = x * scaling if masks is None else x * masks[(i, mod)] * fac
        u = P.r(O._lin(P.r(xd), A, None, P))
        return P.r(P.r(O._lin(x, w, None, P)) + O._lin(u, Bm, None, P))

    x = P.r(inputs_embeds.to(torch.float32))
    for i in range(cfg.n_layers):
        p_ = f"model.layers.{i}."
        y = P.r(O.rmsnorm(x, sd[p_ + "input_layernorm.weight"], cfg.rms_eps))
        q = lin(i, "q", y, sd[p_ + "self_attn.q_proj.weight"]).view(B_, S, nh, hd)
        k = lin(i, "k", y, sd[p_ + "self_attn.k_proj.weight"]).view(B_, S, nkv, hd)
        v = lin(i, "v", y, sd[p_ + "self_attn.v_proj.weight"]).view(B_, S, nkv, hd)
        q = P.r(q * cos + O._rot_half(q) * sin)
        k = P.r(k * cos + O._rot_half(k) * sin)
        a = O._attention(q, k, v, scale=hd ** -0.5, P=P, mask=keep).reshape(B_, S, nh * hd)
        x = P.r(lin(i, "o", a, sd[p_ + "self_attn.o_proj.weight"]) + x)
        y = P.r(O.rmsnorm(x, sd[p_ + "post_attention_layernorm.weight"], cfg.rms_eps))
        g = lin(i, "gate", y, sd[p_ + "mlp.gate_proj.weight"])
        u = lin(i, "up", y, sd[p_ + "mlp.up_proj.weight"])
        a = P.r(F.silu(g) * u)
        x = P.r(lin(i, "down", a, sd[p_ + "mlp.down_proj.weight"]) + x)
    hfin = P.r(O.rmsnorm(x, sd["model.norm.weight"], cfg.rms_eps))
    return O._lin(hfin, sd["lm_head.weight"], None, P)


def stage2_grads(cfg, sd, lora, scaling, input_ids, attention_mask, labels, images, p=0.0, seed=0, step=0, P=O.FP32, feats=None):
    """(loss, {peft key / reference projector key: gradient}) of the Stage-2 loss - the Stage-1 loss (oracle/train_oracle.py)
    through the adapted Zephyr; lora = {(layer, module): (A, B)} fp32.  `feats` caches the CLIP output between calls (no_grad)."""
    train = dict(sd)
    leaves = {}
    for k in [k for k in sd if k.startswith(O.QF)]:
        leaves[k] = sd[k].detach().clone().requires_grad_(True)
        train[k] = leaves[k]
    lleaves = {}
    for (i, mod), (A, Bm) in lora.items():
        lleaves[(i, mod)] = (A.detach().clone().float().requires_grad_(True), Bm.detach().clone().float().requires_grad_(True))
    cache = {} if feats is None else feats

    def encode(imgs, text_emb):
        key = (P.bf16, P.bf16_weights)
        if key not in cache:
            with torch.no_grad():
                cache[key] = O.clip_tower(cfg, train, imgs, P)
        return O.qformer(cfg, train, cache[key], text_emb, P)

    with torch.enable_grad():
        _, pos, mask, _, emb, lab = O.prepare_inputs_labels_for_multimodal(cfg, train, input_ids, None, attention_mask, None, labels, images,
                                                                            P=P, encode_fn=encode)
        masks = None if p == 0 else masks_for(cfg, emb.shape[0], emb.shape[1], p, seed, step)
        logits = llm_forward(cfg, train, emb, lleaves, scaling, p, masks, attention_mask=mask, position_ids=pos, P=P)
        V = logits.shape[-1]
        loss = F.cross_entropy(logits[:, :-1].float().reshape(-1, V), lab[:, 1:].reshape(-1), ignore_index=O.IGNORE_INDEX)
        loss.backward()
    grads = {L.PEFT_PREFIX + k: v.grad for k, v in leaves.items()}
    for (i, mod), (A, Bm) in lleaves.items():
        grads[L.peft_key(i, mod, "A")] = A.grad
        grads[L.peft_key(i, mod, "B")] = Bm.grad
    return loss.detach(), grads
