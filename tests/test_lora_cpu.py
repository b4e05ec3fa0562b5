"""Stage-2 LoRA semantics without a GPU: the torch restatement tests/lora_ref.py (the GPU test's oracle) against transformers' own
MistralForCausalLM with its seven linears per layer wrapped in a peft-equivalent LoraLinear; the numpy dropout mask of
vz_hip/lora.py; the adapter files `Stage2Trainer.save` writes, read back by the loader's `load_lora`; peft's initial values."""
import json
import math

import numpy as np
import pytest
import torch

import lora_ref
from oracle import vz_oracle as O
from vz_hip import lora as L, synth, weights as W

R, ALPHA = 8, 16.0


class LoraLinear(torch.nn.Module):
    """peft's `Linear.forward` (lora_dropout -> lora_A -> lora_B, times scaling, added to the frozen base); `mask` replaces the
    nn.Dropout draw with an injected keep mask (scaled by 1 / (1 - p) as nn.Dropout scales)"""

    def __init__(self, base, r, alpha, p):
        super().__init__()
        self.base, self.p, self.scaling = base, p, alpha / r
        self.lora_A = torch.nn.Linear(base.in_features, r, bias=False)
        self.lora_B = torch.nn.Linear(r, base.out_features, bias=False)
        self.mask = None

    def forward(self, x):
        d = x if self.p == 0 else x * self.mask / (1 - self.p)
        return self.base(x) + self.lora_B(self.lora_A(d)) * self.scaling


def _tiny(seed=0):
    transformers = pytest.importorskip("transformers")        # only the pin against MistralForCausalLM needs it
    hcfg = transformers.MistralConfig(vocab_size=96, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                                      num_key_value_heads=2, head_dim=16, max_position_embeddings=128, sliding_window=None, rms_norm_eps=1e-5,
                                      rope_theta=10000.0)
    torch.manual_seed(seed)
    m = transformers.MistralForCausalLM(hcfg).float().eval()
    cfg = synth.ArchConfig(hidden=64, inter=128, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=16, vocab=96, sliding_window=4096)
    return m, cfg


def _wrap(m, cfg, p, g):
    mods = {}
    for i, layer in enumerate(m.model.layers):
        for mod in L.MODULES:
            parent_name, leaf = L.PEFT_MODULE[mod].split(".")
            parent = getattr(layer, parent_name)
            w = LoraLinear(getattr(parent, leaf), R, ALPHA, p)
            with torch.no_grad():
                w.lora_A.weight.copy_((torch.rand(w.lora_A.weight.shape, generator=g) * 2 - 1) * 0.3)
                w.lora_B.weight.copy_((torch.rand(w.lora_B.weight.shape, generator=g) * 2 - 1) * 0.3)
            setattr(parent, leaf, w)
            mods[(i, mod)] = w
    for prm in m.parameters():
        prm.requires_grad_(False)
    for w in mods.values():
        w.lora_A.weight.requires_grad_(True)
        w.lora_B.weight.requires_grad_(True)
    return mods


@pytest.mark.parametrize("p", [0.0, 0.05])
def test_restatement_matches_transformers_with_peft_wrapper(p):
    m, cfg = _tiny()
    g = torch.Generator().manual_seed(1)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}      # frozen weights before wrapping: reference keys
    mods = _wrap(m, cfg, p, g)
    Bsz, S, seed = 2, 24, 77
    emb = torch.randn(Bsz, S, cfg.hidden, generator=g)
    labels = torch.randint(0, cfg.vocab, (Bsz, S), generator=g)
    labels[1, 17:] = -100
    masks = None if p == 0 else lora_ref.masks_for(cfg, Bsz, S, p, seed)
    if masks is not None:
        for key, w in mods.items():
            w.mask = masks[key]
            assert 0.9 < float(masks[key].mean()) < 1.0
    out = m(inputs_embeds=emb, labels=labels)
    out.loss.backward()
    lora = {k: (w.lora_A.weight.detach().clone().requires_grad_(True), w.lora_B.weight.detach().clone().requires_grad_(True)) for k, w in mods.items()}
    with torch.enable_grad():
        logits = lora_ref.llm_forward(cfg, sd, emb, lora, ALPHA / R, p, masks)
        loss = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, cfg.vocab), labels[:, 1:].reshape(-1), ignore_index=-100)
        loss.backward()
    assert abs(float(loss.detach()) - float(out.loss.detach())) <= 1e-5 * float(out.loss.detach())
    for key, w in mods.items():
        for got, want in ((lora[key][0].grad, w.lora_A.weight.grad), (lora[key][1].grad, w.lora_B.weight.grad)):
            assert float((got - want).norm() / want.norm()) <= 1e-4, key
    if p == 0:
        # the same gradients through merged weights W + s B A, with A and B as leaves
        leaves = {k: (a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)) for k, (a, b) in lora.items()}
        merged = dict(sd)
        for (i, mod), (a, b) in leaves.items():
            key = L.reference_weight_key(i, mod)
            merged[key] = sd[key] + (ALPHA / R) * b @ a
        with torch.enable_grad():
            lg, _ = O.llm_forward(cfg, merged, emb)
            l2 = torch.nn.functional.cross_entropy(lg[:, :-1].reshape(-1, cfg.vocab), labels[:, 1:].reshape(-1), ignore_index=-100)
            l2.backward()
        assert abs(float(l2.detach()) - float(loss.detach())) <= 1e-5 * float(loss.detach())
        for key in leaves:
            for got, want in ((leaves[key][0].grad, lora[key][0].grad), (leaves[key][1].grad, lora[key][1].grad)):
                assert float((got - want).norm() / want.norm()) <= 1e-4, key


def test_dropout_mask_rate_and_independence():
    p, rows, cols, S = 0.05, 64, 1024, 32
    n = rows * cols
    keeps = {}
    for tag, step, base in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 2), (223, 7, 5)):
        k = L.dropout_keep(0xABCDEF0123, step, tag, rows, cols, S, base, 40, p)
        rate = 1 - k.mean()
        assert abs(rate - p) <= 5 * math.sqrt(p * (1 - p) / n), (tag, step, base, rate)
        keeps[(tag, step, base)] = k
    ref = keeps[(0, 0, 0)]
    for key, k in keeps.items():
        if key == (0, 0, 0):
            continue
        both = (~ref & ~k).mean()                       # P[both dropped] = p^2 for independent masks
        assert abs(both - p * p) <= 5 * math.sqrt(p * p * (1 - p * p) / n), (key, both)
    # the counter is (sample within the optimiser batch, position): micro-batch 2 of size 1 sees rows 32..63 of the whole batch
    whole = L.dropout_keep(9, 3, 4, 2 * S, 64, S, 0, 40, p)
    part = L.dropout_keep(9, 3, 4, S, 64, S, 1, 40, p)
    assert np.array_equal(whole[S:], part)
    assert L.dropout_keep(9, 3, 4, S, 64, S, 0, 40, 0.0).all()
    # one Philox stream with the sampling tail: word 0 is oracle/sampling_oracle.py's
    from oracle import sampling_oracle as SO
    c0 = np.arange(50, dtype=np.uint64)
    assert np.array_equal(np.asarray(L.philox4x32_10(c0, 3, 5, 0x565A, 11, 12)[0]), np.asarray(SO.philox_word0(c0, 3, 5, 0x565A, 11, 12)))


def test_philox_known_answer():
    """Random123's published known-answer vectors for philox4x32-10"""
    got = L.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(np.asarray(w)) for w in got] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    got = L.philox4x32_10(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(np.asarray(w)) for w in got] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_save_load_lora_round_trip_and_init(tmp_path):
    cfg = synth.ArchConfig(hidden=64, inter=128, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=16, vocab=96)
    g = torch.Generator().manual_seed(4)
    init = L.init_factors(cfg, R, torch.Generator().manual_seed(4))
    # peft's init: A = kaiming_uniform_(a=sqrt(5)) (bound 1 / sqrt(in)), B = 0, drawn in the same order from the same generator
    for i, mod, ab in L.names(cfg.n_layers):
        t = init[L.engine_name(i, mod, ab)]
        if ab == "A":
            want = torch.empty_like(t)
            torch.nn.init.kaiming_uniform_(want, a=math.sqrt(5), generator=g)
            assert torch.equal(t, want)
            assert float(t.abs().max()) <= 1 / math.sqrt(L.module_dims(cfg, mod)[0])
        else:
            assert float(t.abs().max()) == 0.0
    fac = {L.peft_key(i, m, ab): torch.randn(L.shape(cfg, L.engine_name(i, m, ab), R)) for i, m, ab in L.names(cfg.n_layers)}
    proj = {"model.mm_projector.norm.weight": torch.ones(64)}
    L.write_adapter(str(tmp_path), R, ALPHA, 0.05, fac, proj)
    conf = json.load(open(tmp_path / "adapter_config.json"))
    assert conf["peft_type"] == "LORA" and conf["task_type"] == "CAUSAL_LM" and conf["r"] == R and conf["lora_alpha"] == ALPHA
    assert conf["lora_dropout"] == 0.05 and conf["bias"] == "none"
    assert sorted(conf["target_modules"]) == sorted(["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"])
    cfg_r, tensors = L.read_adapter(str(tmp_path))
    assert set(tensors) == set(fac) and all(v.dtype == torch.bfloat16 for v in tensors.values())
    assert "base_model.model.model.layers.1.mlp.down_proj.lora_A.weight" in tensors
    deltas = W.load_lora(str(tmp_path))
    assert set(deltas) == {L.reference_weight_key(i, m) for i in range(2) for m in L.MODULES}
    for i in range(2):
        for m in L.MODULES:
            a = fac[L.peft_key(i, m, "A")].bfloat16().float()
            b = fac[L.peft_key(i, m, "B")].bfloat16().float()
            assert torch.allclose(deltas[L.reference_weight_key(i, m)], b @ a * (ALPHA / R), rtol=1e-6, atol=1e-6)
    pj = dict(W.iter_projector(str(tmp_path / "non_lora_trainables.bin")))
    assert set(pj) == {"model.mm_projector.norm.weight"}
    assert set(L.peft_to_engine(2).values()) == {L.engine_name(i, m, ab) for i, m, ab in L.names(2)}
