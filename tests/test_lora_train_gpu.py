"""Stage-2 LoRA finetune step on the HIP path (vz_hip.train.Stage2Trainer) against the torch restatement tests/lora_ref.py (pinned to
transformers + a peft-equivalent wrapper by tests/test_lora_cpu.py), on the 2-layer synthetic model of tests/test_train_gpu.py.

Tolerance as for Stage 1 (tests/test_train_gpu.py): ||g_hip - g_fp32|| <= 2.5 e_or + 2e-3 relative, cosine >= 0.999, with e_or the
restatement's own bf16-policy distance from its fp32 gradients, per tensor."""
import pytest
import torch

from util import band_tol, errs, record

pytestmark = pytest.mark.gpu

R, ALPHA, SEED = 128, 256.0, 0x5EED1234ABCD


@pytest.fixture(scope="module")
def env():
    from oracle import pin_train_step, train_oracle as T, vz_oracle as O
    from vz_hip import synth
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    cfg = synth.ArchConfig(n_layers=2)
    hf = VisZephyrConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=2, num_attention_heads=cfg.n_heads,
                         num_key_value_heads=cfg.n_kv_heads, vocab_size=cfg.vocab, rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta,
                         sliding_window=cfg.sliding_window, eos_token_id=2, pad_token_id=2, bos_token_id=1)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    model = VisZephyrForCausalLM.from_synthetic(hf, seed=0, max_batch=2, max_ctx=256, max_tiles=4, max_text=64)
    sd = {k: v.cpu() for k, v in synth.iter_state_dict(cfg, 0, device=model.device)}
    torch.cuda.synchronize()
    return dict(cfg=cfg, hf=hf, model=model, sd=sd, T=T, O=O, batch=pin_train_step.batch(cfg), feats={})


def _trainer(env, dropout):
    from vz_hip.train import Stage2Trainer
    tr = Stage2Trainer(env["model"], r=R, alpha=ALPHA, dropout=dropout, seed=SEED)
    tr.set_masters_from_reference((k, v) for k, v in env["sd"].items() if k.startswith("model.mm_projector."))
    return tr


def _random_factors(cfg, seed=7):
    """non-zero A and B (peft's B = 0 would hide every path through B)"""
    from vz_hip import lora as L
    g = torch.Generator().manual_seed(seed)
    out = {}
    for i, mod, ab in L.names(cfg.n_layers):
        shape = L.shape(cfg, L.engine_name(i, mod, ab), R)
        bound = shape[1] ** -0.5 if ab == "A" else 0.02
        out[(i, mod, ab)] = (torch.rand(shape, generator=g) * 2 - 1) * bound
    return out


def _check_against_restatement(env, dropout, tag):
    import lora_ref
    from vz_hip import lora as L
    cfg, sd = env["cfg"], env["sd"]
    ids, mask, lab, images = env["batch"]
    fac = _random_factors(cfg)
    tr = _trainer(env, dropout)
    try:
        tr.set_lora({L.engine_name(i, m, ab): t for (i, m, ab), t in fac.items()})
        tr.zero_grad()
        loss = tr.forward_backward(ids, mask, lab, images)
        grads = {k: v.detach().float().cpu().clone() for k, v in tr.reference_grads().items()}
    finally:
        tr.close()
    # the restatement computes on the rounded factors the device holds (the bf16 working copies)
    lora = {(i, m): (fac[(i, m, "A")].bfloat16().float(), fac[(i, m, "B")].bfloat16().float()) for i in range(cfg.n_layers) for m in L.MODULES}
    kw = dict(p=dropout, seed=SEED, feats=env["feats"])
    loss32, g32 = lora_ref.stage2_grads(cfg, sd, lora, ALPHA / R, ids, mask, lab, images, P=env["O"].FP32, **kw)
    loss16, g16 = lora_ref.stage2_grads(cfg, sd, lora, ALPHA / R, ids, mask, lab, images, P=env["O"].BF16, **kw)
    assert set(grads) == set(g32), sorted(set(grads) ^ set(g32))[:6]
    assert sum(1 for k in grads if ".lora_" in k) == 2 * 7 * cfg.n_layers and sum(1 for k in grads if "mm_projector" in k) == 165
    e_loss_or = abs(float(loss16) - float(loss32)) / float(loss32)
    e_loss = abs(loss - float(loss32)) / float(loss32)
    assert e_loss <= 2.5 * e_loss_or + 2e-3, (loss, float(loss32), float(loss16))
    worst = ("", 0.0, 0.0)
    for n in sorted(g32):
        e_or = errs(g16[n], g32[n])[1]
        e_hip = errs(grads[n], g32[n])[1]
        cos = float(torch.nn.functional.cosine_similarity(grads[n].double().reshape(1, -1), g32[n].double().reshape(1, -1)))
        if e_hip / max(e_or, 1e-9) > worst[1] / max(worst[2], 1e-9) or not worst[0]:
            worst = (n, e_hip, e_or)
        assert cos >= 0.999, (n, cos)
        assert e_hip <= 2.5 * e_or + 2e-3, f"{n}: hip vs fp32 restatement {e_hip:.3e}, its bf16 band {e_or:.3e}"
    record(f"stage2 {tag}", loss=loss, loss_fp32=float(loss32), worst_tensor=worst[0], e_hip=worst[1], e_oracle_bf16=worst[2])
    return loss


def test_dropout_op_matches_numpy_bit_for_bit():
    from vz_hip import binding as BD, lora as L
    g = torch.Generator().manual_seed(3)
    S, nb, cols = 37, 3, 448
    x = (torch.randn(nb * S, cols, generator=g) * 3).bfloat16()
    for p, step, base, stride, tag in ((0.05, 4, 5, 50, 11), (0.5, 0, 0, 37, 0), (0.0, 9, 2, 40, 223)):
        got = BD.lora_dropout(x.cuda(), S, base, stride, tag, step, SEED, p, 2.0).cpu()
        keep = L.dropout_keep(SEED, step, tag, nb * S, cols, S, base, stride, p)
        want = L.dropout_apply(x, keep, 2.0, p)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (p, int((got != want).sum()))
        assert torch.equal(got != 0, torch.from_numpy(keep) & (x != 0))
    # the sampling tail shares the Philox rounds: its draw is pinned by tests/test_sampling_gpu.py against oracle/sampling_oracle.py


def test_gradients_p0_random_factors(env):
    env["loss_p0"] = _check_against_restatement(env, 0.0, "p=0")


def test_gradients_dropout_injected_masks(env):
    _check_against_restatement(env, 0.05, "p=0.05")


def test_peft_init_is_stage1_bit_for_bit(env):
    from vz_hip.train import Stage1Trainer
    ids, mask, lab, images = env["batch"]
    t1 = Stage1Trainer(env["model"])
    try:
        t1.zero_grad()
        loss1 = t1.forward_backward(ids, mask, lab, images)
        g1 = {k: v.detach().clone() for k, v in t1.reference_grads().items()}
    finally:
        t1.close()
    tr = _trainer(env, 0.05)
    try:
        tr.init_lora(torch.Generator().manual_seed(1))
        tr.zero_grad()
        loss2 = tr.forward_backward(ids, mask, lab, images)
        assert loss2 == loss1, (loss2, loss1)
        grads = tr.reference_grads()
        for k, v in g1.items():              # B = 0: the branch adds exact zeros, the projector sees Stage 1's gradient
            assert torch.equal(grads["base_model.model." + k], v), k
        for k, v in grads.items():
            if ".lora_A." in k:
                assert float(v.abs().max()) == 0.0, k
            elif ".lora_B." in k:
                assert float(v.abs().max()) > 0.0, k
    finally:
        tr.close()


def test_micro_batches_allreduce_adamw_and_second_step(env):
    from vz_hip import lora as L
    T = env["T"]
    ids, mask, lab, images = env["batch"]
    tr = _trainer(env, 0.05)
    try:
        fac = _random_factors(env["cfg"], seed=11)
        tr.set_lora({L.engine_name(i, m, ab): t for (i, m, ab), t in fac.items()})
        tr.zero_grad()
        loss_one = tr.forward_backward(ids, mask, lab, images)
        g_one = {k: v.detach().clone() for k, v in tr.reference_grads().items() if ".lora_" in k}
        tr.zero_grad()
        loss_two = tr.forward_backward(ids, mask, lab, images, micro_batch=1)
        assert abs(loss_two - loss_one) <= 2e-4 * abs(loss_one), (loss_two, loss_one)
        worst = 0.0
        for k, v in tr.reference_grads().items():
            if ".lora_" in k:
                worst = max(worst, errs(v, g_one[k])[1])
        record("stage2 micro-batches", loss_one=loss_one, loss_two=loss_two, worst_lora_grad_rel=worst)
        assert worst <= 2e-2, worst
        # a one-rank all-reduce leaves every gradient as it was
        tr.init_comm_single_rank()
        before = {k: v.detach().clone() for k, v in tr.reference_grads().items() if ".lora_" in k}
        tr.all_reduce()
        torch.cuda.synchronize()
        for k, v in tr.reference_grads().items():
            if ".lora_" in k:
                assert torch.equal(v, before[k]), k
        # AdamW over the factors: torch.optim.AdamW's arithmetic (train_oracle.adamw_step) on the masters
        picks = ["lora.0.q.A", "lora.0.gate.B", "lora.1.down.A", "lora.1.v.B"]
        p0 = {n: (tr.master(n).detach().clone(), tr.grad(n).detach().clone()) for n in picks}
        lr = 2e-4
        tr.optimizer_step(lr)
        for n in picks:
            p, g = p0[n]
            zero = torch.zeros_like(p, dtype=torch.float64, device="cpu")
            want, _, _ = T.adamw_step(p.double().cpu(), g.double().cpu(), zero, zero.clone(), 1, lr)
            d_want, d_got = want - p.double().cpu(), tr.master(n).double().cpu() - p.double().cpu()
            assert errs(d_got, d_want)[1] <= 2e-3, (n, errs(d_got, d_want))
            assert float(tr.grad(n).abs().max()) == 0.0
        loss_after = tr.forward_backward(ids, mask, lab, images)
        tr.optimizer_step(lr)
        loss_after2 = tr.forward_backward(ids, mask, lab, images)
        record("stage2 adamw", loss=loss_one, after_one_step=loss_after, after_two=loss_after2)
        assert loss_after != loss_one and loss_after2 != loss_after
        assert loss_after < loss_one
    finally:
        tr.close()


def test_arena_is_sized_by_the_step_itself_with_lora(env):
    """tests/test_train_gpu.py::test_arena_is_sized_by_the_step_itself with the LoRA branches' buffers in the carving: the step that
    sizes the arena uses all of it, the smaller micro-batches after it fit inside."""
    ids, mask, lab, images = env["batch"]
    tr = _trainer(env, 0.05)
    try:
        tr.init_lora(torch.Generator().manual_seed(1))
        tr.zero_grad()
        tr.forward_backward(ids, mask, lab, images)
        arena, peak = tr.ws_info()
        assert peak == arena > 0, (arena, peak)
        tr.zero_grad()
        tr.forward_backward(ids, mask, lab, images, micro_batch=1)
        arena_mb, peak_mb = tr.ws_info()
        assert arena_mb == arena and 0 < peak_mb <= arena, (arena_mb, peak_mb, arena)
        record("stage2 step arena", batch_bytes=arena, last_micro_batch_bytes=peak_mb)
    finally:
        tr.close()


def test_save_then_load_pretrained_model_round_trip(tmp_path, monkeypatch):
    """save() -> load_pretrained_model(dir, model_base=base, model_name="...-lora"), the reference's LoRA load mode, on a tiny on-disk
    base checkpoint (tests/test_loader_gpu.py::_write_checkpoint).  The reloaded model merges W += B A alpha / r of the saved factors
    and computes the trainer's p = 0 loss within 2e-3 (Stage 1's loss tolerance); the factors move the loss by far more than that,
    so a reload that merged nothing, or the wrong deltas, fails."""
    import huggingface_hub.constants as hc
    import transformers
    from test_loader_gpu import _Tok, _write_checkpoint
    from vz_hip import lora as L, synth, weights as W
    from vz_hip.train import Stage2Trainer
    from vis_zephyr.model.builder import load_pretrained_model
    cfg = synth.ArchConfig(n_layers=2, vocab=300)
    base, ckpt, cache = _write_checkpoint(tmp_path, cfg, synth, 300)
    monkeypatch.setenv("HF_HUB_CACHE", str(cache))
    monkeypatch.setenv("HF_HUB_OFFLINE", "1")
    monkeypatch.setattr(hc, "HF_HUB_CACHE", str(cache), raising=False)
    monkeypatch.setattr(transformers.AutoTokenizer, "from_pretrained", staticmethod(lambda *a, **k: _Tok(300)))
    tiles = synth.synth_tiles(2, seed=21)
    ids = synth.synth_ids(40, 300, image_pos=1, seed=22).unsqueeze(0)
    mask = torch.ones_like(ids)
    lab = ids.clone()
    lab[ids == -200] = -100
    lab[:, :2] = -100

    def run(model):
        dev = model.device
        out = model(input_ids=ids.to(dev), attention_mask=mask.to(dev), labels=lab.to(dev), images=[tiles.to(dev)])
        return float(out.loss), out.logits.float().cpu()

    # the Stage-1 checkpoint (base + mm_projector.bin) is the starting point of Stage 2
    _, m1, _, _ = load_pretrained_model(str(ckpt), str(base), "vis-zephyr-7b-v1-pretrain", max_ctx=256)
    loss_s1, logits_s1 = run(m1)
    g = torch.Generator().manual_seed(5)
    fac = {}
    for i, mod, ab in L.names(cfg.n_layers):
        shape = L.shape(m1.arch, L.engine_name(i, mod, ab), R)
        fac[L.engine_name(i, mod, ab)] = (torch.rand(shape, generator=g) * 2 - 1) * (shape[1] ** -0.5 if ab == "A" else 1.0)
    out_dir = tmp_path / "vis-zephyr-7b-finetune-lora"
    tr = Stage2Trainer(m1, r=R, alpha=ALPHA, dropout=0.0, seed=SEED)
    try:
        tr.set_lora(fac)
        loss_tr = tr.forward_backward(ids, mask, lab, [tiles])
        tr.save(str(out_dir))
    finally:
        tr.close()
    for f in ("adapter_config.json", "adapter_model.safetensors", "non_lora_trainables.bin", "config.json"):
        assert (out_dir / f).exists(), f
    del m1
    torch.cuda.empty_cache()
    _, m2, _, _ = load_pretrained_model(str(out_dir), str(base), "vis-zephyr-7b-finetune-lora", max_ctx=256)
    assert m2.engine.cfg.vocab == 301
    # the merged weights are the base's + B A alpha / r of the saved bf16 factors, rounded once to bf16
    base_sd = dict(W.iter_backbone(str(base)))
    deltas = W.load_lora(str(out_dir))
    assert set(deltas) == {L.reference_weight_key(i, m) for i in range(cfg.n_layers) for m in L.MODULES}
    for i in range(cfg.n_layers):
        key = L.reference_weight_key(i, "o")
        want = (base_sd[key].float() + fac[L.engine_name(i, "o", "B")].bfloat16().float() @ fac[L.engine_name(i, "o", "A")].bfloat16().float()
                * (ALPHA / R)).to(torch.bfloat16)
        assert torch.equal(m2.engine.w[f"llm.{i}.o.w"].cpu(), want), i
    loss_m, logits_m = run(m2)
    # the bf16 band: the trainer adds the branch in bf16 (tests/lora_ref.py's BF16 policy), the reloaded model computes with the merged
    # weights rounded once to bf16 (the Stage-1 restatement on those weights); each sits within 2.5x its restatement's distance from
    # the fp32 loss (tests/test_train_gpu.py's criterion) + 2e-3 of Stage 1's loss tolerance
    import lora_ref
    from oracle import train_oracle as T, vz_oracle as O
    clip_dir = W.resolve_hub_path("openai/clip-vit-large-patch14-336")
    sd = {k: v.float() for k, v in W.resize_vocab(W.iter_reference_checkpoint(str(ckpt), str(base), clip_dir), 301)}
    ocfg = synth.ArchConfig(n_layers=2, vocab=301)
    lora = {(i, m): (fac[L.engine_name(i, m, "A")].bfloat16().float(), fac[L.engine_name(i, m, "B")].bfloat16().float())
            for i in range(cfg.n_layers) for m in L.MODULES}
    feats = {}
    l32, _ = lora_ref.stage2_grads(ocfg, sd, lora, ALPHA / R, ids, mask, lab, [tiles], P=O.FP32, feats=feats)
    l16b, _ = lora_ref.stage2_grads(ocfg, sd, lora, ALPHA / R, ids, mask, lab, [tiles], P=O.BF16, feats=feats)
    merged = dict(sd)
    merged.update({k: (sd[k] + d).to(torch.bfloat16).float() for k, d in deltas.items()})
    with torch.no_grad():
        l16m = float(T.stage1_loss(ocfg, merged, ids, mask, lab, [tiles], P=O.BF16))
        ref = {}
        for P in (O.FP32, O.BF16):
            _, pos, msk, _, emb, _ = O.prepare_inputs_labels_for_multimodal(ocfg, merged, ids, None, mask, None, lab, [tiles], P=P)
            ref[P.bf16] = O.llm_forward(ocfg, merged, emb, attention_mask=msk, position_ids=pos, P=P)[0]
    l32, l16b = float(l32), float(l16b)
    tol = 2.5 * (abs(l16b - l32) + abs(l16m - l32)) + 2e-3 * abs(l32)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())  # noqa: E731
    e_or, e_m, e_s1 = rel(ref[True], ref[False]), rel(logits_m, ref[False]), rel(logits_s1, ref[False])
    record("stage2 load_pretrained_model round trip", loss_trainer=loss_tr, loss_reloaded=loss_m, loss_stage1=loss_s1, loss_fp32=l32,
           loss_bf16_branch=l16b, loss_bf16_merged=l16m, tol=tol, logits_rel_reloaded=e_m, logits_rel_stage1=e_s1, logits_band=e_or)
    # the trainer and the reloaded model each within their bf16 band of the fp32 loss, and of each other
    assert abs(loss_tr - l32) <= 2.5 * abs(l16b - l32) + 2e-3 * abs(l32), (loss_tr, l32, l16b)
    assert abs(loss_m - l32) <= 2.5 * abs(l16m - l32) + 2e-3 * abs(l32), (loss_m, l32, l16m)
    assert abs(loss_m - loss_tr) <= tol, (loss_m, loss_tr, tol)
    # the reloaded logits sit in the merged model's bf16 band (smoke()'s criterion), the model without the adapter far outside it
    assert e_m <= band_tol(e_or), (e_m, e_or)
    assert e_s1 > 5 * band_tol(e_or), (e_s1, e_or)
