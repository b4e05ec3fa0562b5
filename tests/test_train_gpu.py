"""Stage-1 pretrain step on the HIP path against the reference's own `loss.backward()` /
`torch.optim.AdamW` (tests/golden/stage1_step.npz, oracle/pin_train_step.py) and against oracle/train_oracle.py run on this box's
host cores: loss, all 165 projector gradients, the AdamW update, micro-batch accumulation, the one-rank RCCL all-reduce.

Tolerance.  The HIP backward carries every gradient stream in bf16 (as the forward carries activations); the oracle's bf16
policy (forward AND backward rounded at the same store points, oracle/train_oracle.py::stage1_grads(P=BF16)) measures what that
costs per tensor: e_or = ||g_bf16 - g_fp32|| / ||g_fp32||.  Every HIP gradient must satisfy ||g_hip - g_fp32|| <= 2.5 e_or + 2e-3
relative, with cosine >= 0.999, and the reference's own gradient norms / slices (fixtures) bound it in absolute terms."""
import numpy as np
import pytest
import torch

from util import errs, record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from oracle import pin_train_step, train_oracle as T, vz_oracle as O
    from vz_hip import synth
    from vz_hip.train import Stage1Trainer
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    cfg = synth.ArchConfig(n_layers=2)
    hf = VisZephyrConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=2, num_attention_heads=cfg.n_heads,
                         num_key_value_heads=cfg.n_kv_heads, vocab_size=cfg.vocab, rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta,
                         sliding_window=cfg.sliding_window, eos_token_id=2, pad_token_id=2, bos_token_id=1)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    model = VisZephyrForCausalLM.from_synthetic(hf, seed=0, max_batch=2, max_ctx=256, max_tiles=4, max_text=64)
    sd = {k: v.cpu() for k, v in synth.iter_state_dict(cfg, 0, device=model.device)}
    tr = Stage1Trainer(model)
    tr.set_masters_from_reference((k, v) for k, v in sd.items() if k.startswith("model.mm_projector."))
    gold = dict(np.load(__import__("os").path.join(__import__("util").GOLDEN, "stage1_step.npz"), allow_pickle=False))
    ids, mask, lab, images = pin_train_step.batch(cfg)
    torch.cuda.synchronize()
    return dict(cfg=cfg, model=model, sd=sd, tr=tr, T=T, O=O, gold=gold, batch=(ids, mask, lab, images))


def test_loss_and_all_projector_gradients(env):
    tr, T, O, cfg, sd, g = env["tr"], env["T"], env["O"], env["cfg"], env["sd"], env["gold"]
    ids, mask, lab, images = env["batch"]
    tr.zero_grad()
    loss = tr.forward_backward(ids, mask, lab, images)
    grads = {k: v.detach().float().cpu().clone() for k, v in tr.reference_grads().items()}
    env["grads"] = grads
    # ---- loss: the reference's own number ----
    ref_loss = float(g["loss"])
    record("stage1 loss", hip=loss, reference=ref_loss, rel=abs(loss - ref_loss) / ref_loss)
    assert abs(loss - ref_loss) <= 2e-3 * ref_loss, (loss, ref_loss)
    # ---- the reference's gradient norms and slices (fixtures) ----
    names = [str(n) for n in g["grad_names"]]
    assert set(names) == set(grads), sorted(set(names) ^ set(grads))[:6]
    worst_norm = 0.0
    for n, ref_norm in zip(names, g["grad_norms"]):
        got = float(grads[n].double().norm())
        worst_norm = max(worst_norm, abs(got - ref_norm) / ref_norm)
        assert torch.isfinite(grads[n]).all(), n
    record("stage1 gradient norms vs reference", worst_rel=worst_norm, tensors=len(names))
    assert worst_norm <= 3e-2, worst_norm
    for key in [k for k in g if k.startswith("grad.") and k.endswith(".sub")]:
        n = key[len("grad."):-len(".sub")]
        stride = int(g[f"grad.{n}.stride"])
        mine = grads[n].reshape(-1)[::stride][:4096]
        mx, l2 = errs(mine, torch.from_numpy(g[key]))
        record(f"stage1 gradient slice {n}", max_err=mx, l2_err=l2)
        assert l2 <= 4e-2, (n, l2)
    # ---- every tensor against the oracle's fp32 gradients, inside the oracle's own bf16 band ----
    # (the band - the BF16-policy oracle's own distance from its fp32 gradients, per tensor - is a committed fixture: oracle/band_train_step.py
    # -> tests/golden/stage1_step_band.npz; the fp32 gradients themselves are gigabytes and are computed here)
    loss32, g32 = T.stage1_grads(cfg, sd, ids, mask, lab, images)
    bandfx = np.load(__import__("os").path.join(__import__("util").GOLDEN, "stage1_step_band.npz"), allow_pickle=False)
    band_of = {str(n): float(b) for n, b in zip(bandfx["names"], bandfx["band"])}
    loss16 = float(bandfx["loss_bf16"])
    assert set(band_of) == set(g32)
    assert abs(float(loss32) - ref_loss) <= 1e-5 * ref_loss and abs(float(bandfx["loss_fp32"]) - ref_loss) <= 1e-5 * ref_loss
    worst = ("", 0.0, 0.0)
    for n in sorted(g32):
        e_or = band_of[n]
        e_hip = errs(grads[n], g32[n])[1]
        cos = float(torch.nn.functional.cosine_similarity(grads[n].double().reshape(1, -1), g32[n].double().reshape(1, -1)))
        if e_hip / max(e_or, 1e-9) > worst[1] / max(worst[2], 1e-9) or not worst[0]:
            worst = (n, e_hip, e_or)
        assert cos >= 0.999, (n, cos)
        assert e_hip <= 2.5 * e_or + 2e-3, f"{n}: hip vs fp32 oracle {e_hip:.3e}, oracle's bf16 band {e_or:.3e}"
    record("stage1 gradients vs oracle", worst_tensor=worst[0], e_hip=worst[1], e_oracle_bf16=worst[2], loss_oracle_bf16=float(loss16))


def test_arena_is_sized_by_the_step_itself(env):
    """The step arena is sized by a launch-free pass of the step's own carving (train_engine.hip, "the step's memory"), so a call that
    sizes the arena uses all of it: peak == arena.  A smaller shape after a larger one reuses the arena and reports the peak the same
    shape has on a fresh sizing.  Shapes: the second sample alone as forward_backward(micro_batch=1) runs it (text padded to the
    batch's longest), the Stage-1 batch, then the micro-batch-of-1 path, whose last call is that first shape again."""
    from vz_hip.train import IMAGE_TOKEN_INDEX, Stage1Trainer
    ids, mask, lab, images = env["batch"]
    ids_cpu = ids.cpu().long()
    Lmax = max(int((ids_cpu[b] != IMAGE_TOKEN_INDEX).sum()) for b in range(ids_cpu.shape[0]))
    last = slice(ids_cpu.shape[0] - 1, ids_cpu.shape[0])
    tr = Stage1Trainer(env["model"])          # its first step sizes the arena
    try:
        assert tr.ws_info() == (0, 0)
        tr.zero_grad()
        tr._accumulate(ids_cpu[last], mask.cpu().bool()[last], lab.cpu().long()[last], list(images)[last], 1.0, Lmax)
        arena_one, peak_one = tr.ws_info()
        assert peak_one == arena_one > 0, (arena_one, peak_one)
        tr.zero_grad()
        tr.forward_backward(ids, mask, lab, images)
        arena, peak = tr.ws_info()
        assert peak == arena > arena_one, (arena, peak, arena_one)
        tr.zero_grad()
        tr.forward_backward(ids, mask, lab, images, micro_batch=1)
        arena_mb, peak_mb = tr.ws_info()
        assert arena_mb == arena and peak_mb == peak_one <= arena, (arena_mb, peak_mb, arena, peak_one)
        record("stage1 step arena", batch_bytes=arena, one_sample_bytes=arena_one)
    finally:
        tr.close()


def test_attention_backward_routes_size_their_own_scratch(env):
    """knob 32 (flash_bwd) = 0 sends the Zephyr layers' attention backward through the materialising batched-GEMM route, (32, 1) back to the
    tile-resident one.  The route depends on the knob alone and each carves its own scratch: both steps succeed, the materialising
    step's arena is at least the tile-resident step's need, and both losses are the fixture's."""
    from vz_hip import binding as B
    from vz_hip.train import Stage1Trainer
    ids, mask, lab, images = env["batch"]
    ref_loss = float(env["gold"]["loss"])
    tr = Stage1Trainer(env["model"])
    try:
        with B.tuned(flash_bwd=0):
            tr.zero_grad()
            loss_gemm = tr.forward_backward(ids, mask, lab, images)
            arena_gemm, peak_gemm = tr.ws_info()
        with B.tuned(flash_bwd=1):
            tr.zero_grad()
            loss_flash = tr.forward_backward(ids, mask, lab, images)
            arena_flash, peak_flash = tr.ws_info()
    finally:
        tr.close()
    record("stage1 attention backward routes", loss_batched_gemm=loss_gemm, loss_tile_resident=loss_flash, arena_batched_gemm=arena_gemm,
           peak_tile_resident=peak_flash)
    assert peak_gemm == arena_gemm > 0, (arena_gemm, peak_gemm)
    assert arena_flash == arena_gemm and 0 < peak_flash <= arena_flash, (arena_flash, peak_flash, arena_gemm)
    assert abs(loss_gemm - ref_loss) <= 2e-3 * ref_loss, (loss_gemm, ref_loss)
    assert abs(loss_flash - ref_loss) <= 2e-3 * ref_loss, (loss_flash, ref_loss)


def test_adamw_step_and_second_step(env):
    tr, T, sd = env["tr"], env["T"], env["sd"]
    ids, mask, lab, images = env["batch"]
    if "grads" not in env:
        tr.zero_grad()
        tr.forward_backward(ids, mask, lab, images)
    picks = ["qf.queries", "qf.3.ffn1.w", "qf.0.sa_in.b", "qf.7.ca_kv.w", "qf.pre_norm.w"]
    before = {n: (tr.master(n).clone(), tr.grad(n).clone()) for n in picks}
    tr.optimizer_step(2e-5)
    state = {}
    for n in picks:
        p0, g0 = before[n]
        want, m1, v1 = T.adamw_step(p0.double().cpu(), g0.double().cpu(), torch.zeros_like(p0, dtype=torch.float64, device="cpu"),
                                    torch.zeros_like(p0, dtype=torch.float64, device="cpu"), 1, 2e-5)
        got = tr.master(n).double().cpu()
        d_want, d_got = want - p0.double().cpu(), got - p0.double().cpu()
        assert errs(d_got, d_want)[1] <= 2e-3, (n, errs(d_got, d_want))       # fp32 update arithmetic vs fp64: the step is 2e-5 of the weight
        assert float(tr.grad(n).abs().max()) == 0.0                            # cleared for the next accumulation
        work = tr.eng.w[n]
        assert torch.equal(work.float(), tr.master(n).to(work.dtype).float())   # the engine computes with the rounded master
        state[n] = (want, m1, v1)
    # the model changed: the loss of the same batch moves (down, for a small enough step) and a second step uses t = 2
    loss2 = tr.forward_backward(ids, mask, lab, images)
    assert loss2 < float(env["gold"]["loss"]) + 1e-3
    g2 = {n: tr.grad(n).clone() for n in picks}
    tr.optimizer_step(2e-5)
    for n in picks:
        want, m1, v1 = state[n]
        want2, _, _ = T.adamw_step(want, g2[n].double().cpu(), m1, v1, 2, 2e-5)
        d_want, d_got = want2 - want, tr.master(n).double().cpu() - want
        assert errs(d_got, d_want)[1] <= 5e-3, (n, errs(d_got, d_want))
    record("stage1 adamw", loss_after_one_step=loss2)


def test_micro_batches_accumulate_and_one_rank_allreduce(env):
    """gradient accumulation over micro-batches of 1 (text padded to the BATCH's longest text, as the reference's forward sees it)
    = the full-batch gradients up to bf16 re-association; the RCCL all-reduce over one rank leaves them untouched."""
    tr = env["tr"]
    ids, mask, lab, images = env["batch"]
    from vz_hip import binding as B
    # whole-K tiles for both runs: the tile GEMM's K slices follow the tile count (the CLIP tower of one sample takes them, the
    # full batch's does not), which is re-association beyond the micro-batching this test is about
    with B.tuned(splitk_mid=0):
        tr.zero_grad()
        l_full = tr.forward_backward(ids, mask, lab, images)
        full = {k: v.clone() for k, v in tr.reference_grads().items()}
        tr.zero_grad()
        l_mb = tr.forward_backward(ids, mask, lab, images, micro_batch=1)
    assert abs(l_mb - l_full) <= 2e-4 * abs(l_full)
    worst = 0.0
    for k, v in tr.reference_grads().items():
        worst = max(worst, errs(v, full[k])[1])
    record("stage1 micro-batch accumulation", worst_rel_l2=worst)
    assert worst <= 2e-2
    before = {k: v.clone() for k, v in tr.reference_grads().items()}
    tr.init_comm_single_rank()
    tr.all_reduce()
    torch.cuda.synchronize()
    for k, v in tr.reference_grads().items():
        assert torch.equal(v, before[k])


def test_data_parallel_mean_of_rank_gradients(env):
    """What the data-parallel all-reduce must produce (the reference: DeepSpeed ZeRO-2 under HF's Trainer AVERAGES the ranks' mean-loss
    gradients; round 2 summed them): two ranks played in turn on this GPU - each back-propagates the mean loss of ITS sample - and the
    mean of the two gradient arenas (ncclAvg's arithmetic, done here with torch on the arena views) against the single-rank gradient
    of the two-sample batch.  Both samples carry the same number of text ids, so the Q-Former's text padding (Appendix A Q3) and the
    target counts agree and mean-of-means = the global batch's gradient up to bf16 re-association; the SUM would be 2 x that."""
    tr, cfg, synth = env["tr"], env["cfg"], __import__("vz_hip.synth", fromlist=["synth"])
    from vz_hip import binding as B
    ids = torch.stack([synth.synth_ids(20, cfg.vocab, image_pos=1, seed=41), synth.synth_ids(20, cfg.vocab, image_pos=1, seed=42)])
    mask = torch.ones_like(ids)
    lab = ids.clone()
    lab[ids == -200] = -100
    images = [synth.synth_tiles(2, seed=43), synth.synth_tiles(1, seed=44)]
    with B.tuned(splitk_mid=0):          # whole-K tiles on both sides (see the micro-batch test)
        per_rank = []
        for b in range(2):
            tr.zero_grad()
            tr.forward_backward(ids[b:b + 1], mask[b:b + 1], lab[b:b + 1], [images[b]])      # normalised by the rank's OWN target count
            per_rank.append({k: v.clone() for k, v in tr.reference_grads().items()})
        tr.zero_grad()
        tr.forward_backward(ids, mask, lab, images)
        both = {k: v.clone() for k, v in tr.reference_grads().items()}
        tr.zero_grad()
    worst_avg, worst_sum = 0.0, 0.0
    for k in both:
        worst_avg = max(worst_avg, errs(0.5 * (per_rank[0][k] + per_rank[1][k]), both[k])[1])
        worst_sum = max(worst_sum, errs(per_rank[0][k] + per_rank[1][k], both[k])[1])
    record("stage1 data-parallel semantics", mean_of_rank_gradients_vs_global_batch=worst_avg, sum_vs_global_batch=worst_sum)
    assert worst_avg <= 2e-2, worst_avg
    assert worst_sum >= 0.9               # what round 2's ncclSum handed AdamW: twice the gradient


def test_save_projector_writes_the_reference_checkpoint(env, tmp_path):
    """`Stage1Trainer.save_projector` = the reference's Stage-1 checkpoint (ref:vis_zephyr/train/vis_zephyr_trainer.py:304-348:
    `mm_projector.bin`, keys `model.mm_projector.*`, SURVEY Appendix C shapes); loading it back through the engine's own loader
    (vz_hip/weights.py, the path ref:vis_zephyr/model/builder.py:118-120 takes) reproduces the working copies bit for bit."""
    tr = env["tr"]
    path = tr.save_projector(str(tmp_path))
    sd = torch.load(path, map_location="cpu")
    cfg = tr.eng.cfg
    H, KD = cfg.hidden, cfg.qf_kv_dim
    assert len(sd) == 165 and all(k.startswith("model.mm_projector.") for k in sd)
    assert tuple(sd["model.mm_projector.learned_queries"].shape) == (32, H)
    assert tuple(sd["model.mm_projector.blocks.3.cross_attn.k_proj_weight"].shape) == (H, KD)
    assert tuple(sd["model.mm_projector.blocks.3.cross_attn.v_proj_weight"].shape) == (H, KD)
    assert tuple(sd["model.mm_projector.blocks.3.cross_attn.in_proj_bias"].shape) == (3 * H,)
    assert tuple(sd["model.mm_projector.blocks.0.self_attn.in_proj_weight"].shape) == (3 * H, H)
    assert all(v.dtype == torch.bfloat16 for v in sd.values())
    # k | v halves and the q | k | v bias against the engine's stacked tensors (bf16 of the fp32 masters = the engine's working copies)
    kv = tr.master("qf.3.ca_kv.w")
    assert torch.equal(sd["model.mm_projector.blocks.3.cross_attn.k_proj_weight"], kv[:H].to(torch.bfloat16).cpu())
    assert torch.equal(sd["model.mm_projector.blocks.3.cross_attn.v_proj_weight"], kv[H:].to(torch.bfloat16).cpu())
    qb, kvb = tr.master("qf.3.ca_q.b"), tr.master("qf.3.ca_kv.b")
    assert torch.equal(sd["model.mm_projector.blocks.3.cross_attn.in_proj_bias"], torch.cat([qb, kvb]).to(torch.bfloat16).cpu())
    # round trip through the loader's key map
    before = {n: tr.eng.w[n].clone() for n in ("qf.queries", "qf.3.ca_kv.w", "qf.5.ffn2.w", "qf.7.sa_in.w")}
    tr.eng.load_weights((k, v) for k, v in sd.items())
    tr.eng.finalize()
    for n, t in before.items():
        assert torch.equal(tr.eng.w[n], t), n


def test_long_sequence_step_against_the_reference(env):
    """The length the reference trains up to (ref:script/pretrain.sh:44 --model_max_length 2048, with FlashAttention-2 and gradient
    checkpointing, ref:vis_zephyr/train/train_mem.py:8-10): one sample of 5 tiles + a 900-id caption -> S = 1059 spliced rows, against
    the reference's own loss.backward() at that length (tests/golden/stage1_long.npz, oracle/pin_train_step.py --long).  The attention
    backward of the frozen Zephyr layers runs at S > 1024; its scratch is bounded per pass (train_engine.hip ATTN_BWD_CAP), not per batch."""
    import os
    from oracle import pin_train_step
    from util import GOLDEN
    path = os.path.join(GOLDEN, "stage1_long.npz")
    if not os.path.exists(path):
        pytest.skip("tests/golden/stage1_long.npz not generated (oracle/pin_train_step.py --long)")
    g = dict(np.load(path, allow_pickle=False))
    from vz_hip import synth
    from vz_hip.train import Stage1Trainer
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    cfg = env["cfg"]
    hf = VisZephyrConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=2, num_attention_heads=cfg.n_heads,
                         num_key_value_heads=cfg.n_kv_heads, vocab_size=cfg.vocab, rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta,
                         sliding_window=cfg.sliding_window, eos_token_id=2, pad_token_id=2, bos_token_id=1)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    model = VisZephyrForCausalLM.from_synthetic(hf, seed=0, max_batch=1, max_ctx=1100, max_tiles=5, max_text=912)
    tr = Stage1Trainer(model)
    tr.set_masters_from_reference((k, v) for k, v in env["sd"].items() if k.startswith("model.mm_projector."))
    ids, mask, lab, images = pin_train_step.long_batch(cfg)
    tr.zero_grad()
    loss = tr.forward_backward(ids, mask, lab, images)
    ref_loss = float(g["loss"])
    record("stage1 long-sequence loss", hip=loss, reference=ref_loss, rel=abs(loss - ref_loss) / ref_loss, S=899 + 160)
    assert abs(loss - ref_loss) <= 2e-3 * ref_loss, (loss, ref_loss)
    grads = tr.reference_grads()
    names = [str(n) for n in g["grad_names"]]
    worst = 0.0
    for n, ref_norm in zip(names, g["grad_norms"]):
        got = float(grads[n].double().norm())
        assert np.isfinite(got), n
        worst = max(worst, abs(got - ref_norm) / max(ref_norm, 1e-30))
    record("stage1 long-sequence gradient norms vs reference", worst_rel=worst, tensors=len(names))
    assert worst <= 5e-2, worst
    for key in [k for k in g if k.startswith("grad.") and k.endswith(".sub")]:
        n = key[len("grad."):-len(".sub")]
        stride = int(g[f"grad.{n}.stride"])
        mine = grads[n].reshape(-1)[::stride][:4096]
        mx, l2 = errs(mine.cpu(), torch.from_numpy(g[key]))
        record(f"stage1 long-sequence gradient slice {n}", max_err=mx, l2_err=l2)
        assert l2 <= 6e-2, (n, l2)
    del tr, model
    torch.cuda.empty_cache()
