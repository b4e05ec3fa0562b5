#!/usr/bin/env python
"""bench.py - image->first-token latency + decode tokens/s of the Vision-Zephyr hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[2], the configuration the metric is quoted on): Zephyr-7B-beta
(32 layers, random-init hash weights, bf16) + CLIP ViT-L/14-336 + Q-Former, ONE request of 5 anyres
tiles (4 crops + 1 global) and a 1889-id prompt -> spliced sequence S = 2048, 128 greedy new tokens.
One "step" = one full `VisZephyrForCausalLM.generate` on that request, inputs resident in HBM:
  image->first-token  = tiles+ids -> CLIP -> fusion -> Q-Former -> splice -> 32-layer prefill -> argmax
  decode              = 127 further tokens against the KV cache.
`value` = decode tokens/s (whole job); `image_to_first_token_ms` rides in the same JSON line.
N > 1: one process per GPU.  `value` = ONE request over the partition the north star names: Zephyr tensor-parallel over the N
GPUs (RCCL all-reduce / all-gather over xGMI inside the per-token graph) + the image tiles dealt over the same group
(tile data parallelism, one all-gather of visual tokens) - "scaling": "strong".  Beside it, as `replicas`: one request per GPU,
no data-path collective (the reference's own multi-GPU inference scheme, ref:script/eval/eval_qa.sh:21-47).  The TP engine is
measured by child processes with a time limit; if RCCL fails there the line falls back to the replica numbers and says so.

A plain run sets up, warms up, times the K steps and prints the line (plus the outputs, with --dump-outputs).
--dump-outputs DIR: after the timed steps, rank 0 writes what its last timed step returned to the caller - the greedy ids,
[1, new_tokens] - as DIR/generated_ids.npy (float64).  The inputs are seeded, so two builds can be compared id for id.

--full adds the extra objects, measured after the timed region: `roofline` (the dominant kernel by time: the decode
weight-streaming GEMV, HBM-bound; HIP events on the launch stream in an instrumented replay of decode steps), `roofline_prefill`
(MFMA tile GEMM of the prefill, same method), `parity` (the request against the reference's fixture), `streamer_path`,
`persistent_kernel`, `fp8_weights` (the W8A16 engine, in a child process), `cpu_baseline` (the CPU oracle = port of the
reference's fp32 CPU path, timed on the host cores on a bounded sample) and, in tensor-parallel mode, `xgmi` (per-collective
times and the one-shot all-reduce probe).  Without --full those keys are absent or null.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "vision-zephyr_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0      # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
MFMA_BF16_PEAK_TF = 2500.0  # dense bf16 MFMA peak


def build_model(n_layers, device, max_ctx, tp_size=1, tp_rank=0, weight_fp8=False):
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    hf = VisZephyrConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=n_layers, num_attention_heads=32,
                         num_key_value_heads=8, vocab_size=32000, rms_norm_eps=1e-5, sliding_window=4096,
                         eos_token_id=2, pad_token_id=2, bos_token_id=1)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    hf.image_aspect_ratio = "anyres"
    hf.mm_grid_pinpoints = "[[336, 672], [672, 336], [336, 1008], [1008, 336], [672, 672]]"
    hf.mm_hidden_size = 5120
    hf.mm_vision_select_layer = "-2,-5,-8,-11,6"
    return VisZephyrForCausalLM.from_synthetic(hf, seed=0, device=device, max_batch=1, max_ctx=max_ctx, max_tiles=5,
                                               max_text=2048, tp_size=tp_size, tp_rank=tp_rank, weight_fp8=weight_fp8)


def algorithmic_work(cfg, S, n_tiles):
    """SURVEY.md section 8(d) figures: bytes per decoded token (weights, bf16) and prefill linear FLOPs."""
    H, I, V, L = cfg.hidden, cfg.inter, cfg.vocab, cfg.n_layers
    qkv = (cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim
    per_layer_w = qkv * H + H * H + 2 * I * H + I * H
    decode_weight_bytes = 2 * (L * per_layer_w + V * H)                       # 14.22 GB at L=32 (lm_head incl., embedding row excl.)
    prefill_linear_flops = 2 * S * L * per_layer_w + 2 * 1 * V * H            # generate(): lm_head on the last row only
    return decode_weight_bytes, prefill_linear_flops


def pmc_traffic(persist=True):
    """HBM read bytes per launch of the dominant kernel from the committed PMC pass (rocprofv3 --pmc FETCH_SIZE in its own run, x1024 x2
    per the gfx950 correction); PMC counters cannot be read from inside this process."""
    names = ("r03_pmc_decode_token_fetch.json",) if persist else ("r03_pmc_gemv_fetch.json", "r02_pmc_gemv_fetch.json", "r01_pmc_gemv_fetch.json")
    for name in names:
        try:
            with open(os.path.join(REPO, "profiles", name)) as f:
                return int(json.load(f)["hbm_read_bytes_per_launch"])
        except Exception:
            continue
    return None


BAND, BAND_ABS = 1.15, 5e-4     # tests/util.py: ||hip - reference|| <= BAND * ||bf16 oracle - reference|| + BAND_ABS


def parity_check(model, ids, tiles, n_layers):
    """the request of this bench against the REFERENCE's own output for it (tests/golden/pin_l32_c2.npz: BASELINE configs[2] through
    the imported reference on bf16-rounded weights, fp32 arithmetic - oracle/pin_against_reference.py --configs2) inside the
    request's own bf16 band (pin_l32_c2_band.npz: the BF16-policy oracle on the same request, oracle/band_configs2.py) - the band
    tests/test_depth32_gpu.py::test_configs2_against_the_reference_fixture_at_32_layers holds it to: the prefill's last-row logits must sit inside 1.15 x the band, and where the free-running greedy ids leave the
    reference's the reference's own top-2 gap at that step must be inside the step's measured error (a near-tie).  Runs outside
    the timed region."""
    import numpy as np
    path = os.path.join(REPO, "tests", "golden", f"pin_l{n_layers}_c2.npz")
    bpath = os.path.join(REPO, "tests", "golden", f"pin_l{n_layers}_c2_band.npz")
    if not (os.path.exists(path) and os.path.exists(bpath)):
        return {"checked": False, "why": f"no fixture for {n_layers} layers"}
    g, gb = np.load(path), np.load(bpath)
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))  # noqa: E731
    eng = model.engine
    emb = model.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [tiles])[4]
    S = emb.shape[1]
    _, last = eng.prefill(emb, [S])
    lo = last[0].float().cpu().numpy()
    e_last = rel(lo, g["F16.logits.last"])
    band_last = rel(gb["C2.bf16_oracle.logits.last"], g["F16.logits.last"])
    n = int(g["F16.generate.ids"].shape[1])
    got = model.generate(input_ids=ids, images=[tiles], do_sample=False, max_new_tokens=n, eos_token_id=None, pad_token_id=2)[0].tolist()
    want = g["F16.generate.ids"][0].tolist()
    first_div = next((i for i in range(n) if got[i] != want[i]), -1)
    out = {"checked": True, "reference": "W16 (reference code, bf16-rounded weights, fp32 CPU arithmetic)", "first_id": got[0],
           "last_row_logits_rel_l2": round(e_last, 5), "bf16_band_last_row": round(band_last, 5),
           "tolerance": f"{BAND} x band + {BAND_ABS}", "greedy_ids_equal_until": first_div if first_div >= 0 else n, "of": n}
    ok = int(np.argmax(lo)) == got[0] and e_last <= BAND * band_last + BAND_ABS
    if ok and first_div == 0:
        # the FIRST id leaves the reference's: allowed only as a near-tie measured on this very row (the whole row is in the fixture)
        ref_row = g["F16.logits.last"].astype(np.float64)
        gap = float(ref_row[want[0]] - ref_row[got[0]])
        tol = 4.0 * e_last * float(np.sqrt((ref_row ** 2).mean()))
        out["near_tie_at_divergence"] = {"step": 0, "reference_gap_to_the_hip_choice": round(gap, 5), "tolerance_4x_step_error_x_rms": round(tol, 5),
                                         "step_logits_rel_l2": round(e_last, 5)}
        ok = gap < tol
    elif ok and first_div > 0:
        # the logits of the step where the ids part: teacher-forced on the shared prefix (= the free-running logits of that step)
        _, last = eng.prefill(emb, [S])
        eng.decode_begin(torch.tensor(want[:1], dtype=torch.int32), [S], [S])
        lg = None
        for t in range(1, first_div + 1):
            _, lg = eng.decode_steps(1, return_logits=True)
            if t < first_div:
                eng.decode_set_row(0, int(want[t]), S + t, S + t)
        row = lg[0, 0].float().cpu().numpy()
        ref_row = g["F16.step_logits.s64"][first_div]
        e_step = rel(row[::64], ref_row)
        gap = float(g["F16.step_top2.vals"][first_div, 0] - g["F16.step_top2.vals"][first_div, 1])
        tol = 4.0 * e_step * float(np.sqrt((ref_row.astype(np.float64) ** 2).mean()))
        out["near_tie_at_divergence"] = {"step": first_div, "reference_top2_gap": round(gap, 5), "tolerance_4x_step_error_x_rms": round(tol, 5),
                                         "step_logits_rel_l2": round(e_step, 5),
                                         "hip_took_the_reference_runner_up": bool(got[first_div] == int(g["F16.step_top2.ids"][first_div, 1]))}
        ok = gap < tol and int(np.argmax(row)) == got[first_div]
    if not ok:
        raise AssertionError(f"bench request deviates from the reference: {json.dumps(out)}")
    return out


class _Streamer:
    def __init__(self):
        self.n = 0

    def put(self, v):
        self.n += 1

    def end(self):
        pass


def streamer_leg(model, ids, tiles, n_new, steps):
    """the path script/run_cli.sh takes (ref:vis_zephyr/serve/cli.py:155-182): TextStreamer-style callback + a stopping criterion per
    token + do_sample at temperature 0.2 (HF's default top_k 50) - per-token graph replay with the device-side sampler, tokens
    read from the host-visible ring, one step kept in flight."""
    def one():
        tm = {}
        t0 = time.perf_counter()
        out = model.generate(input_ids=ids, images=[tiles], do_sample=True, temperature=0.2, max_new_tokens=n_new, eos_token_id=None,
                             pad_token_id=2, seed=1234, streamer=_Streamer(), stopping_criteria=[lambda i, s, **k: False], timing=tm)
        torch.cuda.synchronize()
        assert out.shape == (1, n_new)
        return tm["t_first_token"] - t0, time.perf_counter() - tm["t_first_token"]
    one()
    r = [one() for _ in range(steps)]
    return {"value": round((n_new - 1) * steps / sum(b for _, b in r), 2), "unit": "tokens/s",
            "image_to_first_token_ms": round(sum(a for a, _ in r) / steps * 1e3, 2),
            "what": "generate(streamer, stopping_criteria, do_sample=True, temperature=0.2): device-side sampling inside the per-token "
                    "hipGraph, 4-byte token read-back through a pinned ring, callbacks of token t under step t+1"}




def persistent_leg(model, ids, tiles, n_new):
    """the same request with every decoded token as ONE resident grid (csrc/decode_persist.hip, opt-in vz_tune_set(28, 1)): the round-3
    answer to 'remove launches, not tune them' - bit-identical ids, measured beside the default launch chain, never `value`."""
    from vz_hip import binding as B
    B.check(B.lib().vz_tune_set(28, 1))
    try:
        def one():
            tm = {}
            t0 = time.perf_counter()
            out = model.generate(input_ids=ids, images=[tiles], do_sample=False, max_new_tokens=n_new, eos_token_id=None, pad_token_id=2, timing=tm)
            torch.cuda.synchronize()
            return out[0].tolist(), time.perf_counter() - tm["t_first_token"], model.engine.persist_mode()
        one()
        ids_p, dt, mode = one()
    finally:
        B.check(B.lib().vz_tune_set(28, 0))
    ids_c = model.generate(input_ids=ids, images=[tiles], do_sample=False, max_new_tokens=n_new, eos_token_id=None, pad_token_id=2)[0].tolist()
    if not mode:
        return {"value": None, "why": "not available on this device (needs 256 CUs)"}
    return {"value": round((n_new - 1) / dt, 2), "unit": "tokens/s", "ids_equal_to_the_launch_chain": ids_p == ids_c,
            "what": "one resident 256-workgroup grid per token (129 weight streams + 32 attention phases as phases with in-launch hand-offs); "
                    "opt-in, slower than the launch chain on MI355X: profiles/r03_persist_stamps.txt"}


def cpu_baseline(cfg_full, S, n_tiles, n_new):
    """The oracle (CPU port of the reference's fp32 path) on this box's host cores, bounded sample:
    1 CLIP tile, 1 Q-Former tile at the full text length, 1 decoder layer of prefill at S, 8 decode tokens
    over 2 layers at context S; per-layer / per-tile times are scaled to 32 layers / 5 tiles."""
    from oracle import vz_oracle as O
    from vz_hip import synth
    torch.set_grad_enabled(False)
    threads = torch.get_num_threads()
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    cfg = cfg_full.small(n_layers=2)
    t0 = time.perf_counter()
    sd = {k: v.cpu() for k, v in synth.iter_state_dict(cfg, 0, device=dev)}
    t_w = time.perf_counter() - t0
    tiles = synth.synth_tiles(1, seed=1)
    L = S - 32 * n_tiles
    ids = synth.synth_ids(L, cfg.vocab, image_pos=-1, seed=2)
    te = O.embed_tokens(sd, ids, O.FP32).unsqueeze(0)
    t0 = time.perf_counter(); feats = O.clip_tower(cfg, sd, tiles); t_clip = time.perf_counter() - t0
    t0 = time.perf_counter(); O.qformer(cfg, sd, feats, te); t_qf = time.perf_counter() - t0
    emb = O.embed_tokens(sd, synth.synth_ids(S, cfg.vocab, image_pos=-1, seed=3), O.FP32).unsqueeze(0)
    cfg1 = cfg.small(n_layers=1)
    t0 = time.perf_counter(); O.llm_forward(cfg1, sd, emb, last_only=True); t_pre1 = time.perf_counter() - t0
    _, cache = O.llm_forward(cfg, sd, emb, last_only=True)
    x = emb[:, :1]
    n_dec = 8
    t0 = time.perf_counter()
    for _ in range(n_dec):
        m = torch.ones(1, cache.k[0].shape[1] + 1, dtype=torch.bool)
        _, cache = O.llm_forward(cfg, sd, x, attention_mask=m, cache=cache, last_only=True)
    t_dec2 = (time.perf_counter() - t0) / n_dec
    # lm_head alone (identical in the 1- and 2-layer runs): time it to split layer cost from head cost
    h = torch.randn(1, 1, cfg.hidden)
    t0 = time.perf_counter()
    for _ in range(4):
        O._lin(h, sd["lm_head.weight"], None, O.FP32)
    t_head = (time.perf_counter() - t0) / 4
    t_layer_dec = max(1e-9, (t_dec2 - t_head) / 2)
    tok_s = 1.0 / (cfg_full.n_layers * t_layer_dec + t_head)
    ttft = n_tiles * (t_clip + t_qf) + cfg_full.n_layers * (t_pre1 - t_head) + t_head
    measured = None
    try:
        measured = cpu_measured_c1(cfg_full, dev)
    except Exception as ex:      # (host memory: the full fp32 model is 36 GB)
        measured = {"error": f"{type(ex).__name__}: {ex}"}
    return {"value": round(tok_s, 3), "unit": "tokens/s", "cores": threads, "kind": "port",
            "image_to_first_token_ms": round(ttft * 1e3, 1), "measured_c1": measured,
            "sample": f"oracle fp32 on {threads} host threads ({os.cpu_count()} logical cpus): 1 CLIP tile {t_clip:.2f}s, "
                      f"1 Q-Former tile at L={L} {t_qf:.2f}s, 1 decoder layer prefill at S={S} {t_pre1:.2f}s, "
                      f"{n_dec} decode tokens over 2 layers at ctx {S} {t_dec2 * 1e3:.0f} ms/token, lm_head {t_head * 1e3:.0f} ms; "
                      f"scaled to {n_tiles} tiles / {cfg_full.n_layers} layers (weights generated in {t_w:.0f}s, untimed)"}


def cpu_measured_c1(cfg_full, dev):
    """MEASURED, not scaled: BASELINE configs[0] (the reference's own CPU-runnable case: 3 anyres tiles + 32-id prompt -> S = 127, fp32)
    through the oracle with ALL decoder layers on this box's host cores - image->first-token and 8 greedy decode tokens against the KV
    cache.  The configs[2] figure above is extrapolated from per-layer / per-tile samples (a full S = 2048 fp32 pass takes minutes);
    this one calibrates it."""
    from oracle import vz_oracle as O
    from vz_hip import synth
    t0 = time.perf_counter()
    sd = {k: v.cpu() for k, v in synth.iter_state_dict(cfg_full, 0, device=dev)}
    t_w = time.perf_counter() - t0
    tiles = synth.synth_tiles(3, seed=1)
    ids = synth.synth_ids(32, cfg_full.vocab, image_pos=5, seed=2).unsqueeze(0)
    t0 = time.perf_counter()
    emb = O.prepare_inputs_labels_for_multimodal(cfg_full, sd, ids, None, None, None, None, [tiles])[4]
    t_vis = time.perf_counter() - t0
    logits, cache = O.llm_forward(cfg_full, sd, emb, last_only=True)
    tok = logits[0, -1].argmax().view(1)
    t_first = time.perf_counter() - t0
    n_dec = 8
    t1 = time.perf_counter()
    for _ in range(n_dec):
        x = O.embed_tokens(sd, tok, O.FP32).unsqueeze(0)
        m = torch.ones(1, cache.k[0].shape[1] + 1, dtype=torch.bool)
        logits, cache = O.llm_forward(cfg_full, sd, x, attention_mask=m, cache=cache, last_only=True)
        tok = logits[0, -1].argmax().view(1)
    t_dec = (time.perf_counter() - t1) / n_dec
    del sd
    return {"workload": f"configs[0]: 3 tiles + 32 ids -> S = {emb.shape[1]}, {cfg_full.n_layers} layers, fp32, {n_dec} decode tokens",
            "image_to_first_token_ms": round(t_first * 1e3, 1), "vision_and_splice_ms": round(t_vis * 1e3, 1),
            "decode_tokens_per_s": round(1.0 / t_dec, 3), "weights_generated_s": round(t_w, 1)}


def fp8_leg_only(args):
    """child of the default run: the W8A16 engine on the same request; prints its own JSON object."""
    import torch
    from vz_hip import binding as B, synth
    device = "cuda:0"
    torch.cuda.set_device(device)
    n_tiles, n_ids, n_new = 5, 1889, args.new_tokens
    S = (n_ids - 1) + 32 * n_tiles
    model8 = build_model(args.layers, device, max_ctx=S + n_new + 16, weight_fp8=True)
    cfg = model8.arch
    tiles = synth.synth_tiles(n_tiles, seed=1).to(device, torch.bfloat16)
    ids = synth.synth_ids(n_ids, cfg.vocab, image_pos=5, seed=2).unsqueeze(0).to(device)

    def step8():
        tm = {}
        t0 = time.perf_counter()
        out = model8.generate(input_ids=ids, images=[tiles], do_sample=False, max_new_tokens=n_new, eos_token_id=None,
                              pad_token_id=2, use_cache=True, timing=tm)
        torch.cuda.synchronize()
        assert out.shape == (1, n_new)
        return tm["t_first_token"] - t0, time.perf_counter() - tm["t_first_token"]
    step8()
    r8 = [step8() for _ in range(args.steps)]
    e8 = model8.engine
    emb8 = model8.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [tiles])[4]
    _, last8 = e8.prefill(emb8, [S])
    e8.decode_begin(last8.argmax(-1).to(torch.int32), [S], [S])
    e8.prof_enable(True, B.K_GEMV)
    e8.decode_steps(16)
    torch.cuda.synchronize()
    n_l8, ms8 = e8.prof_read()
    e8.prof_enable(False)
    w_bytes8 = algorithmic_work(cfg, S, n_tiles)[0] // 2 + 4 * (cfg.n_layers * ((cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim
                                                                                 + 2 * cfg.hidden + 2 * cfg.inter) + cfg.vocab)
    ach8 = w_bytes8 / (4 * cfg.n_layers + 1) / (ms8 / max(1, n_l8) * 1e-3) / 1e9
    fp8_leg = {"value": round((n_new - 1) * args.steps / sum(b for _, b in r8), 2), "unit": "tokens/s",
               "image_to_first_token_ms": round(sum(a for a, _ in r8) / args.steps * 1e3, 2),
               "dtype": "w8a16: OCP e4m3 weights + per-row 2^e scales (decode stream), bf16 activations, bf16 MFMA prefill on the "
                        "dequantised weights",
               "roofline": {"bound": "hbm", "kernel": "gemv_bf16_kernel<.., FP8> (decode weight stream, 1 B per weight)",
                            "achieved": round(ach8, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach8 / HBM_PEAK_GBS, 4),
                            "traffic": None, "launches": n_l8, "avg_launch_ms": round(ms8 / max(1, n_l8), 5),
                            "algorithmic_bytes_per_launch": int(w_bytes8 / (4 * cfg.n_layers + 1))}}
    # config 5's "fp8 MFMA weights": the same engine with its Zephyr prefill linears on the fp8 MFMA (e4m3 x e4m3, activations quantised
    # per row on the device; gemm_fp8.hip) - first-token latency and the prefill linears' rate (the quantiser launches are counted in the latency)
    e8.set_prefill_fp8(True)
    step8()
    r8m = [step8() for _ in range(args.steps)]
    e8.prof_enable(True, B.K_GEMM)
    e8.prefill(emb8, [S])
    torch.cuda.synchronize()
    n_lm, ms_m = e8.prof_read()
    e8.prof_enable(False)
    pre_flops8 = algorithmic_work(cfg, S, n_tiles)[1]
    fp8_leg["fp8_mfma_prefill"] = {"image_to_first_token_ms": round(sum(a for a, _ in r8m) / args.steps * 1e3, 2),
                                   "decode_tokens_per_s": round((n_new - 1) * args.steps / sum(b for _, b in r8m), 2),
                                   "prefill_linears": {"achieved": round(pre_flops8 / (ms_m * 1e-3) / 1e12, 1), "unit": "TFLOP/s", "launches": n_lm,
                                                       "total_ms": round(ms_m, 3), "peak_fp8_dense": 5000.0,
                                                       "frac_of_fp8_peak": round(pre_flops8 / (ms_m * 1e-3) / 1e12 / 5000.0, 4)},
                                   "what": "Zephyr prefill linears as e4m3 x e4m3 on v_mfma_scale_f32_16x16x128_f8f6f4 (per-row power-of-two scales on both "
                                           "operands); CLIP / Q-Former / lm_head / decode unchanged"}
    e8.set_prefill_fp8(False)
    del model8, e8
    torch.cuda.empty_cache()
    print(json.dumps(fp8_leg), flush=True)


def _dry_model(world):
    """VZ_BENCH_DRY=1 (tests/test_bench_flow_cpu.py): the multi-rank CONTROL FLOW of this script - rendezvous, barriers, the timed
    region, max over ranks, the tensor-parallel child processes on their own port, the JSON line - without a GPU call."""
    class M:
        arch = None

        def generate(self, timing=None, **kw):
            time.sleep(0.01)
            if timing is not None:
                timing["t_first_token"] = time.perf_counter()
            time.sleep(0.02)
            return torch.zeros(1, kw.get("max_new_tokens", 1), dtype=torch.long)
    return M()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--layers", type=int, default=32, help="decoder layers (32 = Zephyr-7B; anything else is a debug run)")
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-fp8-leg", action="store_true", help="skip the extra W8A16 (e4m3 weight stream) measurement")
    ap.add_argument("--fp8-leg-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's generated ids to DIR/generated_ids.npy (float64)")
    ap.add_argument("--full", action="store_true",
                    help="also run the extra legs after the timed region: rooflines, reference parity, streamer and persistent paths, "
                         "the W8A16 engine, the CPU baseline, the tensor-parallel xGMI timings and one-shot probe")
    args = ap.parse_args()
    if args.fp8_leg_only:
        return fp8_leg_only(args)

    rank = int(os.environ.get("RANK", "0"))
    tune = os.environ.get("VZ_TUNE", "")   # experiments only: "knob=value,..." for vz_tune_set; reported in config when set
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dry = os.environ.get("VZ_BENCH_DRY", "0") == "1"
    dist = None
    # rehearsal on a one-GPU box: VZ_BENCH_SINGLE_DEVICE=1 puts every rank on cuda:0 and uses gloo for the control-plane
    # collectives (barrier, max of the timings) - the multi-rank control flow runs, the GPUs are not what is measured
    single_dev = os.environ.get("VZ_BENCH_SINGLE_DEVICE", "0") == "1" or dry
    if single_dev:
        local_rank = 0
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if single_dev:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"))
    device = f"cuda:{local_rank}"
    sync = (lambda: None) if dry else torch.cuda.synchronize
    if not dry:
        torch.cuda.set_device(device)

    n_tiles, n_ids, n_new = 5, 1889, args.new_tokens
    S = (n_ids - 1) + 32 * n_tiles
    # N > 1: this process measures REPLICAS (one request per GPU); VZ_BENCH_PARALLELISM=tp (set for the child processes below) runs
    # ONE request over the tensor-parallel + tile-data-parallel engine instead - the child's numbers become `value`.
    tp_mode = world > 1 and os.environ.get("VZ_BENCH_PARALLELISM", "replicas") == "tp"
    if dry:
        model, eng, cfg, tiles, ids, B = _dry_model(world), None, None, None, None, None
    else:
        from vz_hip import binding as B, synth
        for kv in filter(None, tune.split(",")):
            k, v = kv.split("=")
            B.check(B.lib().vz_tune_set(int(k), int(v)))
        model = build_model(args.layers, device, max_ctx=S + n_new + 16, tp_size=world if tp_mode else 1,
                            tp_rank=rank if tp_mode else 0)
        eng, cfg = model.engine, model.arch
        tiles = synth.synth_tiles(n_tiles, seed=1).to(device, torch.bfloat16)
        ids = synth.synth_ids(n_ids, cfg.vocab, image_pos=5, seed=2).unsqueeze(0).to(device)

    def barrier():
        sync()
        if dist is not None:
            dist.barrier()
        sync()

    last_out = [None]      # what the latest step returned to its caller (--dump-outputs)

    def step():
        tm = {}
        t0 = time.perf_counter()
        out = model.generate(input_ids=ids, images=None if dry else [tiles], do_sample=False, max_new_tokens=n_new, eos_token_id=None,
                             pad_token_id=2, use_cache=True, timing=tm)
        sync()
        t2 = time.perf_counter()
        assert out.shape == (1, n_new)
        last_out[0] = out
        return tm["t_first_token"] - t0, t2 - tm["t_first_token"]

    for _ in range(args.warmup):
        step()
    barrier()
    t_start = time.perf_counter()
    ttfts, decs = [], []
    for _ in range(args.steps):
        a, b = step()
        ttfts.append(a)
        decs.append(b)
    barrier()
    elapsed = time.perf_counter() - t_start
    stats = torch.tensor([elapsed, sum(ttfts), sum(decs)], dtype=torch.float64, device="cpu" if single_dev else device)
    if dist is not None:
        dist.all_reduce(stats, op=dist.ReduceOp.MAX)
    elapsed, ttft_sum, dec_sum = stats.tolist()
    if args.dump_outputs and rank == 0:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "generated_ids.npy"), last_out[0].cpu().numpy().astype(np.float64))

    # ---- --full, tensor-parallel mode: per-collective time from HIP events (every rank runs the instrumented replay: the collectives
    # need all of them), so that a multi-GPU run yields xGMI numbers ----
    xgmi = None
    if tp_mode and not dry and args.full:
        emb = model.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [tiles])[4]
        eng.prof_enable(True, B.K_COMM)
        _, last = eng.prefill(emb, [S])
        torch.cuda.synchronize()
        n_p, ms_p = eng.prof_read()
        eng.decode_begin(last.argmax(-1).to(torch.int32), [S], [S])
        eng.prof_enable(True, B.K_COMM)
        eng.decode_steps(8)
        torch.cuda.synchronize()
        n_d, ms_d = eng.prof_read()
        eng.prof_enable(False)
        pre_bytes = S * cfg.hidden * 2
        xgmi = {"prefill_allreduce": {"launches": n_p, "avg_us": round(ms_p / max(1, n_p) * 1e3, 2), "bytes": pre_bytes,
                                      "algbw_GBps": round(pre_bytes / max(1e-9, ms_p / max(1, n_p) * 1e-3) / 1e9, 1)},
                "decode_collectives": {"launches": n_d, "avg_us": round(ms_d / max(1, n_d) * 1e3, 2), "bytes": cfg.hidden * 2,
                                       "per_token_ms": round(ms_d / 8, 4)},
                "decode_allreduce_kernel": "one-shot (csrc/comm_oneshot.hip, VZ_TP_ONESHOT=1)" if getattr(eng, "oneshot", False) else "RCCL ncclAllReduce",
                "method": "HIP events around every collective of one prefill and 8 eager decode steps after the timed region (rank 0)"}
        # ---- probe (never `value`): the same decode steps with the decode all-reduces on the hand-written one-shot kernel (csrc/comm_oneshot.hip,
        # peer areas mapped through hipIpc) - no multi-GPU box was available to the build, so a run on real xGMI is the first measurement of it.
        # Bounded: ONE eager step first (an absent peer costs a bounded sweep per all-reduce and raises the async word), every rank agrees on
        # the outcome through a MAX all-reduce before anything longer runs; a failure switches the engine back to RCCL and is reported. ----
        if rank == 0:
            # the leg's numbers go out BEFORE the probe: if the probe ever stalls the child into its time limit, the parent still has them
            print(json.dumps({"early": True, "value": round((n_new - 1) * args.steps / dec_sum, 2), "unit": "tokens/s",
                              "image_to_first_token_ms": round(ttft_sum / args.steps * 1e3, 2), "ms_per_step": round(elapsed / args.steps * 1e3, 2),
                              "scaling": "strong", "xgmi": xgmi,
                              "config": {"parallelism": f"tp{world} + tile-dp{world}: one request, Zephyr tensor-parallel + tiles dealt over the group, RCCL over xGMI"}}),
                  flush=True)
        if os.environ.get("VZ_BENCH_ONESHOT_PROBE", "1") != "0" and not getattr(eng, "oneshot", False):
            probe = {"ok": False}
            try:
                import ctypes as C
                mapped = eng.init_oneshot()
                if not mapped:
                    probe["why"] = "a rank could not export / map a receive area (hipIpcGetMemHandle / hipIpcOpenMemHandle)"
                else:
                    def _err():
                        e_ = C.c_int(0)
                        B.check(eng.lib.vz_engine_async_error(eng.h, C.byref(e_)))
                        return int(e_.value)
                    _, last = eng.prefill(emb, [S])
                    eng.decode_begin(last.argmax(-1).to(torch.int32), [S], [S])
                    eng.prof_enable(True, B.K_COMM)
                    _, lg1 = eng.decode_steps(1, return_logits=True)
                    torch.cuda.synchronize()
                    n_1, ms_1 = eng.prof_read()
                    eng.prof_enable(False)
                    bad = torch.tensor([1.0 if (_err() or not bool(torch.isfinite(lg1).all())) else 0.0], device=device)
                    dist.all_reduce(bad, op=dist.ReduceOp.MAX)
                    if float(bad.item()) > 0:
                        B.check(B.lib().vz_tune_set(29, 0))          # RCCL again for whatever follows
                        probe["why"] = "the first one-shot step raised the async error word or produced non-finite logits on some rank"
                    else:
                        t0 = time.perf_counter()
                        tm = {}
                        out1 = model.generate(input_ids=ids, images=[tiles], do_sample=False, max_new_tokens=n_new, eos_token_id=None, pad_token_id=2,
                                              use_cache=True, timing=tm)
                        sync()
                        t_dec = time.perf_counter() - tm["t_first_token"]
                        B.check(B.lib().vz_tune_set(29, 0))
                        out0 = model.generate(input_ids=ids, images=[tiles], do_sample=False, max_new_tokens=n_new, eos_token_id=None, pad_token_id=2,
                                              use_cache=True)
                        sync()
                        probe = {"ok": True, "decode_tokens_per_s": round((n_new - 1) / t_dec, 2),
                                 "first_step_collectives": {"launches": n_1, "avg_us": round(ms_1 / max(1, n_1) * 1e3, 2)},
                                 "ids_equal_to_rccl": bool(torch.equal(out0, out1)), "async_error_after": _err(),
                                 "what": "128 greedy tokens of the same request with the 64 decode all-reduces per token on comm_oneshot.hip (8-byte {2 x bf16, tag} granules "
                                         "stored into every peer's area, rank-order fp32 sum) inside the per-token hipGraph"}
            except Exception as ex:      # the probe must never cost the leg its numbers
                probe = {"ok": False, "why": f"{type(ex).__name__}: {ex}"[:300]}
                try:
                    B.check(B.lib().vz_tune_set(29, 0))
                except Exception:
                    pass
            xgmi["oneshot_probe"] = probe

    # ---- --full, roofline legs: instrumented replays of the same work, HIP events on the launch stream ----
    roof, roof_prefill, parity, stream_leg, persist_leg = None, None, None, None, None
    if args.full and rank == 0 and not tp_mode and not dry:          # (a tensor-parallel engine needs every rank inside each collective)
        w_bytes, pre_flops = algorithmic_work(cfg, S, n_tiles)
        emb = model.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [tiles])[4]
        _, last = eng.prefill(emb, [S])
        eng.decode_begin(last.argmax(-1).to(torch.int32), [S], [S])
        eng.prof_enable(True, B.K_GEMV)
        n_prof = 16
        eng.decode_steps(n_prof)
        torch.cuda.synchronize()
        n_l, ms = eng.prof_read()
        eng.prof_enable(False)
        persist = eng.persist_mode()
        avg_ms = ms / max(1, n_l)
        # the dominant kernel of a decoded token: ONE launch of the persistent decode-token kernel (decode_persist.hip: all 129 weight
        # streams + the 32 attention phases of the token; its algorithmic bytes = every weight once + the KV cache once), or - launch
        # chain, vz_tune_set(28, 0) / other devices - the 129 weight-streaming GEMV launches (weights only)
        kv_bytes = 2 * cfg.n_layers * cfg.n_kv_heads * cfg.head_dim * 2 * (S + n_prof // 2)
        launches_per_token = n_l / n_prof
        # (default route since round 3: the O projection's weights are streamed by the attention + O launch, attn_o_fused.hip - its bytes
        # are not the GEMV launches' then: 3 GEMVs per layer + the lm_head)
        o_fused = abs(launches_per_token - (3 * cfg.n_layers + 1)) < 0.5
        gemv_bytes = w_bytes - (2 * cfg.n_layers * cfg.hidden * cfg.n_heads * cfg.head_dim if o_fused else 0)
        bytes_per_launch = (w_bytes + kv_bytes) if persist else gemv_bytes / launches_per_token
        ach = bytes_per_launch / (avg_ms * 1e-3) / 1e9
        roof = {"bound": "hbm", "kernel": "decode_token_kernel (one resident grid per token: 129 weight streams + 32 attention phases)" if persist
                else "gemv_bf16_kernel<1> (decode weight stream" + ("; the O projection rides in the attention launch" if o_fused else "") + ")", "achieved": round(ach, 1),
                "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": pmc_traffic(persist),
                "launches": n_l, "launches_per_token": round(launches_per_token, 2), "avg_launch_ms": round(avg_ms, 5),
                "algorithmic_bytes_per_launch": int(bytes_per_launch),
                "method": f"HIP events stamped by every such launch of {n_prof} eager decode steps after the timed region"}
        eng.prof_enable(True, B.K_GEMM)
        eng.prefill(emb, [S])
        torch.cuda.synchronize()
        n_l, ms = eng.prof_read()
        eng.prof_enable(False)
        tf = pre_flops / (ms * 1e-3) / 1e12
        roof_prefill = {"bound": "mfma", "kernel": "gemm_bf16_kernel (Zephyr prefill QKV/O/gate-up/down)", "achieved": round(tf, 1),
                        "peak": MFMA_BF16_PEAK_TF, "unit": "TFLOP/s", "frac": round(tf / MFMA_BF16_PEAK_TF, 4),
                        "traffic": None, "launches": n_l, "total_ms": round(ms, 3),
                        "algorithmic_flops": pre_flops}
        # the whole image->first-token phase against the MFMA peak: the work the engine EXECUTES for this request - CLIP 381.9
        # GFLOP/tile, Q-Former 1186.7 GFLOP/tile at L = 1888 minus the block-0 rows the reference computes and discards (the
        # engine runs block 0's self-attention once per sample on the 32 query rows: -705 GFLOP/tile),
        # Zephyr prefill 30.224 TFLOP at S = 2048 minus the all-position lm_head generate() does not run (0.537 TFLOP) - over
        # the measured latency (attention, norms, splice included).  `survey_flops` = SURVEY section 8(d)'s figure for the same request.
        if cfg.n_layers == 32 and S == 2048 and n_tiles == 5:
            survey_flops = n_tiles * (381.9e9 + 1186.7e9) + 30.224e12 - 0.537e12
            ft_flops = survey_flops - n_tiles * 705e9
            ft_tf = ft_flops / (ttft_sum / args.steps) / 1e12
            roof_prefill["image_to_first_token"] = {"achieved": round(ft_tf, 1), "unit": "TFLOP/s", "frac": round(ft_tf / MFMA_BF16_PEAK_TF, 4),
                                                    "executed_flops": ft_flops, "survey_flops": survey_flops}
        parity = parity_check(model, ids, tiles, cfg.n_layers)
        if world == 1:
            stream_leg = streamer_leg(model, ids, tiles, n_new, args.steps)
            persist_leg = persistent_leg(model, ids, tiles, n_new)

    # ---- --full, extra leg (never `value`): the same request on the W8A16 engine of SURVEY config 5 - e4m3 weights with per-row
    # power-of-two scales streamed by the decode GEMV, bf16 activations, bf16 MFMA prefill on the dequantised weights.
    # Runs in a CHILD process with a time limit (as the tensor-parallel leg does): whatever happens there - an exception, a
    # stall while the second engine is built - the bf16 line of this process is printed. ----
    fp8_leg = None
    if args.full and world == 1 and not args.no_fp8_leg and not dry:
        import subprocess
        cmd = [sys.executable, os.path.abspath(__file__), "--fp8-leg-only", "--steps", str(args.steps), "--layers", str(args.layers),
               "--new-tokens", str(args.new_tokens)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode == 0 and lines:
                fp8_leg = json.loads(lines[-1])
            else:
                fp8_leg = {"value": None, "error": f"child rc={r.returncode}: {(r.stderr or '')[-300:]}"}
        except subprocess.TimeoutExpired:
            fp8_leg = {"value": None, "error": "W8A16 child timed out after 240 s"}

    # ---- N > 1: the north-star partition - ONE request over the tensor-parallel + tile-data-parallel engine - measured by CHILD
    # processes (one per rank, this script in tp mode on its own rendezvous port, the same K steps / W warmup, the same barrier +
    # max-over-ranks timing), so a failure or hang inside the collectives cannot withhold the line; rank 0 takes the child's
    # numbers as `value` (or falls back to the replica numbers and says why). ----
    tp_leg = None
    if world > 1 and not tp_mode and os.environ.get("VZ_BENCH_TP_LEG", "1") != "0":
        import subprocess
        barrier()
        env = dict(os.environ)
        env["VZ_BENCH_PARALLELISM"] = "tp"
        env["VZ_BENCH_TP_LEG"] = "0"
        env["MASTER_PORT"] = str(int(os.environ.get("MASTER_PORT", "29500")) + 23)
        # under torch.distributed.run the workers are CLIENTS of the agent's store (TORCHELASTIC_USE_AGENT_STORE=True); the child
        # group lives on its own port, so its rank 0 must host the store itself - otherwise every child waits for a server forever
        for k in [k for k in env if k.startswith("TORCHELASTIC_")]:
            env.pop(k)
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", str(world), "--steps", str(args.steps), "--warmup", str(max(1, args.warmup)),
               "--layers", str(args.layers), "--new-tokens", str(args.new_tokens), "--no-cpu-baseline", "--no-fp8-leg"]
        if args.full:
            cmd.append("--full")
        limit = int(os.environ.get("VZ_BENCH_TP_TIMEOUT", "300"))
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit)
            if rank == 0:
                lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
                if r.returncode == 0 and lines:
                    tp_leg = json.loads(lines[-1])
                else:
                    tp_leg = {"value": None, "error": f"child rc={r.returncode}: {(r.stderr or '')[-400:]}"}
        except subprocess.TimeoutExpired as ex:
            if rank == 0:
                out = ex.stdout.decode() if isinstance(ex.stdout, (bytes, bytearray)) else (ex.stdout or "")
                lines = [l for l in out.splitlines() if l.startswith("{")]
                if lines:      # the child's early line (its timed region had finished; it stalled afterwards, e.g. inside the one-shot probe)
                    tp_leg = json.loads(lines[-1])
                    tp_leg["note"] = f"child hit its {limit} s limit after printing this line"
                else:
                    tp_leg = {"value": None, "error": f"tensor-parallel child timed out after {limit} s"}
        barrier()
    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return
    cpu = None
    if args.full and not args.no_cpu_baseline and world == 1 and not dry:
        try:
            cpu = cpu_baseline(cfg, S, n_tiles, n_new)
        except Exception as ex:   # the GPU numbers stand on their own; say why the CPU leg is missing
            cpu = {"value": None, "unit": "tokens/s", "cores": torch.get_num_threads(), "kind": "port",
                   "sample": f"failed: {type(ex).__name__}: {ex}"}
    n_dec_tokens = (n_new - 1) * args.steps * (1 if tp_mode else world)
    workload = (f"configs[2]: 5 anyres tiles (4 crops + 1 global) + {n_ids}-id prompt -> S={S}, {n_new} greedy new tokens, "
                f"{args.layers} decoder layers")
    line = {
        "metric": "decode tokens/sec (image->first-token ms alongside), Zephyr-7B anyres 5-tile",
        "value": round(n_dec_tokens / dec_sum, 2),
        "unit": "tokens/s",
        "image_to_first_token_ms": round(ttft_sum / args.steps * 1e3, 2),
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 2),
        "higher_is_better": True, "scaling": "strong" if tp_mode else "weak", "vs_baseline": None,
        "dtype": "bf16", "data": "dry-run (control flow only)" if dry else "synthetic (hash-generated weights seed 0, N(0,1) tiles, uniform ids)",
        "config": {"workload": workload,
                   "parallelism": "single GPU" if world == 1 else
                                  (f"tp{world} + tile-dp{world}: one request, Zephyr tensor-parallel + tiles dealt over the group, RCCL over xGMI" if tp_mode
                                   else f"dp{world} replicas (one request per GPU, no collective)")},
        "roofline": roof, "roofline_prefill": roof_prefill, "cpu_baseline": cpu,
    }
    if tune:
        line["config"]["tune"] = tune
    if xgmi is not None:
        line["xgmi"] = xgmi
    if parity is not None:
        line["parity"] = parity
    if stream_leg is not None:
        line["streamer_path"] = stream_leg
    if persist_leg is not None:
        line["persistent_kernel"] = persist_leg
    if fp8_leg is not None:
        line["fp8_weights"] = fp8_leg
    if tp_leg is not None:
        if tp_leg.get("value") is not None:
            # the north-star partition is the headline; what this process measured (replicas) rides beside it
            replicas = {k: line[k] for k in ("value", "unit", "image_to_first_token_ms", "ms_per_step", "scaling")}
            replicas["parallelism"] = line["config"]["parallelism"]
            for k in ("value", "image_to_first_token_ms", "ms_per_step", "scaling"):
                line[k] = tp_leg[k]
            line["config"]["parallelism"] = tp_leg["config"]["parallelism"]
            if "xgmi" in tp_leg:
                line["xgmi"] = tp_leg["xgmi"]
            line["replicas"] = replicas
        else:
            line["tensor_parallel"] = tp_leg
            line["config"]["parallelism"] += " - the tensor-parallel engine did not produce a number (see tensor_parallel.error)"
    print(json.dumps(line), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
