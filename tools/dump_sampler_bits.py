#!/usr/bin/env python
"""Record what the sampler and logits-processor entry points (csrc/engine.hip, behind vz_hip.binding and vz_hip.engine.Engine) compute
on a fixed list of seeded cases.

    python tools/dump_sampler_bits.py [out.npz]     default: tests/golden/sampler_parent_bits.npz   (needs the GPU)

Run it on the commit whose results are the reference: tests/test_sampler_bits_gpu.py replays the same cases (this module is its case
list) and asserts equality.  It goes through the Python helpers only (binding.sample, sample_rows, token_scores, logits_process;
Engine.set_sampling, set_sampling_rows, decode_set_row_sampling, set_logits_proc, set_scores), whose signatures the C ABI's change of
form left alone - so the same file runs on both sides of that change.

Operator cases, each at V = 1000 (the kernels' staged form) and V = 40000 (> 32768: their loop form):
  sample          2 rows by one parameter set: counter 0, counter 77, counter 77 with the four further warpers
  sample_rows     3 rows: greedy, sampled with top-k and top-p, sampled with all four warpers
  token_scores    the same rows about the tokens sample_rows chose, with the warped score rows
  logits_process  2 rows over a history of 5 ids (row 1: 2 of them): penalty 1.2, n-gram 2, min_new 3 with one eos, two suppressed
                  ids, one bias sequence and one bad-word sequence
Engine cases, on one 2-layer synthetic engine (max_batch 4, max_ctx 64), in this order:
  engine_sampler  set_sampling with warpers + set_logits_proc + set_scores(warped): 8 steps as two calls of 4; then the same
                  parameters under another seed (4 steps: the captured step is replayed) and another temperature (4 steps: captured again)
  engine_rows     set_sampling_rows on the 3 rows above + set_scores(warped): 8 steps with one decode_set_row_sampling after step 4
  engine_greedy   the argmax tail with the draw counter set through set_sampling(False) + set_scores: 4 steps
Per case the file holds every result as bit patterns where it is small (ids, records, graph captures counted from the case's start) and
as a SHA-256 where it is not (score rows).  Everything runs twice (the engine cases on an engine of their own each time) and must
reproduce bit for bit before it is written; what does not is named in `nondet` and left out."""
import hashlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "vision-zephyr_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DEFAULT_OUT = os.path.join(REPO, "tests", "golden", "sampler_parent_bits.npz")
VOCABS = (1000, 40000)
WARP = dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3)
OP_CASES = [f"{op}_v{V}" for V in VOCABS for op in ("sample", "sample_rows", "token_scores", "logits_process")]
ENGINE_CASES = ["engine_sampler", "engine_rows", "engine_greedy"]
CASES = OP_CASES + ENGINE_CASES
SMALL = 4096          # results of up to this many values are stored as they are, larger ones as a digest


def row_mix(seed):
    """greedy | sampled with top-k and top-p | sampled with all four warpers"""
    from vz_hip.sample_rows import GREEDY, RowParams
    return [GREEDY.at(2), RowParams(True, 0.7, 50, 0.9, 0x1234_5678_0000_0000 + seed, 1),
            RowParams(True, 0.9, 40, 0.95, 0x0BAD_5EED_0000_0000 + 7919 * seed, 77, **WARP)]


def proc_config():
    from vz_hip.logits_proc import ProcConfig
    return ProcConfig(penalty=1.2, ngram=2, min_new=3, eos=(2,), suppress=(5, 6), seq=(((11,), 2.5, False), ((4, 9), 0.0, True)))


def logits(rows, V, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, V, generator=g) * 2.5).float().cuda()


def run_op_case(name):
    """dict of the case's result tensors"""
    from vz_hip import binding as B
    from vz_hip.sample_rows import RowParams
    op, V = name.rsplit("_v", 1)
    V = int(V)
    if op == "sample":
        x = logits(2, V, 100 + V)
        warp = RowParams(True, **WARP).warp
        return {"ids_c0": B.sample(x, 0.7, 50, 0.9, 0xFEED_0000_0001, 0), "ids_c77": B.sample(x, 0.7, 50, 0.9, 0xFEED_0000_0001, 77),
                "ids_c77_warp": B.sample(x, 0.9, 40, 0.95, 0xFEED_0000_0002, 77, warp=warp)}
    if op in ("sample_rows", "token_scores"):
        x, params = logits(3, V, 200 + V), row_mix(V)
        ids = B.sample_rows(x, params)
        if op == "sample_rows":
            return {"ids": ids}
        rec, warped = B.token_scores(x, ids, params, warped=True)
        return {"rec": rec, "warped": warped}
    assert op == "logits_process"
    x = logits(2, V, 300 + V)
    hist = torch.tensor([[4, 9, 4, 7, 4], [11, 4, 0, 0, 0]], dtype=torch.int32).cuda()
    hist_len = torch.tensor([5, 2], dtype=torch.int32).cuda()
    return {"logits": B.logits_process(x, proc_config(), hist, hist_len)}


def make_engine():
    from vz_hip import synth
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    cfg = synth.ArchConfig(n_layers=2)
    hf = VisZephyrConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=2, num_attention_heads=32,
                         num_key_value_heads=8, vocab_size=cfg.vocab, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    return VisZephyrForCausalLM.from_synthetic(hf, seed=0, max_batch=4, max_ctx=64, max_tiles=1, max_text=32)


def _prefill(model, lens, seed):
    """ragged prompts of `lens` ids into cache rows 0..: the first token of every row (argmax of the prefill logits)"""
    from vz_hip import binding as B
    from vz_hip import synth
    eng = model.engine
    ids = torch.full((len(lens), max(lens)), 2, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = synth.synth_ids(n, eng.cfg.vocab, image_pos=-1, seed=seed + b)
    _, last = eng.prefill(eng.embed_tokens(ids.to(model.device)), lens)
    return B.argmax(last)


def _steps(eng, out, tag, n, cap0):
    """n decode steps and what the recorder holds of them (the ids go to one buffer per case: it is part of what a captured step freezes)"""
    if "buf" not in out:
        out["buf"] = torch.empty(eng._dec_B, n, dtype=torch.int32, device=eng.device)
    out["ids_" + tag] = eng.decode_steps(n, out=out["buf"]).clone()
    rec, warped, _ = eng.scores_steps(n)
    out["rec_" + tag] = rec.clone()
    if warped is not None:
        out["warped_" + tag] = warped.clone()
    out["captures"].append(eng.decode_info()[1] - cap0)


def run_engine_cases():
    """the engine cases in their order on a fresh engine: {case: dict of result tensors}"""
    model = make_engine()
    eng = model.engine
    res = {}
    warp = row_mix(0)[2].warp

    lens = [9, 17]
    first = _prefill(model, lens, 80)
    out = res["engine_sampler"] = {"captures": []}
    cap0 = eng.decode_info()[1]
    try:
        eng.set_scores(8, rows=2, warped=True)          # (once: its rings are part of what a captured step freezes)
        for tag, temperature, seed in (("a", 0.8, 4242), ("seed", 0.8, 31337), ("temp", 1.1, 31337)):
            eng.set_sampling(True, temperature, 40, 0.92, seed, first_counter=1, warp=warp)
            eng.set_logits_proc(proc_config())          # (again: arming empties the histories; the equal table uploads nothing)
            eng.decode_begin(first, lens, lens)
            _steps(eng, out, tag, 4, cap0)
            if tag == "a":
                _steps(eng, out, "a2", 4, cap0)
    finally:
        eng.set_sampling(False)
        eng.set_logits_proc(None)
        eng.set_scores(None)

    lens = [9, 30, 17]
    first = _prefill(model, lens, 90)
    params = row_mix(1)
    out = res["engine_rows"] = {"captures": []}
    cap0 = eng.decode_info()[1]
    try:
        eng.set_sampling_rows(params)
        eng.set_scores(8, rows=3, warped=True)
        eng.decode_begin(first, lens, lens)
        _steps(eng, out, "a", 4, cap0)
        eng.decode_set_row_sampling(0, params[2].at(5))          # the greedy row takes the warpers' entry; no new graph
        _steps(eng, out, "b", 4, cap0)
    finally:
        eng.set_sampling_rows(None)
        eng.set_scores(None)

    out = res["engine_greedy"] = {"captures": []}
    cap0 = eng.decode_info()[1]
    try:
        eng.set_sampling(False, first_counter=3)
        eng.set_scores(4, rows=3)
        eng.decode_begin(first, lens, lens)
        _steps(eng, out, "a", 4, cap0)
    finally:
        eng.set_scores(None)
    torch.cuda.synchronize()
    eng.check_async()
    for out in res.values():
        del out["buf"]
        out["captures"] = torch.tensor(out["captures"], dtype=torch.int32)
    del model, eng
    torch.cuda.empty_cache()
    return res


def digests(out):
    """what is stored of a case's result tensors: {key: bit patterns (int32) or SHA-256}"""
    d = {}
    for k, t in out.items():
        bits = t.detach().contiguous().cpu().view(torch.int32).numpy()
        if bits.size <= SMALL:
            d["bits." + k] = bits
        else:
            d["sha." + k] = hashlib.sha256(bits.tobytes()).hexdigest()
    return d


def run_all():
    """{case: digests} of every case of CASES"""
    got = {name: digests(run_op_case(name)) for name in OP_CASES}
    got.update({name: digests(out) for name, out in run_engine_cases().items()})
    torch.cuda.synchronize()
    return got


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    first, second = run_all(), run_all()
    store, nondet = {}, []
    for name in CASES:
        if not same(first[name], second[name]):
            nondet.append(name)
            print(f"{name:24s} DOES NOT REPRODUCE: {[k for k in first[name] if not np.array_equal(first[name][k], second[name].get(k))]}", flush=True)
            continue
        for k, v in first[name].items():
            store[f"{name}.{k}"] = np.array(v)
        print(f"{name:24s} {sorted(first[name])}", flush=True)
    for name in ENGINE_CASES:
        print(f"{name:24s} captures {first[name]['bits.captures'].tolist()}", flush=True)
    store["nondet"] = np.array(nondet, dtype=str)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **store)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
