#!/usr/bin/env python
"""Record what the rows-per-sample decoder stack (csrc/engine.hip: vz_llm_prefill_rows and vz_llm_prefill_append) computes and
launches on a fixed list of seeded cases.

    python tools/dump_prefill_bits.py [out.npz]     default: tests/golden/prefill_parent_bits.npz   (needs the GPU)

Run it on the commit whose arithmetic is the reference: tests/test_prefill_bits_gpu.py replays the same cases (this module is
its case list) and asserts equality.  The cases walk the orchestration, not the workload's sizes: plain and ragged prefill,
prefill into a second cache row, the rotated-copy path (knob 33 off), the fp8 MFMA route and an append on the same engine, and the
three attention forms of the append (key-split, key-split with padded rows, flash per run of rows with equal past).

Per case the file holds
  sha.*        SHA-256 of logits_all (rows t < new[b] only: the rest comes from padding), logits_last, the K and V of every layer at
               the slots the call wrote, and the K and V of the slots it had to keep
  bits.*       logits_last[:, :256] and the last layer's K row of the last written slot as bit patterns (sizes a mismatch)
  sha.inputs   the embeds and one weight matrix (a differing input is reported as such)
  peak         the arena mark of vz_engine_ws_info after the call
  launches     launches of the call in the classes K_GEMM, K_NORM, K_ATTN, K_OTHER (a run of the case per class)
Every case runs twice and must reproduce bit for bit before anything is written; one that does not is named in `nondet` and
stored without digests."""
import hashlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "vision-zephyr_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DEFAULT_OUT = os.path.join(REPO, "tests", "golden", "prefill_parent_bits.npz")
CLASSES = ("K_GEMM", "K_NORM", "K_ATTN", "K_OTHER")
SHA_KEYS = ("logits_all", "logits_last", "kv_written", "kv_kept", "inputs")
BIT_KEYS = ("logits_last256", "k_last_slot")

# engines: "main" = the 2-layer full-width synthetic model of tests/test_append_gpu.py, "fp8" = the weight_fp8 engine of
# tests/test_stages_gpu.py::test_fp8_mfma_prefill_matches_quantized_oracle
ENGINES = {
    "main": dict(max_batch=2, max_ctx=512, max_tiles=1, max_text=64),
    "fp8": dict(max_batch=1, max_ctx=256, max_tiles=1, max_text=64, weight_fp8=True),
}

# past: positions each cache row holds before the call (a plain prefill of them is the case's setup), T: rows per sample, new: valid
# rows per sample (default T).  call: "prefill" | "rows" (prefill_rows into row0 = 1 after `first` filled row 0) | "append".
# knobs: {knob name: value} around the whole case.  fp8: set_prefill_fp8(True) and knob 22 (fp8_prefill_min_rows) at 0 around the whole case.
CASES = {
    "plain": dict(call="prefill", T=40),
    "plain_ragged": dict(call="prefill", T=96, new=[96, 37], pos_shift=[0, 3]),
    "rows_into_row1": dict(call="rows", T=24, first=40),
    "plain_ragged_rotated_copy": dict(call="prefill", T=96, new=[96, 37], pos_shift=[0, 3], knobs=dict(rope_in_attn=0)),
    "fp8_prefill": dict(call="prefill", engine="fp8", T=150, fp8=True),
    "fp8_engine_append": dict(call="append", engine="fp8", past=[37], T=20, fp8=True),
    "append_keysplit": dict(call="append", past=[37], T=20),
    "append_keysplit_ragged_padded": dict(call="append", past=[37, 20], T=20, new=[20, 9]),
    "append_flash_one_run": dict(call="append", past=[37, 37], T=260),
    "append_flash_two_runs": dict(call="append", past=[37, 20], T=260),
    "append_flash_small_t": dict(call="append", past=[37], T=20, knobs=dict(append_flash_min_t=8)),
}


def make_env(which):
    from vz_hip import synth
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    cfg = synth.ArchConfig(n_layers=2)
    hf = VisZephyrConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=cfg.n_layers,
                         num_attention_heads=cfg.n_heads, num_key_value_heads=cfg.n_kv_heads, vocab_size=cfg.vocab,
                         rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta, sliding_window=cfg.sliding_window,
                         eos_token_id=2, pad_token_id=2, bos_token_id=1)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    hf.mm_hidden_size = 5120
    model = VisZephyrForCausalLM.from_synthetic(hf, seed=0, **ENGINES[which])
    return dict(cfg=cfg, synth=synth, model=model, eng=model.engine)


class Envs:
    """the engines of ENGINES, each built at its first use"""

    def __init__(self):
        self.made = {}

    def get(self, which):
        if which not in self.made:
            self.made[which] = make_env(which)
        return self.made[which]

    def close(self):
        self.made.clear()
        torch.cuda.empty_cache()


def case_seed(name):
    return 3000 + 10 * sorted(CASES).index(name)


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.contiguous()
        h.update(t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy().tobytes())
    return h.hexdigest()


def _embeds(env, n, seed):
    return env["eng"].embed_tokens(env["synth"].synth_ids(n, env["cfg"].vocab, image_pos=-1, seed=seed))


def _the_call(env, name):
    """the case's setup on the engine; returns (call, embeds, row0, past, new, kept) - `call()` is the call under test, `kept` the
    (row, slots) ranges whose cache bits the call has to leave as the setup wrote them"""
    c, eng, seed = CASES[name], env["eng"], case_seed(name)
    T, kind = c["T"], c["call"]
    Bn = len(c.get("new") or c.get("past") or [0])
    past = list(c.get("past", [0] * Bn))
    new = list(c.get("new", [T] * Bn))
    H = env["cfg"].hidden
    rows = [_embeds(env, past[b] + T, seed + b) for b in range(Bn)]
    emb = torch.stack([rows[b][past[b]:] for b in range(Bn)])
    row0, kept = 0, [(b, past[b]) for b in range(Bn) if past[b]]
    if kind == "append":
        head = torch.zeros(Bn, max(past), H, dtype=torch.bfloat16, device=emb.device)
        for b in range(Bn):
            head[b, :past[b]] = rows[b][:past[b]]
        eng.prefill(head, past, all_logits=False, last_logits=True)
        return (lambda: eng.prefill_append(0, emb, new, past, all_logits=True, last_logits=True)), [emb, head], row0, past, new, kept
    pos = None
    if "pos_shift" in c:          # explicit positions that are not the row indices
        pos = torch.arange(T, dtype=torch.int32).unsqueeze(0) + torch.tensor(c["pos_shift"], dtype=torch.int32).unsqueeze(1)
    if kind == "rows":
        first = _embeds(env, c["first"], seed + 7).unsqueeze(0)
        eng.prefill(first, [c["first"]], all_logits=False, last_logits=True)
        return (lambda: (None, eng.prefill_rows(1, emb, new, pos))), [emb, first], 1, past, new, [(0, c["first"])]
    return (lambda: eng.prefill(emb, new, pos, all_logits=True, last_logits=True)), [emb], row0, past, new, kept


def _armed(env, name, body):
    from vz_hip import binding as B
    c, eng = CASES[name], env["eng"]
    knobs = dict(c.get("knobs", {}), **(dict(fp8_prefill_min_rows=0) if c.get("fp8") else {}))
    try:
        if c.get("fp8"):
            eng.set_prefill_fp8(True)
        with B.tuned(**knobs):
            return body()
    finally:
        if c.get("fp8"):
            eng.set_prefill_fp8(False)


def run_case(envs, name):
    """the case once: dict of its output tensors, `inputs` (digest), `peak` and `untouched` (the call changed no cache bit outside the
    slots it writes)"""
    env = envs.get(CASES[name].get("engine", "main"))
    eng = env["eng"]

    def body():
        call, inputs, row0, past, new, kept = _the_call(env, name)
        before = eng.kv_cache()
        la, ll = call()
        torch.cuda.synchronize()
        eng.check_async()
        peak = eng.ws_info()[1]
        kv = eng.kv_cache()                    # [layer, K|V, cache row, kv head, slot, D]
        written = [kv[:, :, row0 + b, :, past[b]:past[b] + new[b]] for b in range(len(new))]
        out = dict(logits_last=ll, kv_written=torch.cat([w.reshape(-1) for w in written]),
                   kv_kept=torch.cat([kv[:, :, r, :, :n].reshape(-1) for r, n in kept]) if kept else kv.new_zeros(0),
                   logits_all=torch.cat([la[b, :new[b]].reshape(-1) for b in range(len(new))]) if la is not None else ll.new_zeros(0),
                   logits_last256=ll[:, :256].contiguous(), k_last_slot=written[-1][-1, 0, :, -1].contiguous(),
                   inputs=sha(*inputs, eng.w["llm.1.qkv.w"]), peak=peak)
        for b in range(len(new)):              # everything but the written slots is as it was
            before[:, :, row0 + b, :, past[b]:past[b] + new[b]] = written[b]
        out["untouched"] = torch.equal(before, kv)
        return out

    return _armed(env, name, body)


def count_launches(envs, name):
    """launches of the call under test per class of CLASSES (a run of the case per class: the profiler counts one class at a time)"""
    from vz_hip import binding as B
    env = envs.get(CASES[name].get("engine", "main"))
    eng = env["eng"]

    def body():
        counts = []
        for klass in CLASSES:
            call = _the_call(env, name)[0]
            eng.prof_enable(True, getattr(B, klass))
            try:
                call()
                counts.append(eng.prof_read()[0])
            finally:
                eng.prof_enable(False)
        return counts

    return _armed(env, name, body)


def digests(out):
    """what is stored of run_case's result: the digests, the two bit-pattern samples, the arena mark"""
    d = {"sha." + k: (out[k] if k == "inputs" else sha(out[k])) for k in SHA_KEYS}
    d["bits.logits_last256"] = out["logits_last256"].view(torch.int32).cpu().numpy().view(np.uint32)
    d["bits.k_last_slot"] = out["k_last_slot"].view(torch.int16).cpu().numpy().view(np.uint16)
    d["peak"] = int(out["peak"])
    return d


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    envs = Envs()
    store, nondet = {}, []
    for name in CASES:
        first, second = run_case(envs, name), run_case(envs, name)
        assert first["untouched"] and second["untouched"], f"{name}: the call changed cache bits outside the slots it writes"
        assert all(bool(torch.isfinite(first[k].float()).all()) for k in ("logits_all", "logits_last", "kv_written")), name
        a, b = digests(first), digests(second)
        launches = count_launches(envs, name)
        store[name + ".launches"] = np.array(launches, dtype=np.int64)
        if not same(a, b):
            nondet.append(name)
            diff = [k for k in a if not np.array_equal(a[k], b[k])]
            print(f"{name:32s} DOES NOT REPRODUCE: {diff}; |logits_last| max diff "
                  f"{float((first['logits_last'] - second['logits_last']).abs().max()):.3e}", flush=True)
            continue
        for k, v in a.items():
            store[f"{name}.{k}"] = np.array(v)
        print(f"{name:32s} peak {a['peak']:>10d}  launches {dict(zip(CLASSES, launches))}  logits_last {a['sha.logits_last'][:12]}", flush=True)
    store["nondet"] = np.array(nondet, dtype=str)
    envs.close()
    assert len(nondet) <= 2, f"{len(nondet)} of {len(CASES)} cases do not reproduce on this commit: {nondet}"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **store)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
