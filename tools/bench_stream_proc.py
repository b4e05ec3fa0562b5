#!/usr/bin/env python
"""What the per-row logits processors and per-row stop sequences cost per decode step: 32-layer synthetic
Zephyr-7B, 64-id prompts, at 1 row and at 64 rows.
    python tools/bench_stream_proc.py [layers] [rounds] [parent_library.so]
Legs, taken in turn inside every round so that drift hits them alike; every window is 63 graph steps ended by one device synchronise,
behind an untimed window of the same leg that takes the graph capture (and grows the processors' histories to 63 ids: the timed window
sees 63..126 of them); per leg the best and the median of `rounds` windows:
  a  the parent commit's plain step - a second engine on the parent's library (third argument; left out without it)
  b  this tree with both modes off; the spread of a (worst - best) is the run-to-run yardstick b must sit inside
  c  the call-level processor kernel with one config: penalty 1.2, n-gram 3, two bad words
  d  the per-row kernel with that config in every row (same ids as c, asserted)
  e  the per-row kernel with one active row of 64, the others inactive (row 0 = d's row 0, the other rows = b's, asserted)
  fc d's processors in every row + the call-level stop matcher with four id sequences that never match
  fr d's processors in every row + the matcher in per-row mode, the same four sequences in every row's own region
Under `rocprofv3 --kernel-trace --stats` the kernels of interest are logits_process_rows_kernel, logits_process_kernel and
stop_match_kernel (VZ_BENCH_LEGS=d,fr runs legs apart)."""
import ctypes
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vision-zephyr_amd"))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from vz_hip import binding as Bd, logits_proc as LP, stop as ST, synth  # noqa: E402

layers = int(sys.argv[1]) if len(sys.argv) > 1 else 32
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
parent_path = sys.argv[3] if len(sys.argv) > 3 else None
n_steps = 63
only = [s for s in os.environ.get("VZ_BENCH_LEGS", "").split(",") if s]


def build(max_batch):
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    hf = VisZephyrConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=layers, num_attention_heads=32,
                         num_key_value_heads=8, vocab_size=32000, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2,
                         bos_token_id=1)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    hf.mm_hidden_size = 5120
    m = VisZephyrForCausalLM.from_synthetic(hf, seed=0, device="cuda:0", max_batch=max_batch, max_ctx=512, max_tiles=1, max_text=64)
    m._ensure_ready()
    return m


def build_on(path):
    """the same model on another build of the library (the parent commit's): its engine keeps the handle it was created with"""
    lib = ctypes.CDLL(path)
    for name, (res, args) in Bd.SYMBOLS.items():
        fn = getattr(lib, name, None)          # (the symbols this tree adds are not there)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    ours, Bd._lib = Bd.load_library(), lib
    try:
        return build(64)
    finally:
        Bd._lib = ours


model = build(64)
eng = model.engine
parent = build_on(parent_path).engine if parent_path else None
CFG = LP.parse(repetition_penalty=1.2, no_repeat_ngram_size=3, bad_words_ids=[[11, 12], [13, 14, 15]], eos=[], vocab=32000)
SEQS = [[5, 6, 40000 + k] for k in range(4)]          # end past the vocabulary: never a hit
PLAN = ST.Plan(seqs=[(s, 0) for s in SEQS])


class Leg:
    def __init__(self, name, e=eng, proc=None, active=None, stop=None):
        self.name, self.e, self.proc, self.active, self.stop = name, e, proc, active, stop

    def arm(self, B, first):
        e = self.e
        if self.proc == "call":
            e.set_logits_proc(CFG)
        if self.proc == "rows":
            e.set_logits_proc_rows(True)
        if self.stop == "call":
            e.set_stop(PLAN)
        if self.stop == "rows":
            e.set_stop_row_seqs(True)

    def rows(self, B, first, fresh):
        """behind every decode_begin; fresh: the records are written (once per arming: the histories then grow over both windows)"""
        e = self.e
        if self.proc == "rows" and fresh:
            for r in range(B if self.active is None else self.active):
                e.decode_set_row_logits_proc(r, CFG)
        if self.stop == "rows" and fresh:
            for r in range(B):
                e.decode_set_row_stop_seqs(r, SEQS)
        if self.stop:
            e.stop_rows(0, first)

    def disarm(self):
        e = self.e
        if self.stop == "rows":
            e.set_stop_row_seqs(False)
        if self.stop == "call":
            e.set_stop(None)
        if self.proc == "rows":
            e.set_logits_proc_rows(False)
        if self.proc == "call":
            e.set_logits_proc(None)


LEGS = ([Leg("a", parent)] if parent is not None else []) + [
    Leg("b"), Leg("c", proc="call"), Leg("d", proc="rows"), Leg("e", proc="rows", active=1), Leg("fc", proc="rows", stop="call"),
    Leg("fr", proc="rows", stop="rows")]
if only:
    LEGS = [leg for leg in LEGS if leg.name in ("a", "b") or leg.name in only]

for B in (1, 64):
    ids = torch.stack([synth.synth_ids(64, 32000, image_pos=-1, seed=10 + b) for b in range(B)]).cuda()
    firsts = {}
    for e in {leg.e for leg in LEGS}:
        _, last = e.prefill(e.embed_tokens(ids), [64] * B)
        firsts[e] = Bd.argmax(last)
    out = torch.empty(B, n_steps, dtype=torch.int32, device="cuda:0")
    ts = {leg.name: [] for leg in LEGS}
    ref = {}
    for r in range(rounds + 1):          # round 0 warms every leg up
        for leg in LEGS:
            first = firsts[leg.e]
            leg.arm(B, first)
            try:
                for timed in (False, True):
                    leg.e.decode_begin(first, [64] * B, [64] * B)
                    leg.rows(B, first, not timed)
                    if not timed:
                        leg.e.decode_steps(n_steps, out=out)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg.e.decode_steps(n_steps, out=out)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / n_steps * 1e3
                if leg.stop:
                    assert leg.e.stop_at(0, B).tolist() == [-1] * B, f"{leg.name}: a row stopped"
            finally:
                leg.disarm()
            ref.setdefault(leg.name, out.clone())
            assert torch.equal(out, ref[leg.name]), f"{leg.name}: the ids moved between rounds"
            if r:
                ts[leg.name].append(dt)
    if "a" in ref:
        assert torch.equal(ref["a"], ref["b"]), "both modes off: not the parent's ids"
    if "c" in ref and "d" in ref:
        assert torch.equal(ref["c"], ref["d"]) and not torch.equal(ref["c"], ref["b"]), "per-row records: not the call-level kernel's ids"
    if "e" in ref and "d" in ref and B > 1:
        assert torch.equal(ref["e"][0], ref["d"][0]) and torch.equal(ref["e"][1:], ref["b"][1:]), "one active row: the others moved"
    for k in ("fc", "fr"):
        assert k not in ref or "d" not in ref or torch.equal(ref[k], ref["d"]), f"{k}: the matcher moved an id"
    best = {}
    for leg in LEGS:
        v = sorted(ts[leg.name])
        best[leg.name] = (v[0], v[len(v) // 2], v[-1])
        print(f"rows {B:2d} {leg.name:2s}: best {v[0]:.4f} ms/step, median {v[len(v) // 2]:.4f}, worst {v[-1]:.4f}", flush=True)
    base = best.get("a", best["b"])
    print(f"rows {B:2d} spread of {'a' if 'a' in best else 'b'} (worst - best): {(base[2] - base[0]) * 1e3:.1f} us/step", flush=True)
    for x, y in (("b", "a"), ("d", "c"), ("e", "b"), ("d", "b"), ("fr", "fc"), ("fr", "d")):
        if x in best and y in best:
            print(f"rows {B:2d} {x:2s} - {y:2s}: {(best[x][0] - best[y][0]) * 1e3:+.1f} us/step on the best, {(best[x][1] - best[y][1]) * 1e3:+.1f} us on the median",
                  flush=True)
