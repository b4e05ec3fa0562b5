#!/usr/bin/env python
"""Record the exact output bits of the one-launch decode attention (attn_decode.hip, body<> of attn_decode_body.h) on a
fixed list of seeded cases.

    python tools/dump_attn_decode_bits.py [out.npz]     default: tests/golden/attn_decode_parent_bits.npz   (needs the GPU)

Run it on the commit whose arithmetic is the reference: tests/test_attn_decode_bits_gpu.py replays the same cases (this
module is its case list) and asserts torch.equal against the stored bits of `o` and of the appended K / V rows.  Inputs
come from CPU-generator seeds, so only outputs are stored (bf16 as uint16 bit patterns).

Before every call the cache rows >= len AND row `slot` itself (the row the call appends) hold NaN bit patterns (0x7fc0).
The reference never reads them, so its bits do not depend on them; a kernel that lets a clamped or unconditional load of
such a row reach a result turns the output non-finite."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "vision-zephyr_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DEFAULT_OUT = os.path.join(REPO, "tests", "golden", "attn_decode_parent_bits.npz")
HQ, HKV, D = 32, 8, 128
NAN_BF16 = 0x7fc0

# name: lens (one per batch row; len = slot + 1), max_ctx, nsplit, window; first_len = a call at that length goes first on the
# same ticket buffer and the same caches (what it appended stays), and the SECOND call is the one recorded
CASES = {
    "len1": dict(lens=[1], max_ctx=256),                                   # slot 0
    "len128": dict(lens=[128], max_ctx=256),                               # 1 split: the direct path
    "len129": dict(lens=[129], max_ctx=256),                               # 2 splits: the ticket path
    "len1025": dict(lens=[1025], max_ctx=1152),                            # 9 splits
    "len2048": dict(lens=[2048], max_ctx=2176),                            # 16 splits
    "len2049": dict(lens=[2049], max_ctx=2176),                            # 17 splits: the benchmark's case
    "len2944": dict(lens=[2944], max_ctx=3072),                            # 23 splits
    "len4096": dict(lens=[4096], max_ctx=4096),                            # 32 splits, the bound; the cache exactly full
    "len2100_ns18": dict(lens=[2100], max_ctx=2176, nsplit=18),            # the benchmark's bucket
    "len2048_ns4": dict(lens=[2048], max_ctx=2176, nsplit=4),              # four chunks per split: the chunk loop
    "len5000_w4096": dict(lens=[5000], max_ctx=5120, window=4096),         # lo > 0
    "b2_1900_1600": dict(lens=[1900, 1600], max_ctx=2048),                 # ragged rows
    "len300_full": dict(lens=[300], max_ctx=300),                          # cache exactly full: the last chunk runs past its end
    "len2049_second": dict(lens=[2049], max_ctx=2176, first_len=2048),     # same ticket buffer: the merger re-zeroed it
}


def rand(shape, std, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * std


def case_seed(name):
    return 5000 + 10 * sorted(CASES).index(name)


def make_inputs(name, device="cuda"):
    """the seeded tensors of one case on `device`.  The rotation tables are seeded numbers, not cos / sin: the kernel only
    multiplies by them, and a CPU libm may not be the same on every machine"""
    c = CASES[name]
    Bn, max_ctx, seed = len(c["lens"]), c["max_ctx"], case_seed(name)
    return dict(kc=rand((Bn, HKV, max_ctx, D), 1.0, seed).bfloat16().to(device), vc=rand((Bn, HKV, max_ctx, D), 1.0, seed + 1).bfloat16().to(device),
                cos=rand((max_ctx + 8, D // 2), 0.7, seed + 2).to(device).contiguous(), sin=rand((max_ctx + 8, D // 2), 0.7, seed + 3).to(device).contiguous(),
                qkv=[rand((Bn, (HQ + 2 * HKV) * D), 1.0, seed + 4 + i).bfloat16().to(device) for i in range(2)])


def poison(cache, lens):
    """rows >= slot (= len - 1) of every batch row <- NaN bit patterns"""
    bits = cache.view(torch.int16)
    for b, n in enumerate(lens):
        bits[b, :, n - 1:, :] = NAN_BF16


def run_case(B, name, t):
    """the case's call (after its first call, if it has one) on fresh copies of the caches; returns o [B, Hq, D] and the appended
    K and V rows [B, Hkv, D]"""
    c = CASES[name]
    kc, vc = t["kc"].clone(), t["vc"].clone()
    ticket = None
    calls = ([[c["first_len"]]] if c.get("first_len") else []) + [c["lens"]]
    for i, lens in enumerate(calls):
        poison(kc, lens)
        poison(vc, lens)
        slot = torch.tensor([n - 1 for n in lens], dtype=torch.int32, device=kc.device)
        pos = slot + 5
        o, ticket = B.attention_decode_fused(t["qkv"][i], kc, vc, t["cos"], t["sin"], pos, slot, HQ, D ** -0.5,
                                             c.get("nsplit", 32), c.get("window", 0), ticket)
    torch.cuda.synchronize()
    assert int(ticket.abs().sum()) == 0, "ticket not reset by the last arriver"
    idx = slot.long()
    rows = torch.arange(len(lens), device=kc.device)
    return o, kc[rows, :, idx, :].contiguous(), vc[rows, :, idx, :].contiguous()


def to_bits(x):
    return x.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def main():
    from vz_hip import binding as B
    B.load_library()
    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    bits = {}
    for name in CASES:
        o, k, v = run_case(B, name, make_inputs(name))
        assert bool(torch.isfinite(o.float()).all() and torch.isfinite(k.float()).all() and torch.isfinite(v.float()).all()), name
        bits[name + ".o"], bits[name + ".k"], bits[name + ".v"] = to_bits(o), to_bits(k), to_bits(v)
        print(f"{name:18s} o {tuple(o.shape)}  k|v {tuple(k.shape)}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **bits)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
