#!/usr/bin/env python
"""Record the exact output bits of the weight-stream GEMV (gemv.hip) on a fixed list of seeded cases.

    python tools/dump_gemv_bits.py [out.npz]          default: tests/golden/gemv_parent_bits.npz   (needs the GPU)

Run it on the commit whose arithmetic is the reference: tests/test_gemv_stream_gpu.py replays the same cases
(this module is its case list) and asserts torch.equal against the stored outputs.  Inputs come from CPU-generator
seeds, so only the outputs are stored: bf16 as their uint16 bit patterns, fp32 as float32."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "vision-zephyr_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DEFAULT_OUT = os.path.join(REPO, "tests", "golden", "gemv_parent_bits.npz")
ACT_SWIGLU = 3

# name: M, N, K and the options of one launch.  The first four are the batch-1 decode shapes of the 7B model.
CASES = {
    "qkv": dict(M=1, N=6144, K=4096, norm=True),
    "gate_up": dict(M=1, N=28672, K=4096, norm=True, act=ACT_SWIGLU),
    "down": dict(M=1, N=4096, K=14336, residual=True),
    "lm_head": dict(M=1, N=32000, K=4096, norm=True, fp32=True),
    "o_inplace": dict(M=1, N=4096, K=4096, residual=True, inplace=True),
    "k512_n257_m1": dict(M=1, N=257, K=512, bias=True, residual=True),
    "k4608_n6_m2": dict(M=2, N=6, K=4608),
    "k14336_n257_m3": dict(M=3, N=257, K=14336, bias=True, residual=True),
    "k512_n8200_m1": dict(M=1, N=8200, K=512, fp32=True),
    "k512_n16400_m8": dict(M=8, N=16400, K=512),
    "k4096_n257_m8_norm": dict(M=8, N=257, K=4096, norm=True),
    "k2048_n257_m7_norm": dict(M=7, N=257, K=2048, norm=True),
    "swiglu_n128_m2_norm": dict(M=2, N=128, K=4096, norm=True, act=ACT_SWIGLU, residual=True),
    "fp8_k9216_n257_m1": dict(M=1, N=257, K=9216, fp8=True, bias=True, residual=True),
    "fp8_k14336_n4096_m1": dict(M=1, N=4096, K=14336, fp8=True, residual=True),
    "fp8_k4096_n6144_m2_norm": dict(M=2, N=6144, K=4096, fp8=True, norm=True),
}


def rand(shape, std, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * std


def make_inputs(name, device="cuda"):
    """the seeded tensors of one case, on `device`; fp8 cases carry the e4m3 rows, their scales and the dequantised weights"""
    c = CASES[name]
    M, N, K = c["M"], c["N"], c["K"]
    seed = 1000 + 10 * sorted(CASES).index(name)
    n_out = N // 2 if c.get("act") == ACT_SWIGLU else N
    t = dict(x=rand((M, K), 1.0, seed).bfloat16().to(device), w=rand((N, K), 0.03, seed + 1).to(device))
    t["bias"] = rand((N,), 0.3, seed + 2).to(device) if c.get("bias") else None
    t["residual"] = rand((M, n_out), 1.0, seed + 3).bfloat16().to(device) if c.get("residual") else None
    t["norm_w"] = (rand((K,), 0.2, seed + 4) + 1.0).to(device) if c.get("norm") else None
    if c.get("fp8"):
        from vz_hip import quant
        t["w8"], t["scale"] = quant.quantize_rows(t["w"])
        t["wq"] = quant.dequantize_rows(t["w8"], t["scale"])
    else:
        t["w"] = t["w"].bfloat16()
    return t


def run_case(B, name, t):
    """one launch of the case on the GEMV kernel (knob 9 = 0 keeps rows 2..8 off the MFMA stream); returns the output tensor"""
    c = CASES[name]
    act, fp32 = c.get("act", 0), bool(c.get("fp32"))
    res = t["residual"]
    if c.get("inplace"):
        res = res.clone()
    with B.tuned(skinny_mode=0):
        if c.get("fp8"):
            out = B.linear_fp8(t["x"], t["w8"], t["scale"], bias=t["bias"], residual=res, act=act, out_fp32=fp32,
                               norm_w=t["norm_w"], norm_eps=1e-5)
        elif c.get("norm"):
            out = B.linear_rmsnorm(t["x"], t["norm_w"], 1e-5, t["w"], residual=res, act=act, out_fp32=fp32)
        elif c.get("inplace"):      # C == residual, as the decode step adds the O and down projections to the residual stream
            M, K = t["x"].shape
            N = t["w"].shape[0]
            B.check(B.lib().vz_op_linear_impl(1, B.ptr(t["x"]), t["x"].stride(0), B.ptr(t["w"]), t["w"].stride(0), B.ptr(res), res.stride(0),
                                              M, N, K, None, B.ptr(res), res.stride(0), act, 0, B.stream_ptr(res.device)))
            out = res
        else:
            out = B.linear(t["x"], t["w"], bias=t["bias"], residual=res, act=act, out_fp32=fp32, impl=1)
    torch.cuda.synchronize()
    return out


def to_bits(out):
    return out.cpu().numpy() if out.dtype == torch.float32 else out.view(torch.int16).cpu().numpy().view(np.uint16)


def main():
    from vz_hip import binding as B
    B.load_library()
    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    bits = {}
    for name in CASES:
        bits[name] = to_bits(run_case(B, name, make_inputs(name)))
        print(f"{name:28s} {bits[name].dtype} {bits[name].shape}")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **bits)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
