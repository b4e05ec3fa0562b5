"""The weight-stream GEMV (gemv.hip) at the edges of its batch loop, and bit for bit against the commit before the rolling refill.

Every case is forced onto gemv_bf16_kernel: binding.linear(..., impl=1), and linear_rmsnorm / linear_fp8 with knob 9 = 0 (no MFMA
stream for 2..8 rows).  A bf16 chunk is 512 k, a batch 8 chunks (4096 k); e4m3 chunks are 1024 k.

1. Against the float64 product of the same bf16-rounded inputs, tolerances of test_ops_gpu.py::test_gemv (BF16_MAX 6e-3, BF16_L2 3e-3,
   1e-4 for fp32 output): K = 512 (one chunk), 4096 (exactly one batch), 4608 (one refill of one chunk), 14336 (3.5 batches); N = 2, 6,
   257 (row clamp and the n >= N break), 8200 / 16400 at K = 512 (more units than waves in the grid: the workgroups loop); M = 1, 2, 3
   (a zero-filled row of the 4-row form), 8; fused RMSNorm, SwiGLU, bias + residual, in-place residual, fp32 output; e4m3 weights.
2. torch.equal with tests/golden/gemv_parent_bits.npz, which tools/dump_gemv_bits.py wrote on the parent commit (its CASES are the list)."""
import os
import sys

import numpy as np
import pytest
import torch

from util import GOLDEN, REPO, bf16r, check_close

sys.path.insert(0, os.path.join(REPO, "tools"))
import dump_gemv_bits as D  # noqa: E402

pytestmark = pytest.mark.gpu

BF16_MAX = 6e-3
BF16_L2 = 3e-3
ACT_SWIGLU = 3


@pytest.fixture(scope="module")
def B():
    from vz_hip import binding
    binding.load_library()
    return binding


def _rand(shape, std=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std).to("cuda")


def _ref(x, w, bias=None, residual=None, act=0, norm_w=None, eps=1e-5):
    """float64 reference from the bf16-rounded inputs; with norm_w the normalised row is rounded to bf16 as the kernel stages it"""
    xf = bf16r(x).double()
    if norm_w is not None:
        xf = bf16r(norm_w.double() * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps))).double()
    y = xf @ bf16r(w).double().t()
    if bias is not None:
        y = y + bias.double()
    if act == ACT_SWIGLU:
        N = w.shape[0]
        yy = y.view(y.shape[0], N // 32, 2, 16)
        y = (torch.nn.functional.silu(yy[:, :, 0]) * yy[:, :, 1]).reshape(y.shape[0], N // 2)
    if residual is not None:
        y = y + bf16r(residual).double()
    return y.float()


def _Knob9(B):
    """knob 9 (skinny_mode) = 0 for the block: 2..8 rows stay on the GEMV"""
    return B.tuned(skinny_mode=0)


# K x N x M through the plain launch: bias + residual in bf16, and fp32 output (8 rows fit the 160 KiB of LDS up to K = 10224: 9728 is
# 2 batches + 3 chunks).  The last three loop over units at a K of whole batches: the refill of a unit's last batch reaches into the wave's
# next unit (two batches per unit; the 4-row form at one batch; the 1-row form at one batch).
EDGE = [(512, 2, 1), (512, 257, 2), (4096, 6, 1), (4096, 257, 3), (4096, 257, 8), (4608, 2, 1), (4608, 257, 2), (4608, 6, 8),
        (14336, 6, 1), (14336, 257, 2), (14336, 257, 3), (9728, 2, 8), (512, 8200, 1), (512, 8200, 8), (512, 16400, 1), (512, 16400, 8),
        (8192, 8200, 1), (4096, 8200, 4), (4096, 8200, 1)]


@pytest.mark.parametrize("K,N,M", EDGE)
def test_edges_plain(B, K, N, M):
    x = _rand((M, K), 1.0, 14).bfloat16()
    w = _rand((N, K), 0.03, 15).bfloat16()
    bias = _rand((N,), 0.2, 16)
    res = _rand((M, N), 0.5, 17).bfloat16()
    out = B.linear(x, w, bias=bias, residual=res, impl=1)
    check_close(f"gemv stream {M}x{N}x{K}", out, _ref(x, w, bias, res), BF16_MAX, BF16_L2)
    out32 = B.linear(x, w, out_fp32=True, impl=1)
    check_close(f"gemv stream fp32 {M}x{N}x{K}", out32, _ref(x, w), 1e-4, 1e-4)


@pytest.mark.parametrize("K,N,M", [(512, 257, 1), (4096, 6, 1), (4096, 257, 2), (4096, 257, 3), (2048, 257, 8), (4608, 257, 1), (4608, 6, 2),
                                   (14336, 257, 1), (14336, 6, 3)])
def test_edges_fused_rmsnorm(B, K, N, M):
    x = _rand((M, K), 3.0, 24).bfloat16()
    w = _rand((N, K), 0.03, 25).bfloat16()
    nw = _rand((K,), 0.2, 26) + 1.0
    res = _rand((M, N), 0.5, 27).bfloat16()
    with _Knob9(B):
        out = B.linear_rmsnorm(x, nw, 1e-5, w, residual=res)
        out32 = B.linear_rmsnorm(x, nw, 1e-5, w, out_fp32=True)
    torch.cuda.synchronize()
    # the staged row is bf16, and the reference rounds it the same way: where the kernel's fp32 norm and the float64 one round an x entry
    # apart (about 5e-5 of the entries) the sum moves by 2^-8 of ONE of its K terms, ~6e-5 of a typical output at K = 4096
    check_close(f"gemv stream norm {M}x{N}x{K}", out, _ref(x, w, None, res, 0, nw), BF16_MAX, BF16_L2)
    check_close(f"gemv stream norm fp32 {M}x{N}x{K}", out32, _ref(x, w, None, None, 0, nw), 1e-4, 1e-4)


@pytest.mark.parametrize("N", [64, 128])
@pytest.mark.parametrize("K,M,norm", [(4096, 1, True), (4096, 2, False), (4608, 1, False), (14336, 2, False), (512, 3, False)])
def test_edges_swiglu(B, N, K, M, norm):
    x = _rand((M, K), 1.0, 34).bfloat16()
    w = _rand((N, K), 0.03, 35).bfloat16()
    nw = _rand((K,), 0.2, 36) + 1.0 if norm else None
    res = _rand((M, N // 2), 0.5, 37).bfloat16()
    with _Knob9(B):
        out = B.linear_rmsnorm(x, nw, 1e-5, w, residual=res, act=ACT_SWIGLU) if norm else B.linear(x, w, residual=res, act=ACT_SWIGLU, impl=1)
    torch.cuda.synchronize()
    check_close(f"gemv stream swiglu {M}x{N}x{K}", out, _ref(x, w, None, res, ACT_SWIGLU, nw), BF16_MAX, BF16_L2)


@pytest.mark.parametrize("K,N", [(4096, 4096), (14336, 4096), (4608, 257)])
def test_inplace_residual(B, K, N):
    """C == residual, as the decode step adds the O and down projections to the residual stream"""
    x = _rand((1, K), 1.0, 44).bfloat16()
    w = _rand((N, K), 0.03, 45).bfloat16()
    buf = _rand((1, N), 0.5, 46).bfloat16()
    ref = _ref(x, w, None, buf)
    B.check(B.lib().vz_op_linear_impl(1, B.ptr(x), x.stride(0), B.ptr(w), w.stride(0), B.ptr(buf), buf.stride(0), 1, N, K, None, B.ptr(buf),
                                      buf.stride(0), 0, 0, B.stream_ptr(buf.device)))
    torch.cuda.synchronize()
    check_close(f"gemv stream in-place 1x{N}x{K}", buf, ref, BF16_MAX, BF16_L2)


@pytest.mark.parametrize("K,N,M", [(1024, 257, 1), (1024, 6, 3), (9216, 257, 1), (9216, 2, 2), (14336, 257, 1), (9216, 6, 8), (8192, 257, 1)])
def test_edges_e4m3(B, K, N, M):
    """e4m3 chunks are 1024 k: one chunk, 9 (one refill of one chunk), 14 (1.75 batches), 8 (exactly one batch)"""
    from vz_hip import quant
    x = _rand((M, K), 1.0, 54).bfloat16()
    w8, scale = quant.quantize_rows(_rand((N, K), 0.03, 55))
    wq = quant.dequantize_rows(w8, scale)
    bias = _rand((N,), 0.2, 56)
    res = _rand((M, N), 0.5, 57).bfloat16()
    with _Knob9(B):
        out = B.linear_fp8(x, w8, scale, bias=bias, residual=res)
        out32 = B.linear_fp8(x, w8, scale, out_fp32=True)
    torch.cuda.synchronize()
    check_close(f"gemv stream e4m3 {M}x{N}x{K}", out, _ref(x, wq, bias, res), BF16_MAX, BF16_L2)
    check_close(f"gemv stream e4m3 fp32 {M}x{N}x{K}", out32, _ref(x, wq), 1e-4, 1e-4)


@pytest.fixture(scope="module")
def parent_bits():
    z = np.load(os.path.join(GOLDEN, "gemv_parent_bits.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(D.CASES))
def test_bits_equal_parent(B, parent_bits, name):
    got = D.to_bits(D.run_case(B, name, D.make_inputs(name)))
    want = parent_bits[name]
    assert got.dtype == want.dtype and got.shape == want.shape
    same = torch.equal(torch.from_numpy(got.astype(np.int64) if got.dtype == np.uint16 else got),
                       torch.from_numpy(want.astype(np.int64) if want.dtype == np.uint16 else want))
    assert same, f"{name}: {int((got != want).sum())} of {got.size} outputs differ from the parent commit's bits"
