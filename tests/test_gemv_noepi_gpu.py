"""The operand-free form of the weight-stream GEMV (gemv_bf16_noepi_kernel): launches with neither bias nor residual, bf16 weights, one
or two rows.  Everything goes through the production dispatch: binding.linear(..., impl=1), and linear_rmsnorm with knob 9 = 0 (two rows
stay on the GEMV).  No case passes a bias or a residual, so every launch takes the new form.  Shapes, the smallest at which a path exists:

  one unit per wave     K 4096, N 6 / 257, M 1 / 2       row clamp; the 4-wave grid
  looping 8-wave grid   K 4096, N 8200, M 1 / 2          4100 units = 513 workgroups capped to 512: some waves take a second unit
  looping with SwiGLU   K 4096, N 16448, M 1, norm       8224 units: the gate / up interleave across a unit boundary
  K short               K 512, N 8200, M 1               the short-K body
  several batches       K 14336, N 6, M 1                the many-batch body

Two checks per case:
1. against the float64 product of the same bf16-rounded inputs, tolerances of test_gemv_stream_gpu.py / test_ops_gpu.py::test_gemv
   (BF16_MAX 6e-3, BF16_L2 3e-3; 1e-4 for fp32 output);
2. torch.equal with the same launch given an all-zero bf16 residual: that one runs gemv_bf16_kernel, which adds +0 - the new form is the
   old one bit for bit, without a fixture from another commit."""
import pytest
import torch

from util import bf16r, check_close

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


def _ref(x, w, act=0, norm_w=None, eps=1e-5):
    """float64 reference from the bf16-rounded inputs; with norm_w the normalised row is rounded to bf16 as the kernel stages it"""
    xf = bf16r(x).double()
    if norm_w is not None:
        xf = bf16r(norm_w.double() * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps))).double()
    y = xf @ bf16r(w).double().t()
    if act == ACT_SWIGLU:
        N = w.shape[0]
        yy = y.view(y.shape[0], N // 32, 2, 16)
        y = (torch.nn.functional.silu(yy[:, :, 0]) * yy[:, :, 1]).reshape(y.shape[0], N // 2)
    return y.float()


def _run(B, x, w, nw, act, fp32, residual):
    with B.tuned(skinny_mode=0):
        if nw is not None:
            out = B.linear_rmsnorm(x, nw, 1e-5, w, residual=residual, act=act, out_fp32=fp32)
        else:
            out = B.linear(x, w, residual=residual, act=act, out_fp32=fp32, impl=1)
    torch.cuda.synchronize()
    return out


CASES = [(4096, N, M, norm, 0) for N in (6, 257, 8200) for M in (1, 2) for norm in (False, True)]
CASES += [(4096, 16448, 1, True, ACT_SWIGLU)]
CASES += [(512, 8200, 1, norm, 0) for norm in (False, True)]
CASES += [(14336, 6, 1, norm, 0) for norm in (False, True)]


@pytest.mark.parametrize("fp32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("K,N,M,norm,act", CASES)
def test_noepi(B, K, N, M, norm, act, fp32):
    x = _rand((M, K), 3.0 if norm else 1.0, 64).bfloat16()
    w = _rand((N, K), 0.03, 65).bfloat16()
    nw = _rand((K,), 0.2, 66) + 1.0 if norm else None
    n_out = N // 2 if act == ACT_SWIGLU else N
    out = _run(B, x, w, nw, act, fp32, None)
    assert out.dtype == (torch.float32 if fp32 else torch.bfloat16) and tuple(out.shape) == (M, n_out)
    name = f"gemv noepi {M}x{N}x{K} norm={norm} act={act} fp32={fp32}"
    if fp32:
        check_close(name, out, _ref(x, w, act, nw), 1e-4, 1e-4)
    else:
        check_close(name, out, _ref(x, w, act, nw), BF16_MAX, BF16_L2)
    with_operands = _run(B, x, w, nw, act, fp32, torch.zeros(M, n_out, dtype=torch.bfloat16, device="cuda"))
    assert torch.equal(out, with_operands), f"{name}: {int((out != with_operands).sum())} of {out.numel()} outputs differ from gemv_bf16_kernel's"
