"""Operator-level parity of the HIP kernels (through the C ABI) against fp32 references computed
from the same bf16-rounded inputs.  Tolerances: outputs are bf16, so one rounding step is
2^-9 = 1.95e-3 relative; fp32-output kernels are held to 1e-4."""
import math

import pytest
import torch

from util import bf16r, check_close

pytestmark = pytest.mark.gpu

BF16_MAX = 6e-3   # max-norm: <= 1.5 bf16 ulp of the largest element
BF16_L2 = 3e-3    # relative L2: one bf16 rounding is ~1.1e-3 rms


@pytest.fixture(scope="module")
def B():
    from vz_hip import binding
    binding.load_library()
    return binding


def _rand(shape, std=1.0, seed=0, device="cuda"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std).to(device)


def _ref_linear(x, w, bias, residual, act):
    y = bf16r(x).double() @ bf16r(w).double().t()
    if bias is not None:
        y = y + bias.double()
    if act == 1:
        y = y * torch.sigmoid(1.702 * y)
    elif act == 2:
        y = torch.nn.functional.gelu(y)
    elif act == 3:
        N = w.shape[0]
        yy = y.view(y.shape[0], N // 32, 2, 16)
        y = (torch.nn.functional.silu(yy[:, :, 0]) * yy[:, :, 1]).reshape(y.shape[0], N // 2)
    if residual is not None:
        y = y + bf16r(residual).double()
    return y.float()


# (M, N, K): CLIP (577*T rows), patch embed K=640, Zephyr shapes, ragged N = 32001, tiny M through the tile kernel
GEMM_SHAPES = [(577 * 2, 3072, 1024), (576, 1024, 640), (127, 6144, 4096), (300, 4096, 14336 // 4), (64, 32001, 512),
               (1, 256, 128), (129, 130, 64), (2048, 4096, 4096)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_plain(B, M, N, K):
    x = _rand((M, K), 1.0, 1).bfloat16()
    w = _rand((N, K), 0.05, 2).bfloat16()
    out = B.linear(x, w, impl=0)
    check_close(f"gemm {M}x{N}x{K}", out, _ref_linear(x, w, None, None, 0), BF16_MAX, BF16_L2)


def test_gemm_fp32_out_matches_tightly(B):
    M, N, K = 200, 32001, 4096
    x = _rand((M, K), 1.0, 3).bfloat16()
    w = _rand((N, K), 0.02, 4).bfloat16()
    out = B.linear(x, w, out_fp32=True, impl=0)
    assert out.dtype == torch.float32 and out.shape == (M, N)
    check_close("gemm fp32 out", out, _ref_linear(x, w, None, None, 0), 1e-4, 1e-4)


def test_gemm_identity_asymmetric(B):
    """A = I against an asymmetric W: catches a transposed C write or a wrong fragment map exactly."""
    K = 128
    x = torch.eye(K, device="cuda").bfloat16()
    w = (torch.arange(192 * K, device="cuda").view(192, K) % 251 - 125).float().bfloat16()
    out = B.linear(x, w, out_fp32=True, impl=0)
    assert torch.equal(out, w.float().t().contiguous())


@pytest.mark.parametrize("act", [1, 2])
def test_gemm_bias_act_residual(B, act):
    M, N, K = 577, 4096, 1024
    x = _rand((M, K), 1.0, 5).bfloat16()
    w = _rand((N, K), 0.05, 6).bfloat16()
    bias = _rand((N,), 0.5, 7)
    res = _rand((M, N), 1.0, 8).bfloat16()
    out = B.linear(x, w, bias=bias, residual=res, act=act, impl=0)
    check_close(f"gemm epilogue act{act}", out, _ref_linear(x, w, bias, res, act), BF16_MAX, BF16_L2)


def test_gemm_residual_in_place(B):
    """the engine adds the residual into the very buffer it writes (C aliases residual)."""
    M, N, K = 300, 1024, 4096
    x = _rand((M, K), 1.0, 9).bfloat16()
    w = _rand((N, K), 0.02, 10).bfloat16()
    res = _rand((M, N), 1.0, 11).bfloat16()
    ref = _ref_linear(x, w, None, res, 0)
    buf = res.clone()
    import ctypes as C
    B.check(B.lib().vz_op_linear_impl(0, B.ptr(x), K, B.ptr(w), K, B.ptr(buf), N, M, N, K, None, B.ptr(buf), N, 0, 0,
                                      B.stream_ptr()))
    check_close("gemm in-place residual", buf, ref, BF16_MAX, BF16_L2)


@pytest.mark.parametrize("M", [130, 1])
def test_gemm_swiglu(B, M):
    N, K = 2 * 1792, 4096
    x = _rand((M, K), 1.0, 12).bfloat16()
    w = _rand((N, K), 0.03, 13).bfloat16()
    for impl in (0, 1):
        if impl == 1 and M > 8:
            continue
        out = B.linear(x, w, act=3, impl=impl)
        assert out.shape == (M, N // 2)
        check_close(f"swiglu impl{impl} M{M}", out, _ref_linear(x, w, None, None, 3), BF16_MAX, BF16_L2)


# (4, 4096, 14336) / (2, 1024, 28672): x does not fit 64 KiB of LDS -> the 16-wave workgroup form; (8, 512, 4096): 2 rows per wave
@pytest.mark.parametrize("M,N,K", [(1, 6144, 4096), (1, 4096, 14336), (2, 4096, 4096), (4, 1024, 4096), (1, 32001, 4096),
                                   (3, 257, 1024), (4, 4096, 14336), (2, 1024, 28672), (8, 512, 4096), (5, 6144, 4096)])
def test_gemv(B, M, N, K):
    x = _rand((M, K), 1.0, 14).bfloat16()
    w = _rand((N, K), 0.03, 15).bfloat16()
    res = _rand((M, N), 1.0, 16).bfloat16()
    bias = _rand((N,), 0.3, 17)
    out = B.linear(x, w, bias=bias, residual=res, impl=1)
    check_close(f"gemv {M}x{N}x{K}", out, _ref_linear(x, w, bias, res, 0), BF16_MAX, BF16_L2)
    out32 = B.linear(x, w, out_fp32=True, impl=1)
    check_close(f"gemv fp32 {M}x{N}x{K}", out32, _ref_linear(x, w, None, None, 0), 1e-4, 1e-4)


def test_linear_dispatch_rejects_bad_shapes(B):
    x = torch.zeros(4, 100, device="cuda").bfloat16()
    w = torch.zeros(8, 100, device="cuda").bfloat16()
    with pytest.raises(ValueError):
        B.linear(x, w)                      # K not a multiple of 64
    with pytest.raises(ValueError):
        B.linear(torch.zeros(4, 128).bfloat16(), torch.zeros(8, 128).bfloat16())   # CPU tensors: no fallback


@pytest.mark.parametrize("rows,cols", [(577 * 3, 1024), (96, 4096), (576 * 2, 5120), (5, 512)])
def test_layernorm(B, rows, cols):
    x = (_rand((rows, cols), 2.0, 18) + 0.7).bfloat16()
    w = _rand((cols,), 0.2, 19) + 1.0
    b = _rand((cols,), 0.2, 20)
    out = B.layernorm(x, w, b, 1e-5)
    ref = torch.nn.functional.layer_norm(bf16r(x).double(), (cols,), w.double(), b.double(), 1e-5).float()
    check_close(f"layernorm {rows}x{cols}", out, ref, BF16_MAX, BF16_L2)


def test_layernorm_zero_rows_give_bias(B):
    """Q-Former block 0 sees zero-padded text rows: LN(0) must be exactly the bias."""
    cols = 4096
    x = torch.zeros(7, cols, device="cuda").bfloat16()
    w = _rand((cols,), 0.2, 21) + 1.0
    b = _rand((cols,), 0.2, 22)
    out = B.layernorm(x, w, b, 1e-5)
    assert torch.equal(out.float(), bf16r(b).unsqueeze(0).expand(7, -1))


@pytest.mark.parametrize("rows,cols", [(127, 4096), (1, 4096), (2048, 4096)])
def test_rmsnorm(B, rows, cols):
    x = _rand((rows, cols), 3.0, 23).bfloat16()
    w = _rand((cols,), 0.2, 24) + 1.0
    out = B.rmsnorm(x, w, 1e-5)
    xf = bf16r(x).double()
    ref = (w.double() * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5))).float()
    check_close(f"rmsnorm {rows}x{cols}", out, ref, BF16_MAX, BF16_L2)


def _ref_attention(q, k, v, scale, causal, q_pos0, window, kv_len):
    Bn, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    qf, kf, vf = (bf16r(t).double() for t in (q, k, v))
    kf = kf.repeat_interleave(Hq // Hkv, dim=2)
    vf = vf.repeat_interleave(Hq // Hkv, dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", qf, kf) * scale
    kp = torch.arange(Sk, device=q.device).view(1, 1, 1, Sk)
    keep = torch.ones(Bn, 1, Sq, Sk, dtype=torch.bool, device=q.device)
    if kv_len is not None:
        keep = keep & (kp < kv_len.view(Bn, 1, 1, 1))
    if causal:
        qp = (torch.arange(Sq, device=q.device) + q_pos0).view(1, 1, Sq, 1)
        keep = keep & (kp <= qp)
        if window > 0:
            keep = keep & (kp > qp - window)
    s = s.masked_fill(~keep, float("-inf"))
    p = torch.softmax(s, dim=-1)
    p = torch.nan_to_num(p, nan=0.0)
    return torch.einsum("bhqk,bkhd->bqhd", p, vf).float()


ATTN_CASES = [
    # name, B, Sq, Sk, Hq, Hkv, D, causal, q_pos0, window, ragged kv_len
    ("clip", 2, 577, 577, 16, 16, 64, False, 0, 0, False),
    ("zephyr prefill", 1, 300, 300, 32, 8, 128, True, 0, 4096, False),
    # 12 query blocks x 32 heads = 384 workgroups, 256 is not a multiple of 12: the causal load-balancing order must stay a
    # bijection of the query blocks within every (head, batch) row (it was not; S = 2048 hid it)
    ("zephyr prefill 1501", 1, 1501, 1501, 32, 8, 128, True, 0, 4096, False),
    ("zephyr prefill batch 2 x 700", 2, 700, 700, 32, 8, 128, True, 0, 4096, False),
    ("zephyr padded batch", 2, 200, 200, 8, 2, 128, True, 0, 4096, True),
    ("zephyr window", 1, 260, 260, 4, 1, 128, True, 0, 100, False),
    ("qformer self blk0", 2, 32, 63, 8, 8, 512, False, 0, 0, False),
    ("qformer cross", 3, 32, 576, 8, 8, 512, False, 0, 0, False),
    ("qformer self", 2, 32, 32, 8, 8, 512, False, 0, 0, False),
    ("single key", 1, 5, 1, 4, 4, 64, False, 0, 0, False),
]


@pytest.mark.parametrize("case", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_attention(B, case):
    name, Bn, Sq, Sk, Hq, Hkv, D, causal, q_pos0, window, ragged = case
    q = _rand((Bn, Sq, Hq, D), 1.0, 30).bfloat16()
    k = _rand((Bn, Sk, Hkv, D), 1.0, 31).bfloat16()
    v = _rand((Bn, Sk, Hkv, D), 1.0, 32).bfloat16()
    kv_len = None
    if ragged:
        kv_len = torch.tensor([Sk, min(Sk, Sk // 2 + 3), Sk // 3 + 1][:Bn], dtype=torch.int32, device="cuda")
    scale = D ** -0.5
    out = B.attention(q, k, v, scale, causal, q_pos0, window, kv_len)
    ref = _ref_attention(q, k, v, scale, causal, q_pos0, window, kv_len)
    if ragged:   # padded query rows (beyond a row's own length) are don't-care
        for b in range(Bn):
            out[b, int(kv_len[b]):] = 0
            ref[b, int(kv_len[b]):] = 0
    check_close(f"attention {name}", out, ref, 8e-3, 4e-3)


def test_attention_strided_fused_qkv(B):
    """the engine hands Q/K/V as column slices of one fused projection output (CLIP layout)."""
    T, S, H, D = 2, 577, 16, 64
    qkv = _rand((T, S, 3 * H * D), 1.0, 33).bfloat16()
    q = qkv[:, :, :H * D].view(T, S, H, D)
    k = qkv[:, :, H * D:2 * H * D].view(T, S, H, D)
    v = qkv[:, :, 2 * H * D:].view(T, S, H, D)
    out = B.attention(q, k, v, 0.125)
    check_close("attention strided", out, _ref_attention(q, k, v, 0.125, False, 0, 0, None), 8e-3, 4e-3)


def test_attention_softmax_spike(B):
    """one key dominating late in the sequence forces the online-softmax rescale branch."""
    Bn, S, H, D = 1, 256, 2, 128
    q = _rand((Bn, S, H, D), 1.0, 34).bfloat16()
    k = _rand((Bn, S, H, D), 1.0, 35).bfloat16()
    v = _rand((Bn, S, H, D), 1.0, 36).bfloat16()
    k[0, 200] = (q[0, 17] * 4).bfloat16()
    out = B.attention(q, k, v, D ** -0.5)
    check_close("attention spike", out, _ref_attention(q, k, v, D ** -0.5, False, 0, 0, None), 8e-3, 4e-3)


@pytest.mark.parametrize("T,Sq,Sk,split", [(5, 32, 576, 0), (5, 32, 576, 3), (1, 32, 576, 0), (2, 17, 100, 0), (3, 64, 1000, 7),
                                           (24, 32, 576, 0)])
def test_attention_key_split_q_former_cross(B, T, Sq, Sk, split):
    """Q-Former cross-attention shape (32 queries x 576 visual tokens, 8 heads x 512) with the key tiles spread over
    workgroups + combine kernel: against the fp32 reference and against the one-workgroup launch of the same inputs."""
    H, D = 8, 512
    q = _rand((T, Sq, H, D), 1.0, 60).bfloat16()
    kv = _rand((T, Sk, 2 * H * D), 1.0, 61).bfloat16()          # K|V column slices of one projection, as the engine hands them
    k, v = kv[:, :, :H * D].view(T, Sk, H, D), kv[:, :, H * D:].view(T, Sk, H, D)
    k[0, Sk - 5] = (q[0, 3] * 3).bfloat16()                       # one dominating key inside the last split
    nsplit = split if split >= 2 else ((Sk + 31) // 32 + 2) // 3
    ws = torch.empty(T * H * nsplit * Sq * 516, dtype=torch.float32, device="cuda")
    with B.tuned(attn_split=split):
        out = B.attention(q, k, v, D ** -0.5, workspace=ws)
    one = B.attention(q, k, v, D ** -0.5)
    ref = _ref_attention(q, k, v, D ** -0.5, False, 0, 0, None)
    check_close(f"attention key-split T{T} {Sq}x{Sk}", out, ref, 8e-3, 4e-3)
    check_close(f"attention key-split vs one workgroup T{T} {Sq}x{Sk}", out, one.float(), 8e-3, 4e-3)
    # a workspace too small for any split falls back to the one-workgroup kernel: bit-identical
    small = B.attention(q, k, v, D ** -0.5, workspace=ws[:1024])
    assert torch.equal(small, one)
    if split == 0 and T > 1:      # the split follows Sk only: a tile's rows do not change with the tiles beside it
        assert torch.equal(B.attention(q[1:2], k[1:2], v[1:2], D ** -0.5, workspace=ws), out[1:2])


@pytest.mark.parametrize("M,N,K,act,use_res", [(2885, 1024, 4096, 0, True), (577, 1024, 4096, 0, True), (577, 3072, 1024, 0, False),
                                               (1154, 4096, 1024, 1, False), (700, 1000, 2048, 2, True)])
def test_k_slices_for_small_grids(B, M, N, K, act, use_res):
    """grids of fewer than 256 128^2 tiles with M > 512 (CLIP tower at 1..6 tiles) are cut along K into fp32 slabs + finalize:
    same values as the whole-K tiles up to fp32 re-association (one bf16 ulp at most), the same bits from launch to launch."""
    x = _rand((M, K), 1.0, 94).bfloat16()
    w = (_rand((N, K), 1.0, 95) * 0.03).bfloat16()
    bias = _rand((N,), 0.5, 96)
    res = _rand((M, N), 1.0, 97).bfloat16() if use_res else None
    whole = _whole_k(B, lambda: B.linear(x, w, bias, res, act, impl=0))
    a = B.linear(x, w, bias, res, act, impl=0)
    b = B.linear(x, w, bias, res, act, impl=0)
    assert torch.equal(a, b)
    ref = _ref_linear(x, w, bias, res, act)
    check_close(f"K slices {M}x{N}x{K}", a, ref, BF16_MAX, BF16_L2)
    assert float((a.float() - whole.float()).abs().max()) <= 2 ** -7 * float(whole.float().abs().max())


def test_argmax_first_max(B):
    x = _rand((3, 32001), 1.0, 37)
    x[1, 777] = 50.0
    x[1, 31000] = 50.0          # tie: torch.argmax returns the first
    x[2, 32000] = 99.0
    ids = B.argmax(x)
    assert ids.tolist() == torch.argmax(x, dim=-1).tolist()
    assert ids[1].item() == 777 and ids[2].item() == 32000


def test_rope_kv_append(B):
    """rotate-half RoPE on Q/K + cache append against the formula of hf:models/mistral/modeling_mistral.py:51-81."""
    Bn, S, Hq, Hkv, D, max_ctx = 2, 37, 32, 8, 128, 64
    qkv = _rand((Bn * S, (Hq + 2 * Hkv) * D), 1.0, 40).bfloat16()
    pos = (torch.arange(S, dtype=torch.int32).repeat(Bn) + 3).cuda()
    slot = torch.arange(S, dtype=torch.int32).repeat(Bn)
    slot[S + 30:] = -1                               # padded tail of the second row is not cached
    slot = slot.cuda()
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))
    fr = torch.arange(64, dtype=torch.float32).unsqueeze(-1) * inv
    cos, sin = fr.cos().cuda().contiguous(), fr.sin().cuda().contiguous()
    kc = torch.zeros(Bn, Hkv, max_ctx, D, device="cuda").bfloat16()
    vc = torch.zeros_like(kc)
    q = B.rope_kv(qkv, cos, sin, pos, slot, kc, vc, Bn, S, Hq, Hkv, D)
    x = bf16r(qkv).view(Bn * S, Hq + 2 * Hkv, D)
    c = torch.cat([cos, cos], -1)[pos.long()].unsqueeze(1)
    s_ = torch.cat([sin, sin], -1)[pos.long()].unsqueeze(1)
    rot = torch.cat([-x[..., D // 2:], x[..., :D // 2]], -1)
    ref = x * c + rot * s_
    check_close("rope q", q, ref[:, :Hq], BF16_MAX, BF16_L2)
    kref = torch.zeros(Bn, Hkv, max_ctx, D, device="cuda")
    vref = torch.zeros_like(kref)
    for b in range(Bn):
        n = S if b == 0 else 30
        kref[b, :, :n] = ref[b * S:b * S + n, Hq:Hq + Hkv].permute(1, 0, 2)
        vref[b, :, :n] = x[b * S:b * S + n, Hq + Hkv:].permute(1, 0, 2)
    check_close("rope k cache", kc, kref, BF16_MAX, BF16_L2)
    assert torch.equal(vc.float(), vref)


@pytest.mark.parametrize("ctx,nsplit,window", [(1, 4, 0), (77, 8, 0), (1500, 16, 0), (700, 8, 256), (2047, 16, 4096)])
def test_attention_decode(B, ctx, nsplit, window):
    Bn, Hq, Hkv, D, max_ctx = 2, 32, 8, 128, 2048
    q = _rand((Bn, Hq, D), 1.0, 41).bfloat16()
    kc = _rand((Bn, Hkv, max_ctx, D), 1.0, 42).bfloat16()
    vc = _rand((Bn, Hkv, max_ctx, D), 1.0, 43).bfloat16()
    lens = torch.tensor([ctx, max(1, ctx // 2)], dtype=torch.int32, device="cuda")
    out = B.attention_decode(q, kc, vc, lens, D ** -0.5, nsplit, window)
    for b in range(Bn):
        n = int(lens[b])
        lo = max(0, n - window) if window > 0 else 0
        ref = _ref_attention(q[b:b + 1].unsqueeze(1), kc[b:b + 1, :, lo:n].permute(0, 2, 1, 3), vc[b:b + 1, :, lo:n].permute(0, 2, 1, 3),
                             D ** -0.5, False, 0, 0, None)
        check_close(f"attention decode ctx{n} b{b}", out[b], ref[0, 0], BF16_MAX, BF16_L2)


@pytest.mark.parametrize("ctx,nsplit,window", [(1, 32, 0), (2, 4, 0), (77, 32, 0), (1500, 32, 0), (2047, 32, 4096), (700, 16, 256),
                                               (3000, 8, 0)])
def test_attention_decode_fused_equals_rope_plus_decode(B, ctx, nsplit, window):
    """the engine's one-launch decode attention (RoPE + append + split attention + in-launch combine) against the
    two-kernel path, twice in a row on the same ticket buffer (graph replays reuse it)."""
    Bn, Hq, Hkv, D, max_ctx = 2, 32, 8, 128, 3072
    kc = _rand((Bn, Hkv, max_ctx, D), 1.0, 50).bfloat16()
    vc = _rand((Bn, Hkv, max_ctx, D), 1.0, 51).bfloat16()
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))
    fr = torch.arange(max_ctx + 8, dtype=torch.float32).unsqueeze(-1) * inv
    cos, sin = fr.cos().cuda().contiguous(), fr.sin().cuda().contiguous()
    ticket = None
    for rep in range(2):
        slot = torch.tensor([ctx - 1 + rep, max(0, ctx // 2 - 1) + rep], dtype=torch.int32, device="cuda")
        pos = slot + 5
        qkv = _rand((Bn, (Hq + 2 * Hkv) * D), 1.0, 52 + rep).bfloat16()
        kc1, vc1 = kc.clone(), vc.clone()
        q = B.rope_kv(qkv, cos, sin, pos, slot, kc1, vc1, Bn, 1, Hq, Hkv, D)
        ref = B.attention_decode(q.view(Bn, Hq, D), kc1, vc1, slot + 1, D ** -0.5, 8, window)
        kc2, vc2 = kc.clone(), vc.clone()
        out, ticket = B.attention_decode_fused(qkv, kc2, vc2, cos, sin, pos, slot, Hq, D ** -0.5, nsplit, window, ticket)
        assert torch.equal(kc1, kc2) and torch.equal(vc1, vc2), "cache append differs"
        check_close(f"fused decode attention ctx{ctx} rep{rep}", out, ref.float(), 8e-3, 2e-3)
        assert int(ticket.abs().sum()) == 0, "ticket not reset by the last arriver"
        kc, vc = kc2, vc2


# (520, 1024, 8192): 12 tiles x 128 K-tiles -> 8 K-slices per tile; (700, 1300, 4160): 18 tiles x 65 K-tiles cut unevenly;
# (1, 32001, 512): workgroups that run two whole tiles each; (2048, 28672, 4096): 3 full rounds + a split half round;
# (2885, ...), (3291, 1100, 256), (5000, 300, 128): more than 8 row tiles -> grouped tile order with a short last group (4, 5, 4 rows)
GEMM256_SHAPES = [(2048, 6144, 4096), (2048, 4096, 14336), (2885, 4096, 1024), (300, 520, 128), (256, 256, 64), (257, 255, 192),
                  (1, 32001, 512), (2048, 28672, 4096), (2048, 4096, 4096), (520, 1024, 8192), (700, 1300, 4160),
                  (3291, 1100, 256), (5000, 300, 128)]


def _whole_k(B, fn):
    """the 128^2 kernel with every tile summing its whole K in one workgroup (knob 26 = 0: no K slices for small grids), the
    order the 256^2 kernel's whole tiles reproduce bit for bit"""
    with B.tuned(splitk_mid=0):
        return fn()


@pytest.mark.parametrize("M,N,K", GEMM256_SHAPES)
def test_gemm256_matches_gemm128(B, M, N, K):
    """The 256x256 kernel accumulates K in the same order as the 128x128 kernel, so with whole tiles its fp32 outputs
    must be BIT-IDENTICAL.  Any LDS-DMA tile read before it landed (RAW) or overwritten too early (WAR) breaks
    equality, so the comparison is repeated under different machine states (back-to-back launches, other kernels in
    between).  With the stream-K tail a tile's K range is summed in slices (fp32 re-association, ~1e-7 relative):
    the result must agree to fp32 precision and must be bit-identical from launch to launch (fixed slice order,
    whoever arrives last)."""
    x = _rand((M, K), 1.0, 60).bfloat16()
    w = _rand((N, K), 0.05, 61).bfloat16()
    ref = _whole_k(B, lambda: B.linear(x, w, out_fp32=True, impl=0))
    check_close(f"gemm128 ref {M}x{N}x{K}", ref, _ref_linear(x, w, None, None, 0), 1e-4, 1e-4)
    scale = float(ref.abs().max())
    for streamk in (2, 1, 0):          # stream-K tail forced / production heuristic / whole tiles only
        with B.tuned(gemm256_streamk=streamk):
            first = None
            for rep in range(6):
                if rep % 2:
                    torch.randn(1 << 22, device="cuda").sum()      # perturb caches / clocks between launches
                out = B.linear(x, w, out_fp32=True, impl=2)
                if streamk == 0:
                    assert torch.equal(out, ref), (f"rep {rep}: {(out != ref).sum().item()} elements differ, "
                                                   f"max {float((out - ref).abs().max()):.3e}")
                else:
                    err = float((out - ref).abs().max())
                    assert err <= 1e-5 * scale, f"stream-K rep {rep}: max abs err {err:.3e} vs scale {scale:.3e}"
                    if first is None:
                        first = out.clone()
                    assert torch.equal(out, first), f"stream-K rep {rep}: result changed between launches"


@pytest.mark.parametrize("M,N,K", [(700, 1024, 1024), (520, 1024, 4096)])     # whole tiles / 4 K-slices per tile
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_gemm256_epilogues(B, act, M, N, K):
    x = _rand((M, K), 1.0, 62).bfloat16()
    w = _rand((N, K), 0.05, 63).bfloat16()
    bias = None if act == 3 else _rand((N,), 0.5, 64)
    n_out = N // 2 if act == 3 else N
    res = _rand((M, n_out), 1.0, 65).bfloat16()
    with B.tuned(gemm256_streamk=2):          # stream-K tail forced
        out = B.linear(x, w, bias=bias, residual=res, act=act, impl=2)
    ref128 = _whole_k(B, lambda: B.linear(x, w, bias=bias, residual=res, act=act, impl=0))
    check_close(f"gemm256 epilogue act{act}", out, _ref_linear(x, w, bias, res, act), BF16_MAX, BF16_L2)
    # stream-K re-associates the fp32 sum: a handful of outputs may round to the neighbouring bf16 value
    assert float((out.float() - ref128.float()).abs().max()) <= 2 ** -7 * float(ref128.float().abs().max())
    with B.tuned(gemm256_streamk=0):
        assert torch.equal(B.linear(x, w, bias=bias, residual=res, act=act, impl=2), ref128)


def test_gemm256_identity_asymmetric(B):
    K = 256
    x = torch.eye(K, device="cuda").bfloat16()
    w = (torch.arange(384 * K, device="cuda").view(384, K) % 251 - 125).float().bfloat16()
    out = B.linear(x, w, out_fp32=True, impl=2)
    assert torch.equal(out, w.float().t().contiguous())


@pytest.mark.parametrize("case", [c for c in ATTN_CASES if c[6] in (64, 128)], ids=[c[0] for c in ATTN_CASES if c[6] in (64, 128)])
def test_attention_v2_matches_v1(B, case):
    """v2 / v3 (32 rows per wave, K and V by LDS-DMA into XOR-swizzled double buffers, hardware-transposed V reads, exp2-based softmax,
    mask-free fast path; v3 = the production deferred-maximum softmax step) against
    v1 (transposed LDS writes, expf).  v2 advances the running maximum every 32 keys instead of 64, so the bf16 rounding of
    the probabilities is taken against a different reference maximum: the two outputs are two independent bf16 roundings
    of the same attention (each within one bf16 step of the fp64 reference, checked in test_attention)."""
    name, Bn, Sq, Sk, Hq, Hkv, D, causal, q_pos0, window, ragged = case
    q = _rand((Bn, Sq, Hq, D), 1.0, 70).bfloat16()
    k = _rand((Bn, Sk, Hkv, D), 1.0, 71).bfloat16()
    v = _rand((Bn, Sk, Hkv, D), 1.0, 72).bfloat16()
    kv_len = torch.tensor([Sk, Sk // 2 + 3][:Bn], dtype=torch.int32, device="cuda") if ragged else None
    with B.tuned(attn_version=1):
        o1 = B.attention(q, k, v, D ** -0.5, causal, q_pos0, window, kv_len)
    with B.tuned(attn_version=2):
        o2 = B.attention(q, k, v, D ** -0.5, causal, q_pos0, window, kv_len)      # classic online-softmax step
    o3 = B.attention(q, k, v, D ** -0.5, causal, q_pos0, window, kv_len)          # production: deferred-maximum step
    if ragged:
        for b in range(Bn):
            o1[b, int(kv_len[b]):] = 0
            o2[b, int(kv_len[b]):] = 0
            o3[b, int(kv_len[b]):] = 0
    check_close(f"attention v2 vs v1 {name}", o2, o1.float(), 8e-3, 2.5e-3)
    # v3 rounds its probabilities against a DEFERRED reference maximum (up to 2^8 above one): the bf16 mantissas it rounds are not the
    # ones v1 rounds, so the two roundings are independent and the distance between the two outputs is ~sqrt(2) x one implementation's
    # distance from the exact attention (each is within one bf16 step of the fp64 reference: test_attention runs the production kernel)
    check_close(f"attention v3 vs v1 {name}", o3, o1.float(), 1e-2, 3.6e-3)


@pytest.mark.parametrize("M,N,K,act", [(160, 4096, 4096, 0), (160, 8192, 4096, 2), (32, 12288, 4096, 0), (4, 4096, 14336, 0), (512, 4096, 8192, 0)])
def test_gemm_splitk_small_m(B, M, N, K, act):
    """Q-Former-shaped products (few row tiles, long K) run split-K: slices of K per tile, fp32 slabs, one finalize pass."""
    x = _rand((M, K), 1.0, 80).bfloat16()
    w = _rand((N, K), 0.03, 81).bfloat16()
    bias = _rand((N,), 0.3, 82)
    res = _rand((M, N), 1.0, 83).bfloat16()
    out = B.linear(x, w, bias=bias, residual=res, act=act, impl=0)
    check_close(f"gemm split-K {M}x{N}x{K}", out, _ref_linear(x, w, bias, res, act), BF16_MAX, BF16_L2)
    with B.tuned(splitk_mode=1):
        plain = B.linear(x, w, bias=bias, residual=res, act=act, impl=0)
    check_close(f"gemm split-K vs single pass {M}x{N}x{K}", out, plain.float(), 8e-3, 5e-4)
    o32 = B.linear(x, w, out_fp32=True, impl=0)
    check_close(f"gemm split-K fp32 {M}x{N}x{K}", o32, _ref_linear(x, w, None, None, 0), 1e-4, 1e-4)


# ---- W8A16 weight stream (SURVEY config 5): e4m3 rows + one power-of-two scale per row ----
@pytest.mark.parametrize("M,N,K,act", [(1, 6144, 4096, 0), (1, 4096, 14336, 0), (1, 28672, 4096, 3), (2, 4096, 4096, 0),
                                       (4, 1024, 4096, 0), (8, 2048, 2048, 3), (1, 32001, 4096, 0), (3, 257, 1024, 0),
                                       (16, 28672, 4096, 3), (11, 4096, 14336, 0)])
def test_gemv_fp8_weights(B, M, N, K, act):
    """The fp8 GEMV must equal the dot product with the DEQUANTISED weights (2^e * e4m3, exact in bf16) to fp32
    accumulation accuracy, through every epilogue; and the dequantised bf16 weights through the bf16 GEMV must give the
    same result (prefill and decode run one model)."""
    from vz_hip import quant
    x = _rand((M, K), 1.0, 90).bfloat16()
    w = _rand((N, K), 0.03, 91)
    w[5] *= 37.0                                   # rows of very different magnitude: per-row scales matter
    w[7] = 0.0                                     # an all-zero row quantises to scale 1, bytes 0
    w8, scale = quant.quantize_rows(w)
    wq = quant.dequantize_rows(w8, scale)
    assert torch.equal(wq.bfloat16().float(), wq)  # exactly representable in bf16
    assert float((wq - w).abs().max() / w.abs().max()) < 0.07
    n_out = N // 2 if act == 3 else N
    res = _rand((M, n_out), 1.0, 92).bfloat16()
    bias = None if act == 3 else _rand((N,), 0.3, 93)
    for mode in (1, 0):          # 2..16 rows: MFMA weight stream (gemm_skinny.hip) / the GEMV form (M <= 8); 1 row: always the GEMV
        if mode == 0 and M > 8:
            continue
        with B.tuned(skinny_mode=mode):
            out32 = B.linear_fp8(x, w8, scale, act=act, out_fp32=True)
            out = B.linear_fp8(x, w8, scale, bias=bias, residual=res, act=act)
        check_close(f"fp8 fp32 {M}x{N}x{K} act{act} mode{mode}", out32, _ref_linear(x, wq, None, None, act), 1e-4, 1e-4)
        check_close(f"fp8 {M}x{N}x{K} act{act} mode{mode}", out, _ref_linear(x, wq, bias, res, act), BF16_MAX, BF16_L2)
    same = B.linear(x, wq.bfloat16(), bias=bias, residual=res, act=act, impl=1 if M <= 8 else 3)
    # identical products and the same fp32 accumulation order per lane would make these bit-equal; the lane -> k mapping
    # differs (16 vs 8 weights per lane), so allow fp32 re-association: at most one bf16 step on a handful of outputs
    assert float((out.float() - same.float()).abs().max()) <= 2 ** -7 * float(same.float().abs().max()) + 1e-6


@pytest.mark.parametrize("M", [2, 4, 7])          # 4, 7: one wave per activation row in the staging prologue
def test_gemv_fp8_fused_rmsnorm(B, M):
    from vz_hip import quant
    K, N = 4096, 6144
    x = _rand((M, K), 3.0, 94).bfloat16()
    nw = _rand((K,), 0.2, 95) + 1.0
    w8, scale = quant.quantize_rows(_rand((N, K), 0.02, 96))
    wq = quant.dequantize_rows(w8, scale)
    xf = bf16r(x).double()
    xn = (nw.double() * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5))).float().bfloat16()
    out = B.linear_fp8(x, w8, scale, out_fp32=True, norm_w=nw, norm_eps=1e-5)
    ref = _ref_linear(xn, wq, None, None, 0)
    # the fused norm rounds x to bf16 like the stand-alone kernel; a different rounding of a few x entries moves the
    # sum by ~2^-9 relative
    check_close("gemv fp8 fused rmsnorm", out, ref, 2e-2, 3e-3)


def test_gemv_fp8_rejects_bad_arguments(B):
    from vz_hip import quant
    w8, scale = quant.quantize_rows(_rand((64, 1536), 0.02, 97))
    with pytest.raises(ValueError):
        B.linear_fp8(_rand((1, 1536), 1.0, 98).bfloat16(), w8, scale)        # K not a multiple of 1024
    w8, scale = quant.quantize_rows(_rand((64, 2048), 0.02, 97))
    with pytest.raises(ValueError):
        B.linear_fp8(_rand((65, 2048), 1.0, 98).bfloat16(), w8, scale)       # M > 64: the fp8 stream serves decode batches only


# ---- MFMA weight stream for 2..16 activation rows (batched decode; gemm_skinny.hip) ----
@pytest.mark.parametrize("M,N,K,act", [(2, 6144, 4096, 0), (4, 4096, 14336, 0), (4, 28672, 4096, 3), (8, 4096, 4096, 0), (16, 6144, 4096, 0),
                                       (16, 2048, 14336, 0), (3, 32001, 4096, 0), (5, 257, 1024, 0), (7, 64, 512, 3), (16, 1024, 576, 0)])
def test_skinny_gemm(B, M, N, K, act):
    """one 16x16x32 MFMA per KiB of weights for all rows: results must match the fp64 reference like the GEMV does (fp32
    accumulation, one bf16 rounding), through bias / activation / SwiGLU / residual / fp32 output, ragged N included."""
    x = _rand((M, K), 1.0, 100).bfloat16()
    w = _rand((N, K), 0.03, 101).bfloat16()
    n_out = N // 2 if act == 3 else N
    res = _rand((M, n_out), 1.0, 102).bfloat16()
    bias = None if act == 3 else _rand((N,), 0.3, 103)
    out = B.linear(x, w, bias=bias, residual=res, act=act, impl=3)
    check_close(f"skinny {M}x{N}x{K} act{act}", out, _ref_linear(x, w, bias, res, act), BF16_MAX, BF16_L2)
    out32 = B.linear(x, w, act=act, out_fp32=True, impl=3)
    check_close(f"skinny fp32 {M}x{N}x{K} act{act}", out32, _ref_linear(x, w, None, None, act), 1e-4, 1e-4)
    # rows are independent: every row equals what it gets in a 2-row launch (batch invariance of the decode path)
    pair = B.linear(x[:2].contiguous(), w, act=act, out_fp32=True, impl=3)
    assert torch.equal(pair, out32[:2])
    # the production dispatch takes this path for 3..16 rows; 2 rows go to the GEMV (both rows in LDS: it streams like a 1-row launch)
    prod = B.linear(x, w, act=act, out_fp32=True)
    if M == 2:
        check_close(f"2-row GEMV vs MFMA stream {N}x{K} act{act}", prod, out32, 1e-4, 1e-4)
    else:
        assert torch.equal(prod, out32)


@pytest.mark.parametrize("M,act", [(2, 0), (4, 3), (9, 0), (16, 3)])
def test_skinny_gemm_fused_rmsnorm(B, M, act):
    K, N = 4096, 6144
    x = _rand((M, K), 3.0, 104).bfloat16()
    nw = _rand((K,), 0.2, 105) + 1.0
    w = _rand((N, K), 0.02, 106).bfloat16()
    xf = bf16r(x).double()
    xn = (nw.double() * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5))).float().bfloat16()
    out = B.linear_rmsnorm(x, nw, 1e-5, w, act=act, out_fp32=True)
    check_close(f"skinny fused rmsnorm M{M} act{act}", out, _ref_linear(xn, w, None, None, act), 2e-2, 3e-3)
    # exactly the stand-alone norm kernel followed by the same GEMM (2 rows: the production dispatch is the GEMV with its own fused norm)
    unfused = B.linear(B.rmsnorm(x, nw, 1e-5), w, act=act, out_fp32=True, impl=3)
    if M == 2:
        check_close("2-row GEMV fused norm vs norm + MFMA stream", out, unfused, 1e-4, 1e-4)
    else:
        assert torch.equal(out, unfused)
    # and, with the knob off, the GEMV path fuses the norm the same way (M <= 8)
    if M <= 8:
        with B.tuned(skinny_mode=0):
            gv = B.linear_rmsnorm(x, nw, 1e-5, w, act=act, out_fp32=True)
        check_close(f"gemv vs skinny fused norm M{M}", gv, out, 1e-4, 1e-4)


@pytest.mark.parametrize("M,N,K,act", [(17, 6144, 4096, 0), (32, 4096, 14336, 0), (32, 28672, 4096, 3), (25, 4000, 1024, 1), (32, 32001, 4096, 0),
                                       (33, 6144, 4096, 0), (64, 4096, 14336, 0), (64, 28672, 4096, 3), (50, 4000, 1024, 2), (64, 32001, 4096, 0)])
def test_skinny_wide_rows(B, M, N, K, act):
    """17..64 rows: the weight fragment meets two / four B operands (rows 16h .. 16h+15).  Against the fp64 reference, rows 0..15
    bit-identical to the 16-row kernel on the same rows where both run 8 waves per group, with bias + residual, ragged N, and
    the e4m3 weight stream."""
    x = _rand((M, K), 1.0, 301).bfloat16()
    w = _rand((N, K), 0.03, 302).bfloat16()
    n_out = N // 2 if act == 3 else N
    bias = None if act == 3 else _rand((N,), 0.1, 303)
    res = _rand((M, n_out), 0.5, 304).bfloat16()
    out = B.linear(x, w, bias=bias, residual=res, act=act, out_fp32=True)
    check_close(f"skinny wide M{M} N{N} K{K} act{act}", out, _ref_linear(x, w, bias, res, act), 1e-4, 1e-4)
    groups = N // 32 if act == 3 else (N + 15) // 16
    head = B.linear(x[:16].contiguous(), w, bias=bias, residual=res[:16].contiguous(), act=act, out_fp32=True)
    if groups < 512 or (K >> 6) < 16:
        assert torch.equal(out[:16], head), "rows 0..15 differ from the 16-row kernel"
    else:
        check_close("wide vs 16-row kernel (4-wave groups)", out[:16], head, 1e-5, 1e-5)
    for rep in range(2):
        assert torch.equal(B.linear(x, w, bias=bias, residual=res, act=act, out_fp32=True), out)
    if K % 1024 == 0 and (act != 3 or N % 64 == 0):
        from vz_hip import quant
        w8, ws = quant.quantize_rows(w)
        wq = quant.dequantize_rows(w8, ws).bfloat16()
        o8 = B.linear_fp8(x, w8, ws, bias=bias, residual=res, act=act, out_fp32=True)
        check_close(f"skinny wide fp8 M{M} N{N}", o8, B.linear(x, wq, bias=bias, residual=res, act=act, out_fp32=True), 1e-4, 1e-4)


@pytest.mark.parametrize("M,N,act", [(5, 6144, 0), (16, 6144, 3), (16, 28672, 3), (9, 32001, 0), (12, 4000, 1), (16, 48, 0)])
def test_skinny_persistent_fused_norm(B, M, N, act):
    """5..16 rows with the RMSNorm fused: ONE workgroup per CU stages the normalised rows in LDS once and walks its row groups
    (weight prefetch running across group boundaries).  Same K-slices and slice order as the one-group-per-workgroup kernel
    (knob 9 = 2 routes the same call there): bit-identical where that kernel also runs 8 waves per group (< 512 groups),
    fp32-close beyond (4-wave groups there); ragged N (lm_head 32001), fewer groups than CUs (48), fp8 rows."""
    K = 4096
    x = _rand((M, K), 3.0, 204).bfloat16()
    nw = _rand((K,), 0.2, 205) + 1.0
    w = _rand((N, K), 0.02, 206).bfloat16()
    xf = bf16r(x).double()
    xn = (nw.double() * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5))).float().bfloat16()
    groups = N // 32 if act == 3 else (N + 15) // 16
    for rep in range(3):
        out = B.linear_rmsnorm(x, nw, 1e-5, w, act=act, out_fp32=True)
        if rep == 0:
            first = out.clone()
            check_close(f"persistent skinny M{M} N{N} act{act}", out, _ref_linear(xn, w, None, None, act), 2e-2, 3e-3)
        assert torch.equal(out, first), "result changed between launches"
        torch.randn(1 << 21, device="cuda").sum()
    with B.tuned(skinny_mode=2):
        old = B.linear_rmsnorm(x, nw, 1e-5, w, act=act, out_fp32=True)
    if groups < 512:
        assert torch.equal(old, first), f"{(old != first).sum().item()} elements differ from the one-group-per-workgroup kernel"
    else:
        check_close(f"persistent vs 4-wave groups M{M} N{N}", first, old, 1e-4, 1e-4)
    if act != 3 or N % 64 == 0:
        from vz_hip import quant
        w8, ws = quant.quantize_rows(w)
        wq = quant.dequantize_rows(w8, ws).bfloat16()
        o8 = B.linear_fp8(x, w8, ws, act=act, out_fp32=True, norm_w=nw, norm_eps=1e-5)         # e4m3 rows widened in registers (exact)
        check_close(f"persistent skinny fp8 M{M} N{N}", o8, B.linear_rmsnorm(x, nw, 1e-5, wq, act=act, out_fp32=True), 1e-4, 1e-4)


# ---- seeded shape fuzz through the PRODUCTION dispatch: every kernel family must agree with the fp64 reference at shapes
# ---- nobody tuned for (ragged M / N, odd tile counts, grids that do not divide the CU count, every epilogue) ----
def _fuzz_linear_cases(n=28, seed=1234):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))      # noqa: E731
    cases = []
    for i in range(n):
        kind = i % 4
        if kind == 0:
            M = ri(1, 16)                                   # weight-stream kernels
            K = 512 * ri(1, 12)
        elif kind == 1:
            M = ri(17, 600)                                 # small tile grids, split-K
            K = 64 * ri(1, 96)
        else:
            M = ri(600, 3100)                               # 128^2 / 256^2 tile GEMMs, stream-K tails
            K = 64 * ri(4, 80)
        act = ri(0, 3)
        N = (32 * ri(1, 280)) if act == 3 else ri(16, 9000)
        if act == 3 and M <= 8:
            N = 64 * ri(1, 140)
        cases.append((M, N, K, act, bool(ri(0, 1)), bool(ri(0, 1)), bool(ri(0, 3) == 0)))
    return cases


@pytest.mark.parametrize("M,N,K,act,use_bias,use_res,fp32", _fuzz_linear_cases())
def test_linear_dispatch_shape_fuzz(B, M, N, K, act, use_bias, use_res, fp32):
    x = _rand((M, K), 1.0, M + N).bfloat16()
    w = _rand((N, K), 0.04, N + K).bfloat16()
    n_out = N // 2 if act == 3 else N
    bias = _rand((N,), 0.3, 7) if (use_bias and act != 3) else None
    res = _rand((M, n_out), 1.0, 8).bfloat16() if use_res else None
    out = B.linear(x, w, bias=bias, residual=res, act=act, out_fp32=fp32)
    ref = _ref_linear(x, w, bias, res, act)
    if fp32:
        check_close(f"fuzz linear {M}x{N}x{K} act{act} fp32", out, ref, 2e-4, 1e-4)
    else:
        check_close(f"fuzz linear {M}x{N}x{K} act{act}", out, ref, BF16_MAX, BF16_L2)


def _fuzz_attention_cases(n=14, seed=4321):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))      # noqa: E731
    cases = []
    for i in range(n):
        D = (64, 128)[i % 2]
        Hkv = (1, 2, 4, 8)[ri(0, 3)]
        Hq = Hkv * (1 if D == 64 else (1, 4)[ri(0, 1)])
        Bn = ri(1, 3)
        Sq = ri(1, 1700 if Bn == 1 else 600)
        causal = D == 128 or bool(ri(0, 1))
        q_pos0 = 0
        Sk = Sq if causal else ri(1, 900)
        window = (0, 4096, ri(16, 300))[ri(0, 2)] if causal else 0
        cases.append((f"fuzz{i}", Bn, Sq, Sk, Hq, Hkv, D, causal, q_pos0, window, Bn > 1 and bool(ri(0, 1))))
    return cases


@pytest.mark.parametrize("case", _fuzz_attention_cases(), ids=lambda c: f"{c[0]}-B{c[1]}-Sq{c[2]}-Sk{c[3]}-H{c[4]}/{c[5]}-D{c[6]}-c{int(c[7])}-w{c[9]}")
def test_attention_shape_fuzz(B, case):
    test_attention(B, case)


# ---------------------------------------------------------------------------------------------------------------------
# stream-K state is per (device, stream); an expired fix-up wait raises the async error word and poisons its tile
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,act", [(8192, 4096, 512, 0), (2048, 28672, 1024, 3), (5000, 6144, 768, 1), (12736, 4096, 256, 0)])
def test_gemm256_persistent_tiles_equal_one_workgroup_per_tile(B, M, N, K, act):
    """Round 3: with more whole tiles than CUs, 256 workgroups walk the tiles (tile b, b + 256, ...) instead of one workgroup each
    (gemm256.hip::plan_and_launch, knob 34 (gemm256_persist) = 0 = off).  Same tile arithmetic, same stream-K tail: bit-identical outputs - with bias,
    residual and the fused activations, a partial last row tile (M = 5000) and a stream-K remainder (896 tiles = 3.5 rounds)."""
    x = _rand((M, K), 1.0, 310).bfloat16()
    w = _rand((N, K), 0.03, 311).bfloat16()
    n_out = N // 2 if act == 3 else N
    bias = _rand((N,), 0.3, 312) if act != 3 else None
    res = _rand((M, n_out), 1.0, 313).bfloat16()
    outs = []
    for knob in (1, 0):
        with B.tuned(gemm256_persist=knob):
            outs.append(B.linear(x, w, bias=bias, residual=res, act=act, impl=2))
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0], outs[1])
    ref = x.float() @ w.float().t()
    if act == 3:
        r = ref.view(M, -1, 2, 16)
        ref = (torch.nn.functional.silu(r[:, :, 0]) * r[:, :, 1]).reshape(M, n_out)
    else:
        ref = ref + bias
        if act == 1:
            ref = ref * torch.sigmoid(1.702 * ref)
    ref = ref + res.float()
    check_close(f"persistent gemm256 {M}x{N}x{K}", outs[0], ref, 2e-2, 6e-3)


def test_gemm256_streamk_two_streams_do_not_share_tickets(B):
    """Round 1 kept ONE process-wide set of stream-K slots / tickets: two streams (or two engines) running stream-K GEMMs at the
    same time met on it.  Now every (device, stream) has its own: interleaved launches on two streams give the results of
    the same launches run alone."""
    M, N, K = 640, 1100, 4096           # 3 x 5 = 15 tiles on 256 CUs: the whole launch is a stream-K tail when forced
    x1, w1 = _rand((M, K), 1.0, 70).bfloat16(), _rand((N, K), 0.05, 71).bfloat16()
    x2, w2 = _rand((M, K), 1.0, 72).bfloat16(), _rand((N, K), 0.05, 73).bfloat16()
    with B.tuned(gemm256_streamk=2):
        alone1 = B.linear(x1, w1, out_fp32=True, impl=2)
        alone2 = B.linear(x2, w2, out_fp32=True, impl=2)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs1, outs2 = [], []
        for _ in range(8):
            with torch.cuda.stream(s1):
                outs1.append(B.linear(x1, w1, out_fp32=True, impl=2))
            with torch.cuda.stream(s2):
                outs2.append(B.linear(x2, w2, out_fp32=True, impl=2))
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            assert B.op_async_error() == 0
        with torch.cuda.stream(s2):
            assert B.op_async_error() == 0
    for o in outs1:
        assert torch.equal(o, alone1)
    for o in outs2:
        assert torch.equal(o, alone2)


def test_gemm256_streamk_expired_wait_raises_and_poisons(B):
    """Tickets that no launch can complete from (here: `ready` preset beyond the slice count of remainder tile 0): the finisher's
    bounded wait expires -> the launch ENDS, the async error word reads VZ_ASYNC_STREAMK, that tile is NaN (never a sum of
    stale slots), every other tile is right; reading the error resets the tickets and the next launch is clean."""
    M, N, K = 640, 1100, 4096
    x, w = _rand((M, K), 1.0, 74).bfloat16(), _rand((N, K), 0.05, 75).bfloat16()
    with B.tuned(gemm256_streamk=2):
        good = B.linear(x, w, out_fp32=True, impl=2)
        assert B.op_async_error() == 0
        B.check(B.lib().vz_test_corrupt_streamk(B.stream_ptr(), 0, 0, 100))
        bad = B.linear(x, w, out_fp32=True, impl=2)
        torch.cuda.synchronize()
        assert B.op_async_error() == B.VZ_ASYNC_STREAMK
        nan = torch.isnan(bad)
        assert nan.any() and int(nan.sum()) <= 256 * 256, int(nan.sum())
        assert torch.equal(bad[~nan], good[~nan])
        assert B.op_async_error() == 0                      # cleared, tickets reset
        again = B.linear(x, w, out_fp32=True, impl=2)
        assert torch.equal(again, good) and B.op_async_error() == 0


@pytest.mark.parametrize("M,N,K,act", [(33, 6144, 4096, 0), (64, 4096, 4096, 0), (48, 4096, 14336, 0), (64, 28672, 4096, 3), (40, 3584, 4096, 3),
                                       (64, 32000, 4096, 0)])
def test_decode_tile_route_splitk(B, M, N, K, act):
    """33..64-row decode steps run their linears on the 128^2 tile GEMM with a finer split-K (impl 4): QKV / O x8, down x16, gate|up x2
    with the SwiGLU pairs formed by the finalize kernel.  Against the fp64 reference and the un-split tile GEMM, with residual."""
    x = _rand((M, K), 1.0, 401).bfloat16()
    w = _rand((N, K), 0.03, 402).bfloat16()
    n_out = N // 2 if act == 3 else N
    res = _rand((M, n_out), 0.5, 403).bfloat16()
    out = B.linear(x, w, residual=res, act=act, out_fp32=True, impl=4)
    check_close(f"decode tile route M{M} N{N} K{K} act{act}", out, _ref_linear(x, w, None, res, act), 1e-4, 1e-4)
    check_close("vs whole-K tile GEMM", out, B.linear(x, w, residual=res, act=act, out_fp32=True, impl=0), 2e-5, 2e-5)
    o16 = B.linear(x, w, residual=res, act=act, impl=4)
    check_close("bf16 out", o16, _ref_linear(x, w, None, res, act), BF16_MAX, BF16_L2)
    assert torch.equal(B.linear(x, w, residual=res, act=act, out_fp32=True, impl=4), out)


@pytest.mark.parametrize("M,N,K,act,norm", [(2, 6144, 4096, 0, True), (3, 4096, 4096, 0, False), (7, 28672, 4096, 3, True), (16, 4096, 14336, 0, False),
                                            (16, 28672, 4096, 3, True), (24, 6144, 4096, 0, False), (40, 28672, 4096, 3, False), (64, 4096, 14336, 0, False)])
def test_skinny_tiled_weights_bit_identical(B, M, N, K, act, norm):
    """the fragment-tiled copy of a weight (vz_op_tile_weights) holds the same values in the order the MFMA weight stream consumes them:
    the layout equals its definition (include/viszephyr.h), and a launch on it equals the row-major launch bit for bit - fused RMSNorm,
    SwiGLU pairs, residual, 2..64 rows (two and four B operands per fragment)."""
    x = _rand((M, K), 1.0, 90).bfloat16()
    w = (_rand((N, K), 1.0, 91) * K ** -0.5).bfloat16()
    wt = B.tile_weights(w)
    ref_t = w.view(N // 16, 16, K // 64, 4, 2, 8).permute(0, 2, 4, 3, 1, 5).contiguous().view(-1)      # (G, r, s, g, j, e) -> (G, s, j, g, r, e)
    assert torch.equal(wt, ref_t)
    n_out = N // 2 if act == 3 else N
    res = _rand((M, n_out), 1.0, 92).bfloat16()
    nw = (_rand((K,), 0.2, 93) + 1.0) if norm and M <= 16 else None
    with B.tuned(wide_mode=0):          # 17..64 rows: keep linear_tiled on the MFMA weight stream (not gemm_wide.hip)
        if nw is not None and M > 2:
            a = B.linear_rmsnorm(x, nw, 1e-5, w, residual=res, act=act)
            b = B.linear_tiled(x, w, wt, residual=res, act=act, norm_w=nw, norm_eps=1e-5)
        else:                                        # (2 rows with a fused norm: the production dispatch is the GEMV)
            a = B.linear(x, w, residual=res, act=act, impl=3)
            b = B.linear_tiled(x, w, wt, residual=res, act=act)
    assert torch.equal(a, b), f"max diff {float((a.float() - b.float()).abs().max()):.3e}"


@pytest.mark.parametrize("M,N,K,act", [(17, 4096, 4096, 0), (32, 6144, 4096, 0), (24, 28672, 4096, 3), (32, 4096, 14336, 0), (33, 4096, 4096, 1),
                                       (64, 6144, 4096, 0), (64, 28672, 4096, 3), (50, 4096, 14336, 0), (64, 32000, 4096, 0), (48, 3584, 4096, 3)])
def test_wide_tiled_gemm(B, M, N, K, act):
    """gemm_wide.hip (17..64-row decode steps): eight row groups per workgroup on the tiled weight copy, the activations of a 512-k chunk
    staged once in LDS, K splits (P = 8 / 4 / 1 / 7 for these shapes) combined by the last arriver.  Against the fp64 reference through
    bias / activation / SwiGLU / residual, bf16 and fp32 outputs; the split-K sum is in split order: two launches agree bit for bit,
    and rows do not depend on the rows beside them (same row-block count class: 17..32 or 33..64)."""
    x = _rand((M, K), 1.0, 401).bfloat16()
    w = (_rand((N, K), 1.0, 402) * K ** -0.5).bfloat16()
    wt = B.tile_weights(w)
    n_out = N // 2 if act == 3 else N
    bias = None if act == 3 else _rand((N,), 0.1, 403)
    res = _rand((M, n_out), 0.5, 404).bfloat16()
    out32 = B.linear_tiled(x, w, wt, bias=bias, residual=res, act=act, out_fp32=True)
    check_close(f"wide tiled fp32 M{M} N{N} K{K} act{act}", out32, _ref_linear(x, w, bias, res, act), 1e-4, 1e-4)
    out = B.linear_tiled(x, w, wt, bias=bias, residual=res, act=act)
    check_close(f"wide tiled bf16 M{M} N{N} K{K} act{act}", out, _ref_linear(x, w, bias, res, act), BF16_MAX, BF16_L2)
    for _ in range(3):
        assert torch.equal(B.linear_tiled(x, w, wt, bias=bias, residual=res, act=act, out_fp32=True), out32)
    lo = 17 if M <= 32 else 33
    head = B.linear_tiled(x[:lo].contiguous(), w, wt, bias=bias, residual=res[:lo].contiguous(), act=act, out_fp32=True)
    assert torch.equal(head, out32[:lo])


@pytest.mark.parametrize("M,N,K,act", [(64, 4096, 4096, 0), (24, 6144, 4096, 0), (64, 28672, 4096, 3), (33, 28672, 4096, 3), (64, 4096, 14336, 0),
                                       (17, 4096, 14336, 0), (64, 32000, 4096, 0), (40, 1024, 2048, 1)])
def test_wide_tiled_gemm_fp8(B, M, N, K, act):
    """gemm_wide.hip's W8A16 stream (17..64-row decode steps of the e4m3-weight engine, round 3): the e4m3 fragment-tiled copy, widened to
    bf16 in registers (exact), the row's 2^e on the finished sums - against the fp64 product with the DEQUANTISED weights (the
    quantisation is exact data, so only fp32 accumulation and the output rounding remain), through bias / activation / SwiGLU / residual,
    bf16 and fp32 outputs; K splits combined in split order: launches agree bit for bit; rows do not depend on the rows beside them; the
    tiled copy holds exactly the row-major bytes (checked through the layout formula of include/viszephyr.h)."""
    from vz_hip import quant
    x = _rand((M, K), 1.0, 421).bfloat16()
    w = (_rand((N, K), 1.0, 422) * K ** -0.5).bfloat16()
    w8, ws = quant.quantize_rows(w)
    wq = quant.dequantize_rows(w8, ws).bfloat16()
    w8t = B.tile_weights_fp8(w8)
    # layout: W8t[((G * S + s) * 64 + 16 g + r) * 16 + i] = W8[16 G + r][64 s + 16 g + i]
    S = K // 64
    back = w8t.view(N // 16, S, 4, 16, 16).permute(0, 3, 1, 2, 4).reshape(N, K)      # [G, s, g, r, i] -> [G, r, s, g, i]
    assert torch.equal(back, w8)
    n_out = N // 2 if act == 3 else N
    bias = None if act == 3 else _rand((N,), 0.1, 423)
    res = _rand((M, n_out), 0.5, 424).bfloat16()
    out32 = B.linear_tiled_fp8(x, w8t, ws, N, bias=bias, residual=res, act=act, out_fp32=True)
    check_close(f"wide tiled fp8 fp32 M{M} N{N} K{K} act{act}", out32, _ref_linear(x, wq, bias, res, act), 1e-4, 1e-4)
    out = B.linear_tiled_fp8(x, w8t, ws, N, bias=bias, residual=res, act=act)
    check_close(f"wide tiled fp8 bf16 M{M} N{N} K{K} act{act}", out, _ref_linear(x, wq, bias, res, act), BF16_MAX, BF16_L2)
    for _ in range(3):
        assert torch.equal(B.linear_tiled_fp8(x, w8t, ws, N, bias=bias, residual=res, act=act, out_fp32=True), out32)
    lo = 17 if M <= 32 else 33
    head = B.linear_tiled_fp8(x[:lo].contiguous(), w8t, ws, N, bias=bias, residual=res[:lo].contiguous(), act=act, out_fp32=True)
    assert torch.equal(head, out32[:lo])


def test_quant_rows_fp8_equals_host_quantiser(B):
    """the activation quantiser of the fp8 MFMA prefill = vz_hip.quant.quantize_rows (the weights' quantiser; the oracle's restatement is
    checked against the same function in tests/test_quant_cpu.py): scales and e4m3 bytes equal, exact powers of two and the 448 boundary included."""
    from vz_hip import quant
    x = _rand((37, 4096), 3.0, 501).bfloat16()
    x[0] = 0
    x[1, 5] = 448.0
    x[2, 7] = 449.0 * 4          # just past 1.75 * 2^k: the exponent steps up
    x[3] = (torch.arange(4096, device="cuda") % 7 - 3).float().bfloat16() * 2.0 ** -20
    x[4, 100] = 1.75 * 2.0 ** 3  # exactly on the boundary
    q, sc = B.quant_rows_fp8(x)
    q_ref, sc_ref = quant.quantize_rows(x)
    assert torch.equal(sc, sc_ref.to(sc.device))
    assert torch.equal(q, q_ref.to(q.device))
    # RMSNorm + quantiser in one launch = the two launches, byte for byte
    nw = _rand((4096,), 0.2, 502) + 1.0
    q2, sc2 = B.rmsnorm_quant_fp8(x, nw, 1e-5)
    q3, sc3 = B.quant_rows_fp8(B.rmsnorm(x, nw, 1e-5))
    assert torch.equal(sc2, sc3) and torch.equal(q2, q3)


@pytest.mark.parametrize("M,N,K,act", [(128, 4096, 4096, 0), (300, 6144, 4096, 0), (2048, 28672, 4096, 3), (257, 4096, 14336, 0), (64, 4000, 1024, 1),
                                       (2048, 4096, 14336, 0), (2048, 6144, 4096, 0)])
def test_linear_fp8_mfma(B, M, N, K, act):
    """e4m3 x e4m3 on the scaled-MFMA with per-row power-of-two scales: against the fp64 product of the DEQUANTISED operands (the
    quantisation is exact data here, so only fp32 accumulation and the output rounding remain), through SwiGLU / bias / activation /
    residual, bf16 and fp32 outputs, ragged M and N."""
    from vz_hip import quant
    x = _rand((M, K), 1.0, 510).bfloat16()
    w = (_rand((N, K), 1.0, 511) * K ** -0.5).bfloat16()
    x8, xs = B.quant_rows_fp8(x)
    w8, ws = quant.quantize_rows(w)
    xq = quant.dequantize_rows(x8, xs).bfloat16()       # exactly representable: 2^e * e4m3
    wq = quant.dequantize_rows(w8, ws).bfloat16()
    n_out = N // 2 if act == 3 else N
    bias = None if act == 3 else _rand((N,), 0.1, 512)
    res = _rand((M, n_out), 0.5, 513).bfloat16()
    ref = _ref_linear(xq, wq, bias, res, act)
    for choice, what in ((1, "two-stage 128^2 kernel"), (2, "256^2 pipeline (gemm256.hip's ring, stream-K tail included)")):
        with B.tuned(fp8_gemm_choice=choice):
            out32 = B.linear_fp8_mfma(x8, xs, w8.cuda(), ws.cuda(), bias=bias, residual=res, act=act, out_fp32=True)
            check_close(f"fp8 mfma fp32 M{M} N{N} K{K} act{act} {what}", out32, ref, 1e-4, 1e-4)
            out = B.linear_fp8_mfma(x8, xs, w8.cuda(), ws.cuda(), bias=bias, residual=res, act=act)
            check_close(f"fp8 mfma bf16 M{M} N{N} K{K} act{act} {what}", out, ref, BF16_MAX, BF16_L2)
    assert B.op_async_error() == 0
