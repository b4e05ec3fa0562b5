"""The float64 references of tests/train_ref.py against torch float64 autograd of the corresponding forward (<= 1e-12 relative), AdamW against
oracle/train_oracle.adamw_step (itself pinned to torch.optim.AdamW).  Keeps the yardstick of tests/test_train_ops_gpu.py independent of the
kernels it measures.  The second half asks the library's launchers to refuse what their kernels cannot take: a refusal comes before any
launch, so it needs no GPU and the addresses passed are never touched."""
import math

import pytest
import torch
import torch.nn.functional as F

import train_ref as R

REL = 1e-12


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("rows,H,Sq,Sk,causal,window,kv", [(12, 2, 3, 9, False, 0, None), (12, 2, 3, 9, True, 0, None), (30, 3, 5, 7, True, 2, [7, 3]),
                                                            (30, 3, 5, 7, True, 1, None), (20, 2, 5, 6, False, 0, [0, 9])])
def test_softmax_backward_is_autograd_of_masked_softmax(rows, H, Sq, Sk, causal, window, kv):
    kv_len = None if kv is None else torch.tensor(kv, dtype=torch.int32)
    vis = R.softmax_visible(rows, H, Sq, Sk, causal, window, kv_len)
    S = torch.randn(rows, Sk, generator=_g(1), dtype=torch.float64, requires_grad=True)
    dP = torch.randn(rows, Sk, generator=_g(2), dtype=torch.float64)
    scale = 0.37
    live = vis.any(1)
    z = (S * scale).masked_fill(~vis, -math.inf)
    P = torch.zeros(rows, Sk, dtype=torch.float64)
    P[live] = torch.softmax(z[live], dim=1)
    assert _rel(R.softmax_fwd(S.detach(), vis, scale), P.detach()) <= REL
    assert (R.softmax_fwd(S.detach(), vis, scale)[~vis] == 0).all() and (R.softmax_fwd(S.detach(), vis, scale)[~live] == 0).all()
    (dS,) = torch.autograd.grad(P, S, dP)
    dP_nan = torch.where(P.detach() != 0, dP, torch.full_like(dP, math.nan))            # the reference never reads dP where P == 0
    got = R.softmax_bwd(P.detach(), dP_nan, scale)
    assert torch.isfinite(got).all() and _rel(got, dS) <= REL


def test_softmax_visibility_by_hand():
    vis = R.softmax_visible(8, 1, 4, 4, True, 2, torch.tensor([4, 3], dtype=torch.int32))
    want = torch.tensor([[1, 0, 0, 0], [1, 1, 0, 0], [0, 1, 1, 0], [0, 0, 1, 1], [1, 0, 0, 0], [1, 1, 0, 0], [0, 1, 1, 0], [0, 0, 1, 0]], dtype=torch.bool)
    assert torch.equal(vis, want)


@pytest.mark.parametrize("rows,cols", [(5, 48), (3, 1000)])
@pytest.mark.parametrize("with_res", [False, True])
def test_rmsnorm_backward_is_autograd_of_mistral_rmsnorm(rows, cols, with_res):
    x = (torch.randn(rows, cols, generator=_g(3), dtype=torch.float64) + 3.0).requires_grad_()
    w = torch.randn(cols, generator=_g(4), dtype=torch.float64)
    dy = torch.randn(rows, cols, generator=_g(5), dtype=torch.float64)
    dres = torch.randn(rows, cols, generator=_g(6), dtype=torch.float64) if with_res else None
    eps = 1e-5
    # MistralRMSNorm.forward: variance = x.pow(2).mean(-1, keepdim=True); x * rsqrt(variance + eps); weight * x   (+ the residual stream x itself)
    y = w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))
    (dx,) = torch.autograd.grad(y, x, dy)
    if with_res:
        dx = dx + dres
    assert _rel(R.rmsnorm_bwd(x.detach(), w, dy, dres, eps), dx) <= REL
    assert _rel(R.rmsnorm_fwd(x.detach(), w, eps), y.detach()) <= REL


@pytest.mark.parametrize("rows,cols,shift", [(7, 8, 0.0), (129, 520, 0.0), (9, 1408, 50.0)])
def test_layernorm_backward_is_autograd_of_layer_norm(rows, cols, shift):
    x = (torch.randn(rows, cols, generator=_g(7), dtype=torch.float64) * (0.5 if shift else 1.0) + shift).requires_grad_()
    w = torch.randn(cols, generator=_g(8), dtype=torch.float64, requires_grad=True)
    b = torch.randn(cols, generator=_g(9), dtype=torch.float64, requires_grad=True)
    dy = torch.randn(rows, cols, generator=_g(10), dtype=torch.float64)
    dres = torch.randn(rows, cols, generator=_g(11), dtype=torch.float64)
    eps = 1e-6
    y = F.layer_norm(x, (cols,), w, b, eps)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), dy)
    got = R.layernorm_bwd(x.detach(), w.detach(), dy, dres, eps)
    assert _rel(got[0], dx + dres) <= REL and _rel(got[1], dw) <= REL and _rel(got[2], db) <= REL
    assert _rel(got[3], x.detach().mean(-1)) <= REL
    assert _rel(got[4], torch.rsqrt(x.detach().var(-1, unbiased=False) + eps)) <= REL
    assert (got[5] >= got[1].abs() * (1 - 1e-9)).all() and (got[6] >= got[2].abs() * (1 - 1e-9)).all()


def test_gelu_backward_is_autograd_of_exact_gelu():
    h = torch.cat((torch.linspace(-8, 8, 1001, dtype=torch.float64), torch.zeros(1, dtype=torch.float64))).requires_grad_()
    dy = torch.randn(h.shape, generator=_g(12), dtype=torch.float64)
    y = F.gelu(h, approximate="none")
    (dh,) = torch.autograd.grad(y, h, dy)
    assert _rel(R.gelu_fwd(h.detach()), y.detach()) <= REL and _rel(R.gelu_bwd(h.detach(), dy), dh) <= REL


@pytest.mark.parametrize("rows,I", [(3, 16), (5, 48)])
def test_swiglu_backward_is_autograd_of_silu_gate_times_up(rows, I):
    gu = (torch.randn(rows, 2 * I, generator=_g(13), dtype=torch.float64) * 3).requires_grad_()
    dact = torch.randn(rows, I, generator=_g(14), dtype=torch.float64)
    # the interleave, stated by index: gate column c sits at (c // 16) * 32 + c % 16, up column c 16 further
    c = torch.arange(I)
    gi = (c // 16) * 32 + c % 16
    y = F.silu(gu[:, gi]) * gu[:, gi + 16]
    (dgu,) = torch.autograd.grad(y, gu, dact)
    assert _rel(R.swiglu_fwd(gu.detach(), I), y.detach()) <= REL and _rel(R.swiglu_bwd(gu.detach(), dact, I), dgu) <= REL
    g, u = R.deinterleave(gu.detach(), I)
    assert torch.equal(R.interleave(g, u), gu.detach())


@pytest.mark.parametrize("Hq,Hkv,D", [(4, 1, 128), (8, 8, 64)])
def test_rope_backward_is_autograd_of_hf_rotate_half(Hq, Hkv, D):
    B, S, Sk_ld, n_pos = 2, 5, 7, 40
    pos = torch.randint(0, n_pos, (B * S,), generator=_g(15), dtype=torch.int32)
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    ang = torch.arange(n_pos, dtype=torch.float64)[:, None] * inv_freq[None, :]
    cosT, sinT = ang.cos(), ang.sin()
    qkv = torch.randn(B * S, (Hq + 2 * Hkv) * D, generator=_g(16), dtype=torch.float64, requires_grad=True)
    # HF apply_rotary_pos_emb: cos / sin = cat(freqs, freqs); q_embed = q * cos + rotate_half(q) * sin, rotate_half(x) = cat(-x2, x1)
    cos = torch.cat((cosT, cosT), -1)[pos.long()][:, None, :]
    sin = torch.cat((sinT, sinT), -1)[pos.long()][:, None, :]

    def hf_rot(x):
        x1, x2 = x[..., : D // 2], x[..., D // 2:]
        return x * cos + torch.cat((-x2, x1), dim=-1) * sin
    q = hf_rot(qkv[:, : Hq * D].reshape(B * S, Hq, D))
    k = hf_rot(qkv[:, Hq * D: (Hq + Hkv) * D].reshape(B * S, Hkv, D))
    v = qkv[:, (Hq + Hkv) * D:].reshape(B * S, Hkv, D)
    dq = torch.randn(B * S, Hq, D, generator=_g(17), dtype=torch.float64)
    dk = torch.randn(B, Hkv, Sk_ld, D, generator=_g(18), dtype=torch.float64)
    dv = torch.randn(B, Hkv, Sk_ld, D, generator=_g(19), dtype=torch.float64)
    to_rows = lambda t: t[:, :, :S].permute(0, 2, 1, 3).reshape(B * S, Hkv, D)  # noqa: E731
    (dqkv,) = torch.autograd.grad((q, k, v), qkv, (dq, to_rows(dk), to_rows(dv)))
    assert _rel(R.rope_bwd_assemble(dq, dk, dv, cosT, sinT, pos, B, S, Hq, Hkv, D), dqkv) <= REL
    assert _rel(R.rope_fwd(qkv[:, : Hq * D].reshape(B * S, Hq, D).detach(), cosT[pos.long()][:, None], sinT[pos.long()][:, None]), q.detach()) <= REL


def test_cross_entropy_is_autograd_of_shifted_cross_entropy():
    B, S, V = 3, 5, 50
    logits = (torch.randn(B, S, V, generator=_g(20), dtype=torch.float64) * 4).requires_grad_()
    labels = torch.randint(0, V, (B, S), generator=_g(21))
    labels[0, 2] = -100
    labels[2, 4] = -100
    inv_n = 1.0 / 7.0
    shift_logits, shift_labels = logits[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1)
    total = F.cross_entropy(shift_logits, shift_labels, ignore_index=-100, reduction="sum") * inv_n
    (d,) = torch.autograd.grad(total, logits)
    rows = F.cross_entropy(shift_logits, shift_labels, ignore_index=-100, reduction="none").detach().reshape(B, S - 1)
    loss, dl, terms = R.cross_entropy(logits.detach(), labels, inv_n)
    assert _rel(dl, d.reshape(B * S, V)) <= REL
    assert _rel(loss.reshape(B, S)[:, :-1], rows) <= REL and (loss.reshape(B, S)[:, -1] == 0).all()
    assert (dl.reshape(B, S, V)[:, -1] == 0).all() and (dl.reshape(B, S, V)[0, 1] == 0).all() and loss.reshape(B, S)[0, 1] == 0
    assert (terms >= loss.abs()).all()
    # a label >= V: torch raises, the reference (like the kernel) ignores the row
    labels[1, 3] = V + 2
    with pytest.raises((IndexError, RuntimeError)):
        F.cross_entropy(logits[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100)
    loss2, dl2, _ = R.cross_entropy(logits.detach(), labels, inv_n)
    assert loss2.reshape(B, S)[1, 2] == 0 and (dl2.reshape(B, S, V)[1, 2] == 0).all()
    keep = torch.ones(B * S, dtype=torch.bool)
    keep[1 * S + 2] = False
    assert torch.equal(loss2[keep], loss[keep]) and torch.equal(dl2[keep], dl[keep])


def test_row_movers_by_hand():
    src = torch.arange(12, dtype=torch.float64).reshape(4, 3)
    assert torch.equal(R.gather_rows_idx(src, torch.tensor([2, -1, 2, 0])), torch.stack((src[2], torch.zeros(3, dtype=torch.float64), src[2], src[0])))
    seg = R.segment_sum_rows(src, torch.tensor([1, 1]), 2, 3)
    assert torch.equal(seg, torch.cat((torch.zeros(2, 3, dtype=torch.float64), src[:2] + src[2:], torch.zeros(2, 3, dtype=torch.float64))))
    flat = torch.arange(20, dtype=torch.float64)
    out, terms = R.acc_rows(torch.ones(4, dtype=torch.float64), flat, 3, 7, 4)
    assert torch.equal(out, 1 + flat[0:4] + flat[7:11] + flat[14:18]) and torch.equal(terms, out)


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw_reference_is_the_pinned_oracle_and_torch(t, wd):
    from oracle import train_oracle as TO
    n = 257
    p = torch.randn(n, generator=_g(22), dtype=torch.float64)
    g = torch.randn(n, generator=_g(23), dtype=torch.float64)
    g[::5] = 0
    m = torch.randn(n, generator=_g(24), dtype=torch.float64) * 0.1
    v = torch.rand(n, generator=_g(25), dtype=torch.float64) * 0.01
    p1, m1, v1 = TO.adamw_step(p, g, m, v, t, 1e-3, 0.9, 0.999, 1e-8, wd)
    # torch.optim.AdamW at step t with the same state
    q = p.clone().requires_grad_()
    opt = torch.optim.AdamW([q], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    q.grad = g.clone()
    opt.step()
    assert _rel(p1, q.detach()) <= REL and _rel(m1, opt.state[q]["exp_avg"]) <= REL and _rel(v1, opt.state[q]["exp_avg_sq"]) <= REL


def test_tolerance_helpers():
    ref = torch.tensor([1.0, -2.0, 0.0], dtype=torch.float64)
    assert R.delta_of(ref.float() + torch.tensor([0.0, 0.25, 0.0]), ref) == 8 * 0.25
    assert torch.equal(R.bound_bf16(ref, 0.5), torch.tensor([2.0 ** -8 + 0.5, 2.0 ** -7 + 0.5, 0.5], dtype=torch.float64))
    assert R.f32(0.999) == float(torch.tensor(0.999, dtype=torch.float32)) and R.pad64(65) == 128 and R.pad64(64) == 64


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals: every launcher checks its arguments before it launches, so these calls return VZ_ERR_ARG without touching a device.  OK / BAD
# stand for a 16-byte-aligned and a 4-element-offset address; neither is ever read - as long as no device is there to launch on, which is
# why these run only where none is visible (should a check regress, the launch then fails cleanly instead of reaching a device with made-up
# addresses).  Where there is one, tests/test_train_ops_gpu.py makes the same calls on real allocations.
# ------------------------------------------------------------------------------------------------------------------------------------
OK, BAD = 0x7F0000001000, 0x7F0000001008


@pytest.fixture(scope="module")
def L():
    from vz_hip import binding
    if torch.cuda.is_available():
        pytest.skip("made-up addresses: only where no device is visible (test_train_ops_gpu.py covers the refusals on a device)")
    return binding.load_library()


def _refused(L, rc, word):
    from vz_hip import binding
    assert rc == binding.VZ_ERR_ARG, rc
    assert word in L.vz_last_error().decode(), L.vz_last_error()


def test_swiglu_refuses_a_width_off_the_interleave(L):
    _refused(L, L.vz_op_swiglu_fwd(OK, OK, 4, 24, None), "swiglu_fwd")
    _refused(L, L.vz_op_swiglu_bwd(OK, OK, OK, 4, 24, None), "swiglu_bwd")
    _refused(L, L.vz_op_swiglu_fwd(OK, OK, 4, 8, None), "swiglu_fwd")


def test_elementwise_and_row_movers_refuse_null_and_empty(L):
    _refused(L, L.vz_op_gelu_fwd(None, OK, 16, None), "gelu_fwd")
    _refused(L, L.vz_op_gelu_fwd(OK, None, 16, None), "gelu_fwd")
    _refused(L, L.vz_op_gelu_fwd(OK, OK, 0, None), "gelu_fwd")
    _refused(L, L.vz_op_gelu_bwd(OK, None, OK, 16, None), "gelu_bwd")
    _refused(L, L.vz_op_gelu_bwd(OK, OK, OK, -1, None), "gelu_bwd")
    _refused(L, L.vz_op_swiglu_fwd(None, OK, 4, 16, None), "swiglu_fwd")
    _refused(L, L.vz_op_swiglu_fwd(OK, OK, 0, 16, None), "swiglu_fwd")
    _refused(L, L.vz_op_swiglu_bwd(OK, OK, None, 4, 16, None), "swiglu_bwd")
    _refused(L, L.vz_op_swiglu_bwd(OK, OK, OK, 4, 0, None), "swiglu_bwd")
    _refused(L, L.vz_op_gather_rows_idx(None, OK, OK, 4, 64, None), "gather_rows_idx")
    _refused(L, L.vz_op_gather_rows_idx(OK, None, OK, 4, 64, None), "gather_rows_idx")
    _refused(L, L.vz_op_gather_rows_idx(OK, OK, OK, 0, 64, None), "gather_rows_idx")
    _refused(L, L.vz_op_gather_rows_idx(OK, OK, OK, 4, 60, None), "gather_rows_idx")
    _refused(L, L.vz_op_segment_sum_rows(OK, None, 2, 2, OK, 2, 8, None), "segment_sum_rows")
    _refused(L, L.vz_op_segment_sum_rows(OK, OK, 0, 2, OK, 2, 8, None), "segment_sum_rows")
    _refused(L, L.vz_op_segment_sum_rows(OK, OK, 2, 2, OK, 2, 0, None), "segment_sum_rows")
    _refused(L, L.vz_op_acc_rows_f32(None, OK, 2, 64, 2, 8, None), "acc_rows_f32")
    _refused(L, L.vz_op_acc_rows_f32(OK, OK, 0, 64, 2, 8, None), "acc_rows_f32")
    _refused(L, L.vz_op_acc_rows_f32(OK, OK, 2, 64, 2, -8, None), "acc_rows_f32")


def test_rope_backward_refuses_odd_head_dim_null_and_empty(L):
    args = lambda D, S=4, dq=OK, pos=OK: (dq, OK, OK, OK, OK, OK, pos, 2, S, 4, 1, D, 8, None)  # noqa: E731
    _refused(L, L.vz_op_rope_bwd_assemble(*args(127)), "odd head_dim")
    _refused(L, L.vz_op_rope_bwd_assemble(*args(128, dq=None)), "rope_bwd_assemble")
    _refused(L, L.vz_op_rope_bwd_assemble(*args(128, pos=None)), "rope_bwd_assemble")
    _refused(L, L.vz_op_rope_bwd_assemble(*args(128, S=0)), "rope_bwd_assemble")
    _refused(L, L.vz_op_rope_bwd_assemble(*args(128, S=9)), "rope_bwd_assemble")          # the K / V cache rows are shorter than the sequence


def test_sixteen_byte_loads_refuse_misaligned_bases(L):
    n = L.vz_op_layernorm_bwd_scratch_floats(4, 64)
    assert n == 4 * 2 * 64 + 2 * 4 and L.vz_op_layernorm_bwd_scratch_floats(1000, 8) == 128 * 2 * 8 + 2000
    for bad in range(4):            # x, dy, dres, dx in turn
        a = [OK, OK, OK, OK]
        a[bad] = BAD
        _refused(L, L.vz_op_layernorm_bwd(a[0], OK, a[1], a[2], a[3], OK, n, OK, OK, 4, 64, 1e-6, None), "16-byte")
    _refused(L, L.vz_op_layernorm_bwd(OK, OK, OK, None, OK, OK, n - 1, OK, OK, 4, 64, 1e-6, None), "scratch")
    _refused(L, L.vz_op_layernorm_bwd(OK, OK, OK, None, OK, OK, n, OK, OK, 4, 60, 1e-6, None), "layernorm_bwd")
    _refused(L, L.vz_op_gather_rows_idx(BAD, OK, OK, 4, 64, None), "16-byte")
    _refused(L, L.vz_op_gather_rows_idx(OK, OK, BAD, 4, 64, None), "16-byte")


def test_softmax_and_cross_entropy_refuse_short_leading_dimensions(L):
    _refused(L, L.vz_op_softmax_fwd(OK, 64, OK, 64, 4, 1, 4, 65, 1.0, 0, 0, None, None), "softmax_fwd")
    _refused(L, L.vz_op_softmax_fwd(OK, 64, OK, 64, 4, 1, 0, 64, 1.0, 0, 0, None, None), "softmax_fwd")
    _refused(L, L.vz_op_softmax_bwd(OK, 64, OK, 64, OK, 32, 4, 64, 1.0, None), "softmax_bwd")
    _refused(L, L.vz_op_cross_entropy(OK, 100, OK, 4, 2, 1.0, OK, OK, 96, None), "cross_entropy")
    _refused(L, L.vz_op_cross_entropy(OK, 100, OK, 4, 0, 1.0, OK, OK, 128, None), "cross_entropy")          # row % S on the device
    _refused(L, L.vz_op_cross_entropy(OK, 0, OK, 4, 2, 1.0, OK, None, 0, None), "cross_entropy")
    _refused(L, L.vz_op_cross_entropy(OK, 100, OK, 2 ** 31, 2, 1.0, OK, None, 0, None), "cross_entropy")    # one workgroup per row: an int grid
    _refused(L, L.vz_op_adamw(OK, OK, OK, OK, OK, 1, 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None), "adamw")
    _refused(L, L.vz_op_transpose_batched(OK, 8, 0, 0, OK, 8, 0, 0, 8, 8, 300, 300, 0, None), "transpose")
