"""Plain torch restatements of the operations of the Stage-1 training kernels (csrc/train.hip), written from the math and from the HF
definitions the kernels' comments quote - not from the kernels.  Every function takes `dt`: float64 gives the reference, float32 the
unrounded fp32 evaluation whose distance from the reference sets the fp32-arithmetic allowance `delta` of a test (see `bound_bf16`).
Inputs are the exact bf16 / fp32 values a kernel sees, upcast; scalars (eps, scale, lr, ...) are passed through `f32` first, since the
C ABI hands them over as floats.  tests/test_train_ref_cpu.py holds every backward here to float64 autograd of its forward."""
import math
import struct

import torch

F64, F32 = torch.float64, torch.float32
U_BF16 = 2.0 ** -8          # unit roundoff of bf16 (8 significand bits, round to nearest)
U_FP32 = 2.0 ** -24         # unit roundoff of fp32
FP32_FACTOR = 8.0           # __expf / rsqrtf at a few ulp where libm has half an ulp, and another summation order


def f32(v: float) -> float:
    """the float the C ABI delivers for a Python scalar"""
    return struct.unpack("f", struct.pack("f", v))[0]


def pad64(n: int) -> int:
    return (n + 63) // 64 * 64


# ---------------------------------------------------------------------------------------------------------------------------------
# masked softmax.  Row = (b * H + h) * Sq + i; query i sits at position i.  Key j is visible iff j < min(kv_len[b], Sk), and, when causal,
# j <= i and (window > 0) j > i - window.  A row that sees nothing is all zeros.
# ---------------------------------------------------------------------------------------------------------------------------------
def softmax_visible(rows, H, Sq, Sk, causal, window, kv_len):
    r = torch.arange(rows)
    i = (r % Sq)[:, None]
    b = r // (Sq * H)
    j = torch.arange(Sk)[None, :]
    hi = torch.full((rows,), Sk, dtype=torch.long) if kv_len is None else kv_len.long().cpu()[b].clamp(max=Sk)
    vis = j < hi[:, None]
    if causal:
        vis = vis & (j <= i)
        if window > 0:
            vis = vis & (j > i - window)
    return vis


def softmax_fwd(S, vis, scale, dt=F64):
    z = (S.to(dt) * scale).masked_fill(~vis, -math.inf)
    m = z.max(dim=1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.where(vis, torch.exp(z - m), torch.zeros_like(z))
    l = e.sum(dim=1, keepdim=True)
    return torch.where(l > 0, e / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(e))


def softmax_bwd(P, dP, scale, dt=F64):
    """dS = P o (dP - sum_j P dP) scale; where P == 0 the result is 0 and dP does not enter (it may hold anything)"""
    P = P.to(dt)
    live = P != 0
    dPz = torch.where(live, dP.to(dt), torch.zeros_like(P))
    d = (P * dPz).sum(dim=1, keepdim=True)
    return P * (dPz - d) * scale


# ---------------------------------------------------------------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------------------------------------------------------------
def rmsnorm_fwd(x, w, eps):
    """MistralRMSNorm: w * x * rsqrt(mean(x^2) + eps)"""
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def rmsnorm_bwd(x, w, dy, dres, eps, dt=F64):
    x, w, dy = x.to(dt), w.to(dt), dy.to(dt)
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    xh, g = x * r, dy * w
    dx = r * (g - xh * (g * xh).mean(-1, keepdim=True))
    return dx if dres is None else dx + dres.to(dt)


def layernorm_bwd(x, w, dy, dres, eps, dt=F64):
    """-> dx, dw, db, mean, rstd, |dw| terms, |db| terms   (torch.nn.LayerNorm: biased variance)"""
    x, w, dy = x.to(dt), w.to(dt), dy.to(dt)
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = torch.rsqrt(xc.pow(2).mean(-1, keepdim=True) + eps)
    xh, g = xc * rstd, dy * w
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres.to(dt)
    return dx, (dy * xh).sum(0), dy.sum(0), mean[:, 0], rstd[:, 0], (dy * xh).abs().sum(0), dy.abs().sum(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# element-wise
# ---------------------------------------------------------------------------------------------------------------------------------
def gelu_fwd(h, dt=F64):
    h = h.to(dt)
    return 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))


def gelu_bwd(h, dy, dt=F64):
    h = h.to(dt)
    cdf = 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)
    return dy.to(dt) * (cdf + h * pdf)


def deinterleave(gu, I):
    """gu [rows, 2I] in column order [16 g | 16 u | 16 g | ...] -> (g, u), each [rows, I]"""
    t = gu.reshape(gu.shape[0], I // 16, 2, 16)
    return t[:, :, 0, :].reshape(-1, I), t[:, :, 1, :].reshape(-1, I)


def interleave(g, u):
    rows, I = g.shape
    return torch.stack((g.reshape(rows, I // 16, 16), u.reshape(rows, I // 16, 16)), dim=2).reshape(rows, 2 * I)


def swiglu_fwd(gu, I, dt=F64):
    g, u = deinterleave(gu.to(dt), I)
    return g * torch.sigmoid(g) * u


def swiglu_bwd(gu, dact, I, dt=F64):
    g, u = deinterleave(gu.to(dt), I)
    d = dact.to(dt)
    sg = torch.sigmoid(g)
    return interleave(d * u * sg * (1.0 + g * (1.0 - sg)), d * g * sg)


# ---------------------------------------------------------------------------------------------------------------------------------
# RoPE (HF rotate_half): y = x cos + rotate_half(x) sin with rotate_half(x) = [-x2, x1], cos / sin = [table, table].  Its transpose:
# dx = dy cos + rotate_half^T(dy sin), rotate_half^T(z) = [z2, -z1].
# ---------------------------------------------------------------------------------------------------------------------------------
def rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


def rope_fwd(x, cos, sin):
    """x [..., D], cos / sin [..., D/2] (broadcastable)"""
    c, s = torch.cat((cos, cos), -1), torch.cat((sin, sin), -1)
    return x * c + rotate_half(x) * s


def rope_bwd(dy, cos, sin):
    c, s = torch.cat((cos, cos), -1), torch.cat((sin, sin), -1)
    z = dy * s
    h = z.shape[-1] // 2
    return dy * c + torch.cat((z[..., h:], -z[..., :h]), dim=-1)


def rope_bwd_assemble(dq, dk, dv, cosT, sinT, pos, B, S, Hq, Hkv, D, dt=F64):
    """dq [B*S, Hq, D], dk / dv [B, Hkv, Sk_ld, D] (positions >= S unused) -> dqkv [B*S, (Hq + 2 Hkv) D]"""
    c, s = cosT.to(dt)[pos.long()][:, None, :], sinT.to(dt)[pos.long()][:, None, :]          # [B*S, 1, D/2]
    k = dk.to(dt)[:, :, :S].permute(0, 2, 1, 3).reshape(B * S, Hkv, D)
    v = dv.to(dt)[:, :, :S].permute(0, 2, 1, 3).reshape(B * S, Hkv, D)
    return torch.cat((rope_bwd(dq.to(dt), c, s).reshape(B * S, -1), rope_bwd(k, c, s).reshape(B * S, -1), v.reshape(B * S, -1)), dim=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# causal-LM cross-entropy (HF ForCausalLMLoss): row (b, s) is scored against labels[b][s + 1]; the last position of a sequence and a
# target of -100 are ignored.  A target >= V is ignored too - a departure from torch, whose cross_entropy raises on it: the kernel cannot
# raise, and the trainer pads its vocabulary, so such a label counts as "no target".
# ---------------------------------------------------------------------------------------------------------------------------------
def ce_targets(labels, V):
    """labels [B, S] -> target [B, S] (-100 where ignored)"""
    t = torch.full_like(labels, -100)
    t[:, :-1] = labels[:, 1:]
    return torch.where((t >= 0) & (t < V), t, torch.full_like(t, -100))


def cross_entropy(logits, labels, inv_n, dt=F64):
    """logits [B, S, V], labels [B, S] -> loss_rows [B*S], dlogits [B*S, V], |terms| of a loss row"""
    B, S, V = logits.shape
    l = logits.to(dt).reshape(B * S, V)
    t = ce_targets(labels.long(), V).reshape(-1)
    valid = t >= 0
    tc = t.clamp(min=0)
    lse = torch.logsumexp(l, dim=1)
    lt = l.gather(1, tc[:, None])[:, 0]
    loss = torch.where(valid, lse - lt, torch.zeros_like(lse))
    onehot = torch.zeros_like(l).scatter_(1, tc[:, None], 1.0)
    d = torch.where(valid[:, None], (torch.softmax(l, dim=1) - onehot) * inv_n, torch.zeros_like(l))
    return loss, d, lse.abs() + lt.abs()


# ---------------------------------------------------------------------------------------------------------------------------------
# row movers
# ---------------------------------------------------------------------------------------------------------------------------------
def gather_rows_idx(src, idx):
    out = src[idx.long().clamp(min=0)].clone()
    out[idx < 0] = 0
    return out


def segment_sum_rows(src, seg_map, rows_per, n_dst, dt=F64):
    """src [n_src * rows_per, cols] -> [n_dst * rows_per, cols]: block r = sum of the source blocks k with seg_map[k] == r"""
    cols = src.shape[1]
    s = src.to(dt).reshape(-1, rows_per, cols)
    out = torch.zeros(n_dst, rows_per, cols, dtype=dt)
    for k, r in enumerate(seg_map.tolist()):
        if 0 <= r < n_dst:
            out[r] += s[k]
    return out.reshape(n_dst * rows_per, cols)


def acc_rows(out0, src_flat, n_batches, stride, n, dt=F64):
    """out0 [n] + sum_b src_flat[b * stride : b * stride + n]; also the sum of absolute terms"""
    terms = torch.stack([src_flat[b * stride:b * stride + n].to(dt) for b in range(n_batches)])
    return out0.to(dt) + terms.sum(0), out0.to(dt).abs() + terms.abs().sum(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the yardstick: bf16 output  |hip - ref| <= 2^-8 |ref| + delta,  delta = 8 x max |fp32 evaluation - ref| over the test's
# inputs; fp32 output the same with both sides divided by the sum of absolute terms of the element's reduction (no bf16 term)
# ---------------------------------------------------------------------------------------------------------------------------------
def delta_of(ref32, ref64, terms=None):
    d = (ref32.to(F64) - ref64).abs()
    if terms is not None:
        d = d / terms.clamp_min(1e-300)
    return FP32_FACTOR * float(d.max()) if d.numel() else 0.0


def bound_bf16(ref64, delta):
    return U_BF16 * ref64.abs() + delta
