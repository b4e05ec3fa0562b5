"""fp32 torch reference of the append attention (vz_op_attention_append) and the poisoned buffers its tests run on."""
import torch

NAN = float("nan")


def append_attention_ref(q, kc, vc, past, new, scale, window=0):
    """q [B,T,Hq,D], caches [B,Hkv,max_ctx,D] (bf16 values), past / new: python ints per row.  Token i < new[b] of row b attends the
    slots j <= past[b] + i (window > 0: and j > past[b] + i - window); only slots below past[b] + new[b] are touched.  Returns fp32
    [B,T,Hq,D] with NaN in the token rows >= new[b]."""
    Bn, T, Hq, D = q.shape
    Hkv = kc.shape[1]
    out = torch.full((Bn, T, Hq, D), NAN, dtype=torch.float32, device=q.device)
    for b in range(Bn):
        n, kv = int(new[b]), int(past[b]) + int(new[b])
        qf = q[b, :n].float()                                                   # [n,Hq,D]
        kf = kc[b, :, :kv].float().repeat_interleave(Hq // Hkv, dim=0)          # [Hq,kv,D]
        vf = vc[b, :, :kv].float().repeat_interleave(Hq // Hkv, dim=0)
        s = torch.einsum("qhd,hkd->hqk", qf, kf) * scale
        qp = (torch.arange(n, device=q.device) + int(past[b])).view(1, n, 1)
        kp = torch.arange(kv, device=q.device).view(1, 1, kv)
        keep = kp <= qp
        if window > 0:
            keep = keep & (kp > qp - window)
        p = torch.softmax(s.masked_fill(~keep, float("-inf")), dim=-1)
        out[b, :n] = torch.einsum("hqk,hkd->qhd", p, vf)
    return out


def poisoned_case(Bn, T, Hq, Hkv, D, max_ctx, past, new, seed, device="cuda"):
    """(q, kc, vc): random bf16 where the op may read, NaN everywhere else - cache slots at and behind past + new, query rows >= new."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn(Bn, T, Hq, D, generator=g).bfloat16()
    kc = torch.randn(Bn, Hkv, max_ctx, D, generator=g).bfloat16()
    vc = torch.randn(Bn, Hkv, max_ctx, D, generator=g).bfloat16()
    for b in range(Bn):
        q[b, int(new[b]):] = NAN
        kc[b, :, int(past[b]) + int(new[b]):] = NAN
        vc[b, :, int(past[b]) + int(new[b]):] = NAN
    return q.to(device), kc.to(device), vc.to(device)
