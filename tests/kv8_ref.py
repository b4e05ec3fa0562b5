"""Shared helpers of the e4m3 KV-mirror tests: the quantiser as the mirror's definition states it, an fp32
reference of the decode attention over a mirror, and the poisoned-case builder of the op test."""
import torch

from vz_hip import quant

D = 128


def quantize_kv(x: torch.Tensor):
    """x [..., 128] (any float dtype) -> (uint8 [..., 128] e4m3 bytes, fp32 [...] scales = 2^e): every 128-value row through
    quant.quantize_rows - e = the smallest integer with max|x| <= 448 * 2^e (0 for an all-zero row), q = e4m3_rne(x * 2^-e)."""
    assert x.shape[-1] == D
    q, s = quant.quantize_rows(x.reshape(-1, D))
    return q.reshape(x.shape), s.reshape(x.shape[:-1])


def dequant(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """fp32 [..., 128] = 2^e * e4m3 (exact)"""
    return q.view(torch.float8_e4m3fn).float() * s.float().unsqueeze(-1)


def rope_rows(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """rotate-half RoPE of x fp32 [B, heads, 128] at positions pos [B] with the [max_pos, 64] tables, rounded to bf16 as the kernels do"""
    c = torch.cat([cos, cos], -1)[pos.long()].unsqueeze(1)
    s = torch.cat([sin, sin], -1)[pos.long()].unsqueeze(1)
    rot = torch.cat([-x[..., D // 2:], x[..., :D // 2]], -1)
    return (x * c + rot * s).bfloat16().float()


def decode_attention_ref(q_rot, k_new, v_new, kf, vf, slot, scale, window, dtype=torch.float32):
    """One decode step over float caches kf / vf [B,Hkv,ctx,128], in `dtype` arithmetic.  q_rot [B,Hq,128], k_new / v_new [B,Hkv,128]: the
    rotated, bf16-rounded new token; slot [B] (ints).  Keys of row b: cache slots [lo, slot[b]), then the new row itself at slot[b];
    lo = max(0, slot + 1 - window) for window > 0.  Nothing from slot[b] on is read from the caches.  -> [B,Hq,128] in `dtype`."""
    B, Hq, _ = q_rot.shape
    Hkv = k_new.shape[1]
    G = Hq // Hkv
    out = torch.zeros(B, Hq, D, dtype=dtype, device=q_rot.device)
    for b in range(B):
        n = int(slot[b])
        lo = max(0, n + 1 - window) if window > 0 else 0
        k = torch.cat([kf[b, :, lo:n].float(), k_new[b].float().unsqueeze(1)], 1).to(dtype)      # [Hkv, keys, 128]
        v = torch.cat([vf[b, :, lo:n].float(), v_new[b].float().unsqueeze(1)], 1).to(dtype)
        q = q_rot[b].to(dtype).view(Hkv, G, D)
        p = torch.softmax(torch.einsum("hgd,hkd->hgk", q, k) * scale, -1)
        out[b] = torch.einsum("hgk,hkd->hgd", p, v).reshape(Hq, D)
    return out


def decode_attention_kv8_ref(q_rot, k_new, v_new, k8, ks, v8, vs, slot, scale, window, dtype=torch.float32):
    """decode_attention_ref over a mirror: k8 / v8 uint8 [B,Hkv,ctx,128] with scales ks / vs [B,Hkv,ctx] - the DEQUANTISED mirror for slots
    < slot[b], the new row itself (its bf16 values, not quantised) at slot[b]."""
    return decode_attention_ref(q_rot, k_new, v_new, dequant(k8, ks), dequant(v8, vs), slot, scale, window, dtype)


def rope_tables(max_pos: int, device="cpu"):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))
    fr = torch.arange(max_pos, dtype=torch.float32).unsqueeze(-1) * inv
    return fr.cos().to(device).contiguous(), fr.sin().to(device).contiguous()


def uneven_rows(shape, seed: int, device="cpu", phase: int = 0) -> torch.Tensor:
    """bf16 [..., slots, 128] of unit-normal rows whose magnitudes alternate between 2^-8 (slot % 2 == phase) and 2^6 along the slot
    axis: neighbouring keys get scales 2^14 apart, so a dropped or misplaced scale cannot hide"""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(*shape, D, generator=g, device=device)
    mag = torch.where(torch.arange(shape[-1], device=device) % 2 == phase, 2.0 ** -8, 2.0 ** 6).view(*([1] * (len(shape) - 1)), shape[-1], 1)
    return (x * mag).bfloat16()


def poisoned_case(B: int, Hq: int, Hkv: int, max_ctx: int, slots, seed: int, device="cuda"):
    """The inputs of one attention call with everything the kernel may not read poisoned.  The caches hold uneven_rows in front of each
    row's slot (K's large rows on odd slots, V's on even ones, so that keys of either scale carry weight; the queries are scaled by 1/16
    to keep the softmax from collapsing onto one large key) and NaN from the slot on (bf16 caches, mirror bytes - 0x7f is e4m3's NaN -
    and scales); the output buffer is NaN.
    -> dict(qkv, kc, vc, k8, ks, v8, vs, out, slot, pos, cos, sin, k_src, v_src) with k_src / v_src the unquantised bf16 rows."""
    assert len(slots) == B and all(0 <= s < max_ctx for s in slots)
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g)
    qkv[:, :Hq * D] *= 1.0 / 16
    qkv = qkv.bfloat16().to(device)
    k_src = uneven_rows((B, Hkv, max_ctx), seed + 1, device, phase=0)
    v_src = uneven_rows((B, Hkv, max_ctx), seed + 2, device, phase=1)
    k8, ks = quantize_kv(k_src)
    v8, vs = quantize_kv(v_src)
    kc, vc = k_src.clone(), v_src.clone()
    for b, s in enumerate(slots):
        kc[b, :, s:] = float("nan"); vc[b, :, s:] = float("nan")
        k8[b, :, s:] = 0x7f; v8[b, :, s:] = 0x7f
        ks[b, :, s:] = float("nan"); vs[b, :, s:] = float("nan")
    slot = torch.tensor(list(slots), dtype=torch.int32, device=device)
    pos = slot + 5
    cos, sin = rope_tables(max_ctx + 8, device)
    out = torch.full((B, Hq, D), float("nan"), dtype=torch.bfloat16, device=device)
    return dict(qkv=qkv, kc=kc, vc=vc, k8=k8.contiguous(), ks=ks.contiguous(), v8=v8.contiguous(), vs=vs.contiguous(), out=out, slot=slot, pos=pos,
                cos=cos, sin=sin, k_src=k_src, v_src=v_src)


def new_rows(case, Hq: int, Hkv: int):
    """(q_rot [B,Hq,128], k_new [B,Hkv,128], v_new [B,Hkv,128]) fp32: the rotated, bf16-rounded new token of a poisoned_case"""
    x = case["qkv"].float().view(-1, Hq + 2 * Hkv, D)
    q = rope_rows(x[:, :Hq], case["cos"], case["sin"], case["pos"])
    k = rope_rows(x[:, Hq:Hq + Hkv], case["cos"], case["sin"], case["pos"])
    return q, k, x[:, Hq + Hkv:].contiguous()


def scale_ok(s: torch.Tensor) -> bool:
    """every scale is a power of two"""
    m, _ = torch.frexp(s.double())
    return bool((m == 0.5).all())

