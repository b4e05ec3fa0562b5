"""fp32 torch reference of the shared-prefix decode attention (vz_op_attention_shared) and the poisoned buffers its
tests run on."""
import torch

NAN = float("nan")


def visible(r, n, shared, slot, window=0):
    """[(cache row, slot)] row r of the step sees, in slot order: the slots [0, shared[g]) of cache row g * n and the slots
    [shared[g], slot[r]] of its own row (a row with slot[r] < shared[g] shares nothing: its own slots [0, slot[r]]); window > 0: only the
    slots > slot[r] - window of that union."""
    g, sl = r // n, int(slot[r])
    sh = int(shared[g]) if sl >= int(shared[g]) else 0
    keys = [(g * n, j) for j in range(sh)] + [(r, j) for j in range(sh, sl + 1)]
    return [(row, j) for row, j in keys if window <= 0 or j > sl - window]


def shared_attention_ref(q, kc, vc, n, shared, slot, scale, window=0):
    """q [R,Hq,D], caches [R,Hkv,max_ctx,D] (bf16 values), shared [R / n] and slot [R]: python ints.  Per row, the visible slots
    concatenated and softmax attention over them in fp32.  Returns fp32 [R,Hq,D]."""
    R, Hq, D = q.shape
    Hkv = kc.shape[1]
    out = torch.empty(R, Hq, D, dtype=torch.float32, device=q.device)
    for r in range(R):
        keys = visible(r, n, shared, slot, window)
        rows = torch.tensor([k[0] for k in keys], device=q.device)
        slots = torch.tensor([k[1] for k in keys], device=q.device)
        kf = kc[rows, :, slots].float().permute(1, 0, 2).repeat_interleave(Hq // Hkv, dim=0)          # [Hq,keys,D]
        vf = vc[rows, :, slots].float().permute(1, 0, 2).repeat_interleave(Hq // Hkv, dim=0)
        p = torch.softmax(torch.einsum("hd,hkd->hk", q[r].float(), kf) * scale, dim=-1)
        out[r] = torch.einsum("hk,hkd->hd", p, vf)
    return out


def poisoned_case(R, n, Hq, Hkv, D, max_ctx, shared, slot, seed, device="cuda"):
    """(q, kc, vc, out): random bf16 where the op may read, NaN everywhere else - the first shared[g] slots of every non-first row of a
    group (the prefix is not read from the own row), every slot behind slot[r] (in a group's first row: behind the shared slots too),
    the whole output buffer."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn(R, Hq, D, generator=g).bfloat16()
    kc = torch.randn(R, Hkv, max_ctx, D, generator=g).bfloat16()
    vc = torch.randn(R, Hkv, max_ctx, D, generator=g).bfloat16()
    for r in range(R):
        sh, sl = int(shared[r // n]), int(slot[r])
        if r % n:
            if sl >= sh:          # (a row with slot < shared reads its own slots [0, slot], nothing of the group's: those stay)
                kc[r, :, :sh] = NAN
                vc[r, :, :sh] = NAN
            end = sl + 1
        else:
            end = max(sl + 1, sh)
        kc[r, :, end:] = NAN
        vc[r, :, end:] = NAN
    out = torch.full((R, Hq, D), NAN, dtype=torch.bfloat16)
    return q.to(device), kc.to(device), vc.to(device), out.to(device)


def copied_cache(kc, vc, n, shared):
    """the caches of the copy route: every group's shared slots copied from its first row into its other rows"""
    kc, vc = kc.clone(), vc.clone()
    for r in range(kc.shape[0]):
        if r % n:
            sh = int(shared[r // n])
            kc[r, :, :sh] = kc[r - r % n, :, :sh]
            vc[r, :, :sh] = vc[r - r % n, :, :sh]
    return kc, vc
