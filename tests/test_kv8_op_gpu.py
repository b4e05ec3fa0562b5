"""The e4m3 KV mirror's two kernels on caller buffers (csrc/attn_decode_kv8.hip), at Hq 32, Hkv 8, D 128, max_ctx 512:
the mirror writer byte for byte against the quantiser's definition, and the decode attention against the fp32 reference over the
dequantised mirror, with everything behind each row's slot poisoned."""
import pytest
import torch

import kv8_ref as R
from util import check_close, errs, record

pytestmark = pytest.mark.gpu

HQ, HKV, D, CTX = 32, 8, 128, 512
SCALE = D ** -0.5
SLOTS = [0, 1, 63, 64, 127, 128, 129, 200, 511]


@pytest.fixture(scope="module")
def B():
    from vz_hip import binding
    binding.load_library()
    return binding


def test_mirror_rows_equal_the_quantiser(B):
    """ranges [0, n), n in {1, 63, 64, 65, 512} (and an untouched row) in ONE launch, rows listed out of order; row magnitudes 2^-10 .. 2^9 and
    an all-zero row; every slot >= n keeps its pre-filled pattern"""
    rows, lens = [4, 0, 5, 2, 1, 3], [1, 63, 64, 65, 512, 0]
    Rn = 7                                                       # cache row 6 is not listed at all
    g = torch.Generator().manual_seed(7)
    mag = torch.exp2(torch.randint(-10, 10, (Rn, HKV, CTX, 1), generator=g).float())
    kc = (torch.randn(Rn, HKV, CTX, D, generator=g) * mag).bfloat16().cuda()
    vc = (torch.randn(Rn, HKV, CTX, D, generator=g) * mag.flip(2)).bfloat16().cuda()
    kc[0, 3, 17] = 0                                             # all-zero rows inside covered ranges
    vc[1, 0, 500] = 0
    kc[2, 1, 3] = 1.0                                            # the boundary, and just past it
    vc[2, 1, 3] = 1.0
    kc[2, 1, 3, 40] = 448.0
    vc[2, 1, 3, 40] = 450.0
    k8 = torch.full((Rn, HKV, CTX, D), 0xA5, dtype=torch.uint8, device="cuda")
    v8 = torch.full_like(k8, 0x5A)
    ks = torch.full((Rn, HKV, CTX), -7.0, device="cuda")
    vs = torch.full_like(ks, -9.0)
    B.kv8_mirror_rows(kc, vc, k8, v8, ks, vs, rows, lens)
    torch.cuda.synchronize()
    want_k8, want_ks = R.quantize_kv(kc)
    want_v8, want_vs = R.quantize_kv(vc)
    assert R.scale_ok(want_ks) and float(want_ks[0, 3, 17]) == 1.0 and float(want_ks[2, 1, 3]) == 1.0 and float(want_vs[2, 1, 3]) == 2.0
    n_of = dict(zip(rows, lens))
    for r in range(Rn):
        n = n_of.get(r, 0)
        for got, want, fill in ((k8, want_k8, 0xA5), (v8, want_v8, 0x5A)):
            assert torch.equal(got[r, :, :n], want[r, :, :n]), f"row {r}: mirror bytes of [0, {n})"
            assert bool((got[r, :, n:] == fill).all()), f"row {r}: bytes behind {n} touched"
        for got, want, fill in ((ks, want_ks, -7.0), (vs, want_vs, -9.0)):
            assert torch.equal(got[r, :, :n], want[r, :, :n]), f"row {r}: scales of [0, {n})"
            assert bool((got[r, :, n:] == fill).all()), f"row {r}: scales behind {n} touched"


def _ragged(Bn, seed):
    g = torch.Generator().manual_seed(seed)
    pick = torch.randint(0, len(SLOTS), (Bn,), generator=g).tolist()
    s = [SLOTS[i] for i in pick]
    s[:min(Bn, len(SLOTS))] = SLOTS[:min(Bn, len(SLOTS))]       # every listed slot appears once the batch is wide enough
    return s


# (rows' slots, key splits, window).  Splits: what the engine's launcher can choose at max_ctx 512 - 1..4 chunks of 128 keys, held to
# 512 / (rows x 8) workgroups (64 rows: 1, 17 rows: 3) - and forced ones beyond it (7, 32: most splits find no keys and leave at once).
CASES = [([s], ns, 0) for s, ns in zip(SLOTS, [4, 1, 2, 32, 3, 4, 2, 7, 4])] + [
    ([0, 129, 511], 4, 0), ([63, 64, 200], 3, 0), ([511, 128, 1], 32, 0), ([127, 200, 511], 2, 0), ([511, 511, 511], 1, 0),
    (_ragged(17, 1), 3, 0), (_ragged(17, 2), 1, 0), (_ragged(17, 3), 32, 0),
    (_ragged(64, 4), 1, 0), (_ragged(64, 5), 4, 0),
    # windows: 8 and 48 keys; slot 200 with window 48 is keys 153..200 - a range that starts and ends inside one chunk; slot 5 < window
    ([200, 511, 5], 4, 8), ([200, 511, 5], 4, 48), ([129], 2, 8), ([130, 47, 48], 3, 48), (_ragged(17, 6), 3, 48), (_ragged(64, 7), 1, 8),
]


@pytest.mark.parametrize("slots,nsplit,window", CASES, ids=[f"B{len(s)}-slot{s[0]}-ns{ns}-w{w}" for s, ns, w in CASES])
def test_attention_kv8(B, slots, nsplit, window):
    Bn = len(slots)
    c = R.poisoned_case(Bn, HQ, HKV, CTX, slots, seed=100 + Bn + nsplit + window)
    before = {k: c[k].clone() for k in ("kc", "vc", "k8", "v8", "ks", "vs")}
    out, ticket = B.attention_decode_kv8(c["qkv"], c["kc"], c["vc"], c["k8"], c["v8"], c["ks"], c["vs"], c["cos"], c["sin"], c["pos"], c["slot"],
                                         HQ, SCALE, nsplit, window, out=c["out"])
    torch.cuda.synchronize()
    assert int(ticket.abs().sum()) == 0, "ticket not reset by the last arriver"
    q_rot, k_new, v_new = R.new_rows(c, HQ, HKV)
    ref = R.decode_attention_kv8_ref(q_rot, k_new, v_new, before["k8"], before["ks"], before["v8"], before["vs"], slots, SCALE, window)
    name = f"kv8 decode attention B{Bn} nsplit{nsplit} window{window}"
    for b in range(Bn):
        check_close(f"{name} row {b} slot {slots[b]}", out[b], ref[b], 8e-3, 4e-3)
    # the existing bf16 kernel on the same, unquantised rows: its append is what the kv8 kernel must append, bit for bit; its error
    # against the fp32 attention over the unquantised rows is recorded next to the kv8 kernel's (not asserted)
    kc2, vc2 = c["k_src"].clone(), c["v_src"].clone()
    out16, _ = B.attention_decode_fused(c["qkv"], kc2, vc2, c["cos"], c["sin"], c["pos"], c["slot"], HQ, SCALE, nsplit, window)
    ref16 = R.decode_attention_ref(q_rot, k_new, v_new, c["k_src"], c["v_src"], slots, SCALE, window)
    record(name, kv8_vs_mirror_ref=errs(out, ref), bf16_vs_unquantised_ref=errs(out16, ref16), kv8_vs_unquantised_ref=errs(out, ref16))
    bits = lambda t: t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) if t.dtype == torch.float32 else t      # noqa: E731
    for b, s in enumerate(slots):
        assert torch.equal(bits(c["kc"][b, :, s]), bits(kc2[b, :, s])) and torch.equal(bits(c["vc"][b, :, s]), bits(vc2[b, :, s])), f"row {b}: bf16 append differs"
        k8n, ksn = R.quantize_kv(c["kc"][b, :, s])
        v8n, vsn = R.quantize_kv(c["vc"][b, :, s])
        assert torch.equal(c["k8"][b, :, s], k8n) and torch.equal(c["ks"][b, :, s], ksn), f"row {b}: mirror K row {s}"
        assert torch.equal(c["v8"][b, :, s], v8n) and torch.equal(c["vs"][b, :, s], vsn), f"row {b}: mirror V row {s}"
        for k, t in before.items():      # nothing else changed: put the old row back and compare the bits (NaN poison included)
            c[k][b, :, s] = t[b, :, s]
    for k, t in before.items():
        assert torch.equal(bits(c[k]), bits(t)), f"{k}: bytes outside the appended rows changed"
