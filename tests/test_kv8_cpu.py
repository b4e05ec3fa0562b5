"""Host side of the e4m3 KV mirror (vz_hip/kv8.py), the quantiser's edge rows and the attention reference the GPU
tests hold the kernel to - all without a GPU."""
import pytest
import torch

import kv8_ref as R
from vz_hip import kv8
from vz_hip.synth import ArchConfig


def test_layout_and_memory():
    cfg = ArchConfig(n_layers=2)
    q, s = kv8.mirror_shape(cfg, 3, 512)
    assert q == (2, 2, 3, cfg.n_kv_heads, 512, 128) and s == q[:-1]
    rows = 2 * 2 * 3 * cfg.n_kv_heads * 512
    assert kv8.mirror_bytes(cfg, 3, 512) == rows * 128 + rows * 4
    assert kv8.cache_bytes(cfg, 3, 512) == rows * 128 * 2
    # + 50 % KV memory, + 1/64 for the scales
    assert kv8.mirror_bytes(cfg, 3, 512) / kv8.cache_bytes(cfg, 3, 512) == 0.5 + 1 / 64
    # the scale index of a row; its bytes start at 128 times that, the element offset of the same row in the bf16 cache
    t = torch.arange(rows).reshape(s)
    for at in [(0, 0, 0, 0, 0), (1, 1, 2, cfg.n_kv_heads - 1, 511), (0, 1, 1, 3, 77)]:
        assert kv8.row_offset(cfg, 3, 512, *at) == int(t[at])
    with pytest.raises(ValueError):
        kv8.row_offset(cfg, 3, 512, 0, 0, 3, 0, 0)
    with pytest.raises(ValueError):
        kv8.row_offset(cfg, 3, 512, 0, 2, 0, 0, 0)
    with pytest.raises(ValueError):
        kv8.mirror_shape(cfg, 0, 512)
    assert kv8.mirror_shape(cfg, 1, 64, tp_size=2)[1][3] == cfg.n_kv_heads // 2


def test_refusals():
    kv8.check_call(None, False)
    kv8.check_call(1, False)
    with pytest.raises(NotImplementedError):
        kv8.check_call(2, False)
    with pytest.raises(NotImplementedError):
        kv8.check_call(1, True)
    kv8.check_engine(1)
    with pytest.raises(NotImplementedError):
        kv8.check_engine(2)
    assert kv8.lookup_effective(True, 4) is None and kv8.lookup_effective(False, 4) == 4 and kv8.lookup_effective(False, None) is None


def test_model_takes_the_keyword():
    """the keyword reaches the engine through every constructor that builds one"""
    import inspect
    from vis_zephyr.model import VisZephyrForCausalLM
    from vis_zephyr.model.builder import load_pretrained_model
    from vz_hip.engine import Engine
    assert inspect.signature(Engine.__init__).parameters["kv_fp8"].default is False
    assert inspect.signature(VisZephyrForCausalLM.__init__).parameters["kv_fp8"].default is False
    assert inspect.signature(load_pretrained_model).parameters["kv_fp8"].default is False
    assert '"kv_fp8"' in inspect.getsource(VisZephyrForCausalLM.from_pretrained)
    assert hasattr(Engine, "set_kv_fp8")


def _row(fill: float, amax: float) -> torch.Tensor:
    x = torch.full((128,), fill)
    x[5] = -amax
    return x


def test_quantize_kv_edge_rows():
    # all zero -> scale 1, zero bytes
    q, s = R.quantize_kv(torch.zeros(2, 128))
    assert s.tolist() == [1.0, 1.0] and int(q.sum()) == 0
    # amax exactly 448 -> e = 0: 448 is e4m3's largest finite value (0x7e), sign bit set here
    q, s = R.quantize_kv(_row(1.0, 448.0))
    assert float(s) == 1.0 and int(q[5]) == 0xfe and float(R.dequant(q, s)[5]) == -448.0 and float(R.dequant(q, s)[0]) == 1.0
    # just above it (the next bf16: 450) -> the next exponent
    q, s = R.quantize_kv(_row(1.0, 450.0).bfloat16())
    assert float(s) == 2.0 and float(R.dequant(q, s)[5]) == -448.0      # 225 rounds to 224 (a tie goes to the even code)
    # 1e-3 and 1e3: e = ceil(log2(amax / 448))
    for amax, e in ((1e-3, -18), (1e3, 2)):
        x = _row(amax / 3, amax).bfloat16()
        q, s = R.quantize_kv(x)
        assert float(s) == 2.0 ** e and float(x.float().abs().max()) <= 448 * 2.0 ** e and float(x.float().abs().max()) > 448 * 2.0 ** (e - 1)
        d = R.dequant(q, s)
        assert float((d - x.float()).abs().max()) <= float(x.float().abs().max()) * 2.0 ** -4      # 3 mantissa bits: half an ulp of the top binade
        assert torch.equal(d.bfloat16().float(), d)      # exactly a bf16 number
    assert R.scale_ok(R.quantize_kv(torch.randn(64, 128) * 37.0)[1])
    # a row with one NaN is the caller's problem.  What quantize_rows does: the row's maximum is NaN, which is not > 0, so the row takes the
    # all-zero row's exponent - scale 1 whatever the finite values are - the NaN's byte is e4m3's NaN and the other values are rounded
    # at scale 1.  (The device writers take the maximum with fmaxf, which drops a NaN: they give the finite values' scale.  No cache
    # row the engine writes holds a NaN, and no test compares such a row.)
    x = _row(0.5, 3.0)
    x[9] = float("nan")
    qn, sn = R.quantize_kv(x)
    assert float(sn) == 1.0 and int(qn[9]) & 0x7f == 0x7f
    keep = torch.arange(128) != 9
    assert torch.equal(qn[keep], x[keep].to(torch.float8_e4m3fn).view(torch.uint8))


def test_reference_against_float64():
    """decode_attention_kv8_ref in fp32 against the same attention in float64 over the dequantised tensors, ragged slots and a window"""
    B, Hq, Hkv, ctx = 3, 8, 2, 96
    g = torch.Generator().manual_seed(3)
    k8, ks = R.quantize_kv(R.uneven_rows((B, Hkv, ctx), 10))
    v8, vs = R.quantize_kv(R.uneven_rows((B, Hkv, ctx), 11))
    q = torch.randn(B, Hq, 128, generator=g).bfloat16().float()
    kn = torch.randn(B, Hkv, 128, generator=g).bfloat16().float()
    vn = torch.randn(B, Hkv, 128, generator=g).bfloat16().float()
    for slots, window in (([0, 1, 95], 0), ([40, 7, 64], 8), ([95, 50, 3], 48)):
        got = R.decode_attention_kv8_ref(q, kn, vn, k8, ks, v8, vs, slots, 128 ** -0.5, window)
        for b, n in enumerate(slots):
            lo = max(0, n + 1 - window) if window > 0 else 0
            k = torch.cat([R.dequant(k8[b, :, lo:n], ks[b, :, lo:n]), kn[b].unsqueeze(1)], 1).double()
            v = torch.cat([R.dequant(v8[b, :, lo:n], vs[b, :, lo:n]), vn[b].unsqueeze(1)], 1).double()
            for h in range(Hq):
                p = torch.softmax((k[h // (Hq // Hkv)] @ q[b, h].double()) * 128 ** -0.5, 0)
                ref = p @ v[h // (Hq // Hkv)]
                assert float((got[b, h].double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max().clamp_min(1e-30)) + 1e-6
    # slots behind `slot` do not reach the result
    k8p, ksp = k8.clone(), ks.clone()
    k8p[:, :, 41:] = 0x7f
    ksp[:, :, 41:] = float("nan")
    a = R.decode_attention_kv8_ref(q, kn, vn, k8, ks, v8, vs, [40, 7, 3], 128 ** -0.5, 0)
    b = R.decode_attention_kv8_ref(q, kn, vn, k8p, ksp, v8, vs, [40, 7, 3], 128 ** -0.5, 0)
    assert torch.equal(a, b)
