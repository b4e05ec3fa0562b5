"""The host side of the shared prompt KV (vz_hip/share.py): the plan's arithmetic and refusals, the arming scope,
the workspace rule of the built library, and the tests' own reference against a brute-force float64 loop.  No GPU."""
import math

import pytest
import torch

from share_ref import copied_cache, shared_attention_ref, visible
from test_decode_loop_cpu import RecordingEngine
from vz_hip import decode_loop as DL
from vz_hip import share as SH


def test_plan_arithmetic():
    p = SH.plan([40, 17], 3, 8, 256, 4096, max_batch=6)
    assert p.n == 3 and p.shared == [40, 17] and p.rows == 6
    assert SH.plan([248], 2, 8, 256).shared == [248]                   # prompt + max_new == max_ctx still fits
    assert SH.plan([1] * 32, 2, 1, 8).rows == 64


def test_plan_refusals():
    with pytest.raises(ValueError):
        SH.plan([40], 1, 8, 256)                                       # one row per group shares nothing
    with pytest.raises(NotImplementedError):
        SH.plan([40], 65, 8, 256, max_batch=128)                       # more rows per group than the kernels take
    with pytest.raises(ValueError):
        SH.plan([], 2, 8, 256)
    with pytest.raises(ValueError):
        SH.plan([40, 0], 2, 8, 256)                                    # an empty prompt
    with pytest.raises(ValueError):
        SH.plan([249], 2, 8, 256)                                      # prompt + max_new past the cache
    with pytest.raises(ValueError):
        SH.plan([40, 17], 4, 8, 256, max_batch=6)                      # 8 rows, the batch holds 6
    with pytest.raises(ValueError):
        SH.plan([40] * 5, 16, 8, 256, max_batch=128)                   # 80 rows, a decode batch holds 64
    with pytest.raises(ValueError):
        SH.plan([40], 2, 0, 256)


def test_call_refusals():
    ok = dict(num_return_sequences=4, num_beams=1, guidance=False, past_key_values=False, prompt_lookup=None, tp_size=1)
    SH.check_call(**ok)
    for bad in (dict(num_beams=2), dict(guidance=True), dict(past_key_values=True), dict(prompt_lookup=3), dict(tp_size=2),
                dict(num_return_sequences=1), dict(num_return_sequences=None)):
        with pytest.raises(NotImplementedError):
            SH.check_call(**{**ok, **bad})


def test_fan_share_moves_nothing():
    eng = RecordingEngine()
    pos = torch.tensor([[0, 1, 2, 7, 9], [0, 1, 5, 0, 0]])
    assert DL.fan_share(eng, [5, 3], None, 2) == ([5, 5, 3, 3], [5, 5, 3, 3])
    assert DL.fan_share(eng, [5, 3], pos, 2) == ([10, 10, 6, 6], [5, 5, 3, 3])
    assert eng.log == []                                               # no engine call at all: no kv_move_rows


@pytest.mark.parametrize("fail", [None, ("decode_steps", 1), ("set_share", 1)])
def test_armed_share_order(fail):
    """the plan is armed last, in front of decode_begin, and disarmed first - whatever happens inside"""
    eng = RecordingEngine(fail)
    plan = SH.plan([5, 3], 2, 4, 64)
    first = torch.tensor([5, 6, 7, 8], dtype=torch.int32)

    def run():
        with DL.armed(eng, proc="PROC", sampling_rows=["ROW"] * 4, stop="PLAN", share=plan) as begin:
            begin(first, [5, 5, 3, 3], [5, 5, 3, 3])
            eng.decode_steps(1)

    if fail is None:
        run()
    else:
        with pytest.raises(RuntimeError):
            run()
    on = [("set_logits_proc", "PROC"), ("set_sampling_rows", ["ROW"] * 4), ("set_stop", "PLAN")]
    off = [("set_stop", None), ("set_sampling_rows", None), ("set_logits_proc", None)]
    if fail == ("set_share", 1):          # the arming itself failed: nothing of it to undo, no batch begun
        assert eng.log == on + [("set_share", plan)] + off
    else:
        assert eng.log == on + [("set_share", plan), ("decode_begin", first, [5, 5, 3, 3], [5, 5, 3, 3]), ("stop_rows", 0, first),
                                ("decode_steps", 1), ("set_share", None)] + off


def test_plain_scope_never_touches_share():
    eng = RecordingEngine()
    with DL.armed(eng, sampling_rows=["ROW"]) as begin:
        begin(torch.tensor([1]), [2], [2])
    assert all(c[0] != "set_share" for c in eng.log)


def _ws(R, n, Hq, Hkv, max_ctx):
    """the rule of csrc/attn_shared.hip, written out: splits for two workgroups per CU (512), at most the 64-key tiles, at most 64"""
    if R < 1 or n < 2 or n > 64 or R % n or Hkv < 1 or Hq < Hkv or Hq % Hkv or 16 % (Hq // Hkv) or max_ctx < 1:
        return 0
    base = (R // n) * Hkv * ((n * (Hq // Hkv) + 63) // 64)
    nsplit = max(1, min(max(1, 512 // base), (max_ctx + 63) // 64, 64))
    return R * Hq * nsplit * 132


def test_ws_floats_host_arithmetic():
    from vz_hip import binding as B
    B.load_library()
    for R, n, Hq, Hkv, ctx in [(64, 16, 32, 8, 4096), (64, 64, 32, 8, 4096), (16, 2, 32, 8, 256), (6, 3, 32, 8, 256), (4, 4, 32, 8, 64),
                               (64, 2, 32, 8, 8192), (2, 2, 8, 8, 100000), (34, 17, 32, 8, 512), (4, 2, 16, 4, 1)]:
        assert B.attention_shared_ws_floats(R, n, Hq, Hkv, ctx) == _ws(R, n, Hq, Hkv, ctx) > 0, (R, n, Hq, Hkv, ctx)
    for bad in [(4, 1, 32, 8, 256), (65, 65, 32, 8, 256), (5, 2, 32, 8, 256), (0, 2, 32, 8, 256), (4, 2, 32, 5, 256), (4, 2, 32, 8, 0),
                (4, 2, 24, 8, 256)]:
        assert B.attention_shared_ws_floats(*bad) == 0, bad
    assert _ws(64, 16, 32, 8, 4096) == 64 * 32 * 16 * 132              # 4 prompts x 16 samples: 32 base workgroups -> 16 splits


def _brute(q, kc, vc, n, shared, slot, scale, window):
    R, Hq, D = q.shape
    G = Hq // kc.shape[1]
    out = torch.zeros(R, Hq, D, dtype=torch.float64)
    for r in range(R):
        g, sl = r // n, slot[r]
        sh = shared[g] if sl >= shared[g] else 0
        for h in range(Hq):
            keys = []
            for j in range(sl + 1):
                if window > 0 and j <= sl - window:
                    continue
                keys.append((g * n if j < sh else r, j))
            s = [scale * sum(float(q[r, h, d]) * float(kc[row, h // G, j, d]) for d in range(D)) for row, j in keys]
            m = max(s)
            w = [math.exp(v - m) for v in s]
            for (row, j), wk in zip(keys, w):
                out[r, h] += wk / sum(w) * vc[row, h // G, j].double()
    return out


@pytest.mark.parametrize("window", [0, 3, 5])
def test_reference_against_brute_force(window):
    n, shared, slot = 2, [4, 2], [6, 4, 1, 5]          # row 2 sits in front of its group's shared slots
    g = torch.Generator().manual_seed(window)
    q = torch.randn(4, 4, 8, generator=g).bfloat16()
    kc = torch.randn(4, 2, 8, 8, generator=g).bfloat16()
    vc = torch.randn(4, 2, 8, 8, generator=g).bfloat16()
    ref = shared_attention_ref(q, kc, vc, n, shared, slot, 0.35, window)
    want = _brute(q, kc, vc, n, shared, slot, 0.35, window)
    assert float((ref.double() - want).abs().max()) < 1e-5
    assert visible(1, n, shared, slot) == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 4)]
    assert visible(2, n, shared, slot) == [(2, 0), (2, 1)]
    assert visible(3, n, shared, slot, 3) == [(3, 3), (3, 4), (3, 5)] and visible(3, n, shared, slot, 5) == [(2, 1), (3, 2), (3, 3), (3, 4), (3, 5)]
    # on the copy route's cache every row reads its own row only: the same numbers
    kcc, vcc = copied_cache(kc, vc, n, shared)
    own = _brute(q, kcc, vcc, 1, [0] * 4, slot, 0.35, window)
    live = [r for r in range(4) if slot[r] >= shared[r // n]]
    assert float((own[live] - want[live]).abs().max()) < 1e-12
