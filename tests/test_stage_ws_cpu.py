"""The memory plan of the inference stages (csrc/engine.hip: carve_clip, carve_qformer, carve_prefill, carve_append, carve_decode) through
vz_op_stage_ws_bytes - no GPU needed.  Each stage has one carving function that both sizes the arena and lays it out; the query runs the
same function over a null arena.

The expectations restate, in plain Python, what the stages reserved BEFORE they had one carving each: the 256-byte-aligned running sum of
their take lists (without the `+ 256` slack each added), and vz_llm_decode_steps' closed upper bound for decode."""
import dataclasses

import pytest

TP_SIZES = (1, 2, 8)
CAP = dict(max_batch=64, max_ctx=512, max_tiles=4, max_text=64)
BF16, F32, I32, U8 = 2, 4, 4, 1


@pytest.fixture(scope="module")
def B():
    from test_abi_cpu import _ensure_built
    from vz_hip import binding
    binding.load_library(_ensure_built())
    return binding


def _arch():
    from vz_hip.synth import ArchConfig
    return ArchConfig()


def _cfg(B, tp_size, **over):
    a = _arch()
    fields = {f.name: getattr(a, f.name) for f in dataclasses.fields(a)}
    fields["clip_keep_cls"] = int(fields["clip_keep_cls"])
    fields.update(CAP, tp_size=tp_size, tp_rank=0, weight_fp8=0)
    fields.update(over)
    return B.VzConfig(**fields)


def _carved(takes):
    """Carver: every take starts at the next multiple of 256 bytes; the need is where the last one ends."""
    off = 0
    for n, size in takes:
        off = (off + 255) // 256 * 256 + n * size
    return off


def _ceil(a, b):
    return (a + b - 1) // b


def _shard(a, tp):
    """(Hq, Hkv, I, QKV, A) of one rank, as vz_engine_create derives them"""
    hq, hkv, inter = a.n_heads // tp, a.n_kv_heads // tp, a.inter // tp
    return hq, hkv, inter, (hq + 2 * hkv) * a.head_dim, hq * a.head_dim


def _clip_takes(a, T, caller_hidden):
    P, C = a.clip_patches, a.clip_hidden
    kpad = _ceil(3 * a.clip_patch * a.clip_patch, 64) * 64
    rows = T * (P + 1)
    hs_layer = rows * C
    takes = [(T * P * kpad, BF16), (T * P * C, BF16)]
    if not caller_hidden:
        takes.append((hs_layer * (a.clip_layers + 1), BF16))
    return takes + [(hs_layer, BF16), (hs_layer * 3, BF16), (hs_layer, BF16), (rows * a.clip_inter, BF16)]


def _split_rule(Sk):
    """key splits of a head_dim-512 launch over Sk keys (csrc/attention.hip, default knob 23): three 32-key tiles each from 6 tiles on; 0 = unsplit"""
    tiles = _ceil(Sk, 32)
    return _ceil(tiles, 3) if tiles >= 6 else 0


def _qformer_takes(a, T, n_samples, Lmax, kv_all, splits):
    H, NQ, KD, P = a.hidden, a.qf_queries, a.qf_kv_dim, a.clip_patches + (1 if a.clip_keep_cls else 0)
    N0, R = NQ + Lmax, T * NQ
    kv_ld = a.qf_blocks * 2 * H if kv_all else 2 * H
    part = max(T * splits(P), n_samples * splits(N0)) * a.qf_heads * NQ * (512 + 4)
    return [(T * P * KD, BF16), (T * P * kv_ld, BF16), (n_samples * N0 * H, BF16), (n_samples * N0 * H, BF16), (n_samples * N0 * 2 * H, BF16),
            (NQ * H, BF16), (n_samples * NQ * H, BF16), (n_samples * NQ * H, BF16), (R * H, BF16), (R * H, BF16), (R * 3 * H, BF16), (R * H, BF16),
            (R * 2 * H, BF16), (part, F32)]


def _prefill_takes(a, tp, Bn, S):
    _, _, inter, QKV, A = _shard(a, tp)
    H, rows = a.hidden, Bn * S
    return [(rows * H, BF16), (rows * H, BF16), (rows * QKV, BF16), (rows * A, BF16), (rows * A, BF16), (rows * inter, BF16), (rows + Bn + 16, I32),
            (Bn * H * 2, BF16), (rows * max(H, A, inter), U8), (rows, F32)]


def _append_takes(B, a, tp, Bn, T, max_ctx):
    """the six row buffers, slot[rows] | kv_len[B] | past[B] | new[B], the last rows, the key-split kernel's partials"""
    hq, hkv, inter, QKV, A = _shard(a, tp)
    H, rows = a.hidden, Bn * T
    return [(rows * H, BF16), (rows * H, BF16), (rows * QKV, BF16), (rows * A, BF16), (rows * A, BF16), (rows * inter, BF16), (rows + 3 * Bn + 16, I32),
            (Bn * H * 2, BF16), (B.attention_append_ws_floats(Bn, T, hq, hkv, max_ctx), F32)]


def _decode_takes(a, tp, Bn, spec):
    _, _, inter, QKV, A = _shard(a, tp)
    takes = [(Bn * a.hidden, BF16), (Bn * QKV, BF16), (Bn * A, BF16), (Bn * inter, BF16)]
    return takes + [(Bn * A, BF16)] if spec else takes


def _decode_bound_before(a, Bn):
    """vz_llm_decode_steps' closed formula: tp = 1 sizes, 3H pays for q_rot, 8192 for alignment"""
    return Bn * (3 * a.hidden + (a.n_heads + 2 * a.n_kv_heads) * a.head_dim + a.inter) * 2 + 8192


@pytest.mark.parametrize("tp", TP_SIZES)
def test_clip_takes_what_it_took(B, tp):
    a, cfg = _arch(), _cfg(B, tp)
    for T in (1, 3, 4):
        for caller_hidden in (False, True):
            got = B.stage_ws_bytes(cfg, B.STAGE_CLIP, T, flags=B.WS_CALLER_HIDDEN if caller_hidden else 0)
            assert got == _carved(_clip_takes(a, T, caller_hidden)), (T, caller_hidden)


@pytest.mark.parametrize("tp", TP_SIZES)
def test_qformer_takes_what_it_took_with_part_sized_by_the_split_rule(B, tp):
    a, cfg = _arch(), _cfg(B, tp)
    for T, n_samples, Lmax in ((1, 1, 0), (3, 1, 31), (4, 4, 64)):
        for kv_all in (False, True):
            got = B.stage_ws_bytes(cfg, B.STAGE_QFORMER, T, n_samples, Lmax, B.WS_QF_KV_CONTIG if kv_all else 0)
            before = _carved(_qformer_takes(a, T, n_samples, Lmax, kv_all, lambda Sk: _ceil(Sk, 96)))
            assert got == _carved(_qformer_takes(a, T, n_samples, Lmax, kv_all, _split_rule)), (T, n_samples, Lmax, kv_all)
            assert got <= before, (T, n_samples, Lmax, kv_all)


@pytest.mark.parametrize("tp", TP_SIZES)
def test_prefill_takes_what_it_took(B, tp):
    a, cfg = _arch(), _cfg(B, tp)
    for Bn, S in ((1, 1), (1, 40), (2, 96), (2, 512)):
        assert B.stage_ws_bytes(cfg, B.STAGE_PREFILL, Bn, S) == _carved(_prefill_takes(a, tp, Bn, S)), (Bn, S)


@pytest.mark.parametrize("tp", TP_SIZES)
def test_append_takes_what_it_took(B, tp):
    a, cfg = _arch(), _cfg(B, tp)
    for Bn, T in ((1, 1), (1, 20), (2, 260), (2, 512)):
        assert B.stage_ws_bytes(cfg, B.STAGE_APPEND, Bn, T) == _carved(_append_takes(B, a, tp, Bn, T, CAP["max_ctx"])), (Bn, T)
    assert B.stage_ws_bytes(cfg, B.STAGE_APPEND, 0, 8) == -1 and B.stage_ws_bytes(cfg, B.STAGE_APPEND, 1, CAP["max_ctx"] + 1) == -1


@pytest.mark.parametrize("tp", TP_SIZES)
def test_decode_takes_its_own_buffers_and_stays_inside_the_old_bound(B, tp):
    a, cfg = _arch(), _cfg(B, tp)
    for Bn, spec in [(b, False) for b in (1, 2, 5, 16, 17, 64)] + [(2, True), (8, True)]:
        got = B.stage_ws_bytes(cfg, B.STAGE_DECODE, Bn, flags=B.WS_SPEC_TAIL if spec else 0)
        assert got == _carved(_decode_takes(a, tp, Bn, spec)), (Bn, spec)
        assert got <= _decode_bound_before(a, Bn), (Bn, spec)
    plain, tail = (B.stage_ws_bytes(cfg, B.STAGE_DECODE, 2, flags=f) for f in (0, B.WS_SPEC_TAIL))
    assert tail - plain == 2 * _shard(a, tp)[4] * BF16          # one q_rot [R, A] more, nothing else


def test_refused_shapes_and_configs_answer_minus_one(B):
    cfg = _cfg(B, 1)
    last_error = B.lib().vz_last_error()
    assert B.stage_ws_bytes(cfg, B.STAGE_CLIP, 0) == -1 and B.stage_ws_bytes(cfg, B.STAGE_CLIP, CAP["max_tiles"] + 1) == -1
    assert B.stage_ws_bytes(cfg, B.STAGE_QFORMER, 0, 1, 0) == -1 and B.stage_ws_bytes(cfg, B.STAGE_QFORMER, 2, 3, 0) == -1
    assert B.stage_ws_bytes(cfg, B.STAGE_QFORMER, 1, 1, CAP["max_text"] + 1) == -1
    assert B.stage_ws_bytes(cfg, B.STAGE_PREFILL, 0, 8) == -1 and B.stage_ws_bytes(cfg, B.STAGE_PREFILL, 1, CAP["max_ctx"] + 1) == -1
    assert B.stage_ws_bytes(cfg, B.STAGE_DECODE, 0) == -1 and B.stage_ws_bytes(cfg, B.STAGE_DECODE, 65) == -1
    assert B.stage_ws_bytes(cfg, B.STAGE_DECODE, 1, flags=B.WS_SPEC_TAIL) == -1 and B.stage_ws_bytes(cfg, B.STAGE_DECODE, 9, flags=B.WS_SPEC_TAIL) == -1
    assert B.stage_ws_bytes(cfg, 4, 1) == -1
    assert B.stage_ws_bytes(_cfg(B, 3), B.STAGE_DECODE, 1) == -1            # tp_size 3 does not divide the heads: vz_engine_create refuses it
    assert B.stage_ws_bytes(_cfg(B, 1, head_dim=64), B.STAGE_PREFILL, 1, 8) == -1
    assert B.lib().vz_last_error() == last_error          # a query reports through its result: it leaves no message behind


def test_qformer_follows_the_split_knob(B):
    """knob 23 >= 2 pins the split count: the engine reserves what the launcher then asks for, not the default rule's count"""
    a, cfg = _arch(), _cfg(B, 1)
    with B.tuned(attn_split=9):
        got = B.stage_ws_bytes(cfg, B.STAGE_QFORMER, 2, 1, 31)
        assert got == _carved(_qformer_takes(a, 2, 1, 31, False, lambda Sk: min(9, _ceil(Sk, 32)) if _ceil(Sk, 32) >= 2 else 0))
    with B.tuned(attn_split=1):
        assert B.stage_ws_bytes(cfg, B.STAGE_QFORMER, 2, 1, 31) == _carved(_qformer_takes(a, 2, 1, 31, False, lambda Sk: 0))
