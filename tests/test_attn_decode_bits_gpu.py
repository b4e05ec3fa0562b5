"""The one-launch decode attention (csrc/attn_decode_body.h: body<>, shared by attn_decode.hip, attn_o_fused.hip and decode_persist.hip)
bit for bit against the commit before its head and merge were turned into single batches of loads.

1. torch.equal with tests/golden/attn_decode_parent_bits.npz, which tools/dump_attn_decode_bits.py wrote on the parent commit (its CASES
   are the list: 1 .. 32 splits, the direct path and the ticket path, several chunks per split, a window, ragged rows, a cache that is
   exactly full, a second call on the same ticket buffer).  Cache rows >= len and row `slot` itself hold NaN bit patterns before each
   call: the reference never read them, and a clamped or unconditional load of one that reaches a result turns it non-finite.
2. The fused attention + O launch on the 2-layer engine at S = 2900 and 3990 (23 and 32 splits; tests/test_persist_gpu.py stops at 2200)
   against the two launches (knob 30 (attn_o) = 0): logits and ids EQUAL, eager and through the captured graph, check_async() clean."""
import os
import sys

import numpy as np
import pytest
import torch

from util import GOLDEN, REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import dump_attn_decode_bits as D  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from vz_hip import binding
    binding.load_library()
    return binding


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "attn_decode_parent_bits.npz"))


@pytest.mark.parametrize("name", list(D.CASES))
def test_bits_equal_the_parent_commit(B, golden, name):
    o, k, v = D.run_case(B, name, D.make_inputs(name))
    for key, got in (("o", o), ("k", k), ("v", v)):
        assert torch.isfinite(got.float()).all(), f"{name}.{key}: non-finite (a poisoned cache row reached the result)"
        want = torch.from_numpy(golden[f"{name}.{key}"].view(np.int16)).to(got.device)
        assert want.shape == got.shape, (name, key, tuple(want.shape), tuple(got.shape))
        same = torch.equal(got.contiguous().view(torch.int16), want)
        assert same, f"{name}.{key}: {int((got.contiguous().view(torch.int16) != want).sum())} of {want.numel()} values differ from the parent commit's bits"


@pytest.fixture(scope="module")
def long_ctx():
    from vz_hip import synth
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    cfg = synth.ArchConfig(n_layers=2)
    hf = VisZephyrConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=2, num_attention_heads=cfg.n_heads,
                         num_key_value_heads=cfg.n_kv_heads, vocab_size=cfg.vocab, rms_norm_eps=cfg.rms_eps, rope_theta=cfg.rope_theta,
                         sliding_window=cfg.sliding_window, eos_token_id=2, pad_token_id=2, bos_token_id=1)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    hf.mm_hidden_size = 5120
    model = VisZephyrForCausalLM.from_synthetic(hf, seed=0, max_batch=1, max_ctx=4096, max_tiles=1, max_text=4096)
    yield cfg, synth, model
    del model
    torch.cuda.empty_cache()


@pytest.mark.parametrize("S", [2900, 3990])
def test_fused_attention_o_launch_at_long_contexts(B, long_ctx, S):
    cfg, synth, model = long_ctx
    eng = model.engine
    emb = eng.embed_tokens(synth.synth_ids(S, cfg.vocab, image_pos=-1, seed=700 + S).unsqueeze(0))
    res = {}
    for fused in (1, 0):
        with B.tuned(attn_o=fused):
            _, last = eng.prefill(emb, [S], all_logits=False, last_logits=True)
            eng.decode_begin(last.argmax(-1).to(torch.int32), [S], [S])
            ids, lg = eng.decode_steps(5, return_logits=True)
            _, last = eng.prefill(emb, [S], all_logits=False, last_logits=True)
            eng.decode_begin(last.argmax(-1).to(torch.int32), [S], [S])
            ids_g = eng.decode_steps(12)
            torch.cuda.synchronize()
            eng.check_async()
            res[fused] = (ids[0].clone(), lg[:, 0].clone(), ids_g[0].clone())
    assert torch.isfinite(res[1][1]).all()
    assert torch.equal(res[1][0], res[0][0]) and torch.equal(res[1][2], res[0][2])
    assert torch.equal(res[1][1], res[0][1]), f"S={S}: max |diff| {float((res[1][1] - res[0][1]).abs().max()):.3e}"
