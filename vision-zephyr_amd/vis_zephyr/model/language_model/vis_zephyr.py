"""VisZephyrForCausalLM for MI355X: the reference's model API
(ref:vis_zephyr/model/language_model/vis_zephyr.py:19-174) on top of the native engine.

The reference class IS an HF `MistralForCausalLM` and delegates generation to `GenerationMixin`.
This one owns a `vz_hip.Engine` (weights + KV cache in HBM, hand-written HIP kernels) and implements
`forward` / `generate` itself with the same observable contract:

  * forward(input_ids|inputs_embeds, images=...) -> object with .loss/.logits/.past_key_values;
    logits for ALL positions, fp32, [B,S,vocab] (what the reference's forward returns).
  * generate(input_ids, images=..., images_size=..., do_sample, temperature, top_p, max_new_tokens,
    eos_token_id, pad_token_id, streamer, stopping_criteria, use_cache) -> LongTensor [B, n_new]
    holding NEW tokens only (HF semantics when generation starts from inputs_embeds; Appendix A Q6).
    streamer.put()/end() and stopping_criteria(ids, scores) are invoked once per token, as HF does.
  * `inputs_embeds=` passed to generate raises NotImplementedError (ref :113-114).
"""
from __future__ import annotations

import time
from types import SimpleNamespace
from typing import List, Optional, Sequence, Union

import torch

from vz_hip import decode_loop as DL
from vz_hip.engine import Engine
from vz_hip.synth import ArchConfig

from ..vis_zephyr_arch import VisZephyrMetaForCausalLM, VisZephyrMetaModel

try:                                    # configuration class only - no HF modelling code on this path
    from transformers import MistralConfig as _BaseConfig
except Exception:                       # pragma: no cover - transformers absent
    class _BaseConfig:                  # minimal stand-in with attribute storage
        def __init__(self, **kw):
            for k, v in kw.items():
                setattr(self, k, v)


class VisZephyrConfig(_BaseConfig):
    model_type = "vis_zephyr"


def arch_from_config(config) -> ArchConfig:
    g = lambda k, d: getattr(config, k, d) if getattr(config, k, d) is not None else d  # noqa: E731
    hidden = g("hidden_size", 4096)
    heads = g("num_attention_heads", 32)
    return ArchConfig(hidden=hidden, inter=g("intermediate_size", 14336), n_layers=g("num_hidden_layers", 32),
                      n_heads=heads, n_kv_heads=g("num_key_value_heads", 8), head_dim=g("head_dim", hidden // heads),
                      vocab=g("vocab_size", 32000), rms_eps=g("rms_norm_eps", 1e-5),
                      rope_theta=float(g("rope_theta", 10000.0)), sliding_window=g("sliding_window", 4096),
                      # 'cls_patch' keeps the class token: 577 visual tokens per tile (ref vision_encoder.py:66-73)
                      clip_keep_cls=g("mm_vision_select_feature", "patch") == "cls_patch")


class _Embedding:
    """`model.get_model().embed_tokens(ids)` (ref vis_zephyr_arch.py:170,211,248,275)."""

    def __init__(self, owner):
        self._owner = owner

    def __call__(self, ids):
        self._owner._ensure_ready()
        return self._owner.engine.embed_tokens(ids)

    @property
    def weight(self):
        return self._owner.engine.w["llm.embed"]


class _LMHead:
    def __init__(self, owner):
        self._owner = owner

    @property
    def weight(self):
        return self._owner.engine.w["llm.lm_head"]

    def __call__(self, hidden):
        from vz_hip import binding as B
        h = hidden.to(self._owner.device, torch.bfloat16)
        return B.linear(h.reshape(-1, h.shape[-1]).contiguous(), self.weight, out_fp32=True).view(*h.shape[:-1], -1)


class VisZephyrModel(VisZephyrMetaModel):
    """`model.get_model()`: embed_tokens + vision tower + projector (ref vis_zephyr.py:22-26)."""
    config_class = VisZephyrConfig

    def __init__(self, config, owner):
        self.config = config
        self.embed_tokens = _Embedding(owner)
        self._init_vision(config, owner)


class PastKeyValues:
    """The KV cache lives in the engine ([layer][k|v][slot][kv_head][pos][128] bf16); this handle records how
    many positions of each slot are filled.  A handle that generate() returns also remembers the ids those positions stand for
    (the prompt ids as given - an image is one id - plus every emitted id but the last) and each row's next rotary position, so that
    generate(<the whole conversation>, past_key_values=handle) can tell the cached part from the new one (vz_hip/append.py)."""

    def __init__(self, lengths: Sequence[int], owner=None, epoch: int = 0, continuable: bool = False, ids=None, next_pos=None):
        self.lengths = list(lengths)
        self.ids = None if ids is None else [list(r) for r in ids]
        self.next_pos = None if next_pos is None else list(next_pos)
        # which model's cache this describes and at which point of its history: the engine owns ONE cache, so a handle is live only
        # until the next forward / generate (forward(past_key_values=...) checks it)
        self.owner, self.epoch, self.continuable = owner, epoch, continuable

    def get_seq_length(self, layer_idx: int = 0):
        return max(self.lengths) if self.lengths else 0


class VisZephyrForCausalLM(VisZephyrMetaForCausalLM):
    config_class = VisZephyrConfig

    def __init__(self, config, device: Union[str, torch.device] = "cuda:0", max_batch: int = 1,
                 max_ctx: int = 4096, max_tiles: int = 8, max_text: int = 2048, engine: Optional[Engine] = None,
                 tp_size: int = 1, tp_rank: int = 0, weight_fp8: bool = False, weight_nf4: bool = False, kv_fp8: bool = False):
        self.config = config
        self.arch = arch_from_config(config)
        self.engine = engine if engine is not None else Engine(self.arch, device=device, max_batch=max_batch,
                                                               max_ctx=max_ctx, max_tiles=max_tiles,
                                                               max_text=max_text, tp_size=tp_size, tp_rank=tp_rank,
                                                               weight_fp8=weight_fp8, weight_nf4=weight_nf4, kv_fp8=kv_fp8)
        self.device = self.engine.device
        self.dtype = torch.bfloat16
        self.model = VisZephyrModel(config, self)
        self.lm_head = _LMHead(self)
        # hf:generation/configuration_utils.py (pinned 4.52.4) defaults that the reference's callers rely on without naming them:
        # do_sample=True with only `temperature` passed (ref:vis_zephyr/serve/cli.py:171-182) still goes through TopKLogitsWarper(50)
        self.generation_config = SimpleNamespace(eos_token_id=getattr(config, "eos_token_id", 2),
                                                 pad_token_id=getattr(config, "pad_token_id", None), top_k=50, top_p=1.0,
                                                 temperature=1.0)
        self._ring = None
        self._kv_epoch = 0            # bumped by everything that rewrites the engine's KV cache: cache handles of earlier calls go stale

    # ---- construction helpers -------------------------------------------------------------------
    @classmethod
    def from_synthetic(cls, config, seed: int = 0, **kw):
        m = cls(config, **kw)
        m.engine.load_synthetic(seed)
        m.engine.init_comm()
        if m.get_vision_tower() is not None:
            m.get_vision_tower().is_loaded = True
        return m

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *model_args, config=None, low_cpu_mem_usage=True, torch_dtype=None,
                        device_map=None, device="cuda:0", **kw):
        """HF's entry point with the reference's usage (ref:vis_zephyr/model/builder.py:108-129): a directory or a hub id
        resolved through the LOCAL cache; `config=` overrides the directory's config.json (the base + mm_projector.bin mode
        passes the finetuned config while the weights come from the Zephyr base).  Streams every weight file of the directory
        into the engine; what the directory lacks (mm_projector.bin arrives through `load_state_dict`, the CLIP tower through
        `get_vision_tower().load_model()`) is completed later - the engine is finalized at first use."""
        import json
        import os
        from vz_hip import weights as W
        path = W.resolve_hub_path(pretrained_model_name_or_path, "pretrained_model_name_or_path")
        if config is None:
            with open(os.path.join(path, "config.json")) as f:
                d = json.load(f)
            for k in ("model_type", "architectures", "transformers_version"):
                d.pop(k, None)
            config = VisZephyrConfig(**d)
        if isinstance(device_map, dict) and "" in device_map:          # ref builder.py:29-31: device_map = {"": device}
            device = device_map[""]
        dev = "cuda:0" if str(device) == "cuda" else device
        engine_kw = {k: kw.pop(k) for k in ("max_batch", "max_ctx", "max_tiles", "max_text", "tp_size", "tp_rank", "weight_fp8", "weight_nf4", "kv_fp8") if k in kw}
        model = cls(config, device=dev, **engine_kw)
        for name, t in W.iter_backbone(path):
            model.engine.add_weight(name, t)
        return model

    def load_state_dict(self, state_dict, strict: bool = True):
        """`model.load_state_dict(mm_projector_weights, strict=False)` (ref builder.py:121-123): reference-named tensors into
        the engine.  Returns HF's (missing_keys, unexpected_keys) shape with the keys the engine does not take."""
        from vz_hip import weights as W
        unexpected = [k for k, v in W.normalize_keys(state_dict.items()) if not self.engine.add_weight(k, v)]
        if strict and unexpected:
            raise RuntimeError(f"Unexpected key(s) in state_dict: {unexpected[:8]}")
        return SimpleNamespace(missing_keys=[], unexpected_keys=unexpected)

    def _ensure_ready(self):
        """finalize lazily: weights may arrive in several steps (from_pretrained, load_state_dict, the tower's load_model);
        the C side names the first missing tensor if something never arrived."""
        if not self.engine.ready:
            self.engine.finalize()
            self.engine.init_comm()

    def load_state_dict_stream(self, named_tensors):
        """feed (reference key, tensor) pairs - e.g. safetensors shards + mm_projector.bin
        (ref:vis_zephyr/model/builder.py:102-138)."""
        self.engine.load_weights(named_tensors)

    # nn.Module-flavoured no-ops the reference's callers invoke
    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def half(self):
        return self

    def get_model(self):
        return self.model

    def resize_token_embeddings(self, n: int):
        """ref:vis_zephyr/model/builder.py:141-153 grows embed_tokens / lm_head by `<im_patch>`; new rows are
        the mean of the old ones (HF mean-resizing)."""
        old = self.arch.vocab
        if n is None or n == old:
            return self.model.embed_tokens
        self.engine.resize_vocab(int(n))
        self.arch = self.engine.cfg
        self.config.vocab_size = int(n)
        return self.model.embed_tokens

    # ---- forward (a2) -----------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None,
                inputs_embeds=None, labels=None, use_cache=None, output_attentions=None,
                output_hidden_states=None, images=None, images_size=None, return_dict=None, **kwargs):
        self._ensure_ready()
        if past_key_values is not None:
            return self._forward_continue(input_ids, attention_mask, position_ids, past_key_values, inputs_embeds, labels, images)
        if inputs_embeds is None:
            (input_ids, position_ids, attention_mask, past_key_values, inputs_embeds, labels) = \
                self.prepare_inputs_labels_for_multimodal(input_ids, position_ids, attention_mask, past_key_values,
                                                          labels, images, images_size)
        if inputs_embeds is None:
            inputs_embeds = self.get_model().embed_tokens(input_ids)
        Bsz, S = inputs_embeds.shape[0], inputs_embeds.shape[1]
        inputs_embeds, rp_mask, position_ids, shifts = self._to_right_padded(inputs_embeds, attention_mask, position_ids)
        seqlens = self._seqlens(rp_mask, Bsz, S)
        logits = torch.empty(Bsz, S, self.arch.vocab, dtype=torch.float32, device=self.device)
        mb = self.engine.max_batch
        for b0 in range(0, Bsz, mb):        # the engine owns `max_batch` KV slots; larger batches run in chunks
            sl = slice(b0, min(Bsz, b0 + mb))
            la, _ = self.engine.prefill(inputs_embeds[sl], seqlens[sl], None if position_ids is None else position_ids[sl],
                                        all_logits=True, last_logits=False)
            logits[sl] = la
        if shifts is not None:              # back to the caller's (left-padded) column order
            logits = torch.stack([torch.roll(logits[b], shifts[b], 0) for b in range(Bsz)])
        loss = None
        if labels is not None:
            from vz_hip import binding as B
            lab = labels.to(logits.device)
            loss, _ = B.causal_lm_loss(logits.contiguous(), lab)      # hf ForCausalLMLoss on the device (shift, ignore -100, mean over valid)
        self._kv_epoch += 1
        return SimpleNamespace(loss=loss, logits=logits, past_key_values=PastKeyValues(seqlens, self, self._kv_epoch, shifts is None and Bsz <= mb),
                               hidden_states=None, attentions=None)

    def _check_handle(self, past_key_values, who: str):
        if not isinstance(past_key_values, PastKeyValues) or past_key_values.owner is not self or past_key_values.epoch != self._kv_epoch:
            raise ValueError(f"{who}(past_key_values=...): this cache handle is stale - the engine owns ONE cache, and a later forward / "
                             "generate call has overwritten it")
        if not past_key_values.continuable:
            raise NotImplementedError(f"{who}(past_key_values=...) after a left-padded or chunked batch: re-run the prompt right-padded")

    def _forward_continue(self, input_ids, attention_mask, position_ids, past_key_values, inputs_embeds, labels, images):
        """forward(input_ids [B, T], past_key_values=<handle of the previous forward>): HF's step API (hf:models/mistral/modeling_mistral.py
        forward with a cache).  The KV cache is the engine's, so only the handle of the LATEST forward on this model is live; the new
        tokens run on top of it (teacher-forced), logits [B, T, V] and a handle T positions longer come back.  Fewer than
        `vz_hip.append.APPEND_MIN_NEW` new tokens run as decode steps; from there on ONE append prefill (`Engine.prefill_append`, DESIGN.md
        section 6l) puts all T behind the cache in a single weight sweep.  Rows may differ in cached length."""
        self._check_handle(past_key_values, "forward")
        if images is not None or inputs_embeds is not None or labels is not None or input_ids is None:
            raise NotImplementedError("forward(past_key_values=...) takes new input_ids only (the decode step embeds token ids on the device)")
        from vz_hip.append import APPEND_MIN_NEW
        ids = input_ids.to(self.device)
        Bsz, T = ids.shape
        if Bsz != len(past_key_values.lengths):
            raise ValueError(f"forward(past_key_values=...): {Bsz} rows of new tokens for a cache of {len(past_key_values.lengths)} rows")
        if attention_mask is not None and not bool(attention_mask[:, -T:].bool().all()):
            raise NotImplementedError("forward(past_key_values=...): padded new tokens")
        lens = list(past_key_values.lengths)
        if max(lens) + T > self.engine.max_ctx:
            raise ValueError(f"forward(past_key_values=...): {max(lens) + T} positions exceed max_ctx = {self.engine.max_ctx}")
        pos0 = lens if past_key_values.next_pos is None else list(past_key_values.next_pos)
        if T >= APPEND_MIN_NEW:
            if self.engine.tp_size > 1:
                raise NotImplementedError(f"forward(past_key_values=...) with {T} >= {APPEND_MIN_NEW} new tokens on a tensor-parallel engine is not built")
            pos = position_ids if position_ids is not None else \
                torch.tensor([[p + t for t in range(T)] for p in pos0], dtype=torch.int32)
            if int(pos.max()) >= self.engine.max_ctx:
                raise ValueError(f"forward(past_key_values=...): rotary position {int(pos.max())} exceeds max_ctx = {self.engine.max_ctx}")
            out, _ = self.engine.prefill_append(0, self.get_model().embed_tokens(ids), [T] * Bsz, lens, pos, all_logits=True, last_logits=False)
        else:
            out = torch.empty(Bsz, T, self.arch.vocab, dtype=torch.float32, device=self.device)
            for t in range(T):
                pos = [int(position_ids[b, t]) for b in range(Bsz)] if position_ids is not None else [p + t for p in pos0]
                self.engine.decode_begin(ids[:, t].to(torch.int32).contiguous(), pos, [l + t for l in lens])
                _, lg = self.engine.decode_steps(1, return_logits=True)
                out[:, t] = lg[0]
        self._kv_epoch += 1
        nxt = [int(position_ids[b, -1]) + 1 for b in range(Bsz)] if position_ids is not None else [p + T for p in pos0]
        known = None if past_key_values.ids is None else [r + ids[b].tolist() for b, r in enumerate(past_key_values.ids)]
        return SimpleNamespace(loss=None, logits=out,
                               past_key_values=PastKeyValues([l + T for l in lens], self, self._kv_epoch, True, known, nxt),
                               hidden_states=None, attentions=None)

    __call__ = forward

    @staticmethod
    def _seqlens(attention_mask, Bsz, S) -> List[int]:
        if attention_mask is None:
            return [S] * Bsz
        m = attention_mask.bool().cpu()
        lens = m.sum(1).tolist()
        for b in range(Bsz):
            if not bool(m[b, :lens[b]].all()):
                raise NotImplementedError("attention mask is neither right- nor left-padded (holes are not built)")
        return [max(1, int(x)) for x in lens]

    @staticmethod
    def _to_right_padded(inputs_embeds, attention_mask, position_ids):
        """The engine's KV cache holds every sequence from slot 0 (right padding).  A left-padded batch
        (`tokenizer_padding_side = "left"`, ref:vis_zephyr/model/vis_zephyr_arch.py:515-521) is rolled so that each row's
        real tokens start at column 0; returns the shifts so that per-position outputs can be rolled back."""
        if attention_mask is None:
            return inputs_embeds, attention_mask, position_ids, None
        m = attention_mask.bool()
        Bsz, S = m.shape
        lens = m.sum(1)
        is_left = [bool(lens[b] < S and m[b, S - int(lens[b]):].all() and not m[b, 0]) for b in range(Bsz)]
        if not any(is_left):
            return inputs_embeds, attention_mask, position_ids, None
        shifts = [S - int(lens[b]) if is_left[b] else 0 for b in range(Bsz)]
        emb = torch.stack([torch.roll(inputs_embeds[b], -shifts[b], 0) for b in range(Bsz)])
        msk = torch.stack([torch.roll(attention_mask[b], -shifts[b], 0) for b in range(Bsz)])
        pos = None if position_ids is None else torch.stack([torch.roll(position_ids[b], -shifts[b], 0) for b in range(Bsz)])
        return emb, msk, pos, shifts

    # ---- generate (a3, a13) -------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, input_ids: Optional[torch.Tensor] = None, images=None, images_size=None, **kwargs):
        self._ensure_ready()
        if self.engine.kv_fp8:      # the e4m3 KV mirror (vz_hip/kv8.py): what its step does not build is refused before anything runs
            from vz_hip import kv8 as KV8
            KV8.check_call(kwargs.get("num_beams"), bool(kwargs.get("share_prompt_kv")))
            if "prompt_lookup_num_tokens" in kwargs:      # without effect: the plain path
                kwargs["prompt_lookup_num_tokens"] = KV8.lookup_effective(True, kwargs["prompt_lookup_num_tokens"])
        if kwargs.get("share_prompt_kv"):      # what the shared-prefix route does not build is refused here, before anything runs
            from vz_hip import share as SH
            scale = kwargs.get("guidance_scale", getattr(self.generation_config, "guidance_scale", None))
            SH.check_call(kwargs.get("num_return_sequences"), kwargs.get("num_beams"),
                          (scale is not None and scale != 1) or kwargs.get("negative_prompt_ids") is not None,
                          kwargs.get("past_key_values") is not None, kwargs.get("prompt_lookup_num_tokens"), self.engine.tp_size)
        if kwargs.get("past_key_values") is not None:
            return self._generate_continue(input_ids, kwargs.pop("past_key_values"), kwargs)
        kwargs.pop("past_key_values", None)
        self._kv_epoch += 1
        position_ids = kwargs.pop("position_ids", None)
        attention_mask = kwargs.pop("attention_mask", None)
        if "inputs_embeds" in kwargs:
            raise NotImplementedError("`inputs_embeds` is not supported in this generate function.")
        mask_in = attention_mask
        if kwargs.get("return_dict_in_generate") and input_ids is not None:      # what the returned cache handle remembers (vz_hip/append.py)
            from vz_hip import append as AP
            kwargs["_prompt_rows"] = lambda: AP.masked_rows(input_ids, mask_in)
        neg = self._negative_branch(input_ids, kwargs)
        if neg is not None:
            kwargs["_guidance"] = neg
        if images is not None:
            (_, position_ids, attention_mask, _, inputs_embeds, _) = self.prepare_inputs_labels_for_multimodal(
                input_ids, position_ids, attention_mask, None, None, images, images_size)
            if inputs_embeds is None:       # single-token prompt: the reference's early-out returns the ids untouched
                inputs_embeds = self.get_model().embed_tokens(input_ids)
        else:
            inputs_embeds = self.get_model().embed_tokens(input_ids)
        if kwargs.get("prompt_lookup_num_tokens") and input_ids is not None and input_ids.shape[0] == 1:
            # built only once the call is known to run with drafts (_generate_from_embeds): every other call stays as it was
            kwargs["_spec_history"] = lambda: self._spec_history(input_ids, mask_in, images, inputs_embeds.shape[1])
        return self._generate_from_embeds(inputs_embeds, attention_mask, position_ids, **kwargs)

    def _generate_continue(self, input_ids, handle, kwargs):
        """generate(input_ids=<the whole conversation so far>, past_key_values=<the handle the previous call returned>): HF's way to
        continue a conversation.  The cached positions stay as they were computed (the reference re-conditions the Q-Former on the whole
        conversation every turn; a caller who hands over a cache gets HF's semantics instead - DESIGN.md section 6l); only the new ids
        are embedded and put behind them by one append prefill, and the call goes on as any other from the first token.  `images` is
        ignored: the cached part holds them, as HF drops pixel values after its first step."""
        from vz_hip import append as AP
        from vis_zephyr.constants import IMAGE_TOKEN_INDEX
        self._check_handle(handle, "generate")
        eng = self.engine
        if "inputs_embeds" in kwargs:
            raise NotImplementedError("`inputs_embeds` is not supported in this generate function.")
        if (kwargs.get("num_beams") or 1) != 1:
            raise NotImplementedError("generate(past_key_values=...) with num_beams > 1 is not built: the beams' rows start from one prompt prefill")
        scale = kwargs.get("guidance_scale", getattr(self.generation_config, "guidance_scale", None))
        if (scale is not None and scale != 1) or kwargs.get("negative_prompt_ids") is not None:      # (checked before anything is embedded)
            raise NotImplementedError("generate(past_key_values=...) with guidance_scale is not built: the negative prompt's cache row is not kept")
        for k in ("guidance_scale", "negative_prompt_ids", "negative_prompt_attention_mask", "negative_images", "negative_images_size"):
            kwargs.pop(k, None)
        if (kwargs.get("num_return_sequences") or 1) != 1:
            raise NotImplementedError("generate(past_key_values=...) with num_return_sequences > 1 is not built: one cache row per conversation is kept")
        if eng.tp_size > 1:
            raise NotImplementedError("generate(past_key_values=...) on a tensor-parallel engine is not built")
        if input_ids is None or input_ids.shape[0] > min(eng.max_batch, 64):
            raise NotImplementedError(f"generate(past_key_values=...) needs input_ids of at most max_batch = {min(eng.max_batch, 64)} rows")
        attention_mask = kwargs.pop("attention_mask", None)
        kwargs.pop("position_ids", None)          # the cached part fixes every row's positions
        rows = AP.masked_rows(input_ids, attention_mask)
        plan = AP.plan(rows, handle.lengths, handle.ids, handle.next_pos, IMAGE_TOKEN_INDEX)
        Bsz, T = len(rows), plan.width          # (the handle goes stale in `_generate_from_embeds`, behind that function's own refusals)
        ids = torch.zeros(Bsz, T, dtype=torch.long)
        mask = torch.zeros(Bsz, T, dtype=torch.long)
        for b, new in enumerate(plan.suffix):
            ids[b, :len(new)] = torch.tensor(new, dtype=torch.long)
            mask[b, :len(new)] = 1
        pos = torch.tensor([[min(p + t, eng.max_ctx - 1) for t in range(T)] for p in plan.next_pos], dtype=torch.int32)      # (padding stays inside the rotary tables)
        kwargs["_prompt_rows"] = lambda: rows
        return self._generate_from_embeds(self.get_model().embed_tokens(ids.to(self.device)), mask.to(self.device), pos.to(self.device),
                                          _append=plan, **kwargs)

    def _negative_branch(self, input_ids, kwargs):
        """takes the guidance keywords out of a generate() call's `kwargs`: None = guidance is off, else the call's unconditional branch
        (vz_hip.guidance.Negative) - `negative_prompt_ids` embedded as prompts are: text only, or, with `negative_images` (this package's
        extension for the degraded-image contrast), spliced by `prepare_inputs_labels_for_multimodal`; right-padded like the prompts."""
        from vz_hip import guidance as GD
        from vis_zephyr.constants import IMAGE_TOKEN_INDEX
        scale, ids, mask, imgs, sizes = (kwargs.pop(k, None) for k in ("guidance_scale", "negative_prompt_ids", "negative_prompt_attention_mask",
                                                                       "negative_images", "negative_images_size"))
        parsed = GD.parse(scale, ids, mask, imgs, 0 if input_ids is None else input_ids.shape[0], self.generation_config, IMAGE_TOKEN_INDEX)
        if parsed is None:
            return None
        scale, ids, mask = parsed
        ids = ids.to(self.device)
        mask = None if mask is None else mask.to(self.device)
        pos = None
        emb = None
        if imgs is not None:
            (_, pos, mask, _, emb, _) = self.prepare_inputs_labels_for_multimodal(ids, None, mask, None, None, imgs, sizes)
        if emb is None:
            emb = self.get_model().embed_tokens(ids)
        emb, mask, pos, _ = self._to_right_padded(emb, mask, pos)
        return GD.Negative(scale, emb, self._seqlens(mask, emb.shape[0], emb.shape[1]), pos)

    def _spec_history(self, input_ids, attention_mask, images, n_positions: int) -> List[int]:
        """one id per position of the (spliced) prompt for the prompt-lookup drafts (vz_hip.spec): text ids, -1 where a visual token sits."""
        from vz_hip import spec
        from vis_zephyr.constants import IMAGE_TOKEN_INDEX
        ids = input_ids[0].detach().to("cpu", torch.long)
        spliced = images is not None and self.get_vision_tower() is not None and input_ids.shape[1] != 1
        if attention_mask is not None:          # the caller's mask: pads (left or right) hold no position of the sequence
            ids = ids[attention_mask[0].detach().to("cpu").bool()]
        if spliced:
            tiles = [1 if x.ndim == 3 else int(x.shape[0]) for x in images] if isinstance(images, (list, tuple)) else \
                [int(images[i].shape[0]) for i in range(images.shape[0])]
            hist = spec.spliced_history(ids.tolist(), tiles, IMAGE_TOKEN_INDEX, self.arch.qf_queries,
                                        getattr(self.config, "tokenizer_model_max_length", None))
            assert len(hist) == n_positions, f"history of {len(hist)} ids for a spliced prompt of {n_positions} positions"
            return hist
        return ids.tolist()          # text only: the ids as given

    def _generate_from_embeds(self, inputs_embeds, attention_mask, position_ids, max_new_tokens: Optional[int] = None,
                              max_length: Optional[int] = None, do_sample: bool = False, temperature: float = 1.0,
                              top_p: Optional[float] = None, top_k: Optional[int] = -1, eos_token_id=None,
                              pad_token_id=None, streamer=None, stopping_criteria=None, use_cache: bool = True,
                              num_beams: int = 1, generator: Optional[torch.Generator] = None, seed: Optional[int] = None,
                              sync_every: int = 16, timing: Optional[dict] = None, prompt_lookup_num_tokens: Optional[int] = None,
                              max_matching_ngram_size: Optional[int] = None, _spec_history=None,
                              repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                              min_new_tokens: Optional[int] = None, suppress_tokens=None, num_return_sequences: int = 1,
                              return_dict_in_generate: bool = False, output_scores: bool = False, output_logits: bool = False,
                              output_logprobs: bool = False, stop_strings=None, tokenizer=None, device_stop: bool = True,
                              min_p: Optional[float] = None, typical_p: Optional[float] = None, epsilon_cutoff: Optional[float] = None,
                              eta_cutoff: Optional[float] = None, sequence_bias=None, bad_words_ids=None, beam_extended: bool = False,
                              _guidance=None, _append=None, _prompt_rows=None, share_prompt_kv: bool = False, **unused):
        """`return_dict_in_generate=True` returns HF's `GenerateDecoderOnlyOutput` (a subclass with two more fields; `sequences` = the
        generated ids as the plain call returns them - generation starts from embeddings, so there are no prompt ids in front).  With
        `output_scores` / `output_logits` (HF's: tuples of [rows, V] fp32 per step, the processed and warped scores / the raw logits) or
        `output_logprobs` (ours: only `token_logprobs` = log-prob of each token under the model's distribution after the processors at
        temperature 1, and `token_logprobs_warped` = under the distribution it was drawn from, both [rows, T], no [T, rows, V] tensors)
        every step also runs the step recorder behind its tail, inside the per-token graph (csrc/sampling.hip: token_scores_kernel;
        vz_hip/scores.py); without `return_dict_in_generate` they are ignored, as in HF.  Positions behind a row's eos are 0.0 in both
        log-prob tensors; their `scores` / `logits` rows are whatever the parked row produced.  With any of the three,
        `prompt_lookup_num_tokens` takes the plain path (greedy: the ids are the same by construction; sampled: the same draws on
        the 1-row routes' logits).  With a streamer or stopping
        criteria the records wait in a device ring of `max_new_tokens` slots that is allocated up front: 16 bytes per slot, and with
        `output_scores` / `output_logits` another V fp32 per slot and output (260 MB each at V = 32000, max_new_tokens = 2048), even if
        a criterion stops the call after a few tokens - HF's [T, rows, V] outputs cost that; `output_logprobs` does not.

        Beam search (`num_beams` 2..16; `_generate_beam`): `return_dict_in_generate` gives HF's `GenerateBeamDecoderOnlyOutput` with
        `sequences`, `sequences_scores` and `beam_indices`.  The rest of HF's surface there is opt-in, `beam_extended=True`: calls written
        against the earlier versions rely on `NotImplementedError` for the logits-processor and `output_*` keywords with beams, and
        without the flag they still get it.  With it: `output_scores` / `output_logits` give `scores` / `logits`, tuples of
        [Bsz * num_beams, V] fp32 per step (rows prompt-major, beam-minor) - the log-softmax rows after the logits processors / the
        raw logits, as `_beam_search` fills them; `compute_transition_scores(sequences, scores, beam_indices)` gathers through them.
        The logits-processor keywords then work with beams: they act on every beam's log-softmax row over that beam's own ids, as in HF.
        Two deviations, both documented in INTEGRATION.md: at step 0 HF runs `num_beams` identical rows per prompt, this engine
        prefills one and replicates its row; and when `Bsz * num_beams` exceeds the cache rows the prompts run in chunks that may
        take different numbers of steps - `len(scores)` is the largest step count any prompt's search took, and the rows of a
        prompt behind the step at which its own search ended are zeros.  `output_logprobs`, sampling, `stopping_criteria` and
        `stop_strings` with beams raise NotImplementedError.

        Stops (vz_hip/stop.py; csrc/stop.hip: stop_match_kernel): HF's `stop_strings=` (+ `tokenizer=`; default
        `generation_config.stop_strings`), and `stopping_criteria` made only of HF's `StopStringCriteria` and this package's
        `KeywordsStoppingCriteria`, are decided on the device, behind every step's tail inside the per-token graph: the call keeps its
        batched route (`Bsz > 1` greedy rows decode together, `num_return_sequences > 1` works), the host reads where each row stopped at
        the syncs it already has, and a stopped row keeps its stopping token and shows `pad_token_id` behind it, as behind eos.  With a
        streamer, `num_beams > 1`, a tensor-parallel engine, any other criterion in the list, a stop set beyond the matcher's limits or
        `device_stop=False` every criterion stays on the host (one sequence at a time, one callback per token), and stop strings given
        by keyword join them as a `StopStringCriteria`.

        Warpers: HF's `min_p`, `typical_p`, `epsilon_cutoff` and `eta_cutoff` (default: the generation config's)
        act behind temperature / top-k / top-p in HF's order, inside the device-side sampler (csrc/sampling.hip), on every sampled
        route; a greedy call ignores them, as HF does.  HF's `sequence_bias` and `bad_words_ids` (default: the generation config's) join
        the logits processors (csrc/logits_proc.hip), over the generated ids only, in HF's positions: the bias in front of the
        repetition penalty, the bad words behind the n-gram ban; up to 64 sequences of up to 8 ids, NotImplementedError beyond.

        Classifier-free guidance (vz_hip/guidance.py; csrc/guidance.hip): HF's `guidance_scale` (default: the
        generation config's; None or 1 = off) with `negative_prompt_ids` [Bsz, L] (+ `negative_prompt_attention_mask`; required - generation
        starts from embeddings, so HF's fallback to the last prompt id does not exist) and, ours, `negative_images` / `negative_images_size`,
        which splice the negative prompt as `images` splice the prompt.  Every sequence takes two cache rows, the prompt's and the negative
        prompt's, that share each step's weight sweep; behind the logits the conditional row becomes `s * (lc - lu) + lu` of the two
        log-softmax rows, in front of the processors, and the token chosen on it is fed to both rows.  Greedy and sampled, batched,
        `num_return_sequences`, streamer, processors, scores and device stops all take it; `output_logits` rows are the conditional raw
        logits, `output_scores` rows and the log-probs are taken behind the combine.  `num_beams > 1` and tensor-parallel engines raise
        NotImplementedError, `max_batch < 2` ValueError; `prompt_lookup_num_tokens` takes the guided path.

        Prompt lookup (vz_hip/spec.py): `prompt_lookup_num_tokens=k` (+ `max_matching_ngram_size`) runs one
        sequence - greedy or sampled - in verify steps of up to 8 rows.  A sampled call draws row i of a step at the draw counter of the
        token that row would emit, so its ids are a function of (seed, logits) and not of the guesses; against the same call without
        the keyword the logits differ to bf16 rounding (R-row routes instead of 1-row routes), so ids under one seed can differ at a
        near-tie of the race, while the distribution is the same.  With processors, a streamer, stopping criteria or device stops,
        scores, guidance, `past_key_values`, beams, several sequences or `num_return_sequences > 1` the keyword is without effect.

        The cache handle (vz_hip/append.py): with `return_dict_in_generate=True` the output's `past_key_values` is a
        live handle whenever the rows of the call are the engine's cache rows - one sequence, or a greedy batch that decodes together;
        None for beams, guidance, `num_return_sequences > 1`, prompt lookup and batches run in parts.  It records per row the cached
        positions (the spliced prompt plus every emitted token but the last, as HF leaves its cache), the next rotary position and the
        ids those positions stand for.  `generate(<the whole conversation so far>, past_key_values=handle)` (`_generate_continue`) puts
        only the new ids behind the cache.  The logits processors' histories and the stop matcher's rings of such a call start from the
        conversation so far (`Engine.seed_history`): `repetition_penalty`, the n-gram ban, `sequence_bias` and `bad_words_ids` see the cached
        ids as HF's see a prompt's, a stop string may begin in them, host-side criteria get them in front of the new ids; `min_new_tokens`
        and the id-sequence stops count generated ids only.  `num_beams > 1`, guidance, `num_return_sequences > 1`, more rows than
        `max_batch`, tensor-parallel engines and a sampled or per-token batch of several rows raise NotImplementedError - all before the
        handle goes stale; `prompt_lookup_num_tokens` takes the plain path.

        Shared prompt KV (vz_hip/share.py; csrc/attn_shared.hip): `share_prompt_kv=True` with `do_sample=True` and
        `num_return_sequences = n >= 2` keeps each prompt's KV in the one cache row it was prefilled into - no copy into the other n - 1
        rows - and every step's attention reads those slots once per (prompt, KV head) for all n rows as one stacked MFMA pass, each row
        adding only its own generated slots.  The logits differ from the copy route's to bf16 rounding (another summation order), so ids
        under one seed can differ at a near-tie; processors, per-row sampling, scores / log-probs and device stops work as on the copy
        route.  Opt-in: absent or False, the call is the copy route, untouched.  With `num_beams > 1`, `guidance_scale`,
        `past_key_values`, `prompt_lookup_num_tokens`, a tensor-parallel engine or `num_return_sequences == 1` the keyword raises
        NotImplementedError before anything runs.

        A model built with `kv_fp8=True` (vz_hip/kv8.py; csrc/attn_decode_kv8.hip) decodes from the e4m3 mirror of
        its KV cache: `num_beams > 1` and `share_prompt_kv=True` raise NotImplementedError before anything runs,
        `prompt_lookup_num_tokens` takes the plain path, every other keyword works as without it."""
        from vz_hip import logits_proc, sample_rows
        from vz_hip import scores as SC
        from vz_hip import stop as ST
        # what the device takes of the call's stop conditions (all or nothing); every check below sees the host's remainder only
        stop, stopping_criteria = ST.parse(stop_strings, tokenizer, stopping_criteria, self.generation_config,
                                           device_stop and streamer is None and num_beams == 1 and self.engine.tp_size == 1)
        what = SC.check_outputs(return_dict_in_generate, output_scores, output_logits, output_logprobs, num_beams, bool(beam_extended))
        sink = SC.Sink(what) if what else None
        Bsz, S = inputs_embeds.shape[0], inputs_embeds.shape[1]
        app = _append                        # continuing on a kept cache (vz_hip.append.Plan): the embeddings are the new suffix only
        d = DL.resolve_defaults(self.generation_config, eos_token_id, max_new_tokens, max_length,
                                S if app is None else max(p + n for p, n in zip(app.past, app.new_lens)), pad_token_id)
        eos = d.eos
        # HF's logits processors (csrc/logits_proc.hip): None = none of the four keywords is active, every path below is as it was
        gcf = self.generation_config
        proc = logits_proc.parse(repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens, sorted(eos),
                                 getattr(gcf, "sequence_bias", None) if sequence_bias is None else sequence_bias,
                                 getattr(gcf, "bad_words_ids", None) if bad_words_ids is None else bad_words_ids, self.config.vocab_size)
        if proc is not None and num_beams != 1 and not beam_extended:
            raise NotImplementedError("logits processors with num_beams > 1 need `beam_extended=True` (HF applies them to every beam's "
                                      "log-softmax scores there, and so does the beam step then)")
        if proc is not None and self.engine.tp_size > 1:
            raise NotImplementedError("logits processors on a tensor-parallel engine are not built")
        neg = _guidance
        if neg is not None:
            from vz_hip import guidance as GD
            if num_beams != 1:
                raise NotImplementedError("guidance_scale with num_beams > 1 is not built: the beam tail owns every row of its batch")
            if self.engine.tp_size > 1:
                raise NotImplementedError("guidance_scale on a tensor-parallel engine is not built")
            GD.prompts_per_chunk(self.engine.max_batch)          # ValueError: fewer than two cache rows
            if max(neg.seqlens) + d.max_new > self.engine.max_ctx:
                raise ValueError(f"negative prompt ({max(neg.seqlens)}) + max_new_tokens ({d.max_new}) exceeds the engine's max_ctx ({self.engine.max_ctx})")
        if num_beams != 1:
            return self._generate_beam(inputs_embeds, attention_mask, position_ids, num_beams, max_new_tokens, max_length, do_sample,
                                       eos_token_id, pad_token_id, streamer, stopping_criteria, sync_every, timing=timing,
                                       num_return_sequences=num_return_sequences, return_dict_in_generate=return_dict_in_generate,
                                       proc=proc, what=what, **unused)
        max_new_tokens, pad_token_id = d.max_new, d.fill
        greedy = (not do_sample) or temperature is None or temperature <= 0
        nrs = sample_rows.check_return_sequences(num_return_sequences, greedy, self.engine.max_batch, streamer, stopping_criteria)
        if neg is not None:
            GD.prompts_per_chunk(self.engine.max_batch, nrs)     # ValueError: 2 * nrs cache rows do not exist
        if top_k == -1:                      # not passed: HF's generation-config default (50); None / 0 = no top-k filter
            top_k = self.generation_config.top_k
        if top_p is None:
            top_p = self.generation_config.top_p
        # HF's further warpers as RowParams fields: {} = none is active (a greedy call, None, HF's off values), every path below is as it was
        gc = self.generation_config
        warp = {} if greedy else sample_rows.parse_warpers(
            getattr(gc, "min_p", None) if min_p is None else min_p, getattr(gc, "typical_p", None) if typical_p is None else typical_p,
            getattr(gc, "epsilon_cutoff", None) if epsilon_cutoff is None else epsilon_cutoff,
            getattr(gc, "eta_cutoff", None) if eta_cutoff is None else eta_cutoff)
        if seed is None:                     # one 64-bit seed per generate call: from the caller's generator, else from torch's global one
            seed = 0 if greedy else int(torch.randint(0, 2 ** 62, (1,), generator=generator,
                                                      device=generator.device if generator is not None else "cpu").item())
        inputs_embeds, attention_mask, position_ids, _ = self._to_right_padded(inputs_embeds, attention_mask, position_ids)
        seqlens = self._seqlens(attention_mask, Bsz, S)
        def done(seqs, cached: bool = False):      # the plain tensor unless asked; cached: the call's rows are the engine's cache rows
            out = self._generate_output(seqs, sink, eos, return_dict_in_generate)
            if return_dict_in_generate and cached and _prompt_rows is not None:
                out.past_key_values = self._handle_after(seqs, eos, pad_token_id if stop is not None and Bsz > 1 else None, _prompt_rows())
            return out
        if app is not None:                  # every refusal of a continued call lies in front of this line: a refused call leaves the handle live
            if Bsz > 1 and not (greedy and streamer is None and stopping_criteria is None):
                raise NotImplementedError("generate(past_key_values=...): a sampled batch, or one with a streamer or stopping criteria, runs one "
                                          "sequence at a time through cache row 0 and cannot continue several kept rows")
            if max(app.past) + S + max_new_tokens > self.engine.max_ctx:
                raise ValueError(f"prompt ({max(app.past) + S}) + max_new_tokens ({max_new_tokens}) exceeds the engine's max_ctx ({self.engine.max_ctx})")
            self._kv_epoch += 1
        if nrs > 1:                          # n samples of every prompt decode together, each row on its own seed (the per-row tail)
            return done(self._generate_samples(inputs_embeds, seqlens, position_ids, nrs, max_new_tokens, temperature, top_k, top_p, seed, eos,
                                               pad_token_id, sync_every, timing, proc, sink=sink, stop=stop, warp=warp, neg=neg, share=bool(share_prompt_kv)))
        if prompt_lookup_num_tokens and _spec_history is not None and proc is None and sink is None and stop is None and neg is None and app is None:      # (with processors, scores, device stops or guidance: the plain / guided greedy path)
            # HF's prompt lookup decoding: the ids the call yields anyway - the argmax, or in a sampled call the draw of each position under
            # the call's seed - several per weight sweep when the continuation repeats the context (vz_hip/spec.py)
            from vz_hip import spec
            ngram = 2 if max_matching_ngram_size is None else int(max_matching_ngram_size)
            D = spec.draft_slots(prompt_lookup_num_tokens, ngram, n_seq=Bsz, greedy=greedy, num_beams=num_beams, streamer=streamer,
                                 stopping_criteria=stopping_criteria, tp_size=self.engine.tp_size, max_batch=self.engine.max_batch,
                                 prompt_len=seqlens[0], max_new=max_new_tokens, max_ctx=self.engine.max_ctx, n_eos=len(eos),
                                 heads_per_kv=self.arch.n_heads // max(1, self.arch.n_kv_heads), sampled=not greedy)
            if D:
                _spec_history = _spec_history()
                assert len(_spec_history) == seqlens[0], f"history of {len(_spec_history)} ids for a prompt of {seqlens[0]} positions"
                par = None if greedy else sample_rows.RowParams(True, float(temperature), int(top_k or 0), float(1.0 if top_p is None else top_p),
                                                                int(seed), 0, **warp)
                out = self._generate_spec(inputs_embeds[0:1, :seqlens[0]], None if position_ids is None else position_ids[0:1, :seqlens[0]],
                                          _spec_history, D, ngram, max_new_tokens, eos, sync_every, timing, par)
                return done(torch.tensor([out], dtype=torch.long, device=self.device))
        if Bsz > 1 and greedy and streamer is None and stopping_criteria is None:
            return done(self._generate_batched(inputs_embeds, seqlens, position_ids, max_new_tokens, eos, pad_token_id, sync_every, timing, proc, sink, stop, neg, app),
                        cached=neg is None and Bsz <= min(self.engine.max_batch, 64))
        outs = []
        for b in range(Bsz):               # per-token host callbacks / sampling: one sequence at a time
            outs.append(self._generate_one(inputs_embeds[b:b + 1, :seqlens[b]],
                                           None if position_ids is None else position_ids[b:b + 1, :seqlens[b]],
                                           max_new_tokens, greedy, temperature, top_p, top_k, eos, streamer if Bsz == 1 else None,
                                           stopping_criteria, seed + b, sync_every, timing, proc, sink, stop, warp,
                                           None if neg is None else neg.rows(b, b + 1), app))
        return done(DL.pad_parts([torch.tensor([o], dtype=torch.long, device=self.device) for o in outs], pad_token_id, self.device),
                    cached=neg is None and Bsz == 1)

    def _handle_after(self, seqs, eos, fill, prompt_rows):
        """the cache handle of a finished generate() call whose rows are the engine's cache rows (vz_hip.append.after_generate)"""
        from vz_hip import append as AP
        rows = seqs.tolist()
        emitted = [r[:n] for r, n in zip(rows, AP.emitted_counts(rows, eos, fill))]
        next_pos, ctx_len = self._begin_state
        lengths, pos, ids = AP.after_generate(prompt_rows, ctx_len, next_pos, emitted)
        return PastKeyValues(lengths, self, self._kv_epoch, True, ids, pos)

    def _generate_output(self, seqs, sink, eos, return_dict_in_generate):
        """what generate() returns for the new tokens `seqs` [rows, T]: the tensor, or HF's output object with what `sink` recorded"""
        if not return_dict_in_generate:
            return seqs
        from vz_hip import scores as SC
        Scored, _ = SC.output_classes()
        if sink is None:
            return Scored(sequences=seqs)
        f = sink.finish(seqs, eos)
        return Scored(sequences=seqs, scores=f["scores"], logits=f["logits"], token_logprobs=f["token_logprobs"],
                      token_logprobs_warped=f["token_logprobs_warped"])

    def compute_transition_scores(self, sequences, scores, beam_indices=None, normalize_logits: bool = False):
        """HF's `GenerationMixin.compute_transition_scores` for the outputs of `generate(return_dict_in_generate=True, output_scores=True)`;
        with beam search pass the output's `beam_indices`."""
        from vz_hip import scores as SC
        if beam_indices is None:
            return SC.transition_scores(sequences, scores, None, normalize_logits)
        return SC.beam_transition_scores(sequences, scores, beam_indices, normalize_logits, self.config.vocab_size)

    def _generate_spec(self, embeds, position_ids, history, D, max_ngram, max_new, eos, sync_every, timing=None, par=None) -> List[int]:
        """One sequence with prompt-lookup drafts: the first token from the prefill as always, then verify steps of D + 1 rows
        (csrc/spec.hip), `sync_every` per host sync.  par = None: greedy; a sampled vz_hip.sample_rows.RowParams: the first token is one
        draw of the device sampler with counter 0, as `_generate_one` draws it, and the verify steps draw their rows by the same record."""
        from vz_hip import binding as B
        from vz_hip import spec
        eng = self.engine
        S = embeds.shape[1]
        _, last = eng.prefill(embeds, [S], position_ids, all_logits=False, last_logits=True)
        next_pos = S if position_ids is None else int(position_ids[0, -1]) + 1
        if par is None:
            tok = int(B.argmax(last)[0])          # int(): the host holds the first token here
        else:
            tok = int(B.sample(last, par.temperature, par.top_k, par.top_p, par.seed, 0, par.warp)[0])
        if timing is not None:
            timing["t_first_token"] = time.perf_counter()
        report = {}
        out = spec.decode(eng, tok, next_pos, S, history, D, max_new, eos, max_ngram, max(1, int(sync_every)), report=report, sample=par)
        if timing is not None:
            timing["spec"] = report
        return out

    def _generate_batched(self, embeds, seqlens, position_ids, max_new, eos, pad_token_id, sync_every, timing=None, proc=None, sink=None,
                          stop=None, neg=None, app=None) -> torch.Tensor:
        """Greedy decoding of up to `max_batch` (<= 64) sequences at once: one right-padded prefill, then every decode step
        streams the weights once for all rows (the KV cache, positions and lengths are per slot).  Rows that hit eos keep
        their slot but emit `pad_token_id` from then on, as HF does.  `proc`: HF's logits processors (vz_hip.logits_proc) on the
        prefill logits and, armed in the engine, on every step's.  `stop`: the stop conditions the engine's matcher decides per row
        (vz_hip.stop.Plan): a row that stops is treated as a row that emitted eos.  `neg`: the prompts' unconditional branch
        (vz_hip.guidance.Negative): every prompt takes a second cache row for its negative prompt, so half as many decode together."""
        eng = self.engine
        Bsz, S = embeds.shape[0], embeds.shape[1]
        cap = min(eng.max_batch, 64) if neg is None else min(eng.max_batch, 64) // 2
        if Bsz > cap:
            part = lambda lo, hi, tm: self._generate_batched(embeds[lo:hi], seqlens[lo:hi], None if position_ids is None else position_ids[lo:hi],      # noqa: E731
                                                             max_new, eos, pad_token_id, sync_every, tm, proc, sink, stop,
                                                             None if neg is None else neg.rows(lo, hi))
            return DL.run_parts(part, Bsz, cap, pad_token_id, self.device, timing)
        if S + max_new + (0 if app is None else max(app.past)) > eng.max_ctx:
            raise ValueError(f"prompt ({S + (0 if app is None else max(app.past))}) + max_new_tokens ({max_new}) exceeds the engine's max_ctx ({eng.max_ctx})")
        from vz_hip.sample_rows import GREEDY
        if neg is None:
            last, next_pos, ctx_len = DL.prefill_or_append(eng, embeds, seqlens, position_ids, app)
            self._begin_state = (list(next_pos), list(ctx_len))      # what the rows hold in front of the first emitted token: for the call's cache handle
            uncond = None
        else:
            last, last_u, next_pos, ctx_len = DL.pair_prefill(eng, embeds, seqlens, position_ids, neg)
            uncond = (last_u, neg.scale)
        hist = None if app is None else app.history
        first, first_cpu, blk = DL.first_tokens(last, [GREEDY] * Bsz, proc, sink, timing, uncond=uncond, history=hist)
        with DL.armed(eng, proc=proc, scores=DL.chunk_recorder(sink, Bsz, sync_every, max_new), stop=stop, history=hist,
                      guidance=None if neg is None else neg.config(Bsz)) as begin:
            begin(first, next_pos, ctx_len)
            return DL.decode_rows(eng, first_cpu, max_new, eos, pad_token_id, sync_every, blk, stop is not None).to(self.device)

    # ---- n samples per prompt (hf:generation/utils.py `_sample` with num_return_sequences; csrc/sampling.hip: sample_rows_kernel) ----
    def _generate_samples(self, embeds, seqlens, position_ids, n, max_new, temperature, top_k, top_p, seed, eos, pad_token_id, sync_every,
                          timing=None, proc=None, prompt0: int = 0, sink=None, stop=None, warp=None, neg=None, share: bool = False) -> torch.Tensor:
        """`n` sampled sequences of every prompt: [Bsz * n, T] in HF's order (prompt-major, a prompt's samples adjacent).  Each prompt is
        prefilled once into its first cache row, its prompt KV copied into its other n - 1 rows, its n first tokens drawn from the one
        row of prefill logits, and then all rows step together with the per-row tail: row j of prompt b draws under seed
        `seed + b * n + j` (vz_hip.sample_rows.row_seed) with its own counter, so it gets the tokens that seed gives it alone.  `neg`
        (vz_hip.guidance.Negative): each negative prompt is prefilled once as well and spread over the n unconditional rows of its prompt.
        `share` (generate's `share_prompt_kv`; vz_hip/share.py): no copy - the prompt's KV stays in its first row and the armed step's
        attention reads it from there for all n rows."""
        from vz_hip import sample_rows as SR
        eng = self.engine
        if eng.tp_size > 1:
            raise NotImplementedError("num_return_sequences > 1 on a tensor-parallel engine (tp_size > 1) is not built")
        Bsz = embeds.shape[0]
        if neg is None:
            G = SR.prompts_per_chunk(n, eng.max_batch)
        else:
            from vz_hip.guidance import prompts_per_chunk
            G = prompts_per_chunk(eng.max_batch, n)
        if Bsz > G:
            part = lambda lo, hi, tm: self._generate_samples(embeds[lo:hi], seqlens[lo:hi], None if position_ids is None else position_ids[lo:hi], n,      # noqa: E731
                                                             max_new, temperature, top_k, top_p, seed, eos, pad_token_id, sync_every, tm, proc,
                                                             prompt0 + lo, sink, stop, warp, None if neg is None else neg.rows(lo, hi), share)
            return DL.run_parts(part, Bsz, G, pad_token_id, self.device, timing)
        if max(seqlens) + max_new > eng.max_ctx:
            raise ValueError(f"prompt ({max(seqlens)}) + max_new_tokens ({max_new}) exceeds the engine's max_ctx ({eng.max_ctx})")
        plan = None
        if share:
            from vz_hip import share as SH
            plan = SH.plan(seqlens, n, max_new, eng.max_ctx, getattr(self.config, "sliding_window", 0) or 0, eng.max_batch)
        R = Bsz * n
        uncond = None
        if neg is None:
            last = DL.fan_prefill(eng, embeds, seqlens, position_ids, n)
        else:
            last, last_u, next_pos, ctx_len = DL.pair_prefill(eng, embeds, seqlens, position_ids, neg, n)
            uncond = (last_u, neg.scale)
        params = [SR.RowParams(True, float(temperature), int(top_k or 0), float(1.0 if top_p is None else top_p),
                               SR.row_seed(seed, prompt0 + r // n, n, r % n), 0, **(warp or {})) for r in range(R)]
        first, first_cpu, blk = DL.first_tokens(last, params, proc, sink, timing, uncond=uncond)
        if neg is None:
            next_pos, ctx_len = (DL.fan_share if share else DL.fan_spread)(eng, seqlens, position_ids, n)
        with DL.armed(eng, proc=proc, sampling_rows=[p.at(1) for p in params], scores=DL.chunk_recorder(sink, R, sync_every, max_new),
                      stop=stop, guidance=None if neg is None else neg.config(R), share=plan) as begin:
            begin(first, next_pos, ctx_len)
            return DL.decode_rows(eng, first_cpu, max_new, eos, pad_token_id, sync_every, blk, stop is not None).to(self.device)

    # ---- beam search (hf:generation/utils.py `_beam_search`, do_sample=False; csrc/beam.hip + vz_hip/beam.py) ----------------
    def _generate_beam(self, inputs_embeds, attention_mask, position_ids, num_beams, max_new_tokens, max_length, do_sample,
                       eos_token_id, pad_token_id, streamer, stopping_criteria, sync_every, length_penalty: float = 1.0,
                       early_stopping=False, num_return_sequences: int = 1, return_dict_in_generate: bool = False,
                       timing: Optional[dict] = None, proc=None, what: int = 0, **unused):
        """Beam search over the prompts of a batch: `Bsz * num_return_sequences` rows of new tokens, HF's `sequences` of a
        decoder-only model generating from inputs_embeds (shorter hypotheses filled as HF fills them, vz_hip.beam.fill_value).
        Each prompt is prefilled once; its first step is chosen on the prefill logits (vz_op_beam_select), its prompt KV copied
        into its num_beams cache rows, and then the decode steps run with the beam tail (selection + KV reorder on the device),
        `sync_every` steps per host sync, whose history records the host replays (vz_hip.beam.BeamReplay) to keep HF's finished
        hypotheses and to stop where HF stops.
        proc (vz_hip.logits_proc config): HF's logits processors on every beam's log-prob row over that beam's own ids, on the
        device.  what (vz_hip.scores flags): the steps' processed rows / raw logits rows are recorded on the
        device and returned as HF's `scores` / `logits`; step 0 replicates each prompt's one prefill row over its beams, and a
        prompt's rows behind the step at which its own search ended are zeros (chunked batches run different numbers of steps)."""
        from vz_hip import beam as BM
        from vz_hip import scores as SC
        eng = self.engine
        nb = int(num_beams)
        if do_sample:
            raise NotImplementedError("beam sampling (num_beams > 1 with do_sample=True) is not built: beam search here is deterministic")
        if streamer is not None:
            raise ValueError("`streamer` cannot be used with beam search (yet!). Make sure that `num_beams` is set to 1.")
        if stopping_criteria is not None:
            raise NotImplementedError("stopping_criteria with num_beams > 1: the beam tail stops on eos ids and the length limit only")
        if eng.tp_size > 1:
            raise NotImplementedError("beam search on a tensor-parallel engine (tp_size > 1) is not built")
        if not 2 <= nb <= 16:
            raise NotImplementedError(f"num_beams = {nb}: the device beam tail takes 2..16 beams")
        if nb > min(eng.max_batch, 64):
            raise ValueError(f"num_beams = {nb} exceeds the engine's max_batch ({eng.max_batch}): every beam needs a KV-cache row")
        nrs = int(num_return_sequences)
        if not 1 <= nrs <= nb:
            raise ValueError("`num_return_sequences` has to be smaller or equal to `num_beams`.")
        if early_stopping not in (False, True, "never"):
            raise ValueError(f"`early_stopping` must be a boolean or 'never', but is {early_stopping}.")
        Bsz, S = inputs_embeds.shape[0], inputs_embeds.shape[1]
        d = DL.resolve_defaults(self.generation_config, eos_token_id, max_new_tokens, max_length, S, pad_token_id)
        max_new, eos = d.max_new, d.eos_list          # the ids in the caller's order, as the device and `fill_value` take them
        if len(eos) > 4:
            raise NotImplementedError(f"{len(eos)} eos ids: the beam tail takes up to 4")
        fill = BM.fill_value(d.pad, eos)
        inputs_embeds, attention_mask, position_ids, _ = self._to_right_padded(inputs_embeds, attention_mask, position_ids)
        seqlens = self._seqlens(attention_mask, Bsz, S)
        if max(seqlens) + max_new > eng.max_ctx:
            raise ValueError(f"prompt ({max(seqlens)}) + max_new_tokens ({max_new}) exceeds the engine's max_ctx ({eng.max_ctx})")
        G = max(1, min(Bsz, min(eng.max_batch, 64) // nb))          # prompts per chunk: G * nb cache rows
        replays, rows = [], []
        for b0 in range(0, Bsz, G):
            r, rw = self._beam_chunk(inputs_embeds[b0:b0 + G], seqlens[b0:b0 + G],
                                     None if position_ids is None else position_ids[b0:b0 + G], nb, max_new, eos,
                                     float(length_penalty), early_stopping, max(1, int(sync_every)), timing, proc, what)
            replays += r
            rows.append(rw)
        hyps = [r.best(nrs) for r in replays]
        seqs = DL.pad_parts([torch.tensor([t], dtype=torch.long) for h in hyps for t, _ in h], fill, "cpu").to(self.device)
        if return_dict_in_generate:
            scores = torch.tensor([sc for h in hyps for _, sc in h], dtype=torch.float32, device=self.device)
            idx = BM.flat_beam_indices([r.best_indices(nrs) for r in replays], nb).to(self.device)
            T = max(r.cur_len for r in replays)          # the steps of the longest search: what a chunk's device ran past it is dropped

            def per_step(key):          # the chunks' rows [steps_i, G_i * nb, V] side by side, cut or zero-padded to T steps: T x [Bsz * nb, V]
                if rows[0][key] is None:
                    return None
                parts = [rw[key][:T] for rw in rows]
                parts = [x if x.shape[0] == T else torch.cat([x, x.new_zeros((T - x.shape[0],) + tuple(x.shape[1:]))], 0) for x in parts]
                full = parts[0] if len(parts) == 1 else torch.cat(parts, 1)
                return tuple(full[t] for t in range(T))
            return SC.output_classes()[1](sequences=seqs, sequences_scores=scores, scores=per_step("scores"), logits=per_step("logits"),
                                          beam_indices=idx)      # HF's GenerateBeamDecoderOnlyOutput
        return seqs

    def _beam_chunk(self, embeds, seqlens, position_ids, nb, max_new, eos, length_penalty, early_stopping, sync_every, timing=None,
                    proc=None, what: int = 0):
        """one chunk of G prompts x nb cache rows: (the prompts' finished replays, {"scores", "logits"}: the chunk's recorded rows fp32
        [steps, G * nb, V] with zeros behind each prompt's own last step, or None when not asked for)"""
        from vz_hip import beam as BM
        from vz_hip import binding as B
        from vz_hip import scores as SC
        eng = self.engine
        G = embeds.shape[0]
        want_sc, want_raw = bool(what & SC.SCORE_WARPED), bool(what & SC.SCORE_RAW)
        last = DL.fan_prefill(eng, embeds, seqlens, position_ids, nb)          # one prefill per prompt into its first beam row
        fan = lambda x: x.repeat_interleave(nb, dim=0).unsqueeze(0)            # noqa: E731  (step 0: a prompt's one row, once per beam)
        sc_rows, raw_rows = [], [fan(last)] if want_raw else []
        if proc is not None or want_sc:
            # HF: log_softmax, then the processors (no ids yet), then the choice among the first beam's continuations
            lp = B.beam_logprob_rows(last)
            if proc is not None:
                B.logits_process(lp, proc)
            if want_sc:
                sc_rows.append(fan(lp))
            rec, tok, sc, _ = B.beam_select(lp, None, 1, nb, eos, on_rows=True)
        else:
            rec, tok, sc, _ = B.beam_select(last, None, 1, nb, eos)
        replays = [BM.BeamReplay(nb, eos, max_new, length_penalty, early_stopping) for _ in range(G)]
        s0, t0, p0 = BM.decode_records(rec)
        if timing is not None:
            timing["t_first_token"] = time.perf_counter()        # the host holds every prompt's first step here
        for g in range(G):
            replays[g].step(s0[g], t0[g], p0[g])
        if not all(r.done for r in replays):
            next_pos, ctx_len = DL.fan_spread(eng, seqlens, position_ids, nb)          # the prompt KV of each prompt into its beam rows
            hist = torch.empty(max(1, max_new - 1), G, BM.beam_k(nb, len(eos)), 3, dtype=torch.int32, device=self.device)
            rings = (max(1, min(sync_every, max_new - 1)), G * nb, want_sc, want_raw) if (want_sc or want_raw) else None
            with DL.armed(eng, proc=proc, beam_rows=rings, beam=(True, nb, G, eos, [int(v) for v in seqlens], sc, hist)) as begin:
                begin(tok, next_pos, ctx_len)
                done_steps, remaining = 0, max_new - 1
                while remaining > 0 and not all(r.done for r in replays):
                    n = min(sync_every, remaining)
                    eng.decode_steps(n)
                    s, t, p = BM.decode_records(hist[done_steps:done_steps + n])      # the only host sync of the chunk
                    done_steps += n
                    remaining -= n
                    if rings is not None:
                        a, b = eng.beam_rows_steps(done_steps, n)
                        if want_sc:
                            sc_rows.append(a)
                        if want_raw:
                            raw_rows.append(b)
                    for i in range(n):
                        for g in range(G):
                            if not replays[g].done:
                                replays[g].step(s[i, g], t[i, g], p[i, g])
        out = {"scores": None, "logits": None}
        for key, parts in (("scores", sc_rows), ("logits", raw_rows)):
            if parts:
                x = torch.cat(parts, 0)                                        # [steps the device ran + 1, G * nb, V]
                for g in range(G):
                    x[replays[g].cur_len:, g * nb:(g + 1) * nb] = 0            # behind the prompt's own last step
                out[key] = x
        return replays, out

    # ---- continuous batching: the 23 K-item eval loop without waiting for a batch's longest answer ----
    @torch.no_grad()
    def generate_stream(self, requests, max_new_tokens: int = 128, eos_token_id=None, rows: Optional[int] = None, sync_every: int = 16,
                        admit: Optional[int] = None, stop_strings=None, tokenizer=None, stop_token_sequences=None, per_request: bool = False):
        """Generation over an iterable of requests - dicts with `input_ids` [1, L] (IMAGE_TOKEN_INDEX sentinels allowed),
        optional `images` ([N,3,336,336]) / `images_size`, optional `max_new_tokens`, optional sampling parameters `do_sample`,
        `temperature`, `top_p`, `top_k`, `seed` (read as `generate` reads them; greedy without them) - with CONTINUOUS batching: up to `rows`
        KV-cache rows decode together; a row whose sequence ends (eos or its token budget) is re-armed with the next request at
        the next host sync (every `sync_every` steps), the other rows keep decoding.  Yields `(index, LongTensor[n_new])` in
        completion order.  Rows are independent sequences: every sequence gets the tokens `generate` gives it alone UP TO kernel-route
        re-association - the number of rows decoding together (GEMV / MFMA weight stream / tile GEMM by row count) and, for a shared
        admission prefill, the padded group size (split-K factor of the tile GEMM, fp8 MFMA threshold of a prefill_fp8 engine) choose
        different but equally accurate bf16 evaluation orders, so a near-tie between two candidates can flip.  With the route choice
        pinned (vz_tune_set(26, 0)) the ids are bit-identical (tests/test_stages_gpu.py::test_continuous_batching_matches_static_batches);
        at the default knobs they agree up to the first near-tie (::test_continuous_batching_default_knobs_near_tie).

        Greedy and sampled requests share a batch.  A sampled request (do_sample=True, temperature > 0; top_k defaults to the generation
        config's 50, top_p to 1.0, a missing seed is drawn from torch's global generator) gets, up to the same kernel-route
        re-association, the tokens `generate(input_ids, do_sample=True, seed=s, ...)` gives it alone: its first token is drawn from
        its prefill logits with draw counter 0 and its row then steps with the per-row tail (csrc/sampling.hip: sample_rows_kernel)
        under the request's own seed and counter, whichever cache row it lands in.  The per-row tail is armed when the first sampled
        request is admitted; a call in which no request samples runs as it always did.  `repetition_penalty`, `no_repeat_ngram_size`,
        `min_new_tokens` and `suppress_tokens` in a request raise NotImplementedError (so do `sequence_bias`, `bad_words_ids` and
        `stop_token_sequences`) unless the call opts in with `per_request=True`, below.

        Admissions are BATCHED when the engine has cache rows to spare (`max_batch > rows`): all requests entering at one sync
        share one Zephyr prefill (right-padded, up to `admit` = min(max_batch - rows, 16) sequences) into the spare rows, one
        argmax readback, and their KV is then moved to the freed rows (`vz_llm_kv_move_rows`).  The vision stage stays per request:
        the Q-Former's text conditioning makes a request's visual tokens depend on the padded length of its batch.

        A request may carry `logprobs=True`: that request, and only that one, is yielded as `(index, ids, logprobs)` with `logprobs` fp32
        [n_new] = the log-prob of each of its tokens under the model's own distribution at temperature 1 (`generate`'s `token_logprobs`).
        The step recorder (csrc/sampling.hip: token_scores_kernel) is armed when the first such request is admitted - the step's graph is
        captured once more, no id changes - and one more device-to-host copy of [n, rows, 4] words rides with each chunk's ids; a call
        in which no request asks runs as it always did.

        `stop_strings` (+ `tokenizer`, HF's keywords) and `stop_token_sequences` (lists of ids) are call-level stop conditions that
        apply to every request: the stop matcher (csrc/stop.hip: stop_match_kernel; vz_hip/stop.py) is armed once, before the first
        admission, and decides them on the device behind every step's tail; where each row stopped rides with the chunk's ids.  A
        stopped request is yielded inclusive of its stopping token and its row parked at that sync.  A stop set beyond the matcher's
        limits raises (NotImplementedError for stop strings, ValueError for more than 16 or malformed `stop_token_sequences`) before
        anything runs: this loop has no per-token host path, and a stop condition is never dropped.

        `per_request=True` (opt-in, as `beam_extended` is for the beam path): a request may carry its own logits processors -
        `repetition_penalty`, `no_repeat_ngram_size`, `min_new_tokens`, `suppress_tokens`, `sequence_bias`, `bad_words_ids`, read by
        vz_hip.logits_proc.parse with the call's eos ids and the model's vocabulary (HF's ValueErrors, the kernel's limits) - and its own
        `stop_token_sequences`, matched behind the call's (together at most 16).  Up to the same kernel-route re-association every
        request gets the tokens `generate(input_ids, <its own keywords>)` gives it alone; one that stops on a sequence is yielded
        inclusive of the stopping token.  Both modes are armed once, before the first admission: every step then
        runs the per-row processor kernel (csrc/logits_proc.hip: logits_process_rows_kernel; a row whose request names no key has an
        inactive record and is left alone) and the stop matcher in its per-row mode, their tables written per row at admission with no
        re-capture.  A request's first token goes through `binding.logits_process_rows` on its prefill logits row with an empty history;
        when its row is parked its record is deactivated.  A stream in which no request names a key yields the ids of the same stream
        with the flag off.  Per-request stop strings, guidance and eos ids are not built; tensor-parallel engines: NotImplementedError."""
        from vz_hip import stop as ST
        from vz_hip import stream
        stop, host_stop = ST.parse(stop_strings, tokenizer, None, self.generation_config, True, stop_token_sequences)
        if host_stop is not None or (stop is not None and self.engine.tp_size > 1):
            raise NotImplementedError("generate_stream: these stop strings are beyond what the device matcher takes (vz_hip.stop.parse)")
        if per_request and self.engine.tp_size > 1:
            raise NotImplementedError("generate_stream: per_request=True on a tensor-parallel engine is not built")
        self._kv_epoch += 1
        self._ensure_ready()
        eos = DL.resolve_defaults(self.generation_config, eos_token_id, max_new_tokens).eos

        def embed(idx, req):
            if req.get("guidance_scale") is not None or req.get("negative_prompt_ids") is not None:
                raise NotImplementedError(f"request {idx}: guidance_scale / negative_prompt_ids per request are not built in generate_stream "
                                          "(a guided sequence takes two cache rows); use generate()")
            ids = req["input_ids"]
            ids = ids if ids.dim() == 2 else ids.unsqueeze(0)
            images = req.get("images")
            if images is None:
                return self.engine.embed_tokens(ids.to(self.device))
            images = images if isinstance(images, (list, tuple)) else [images]
            return self.prepare_inputs_labels_for_multimodal(ids.to(self.device), None, None, None, None, images, req.get("images_size"))[4]

        # the scheduler (vz_hip/stream.py): admit, step, harvest until the requests and the rows run out.  The vocabulary is what a request's
        # own processors are checked against: only a per_request call reads it
        yield from stream.run(self.engine, requests, embed, gen=self.generation_config, vocab=self.config.vocab_size if per_request else None,
                              eos=eos, max_new=max_new_tokens, stop=stop, per_request=per_request, rows=rows, admit=admit, sync_every=sync_every)

    def _token_ring(self, n: int = 8) -> torch.Tensor:
        """pinned host buffer the step tails write their tokens to (device-visible: hipHostMalloc memory is mapped)."""
        if self._ring is None or self._ring.numel() != n:
            self._ring = torch.zeros(n, dtype=torch.int32).pin_memory()
        return self._ring

    def _generate_one(self, embeds, position_ids, max_new, greedy, temperature, top_p, top_k, eos, streamer,
                      stopping_criteria, seed, sync_every, timing=None, proc=None, sink=None, stop=None, warp=None, neg=None, app=None) -> List[int]:
        """One sequence.  The first token comes from the prefill logits (argmax / one draw of the device sampler with counter 0),
        every later one from a replay of the per-token hipGraph whose tail is the argmax or the sampling kernel - also on the path
        `script/run_cli.sh` takes (streamer + stopping criteria + do_sample, ref:vis_zephyr/serve/cli.py:155-182): there the host
        keeps ONE step in flight and reads token t from a host-visible ring when the event behind step t fires, so the callbacks
        of token t run under step t+1 and no logits ever travel.  `proc`: HF's logits processors (vz_hip.logits_proc) run on the
        prefill logits before the first token is chosen and, armed in the engine, in front of every step's tail.  `neg`
        (vz_hip.guidance.Negative of this one sequence): the negative prompt is prefilled into cache row 1 and steps beside the prompt."""
        from vz_hip.sample_rows import GREEDY, RowParams
        eng = self.engine
        S = embeds.shape[1]
        if S + max_new + (0 if app is None else app.past[0]) > eng.max_ctx:
            raise ValueError(f"prompt ({S + (0 if app is None else app.past[0])}) + max_new_tokens ({max_new}) exceeds the engine's max_ctx ({eng.max_ctx})")
        if neg is None:
            last, next_pos, ctx_len = DL.prefill_or_append(eng, embeds, [S], position_ids, app)
            self._begin_state = (list(next_pos), list(ctx_len))
            uncond, guid = None, None
        else:
            last, last_u, next_pos, ctx_len = DL.pair_prefill(eng, embeds, [S], position_ids, neg)
            uncond, guid = (last_u, neg.scale), neg.config(1)
        per_token = streamer is not None or stopping_criteria is not None
        if streamer is not None:
            # HF hands the (empty, since generation starts from embeddings) prompt ids to the streamer first;
            # TextStreamer(skip_prompt=True) swallows exactly one put() as "the prompt"
            streamer.put(torch.empty((1, 0), dtype=torch.long))
        par = GREEDY if greedy else RowParams(True, float(temperature), int(top_k or 0), float(1.0 if top_p is None else top_p), 0, 0, **(warp or {}))
        more = () if par.warp is None else (par.warp,)      # the further warpers' column, named only when one is active
        hist = None if app is None else app.history          # continuing on a kept cache: what the row was fed so far (the filters' histories)
        seen = [] if hist is None else hist[0]                # ... and what host-side stopping criteria see in front of the new tokens
        first, first_cpu, blk = DL.first_tokens(last, [par], proc, sink, timing, None if greedy else (temperature, top_k, top_p, seed) + more, uncond,
                                                history=hist)
        out: List[int] = [int(first_cpu[0])]
        if self._emit(out, streamer, stopping_criteria, None, eos, seen) or max_new <= 1:
            return self._finish(out, streamer)
        # the step's tail: a greedy call names it only with the ring, whose slot is the draw counter that `set_sampling` starts at 1
        tail = None if greedy and not per_token else (not greedy, 1.0 if greedy else temperature, top_k, top_p, seed, 1) + more
        if not per_token:
            # no host callbacks: steps are enqueued back to back, the host looks at the ids every `sync_every` tokens only to honour eos
            # and the stop conditions the device decides (vz_hip.stop)
            with DL.armed(eng, proc=proc, sampling=tail, scores=DL.chunk_recorder(sink, 1, sync_every, max_new), stop=stop, guidance=guid,
                          history=hist) as begin:
                begin(first, next_pos, ctx_len)
                return DL.decode_rows(eng, first_cpu, max_new, eos, 0, sync_every, blk, stop is not None)[0].tolist()
        ring = self._token_ring()
        R = ring.numel()
        # with a sink: a device ring of max_new slots, read once at the end - no step waits for its record
        with DL.armed(eng, proc=proc, sampling=tail, ring=ring, scores=None if blk is None else (max_new, 1, sink.warped, sink.raw),
                      guidance=guid, history=hist) as begin:
            begin(first, next_pos, ctx_len)
            dev_out = torch.empty(1, 1, dtype=torch.int32, device=self.device)
            events = {}

            def launch(t):               # step producing generated token index t (draw counter t)
                eng.decode_steps(1, out=dev_out)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
                events[t] = ev

            launch(1)
            t = 1
            while True:
                if t + 1 < max_new:
                    launch(t + 1)        # speculative: its cache slot / ring slot are simply ignored if token t stops the sequence
                events.pop(t).synchronize()
                out.append(int(ring[t % R]))
                if self._emit(out, streamer, stopping_criteria, None, eos, seen) or len(out) >= max_new:
                    break
                t += 1
            torch.cuda.current_stream(self.device).synchronize()      # a speculative step may still be running
            eng.check_async()
            if blk is not None:
                blk.add(*eng.scores_steps(len(out) - 1, first=0))     # (a speculative step's record behind them is not read)
            return self._finish(out, streamer)

    def _emit(self, out, streamer, stopping_criteria, scores, eos, seen=()) -> bool:
        """per-token host callbacks; returns True when generation must stop.  seen: the ids in front of `out` that the criteria see with it
        (a call that continues on a kept cache: the conversation so far, as HF's criteria see its input_ids)."""
        if streamer is not None:
            streamer.put(torch.tensor([out[-1]], dtype=torch.long))
        stop = out[-1] in eos
        if stopping_criteria is not None and not stop:
            ids = torch.tensor([list(seen) + out], dtype=torch.long, device=self.device)
            crits = stopping_criteria if isinstance(stopping_criteria, (list, tuple)) else [stopping_criteria]
            for c in crits:
                r = c(ids, scores)
                if bool(r.all() if torch.is_tensor(r) else r):
                    stop = True
        return stop

    @staticmethod
    def _finish(out, streamer):
        if streamer is not None:
            streamer.end()
        return out

    def prepare_inputs_for_generation(self, input_ids, past_key_values=None, inputs_embeds=None, **kwargs):
        """ref vis_zephyr.py:144-170: pass-through that re-attaches images / images_size."""
        images = kwargs.pop("images", None)
        images_size = kwargs.pop("images_size", None)
        inputs = dict(input_ids=input_ids, past_key_values=past_key_values, inputs_embeds=inputs_embeds, **kwargs)
        if images is not None:
            inputs["images"] = images
        if images_size is not None:
            inputs["images_size"] = images_size
        return inputs


# Register the model / config with HF's Auto classes (ref:vis_zephyr/model/language_model/vis_zephyr.py:173-174): lets
# `AutoConfig.from_pretrained` read a `"model_type": "vis_zephyr"` config.json and `AutoModelForCausalLM.from_pretrained(...)`
# dispatch to VisZephyrForCausalLM.from_pretrained above.
try:
    from transformers import AutoConfig, AutoModelForCausalLM
    AutoConfig.register("vis_zephyr", VisZephyrConfig, exist_ok=True)
    AutoModelForCausalLM.register(VisZephyrConfig, VisZephyrForCausalLM, exist_ok=True)
except Exception:                       # pragma: no cover - transformers absent or too old for exist_ok
    pass
