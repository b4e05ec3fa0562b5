"""Python owner of one native engine (vz_engine): weight packing from the reference's state-dict
names into the engine's HBM layout, and thin stage calls.  torch is plumbing only (device memory,
dtype casts at load time, streams); every stage runs in libviszephyr_hip.so.

HBM layout: all matrices bf16 row-major [out_features, in_features] exactly
as the reference stores them, except
  * q/k/v (CLIP, Zephyr) stacked into one [3C,C] / [6144,4096] matrix -> one GEMM per layer,
  * cross-attention k|v stacked [8192,5120],
  * Zephyr gate/up interleaved in 16-row groups [16 gate | 16 up | ...] so the SwiGLU product is
    formed inside the GEMM epilogue,
  * the CLIP patch convolution flattened to [1024, 588] and zero-padded to K = 640.
Vectors (biases, LayerNorm/RMSNorm scales) are fp32.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from . import binding as B
from . import tp as TP
from .synth import ArchConfig, iter_state_dict

_CLIP_PREFIXES = ("model.vision_tower.vision_tower.vision_model.", "model.vision_tower.vision_tower.")
_QF = "model.mm_projector."


def rope_tables(cfg: ArchConfig, max_pos: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 cos/sin [max_pos, head_dim/2] (hf:models/mistral/modeling_mistral.py:262-317: inv_freq =
    theta^(-2i/d), angle = pos * inv_freq computed in fp32)."""
    d = cfg.head_dim
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, d, 2, dtype=torch.int64).float() / d))
    fr = torch.arange(max_pos, dtype=torch.float32).unsqueeze(-1) * inv
    return fr.cos().contiguous(), fr.sin().contiguous()


class Engine:
    def __init__(self, cfg: ArchConfig, device="cuda:0", max_batch: int = 1, max_ctx: int = 4096,
                 max_tiles: int = 8, max_text: int = 2048, tp_size: int = 1, tp_rank: int = 0, weight_fp8: bool = False,
                 weight_nf4: bool = False, kv_fp8: bool = False):
        self.lib = B.load_library()            # raises when the HIP library is absent: no fallback
        self._qf_kv_pool = {}
        if not torch.cuda.is_available():
            raise RuntimeError("vz_hip.Engine needs a ROCm GPU (gfx950); there is no CPU fallback")
        self.cfg = cfg
        TP.check_divisible(cfg, tp_size)
        self.tp_size, self.tp_rank = tp_size, tp_rank
        self.vp = (cfg.vocab + tp_size - 1) // tp_size          # lm_head rows per rank (zero padded)
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.max_batch, self.max_ctx, self.max_tiles, self.max_text = max_batch, max_ctx, max_tiles, max_text
        c = B.VzConfig(
            hidden=cfg.hidden, inter=cfg.inter, n_layers=cfg.n_layers, n_heads=cfg.n_heads, n_kv_heads=cfg.n_kv_heads,
            head_dim=cfg.head_dim, vocab=cfg.vocab, rms_eps=cfg.rms_eps, rope_theta=cfg.rope_theta,
            sliding_window=cfg.sliding_window, clip_hidden=cfg.clip_hidden, clip_inter=cfg.clip_inter,
            clip_layers=cfg.clip_layers, clip_heads=cfg.clip_heads, clip_image=cfg.clip_image,
            clip_patch=cfg.clip_patch, clip_eps=cfg.clip_eps, qf_queries=cfg.qf_queries, qf_blocks=cfg.qf_blocks,
            qf_heads=cfg.qf_heads, qf_kv_dim=cfg.qf_kv_dim, qf_eps=cfg.qf_eps, fusion_groups=cfg.fusion_groups,
            fusion_layers_per_group=cfg.fusion_layers_per_group, max_batch=max_batch, max_ctx=max_ctx,
            max_tiles=max_tiles, max_text=max_text, tp_size=tp_size, tp_rank=tp_rank,
            clip_keep_cls=int(cfg.clip_keep_cls), weight_fp8=int(weight_fp8))
        self.c_cfg = c                         # what vz_op_stage_ws_bytes is asked with (stage_ws_bytes)
        self.weight_fp8 = bool(weight_fp8)
        if weight_fp8 and weight_nf4:
            raise ValueError("weight_fp8 and weight_nf4 are two quantisations of the same linears: pick one")
        self.weight_nf4 = bool(weight_nf4)
        self._nf4_done = set()
        self.prefill_fp8 = False
        h = C.c_void_p()
        B.check(self.lib.vz_engine_create(C.byref(c), C.byref(h)))
        self.h = h
        self.w: Dict[str, torch.Tensor] = {}
        self._registered = set()
        cos, sin = rope_tables(cfg, max_ctx)
        self._cos, self._sin = cos.to(self.device), sin.to(self.device)
        B.check(self.lib.vz_engine_set_rope(self.h, B.ptr(self._cos), B.ptr(self._sin), max_ctx))
        self.ready = False
        self._score = None                     # the step recorder's rings and step count while armed (set_scores)
        self._guid = None                      # the armed vz_hip.guidance.GuidanceConfig (set_guidance)
        self._beam_rows = None                 # the beam tail's row rings while armed (set_beam_rows)
        self.kv_fp8 = False
        if kv_fp8:
            self.set_kv_fp8(True)

    def set_kv_fp8(self, on: bool = True):
        """The opt-in e4m3 mirror of the KV cache (vz_hip.kv8): on, the decode attention streams one byte per cached K / V
        element plus one scale per 128 instead of two bytes, at +50 % KV memory (the bf16 cache stays for the prefills).  Switching it on
        invalidates every row's mirror: a row decodes again after a prefill or a kv_move_rows into it.  Beams, share_prompt_kv and
        speculative steps are refused while it is on.  Off by default: every call is the plain engine's."""
        from . import kv8 as KV8
        if on:
            KV8.check_engine(self.tp_size)
        B.check(self.lib.vz_engine_kv_fp8(self.h, int(bool(on))))
        self.kv_fp8 = bool(on)

    def kv8_mirror(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """a copy of the whole e4m3 mirror: (uint8 [n_layers, 2 (K|V), max_batch, kv heads, max_ctx, head_dim], fp32 scales
        [n_layers, 2, max_batch, kv heads, max_ctx]) (tests)."""
        from . import kv8 as KV8
        if not self.kv_fp8:
            raise RuntimeError("kv8_mirror: the e4m3 KV mirror is off (Engine(kv_fp8=True) / set_kv_fp8)")
        qs, ss = KV8.mirror_shape(self.cfg, self.max_batch, self.max_ctx, self.tp_size)
        q = torch.empty(qs, dtype=torch.uint8, device=self.device)
        sc = torch.empty(ss, dtype=torch.float32, device=self.device)
        nq, ns = C.c_size_t(0), C.c_size_t(0)
        B.check(self.lib.vz_llm_kv8_copy_out(self.h, None, 0, None, 0, C.byref(nq), C.byref(ns), self._s()))
        assert q.numel() == nq.value and sc.numel() == ns.value
        B.check(self.lib.vz_llm_kv8_copy_out(self.h, B.ptr(q), nq.value, B.ptr(sc), ns.value, C.byref(nq), C.byref(ns), self._s()))
        return q, sc

    def set_prefill_fp8(self, on: bool = True):
        """weight_fp8 engines: run the Zephyr prefill linears on the fp8 MFMA (activations quantised to e4m3 per row on the device,
        weights = the e4m3 copies the decode stream reads) instead of bf16 MFMA on the dequantised tensors.  Off by default."""
        B.check(self.lib.vz_engine_prefill_fp8(self.h, int(bool(on))))
        self.prefill_fp8 = bool(on)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.vz_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --------------------------------------------------------------------------------------------
    # weights
    # --------------------------------------------------------------------------------------------
    @staticmethod
    def _fp8_names(name: str):
        return (name + "8", name + "s") if name.endswith("lm_head") else (name + "8", name[:-1] + "ws")

    def _drop_fp8_copy(self, name: str):
        """the e4m3 copy + row scales of a bf16 decode weight are derived data: whoever rewrites (or replaces) the bf16 tensor
        invalidates them, so that finalize() re-quantises (a second load_weights / LoRA re-merge / resize_vocab on a
        weight_fp8 engine must not leave decode streaming the OLD e4m3 rows)."""
        self._nf4_done.discard(name)          # a rewritten tensor holds unquantised values again
        nt = name + "t"
        if nt in self.w:                      # the fragment-tiled copy of a bf16 decode weight (bf16 engines)
            del self.w[nt]
            self._registered.discard(nt)
            B.check(self.lib.vz_engine_unset_weight(self.h, nt.encode()))
        if not (self.weight_fp8 and self._FP8_NAMES.match(name)):
            return
        n8, ns = self._fp8_names(name)
        for n in (n8, ns, n8 + "t"):          # e4m3 rows, their scales, the fragment-tiled e4m3 copy
            if n in self.w:
                del self.w[n]
                self._registered.discard(n)
                B.check(self.lib.vz_engine_unset_weight(self.h, n.encode()))

    _QF_KV = re.compile(r"qf\.(\d+)\.ca_kv\.(w|b)$")

    def _dest(self, name: str, shape, dtype) -> torch.Tensor:
        self._drop_fp8_copy(name)
        t = self.w.get(name)
        if t is None:
            m = self._QF_KV.match(name)
            if m:
                # the cross-attention K|V projections of all Q-Former blocks read the same pre-normed visual features: laid out back
                # to back (block-major), vz_qformer runs them as ONE GEMM over N = blocks * 2H (whole 256^2 tiles, no stream-K tail)
                pool = self._qf_kv_pool.get(m.group(2))
                if pool is None:
                    pool = torch.zeros(self.cfg.qf_blocks, *shape, dtype=dtype, device=self.device)
                    self._qf_kv_pool[m.group(2)] = pool
                t = pool[int(m.group(1))]
            else:
                t = torch.zeros(*shape, dtype=dtype, device=self.device)
            self.w[name] = t
        return t

    def _mat(self, name, shape, src: torch.Tensor, rows: Optional[slice] = None):
        d = self._dest(name, shape, torch.bfloat16)
        s = src.to(self.device, non_blocking=True).to(torch.bfloat16)
        (d if rows is None else d[rows]).copy_(s.reshape((d if rows is None else d[rows]).shape))

    def _vec(self, name, n, src: torch.Tensor, sl: Optional[slice] = None):
        d = self._dest(name, (n,), torch.float32)
        s = src.to(self.device, non_blocking=True).to(torch.float32)
        (d if sl is None else d[sl]).copy_(s.reshape(-1))

    def add_weight(self, name: str, t: torch.Tensor) -> bool:
        """Consume one tensor under its reference state-dict key.  Returns False for keys that are
        not on the hot path (CLIP post_layernorm, buffers)."""
        cfg = self.cfg
        H, Cc, I = cfg.hidden, cfg.clip_hidden, cfg.inter
        for pre in _CLIP_PREFIXES:
            if name.startswith(pre):
                return self._add_clip(name[len(pre):], t)
        if name.startswith(_QF):
            return self._add_qformer(name[len(_QF):], t)
        t = TP.shard(name, t, self.tp_rank, self.tp_size)       # this rank's slice (identity at tp_size 1 / replicated tensors)
        I = cfg.inter // self.tp_size
        if name == "model.embed_tokens.weight":
            self._mat("llm.embed", (cfg.vocab, H), t)
        elif name == "lm_head.weight":
            self._mat("llm.lm_head", (self.vp, H), t, slice(0, t.shape[0]))
        elif name == "model.norm.weight":
            self._vec("llm.norm", H, t)
        else:
            m = re.fullmatch(r"model\.layers\.(\d+)\.(.+)", name)
            if not m:
                return False
            i, rest = int(m.group(1)), m.group(2)
            p = f"llm.{i}."
            qd, kvd = cfg.n_heads * cfg.head_dim // self.tp_size, cfg.n_kv_heads * cfg.head_dim // self.tp_size
            if rest == "input_layernorm.weight":
                self._vec(p + "in_norm", H, t)
            elif rest == "post_attention_layernorm.weight":
                self._vec(p + "post_norm", H, t)
            elif rest == "self_attn.q_proj.weight":
                self._mat(p + "qkv.w", (qd + 2 * kvd, H), t, slice(0, qd))
            elif rest == "self_attn.k_proj.weight":
                self._mat(p + "qkv.w", (qd + 2 * kvd, H), t, slice(qd, qd + kvd))
            elif rest == "self_attn.v_proj.weight":
                self._mat(p + "qkv.w", (qd + 2 * kvd, H), t, slice(qd + kvd, qd + 2 * kvd))
            elif rest == "self_attn.o_proj.weight":
                self._mat(p + "o.w", (H, qd), t)
            elif rest in ("mlp.gate_proj.weight", "mlp.up_proj.weight"):
                d = self._dest(p + "gu.w", (2 * I, H), torch.bfloat16).view(I // 16, 2, 16, H)
                d[:, 0 if "gate" in rest else 1].copy_(t.to(self.device).to(torch.bfloat16).view(I // 16, 16, H))
            elif rest == "mlp.down_proj.weight":
                self._mat(p + "down.w", (H, I), t)
            else:
                return False
        return True

    def _add_clip(self, k: str, t: torch.Tensor) -> bool:
        cfg = self.cfg
        Cc = cfg.clip_hidden
        kreal = 3 * cfg.clip_patch * cfg.clip_patch
        kpad = (kreal + 63) // 64 * 64
        if k == "embeddings.class_embedding":
            self._mat("clip.cls", (Cc,), t)
        elif k == "embeddings.patch_embedding.weight":
            d = self._dest("clip.patch_w", (Cc, kpad), torch.bfloat16)
            d[:, :kreal].copy_(t.to(self.device).to(torch.bfloat16).reshape(Cc, kreal))
        elif k == "embeddings.position_embedding.weight":
            self._mat("clip.pos", (cfg.clip_tokens, Cc), t)
        elif k.startswith("pre_layrnorm."):
            self._vec("clip.pre_ln." + ("w" if k.endswith("weight") else "b"), Cc, t)
        else:
            m = re.fullmatch(r"encoder\.layers\.(\d+)\.(.+)\.(weight|bias)", k)
            if not m:
                return False
            i, mod, wb = int(m.group(1)), m.group(2), m.group(3)
            p = f"clip.{i}."
            isw = wb == "weight"
            if mod in ("layer_norm1", "layer_norm2"):
                self._vec(p + ("ln1." if mod.endswith("1") else "ln2.") + ("w" if isw else "b"), Cc, t)
            elif mod in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"):
                j = "qkv".index(mod[-6])
                sl = slice(j * Cc, (j + 1) * Cc)
                if isw:
                    self._mat(p + "qkv.w", (3 * Cc, Cc), t, sl)
                else:
                    self._vec(p + "qkv.b", 3 * Cc, t, sl)
            elif mod == "self_attn.out_proj":
                self._mat(p + "o.w", (Cc, Cc), t) if isw else self._vec(p + "o.b", Cc, t)
            elif mod == "mlp.fc1":
                self._mat(p + "fc1.w", (cfg.clip_inter, Cc), t) if isw else self._vec(p + "fc1.b", cfg.clip_inter, t)
            elif mod == "mlp.fc2":
                self._mat(p + "fc2.w", (Cc, cfg.clip_inter), t) if isw else self._vec(p + "fc2.b", Cc, t)
            else:
                return False
        return True

    def _add_qformer(self, k: str, t: torch.Tensor) -> bool:
        cfg = self.cfg
        H, KD = cfg.hidden, cfg.qf_kv_dim
        if k == "learned_queries":
            self._mat("qf.queries", (cfg.qf_queries, H), t)
        elif k in ("pre_norm.weight", "pre_norm.bias"):
            self._vec("qf.pre_norm." + ("w" if k.endswith("weight") else "b"), KD, t)
        elif k in ("norm.weight", "norm.bias"):
            self._vec("qf.norm." + ("w" if k.endswith("weight") else "b"), H, t)
        else:
            m = re.fullmatch(r"blocks\.(\d+)\.(.+)", k)
            if not m:
                return False
            i, rest = int(m.group(1)), m.group(2)
            p = f"qf.{i}."
            mm = re.fullmatch(r"norm([123])\.(weight|bias)", rest)
            if mm:
                self._vec(p + f"n{mm.group(1)}." + ("w" if mm.group(2) == "weight" else "b"), H, t)
            elif rest == "self_attn.in_proj_weight":
                self._mat(p + "sa_in.w", (3 * H, H), t)
            elif rest == "self_attn.in_proj_bias":
                self._vec(p + "sa_in.b", 3 * H, t)
            elif rest == "self_attn.out_proj.weight":
                self._mat(p + "sa_out.w", (H, H), t)
            elif rest == "self_attn.out_proj.bias":
                self._vec(p + "sa_out.b", H, t)
            elif rest == "cross_attn.q_proj_weight":
                self._mat(p + "ca_q.w", (H, H), t)
            elif rest == "cross_attn.k_proj_weight":
                self._mat(p + "ca_kv.w", (2 * H, KD), t, slice(0, H))
            elif rest == "cross_attn.v_proj_weight":
                self._mat(p + "ca_kv.w", (2 * H, KD), t, slice(H, 2 * H))
            elif rest == "cross_attn.in_proj_bias":
                tt = t.reshape(-1)
                self._vec(p + "ca_q.b", H, tt[:H])
                self._vec(p + "ca_kv.b", 2 * H, tt[H:])
            elif rest == "cross_attn.out_proj.weight":
                self._mat(p + "ca_out.w", (H, H), t)
            elif rest == "cross_attn.out_proj.bias":
                self._vec(p + "ca_out.b", H, t)
            elif rest == "ffn.0.weight":
                self._mat(p + "ffn1.w", (2 * H, H), t)
            elif rest == "ffn.0.bias":
                self._vec(p + "ffn1.b", 2 * H, t)
            elif rest == "ffn.2.weight":
                self._mat(p + "ffn2.w", (H, 2 * H), t)
            elif rest == "ffn.2.bias":
                self._vec(p + "ffn2.b", H, t)
            else:
                return False
        return True

    def load_weights(self, named: Iterable[Tuple[str, torch.Tensor]]):
        for name, t in named:
            self.add_weight(name, t)
        self.finalize()

    def init_comm(self):
        """create the RCCL communicator of a tensor-parallel engine: rank 0's unique id travels over torch.distributed
        (already initialised by the launcher), then every rank joins."""
        if self.tp_size == 1:
            return
        import torch.distributed as dist
        buf = C.create_string_buffer(128)
        if self.tp_rank == 0:
            B.check(self.lib.vz_comm_unique_id(buf))
        box = [bytes(buf.raw)]
        dist.broadcast_object_list(box, src=0)
        B.check(self.lib.vz_comm_init(self.h, box[0]))
        if os.environ.get("VZ_TP_ONESHOT", "0") == "1":
            self.init_oneshot()

    def init_oneshot(self) -> bool:
        """Opt-in (VZ_TP_ONESHOT=1): the decode step's [B, hidden] all-reduces on the one-shot kernel (csrc/comm_oneshot.hip) instead of
        RCCL - every rank's receive area is exported with hipIpcGetMemHandle, the handles travel over torch.distributed, the peers' areas
        are opened with hipIpcOpenMemHandle (peer-mapped over xGMI) and handed to the engine in rank order.  Returns False (RCCL stays)
        if any rank fails to map a peer.  UNMEASURED: no multi-GPU box has been available to the build; the kernel's protocol and
        arithmetic are tested in one process (tests/test_oneshot_gpu.py), this wiring only by tests/test_tp_gloo.py's dry plan."""
        import torch.distributed as dist
        class IpcHandle(C.Structure):                            # hipIpcMemHandle_t: 64 opaque bytes, passed BY VALUE to hipIpcOpenMemHandle
            _fields_ = [("reserved", C.c_char * 64)]
        hip = C.CDLL("libamdhip64.so")
        hip.hipIpcGetMemHandle.argtypes = [C.POINTER(IpcHandle), C.c_void_p]
        hip.hipIpcOpenMemHandle.argtypes = [C.POINTER(C.c_void_p), IpcHandle, C.c_uint]
        area, nbytes = C.c_void_p(), C.c_size_t()
        B.check(self.lib.vz_comm_oneshot_local(self.h, C.byref(area), C.byref(nbytes)))
        handle = IpcHandle()
        ok = hip.hipIpcGetMemHandle(C.byref(handle), area) == 0
        box = [None] * self.tp_size
        dist.all_gather_object(box, (ok, bytes(C.string_at(C.byref(handle), 64))))
        areas = (C.c_void_p * self.tp_size)()
        good = all(o for o, _ in box)
        if good:
            for q, (_, h) in enumerate(box):
                if q == self.tp_rank:
                    areas[q] = area.value
                    continue
                peer = C.c_void_p()
                hq = IpcHandle()
                C.memmove(C.byref(hq), h, 64)
                if hip.hipIpcOpenMemHandle(C.byref(peer), hq, 1) != 0:        # hipIpcMemLazyEnablePeerAccess
                    good = False
                    break
                areas[q] = peer.value
        flags = [None] * self.tp_size
        dist.all_gather_object(flags, bool(good))
        if not all(flags):
            return False
        B.check(self.lib.vz_comm_oneshot_attach(self.h, areas, self.tp_size))
        self.oneshot = True
        return True

    def resize_vocab(self, n: int):
        """grow (new rows = mean of the old ones, as vz_hip.weights.resize_vocab does at load time) or shrink the
        embedding and lm_head tables of a live engine (HF `resize_token_embeddings`; ref builder.py:141-153)."""
        import dataclasses
        if self.tp_size != 1:
            raise NotImplementedError("resize_vocab on a tensor-parallel engine: rebuild it at the new vocabulary")
        old = self.cfg.vocab
        if n == old:
            return
        tables = {}
        for name in ("llm.embed", "llm.lm_head"):
            t = self.w[name]
            if n > old:
                extra = t.float().mean(0, keepdim=True).to(t.dtype).expand(n - old, -1)
                tables[name] = torch.cat([t, extra], 0).contiguous()
            else:
                tables[name] = t[:n].contiguous()
        torch.cuda.synchronize(self.device)
        B.check(self.lib.vz_engine_resize_vocab(self.h, n))
        self.cfg = dataclasses.replace(self.cfg, vocab=n)
        self.vp = n
        for name, t in tables.items():
            self._drop_fp8_copy(name)          # old-size e4m3 table / scales of lm_head
            self.w[name] = t
            self._registered.discard(name)
        self.finalize()

    def init_comm_single_rank(self):
        """self-test: give a tp_size == 1 engine a ONE-rank RCCL communicator; with vz_tune_set(7, 1) its all-reduce /
        all-gather call sites then really go through RCCL (identity results) on a single GPU."""
        assert self.tp_size == 1
        buf = C.create_string_buffer(128)
        B.check(self.lib.vz_comm_unique_id(buf))
        B.check(self.lib.vz_comm_init(self.h, bytes(buf.raw)))

    def all_gather(self, send: torch.Tensor) -> torch.Tensor:
        """RCCL all-gather of one equally sized contiguous tensor per rank -> [tp_size, *send.shape] (rank order)."""
        send = send.to(self.device).contiguous()
        recv = torch.empty((self.tp_size,) + tuple(send.shape), dtype=send.dtype, device=self.device)
        B.check(self.lib.vz_tp_all_gather(self.h, B.ptr(send), B.ptr(recv), send.numel() * send.element_size(), self._s()))
        return recv

    def load_synthetic(self, seed: int = 0):
        """hash-generated weights, produced on the device (bit-identical to the CPU generator)."""
        self.load_weights(iter_state_dict(self.cfg, seed, device=self.device))

    _FP8_NAMES = re.compile(r"llm\.(\d+\.(qkv|o|gu|down)\.w|lm_head)$")

    def _quantize_decode_weights(self):
        """weight_fp8: every decode-side Zephyr linear gets an e4m3 copy + per-row 2^e scales (vz_hip/quant.py); the bf16
        tensor is replaced by the exactly-equal dequantised values, so prefill (bf16 MFMA) and decode (fp8 stream) agree."""
        from . import quant
        for name in [n for n in self.w if self._FP8_NAMES.match(n)]:
            n8, ns = self._fp8_names(name)
            if n8 in self.w:
                continue
            w = self.w[name]
            w8, scale = quant.quantize_rows(w)
            w.copy_(quant.dequantize_rows(w8, scale).to(torch.bfloat16))
            self.w[n8], self.w[ns] = w8.contiguous(), scale.contiguous()
            self._registered.discard(name)

    def _tile_decode_weights(self):
        """every decode-side Zephyr linear gets a copy in MFMA-fragment order that the 2..64-row decode steps stream with 1-KiB
        wave-instructions; same values, same k order as the row-major tensor the prefill GEMMs and the 1-row GEMV keep using.
        bf16 engines: vz_op_tile_weights on the bf16 tensors (+14.5 GB for Zephyr-7B).  e4m3 engines (round 3): vz_op_tile_weights_fp8
        on the e4m3 copies (+7.3 GB; their 17..64-row steps stream those, 2..16 rows keep the row-major e4m3 rows).
        VZ_DECODE_TILED=0 turns it off."""
        if os.environ.get("VZ_DECODE_TILED", "1") == "0":
            return
        for name in [n for n in self.w if self._FP8_NAMES.match(n)]:
            if self.weight_fp8:
                n8 = self._fp8_names(name)[0]
                w8 = self.w.get(n8)
                if w8 is None or n8 + "t" in self.w or w8.shape[0] % 128 or w8.shape[1] % 1024:
                    continue
                self.w[n8 + "t"] = B.tile_weights_fp8(w8)
                continue
            w = self.w[name]
            if name + "t" in self.w or w.shape[0] % 16 or w.shape[1] % 64:
                continue
            self.w[name + "t"] = B.tile_weights(w)

    _NF4_NAMES = re.compile(r"llm\.\d+\.(qkv|o|gu|down)\.w$")       # the decoder layers' linears; lm_head stays as it is (bitsandbytes' default skip list)

    def _nf4_decode_weights(self):
        """weight_nf4 (`load_4bit`): every decoder-layer linear is replaced by its NF4 fake-quantisation (vz_hip/quant.py: 64-element
        blocks, fp32 absmax) rounded to bf16; every kernel then runs on those values - the 4-bit model on the bf16 engine."""
        from . import quant
        for name in [n for n in self.w if self._NF4_NAMES.match(n) and n not in self._nf4_done]:
            w = self.w[name]
            w.copy_(quant.fake_quantize_nf4(w).to(torch.bfloat16))
            self._nf4_done.add(name)
            self._registered.discard(name)

    def finalize(self):
        if self.weight_nf4:
            self._nf4_decode_weights()
        if self.weight_fp8:
            self._quantize_decode_weights()
        if self.max_batch > (16 if self.weight_fp8 else 1):      # (an e4m3 engine streams row-major e4m3 rows up to 16 rows, the tiled e4m3 copies beyond)
            self._tile_decode_weights()
        for name, t in self.w.items():
            if name in self._registered:
                continue
            B.check(self.lib.vz_engine_set_weight(self.h, name.encode(), B.ptr(t),
                                                  0 if t.dtype == torch.bfloat16 else (2 if t.dtype == torch.uint8 else 1),
                                                  t.numel()))
            self._registered.add(name)
        B.check(self.lib.vz_engine_finalize(self.h))
        self.ready = True

    # --------------------------------------------------------------------------------------------
    # stages
    # --------------------------------------------------------------------------------------------
    def _s(self):
        return B.stream_ptr(self.device)

    def clip_fused_features(self, images: torch.Tensor, return_hidden: bool = False):
        """images [T,3,336,336] -> bf16 [T,576,5*C]  (+ all hidden states [L+1,T,577,C] for tests)."""
        cfg = self.cfg
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] != cfg.clip_image or images.shape[3] != cfg.clip_image:
            raise ValueError(f"Input image size ({images.shape[-2]}*{images.shape[-1]}) doesn't match model "
                             f"({cfg.clip_image}*{cfg.clip_image}).")
        x = images.to(self.device, torch.bfloat16).contiguous()
        T = x.shape[0]
        out = torch.empty(T, cfg.vision_tokens, (cfg.fusion_groups + 1) * cfg.clip_hidden, dtype=torch.bfloat16,
                          device=self.device)
        hid = None
        if return_hidden:
            hid = torch.empty(cfg.clip_layers + 1, T, cfg.clip_tokens, cfg.clip_hidden, dtype=torch.bfloat16,
                              device=self.device)
        B.check(self.lib.vz_clip_fused_features(self.h, B.ptr(x), T, B.ptr(out), B.ptr(hid), self._s()))
        return (out, hid) if return_hidden else out

    def qformer(self, feats: torch.Tensor, text: Optional[torch.Tensor], tile_sample: Sequence[int]):
        """feats bf16 [T,576,5120]; text bf16 [n_samples,Lmax,H] or None; tile_sample[t] = sample of tile t."""
        cfg = self.cfg
        feats = feats.to(self.device, torch.bfloat16).contiguous()
        T = feats.shape[0]
        if text is not None and text.shape[1] == 0:
            text = None
        if text is not None:
            text = text.to(self.device, torch.bfloat16).contiguous()
            n_samples, Lmax = text.shape[0], text.shape[1]
        else:
            n_samples, Lmax = (max(tile_sample) + 1 if len(tile_sample) else 1), 0
        ts = (C.c_int * T)(*[int(v) for v in tile_sample])
        out = torch.empty(T, cfg.qf_queries, cfg.hidden, dtype=torch.bfloat16, device=self.device)
        B.check(self.lib.vz_qformer(self.h, B.ptr(feats), T, B.ptr(text), n_samples, Lmax, ts, B.ptr(out), self._s()))
        return out

    def embed_tokens(self, ids: torch.Tensor) -> torch.Tensor:
        ids32 = ids.to(self.device, torch.int32).contiguous().view(-1)
        if ids32.numel() == 0:
            return torch.empty(*ids.shape, self.cfg.hidden, dtype=torch.bfloat16, device=self.device)
        if int(ids32.min()) < 0 or int(ids32.max()) >= self.cfg.vocab:
            raise IndexError("token id out of range for embed_tokens")
        out = torch.empty(ids32.numel(), self.cfg.hidden, dtype=torch.bfloat16, device=self.device)
        B.check(self.lib.vz_embed_splice(self.h, None, B.ptr(ids32), ids32.numel(), None, B.ptr(out), self._s()))
        return out.view(*ids.shape, self.cfg.hidden)

    def splice(self, kind: torch.Tensor, idx: torch.Tensor, visual: Optional[torch.Tensor]) -> torch.Tensor:
        """rows: kind 0 = embedding row idx, 1 = visual row idx, 2 = zero."""
        kind = kind.to(self.device, torch.int32).contiguous()
        idx = idx.to(self.device, torch.int32).contiguous()
        out = torch.empty(kind.numel(), self.cfg.hidden, dtype=torch.bfloat16, device=self.device)
        vis = None if visual is None else visual.to(torch.bfloat16).contiguous()
        B.check(self.lib.vz_embed_splice(self.h, B.ptr(kind), B.ptr(idx), kind.numel(), B.ptr(vis), B.ptr(out), self._s()))
        return out

    def prefill(self, embeds: torch.Tensor, seqlens: Sequence[int], position_ids: Optional[torch.Tensor] = None,
                all_logits: bool = False, last_logits: bool = True):
        """embeds bf16 [B,S,H] right-padded.  Returns (logits_all fp32 [B,S,V] | None, logits_last fp32 [B,V] | None)."""
        x, pos, la, ll, (sl,) = self._rows_call(embeds, position_ids, None, all_logits, last_logits, seqlens)
        B.check(self.lib.vz_llm_prefill(self.h, B.ptr(x), x.shape[0], x.shape[1], sl, B.ptr(pos), B.ptr(la), B.ptr(ll), self._s()))
        return la, ll

    def _rows_call(self, embeds, position_ids, past_lens, all_logits, last_logits, *lens):
        """what the prefill calls hand the library: embeds as contiguous bf16 [B,T,H], int32 positions [B,T] (default past + t, the
        padding rows of an append kept inside the rotary tables), the two logits outputs (or None), each of `lens` as a c_int array."""
        x = embeds.to(self.device, torch.bfloat16).contiguous()
        Bn, T = x.shape[0], x.shape[1]
        if position_ids is None and past_lens is None:
            position_ids = torch.arange(T, dtype=torch.int32, device=self.device).unsqueeze(0).expand(Bn, T)
        elif position_ids is None:
            position_ids = (torch.tensor([int(p) for p in past_lens], dtype=torch.int32).unsqueeze(1)
                            + torch.arange(T, dtype=torch.int32).unsqueeze(0)).clamp_(max=self.max_ctx - 1)
        pos = position_ids.to(self.device, torch.int32).contiguous()
        la = torch.empty(Bn, T, self.cfg.vocab, dtype=torch.float32, device=self.device) if all_logits else None
        ll = torch.empty(Bn, self.cfg.vocab, dtype=torch.float32, device=self.device) if last_logits else None
        return x, pos, la, ll, [(C.c_int * Bn)(*[int(v) for v in l]) for l in lens]

    def prefill_rows(self, row0: int, embeds: torch.Tensor, seqlens: Sequence[int], position_ids: Optional[torch.Tensor] = None):
        """`prefill` into KV-cache rows row0 .. row0+B-1 (continuous batching); returns the last-position logits fp32 [B,V]."""
        x, pos, _, ll, (sl,) = self._rows_call(embeds, position_ids, None, False, True, seqlens)
        B.check(self.lib.vz_llm_prefill_rows(self.h, int(row0), B.ptr(x), x.shape[0], x.shape[1], sl, B.ptr(pos), None, B.ptr(ll), self._s()))
        return ll

    def prefill_append(self, row0: int, embeds: torch.Tensor, new_lens: Sequence[int], past_lens: Sequence[int],
                       position_ids: Optional[torch.Tensor] = None, all_logits: bool = False, last_logits: bool = True):
        """embeds bf16 [B,T,H] right-padded: new_lens[b] rows go behind the past_lens[b] positions cache row row0+b keeps, at cache
        slots past+t and rotary positions position_ids[b,t] (default past+t).  Returns (logits_all fp32 [B,T,V] | None, logits_last
        fp32 [B,V] | None); logits_all rows t >= new_lens[b] come from padding."""
        Bn, T = embeds.shape[0], embeds.shape[1]
        if len(new_lens) != Bn or len(past_lens) != Bn:
            raise ValueError(f"prefill_append: {Bn} samples, {len(new_lens)} new lengths, {len(past_lens)} past lengths")
        x, pos, la, ll, (nl, pl) = self._rows_call(embeds, position_ids, past_lens, all_logits, last_logits, new_lens, past_lens)
        if tuple(pos.shape) != (Bn, T):
            raise ValueError(f"prefill_append: position_ids {tuple(pos.shape)}, expected {(Bn, T)}")
        B.check(self.lib.vz_llm_prefill_append(self.h, int(row0), B.ptr(x), Bn, T, nl, pl, B.ptr(pos), B.ptr(la), B.ptr(ll), self._s()))
        return la, ll

    def kv_move_rows(self, src: Sequence[int], dst: Sequence[int], lens: Sequence[int]):
        """first lens[i] cache positions of row src[i] -> row dst[i] (all layers), stream-ordered behind the prefill that wrote them."""
        n = len(src)
        assert n == len(dst) == len(lens) and n >= 1
        arr = lambda v: (C.c_int * n)(*[int(x) for x in v])    # noqa: E731
        B.check(self.lib.vz_llm_kv_move_rows(self.h, n, arr(src), arr(dst), arr(lens), self._s()))

    def decode_set_row(self, row: int, token: int, next_pos: int, ctx_len: int):
        """(re)arm one row of the running decode batch; ctx_len 0 parks it."""
        B.check(self.lib.vz_llm_decode_set_row(self.h, int(row), int(token), int(next_pos), int(ctx_len), self._s()))

    def decode_begin(self, first_ids: torch.Tensor, next_pos: Sequence[int], ctx_len: Sequence[int]):
        ids = first_ids.to(self.device, torch.int32).contiguous().view(-1)
        Bn = ids.numel()
        np_ = (C.c_int * Bn)(*[int(v) for v in next_pos])
        cl = (C.c_int * Bn)(*[int(v) for v in ctx_len])
        self._dec_keep = ids
        self._spec = None                  # a new batch starts with the plain tail (the library clears the mode too)
        B.check(self.lib.vz_llm_decode_begin(self.h, Bn, B.ptr(ids), np_, cl, self._s()))
        self._dec_B = Bn
        if self._score is not None:
            self._score["count"] = 0       # the recorder's ring restarts with the batch

    def decode_steps(self, n: int, out: Optional[torch.Tensor] = None, return_logits: bool = False):
        """enqueue n greedy steps; returns int32 [B,n] (device; no host sync) (+ fp32 logits [n,B,V]).  With the speculative tail
        armed (`set_spec`): n verify steps, then ONE readback - returns the 1-D int32 ids (host) those n steps emitted."""
        Bn = self._dec_B
        sp = getattr(self, "_spec", None)
        if sp is not None:
            lg = torch.empty(n, Bn, self.cfg.vocab, dtype=torch.float32, device=self.device) if return_logits else None
            B.check(self.lib.vz_llm_decode_steps(self.h, n, B.ptr(sp["out"]), B.ptr(lg), self._s()))
            host = sp["buf"][:sp["head"]].cpu()                  # control words | emitted ids | stats records: one copy, one sync
            w0, w1 = sp["w"], int(host[B.SPEC_CTL_WRITE])
            s0, s1 = sp["steps"], int(host[B.SPEC_CTL_STEPS])
            sp["w"], sp["steps"], sp["done"] = w1, s1, bool(host[B.SPEC_CTL_DONE])
            rec = host[B.SPEC_CTL_WORDS + sp["budget"]:].view(-1, 3)[s0:min(s1, sp["budget"])]
            sp["records"].extend(rec.tolist())
            ids = host[B.SPEC_CTL_WORDS + w0:B.SPEC_CTL_WORDS + w1].clone()
            return (ids, lg) if return_logits else ids
        rows = Bn if self._guid is None else self._guid.pairs      # a guided batch: ids and records of its conditional rows only
        if out is None:
            out = torch.empty(rows, n, dtype=torch.int32, device=self.device)
        lg = torch.empty(n, Bn, self.cfg.vocab, dtype=torch.float32, device=self.device) if return_logits else None
        sc = self._score
        if sc is not None and sc["rows"] != rows:        # the rings are [cap_steps][rows]: the recorder writes one record per row of the batch
            raise ValueError(f"decode_steps: the step recorder was armed for {sc['rows']} rows (set_scores), the decode batch has {rows}")
        B.check(self.lib.vz_llm_decode_steps(self.h, n, B.ptr(out), B.ptr(lg), self._s()))
        if sc is not None:
            sc["count"] += n
        return (out, lg) if return_logits else out

    def set_scores(self, cap_steps: Optional[int] = None, rows: int = 1, warped: bool = False, raw: bool = False):
        """the step recorder (sampling.hip: token_scores_kernel): every step of a `rows`-row decode batch records (x_tok, lse, lse_kept,
        n_kept) per row about the token its tail chose - with `warped` also the score rows HF calls scores[t], with `raw` the logits rows
        as the lm_head left them - into device rings of `cap_steps` steps, read with `scores_steps`.  None = off.  Arming restarts the
        ring, as `decode_begin` does; `decode_steps` refuses more than `cap_steps` steps per call."""
        if cap_steps is None:
            self._score = None
            B.check(self.lib.vz_llm_decode_scores(self.h, 0, None, None, None, 0, self._s()))
            return
        cap, rows, V = int(cap_steps), int(rows), self.cfg.vocab
        sc = {"cap": cap, "rows": rows, "count": 0, "rec": torch.zeros(cap, rows, 4, dtype=torch.float32, device=self.device),
              "warped": torch.empty(cap, rows, V, dtype=torch.float32, device=self.device) if warped else None,
              "raw": torch.empty(cap, rows, V, dtype=torch.float32, device=self.device) if raw else None}
        what = B.SCORE_REC | (B.SCORE_WARPED if warped else 0) | (B.SCORE_RAW if raw else 0)
        B.check(self.lib.vz_llm_decode_scores(self.h, what, B.ptr(sc["rec"]), B.ptr(sc["warped"]), B.ptr(sc["raw"]), cap, self._s()))
        self._score = sc

    def scores_steps(self, n: int, first: Optional[int] = None):
        """what the recorder holds of `n` steps, from step `first` counted from the last `decode_begin` / `set_scores` (default: the last
        n): (records fp32 [n, rows, 4], warped rows [n, rows, V] or None, raw rows or None), device tensors in step order."""
        from . import scores as SC
        sc = self._score
        assert sc is not None, "scores_steps: the recorder is off (set_scores)"
        pick = lambda ring: None if ring is None else SC.ring_order(ring, sc["count"], n, first)      # noqa: E731
        return pick(sc["rec"]), pick(sc["warped"]), pick(sc["raw"])

    def set_stop(self, plan=None):
        """the stop matcher (stop.hip: stop_match_kernel): every decode step passes the token each row's tail chose through the stop
        conditions of `plan` (vz_hip.stop.Plan) and records the index of the token at which one first held (`stop_at`); None = off.  A
        row is watched from `stop_rows` on.  The tables are copied into the engine's own device memory; the step's graph is captured
        once more when the matcher comes or goes."""
        if plan is None:
            B.check(self.lib.vz_llm_decode_stop(self.h, 0, None, 0, 0, 0, 0, 0, 0, None, None, 0, self._s()))
            return
        seq = plan.seq_table().contiguous() if plan.seqs else None
        emb = None if plan.emb is None else plan.emb.to("cpu", torch.int32).contiguous()
        tgt = None if plan.target is None else plan.target.to("cpu", torch.int32).contiguous()
        B.check(self.lib.vz_llm_decode_stop(self.h, 1, B.ptr(emb), 0 if emb is None else emb.shape[0], plan.vec, plan.n_str, plan.max_pos, plan.max_end,
                                            plan.window, B.ptr(tgt), B.ptr(seq), len(plan.seqs), self._s()))

    def stop_rows(self, row0: int, first_ids: torch.Tensor):
        """rows row0.. of the matcher start clean and take their first tokens (chosen from the prefill logits) through the step's own
        kernel: call it where `decode_begin` / `decode_set_row` arm those rows"""
        ids = first_ids.to(self.device, torch.int32).contiguous().view(-1)
        B.check(self.lib.vz_llm_decode_stop_rows(self.h, int(row0), ids.numel(), B.ptr(ids), self._s()))

    def seed_history(self, rows, proc: bool = False, stop: bool = False):
        """rows: per cache row the ids that were fed before generation begins (a call that continues on a kept cache).  proc: they become
        the logits processors' histories (min_new_tokens still counts generated ids only); stop: their tails enter the stop matcher's
        rings, so a stop string may begin in them.  Behind `set_logits_proc` / `set_stop`, in front of `decode_begin` / `stop_rows`."""
        for r, ids in enumerate(rows):
            ids = [int(t) for t in ids]
            if proc:
                tail = ids[-self.max_ctx:]
                B.check(self.lib.vz_llm_decode_logits_proc_seed(self.h, r, (C.c_int * len(tail))(*tail), len(tail), self._s()))
            if stop:
                tail = ids[-63:]
                B.check(self.lib.vz_llm_decode_stop_seed(self.h, r, (C.c_int * len(tail))(*tail), len(tail), self._s()))

    def stop_at(self, row0: int, rows: int) -> torch.Tensor:
        """int32 [rows] (device): per row -1, or the 0-based index of the generated token at which a stop condition first held"""
        at = torch.empty(int(rows), dtype=torch.int32, device=self.device)
        B.check(self.lib.vz_llm_decode_stop_read(self.h, int(row0), int(rows), B.ptr(at), self._s()))
        return at

    def set_sampling(self, on: bool, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0, first_counter: int = 1,
                     warp=None):
        """tail of every decode step: greedy argmax (off) or the device-side sampler (sampling.hip); applies from the next decode_begin.
        warp: None, or (min_p, typical_p, epsilon_cutoff, eta_cutoff) behind top-p, 0 = off (vz_hip.sample_rows.RowParams.warp)."""
        w = warp or (0.0, 0.0, 0.0, 0.0)
        rec = B.VzSampleParams(B.ROW_SAMPLE if on else B.ROW_GREEDY, float(temperature), int(top_k or 0), float(1.0 if top_p is None else top_p),
                               int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_counter), 0, *(float(v) for v in w))
        B.check(self.lib.vz_llm_decode_sampling(self.h, C.byref(rec)))

    def set_sampling_rows(self, params=None):
        """the per-row tail (sampling.hip: sample_rows_kernel): params = a list of vz_hip.sample_rows.RowParams, one per row of the NEXT
        decode_begin (rows behind the list, or an empty list: greedy until `decode_set_row_sampling` arms them); None = off."""
        if params is None:
            B.check(self.lib.vz_llm_decode_sampling_rows(self.h, 0, 0, None))
            return
        B.check(self.lib.vz_llm_decode_sampling_rows(self.h, 1, len(params), B.sample_params(params)))

    def decode_set_row_sampling(self, row: int, p):
        """one row's entry of the running batch's per-row table (p: vz_hip.sample_rows.RowParams), stream-ordered like `decode_set_row`."""
        B.check(self.lib.vz_llm_decode_set_row_sampling(self.h, int(row), B.sample_params([p]), self._s()))

    def set_logits_proc(self, cfg=None):
        """HF's logits processors in front of the argmax / the sampler of every decode step (logits_proc.hip; cfg =
        vz_hip.logits_proc.parse(...), None = off).  Arming empties every row's history of generated ids: call it before
        `decode_begin`, after the first token was chosen on logits that went through `binding.logits_process`."""
        if cfg is None:
            B.check(self.lib.vz_llm_decode_logits_proc(self.h, None, self._s()))
            return
        B.check(self.lib.vz_llm_decode_logits_proc(self.h, C.byref(B.proc_params(cfg)), self._s()))

    def set_logits_proc_rows(self, on: bool):
        """the per-row logits processors (logits_proc.hip: logits_process_rows_kernel): armed, every decode step runs each row's logits
        through that row's own record of a device table, in front of the argmax / the sampler / the per-row tail.  Arming leaves every
        record inactive and every history empty; `decode_set_row_logits_proc` arms a row.  Not together with `set_logits_proc`."""
        B.check(self.lib.vz_llm_decode_logits_proc_rows(self.h, int(bool(on)), self._s()))

    def decode_set_row_logits_proc(self, row: int, cfg=None):
        """one row's record and id sequences (cfg = vz_hip.logits_proc.parse(...); None: the row is left alone from now on), stream-ordered
        like `decode_set_row`; the row's history restarts empty.  Captures nothing."""
        seq = cfg.seq_table() if cfg is not None and cfg.seq else []
        B.check(self.lib.vz_llm_decode_set_row_logits_proc(self.h, int(row), C.byref(B.proc_row(cfg)) if cfg is not None else None,
                                                           (C.c_int * len(seq))(*seq) if seq else None, len(seq) // 12, self._s()))

    def set_stop_row_seqs(self, on: bool):
        """per-row stop sequences (stop.hip): armed - behind `set_stop(plan)`, or on its own - the matcher's id-sequence rule reads each
        row's own sequences; every row starts with the call's (`plan.seqs`) and unwatched.  Disarm it before `set_stop` is called again."""
        B.check(self.lib.vz_llm_decode_stop_row_seqs(self.h, int(bool(on)), self._s()))

    def decode_set_row_stop_seqs(self, row: int, seqs=()):
        """one row's own stop sequences (id lists; behind the call's, together at most 16), stream-ordered; call `stop_rows` behind it"""
        from . import stop as ST
        tab = ST.row_seq_table(seqs).contiguous() if seqs else None
        B.check(self.lib.vz_llm_decode_stop_set_row_seqs(self.h, int(row), B.ptr(tab), len(seqs), self._s()))

    def set_guidance(self, cfg=None):
        """HF's classifier-free guidance in every decode step (guidance.hip; cfg = vz_hip.guidance.GuidanceConfig, None = off): the NEXT
        `decode_begin` takes 2 * cfg.pairs rows - row r < pairs a prompt, row pairs + r its negative prompt - and every step combines each
        pair's logits into row r's in front of the processors and the tail, which then run on the first `pairs` rows only: `decode_steps`
        returns [pairs, n] ids, and `set_scores` / `set_sampling_rows` / `stop_rows` / `set_ring` describe `pairs` rows."""
        if cfg is None:
            self._guid = None
            B.check(self.lib.vz_llm_decode_guidance(self.h, 0, 1.0, 0, self._s()))
            return
        B.check(self.lib.vz_llm_decode_guidance(self.h, 1, float(cfg.scale), int(cfg.pairs), self._s()))
        self._guid = cfg

    def set_share(self, plan=None):
        """Shared-prefix decode attention (attn_shared.hip; plan = vz_hip.share.Plan, None = off): the NEXT
        `decode_begin` takes len(plan.shared) * plan.n rows, and the n adjacent rows of group g read their first plan.shared[g] cache slots
        from cache row g * n - nothing is copied into the other rows.  Armed, the engine refuses what would write into those slots."""
        if plan is None:
            B.check(self.lib.vz_llm_decode_share(self.h, 0, None, 0, self._s()))
            return
        tab = (C.c_int * len(plan.shared))(*[int(v) for v in plan.shared])
        B.check(self.lib.vz_llm_decode_share(self.h, int(plan.n), tab, len(plan.shared), self._s()))

    def set_ring(self, ring: Optional[torch.Tensor]):
        """host-visible (pinned) int32 ring the step tails write their tokens to: [slots] for a one-row batch or [rows, slots]
        (slot = draw counter mod slots); None = off.  decode_steps refuses a batch with more rows than the ring has."""
        rows = slots = 0
        if ring is not None:
            assert ring.dtype == torch.int32 and ring.is_pinned() and ring.dim() in (1, 2) and ring.is_contiguous() and ring.shape[-1] >= 2
            rows, slots = (1 if ring.dim() == 1 else int(ring.shape[0])), int(ring.shape[-1])
        self._ring_keep = ring
        B.check(self.lib.vz_llm_decode_ring(self.h, B.ptr(ring), slots, rows))

    def set_spec(self, on: bool, D: int = 0, max_ngram: int = 2, history: Sequence[int] = (), eos: Sequence[int] = (), budget: int = 0,
                 source: int = 0, stream: Optional[Sequence[int]] = None, sample=None):
        """prompt-lookup speculative decoding (spec.hip) for the R = D + 1 rows `decode_begin` just armed (one sequence: row i at
        position p + i, context L + i): every decode step becomes a verify step that emits 1..R ids, at most `budget` in all, and
        stops at the first of `eos`.  history = one id per position of the sequence so far, the token of row 0 included (-1 = no text
        id there).  source 0 drafts by the n-gram rule; 1 drafts the ids of `stream` that follow the step's own position (stream[t]
        = the t-th id these steps are expected to emit: tests, benchmarks).  sample (a sampled vz_hip.sample_rows.RowParams; its
        counter is not read): the verify steps draw their rows instead of taking the argmax, row i at the draw counter of the token it
        would emit (sampling.hip: spec_sample_kernel).  off: the plain tail again."""
        if not on:
            self._spec = None
            B.check(self.lib.vz_llm_decode_spec(self.h, 0, 0, 0, None, 0, 0, None, 0, None, 0, None, None, 0, 0, None, 0, self._s()))
            return
        budget = int(budget)
        head = B.SPEC_CTL_WORDS + 4 * budget                      # control words | out [budget] | stats [budget][3]
        buf = torch.zeros(head + 1, dtype=torch.int32, device=self.device)
        hist = torch.tensor(list(history) + [0] * budget, dtype=torch.int32).to(self.device) if source == 0 else None
        sids = torch.tensor(list(stream if stream is not None else []) + [0], dtype=torch.int32).to(self.device) if source == 1 else None
        ea = (C.c_int * max(1, len(eos)))(*[int(t) for t in eos])
        out, stats = buf[B.SPEC_CTL_WORDS:], buf[B.SPEC_CTL_WORDS + budget:]
        B.check(self.lib.vz_llm_decode_spec(self.h, 1, int(D), int(max_ngram), B.ptr(hist), len(history), 0 if hist is None else hist.numel(),
                                            ea, len(eos), B.ptr(out), budget, B.ptr(buf), B.ptr(stats), budget, int(source), B.ptr(sids),
                                            0 if sids is None else sids.numel() - 1, self._s()))
        if sample is not None and sample.sample:
            B.check(self.lib.vz_llm_decode_spec_sampling(self.h, B.sample_params([sample])))
        self._spec = {"buf": buf, "out": out, "hist": hist, "stream": sids, "head": head, "budget": budget, "D": int(D), "w": 0, "steps": 0,
                      "done": budget == 0, "records": []}

    def spec_state(self) -> dict:
        """what the last readback of the speculative tail showed: done flag, steps run, ids emitted, per-step [drafted, used, emitted]."""
        sp = self._spec
        return {"done": sp["done"], "steps": sp["steps"], "tokens": sp["w"], "records": sp["records"], "D": sp["D"]}

    def set_beam(self, on: bool, num_beams: int = 0, groups: int = 0, eos: Sequence[int] = (), base: Sequence[int] = (),
                 scores: Optional[torch.Tensor] = None, hist: Optional[torch.Tensor] = None):
        """tail of every decode step: beam selection on the device (beam.hip) for `groups` prompts x `num_beams` rows of the running
        batch, running scores fp32 [groups * num_beams], prompt lengths `base` (the cache from there on follows the chosen parents),
        history records hist int32 [steps, groups, K, 3] written at a device-side step index that restarts at 0 here.  off: argmax /
        the sampler again."""
        if not on:
            self._beam_keep = None
            B.check(self.lib.vz_llm_decode_beam(self.h, 0, 0, 0, None, 0, None, None, None, 0, self._s()))
            return
        eos = [int(t) for t in eos]
        scores = scores.to(self.device, torch.float32).contiguous()
        assert hist is not None and hist.dtype == torch.int32 and hist.is_contiguous() and hist.dim() == 4
        self._beam_keep = (scores, hist)
        ea = (C.c_int * max(1, len(eos)))(*eos)
        ba = (C.c_int * len(base))(*[int(v) for v in base])
        B.check(self.lib.vz_llm_decode_beam(self.h, 1, int(num_beams), int(groups), ea, len(eos), ba, B.ptr(scores), B.ptr(hist),
                                            int(hist.shape[0]), self._s()))

    def set_beam_rows(self, cap_steps: Optional[int] = None, rows: int = 0, scores: bool = False, raw: bool = False):
        """the beam tail's row recorder (beam.hip): every beam step of a `rows`-row batch copies its processed log-prob rows (`scores`:
        HF's scores[t]) and / or its logits rows (`raw`) into device rings of `cap_steps` steps, inside the step; read with
        `beam_rows_steps`.  None = off.  The ring slot is the beam tail's history index, which `set_beam` restarts."""
        if cap_steps is None or not (scores or raw):
            self._beam_rows = None
            B.check(self.lib.vz_llm_decode_beam_rows(self.h, None, None, 0))
            return
        cap, rows, V = int(cap_steps), int(rows), self.cfg.vocab
        ring = lambda on: torch.empty(cap, rows, V, dtype=torch.float32, device=self.device) if on else None      # noqa: E731
        br = {"cap": cap, "scores": ring(scores), "raw": ring(raw)}
        B.check(self.lib.vz_llm_decode_beam_rows(self.h, B.ptr(br["scores"]), B.ptr(br["raw"]), cap))
        self._beam_rows = br

    def beam_rows_steps(self, count: int, n: int):
        """the rows of the last `n` of the `count` beam steps run since `set_beam`: (scores [n, rows, V] or None, raw or None), device
        tensors in step order"""
        from . import scores as SC
        br = self._beam_rows
        assert br is not None, "beam_rows_steps: the row recorder is off (set_beam_rows)"
        pick = lambda ring: None if ring is None else SC.ring_order(ring, count, n)      # noqa: E731
        return pick(br["scores"]), pick(br["raw"])

    def kv_beam_reorder(self, num_beams: int, groups: int, base: Sequence[int], end: Sequence[int], parent: torch.Tensor):
        """for every group g: cache positions [base[g], end[g]) of row g * num_beams + j become those of row g * num_beams + parent[...]
        (local beam indices, int32 on the device), every layer, K and V, in place - the beam tail's reorder on its own."""
        parent = parent.to(self.device, torch.int32).contiguous()
        arr = lambda v: (C.c_int * groups)(*[int(x) for x in v])    # noqa: E731
        B.check(self.lib.vz_llm_kv_beam_reorder(self.h, int(num_beams), int(groups), arr(base), arr(end), B.ptr(parent), self._s()))

    def kv_cache(self) -> torch.Tensor:
        """a copy of the whole KV cache, bf16 [n_layers, 2 (K|V), max_batch, kv heads, max_ctx, head_dim] (tests)."""
        n = C.c_size_t(0)
        B.check(self.lib.vz_llm_kv_copy_out(self.h, None, 0, C.byref(n), self._s()))
        cfg = self.cfg
        out = torch.empty(cfg.n_layers, 2, self.max_batch, cfg.n_kv_heads // self.tp_size, self.max_ctx, cfg.head_dim,
                          dtype=torch.bfloat16, device=self.device)
        assert out.numel() * 2 == n.value
        B.check(self.lib.vz_llm_kv_copy_out(self.h, B.ptr(out), n.value, C.byref(n), self._s()))
        return out

    def check_async(self):
        """raise if a bounded device-side wait expired since the last check (outputs invalid): the stream-K fix-up of
        the 256^2 GEMM (its tile is NaN, never a stale sum)."""
        err = C.c_int(0)
        B.check(self.lib.vz_engine_async_error(self.h, C.byref(err)))
        if err.value:
            what = {B.VZ_ASYNC_STREAMK: "stream-K fix-up of the 256^2 GEMM (another launch shared its tickets?)",
                    B.VZ_ASYNC_PERSIST: "phase hand-off of the persistent decode-token kernel"}.get(err.value, f"code {err.value}")
            raise RuntimeError(f"vz_hip: a bounded device-side wait expired ({what}); outputs since the last check are invalid")

    def persist_mode(self) -> bool:
        """True if the last decode_steps ran every token as one resident grid (decode_persist.hip)."""
        m = C.c_int(0)
        B.check(self.lib.vz_test_persist_poke(self.h, -1, 0, C.byref(m), self._s()))
        return bool(m.value)

    def persist_poke(self, word: int, value: int):
        """TEST HOOK: preset arrival counter `word` (0..7; 8 = abort) of the persistent decode-token kernel for the next decode_steps."""
        B.check(self.lib.vz_test_persist_poke(self.h, int(word), int(value) & 0xFFFFFFFF, None, self._s()))

    def decode_mode(self):
        """(graph replayed?, RCCL collectives inside the graph?) of the last decode_steps call."""
        g, c = C.c_int(0), C.c_int(0)
        B.check(self.lib.vz_llm_decode_mode(self.h, C.byref(g), C.byref(c)))
        return bool(g.value), bool(c.value)

    def decode_info(self):
        """(context splits of the last decode_steps call = its context bucket, graphs captured since the engine was created)."""
        ns, cap = C.c_int(0), C.c_int(0)
        B.check(self.lib.vz_llm_decode_info(self.h, C.byref(ns), C.byref(cap)))
        return ns.value, cap.value

    def ws_info(self) -> Tuple[int, int]:
        """(bytes of the stage arena, the mark the last stage call's carving reached in it)."""
        arena, peak = C.c_size_t(0), C.c_size_t(0)
        B.check(self.lib.vz_engine_ws_info(self.h, C.byref(arena), C.byref(peak)))
        return arena.value, peak.value

    def stage_ws_bytes(self, stage: int, n: int, n2: int = 0, Lmax: int = 0, flags: int = 0) -> int:
        """What a stage call of these dimensions takes of the arena (binding.stage_ws_bytes on this engine's config; _dest lays the
        Q-Former's ca_kv weights out back to back, so Q-Former queries carry WS_QF_KV_CONTIG)."""
        if stage == B.STAGE_QFORMER:
            flags |= B.WS_QF_KV_CONTIG
        return B.stage_ws_bytes(self.c_cfg, stage, n, n2, Lmax, flags)

    # profiling hooks (bench.py roofline leg)
    def prof_enable(self, on: bool, klass: int = -1):
        B.check(self.lib.vz_prof_enable(self.h, int(on), klass))

    def prof_read(self) -> Tuple[int, float]:
        n, ms = C.c_long(), C.c_double()
        B.check(self.lib.vz_prof_read(self.h, C.byref(n), C.byref(ms)))
        return n.value, ms.value
