"""ctypes binding of libviszephyr_hip.so (include/viszephyr.h).

The product path has no CPU fallback: if the shared library is missing, or a call fails, this
module raises.  torch is used only for device memory and streams (tensor.data_ptr(),
torch.cuda.current_stream()).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libviszephyr_hip.so")

VZ_OK, VZ_ERR_ARG, VZ_ERR_HIP, VZ_ERR_STATE, VZ_ERR_UNSUPPORTED = 0, 1, 2, 3, 4
VZ_ASYNC_STREAMK = 2
VZ_ASYNC_PERSIST = 3
VZ_ASYNC_ONESHOT = 4
VZ_ASYNC_ATTN_O = 5
ABI_VERSION = 12
SCORE_REC, SCORE_WARPED, SCORE_RAW = 1, 2, 4          # vz_llm_decode_scores `what`
SPEC_CTL_WRITE, SPEC_CTL_HIST, SPEC_CTL_DONE, SPEC_CTL_DRAFTED, SPEC_CTL_STEPS, SPEC_CTL_IDS, SPEC_CTL_WORDS = 0, 1, 2, 3, 4, 8, 16
ACT_NONE, ACT_QUICK_GELU, ACT_GELU_ERF, ACT_SWIGLU = 0, 1, 2, 3
K_GEMM, K_GEMV, K_ATTN, K_ATTN_DEC, K_NORM, K_OTHER, K_FUSED, K_COMM = range(8)


class VzConfig(C.Structure):
    _fields_ = [
        ("hidden", C.c_int), ("inter", C.c_int), ("n_layers", C.c_int), ("n_heads", C.c_int),
        ("n_kv_heads", C.c_int), ("head_dim", C.c_int), ("vocab", C.c_int),
        ("rms_eps", C.c_float), ("rope_theta", C.c_float), ("sliding_window", C.c_int),
        ("clip_hidden", C.c_int), ("clip_inter", C.c_int), ("clip_layers", C.c_int), ("clip_heads", C.c_int),
        ("clip_image", C.c_int), ("clip_patch", C.c_int), ("clip_eps", C.c_float),
        ("qf_queries", C.c_int), ("qf_blocks", C.c_int), ("qf_heads", C.c_int), ("qf_kv_dim", C.c_int),
        ("qf_eps", C.c_float),
        ("fusion_groups", C.c_int), ("fusion_layers_per_group", C.c_int),
        ("max_batch", C.c_int), ("max_ctx", C.c_int), ("max_tiles", C.c_int), ("max_text", C.c_int),
        ("tp_size", C.c_int), ("tp_rank", C.c_int), ("clip_keep_cls", C.c_int), ("weight_fp8", C.c_int),
    ]


ROW_GREEDY, ROW_SAMPLE = 0, 1


class VzSampleParams(C.Structure):
    """vz_sample_params: how one row chooses its next token (48 bytes, the entry of the per-row table in device memory)"""
    _fields_ = [
        ("mode", C.c_int), ("temperature", C.c_float), ("top_k", C.c_int), ("top_p", C.c_float),
        ("seed", C.c_ulonglong), ("counter", C.c_int), ("reserved", C.c_int),
        ("min_p", C.c_float), ("typical_p", C.c_float), ("epsilon_cutoff", C.c_float), ("eta_cutoff", C.c_float),
    ]


class VzLogitsProcParams(C.Structure):
    """vz_logits_proc_params: the logits processors' parameters and id lists (the lists are host memory the caller keeps alive)"""
    _fields_ = [
        ("repetition_penalty", C.c_float), ("no_repeat_ngram", C.c_int), ("min_new_tokens", C.c_int),
        ("n_eos", C.c_int), ("n_suppress", C.c_int), ("n_seq", C.c_int),
        ("eos", C.POINTER(C.c_int)), ("suppress", C.POINTER(C.c_int)), ("seq", C.POINTER(C.c_int)),
    ]


class VzProcRow(C.Structure):
    """vz_proc_row: one row's logits processors (128 bytes, the entry of the per-row table in device memory; vz_hip.logits_proc.pack_row
    writes the same bytes)"""
    _fields_ = [
        ("repetition_penalty", C.c_float), ("no_repeat_ngram", C.c_int), ("min_new_tokens", C.c_int),
        ("n_eos", C.c_int), ("eos", C.c_int * 4), ("n_suppress", C.c_int), ("suppress", C.c_int * 16),
        ("n_seq", C.c_int), ("active", C.c_int), ("reserved", C.c_int * 5),
    ]


# every symbol include/viszephyr.h declares: (restype, argtypes)
_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_long, C.c_float
SYMBOLS = {
    "vz_last_error": (C.c_char_p, []),
    "vz_abi_version": (_I, []),
    "vz_target_arch": (C.c_char_p, []),
    "vz_op_linear": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _P]),
    "vz_op_tile_weights": (_I, [_P, _I, _I, _I, _P, _P]),
    "vz_op_linear_tiled": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _P, _F, _P]),
    "vz_op_tile_weights_fp8": (_I, [_P, _I, _I, _I, _P, _P]),
    "vz_op_linear_tiled_fp8": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _P]),
    "vz_engine_prefill_fp8": (_I, [_P, _I]),
    "vz_op_rmsnorm_quant_fp8": (_I, [_P, _I, _P, _F, _P, _I, _P, _I, _I, _P]),
    "vz_op_quant_rows_fp8": (_I, [_P, _I, _P, _I, _P, _I, _I, _P]),
    "vz_op_linear_fp8_mfma": (_I, [_P, _I, _P, _P, _I, _P, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _P]),
    "vz_op_linear_impl": (_I, [_I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _P]),
    "vz_op_linear_route": (_I, [_I, _I, _I, _I, _I, _I, _I, C.c_uint, _I, _P, _P]),
    "vz_op_causal_lm_loss": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
    "vz_op_layernorm": (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _F, _P]),
    "vz_op_rmsnorm": (_I, [_P, _I, _P, _I, _P, _I, _I, _F, _P]),
    "vz_op_attention": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I] + [_L] * 12 + [_F, _I, _I, _I, _P, _P]),
    "vz_op_transpose": (_I, [_P, _L, _P, _L, _I, _I, _P]),
    "vz_op_colsum": (_I, [_P, _I, _L, _I, _P, _L, _P, _P]),
    "vz_op_colsum_groups": (_I, [_L]),
    "vz_op_attention_append": (_I, [_P] * 6 + [_I] * 7 + [_L] * 6 + [_F, _I, _I, _P, _L, _P]),
    "vz_op_attention_append_ws_floats": (_L, [_I] * 5),
    "vz_op_attention_shared": (_I, [_P] * 6 + [_I] * 7 + [_F, _I, _I, _P, _L, _P]),
    "vz_op_attention_shared_ws_floats": (_L, [_I] * 5),
    "vz_op_attention_bwd": (_I, [_P] * 7 + [_I] * 7 + [_F, _I, _I, _P, _P, _L, _P]),
    "vz_op_attention_split": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I] + [_L] * 12 + [_F, _I, _I, _I, _P, _P, _L, _P]),
    "vz_op_argmax": (_I, [_P, _I, _I, _P, _P]),
    "vz_op_rope_kv": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "vz_op_attention_decode": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _P, _P]),
    "vz_op_attention_decode_fused": (_I, [_P] * 10 + [_I] * 7 + [_F, _P]),
    "vz_op_attention_decode_kv8": (_I, [_P] * 14 + [_I] * 7 + [_F, _P]),
    "vz_op_kv8_mirror_rows": (_I, [_P] * 6 + [_I, _P, _P, _I, _I, _I, _P]),
    "vz_engine_kv_fp8": (_I, [_P, _I]),
    "vz_llm_kv8_copy_out": (_I, [_P, _P, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), _P]),
    "vz_engine_create": (_I, [C.POINTER(VzConfig), C.POINTER(_P)]),
    "vz_engine_destroy": (_I, [_P]),
    "vz_engine_ws_info": (_I, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "vz_op_stage_ws_bytes": (_L, [C.POINTER(VzConfig), _I, _I, _I, _I, C.c_uint]),
    "vz_engine_set_weight": (_I, [_P, C.c_char_p, _P, _I, _L]),
    "vz_engine_finalize": (_I, [_P]),
    "vz_engine_set_rope": (_I, [_P, _P, _P, _I]),
    "vz_comm_unique_id": (_I, [C.c_char_p]),
    "vz_comm_init": (_I, [_P, C.c_char_p]),
    "vz_clip_fused_features": (_I, [_P, _P, _I, _P, _P, _P]),
    "vz_qformer": (_I, [_P, _P, _I, _P, _I, _I, C.POINTER(C.c_int), _P, _P]),
    "vz_embed_splice": (_I, [_P, _P, _P, _I, _P, _P, _P]),
    "vz_llm_prefill": (_I, [_P, _P, _I, _I, C.POINTER(C.c_int), _P, _P, _P, _P]),
    "vz_llm_prefill_rows": (_I, [_P, _I, _P, _I, _I, C.POINTER(C.c_int), _P, _P, _P, _P]),
    "vz_llm_prefill_append": (_I, [_P, _I, _P, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int), _P, _P, _P, _P]),
    "vz_llm_decode_set_row": (_I, [_P, _I, _I, _I, _I, _P]),
    "vz_llm_kv_move_rows": (_I, [_P, _I, _P, _P, _P, _P]),
    "vz_llm_decode_begin": (_I, [_P, _I, _P, C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    "vz_llm_decode_steps": (_I, [_P, _I, _P, _P, _P]),
    "vz_llm_decode_mode": (_I, [_P, _P, _P]),
    "vz_llm_decode_info": (_I, [_P, _P, _P]),
    "vz_test_persist_poke": (_I, [_P, _I, C.c_uint, _P, _P]),
    "vz_prof_persist_stamps": (_I, [_P, _P, _I]),
    "vz_op_oneshot_area_bytes": (C.c_size_t, [_I, _I]),
    "vz_op_allreduce_oneshot": (_I, [_P, _I, _I, _I, _P, _P, _I, _P, _P, _P]),
    "vz_test_allreduce_oneshot_all": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _P]),
    "vz_comm_oneshot_local": (_I, [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "vz_comm_oneshot_attach": (_I, [_P, _P, _I]),
    "vz_engine_async_error": (_I, [_P, _P]),
    "vz_tune_set": (_I, [_I, _I]),
    "vz_tune_get": (_I, [_I, C.POINTER(_I)]),
    "vz_tune_info": (_I, [_I, C.POINTER(_I), C.POINTER(C.c_char_p), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "vz_engine_resize_vocab": (_I, [_P, _I]),
    "vz_op_resample_u8": (_I, [_P, _I, _I, _P, _P, _I, _I, _P, _P, _I, _P, _P, _I, _P]),
    "vz_op_anyres_tiles": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "vz_op_linear_rmsnorm": (_I, [_P, _I, _P, _F, _P, _I, _P, _I, _I, _I, _I, _P, _I, _I, _I, _P]),
    "vz_op_linear_fp8": (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _P, _F, _P]),
    "vz_tp_all_gather": (_I, [_P, _P, _P, C.c_size_t, _P]),
    "vz_prof_enable": (_I, [_P, _I, _I]),
    "vz_prof_read": (_I, [_P, C.POINTER(C.c_long), C.POINTER(C.c_double)]),
    "vz_prof_attn_stamps": (_I, [C.POINTER(C.c_longlong)]),
    "vz_prof_gemm_stamps": (_I, [C.POINTER(C.c_longlong), _I, C.POINTER(_I)]),
    "vz_op_async_error": (_I, [_P, C.POINTER(_I)]),
    "vz_test_corrupt_streamk": (_I, [_P, _I, _I, _I]),
    "vz_engine_unset_weight": (_I, [_P, C.c_char_p]),
    "vz_llm_decode_sampling": (_I, [_P, _P]),
    "vz_llm_decode_ring": (_I, [_P, _P, _I, _I]),
    "vz_train_create": (_I, [_P, C.POINTER(_P), _P]),
    "vz_train_destroy": (_I, [_P]),
    "vz_train_set_master": (_I, [_P, C.c_char_p, _P, _L, _P]),
    "vz_train_param_count": (_I, [_P]),
    "vz_train_param_info": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(_L), C.POINTER(_L), C.POINTER(_I)]),
    "vz_train_arenas": (_I, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_L)]),
    "vz_train_stage1_accumulate": (_I, [_P, _P, _I, _P, _I, _I, C.POINTER(_I), _P, _P, _P, _I, _I, C.POINTER(_I), _P, _P, _F, _P]),
    "vz_train_loss_sum": (_I, [_P, C.POINTER(C.c_double), _P]),
    "vz_train_zero_grad": (_I, [_P, _P]),
    "vz_train_comm_init": (_I, [_P, C.c_char_p, _I, _I]),
    "vz_train_allreduce": (_I, [_P, _P]),
    "vz_train_adamw_step": (_I, [_P, _F, _F, _F, _F, _F, _P]),
    "vz_train_ws_info": (_I, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "vz_train_lora_enable": (_I, [_P, _I, _F, _F, C.c_ulonglong, _P]),
    "vz_train_lora_set_counter": (_I, [_P, _I, _L, _L]),
    "vz_op_lora_dropout": (_I, [_P, _I, _P, _I, _I, _I, _I, _L, _L, _I, _I, C.c_ulonglong, _F, _F, _P]),
    "vz_op_vip_point": (_I, [_P, _I, _I, _I, _I, _I, _I, C.c_uint, _P]),
    "vz_op_sample": (_I, [_P, _I, _I, _P, _P, _P]),
    "vz_llm_decode_sampling_rows": (_I, [_P, _I, _I, _P]),
    "vz_llm_decode_set_row_sampling": (_I, [_P, _I, _P, _P]),
    "vz_op_sample_rows": (_I, [_P, _I, _I, _P, _P, _P]),
    "vz_llm_decode_scores": (_I, [_P, C.c_uint, _P, _P, _P, _I, _P]),
    "vz_op_token_scores": (_I, [_P, _I, _I, _P, _P, _P, _P, _P]),
    "vz_llm_decode_stop": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    "vz_llm_decode_stop_rows": (_I, [_P, _I, _I, _P, _P]),
    "vz_llm_decode_stop_seed": (_I, [_P, _I, C.POINTER(C.c_int), _I, _P]),
    "vz_llm_decode_logits_proc_seed": (_I, [_P, _I, C.POINTER(C.c_int), _I, _P]),
    "vz_llm_decode_stop_read": (_I, [_P, _I, _I, _P, _P]),
    "vz_op_stop_match": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    "vz_llm_decode_logits_proc": (_I, [_P, _P, _P]),
    "vz_op_logits_process": (_I, [_P, _I, _I, _P, _I, _P, _P, _P]),
    "vz_llm_decode_logits_proc_rows": (_I, [_P, _I, _P]),
    "vz_llm_decode_set_row_logits_proc": (_I, [_P, _I, _P, _P, _I, _P]),
    "vz_op_logits_process_rows": (_I, [_P, _I, _I, _P, _I, _P, _P, _P, _P, _P]),
    "vz_llm_decode_stop_row_seqs": (_I, [_P, _I, _P]),
    "vz_llm_decode_stop_set_row_seqs": (_I, [_P, _I, _P, _I, _P]),
    "vz_llm_decode_guidance": (_I, [_P, _I, _F, _I, _P]),
    "vz_llm_decode_share": (_I, [_P, _I, _P, _I, _P]),
    "vz_op_cfg_combine": (_I, [_P, _P, _I, _I, _F, _P]),
    "vz_llm_decode_beam": (_I, [_P, _I, _I, _I, _P, _I, _P, _P, _P, _I, _P]),
    "vz_op_beam_select": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P]),
    "vz_llm_kv_beam_reorder": (_I, [_P, _I, _I, _P, _P, _P, _P]),
    "vz_op_beam_logprob_rows": (_I, [_P, _I, _I, _P, _P]),
    "vz_op_beam_select_rows": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _P]),
    "vz_op_hist_beam_reorder": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "vz_llm_decode_beam_rows": (_I, [_P, _P, _P, _I]),
    "vz_llm_kv_copy_out": (_I, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t), _P]),
    "vz_llm_decode_spec": (_I, [_P, _I, _I, _I, _P, _I, _I, _P, _I, _P, _I, _P, _P, _I, _I, _P, _I, _P]),
    "vz_op_spec_draft": (_I, [_P, _I, _I, _I, _P, _I, _P, _P, _P]),
    "vz_op_spec_accept": (_I, [_P, _I, _I, _P, _P, _P, _I, _P, _I, _P, _I, _P, _I, _I, _P]),
    "vz_llm_decode_spec_sampling": (_I, [_P, _P]),
    "vz_op_spec_accept_sampled": (_I, [_P, _I, _I, _P, _P, _P, _P, _I, _P, _I, _P, _I, _P, _I, _I, _P]),
    "vz_op_spec_part_floats": (_L, [_I, _I, _I]),
    "vz_op_attention_verify": (_I, [_P] * 11 + [_I] * 8 + [_F, _P]),
    "vz_op_transpose_batched": (_I, [_P, _L, _L, _L, _P, _L, _L, _L, _I, _I, _I, _I, _I, _P]),
    "vz_op_softmax_fwd": (_I, [_P, _I, _P, _I, _L, _I, _I, _I, _F, _I, _I, _P, _P]),
    "vz_op_softmax_bwd": (_I, [_P, _I, _P, _I, _P, _I, _L, _I, _F, _P]),
    "vz_op_rmsnorm_bwd": (_I, [_P, _P, _P, _P, _P, _L, _I, _F, _P]),
    "vz_op_layernorm_bwd_scratch_floats": (_L, [_L, _I]),
    "vz_op_layernorm_bwd": (_I, [_P, _P, _P, _P, _P, _P, _L, _P, _P, _L, _I, _F, _P]),
    "vz_op_gelu_fwd": (_I, [_P, _P, _L, _P]),
    "vz_op_gelu_bwd": (_I, [_P, _P, _P, _L, _P]),
    "vz_op_swiglu_fwd": (_I, [_P, _P, _L, _I, _P]),
    "vz_op_swiglu_bwd": (_I, [_P, _P, _P, _L, _I, _P]),
    "vz_op_rope_bwd_assemble": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "vz_op_cross_entropy": (_I, [_P, _I, _P, _L, _I, _F, _P, _P, _I, _P]),
    "vz_op_gather_rows_idx": (_I, [_P, _P, _P, _L, _I, _P]),
    "vz_op_segment_sum_rows": (_I, [_P, _P, _I, _I, _P, _I, _I, _P]),
    "vz_op_acc_rows_f32": (_I, [_P, _P, _I, _L, _I, _I, _P]),
    "vz_op_adamw": (_I, [_P, _P, _P, _P, _P, _I, _L, _F, _F, _F, _F, _F, _I, _P]),
}

_lib: Optional[C.CDLL] = None


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """dlopen the HIP library and type every entry point.  Raises if it is missing: there is no
    eager/CPU fallback for the product path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: build it with `make -C vision-zephyr_amd/csrc` (or __graft_entry__.build()). "
            "The Vision-Zephyr MI355X path has no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)      # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def lib() -> C.CDLL:
    return load_library()


class VzError(RuntimeError):
    pass


def check(rc: int):
    if rc == VZ_OK:
        return
    msg = lib().vz_last_error().decode(errors="replace")
    if rc == VZ_ERR_ARG:
        raise ValueError(msg)
    if rc == VZ_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise VzError(f"libviszephyr_hip error {rc}: {msg}")


# ---- the tune knobs (csrc/tune.h): names, a scope that restores what it found ----
_knobs: Optional[dict] = None


def knobs() -> dict:
    """{name: (number, default, lo, hi)} of every knob, in table order: read once from vz_tune_info, never copied here"""
    global _knobs
    if _knobs is None:
        table, i = {}, 0
        k, name, d, lo, hi = C.c_int(), C.c_char_p(), C.c_int(), C.c_int(), C.c_int()
        while lib().vz_tune_info(i, C.byref(k), C.byref(name), C.byref(d), C.byref(lo), C.byref(hi)) == VZ_OK:
            table[name.value.decode()] = (k.value, d.value, lo.value, hi.value)
            i += 1
        _knobs = table
    return _knobs


def _knob_number(knob) -> int:
    """a knob's number from its name, its number or either as a string; an unknown NAME raises KeyError (an unknown number is the library's to refuse)"""
    if isinstance(knob, str) and not knob.lstrip("-").isdigit():
        if knob not in knobs():
            raise KeyError(f"unknown tune knob {knob!r}; known: {', '.join(knobs())}")
        return knobs()[knob][0]
    return int(knob)


def tune(knob, value):
    """vz_tune_set by name or number, for as long as the process lives (a tool's own setting); tests use tuned()"""
    check(lib().vz_tune_set(_knob_number(knob), int(value)))


def tune_get(knob) -> int:
    v = C.c_int()
    check(lib().vz_tune_get(_knob_number(knob), C.byref(v)))
    return v.value


@contextlib.contextmanager
def tuned(*pairs, **values):
    """Scope with knobs set: tuned(splitk_mid=0, gemm256_streamk=0), or tuned((26, 0), (4, 0)) where the knob is a number or a variable.
    On entry each knob's current value is read, then the new one set; on exit - exception or not - what was read is set again, in reverse
    order.  Scopes nest."""
    found = []
    try:
        for knob, value in list(pairs) + list(values.items()):
            number = _knob_number(knob)
            was = tune_get(number)
            tune(number, value)
            found.append((number, was))
        yield
    finally:
        for number, was in reversed(found):
            tune(number, was)


def _knob_args(settings):
    """[(knob, value)] of a tool's --knob / VZ_TUNE settings: a list of "k=v" (k a name or a number), or one string of them joined by commas"""
    if isinstance(settings, str):
        settings = settings.split(",")
    return [tuple(kv.split("=", 1)) for kv in settings if kv]


def tuned_from_args(settings):
    """tuned() over "k=v" settings"""
    return tuned(*_knob_args(settings))


def tune_from_args(settings):
    """tune() over "k=v" settings: a tool's knobs for its whole life; returns {number: value} of what it set"""
    done = {}
    for knob, value in _knob_args(settings):
        tune(knob, value)
        done[_knob_number(knob)] = int(value)
    return done


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("libviszephyr_hip operates on device tensors only (no CPU fallback)")


# ------------------------------------------------------------------------------------------------
# operator wrappers (used by tests and by nothing else in the product: the engine calls the same
# launchers natively)
# ------------------------------------------------------------------------------------------------
def linear(x: torch.Tensor, w: torch.Tensor, bias=None, residual=None, act: int = ACT_NONE, out_fp32=False,
           impl: Optional[int] = None) -> torch.Tensor:
    """epi(x[M,K] @ w[N,K]^T); bf16 in, bf16 (or fp32) out."""
    _need_cuda(x, w, bias, residual)
    assert x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.dim() == 2 and w.dim() == 2
    assert x.stride(1) == 1 and w.stride(1) == 1
    M, K = x.shape
    N = w.shape[0]
    n_out = N // 2 if act == ACT_SWIGLU else N
    out = torch.empty(M, n_out, dtype=torch.float32 if out_fp32 else torch.bfloat16, device=x.device)
    if bias is not None:
        assert bias.dtype == torch.float32
    if residual is not None:
        assert residual.dtype == torch.bfloat16 and residual.stride(1) == 1
    args = (ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(out), out.stride(0), M, N, K, ptr(bias), ptr(residual),
            0 if residual is None else residual.stride(0), act, int(out_fp32), stream_ptr(x.device))
    if impl is None:
        check(lib().vz_op_linear(*args))
    else:
        check(lib().vz_op_linear_impl(impl, *args))
    return out


def tile_weights(w: torch.Tensor) -> torch.Tensor:
    """fragment-tiled copy of a dense bf16 [N, K] weight for the 2..64-row MFMA weight stream (layout: include/viszephyr.h)."""
    _need_cuda(w)
    assert w.dtype == torch.bfloat16 and w.dim() == 2 and w.stride(1) == 1
    wt = torch.empty(w.numel(), dtype=torch.bfloat16, device=w.device)
    check(lib().vz_op_tile_weights(ptr(w), w.shape[0], w.shape[1], w.stride(0), ptr(wt), stream_ptr(w.device)))
    return wt


def oneshot_area(n_ranks: int, max_elems: int, device) -> torch.Tensor:
    """zero-filled receive area of ONE rank of the one-shot all-reduce (comm_oneshot.hip)"""
    return torch.zeros(int(lib().vz_op_oneshot_area_bytes(n_ranks, max_elems)), dtype=torch.uint8, device=device)


def oneshot_seq(device) -> torch.Tensor:
    """the two device words {sequence number = 1, ticket = 0} of one rank"""
    return torch.tensor([1, 0], dtype=torch.int32, device=device)


def allreduce_oneshot(areas, rank: int, max_elems: int, x: torch.Tensor, out: torch.Tensor, seq: torch.Tensor, err: torch.Tensor, stream=None):
    """rank `rank`'s launch of one all-reduce over len(areas) ranks (areas[q] = rank q's receive area); on torch's current stream"""
    _need_cuda(x, out, seq, err, *areas)
    arr = (C.c_void_p * len(areas))(*[a.data_ptr() for a in areas])
    check(lib().vz_op_allreduce_oneshot(arr, rank, len(areas), max_elems, ptr(x), ptr(out), x.numel(), ptr(seq), ptr(err),
                                        stream_ptr(x.device) if stream is None else stream))


def allreduce_oneshot_all(areas, max_elems: int, xs, outs, seqs, err: torch.Tensor):
    """TEST FORM: every rank of one all-reduce as a slice of ONE launch (one process, one GPU)"""
    n = len(areas)
    _need_cuda(err, *areas, *xs, *outs, *seqs)
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])      # noqa: E731
    check(lib().vz_test_allreduce_oneshot_all(arr(areas), n, max_elems, arr(xs), arr(outs), xs[0].numel(), arr(seqs), ptr(err), stream_ptr(err.device)))


def tile_weights_fp8(w8: torch.Tensor) -> torch.Tensor:
    """fragment-tiled copy of dense e4m3 rows (uint8 [N, K]) for the 17..64-row W8A16 stream of gemm_wide.hip."""
    _need_cuda(w8)
    assert w8.dtype == torch.uint8 and w8.dim() == 2 and w8.stride(1) == 1
    wt = torch.empty(w8.numel(), dtype=torch.uint8, device=w8.device)
    check(lib().vz_op_tile_weights_fp8(ptr(w8), w8.shape[0], w8.shape[1], w8.stride(0), ptr(wt), stream_ptr(w8.device)))
    return wt


def linear_tiled_fp8(x: torch.Tensor, w8t: torch.Tensor, wscale: torch.Tensor, N: int, bias=None, residual=None, act: int = ACT_NONE,
                     out_fp32=False) -> torch.Tensor:
    """epi(x @ (wscale[:, None] * e4m3(W8))^T) for 17 <= M <= 64 rows on the tiled e4m3 copy (gemm_wide.hip, W8A16)."""
    _need_cuda(x, w8t, wscale, bias, residual)
    M, K = x.shape
    n_out = N // 2 if act == ACT_SWIGLU else N
    out = torch.empty(M, n_out, dtype=torch.float32 if out_fp32 else torch.bfloat16, device=x.device)
    check(lib().vz_op_linear_tiled_fp8(ptr(x), x.stride(0), ptr(w8t), ptr(wscale), ptr(out), out.stride(0), M, N, K, ptr(bias),
                                       ptr(residual), 0 if residual is None else residual.stride(0), act, int(out_fp32), stream_ptr(x.device)))
    return out


def linear_tiled(x: torch.Tensor, w: torch.Tensor, wt: torch.Tensor, bias=None, residual=None, act: int = ACT_NONE, out_fp32=False,
                 norm_w=None, norm_eps: float = 0.0) -> torch.Tensor:
    """the MFMA weight stream (2 <= M <= 64) reading the tiled copy `wt` of w; bit-identical to linear(impl=3)."""
    _need_cuda(x, w, wt, bias, residual, norm_w)
    M, K = x.shape
    N = w.shape[0]
    n_out = N // 2 if act == ACT_SWIGLU else N
    out = torch.empty(M, n_out, dtype=torch.float32 if out_fp32 else torch.bfloat16, device=x.device)
    check(lib().vz_op_linear_tiled(ptr(x), x.stride(0), ptr(w), ptr(wt), w.stride(0), ptr(out), out.stride(0), M, N, K, ptr(bias),
                                   ptr(residual), 0 if residual is None else residual.stride(0), act, int(out_fp32), ptr(norm_w),
                                   float(norm_eps), stream_ptr(x.device)))
    return out


def linear_rmsnorm(x: torch.Tensor, norm_w: torch.Tensor, eps: float, w: torch.Tensor, residual=None, act: int = ACT_NONE,
                   out_fp32=False) -> torch.Tensor:
    """epi(rmsnorm(x) @ w^T) with the norm fused into the weight-stream kernel's staging; M <= 16."""
    _need_cuda(x, w, norm_w, residual)
    assert x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and norm_w.dtype == torch.float32
    M, K = x.shape
    N = w.shape[0]
    n_out = N // 2 if act == ACT_SWIGLU else N
    out = torch.empty(M, n_out, dtype=torch.float32 if out_fp32 else torch.bfloat16, device=x.device)
    check(lib().vz_op_linear_rmsnorm(ptr(x), x.stride(0), ptr(norm_w), float(eps), ptr(w), w.stride(0), ptr(out), out.stride(0), M, N, K,
                                     ptr(residual), 0 if residual is None else residual.stride(0), act, int(out_fp32), stream_ptr(x.device)))
    return out


def linear_fp8(x: torch.Tensor, w8: torch.Tensor, scale: torch.Tensor, bias=None, residual=None, act: int = ACT_NONE,
               out_fp32=False, norm_w=None, norm_eps: float = 0.0) -> torch.Tensor:
    """W8A16 weight stream: epi(x[M<=64,K] @ (scale[:,None] * e4m3(w8))[N,K]^T); x bf16, w8 uint8 (e4m3 bytes), scale fp32 [N]."""
    _need_cuda(x, w8, scale, bias, residual, norm_w)
    assert x.dtype == torch.bfloat16 and w8.dtype == torch.uint8 and scale.dtype == torch.float32
    assert x.dim() == 2 and w8.dim() == 2 and x.stride(1) == 1 and w8.stride(1) == 1
    M, K = x.shape
    N = w8.shape[0]
    n_out = N // 2 if act == ACT_SWIGLU else N
    out = torch.empty(M, n_out, dtype=torch.float32 if out_fp32 else torch.bfloat16, device=x.device)
    check(lib().vz_op_linear_fp8(ptr(x), x.stride(0), ptr(w8), w8.stride(0), ptr(scale), ptr(out), out.stride(0), M, N, K,
                                 ptr(bias), ptr(residual), 0 if residual is None else residual.stride(0), act, int(out_fp32),
                                 ptr(norm_w), float(norm_eps), stream_ptr(x.device)))
    return out


LIN_ROUTES = ("GEMV", "SKINNY", "SKINNY_PERSIST", "SKINNY_WIDE", "WIDE_BF16", "WIDE_E4M3", "TILE128", "TILE256")
ROUTE_WT, ROUTE_W8, ROUTE_W8T, ROUTE_NORM, ROUTE_BIAS, ROUTE_RESIDUAL, ROUTE_DECODE = 1, 2, 4, 8, 16, 32, 64
LINEAR_ENGINE, LINEAR_OP, LINEAR_RMSNORM, LINEAR_TILED, LINEAR_TILED_FP8, LINEAR_IMPL = 0, 1, 2, 3, 4, 8


def linear_route(M: int, N: int, K: int, lda: Optional[int] = None, ldw: Optional[int] = None, act: int = ACT_NONE, out_fp32=False,
                 flags: int = 0, entry: int = LINEAR_ENGINE):
    """(route name | "NONE", pre_norm, splitk_hint) of a linear of this shape under the current knobs; needs no GPU (vz_op_linear_route)."""
    pre, sk = C.c_int(0), C.c_int(0)
    r = lib().vz_op_linear_route(M, N, K, K if lda is None else lda, K if ldw is None else ldw, act, int(out_fp32), flags, entry,
                                 C.byref(pre), C.byref(sk))
    return (LIN_ROUTES[r] if 0 <= r < len(LIN_ROUTES) else "NONE"), bool(pre.value), sk.value


STAGE_CLIP, STAGE_QFORMER, STAGE_PREFILL, STAGE_DECODE, STAGE_APPEND = range(5)
WS_CALLER_HIDDEN, WS_QF_KV_CONTIG, WS_SPEC_TAIL = 1, 2, 4


def stage_ws_bytes(cfg: VzConfig, stage: int, n: int, n2: int = 0, Lmax: int = 0, flags: int = 0) -> int:
    """Bytes the stage's carving takes for a call of these dimensions on an engine of `cfg`, -1 where the config or the shape would be
    refused; needs no GPU (vz_op_stage_ws_bytes)."""
    return lib().vz_op_stage_ws_bytes(C.byref(cfg), stage, n, n2, Lmax, flags)


def causal_lm_loss(logits: torch.Tensor, labels: torch.Tensor):
    """(loss, valid target count) of fp32 logits [B, S, V] against labels [B, S] (-100 ignored), shifted by one, mean over valid targets."""
    _need_cuda(logits)
    assert logits.dtype == torch.float32 and logits.dim() == 3 and logits.is_contiguous()
    Bn, S, V = logits.shape
    lab = labels.to(logits.device, torch.int32).contiguous()
    assert tuple(lab.shape) == (Bn, S)
    rows = torch.empty(Bn * S, dtype=torch.float32, device=logits.device)
    out = torch.empty(2, dtype=torch.float32, device=logits.device)
    check(lib().vz_op_causal_lm_loss(ptr(logits), Bn, S, V, ptr(lab), ptr(rows), ptr(out), stream_ptr(logits.device)))
    return out[0], out[1]


def quant_rows_fp8(x: torch.Tensor):
    """bf16 [M, K] -> (e4m3 bytes uint8 [M, K], fp32 [M] power-of-two row scales): the device twin of vz_hip.quant.quantize_rows."""
    _need_cuda(x)
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.stride(1) == 1
    M, K = x.shape
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    sc = torch.empty(M, dtype=torch.float32, device=x.device)
    check(lib().vz_op_quant_rows_fp8(ptr(x), x.stride(0), ptr(q), q.stride(0), ptr(sc), M, K, stream_ptr(x.device)))
    return q, sc


def rmsnorm_quant_fp8(x: torch.Tensor, w: torch.Tensor, eps: float):
    """rmsnorm(x) rounded to bf16, then quant_rows_fp8 - in one launch; returns (e4m3 bytes [M, K], fp32 [M] scales)."""
    _need_cuda(x, w)
    assert x.dtype == torch.bfloat16 and w.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    M, K = x.shape
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    sc = torch.empty(M, dtype=torch.float32, device=x.device)
    check(lib().vz_op_rmsnorm_quant_fp8(ptr(x), x.stride(0), ptr(w), float(eps), ptr(q), q.stride(0), ptr(sc), M, K, stream_ptr(x.device)))
    return q, sc


def linear_fp8_mfma(x8: torch.Tensor, xs: torch.Tensor, w8: torch.Tensor, ws: torch.Tensor, bias=None, residual=None, act: int = ACT_NONE,
                    out_fp32=False) -> torch.Tensor:
    """epi((x8 . w8^T) * xs[:, None] * ws[None, :]) on the fp8 MFMA; x8 / w8 uint8 e4m3 bytes, xs / ws fp32 row scales."""
    _need_cuda(x8, xs, w8, ws, bias, residual)
    assert x8.dtype == torch.uint8 and w8.dtype == torch.uint8 and xs.dtype == torch.float32 and ws.dtype == torch.float32
    M, K = x8.shape
    N = w8.shape[0]
    n_out = N // 2 if act == ACT_SWIGLU else N
    out = torch.empty(M, n_out, dtype=torch.float32 if out_fp32 else torch.bfloat16, device=x8.device)
    check(lib().vz_op_linear_fp8_mfma(ptr(x8), x8.stride(0), ptr(xs), ptr(w8), w8.stride(0), ptr(ws), ptr(out), out.stride(0), M, N, K,
                                      ptr(bias), ptr(residual), 0 if residual is None else residual.stride(0), act, int(out_fp32),
                                      stream_ptr(x8.device)))
    return out


def layernorm(x, w, b, eps):
    _need_cuda(x, w, b)
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.stride(1) == 1
    y = torch.empty_like(x)
    check(lib().vz_op_layernorm(ptr(x), x.stride(0), ptr(y), y.stride(0), ptr(w), ptr(b), x.shape[0], x.shape[1],
                                eps, stream_ptr(x.device)))
    return y


def rmsnorm(x, w, eps):
    _need_cuda(x, w)
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.stride(1) == 1
    y = torch.empty_like(x)
    check(lib().vz_op_rmsnorm(ptr(x), x.stride(0), ptr(y), y.stride(0), ptr(w), x.shape[0], x.shape[1], eps,
                              stream_ptr(x.device)))
    return y


def transpose(x):
    """bf16 [R, C] (unit column stride) -> contiguous [C, R] (vz_op_transpose)"""
    _need_cuda(x)
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.stride(1) == 1
    y = torch.empty(x.shape[1], x.shape[0], dtype=torch.bfloat16, device=x.device)
    check(lib().vz_op_transpose(ptr(x), x.stride(0), ptr(y), y.stride(0), x.shape[0], x.shape[1], stream_ptr(x.device)))
    return y


def colsum(y, out):
    """out[c] += sum_r y[r][c]: y bf16 [rows, cols] (unit column stride), out fp32 [cols] (vz_op_colsum, the bias-gradient reduction)"""
    _need_cuda(y, out)
    assert y.dtype == torch.bfloat16 and y.stride(1) == 1 and out.dtype == torch.float32 and out.is_contiguous()
    rows, cols = y.shape
    part = torch.empty(lib().vz_op_colsum_groups(rows) * cols, dtype=torch.float32, device=y.device)
    check(lib().vz_op_colsum(ptr(y), y.stride(0), rows, cols, ptr(part), part.numel(), ptr(out), stream_ptr(y.device)))
    return out


# ---- the kernels of the training step (train.hip) one by one: the wrappers type-check, allocate scratch and pass the caller's tensors through
# as they are (outputs are the caller's, so a test can pre-fill them); eligibility is the launchers' business, a refusal raises ValueError ----
def _bf(*ts):
    for t in ts:
        assert t is None or t.dtype == torch.bfloat16, "bf16 tensor expected"


def _f32(*ts):
    for t in ts:
        assert t is None or t.dtype == torch.float32, "fp32 tensor expected"


def _i32(*ts):
    for t in ts:
        assert t is None or t.dtype == torch.int32, "int32 tensor expected"


def transpose_batched(src, src_rs, src_so, src_si, dst, dst_rs, dst_so, dst_si, R, C, n_outer, n_inner, col0):
    """dst[o][i][c][col0 + r] = src[o][i][r][c] (vz_op_transpose_batched): src / dst are the bf16 base tensors, strides in elements"""
    _need_cuda(src, dst)
    _bf(src, dst)
    check(lib().vz_op_transpose_batched(ptr(src), src_rs, src_so, src_si, ptr(dst), dst_rs, dst_so, dst_si, R, C, n_outer, n_inner, col0,
                                        stream_ptr(src.device)))


def softmax_fwd(S, P, rows, H, Sq, Sk, scale, causal=False, window=0, kv_len=None):
    """P bf16 [rows, ldp] <- masked softmax of the fp32 scores S [rows, lds] (vz_op_softmax_fwd)"""
    _need_cuda(S, P, kv_len)
    _f32(S); _bf(P); _i32(kv_len)
    check(lib().vz_op_softmax_fwd(ptr(S), S.stride(0), ptr(P), P.stride(0), rows, H, Sq, Sk, float(scale), int(causal), int(window), ptr(kv_len),
                                  stream_ptr(S.device)))


def softmax_bwd(P, dP, dS, rows, Sk, scale):
    """dS bf16 [rows, ldds] <- P o (dP - sum P dP) scale (vz_op_softmax_bwd); P bf16 [rows, ldp], dP fp32 [rows, lddp]"""
    _need_cuda(P, dP, dS)
    _bf(P, dS); _f32(dP)
    check(lib().vz_op_softmax_bwd(ptr(P), P.stride(0), ptr(dP), dP.stride(0), ptr(dS), dS.stride(0), rows, Sk, float(scale), stream_ptr(P.device)))


def rmsnorm_bwd(x, w, dy, dres, dx, rows, cols, eps):
    """dx <- RMSNorm backward of contiguous bf16 [rows, cols] (vz_op_rmsnorm_bwd); w fp32 [cols]; dres optional"""
    _need_cuda(x, w, dy, dres, dx)
    _bf(x, dy, dres, dx); _f32(w)
    check(lib().vz_op_rmsnorm_bwd(ptr(x), ptr(w), ptr(dy), ptr(dres), ptr(dx), rows, cols, float(eps), stream_ptr(x.device)))


def layernorm_bwd(x, w, dy, dres, dx, dw, db, rows, cols, eps):
    """dx (or None) <- LayerNorm backward, dw / db fp32 [cols] += the parameter gradients (vz_op_layernorm_bwd); returns the fp32 [rows, 2]
    (mean, rstd) statistics the kernels left at the end of their scratch"""
    _need_cuda(x, w, dy, dres, dx, dw, db)
    _bf(x, dy, dres, dx); _f32(w, dw, db)
    part = torch.empty(max(int(lib().vz_op_layernorm_bwd_scratch_floats(rows, cols)), 1), dtype=torch.float32, device=x.device)
    check(lib().vz_op_layernorm_bwd(ptr(x), ptr(w), ptr(dy), ptr(dres), ptr(dx), ptr(part), part.numel(), ptr(dw), ptr(db), rows, cols, float(eps),
                                    stream_ptr(x.device)))
    return part[part.numel() - 2 * rows:].view(rows, 2)


def gelu_fwd(h, y, n):
    _need_cuda(h, y); _bf(h, y)
    check(lib().vz_op_gelu_fwd(ptr(h), ptr(y), n, stream_ptr(h.device)))


def gelu_bwd(h, dy, dh, n):
    _need_cuda(h, dy, dh); _bf(h, dy, dh)
    check(lib().vz_op_gelu_bwd(ptr(h), ptr(dy), ptr(dh), n, stream_ptr(h.device)))


def swiglu_fwd(gu, act, rows, I):
    """act [rows, I] <- silu(g) u of gu [rows, 2I] in the interleaved [16 g | 16 u] column order (vz_op_swiglu_fwd)"""
    _need_cuda(gu, act); _bf(gu, act)
    check(lib().vz_op_swiglu_fwd(ptr(gu), ptr(act), rows, I, stream_ptr(gu.device)))


def swiglu_bwd(gu, dact, dgu, rows, I):
    _need_cuda(gu, dact, dgu); _bf(gu, dact, dgu)
    check(lib().vz_op_swiglu_bwd(ptr(gu), ptr(dact), ptr(dgu), rows, I, stream_ptr(gu.device)))


def rope_bwd_assemble(dq, dk, dv, dqkv, cos, sin, pos, B, S, Hq, Hkv, D, Sk_ld):
    """dqkv bf16 [B*S, (Hq+2Hkv) D] <- dq bf16 [B*S,Hq,D], dk / dv fp32 [B,Hkv,Sk_ld,D]; cos / sin fp32 [n_pos, D/2]; pos int32 [B*S]"""
    _need_cuda(dq, dk, dv, dqkv, cos, sin, pos)
    _bf(dq, dqkv); _f32(dk, dv, cos, sin); _i32(pos)
    check(lib().vz_op_rope_bwd_assemble(ptr(dq), ptr(dk), ptr(dv), ptr(dqkv), ptr(cos), ptr(sin), ptr(pos), B, S, Hq, Hkv, D, Sk_ld,
                                        stream_ptr(dqkv.device)))


def cross_entropy(logits, labels, rows, S, V, inv_n, loss_rows, dlogits=None):
    """loss_rows fp32 [rows], dlogits bf16 [rows, ldd] (optional) <- fp32 logits [rows, V], int32 labels [rows] (vz_op_cross_entropy)"""
    _need_cuda(logits, labels, loss_rows, dlogits)
    _f32(logits, loss_rows); _i32(labels); _bf(dlogits)
    check(lib().vz_op_cross_entropy(ptr(logits), V, ptr(labels), rows, S, float(inv_n), ptr(loss_rows), ptr(dlogits),
                                    0 if dlogits is None else dlogits.stride(0), stream_ptr(logits.device)))


def gather_rows_idx(src, idx, dst, rows, cols):
    _need_cuda(src, idx, dst); _bf(src, dst); _i32(idx)
    check(lib().vz_op_gather_rows_idx(ptr(src), ptr(idx), ptr(dst), rows, cols, stream_ptr(dst.device)))


def segment_sum_rows(src, seg_map, n_src, rows_per, dst, n_dst, cols):
    _need_cuda(src, seg_map, dst); _bf(src, dst); _i32(seg_map)
    check(lib().vz_op_segment_sum_rows(ptr(src), ptr(seg_map), n_src, rows_per, ptr(dst), n_dst, cols, stream_ptr(dst.device)))


def acc_rows_f32(out, src, n_batches, stride, rows, cols):
    _need_cuda(out, src); _f32(out); _bf(src)
    check(lib().vz_op_acc_rows_f32(ptr(out), ptr(src), n_batches, stride, rows, cols, stream_ptr(out.device)))


def adamw(p, m, v, g, work, n, lr, beta1, beta2, eps, weight_decay, t):
    """one fused AdamW step on fp32 p / m / v / g (vz_op_adamw); work: the bf16 or fp32 working copy"""
    _need_cuda(p, m, v, g, work); _f32(p, m, v, g)
    assert work is None or work.dtype in (torch.bfloat16, torch.float32)
    check(lib().vz_op_adamw(ptr(p), ptr(m), ptr(v), ptr(g), ptr(work), int(work is not None and work.dtype == torch.bfloat16), n, float(lr),
                            float(beta1), float(beta2), float(eps), float(weight_decay), int(t), stream_ptr(p.device)))


def attention_bwd(q, k, v, dO, scale, causal=False, window=0, kv_len=None, dkv_fp32=True):
    """Tile-resident attention backward (vz_op_attention_bwd, head_dim 128): q, dO [B,Sq,Hq,D], k / v [B,Hkv,Sk,D], all contiguous bf16
    -> dq [B,Sq,Hq,D] bf16, dk, dv [B,Hkv,Sk,D] fp32 (or bf16), summed over the query heads of a KV head."""
    _need_cuda(q, k, v, dO, kv_len)
    B, Sq, Hq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    for t in (q, k, v, dO):
        assert t.dtype == torch.bfloat16 and t.is_contiguous()
    assert dO.shape == q.shape and v.shape == k.shape
    if kv_len is not None:
        assert kv_len.dtype == torch.int32
    dq = torch.empty_like(q)
    dk = torch.empty(B, Hkv, Sk, D, dtype=torch.float32 if dkv_fp32 else torch.bfloat16, device=q.device)
    dv = torch.empty_like(dk)
    ws = torch.empty(2 * B * Hq * Sq + 64, dtype=torch.float32, device=q.device)
    check(lib().vz_op_attention_bwd(ptr(q), ptr(k), ptr(v), ptr(dO), ptr(dq), ptr(dk), ptr(dv), int(dkv_fp32), B, Sq, Sk, Hq, Hkv, D,
                                    float(scale), int(causal), int(window), ptr(kv_len), ptr(ws), ws.numel(), stream_ptr(q.device)))
    return dq, dk, dv


def attention(q, k, v, scale, causal=False, q_pos0=0, window=0, kv_len=None, workspace=None):
    """q [B,Sq,Hq,D], k/v [B,Sk,Hkv,D] (any strides with unit stride on D) -> [B,Sq,Hq,D].
    workspace: fp32 tensor; lets a few-row head_dim-512 launch split its keys over workgroups (vz_op_attention_split)."""
    _need_cuda(q, k, v, kv_len)
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    for t in (q, k, v):
        assert t.dtype == torch.bfloat16 and t.stride(3) == 1
    o = torch.empty(B, Sq, Hq, D, dtype=torch.bfloat16, device=q.device)
    if kv_len is not None:
        assert kv_len.dtype == torch.int32
    if workspace is not None:
        _need_cuda(workspace)
        assert workspace.dtype == torch.float32 and workspace.is_contiguous()
        check(lib().vz_op_attention_split(ptr(q), ptr(k), ptr(v), ptr(o), B, Sq, Sk, Hq, Hkv, D,
                                          q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2),
                                          v.stride(0), v.stride(1), v.stride(2), o.stride(0), o.stride(1), o.stride(2),
                                          float(scale), int(causal), q_pos0, window, ptr(kv_len), ptr(workspace),
                                          workspace.numel(), stream_ptr(q.device)))
        return o
    check(lib().vz_op_attention(ptr(q), ptr(k), ptr(v), ptr(o), B, Sq, Sk, Hq, Hkv, D,
                                q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2),
                                v.stride(0), v.stride(1), v.stride(2), o.stride(0), o.stride(1), o.stride(2),
                                float(scale), int(causal), q_pos0, window, ptr(kv_len), stream_ptr(q.device)))
    return o


def argmax(logits):
    _need_cuda(logits)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
    ids = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    check(lib().vz_op_argmax(ptr(logits), logits.shape[0], logits.shape[1], ptr(ids), stream_ptr(logits.device)))
    return ids


def cfg_combine(cond, uncond, scale: float):
    """HF's classifier-free guidance (guidance.hip) IN PLACE on the conditional rows: cond[r] <- scale * (lc - lu) + lu, lc / lu = the fp32
    log-softmax of cond[r] / uncond[r]; fp32 [pairs, V] each on the device (two tensors, or the halves of one [2 * pairs, V] tensor).
    The unconditional rows must be finite and are only read.  Returns `cond`."""
    _need_cuda(cond, uncond)
    for t in (cond, uncond):
        assert t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()
    assert cond.shape == uncond.shape and cond.device == uncond.device
    check(lib().vz_op_cfg_combine(ptr(cond), ptr(uncond), cond.shape[0], cond.shape[1], float(scale), stream_ptr(cond.device)))
    return cond


def proc_params(cfg):
    """the vz_logits_proc_params record of a vz_hip.logits_proc config (it owns its id lists); pass it with C.byref"""
    ints = lambda v: (C.c_int * len(v))(*v) if v else None      # noqa: E731  (an empty list: NULL)
    seq = getattr(cfg, "seq", ())
    return VzLogitsProcParams(float(cfg.penalty), int(cfg.ngram), int(cfg.min_new), len(cfg.eos), len(cfg.suppress), len(seq),
                              ints(cfg.eos), ints(cfg.suppress), ints(cfg.seq_table()) if seq else None)


def logits_process(logits, cfg, hist=None, hist_len=None):
    """HF's logits processors (logits_proc.hip; cfg = vz_hip.logits_proc.parse(...)) IN PLACE on fp32 logits [rows, V] on the device,
    over the histories hist int32 [rows, stride] of hist_len int32 [rows] ids each (None = empty: the first token of a generation).
    Returns `logits`."""
    _need_cuda(logits)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
    rows = logits.shape[0]
    if hist is None:
        hist = torch.zeros(rows, 1, dtype=torch.int32, device=logits.device)
        hist_len = torch.zeros(rows, dtype=torch.int32, device=logits.device)
    assert hist.dtype == torch.int32 and hist.dim() == 2 and hist.is_contiguous() and hist.shape[0] == rows and hist.shape[1] >= 1
    assert hist_len.dtype == torch.int32 and hist_len.is_contiguous() and hist_len.numel() == rows
    assert hist.device == logits.device and hist_len.device == logits.device
    check(lib().vz_op_logits_process(ptr(logits), rows, logits.shape[1], ptr(hist), hist.shape[1], ptr(hist_len), C.byref(proc_params(cfg)),
                                     stream_ptr(logits.device)))
    return logits


def proc_row(cfg):
    """the vz_proc_row record of a vz_hip.logits_proc config; None: an inactive record"""
    from . import logits_proc as LP
    return VzProcRow.from_buffer_copy(LP.pack_row(cfg))


def logits_process_rows(logits, cfgs, hist=None, hist_len=None):
    """the per-row form of `logits_process` (logits_proc.hip: logits_process_rows_kernel) IN PLACE on fp32 logits [rows <= 64, V]: row r by
    cfgs[r] (a vz_hip.logits_proc config; None: the row is left alone), over the histories hist int32 [rows, stride] of hist_len int32
    [rows] ids each (None = empty: the first token of an admitted request).  Nothing is appended.  Returns `logits`."""
    _need_cuda(logits)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous() and len(cfgs) == logits.shape[0]
    rows = logits.shape[0]
    if hist is None:
        hist = torch.zeros(rows, 1, dtype=torch.int32, device=logits.device)
        hist_len = torch.zeros(rows, dtype=torch.int32, device=logits.device)
    assert hist.dtype == torch.int32 and hist.dim() == 2 and hist.is_contiguous() and hist.shape[0] == rows and hist.shape[1] >= 1
    assert hist_len.dtype == torch.int32 and hist_len.is_contiguous() and hist_len.numel() == rows
    assert hist.device == logits.device and hist_len.device == logits.device
    recs = (VzProcRow * rows)(*[proc_row(c) for c in cfgs])
    seq, off = [], [0]
    for c in cfgs:
        seq += c.seq_table() if c is not None and c.seq else []
        off.append(len(seq) // 12)
    ints = lambda v: (C.c_int * len(v))(*v) if v else None      # noqa: E731
    check(lib().vz_op_logits_process_rows(ptr(logits), rows, logits.shape[1], ptr(hist), hist.shape[1], ptr(hist_len), recs, ints(seq),
                                          ints(off) if seq else None, stream_ptr(logits.device)))
    return logits


def sample_params(params):
    """the vz_sample_params records of a list of vz_hip.sample_rows.RowParams, one per row: (min_p, typical_p, epsilon_cutoff, eta_cutoff)
    = the row's `warp`, 0 = off"""
    recs = (VzSampleParams * max(1, len(params)))()
    for rec, p in zip(recs, params):
        w = getattr(p, "warp", None) or (0.0, 0.0, 0.0, 0.0)
        rec.mode, rec.temperature, rec.top_k, rec.top_p = int(p.sample), float(p.temperature), int(p.top_k), float(p.top_p)
        rec.seed, rec.counter = int(p.seed) & 0xFFFFFFFFFFFFFFFF, int(p.counter)
        rec.min_p, rec.typical_p, rec.epsilon_cutoff, rec.eta_cutoff = (float(v) for v in w)
    return recs


def sample(logits, temperature: float, top_k: int = 0, top_p: float = 1.0, seed: int = 0, counter: int = 0, warp=None):
    """one draw per row of fp32 logits [rows, V] on the device (sampling.hip): int32 [rows].  warp: None, or (min_p, typical_p,
    epsilon_cutoff, eta_cutoff) behind top-p, 0 = off."""
    _need_cuda(logits)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
    ids = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    w = warp or (0.0, 0.0, 0.0, 0.0)
    rec = VzSampleParams(ROW_SAMPLE, float(temperature), int(top_k or 0), float(1.0 if top_p is None else top_p), int(seed) & 0xFFFFFFFFFFFFFFFF,
                         int(counter), 0, *(float(v) for v in w))
    check(lib().vz_op_sample(ptr(logits), logits.shape[0], logits.shape[1], C.byref(rec), ptr(ids), stream_ptr(logits.device)))
    return ids


def sample_rows(logits, params):
    """one token per row of fp32 logits [rows <= 64, V] by that row's own parameters (params[r]: vz_hip.sample_rows.RowParams - greedy, or
    sampled with its own temperature / top-k / top-p / seed / draw counter; sampling.hip's per-row kernel): int32 [rows]."""
    _need_cuda(logits)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous() and len(params) == logits.shape[0]
    ids = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    check(lib().vz_op_sample_rows(ptr(logits), logits.shape[0], logits.shape[1], sample_params(params), ptr(ids), stream_ptr(logits.device)))
    return ids


def token_scores(logits, ids, params, warped=False):
    """the step recorder (sampling.hip: token_scores_kernel) on fp32 logits [rows, V] about the tokens ids [rows]: row r by params[r]
    (vz_hip.sample_rows.RowParams: greedy, or temperature / top-k / top-p / the further warpers; seed and counter are not read).  Returns the records fp32
    [rows, 4] = (x_tok, lse, lse_kept, n_kept as int32 bits) (vz_hip.scores.unpack), with warped=True also the score rows fp32 [rows, V]."""
    _need_cuda(logits, ids)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous() and len(params) == logits.shape[0]
    rows, V = logits.shape
    ids = ids.to(torch.int32).contiguous().view(-1)
    assert ids.numel() == rows and ids.device == logits.device
    rec = torch.empty(rows, 4, dtype=torch.float32, device=logits.device)
    w = torch.empty(rows, V, dtype=torch.float32, device=logits.device) if warped else None
    for r0 in range(0, rows, 64):          # the op takes up to 64 rows
        r1 = min(rows, r0 + 64)
        check(lib().vz_op_token_scores(ptr(logits[r0:r1]), r1 - r0, V, ptr(ids[r0:r1]), sample_params(params[r0:r1]), ptr(rec[r0:r1]),
                                       ptr(w[r0:r1]) if warped else None, stream_ptr(logits.device)))
    return (rec, w) if warped else rec


class StopTables:
    """the tables of a vz_hip.stop.Plan in device memory, for `stop_match` (the engine keeps its own copy: Engine.set_stop)"""

    def __init__(self, plan, device):
        self.plan = plan
        self.emb = None if plan.emb is None else plan.emb.to(device)
        self.target = None if plan.target is None else plan.target.to(device)
        self.seq = plan.seq_table().to(device) if plan.seqs else None


def stop_state(rows: int, device) -> torch.Tensor:
    """caller-owned matcher state for `rows` rows, int32 [rows, 2 + 64] = [n | at | ring]; `stop_match(..., reset=True)` starts it"""
    from . import stop as ST
    st = torch.zeros(rows, ST.ROW, dtype=torch.int32, device=device)
    st[:, 1] = ST.UNARMED
    return st


def stop_match(state, ids, tabs: StopTables, reset: bool = False):
    """the stop matcher (stop.hip: stop_match_kernel) on caller-owned state int32 [rows, 2 + 64]: one new id per row (ids [rows]); reset:
    the rows start clean first.  state[:, 0] = tokens seen, state[:, 1] = -1 or the index of the token at which a stop first held."""
    from . import stop as ST
    _need_cuda(state, ids)
    assert state.dtype == torch.int32 and state.dim() == 2 and state.shape[1] == ST.ROW and state.stride(1) == 1 and state.stride(0) == ST.ROW
    ids = ids.to(torch.int32).contiguous().view(-1)
    assert ids.numel() == state.shape[0] and ids.device == state.device
    p = tabs.plan
    check(lib().vz_op_stop_match(ptr(state), state.shape[0], ptr(ids), int(bool(reset)), ptr(tabs.emb), 0 if tabs.emb is None else tabs.emb.shape[0],
                                 p.vec, p.n_str, p.max_pos, p.max_end, p.window, ptr(tabs.target), ptr(tabs.seq), len(p.seqs), stream_ptr(state.device)))
    return state


def beam_k(nb: int, n_eos: int) -> int:
    """candidates per group and step (hf:generation/utils.py `_beam_search`: beams_to_keep)."""
    return max(2, 1 + n_eos) * nb


def beam_logprob_rows(logits, out=None):
    """HF's log_softmax rows of fp32 logits [rows, V] with the beam select's own reductions (beam.hip): fp32 [rows, V]; out may be
    `logits` (in place)."""
    _need_cuda(logits)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
    out = torch.empty_like(logits) if out is None else out
    assert out.dtype == torch.float32 and out.shape == logits.shape and out.is_contiguous()
    check(lib().vz_op_beam_logprob_rows(ptr(logits), logits.shape[0], logits.shape[1], ptr(out), stream_ptr(logits.device)))
    return out


def hist_beam_reorder(hist_len, hist, nb: int, groups: int, parent):
    """the processors' id histories follow the beams (beam.hip), in place: hist int32 [rows, stride] of hist_len int32 [rows] ids; row
    g * nb + j of the first groups * nb rows takes the history and length of row g * nb + parent[g * nb + j]."""
    _need_cuda(hist_len, hist, parent)
    assert hist.dtype == torch.int32 and hist.dim() == 2 and hist.is_contiguous() and hist_len.dtype == torch.int32 and hist_len.is_contiguous()
    assert hist.shape[0] >= nb * groups and hist_len.numel() >= nb * groups
    parent = parent.to(torch.int32).contiguous()
    assert parent.numel() >= nb * groups
    check(lib().vz_op_hist_beam_reorder(ptr(hist_len), ptr(hist), hist.shape[1], int(nb), int(groups), ptr(parent), stream_ptr(hist.device)))


def beam_select(logits, scores, nb_in: int, nb_out: int, eos=(), on_rows: bool = False):
    """the beam tail's selection on fp32 logits [groups * nb_in, V] with running scores [groups * nb_in] (None = 0) on the device
    (beam.hip).  Returns (records int32 [groups, K, 3] = {fp32 score bits, token, parent beam}, next tokens int32, next scores fp32,
    next parents int32 [groups * nb_out]).  on_rows: `logits` are score rows already (`beam_logprob_rows`, maybe processed): they are
    taken as they are, no normalisation."""
    _need_cuda(logits)
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous() and logits.shape[0] % nb_in == 0
    eos = [int(t) for t in eos]
    groups, dev = logits.shape[0] // nb_in, logits.device
    if scores is not None:
        scores = scores.to(dev, torch.float32).contiguous()
        assert scores.numel() == logits.shape[0]
    K = beam_k(nb_out, len(eos))
    rec = torch.empty(groups, K, 3, dtype=torch.int32, device=dev)
    tok = torch.empty(groups * nb_out, dtype=torch.int32, device=dev)
    sc = torch.empty(groups * nb_out, dtype=torch.float32, device=dev)
    par = torch.empty(groups * nb_out, dtype=torch.int32, device=dev)
    arr = (C.c_int * max(1, len(eos)))(*eos)
    op = lib().vz_op_beam_select_rows if on_rows else lib().vz_op_beam_select
    check(op(ptr(logits), logits.shape[0], logits.shape[1], int(nb_in), int(nb_out), arr, len(eos), ptr(scores),
                                  ptr(rec), ptr(tok), ptr(sc), ptr(par), stream_ptr(dev)))
    return rec, tok, sc, par


def lora_dropout(x, S: int, sample_base: int, row_stride: int, tag: int, step: int, seed: int, p: float, scaling: float):
    """the Stage-2 LoRA dropout on the device (lora.hip): x bf16 [B*S, cols] -> keep * x * scaling / (1 - p), bf16; the mask is
    vz_hip/lora.py::dropout_keep's."""
    _need_cuda(x)
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.stride(1) == 1
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    check(lib().vz_op_lora_dropout(ptr(x), x.stride(0), ptr(out), out.stride(0), x.shape[0], x.shape[1], int(S), int(sample_base), int(row_stride),
                                   int(tag), int(step), int(seed) & 0xFFFFFFFFFFFFFFFF, float(p), float(scaling), stream_ptr(x.device)))
    return out


def op_async_error(device=None) -> int:
    """async error word of op-level launches on the current stream (VZ_ASYNC_*; 0 = none); blocking, clears it."""
    err = C.c_int(0)
    check(lib().vz_op_async_error(stream_ptr(device), C.byref(err)))
    return err.value


def rope_kv(qkv, cos, sin, pos, slot, kcache, vcache, B_, S, Hq, Hkv, D):
    """qkv bf16 [B*S,(Hq+2Hkv)*D]; returns rotated q [B*S,Hq,D]; K/V written into the caches in place."""
    _need_cuda(qkv, cos, sin, pos, slot, kcache, vcache)
    q = torch.empty(B_ * S, Hq, D, dtype=torch.bfloat16, device=qkv.device)
    check(lib().vz_op_rope_kv(ptr(qkv), qkv.stride(0), ptr(q), ptr(kcache), ptr(vcache), ptr(cos), ptr(sin), ptr(pos),
                              ptr(slot), B_, S, Hq, Hkv, D, kcache.shape[2], stream_ptr(qkv.device)))
    return q


def attention_append_ws_floats(B, T, Hq, Hkv, max_ctx) -> int:
    """fp32 workspace elements that cover every key split vz_op_attention_append's host rule can choose; needs no GPU."""
    return lib().vz_op_attention_append_ws_floats(B, T, Hq, Hkv, max_ctx)


def attention_append(q, kcache, vcache, past, new, scale, kv_max, window=0, nsplit=0, out=None):
    """q rotated bf16 [B,T,Hq,128] (unit stride on D); caches [B,Hkv,max_ctx,128] holding the new tokens' K / V at slots past[b] ..
    past[b]+new[b]-1; past / new int32 [B] on the device; kv_max = max(past + new) (host) -> o [B,T,Hq,128] (`out` or a new tensor;
    token rows >= new[b] are not written).  nsplit 0 = the host rule, n >= 1 forced."""
    _need_cuda(q, kcache, vcache, past, new)
    B, T, Hq, D = q.shape
    Hkv, max_ctx = kcache.shape[1], kcache.shape[2]
    assert q.dtype == torch.bfloat16 and q.stride(3) == 1 and kcache.is_contiguous() and vcache.is_contiguous()
    assert past.dtype == torch.int32 and new.dtype == torch.int32 and past.numel() == B and new.numel() == B
    o = torch.empty(B, T, Hq, D, dtype=torch.bfloat16, device=q.device) if out is None else out
    assert o.dtype == torch.bfloat16 and o.stride(3) == 1 and tuple(o.shape) == (B, T, Hq, D)
    floats = max(attention_append_ws_floats(B, T, Hq, Hkv, max_ctx), B * Hq * T * min(nsplit, (kv_max + 63) // 64) * (D + 4), 1)
    ws = torch.empty(floats, dtype=torch.float32, device=q.device)
    check(lib().vz_op_attention_append(ptr(q), ptr(kcache), ptr(vcache), ptr(o), ptr(past), ptr(new), B, T, Hq, Hkv, D, max_ctx, int(kv_max),
                                       q.stride(0), q.stride(1), q.stride(2), o.stride(0), o.stride(1), o.stride(2),
                                       float(scale), window, nsplit, ptr(ws), ws.numel(), stream_ptr(q.device)))
    return o


def attention_shared_ws_floats(R, n, Hq, Hkv, max_ctx) -> int:
    """fp32 workspace elements that cover every key split vz_op_attention_shared's host rule can choose; 0 = a refused shape; needs no GPU."""
    return lib().vz_op_attention_shared_ws_floats(R, n, Hq, Hkv, max_ctx)


def attention_shared(q, kcache, vcache, shared, slot, n, scale, shared_max, window=0, nsplit=0, out=None, ws=None):
    """Shared-prefix decode attention (attn_shared.hip).  q rotated bf16 [R,Hq,128]; caches [rows >= R,Hkv,max_ctx,128];
    shared int32 [R / n], slot int32 [R] on the device: row r sees the slots [0, shared[r // n]) of cache row (r // n) * n and the slots
    [shared[r // n], slot[r]] of its own row; shared_max = max(shared) (host) -> o [R,Hq,128] (`out` or a new tensor).  nsplit 0 = the
    host rule, >= 1 forced; ws: the fp32 workspace (default: one that covers the call)."""
    _need_cuda(q, kcache, vcache, shared, slot)
    R, Hq, D = q.shape
    Hkv, max_ctx = kcache.shape[1], kcache.shape[2]
    assert q.dtype == torch.bfloat16 and q.is_contiguous() and kcache.is_contiguous() and vcache.is_contiguous() and kcache.shape[0] >= R
    assert shared.dtype == torch.int32 and slot.dtype == torch.int32 and slot.numel() == R and shared.numel() * n == R
    o = torch.empty(R, Hq, D, dtype=torch.bfloat16, device=q.device) if out is None else out
    assert o.dtype == torch.bfloat16 and o.is_contiguous() and tuple(o.shape) == (R, Hq, D)
    if ws is None:
        floats = max(attention_shared_ws_floats(R, n, Hq, Hkv, max_ctx), R * Hq * min(max(nsplit, 1), 64) * (D + 4), 1)
        ws = torch.empty(floats, dtype=torch.float32, device=q.device)
    check(lib().vz_op_attention_shared(ptr(q), ptr(kcache), ptr(vcache), ptr(o), ptr(shared), ptr(slot), R, int(n), Hq, Hkv, D, max_ctx,
                                       int(shared_max), float(scale), int(window), int(nsplit), ptr(ws), ws.numel(), stream_ptr(q.device)))
    return o


def attention_decode(q, kcache, vcache, ctx_len, scale, nsplit=8, window=0):
    """q bf16 [B,Hq,D]; caches [B,Hkv,max_ctx,D]; ctx_len int32 [B] -> [B,Hq,D]."""
    _need_cuda(q, kcache, vcache, ctx_len)
    Bn, Hq, D = q.shape
    ws = torch.empty(Bn * Hq * nsplit * (D + 2), dtype=torch.float32, device=q.device)
    o = torch.empty_like(q)
    check(lib().vz_op_attention_decode(ptr(q), ptr(kcache), ptr(vcache), ptr(o), ptr(ws), Bn, Hq, kcache.shape[1], D,
                                       kcache.shape[2], nsplit, window, float(scale), ptr(ctx_len), stream_ptr(q.device)))
    return o


def attention_decode_fused(qkv, kcache, vcache, cos, sin, pos, slot, Hq, scale, nsplit=32, window=0, ticket=None):
    """qkv bf16 [B,(Hq+2Hkv)*D] -> o [B,Hq,D]; appends the new K/V rows to the caches in place."""
    _need_cuda(qkv, kcache, vcache, cos, sin, pos, slot)
    Bn, Hkv, max_ctx, D = kcache.shape
    ws = torch.empty(Bn * Hkv * nsplit * (4 * D + 32), dtype=torch.float32, device=qkv.device)
    if ticket is None:
        ticket = torch.zeros(Bn * Hkv, dtype=torch.int32, device=qkv.device)
    o = torch.empty(Bn, Hq, D, dtype=torch.bfloat16, device=qkv.device)
    check(lib().vz_op_attention_decode_fused(ptr(qkv), ptr(kcache), ptr(vcache), ptr(o), ptr(ws), ptr(ticket), ptr(cos),
                                             ptr(sin), ptr(pos), ptr(slot), Bn, Hq, Hkv, D, max_ctx, nsplit, window,
                                             float(scale), stream_ptr(qkv.device)))
    return o, ticket


def kv8_mirror_rows(kcache, vcache, k8, v8, ks, vs, rows, lens):
    """The e4m3 mirror's writer on caller buffers (attn_decode_kv8.hip): slots [0, lens[i]) of cache rows rows[i] (<= 64 of them) of the bf16
    caches [R,Hkv,max_ctx,128] are quantised into k8 / v8 uint8 (same shape) and ks / vs fp32 [R,Hkv,max_ctx], in place; every other slot
    is left untouched."""
    _need_cuda(kcache, vcache, k8, v8, ks, vs)
    R, Hkv, max_ctx, D = kcache.shape
    rows, lens = [int(r) for r in rows], [int(n) for n in lens]
    assert kcache.dtype == torch.bfloat16 and vcache.dtype == torch.bfloat16 and kcache.is_contiguous() and vcache.is_contiguous() and vcache.shape == kcache.shape
    assert k8.dtype == torch.uint8 and v8.dtype == torch.uint8 and k8.is_contiguous() and v8.is_contiguous() and k8.shape == kcache.shape and v8.shape == kcache.shape
    assert ks.dtype == torch.float32 and vs.dtype == torch.float32 and ks.is_contiguous() and vs.is_contiguous() and tuple(ks.shape) == (R, Hkv, max_ctx) and vs.shape == ks.shape
    assert len(rows) == len(lens) and 1 <= len(rows) <= 64 and all(0 <= r < R for r in rows) and all(0 <= n <= max_ctx for n in lens)
    arr = lambda v: (C.c_int * len(v))(*v)    # noqa: E731
    check(lib().vz_op_kv8_mirror_rows(ptr(kcache), ptr(vcache), ptr(k8), ptr(v8), ptr(ks), ptr(vs), len(rows), arr(rows), arr(lens), Hkv, D, max_ctx,
                                      stream_ptr(kcache.device)))


def attention_decode_kv8(qkv, kcache, vcache, k8, v8, ks, vs, cos, sin, pos, slot, Hq, scale, nsplit=32, window=0, ticket=None, out=None):
    """attention_decode_fused over the e4m3 mirror (attn_decode_kv8.hip): qkv bf16 [B,(Hq+2Hkv)*D] -> o [B,Hq,D].  Slots < slot[b] are read
    from k8 / v8 uint8 [B,Hkv,max_ctx,128] with the scales ks / vs fp32 [B,Hkv,max_ctx]; the new token's row is used in bf16 and appended
    to the bf16 caches and, quantised, to the mirror, in place."""
    _need_cuda(qkv, kcache, vcache, k8, v8, ks, vs, cos, sin, pos, slot)
    Bn, Hkv, max_ctx, D = kcache.shape
    assert qkv.dtype == torch.bfloat16 and qkv.is_contiguous() and tuple(qkv.shape) == (Bn, (Hq + 2 * Hkv) * D)
    assert kcache.dtype == torch.bfloat16 and kcache.is_contiguous() and vcache.is_contiguous() and vcache.shape == kcache.shape
    assert k8.dtype == torch.uint8 and v8.dtype == torch.uint8 and k8.is_contiguous() and v8.is_contiguous() and k8.shape == kcache.shape and v8.shape == kcache.shape
    assert ks.dtype == torch.float32 and vs.dtype == torch.float32 and ks.is_contiguous() and vs.is_contiguous() and tuple(ks.shape) == (Bn, Hkv, max_ctx) and vs.shape == ks.shape
    assert pos.dtype == torch.int32 and slot.dtype == torch.int32 and pos.numel() == Bn and slot.numel() == Bn
    ws = torch.empty(Bn * Hkv * nsplit * (4 * D + 32), dtype=torch.float32, device=qkv.device)
    if ticket is None:
        ticket = torch.zeros(Bn * Hkv, dtype=torch.int32, device=qkv.device)
    o = torch.empty(Bn, Hq, D, dtype=torch.bfloat16, device=qkv.device) if out is None else out
    assert o.dtype == torch.bfloat16 and o.is_contiguous() and tuple(o.shape) == (Bn, Hq, D)
    check(lib().vz_op_attention_decode_kv8(ptr(qkv), ptr(kcache), ptr(vcache), ptr(k8), ptr(v8), ptr(ks), ptr(vs), ptr(o), ptr(ws), ptr(ticket), ptr(cos),
                                           ptr(sin), ptr(pos), ptr(slot), Bn, Hq, Hkv, D, max_ctx, nsplit, window, float(scale), stream_ptr(qkv.device)))
    return o, ticket


def _eos_arr(eos):
    eos = [int(t) for t in eos]
    return (C.c_int * max(1, len(eos)))(*eos), len(eos)


def spec_draft(history, D: int, max_ngram: int = 2, eos=()):
    """the prompt-lookup draft rule on the device (spec.hip) for an int32 history tensor: the proposed ids (a list, may be empty)."""
    _need_cuda(history)
    history = history.to(torch.int32).contiguous()
    draft = torch.zeros(D, dtype=torch.int32, device=history.device)
    ctl = torch.zeros(SPEC_CTL_WORDS, dtype=torch.int32, device=history.device)
    arr, n_eos = _eos_arr(eos)
    check(lib().vz_op_spec_draft(ptr(history), history.numel(), int(D), int(max_ngram), arr, n_eos, ptr(draft), ptr(ctl), stream_ptr(history.device)))
    return draft[:int(ctl[SPEC_CTL_DRAFTED])].tolist()


def spec_accept(logits, state, ctl, out, budget: int, hist=None, eos=(), stats=None, max_ctx: int = 1 << 20, rope_max: int = 1 << 20,
                sample=None):
    """argmax of the R logit rows + one acceptance step on caller-provided buffers, all updated in place: state int32 [4, R] =
    cur | pos | slot | len, ctl int32 [SPEC_CTL_WORDS], out int32 [>= budget], hist int32 or None, stats int32 [3] or None.
    sample (a sampled vz_hip.sample_rows.RowParams; its counter is not read): row i is drawn at counter ctl[SPEC_CTL_WRITE] + 1 + i
    instead (sampling.hip: spec_sample_kernel)."""
    _need_cuda(logits, state, ctl, out)
    R, V = logits.shape
    assert state.dtype == torch.int32 and state.is_contiguous() and state.numel() == 4 * R and ctl.numel() >= SPEC_CTL_WORDS and out.numel() >= budget
    arr, n_eos = _eos_arr(eos)
    if sample is not None:
        check(lib().vz_op_spec_accept_sampled(ptr(logits), R, V, sample_params([sample]), ptr(state), ptr(ctl), ptr(out), int(budget), ptr(hist),
                                              0 if hist is None else hist.numel(), arr, n_eos, ptr(stats), int(max_ctx), int(rope_max),
                                              stream_ptr(logits.device)))
        return
    check(lib().vz_op_spec_accept(ptr(logits), R, V, ptr(state), ptr(ctl), ptr(out), int(budget), ptr(hist), 0 if hist is None else hist.numel(),
                                  arr, n_eos, ptr(stats), int(max_ctx), int(rope_max), stream_ptr(logits.device)))


def attention_verify(qkv, kcache, vcache, cos, sin, pos, slot, Hq, scale, nsplit=8, key_bound=None, window=0, ticket=None):
    """qkv bf16 [R, (Hq + 2 Hkv) * D]: R consecutive positions of ONE sequence; caches [Hkv, max_ctx, D] (its cache row); pos / slot int32
    [R].  Appends the R rotated K / V rows in place, returns (o [R, Hq, D], ticket)."""
    _need_cuda(qkv, kcache, vcache, cos, sin, pos, slot)
    Hkv, max_ctx, D = kcache.shape
    R = qkv.shape[0]
    if key_bound is None:
        key_bound = min(max_ctx, int(slot[0]) + R)
    ws = torch.empty(lib().vz_op_spec_part_floats(R, Hkv, nsplit), dtype=torch.float32, device=qkv.device)
    if ticket is None:
        ticket = torch.zeros(Hkv, dtype=torch.int32, device=qkv.device)
    o = torch.empty(R, Hq, D, dtype=torch.bfloat16, device=qkv.device)
    q_rot = torch.empty(R, Hq, D, dtype=torch.bfloat16, device=qkv.device)
    check(lib().vz_op_attention_verify(ptr(qkv), ptr(kcache), ptr(vcache), ptr(o), ptr(q_rot), ptr(ws), ptr(ticket), ptr(cos), ptr(sin), ptr(pos),
                                       ptr(slot), R, Hq, Hkv, D, max_ctx, int(nsplit), int(key_bound), int(window), float(scale),
                                       stream_ptr(qkv.device)))
    return o, ticket
