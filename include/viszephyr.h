/*
 * viszephyr.h - C ABI of libviszephyr_hip.so: the MI355X (gfx950) implementation of the
 * Vision-Zephyr forward/generate hot path.
 *
 * The reference (baohuyvanba/Vision-Zephyr) is 100 % Python and has no FFI layer; its boundary
 * for this path is the Python class API of
 *     vis_zephyr/model/language_model/vis_zephyr.py:28-170   (VisZephyrForCausalLM.forward/generate)
 *     vis_zephyr/model/vis_zephyr_arch.py:120-333            (encode_images, prepare_inputs_labels_for_multimodal)
 * whose arithmetic it delegates to HF transformers / torch.nn.  This header is what a maintainer
 * binds (ctypes stub in INTEGRATION.md) to replace that arithmetic: plain pointers and sizes, no
 * torch types, int status codes, no exceptions across the boundary.  Every pointer named `d_*`
 * is a DEVICE pointer borrowed for the duration of the call (weights: for the engine's lifetime);
 * `stream` is a hipStream_t passed as void* (NULL = the null stream).  bf16 tensors are uint16_t.
 *
 * Two layers:
 *   1. operator entry points  (vz_op_*): one hand-written kernel each; used by the parity tests
 *      and by the engine itself.
 *   2. engine entry points    (vz_engine_* / vz_clip_* / vz_qformer / vz_llm_*): own workspace and
 *      the KV cache, sequence the kernels of one stage on the caller's stream.
 */
#ifndef VISZEPHYR_H
#define VISZEPHYR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VZ_OK 0
#define VZ_ERR_ARG 1          /* bad argument / unsupported shape  -> Python ValueError      */
#define VZ_ERR_HIP 2          /* HIP runtime error                 -> Python RuntimeError    */
#define VZ_ERR_STATE 3        /* call order / missing weights      -> Python RuntimeError    */
#define VZ_ERR_UNSUPPORTED 4  /* reference-unreachable feature     -> NotImplementedError    */

/* values of the async error word (vz_engine_async_error / vz_op_async_error): which bounded device-side wait expired */
/* (1 was the hand-off of the one-launch batch-1 attention half, removed in round 2: it never beat the three kernels) */
#define VZ_ASYNC_STREAMK 2    /* stream-K fix-up of the 256^2 GEMM: the tile was written as NaN, never as a sum of stale slots */
#define VZ_ASYNC_ONESHOT 4    /* a peer's vector never arrived in the one-shot all-reduce (comm_oneshot.hip): the output was poisoned with NaN */
#define VZ_ASYNC_ATTN_O 5     /* the O-projection workgroups of the fused attention + O launch (attn_o_fused.hip) never saw the mergers arrive: x poisoned with NaN */
#define VZ_ASYNC_PERSIST 3    /* a phase hand-off of the persistent decode-token kernel (decode_persist.hip) expired: that token's logits are garbage */

typedef void* vz_stream;
typedef struct vz_engine vz_engine;

/* last error message of the calling thread ("" if none) */
const char* vz_last_error(void);
/* ABI version; bumped on any signature change */
int vz_abi_version(void);
/* name of the code object's target ("gfx950") */
const char* vz_target_arch(void);

/* ------------------------------------------------------------------------------------------
 * 1. Operator entry points
 * ------------------------------------------------------------------------------------------ */

/* epilogue activation ids */
#define VZ_ACT_NONE 0
#define VZ_ACT_QUICK_GELU 1   /* x*sigmoid(1.702x)  hf:activations.py:117-123 (CLIPMLP)            */
#define VZ_ACT_GELU_ERF 2     /* exact GELU         torch nn.GELU (Q-Former FFN, ref builder.py:29) */
#define VZ_ACT_SWIGLU 3       /* silu(gate)*up, W rows interleaved [16 gate | 16 up]; out width N/2
                                 hf:models/mistral/modeling_mistral.py:35-48 (MistralMLP)          */

/* C[M,N'] = epi(A[M,K] . W[N,K]^T): every nn.Linear on the path
 * (hf:models/clip/modeling_clip.py:280-350, hf:models/mistral/modeling_mistral.py:35-48,122-178,
 *  torch MultiheadAttention in/out projections ref:vis_zephyr/model/multimodal_projector/builder.py:16-32).
 * bf16 A/W, fp32 accumulate (MFMA), bias fp32 [N] or NULL, residual bf16 [M,ldr] or NULL (may alias C),
 * out bf16 (out_fp32=0) or fp32.  K % 64 == 0.  M <= 8 routes to the weight-streaming GEMV. */
int vz_op_linear(const void* d_A, int lda, const void* d_W, int ldw, void* d_C, int ldc,
                 int M, int N, int K, const float* d_bias, const void* d_residual, int ldr,
                 int act, int out_fp32, vz_stream stream);
/* W8A16 weight stream for M <= 64 (decode batches; fused RMSNorm: M <= 16): W as OCP e4m3 rows [N, ldw bytes] + one fp32 power-of-two scale per row
 * (vz_hip/quant.py: 2^e * fp8 is exactly a bf16 number, so the bf16 GEMMs of the prefill run on the same weights).
 * Same epilogues as vz_op_linear; K % 1024 == 0; d_norm_w != NULL fuses the RMSNorm of x into the staging. */
int vz_op_linear_fp8(const void* d_A, int lda, const void* d_W8, int ldw, const float* d_wscale, void* d_C, int ldc,
                     int M, int N, int K, const float* d_bias, const void* d_residual, int ldr, int act, int out_fp32,
                     const float* d_norm_w, float norm_eps, vz_stream stream);
/* FP8 MFMA linear (config 5's prefill on a weight_fp8 engine): e4m3 activations x e4m3 weights on v_mfma_scale_f32_16x16x128_f8f6f4,
 * one power-of-two scale per activation row and per weight row applied to the fp32 sum, then vz_op_linear's epilogues.
 * vz_op_quant_rows_fp8 is the activation quantiser: scale[r] = 2^e with e the smallest integer such that max|x_row| <= 448 * 2^e,
 * q = e4m3(x * 2^-e) round-to-nearest-even - the weights' quantiser (vz_hip/quant.py::quantize_rows), byte for byte.  K % 128 == 0. */
/* RMSNorm + that quantiser in one launch (the bytes and scales of vz_op_rmsnorm followed by vz_op_quant_rows_fp8); cols <= 5120 */
int vz_op_rmsnorm_quant_fp8(const void* d_x, int ldx, const float* d_w, float eps, void* d_q, int ldq, float* d_scale, int rows, int cols, vz_stream stream);
int vz_op_quant_rows_fp8(const void* d_x, int ldx, void* d_q, int ldq, float* d_scale, int rows, int K, vz_stream stream);
int vz_op_linear_fp8_mfma(const void* d_A8, int lda, const float* d_ascale, const void* d_W8, int ldw, const float* d_wscale, void* d_C, int ldc,
                          int M, int N, int K, const float* d_bias, const void* d_residual, int ldr, int act, int out_fp32, vz_stream stream);
/* x -> bf16(norm_w * x * rsqrt(mean(x^2) + eps)) fused into the staging of the weight-stream kernels (decode: QKV, gate-up,
 * lm_head; hf:models/mistral/modeling_mistral.py:182-199), then vz_op_linear's contract without bias.  1 <= M <= 16. */
int vz_op_linear_rmsnorm(const void* d_A, int lda, const float* d_norm_w, float norm_eps, const void* d_W, int ldw, void* d_C, int ldc,
                         int M, int N, int K, const void* d_residual, int ldr, int act, int out_fp32, vz_stream stream);
/* Fragment-tiled copy of a dense bf16 weight [N, K] (N % 16 == 0, K % 64 == 0) for the 2..64-row MFMA weight stream: the 16 bytes
 * W[16 G + r][64 s + 16 g + 8 j .. + 7] move to chunk ((G * K/64 + s) * 2 + j) * 64 + (16 g + r), so that every wave-instruction of the
 * stream reads 1 KiB contiguous.  An engine uses the copy registered as "<weight name>t" (same element count) for its decode
 * linears; vz_op_linear_tiled is the same launch at op level (results bit-identical to the row-major stream, impl 3). */
int vz_op_tile_weights(const void* d_W, int N, int K, int ldw, void* d_Wt, vz_stream stream);
int vz_op_linear_tiled(const void* d_A, int lda, const void* d_W, const void* d_Wt, int ldw, void* d_C, int ldc, int M, int N, int K,
                       const float* d_bias, const void* d_residual, int ldr, int act, int out_fp32, const float* d_norm_w,
                       float norm_eps, vz_stream stream);
/* W8A16 form for 17..64 rows (ABI 10; SURVEY config 5: batched decode of the e4m3-weight engine - the reference's analogue is
 * load_8bit / load_4bit, ref:vis_zephyr/model/builder.py:33-43, applied to every generate call of the eval loop,
 * ref:vis_zephyr/eval/eval_vqa.py:176-199).  vz_op_tile_weights_fp8: e4m3 rows [N][ldw bytes] -> fragment order
 * W8t[((G * K/64 + s) * 64 + 16 g + r) * 16 + i] = W8[16 G + r][64 s + 16 g + i] (one 1-KiB wave-instruction per 64-k step and 16-row
 * group).  vz_op_linear_tiled_fp8: C = epi(A . (2^e_row * W8)^T) on that copy, bf16 activations, 17 <= M <= 64, N % 128 == 0,
 * K % 1024 == 0; an engine registers the copy as "<e4m3 name>t" (dtype 2) and its 17..64-row decode steps stream it. */
int vz_op_tile_weights_fp8(const void* d_W8, int N, int K, int ldw, void* d_W8t, vz_stream stream);
int vz_op_linear_tiled_fp8(const void* d_A, int lda, const void* d_W8t, const float* d_wscale, void* d_C, int ldc, int M, int N, int K,
                           const float* d_bias, const void* d_residual, int ldr, int act, int out_fp32, vz_stream stream);
/* same contract, forcing one implementation (tests): impl 0 = 128^2 MFMA tile GEMM, 1 = GEMV (M <= 8), 2 = 256^2 tile GEMM,
 * 3 = MFMA weight stream for 2 <= M <= 64 (batched decode), 4 = the 128^2 tile GEMM with the finer split-K of the 17..64-row decode route */
int vz_op_linear_impl(int impl, const void* d_A, int lda, const void* d_W, int ldw, void* d_C, int ldc,
                      int M, int N, int K, const float* d_bias, const void* d_residual, int ldr,
                      int act, int out_fp32, vz_stream stream);

/* Route query: the kernel family a linear of this shape runs on, without running it (touches no device; works without a GPU).
 * Returns 0 GEMV, 1 SKINNY, 2 SKINNY_PERSIST, 3 SKINNY_WIDE (gemm_skinny.hip's three forms), 4 WIDE_BF16, 5 WIDE_E4M3 (gemm_wide.hip),
 * 6 TILE128, 7 TILE256 - or -1 where the entry point would refuse the arguments.  `flags`: which copies of W exist and what the call
 * fuses; `entry`: whose call it is.  Pointers count as 16-byte aligned, ldc / ldr as the output width.  *pre_norm (may be NULL) = 1 if
 * the RMSNorm runs as its own launch before the linear, *splitk_hint (may be NULL) = the split-K factor handed to the 128^2 GEMM (0 = its own).
 * The planner behind it (csrc/linear_route.hip) reads the tune knobs, so vz_tune_set changes the answer as it changes the launches. */
#define VZ_ROUTE_WT 1u         /* the fragment-tiled bf16 copy exists (vz_op_tile_weights)           */
#define VZ_ROUTE_W8 2u         /* the row-major e4m3 copy + row scales exist                          */
#define VZ_ROUTE_W8T 4u        /* the fragment-tiled e4m3 copy + row scales exist                     */
#define VZ_ROUTE_NORM 8u       /* an RMSNorm over A belongs to the call                               */
#define VZ_ROUTE_BIAS 16u
#define VZ_ROUTE_RESIDUAL 32u
#define VZ_ROUTE_DECODE 64u    /* VZ_LINEAR_ENGINE only: the rows are the sequences of a decode step */
#define VZ_LINEAR_ENGINE 0     /* a linear of an engine stage (prefill, CLIP, Q-Former; VZ_ROUTE_DECODE: a decode step) */
#define VZ_LINEAR_OP 1         /* vz_op_linear, vz_op_linear_fp8 */
#define VZ_LINEAR_RMSNORM 2    /* vz_op_linear_rmsnorm           */
#define VZ_LINEAR_TILED 3      /* vz_op_linear_tiled             */
#define VZ_LINEAR_TILED_FP8 4  /* vz_op_linear_tiled_fp8         */
#define VZ_LINEAR_IMPL 8       /* + impl: vz_op_linear_impl      */
int vz_op_linear_route(int M, int N, int K, int lda, int ldw, int act, int out_fp32, unsigned flags, int entry,
                       int* pre_norm, int* splitk_hint);

/* Causal-LM loss of forward(labels=...) (ref:vis_zephyr/model/language_model/vis_zephyr.py:51-98 hands labels to MistralForCausalLM.forward; hf:loss/loss_utils.py ForCausalLMLoss):
 * fp32 logits [B, S, V], int32 labels [B, S] (-100 = ignored), row (b, s) scored against labels[b][s + 1], mean over the valid targets.
 * d_loss_rows: B * S floats of scratch; d_out[0] = loss (NaN when no target is valid, as torch's mean), d_out[1] = number of valid targets. */
int vz_op_causal_lm_loss(const float* d_logits, int B, int S, int V, const int* d_labels, float* d_loss_rows, float* d_out, vz_stream stream);

/* y = LayerNorm(x) (torch.nn.LayerNorm; CLIP hf:...modeling_clip.py:353-384, Q-Former builder.py:14-27,68-70) */
int vz_op_layernorm(const void* d_x, int ldx, void* d_y, int ldy, const float* d_w, const float* d_b,
                    int rows, int cols, float eps, vz_stream stream);
/* y = w * x * rsqrt(mean(x^2)+eps)  (MistralRMSNorm hf:models/mistral/modeling_mistral.py:182-199) */
int vz_op_rmsnorm(const void* d_x, int ldx, void* d_y, int ldy, const float* d_w,
                  int rows, int cols, float eps, vz_stream stream);

/* softmax(scale * Q K^T [+causal/window mask]) V, fp32 softmax, GQA by head grouping
 * (hf:models/clip/modeling_clip.py:259-277; hf:models/mistral/modeling_mistral.py:84-119;
 *  torch MultiheadAttention).  Element strides (batch, seq, head) per tensor; head_dim in {64,128,512}.
 * causal: query i of batch b sits at absolute position q_pos0 + i and sees keys j <= position,
 * j > position - window (window <= 0: unlimited).  d_kv_len (int32 [B]) or NULL (= Sk) bounds the
 * valid keys of each batch row. */
int vz_op_attention(const void* d_q, const void* d_k, const void* d_v, void* d_o,
                    int B, int Sq, int Sk, int Hq, int Hkv, int head_dim,
                    long q_bs, long q_ss, long q_hs, long k_bs, long k_ss, long k_hs,
                    long v_bs, long v_ss, long v_hs, long o_bs, long o_ss, long o_hs,
                    float scale, int causal, int q_pos0, int window, const int* d_kv_len,
                    vz_stream stream);

/* The same operator given an fp32 workspace of `workspace_floats` elements: a launch with Sq <= 64 un-masked query rows,
 * head_dim 512 and many keys (the Q-Former cross-attention of ref:vis_zephyr/model/multimodal_projector/builder.py:34-39,
 * 32 queries x 576 visual tokens per tile) gives every 96 keys their own workgroup and merges the partial softmaxes in a second
 * kernel (the split depends on Sk only: a row's result is independent of B).  Needs B*Hq*ceil(Sk/96)*Sq*516 floats; with less
 * (or any other shape) it runs as vz_op_attention, which is this call without a workspace. */
int vz_op_attention_split(const void* d_q, const void* d_k, const void* d_v, void* d_o,
                          int B, int Sq, int Sk, int Hq, int Hkv, int head_dim,
                          long q_bs, long q_ss, long q_hs, long k_bs, long k_ss, long k_hs,
                          long v_bs, long v_ss, long v_hs, long o_bs, long o_ss, long o_hs,
                          float scale, int causal, int q_pos0, int window, const int* d_kv_len,
                          float* d_workspace, long workspace_floats, vz_stream stream);

/* Append attention (attn_append.hip): d_new[b] query tokens of cache row b behind d_past[b] cached positions (int32 [B], device), the new
 * tokens' K / V already at cache slots past[b] .. past[b] + new[b] - 1.  d_q rotated bf16 [B, T, Hq, 128] by element strides, caches
 * [B][Hkv][max_ctx][128].  Token i of row b sees the slots j <= past[b] + i (window > 0: and j > past[b] + i - window); token rows
 * i >= new[b] are not written, no slot at or behind past[b] + new[b] is read.  The Hq / Hkv query heads of a KV head share one query tile
 * and the keys are split over workgroups: kv_max = max_b(past[b] + new[b]) on the host chooses the split (nsplit = 0) or nsplit >= 1
 * forces it (cut to the 64-key tiles of kv_max and to 64).  The workspace holds the fp32 partials: vz_op_attention_append_ws_floats(...) floats
 * cover every split the rule can choose up to max_ctx (pure host arithmetic; 0 = a shape the op refuses); a forced split needs
 * B * Hq * nsplit * T * 132.  head_dim 128 only. */
int vz_op_attention_append(const void* d_q, const void* d_kcache, const void* d_vcache, void* d_o, const int* d_past, const int* d_new,
                           int B, int T, int Hq, int Hkv, int head_dim, int max_ctx, int kv_max,
                           long q_bs, long q_ss, long q_hs, long o_bs, long o_ss, long o_hs,
                           float scale, int window, int nsplit, float* d_workspace, long workspace_floats, vz_stream stream);
long vz_op_attention_append_ws_floats(int B, int T, int Hq, int Hkv, int max_ctx);

/* Attention BACKWARD, tile-resident (attn_bwd_flash.hip): dQ, dK, dV of softmax(scale Q K^T + mask) V without an Sq x Sk tensor in memory - the
 * form the reference trains through (ref:vis_zephyr/train/zephyr_flash_attn_monkey_patch.py:100-124; masks as vz_op_attention: causal,
 * sliding window, per-sample key count).  head_dim 128.  q, dO, dq [B,Sq,Hq,D] bf16; k, v [B,Hkv,Sk,D] bf16; dk, dv [B,Hkv,Sk,D] fp32
 * (dkv_fp32 = 1) or bf16, already summed over the query heads of a KV head.  d_ws: >= 2 * B * Hq * Sq + 64 floats. */
int vz_op_attention_bwd(const void* d_q, const void* d_k, const void* d_v, const void* d_dO, void* d_dq, void* d_dk, void* d_dv, int dkv_fp32,
                        int B, int Sq, int Sk, int Hq, int Hkv, int head_dim, float scale, int causal, int window, const int* d_kv_len,
                        float* d_ws, long ws_floats, vz_stream stream);
/* Two helpers of the training step (train.hip) at op level: vz_op_transpose dst[c][r] = src[r][c] (bf16 [R,C] -> [C,R]; 64 x 64 tiles through the
 * hardware transposing LDS read when R, C and the leading dimensions are multiples of 8 and the bases 16-byte aligned), vz_op_colsum
 * d_out[c] += sum_r y[r][c] (fp32, the bias gradients; fixed summation order) with d_part >= vz_op_colsum_groups(rows) * cols floats. */
int vz_op_transpose(const void* d_src, long src_ld, void* d_dst, long dst_ld, int R, int C, vz_stream stream);
int vz_op_colsum(const void* d_y, int ld, long rows, int cols, float* d_part, long part_floats, float* d_out, vz_stream stream);
int vz_op_colsum_groups(long rows);
/* The other kernels of the training step at op level (train.hip; the parity tests of tests/test_train_ops_gpu.py).  bf16 unless said otherwise;
 * every launcher refuses null pointers, non-positive sizes and what its kernel cannot address (VZ_ERR_ARG), it never falls back.
 *   transpose_batched  dst[o][i][c][col0 + r] = src[o][i][r][c] for o < n_outer, i < n_inner (element strides *_rs row, *_so outer, *_si inner):
 *                      128- / 64-wide tiles when R, C, col0 and all strides are multiples of 8 and the bases 16-byte aligned, else 32 x 32
 *   softmax_fwd        P[row][j] = softmax_j(scale S[row][j]) over the visible keys, exactly 0 elsewhere and in the padding up to ldp; S fp32;
 *                      row = (b * H + h) * Sq + i; causal: key j <= i, window > 0: j > i - window; d_kv_len[b] (optional) caps the keys
 *   softmax_bwd        dS = P (dP - sum_j P dP) scale, exactly 0 (and dP unread) where P == 0 and in the padding up to ldds; dP fp32
 *   rmsnorm_bwd        dx = r (dy w - xh mean(dy w xh)) [+ dres], contiguous [rows, cols]; w fp32
 *   layernorm_bwd      dx = rstd (g - mean g - xh mean(g xh)) [+ dres] (d_dx may be NULL), d_dw += sum_rows dy xh, d_db += sum_rows dy (fp32, fixed
 *                      order); cols % 8 == 0, 16-byte-aligned rows; d_part >= vz_op_layernorm_bwd_scratch_floats(rows, cols) floats and ends
 *                      with the (mean, rstd) pair of every row
 *   gelu_* / swiglu_*  exact-erf GELU and silu(g) u on saved pre-activations and their derivatives; SwiGLU reads gu [rows, 2I] in the GEMM's
 *                      interleaved column order [16 g | 16 u] (I % 16 == 0) and writes dgu in the same order
 *   rope_bwd_assemble  fused-QKV gradient rows [Hq D | Hkv D | Hkv D] from dq [B*S,Hq,D] bf16 and dk, dv [B,Hkv,Sk_ld,D] fp32: Q and K parts rotated
 *                      back by the angles of d_pos (tables [pos][D/2] fp32), V copied; D even
 *   cross_entropy      row (b, s) against labels[b][s + 1]: d_loss_rows = lse - logit[target], d_dlogits (optional, leading dimension ldd >= V,
 *                      padding zeroed) = (softmax - onehot) inv_n; a row whose target is < 0, >= V (torch would raise) or beyond the sequence
 *                      is ignored: loss 0, zero gradient row
 *   gather_rows_idx    dst[r] = src[idx[r]], zeros where idx[r] < 0 (cols % 8 == 0, 16-byte-aligned bases)
 *   segment_sum_rows   dst[r][q] = sum over k < n_src with map[k] == r of src[k][q] (blocks of rows_per rows; fp32 sum, bf16 out)
 *   acc_rows_f32       d_out[i] += sum_b src[b * stride + i] for i < rows * cols (fp32)
 *   adamw              torch.optim.AdamW step t >= 1 on fp32 master / moments / gradient; writes the working copy (bf16 or fp32), clears d_g */
int vz_op_transpose_batched(const void* d_src, long src_rs, long src_so, long src_si, void* d_dst, long dst_rs, long dst_so, long dst_si, int R, int C,
                            int n_outer, int n_inner, int col0, vz_stream stream);
int vz_op_softmax_fwd(const float* d_S, int lds, void* d_P, int ldp, long rows, int H, int Sq, int Sk, float scale, int causal, int window,
                      const int* d_kv_len, vz_stream stream);
int vz_op_softmax_bwd(const void* d_P, int ldp, const float* d_dP, int lddp, void* d_dS, int ldds, long rows, int Sk, float scale, vz_stream stream);
int vz_op_rmsnorm_bwd(const void* d_x, const float* d_w, const void* d_dy, const void* d_dres, void* d_dx, long rows, int cols, float eps,
                      vz_stream stream);
long vz_op_layernorm_bwd_scratch_floats(long rows, int cols);
int vz_op_layernorm_bwd(const void* d_x, const float* d_w, const void* d_dy, const void* d_dres, void* d_dx, float* d_part, long part_floats,
                        float* d_dw, float* d_db, long rows, int cols, float eps, vz_stream stream);
int vz_op_gelu_fwd(const void* d_h, void* d_y, long n, vz_stream stream);
int vz_op_gelu_bwd(const void* d_h, const void* d_dy, void* d_dh, long n, vz_stream stream);
int vz_op_swiglu_fwd(const void* d_gu, void* d_act, long rows, int I, vz_stream stream);
int vz_op_swiglu_bwd(const void* d_gu, const void* d_dact, void* d_dgu, long rows, int I, vz_stream stream);
int vz_op_rope_bwd_assemble(const void* d_dq, const float* d_dk, const float* d_dv, void* d_dqkv, const float* d_cos, const float* d_sin,
                            const int* d_pos, int B, int S, int Hq, int Hkv, int head_dim, int Sk_ld, vz_stream stream);
int vz_op_cross_entropy(const float* d_logits, int V, const int* d_labels, long rows, int S, float inv_n, float* d_loss_rows, void* d_dlogits, int ldd,
                        vz_stream stream);
int vz_op_gather_rows_idx(const void* d_src, const int* d_idx, void* d_dst, long rows, int cols, vz_stream stream);
int vz_op_segment_sum_rows(const void* d_src, const int* d_map, int n_src, int rows_per, void* d_dst, int n_dst, int cols, vz_stream stream);
int vz_op_acc_rows_f32(float* d_out, const void* d_src, int n_batches, long stride, int rows, int cols, vz_stream stream);
int vz_op_adamw(float* d_p, float* d_m, float* d_v, float* d_g, void* d_work, int work_bf16, long n, float lr, float beta1, float beta2, float eps,
                float weight_decay, int t, vz_stream stream);
/* RoPE (rotate-half, hf:models/mistral/modeling_mistral.py:51-81) on the Q and K heads of a fused QKV row
 * [B*S, (Hq+2Hkv)*D] + append of K/V to the cache [B][Hkv][max_ctx][D].  d_pos / d_slot: int32 [B*S] position
 * id and cache slot of every token (slot < 0: token not cached).  d_q_out bf16 [B*S,Hq,D].  D = 128. */
int vz_op_rope_kv(const void* d_qkv, int ld, void* d_q_out, void* d_kcache, void* d_vcache, const float* d_cos,
                  const float* d_sin, const int* d_pos, const int* d_slot, int B, int S, int Hq, int Hkv, int head_dim,
                  int max_ctx, vz_stream stream);

/* one query token per slot against the KV cache (decode step of hf:...modeling_mistral.py:139-178).
 * d_q / d_o bf16 [B,Hq,D]; caches [B][Hkv][max_ctx][D]; d_ctx_len int32 [B] = keys visible (device memory, so a
 * captured graph replays for every step); d_workspace fp32 [B*Hq*nsplit*(D+2)]. */
int vz_op_attention_decode(const void* d_q, const void* d_kcache, const void* d_vcache, void* d_o, float* d_workspace,
                           int B, int Hq, int Hkv, int head_dim, int max_ctx, int nsplit, int window, float scale,
                           const int* d_ctx_len, vz_stream stream);

/* The decode step's attention as the engine runs it: RoPE on the new token's Q/K, append of K/V to the cache,
 * attention over the cache (4 query heads per KV head served from one pass over K/V) and the merge of the
 * nsplit context slices, in ONE launch.  d_qkv bf16 [B,(Hq+2Hkv)*D] (un-rotated projection of the new token);
 * d_pos / d_slot int32 [B] (position id, cache slot = tokens already cached); d_ticket uint32 [B*Hkv], zeroed
 * once by the caller; d_workspace fp32 [B*Hkv*nsplit*(4*D+32)].  Same result as vz_op_rope_kv followed by
 * vz_op_attention_decode. */
int vz_op_attention_decode_fused(const void* d_qkv, void* d_kcache, void* d_vcache, void* d_o, float* d_workspace,
                                 unsigned* d_ticket, const float* d_cos, const float* d_sin, const int* d_pos,
                                 const int* d_slot, int B, int Hq, int Hkv, int head_dim, int max_ctx, int nsplit,
                                 int window, float scale, vz_stream stream);

/* ------------------------------------------------------------------------------------------
 * 2. Engine
 * ------------------------------------------------------------------------------------------ */
typedef struct vz_config {
    /* Zephyr-7B-beta (ref:checkpoints/vis-zephyr-7b-v1-pretrain/config.json:10-38) */
    int hidden, inter, n_layers, n_heads, n_kv_heads, head_dim, vocab;
    float rms_eps, rope_theta;
    int sliding_window;
    /* CLIP ViT-L/14-336 (ref:vis_zephyr/model/vision_encoder/vision_encoder.py:21) */
    int clip_hidden, clip_inter, clip_layers, clip_heads, clip_image, clip_patch;
    float clip_eps;
    /* Q-Former (ref:vis_zephyr/model/multimodal_projector/builder.py:49-70) */
    int qf_queries, qf_blocks, qf_heads, qf_kv_dim;
    float qf_eps;
    /* fusion (ref:vis_zephyr/model/vision_encoder/vision_encoder.py:63-64) */
    int fusion_groups, fusion_layers_per_group;
    /* capacity */
    int max_batch;        /* KV-cache slots                                  */
    int max_ctx;          /* tokens per slot                                 */
    int max_tiles;        /* tiles per vz_clip_fused_features / vz_qformer   */
    int max_text;         /* Lmax of the Q-Former text conditioning          */
    /* tensor parallelism over RCCL (1 = single GPU) */
    int tp_size, tp_rank;
    /* mm_vision_select_feature (ref:vis_zephyr/model/vision_encoder/vision_encoder.py:66-73): 0 = 'patch' (drop CLS, 576 tokens per
     * tile, the shipped config), 1 = 'cls_patch' (keep it: 577 tokens per tile into the fusion and the Q-Former) */
    int clip_keep_cls;
    /* 1 = the decode-side linears of Zephyr (q|k|v, o, gate|up, down, lm_head at M <= 8) stream e4m3 copies of the weights
     * ("<name>8" u8 + "<name>s" fp32 row scales, registered beside the bf16 tensors); the bf16 tensors must then hold the
     * dequantised values so that prefill and decode run the same model (vz_hip/quant.py, SURVEY config 5) */
    int weight_fp8;
} vz_config;

int vz_engine_create(const vz_config* cfg, vz_engine** out);
int vz_engine_destroy(vz_engine* e);

/* The stage workspace.  An engine owns one arena; each stage call (CLIP, Q-Former, prefill, decode steps) lays its buffers out in it with
 * that stage's one carving function, which also sizes the arena (it only grows).  vz_engine_ws_info: the arena's bytes and the mark the
 * last stage call's carving reached (equal on the call that sized the arena).  vz_op_stage_ws_bytes: the bytes that carving takes for a
 * call of the given dimensions on an engine of `cfg` - this rank's shard sizes, the current tune knobs - from the same function, without
 * a device (works without a GPU); -1 for a config vz_engine_create or a shape the stage would refuse.
 *   VZ_STAGE_CLIP     n = T tiles;  VZ_WS_CALLER_HIDDEN: the caller supplies d_hidden_dbg
 *   VZ_STAGE_QFORMER  n = T, n2 = n_samples, Lmax;  VZ_WS_QF_KV_CONTIG: the blocks' ca_kv weights lie back to back (vz_qformer's layout
 *                     hint), so the K|V projections of all blocks share one buffer unless the 2 GiB cap or knob 25 says otherwise
 *   VZ_STAGE_PREFILL  n = B, n2 = S
 *   VZ_STAGE_DECODE   n = B rows of the running batch;  VZ_WS_SPEC_TAIL: verify steps of the speculative tail (B = R in 2..8)
 *   VZ_STAGE_APPEND   n = B, n2 = T new token rows per cache row (vz_llm_prefill_append) */
#define VZ_STAGE_APPEND 4
#define VZ_STAGE_CLIP 0
#define VZ_STAGE_QFORMER 1
#define VZ_STAGE_PREFILL 2
#define VZ_STAGE_DECODE 3
#define VZ_WS_CALLER_HIDDEN 1u
#define VZ_WS_QF_KV_CONTIG 2u
#define VZ_WS_SPEC_TAIL 4u
int vz_engine_ws_info(vz_engine* e, size_t* arena_bytes, size_t* peak_bytes);
long vz_op_stage_ws_bytes(const vz_config* cfg, int stage, int n, int n2, int Lmax, unsigned flags);

/* Register one weight under its engine name (see vz_hip/weights.py for the packing from the
 * reference's state-dict keys).  dtype: 0 = bf16, 1 = fp32, 2 = u8 (e4m3 bytes).  The pointer is borrowed until destroy. */
int vz_engine_set_weight(vz_engine* e, const char* name, const void* d_ptr, int dtype, long n_elems);
/* check that every weight the configuration needs has been registered */
int vz_engine_finalize(vz_engine* e);
/* change the vocabulary of a live engine (tokens added to the tokenizer: ref:vis_zephyr/model/builder.py:141-153 grows
 * embed_tokens / lm_head by <im_patch>).  The caller then registers the new "llm.embed" / "llm.lm_head" tables and
 * finalizes again.  tp_size == 1 only. */
int vz_engine_resize_vocab(vz_engine* e, int new_vocab);
/* Tensor parallelism (vz_config.tp_size > 1): one process per GPU; q/k/v/gate/up column-parallel,
 * o/down row-parallel with an RCCL all-reduce of [B,S,hidden] bf16 after each (2 per layer), lm_head vocab-parallel with
 * an all-gather of the fp32 logits; the KV cache is sharded by KV head.  CLIP / Q-Former weights are replicated.
 * vz_comm_unique_id fills a 128-byte ncclUniqueId on one rank; the caller ships it to the other ranks (any transport) and
 * every rank calls vz_comm_init with it before its first prefill. */
int vz_comm_unique_id(char* out128);
int vz_comm_init(vz_engine* e, const char* id128);
/* Tile data parallelism (first row): every anyres tile is an independent unit through CLIP, fusion and
 * the Q-Former, so the host deals tile t to rank t mod tp_size, each rank encodes its tiles, and ONE all-gather of
 * bytes_per_rank bytes per rank (ceil(T / tp_size) x 32 x hidden bf16, zero-padded) hands every rank all visual tokens.
 * d_recv holds tp_size consecutive chunks in rank order.  At tp_size == 1 this is a device copy. */
int vz_tp_all_gather(vz_engine* e, const void* d_send, void* d_recv, size_t bytes_per_rank, vz_stream stream);

/* fp32 rotary tables [max_pos, head_dim/2] (rotate-half convention, hf:...modeling_mistral.py:51-81,262-317) */
int vz_engine_set_rope(vz_engine* e, const float* d_cos, const float* d_sin, int max_pos);

/* a8-a10: CLIPVisionTower.forward + feature_select + fusion
 * (ref:vis_zephyr/model/vision_encoder/vision_encoder.py:58-117, gating_fusion.py:22-50).
 * d_images bf16 [T,3,336,336] -> d_out bf16 [T,576,5*clip_hidden].
 * d_hidden_dbg: NULL, or bf16 [(clip_layers+1),T,577,clip_hidden] receiving every hidden state (tests). */
int vz_clip_fused_features(vz_engine* e, const void* d_images, int T, void* d_out, void* d_hidden_dbg,
                           vz_stream stream);

/* a11: QFormer.forward (ref:vis_zephyr/model/multimodal_projector/builder.py:72-92).
 * d_feats bf16 [T,576,qf_kv_dim]; text conditioning per SAMPLE: d_text bf16 [n_samples,Lmax,hidden]
 * (rows past a sample's own length are the zero padding of ref:vis_zephyr/model/vis_zephyr_arch.py:178-189),
 * h_tile_sample[T] maps each tile to its sample (the reference expands the same text to every tile of a
 * sample, vis_zephyr_arch.py:174).  Lmax = 0: no text.  d_out bf16 [T,32,hidden].
 * Layout hint: when the blocks' "qf.<i>.ca_kv.w" (and ".b") tensors lie back to back in device memory, block-major - one
 * [qf_blocks * 2 * hidden, qf_kv_dim] allocation registered slice by slice - the cross-attention K|V projections of all blocks run
 * as ONE product (they read the same pre-normed features); any other placement computes them block by block, same results up to
 * the stream-K tail's fp32 re-association. */
int vz_qformer(vz_engine* e, const void* d_feats, int T, const void* d_text, int n_samples, int Lmax,
               const int* h_tile_sample, void* d_out, vz_stream stream);

/* a6/a7 data movement: out[r,:] = kind[r]==0 ? embed_tokens[idx[r]] : kind[r]==1 ? d_visual[idx[r]] : 0
 * (the row map itself is host index logic, ref:vis_zephyr/model/vis_zephyr_arch.py:214-333,476-530). */
int vz_embed_splice(vz_engine* e, const int* d_kind, const int* d_idx, int rows, const void* d_visual,
                    void* d_out, vz_stream stream);

/* a12 prefill: MistralForCausalLM.forward on inputs_embeds (hf:models/mistral/modeling_mistral.py:340-466).
 * d_embeds bf16 [B,S,hidden] right-padded, h_seqlens[B] valid lengths, d_pos int32 [B,S] position ids.
 * Fills KV slots 0..B-1 from position 0.  d_logits_all: NULL or fp32 [B,S,vocab] (forward() computes all
 * positions); d_logits_last: NULL or fp32 [B,vocab] (row seqlen-1 of each sample; what generate needs). */
int vz_llm_prefill(vz_engine* e, const void* d_embeds, int B, int S, const int* h_seqlens, const int* d_pos,
                   float* d_logits_all, float* d_logits_last, vz_stream stream);

/* a13 greedy decode.  vz_llm_decode_begin arms the device-side state after a prefill: the first input
 * token of every slot (d_first_ids int32 [B]), next position ids and context lengths (host int [B]).
 * vz_llm_decode_steps enqueues n steps with no host synchronisation: every step embeds the current token,
 * runs the 32 layers against the cache, takes argmax of the fp32 logits (first maximal index, as
 * torch.argmax) and feeds it to the next step.  d_out_ids int32 [B, n] receives the n new tokens;
 * d_logits_dbg NULL or fp32 [n,B,vocab]. */
int vz_llm_decode_begin(vz_engine* e, int B, const int* d_first_ids, const int* h_next_pos, const int* h_ctx_len,
                        vz_stream stream);
int vz_llm_decode_steps(vz_engine* e, int n, int* d_out_ids, float* d_logits_dbg, vz_stream stream);
/* vz_llm_decode_steps rejects (VZ_ERR_ARG) a call whose n steps would take a live row past max_ctx keys or past the rotary
 * tables; rows parked by vz_llm_decode_set_row(ctx_len 0) saturate on the device instead.
 *
 * How one row chooses its next token: the record every sampling entry point takes (ABI 11: it replaces the loose scalars, the parallel
 * host arrays and the *_warp twins of ABI 10).  48 bytes, the entry of the per-row table in device memory as it is:
 *   offset 0 mode, 4 temperature, 8 top_k, 12 top_p, 16 seed (low word first), 24 counter, 28 reserved,
 *   32 min_p, 36 typical_p, 40 epsilon_cutoff, 44 eta_cutoff
 * mode = VZ_ROW_GREEDY: first maximal index; only `counter` is read besides.  mode = VZ_ROW_SAMPLE: logits / temperature, top-k, top-p,
 * then the warpers hf:generation/utils.py `_get_logits_processor` puts behind TopPLogitsWarper, in its order (csrc/sampling.hip step
 * 3b):
 *   min_p           drop p_i < min_p * p_max                              0 <= min_p <= 1; 0 = off
 *   typical_p       ascending in |-log p_i - H| keep the shortest prefix whose mass reaches typical_p (it may leave out the most
 *                   likely token)                                           0 or >= 1 = off
 *   epsilon_cutoff  drop p_i < epsilon                                    0 or >= 1 = off
 *   eta_cutoff      drop p_i < min(eta, sqrt(eta) * exp(-H))              0 or >= 1 = off
 * each over the set the one before it left (p = softmax over that set, H its entropy) and each keeping at least the largest score
 * of that set; then a Gumbel race keyed by Philox4x32-10(seed; vocab index, row, draw counter).  The kept set is a key interval of x;
 * the draw and the step recorder (lse_kept, n_kept, warped rows) take the same one.
 * One check for every entry point, before it touches the device (VZ_ERR_ARG): mode 0 or 1; counter >= 0; a sampled record needs
 * temperature > 0, top_k >= 0 (0 = off), 0 < top_p <= 1 (1 = off), 0 <= min_p <= 1, typical_p / epsilon_cutoff / eta_cutoff >= 0; a NaN
 * fails.  (ABI 10 let vz_op_sample pass top_k < 0, top_p > 1 and counter < 0, refused its temperature <= 0 only after device calls,
 * and let vz_op_token_scores pass counter < 0.) */
#define VZ_ROW_GREEDY 0
#define VZ_ROW_SAMPLE 1
typedef struct vz_sample_params {
    int mode;
    float temperature;
    int top_k;
    float top_p;
    unsigned long long seed;
    int counter;       /* the draw counter of the row's next token */
    int reserved;
    float min_p, typical_p, epsilon_cutoff, eta_cutoff;
} vz_sample_params;
/* Sampling tail (hf:generation/utils.py `_sample`, do_sample=True; ref:vis_zephyr/serve/cli.py:171-182 = temperature 0.2 +
 * HF's default top_k 50): after vz_llm_decode_sampling with a VZ_ROW_SAMPLE record every decode step draws its token on the device
 * by that record, inside the same per-token hipGraph, so a streamer / stopping-criteria loop reads back 4 bytes per token.
 * p->counter is the draw counter the next vz_llm_decode_begin starts from; it is kept for a VZ_ROW_GREEDY record (= the argmax again)
 * too, whose other fields are not looked at.  vz_op_sample: the same kernel on arbitrary fp32 logits rows, one VZ_ROW_SAMPLE record
 * for all of them, the row index in the Philox counter (the first token, drawn from the prefill logits with counter 0; tests).
 * Restated in oracle/sampling_oracle.py. */
int vz_llm_decode_sampling(vz_engine* e, const vz_sample_params* p);
/* Streamer / stopping-criteria loop (ref:vis_zephyr/serve/cli.py:155-182 passes a TextStreamer and a KeywordsStoppingCriteria:
 * one host callback per token): every step's tail also writes its token to ring[row * ring_n + (draw counter mod ring_n)], a
 * device-visible HOST buffer of ring_rows x ring_n ints, so the host keeps a step in flight and reads token t when the event behind
 * step t fires.  vz_llm_decode_steps refuses a decode batch with more rows than the ring holds (ABI 10: ring_rows). */
int vz_llm_decode_ring(vz_engine* e, int* host_visible_ring, int ring_n, int ring_rows);
int vz_op_sample(const float* d_logits, int rows, int cols, const vz_sample_params* p, int* d_ids, vz_stream stream);
/* Logits processors in the step (hf:generation/logits_process.py, in the order of `_get_logits_processor`: sequence bias, repetition
 * penalty, no-repeat-n-gram, bad words, min-new-tokens, suppress-tokens, then the sampler's warpers): after vz_llm_decode_logits_proc
 * with a record every decode step whose tail is the argmax or the sampler first runs them on its fp32 logits, on the device and inside the per-token
 * hipGraph (the parameters are part of what a captured step freezes: a change captures again).  They see the ids generated so
 * far, never the prompt (the reference generates from inputs_embeds): a per-row history kept on the device, emptied here
 * (stream-ordered) and extended at every step by the row's input token - so arm it before vz_llm_decode_begin, after the first
 * token was chosen on logits that went through vz_op_logits_process with empty histories.  repetition_penalty > 0 (1 = off),
 * 0 <= no_repeat_ngram <= 8 (0 = off), the <= 4 eos ids are -inf while fewer than min_new_tokens ids were generated, the <= 16
 * suppressed ids always; vocabularies up to 65536.  vz_llm_decode_steps refuses the mode together with the speculative tail
 * (with the beam tail: see "beam search: processors and rows" below); tensor-parallel engines are VZ_ERR_UNSUPPORTED.  p = NULL:
 * off (no launch is added to the step).
 * seq: the id sequences of hf:SequenceBiasLogitsProcessor (first in HF's chain, in front of the repetition penalty) and
 * hf:NoBadWordsLogitsProcessor (behind the n-gram ban), int32 [n_seq][12] =
 *   [len 1..8 | kind: 0 = bias, 1 = bad word | bias, fp32 bits | 0 | ids[8]],  n_seq <= 64 (0: seq may be NULL)
 * with the one-id sequences first and each group in the caller's order - the order HF adds the biases in.  A one-id sequence acts at
 * every step; a longer one acts on its last id when the ids generated so far end in its first len - 1 ids and (HF's length check) at
 * least len ids were generated.  Biases that land on one id add up in fp32 in table order, then the penalty acts on the biased score,
 * then the bans write -inf; a bad word bans without arithmetic.  Ids outside [0, cols) are ignored.  The engine keeps the table in its
 * own device memory: an arming with the table of the previous arming uploads nothing, a new table is uploaded outside any capture and
 * the next vz_llm_decode_steps captures again.
 * vz_op_logits_process: the same kernel in place on fp32 logits [rows, cols] over the caller's histories d_hist [rows][hist_stride]
 * (int32) of d_hist_len[row] ids each; ids outside [0, cols) are ignored.  Bit-identical to HF's processors on fp32.
 * Both check the whole record before they touch the device (VZ_ERR_ARG). */
typedef struct vz_logits_proc_params {
    float repetition_penalty;
    int no_repeat_ngram, min_new_tokens;
    int n_eos, n_suppress, n_seq;
    const int* eos;        /* n_eos ids                          */
    const int* suppress;   /* n_suppress ids                     */
    const int* seq;        /* n_seq entries of 12 ints, or NULL  */
} vz_logits_proc_params;
int vz_llm_decode_logits_proc(vz_engine* e, const vz_logits_proc_params* p, vz_stream stream);
int vz_op_logits_process(float* d_logits, int rows, int cols, int* d_hist, int hist_stride, int* d_hist_len,
                         const vz_logits_proc_params* p, vz_stream stream);
/* Per-row logits processors (csrc/logits_proc.hip: logits_process_rows_kernel): the rows of a continuous batch are
 * independent requests, so each row takes its processors from its own record of a table in device memory - the per-row tail's form
 * (vz_llm_decode_sampling_rows) carried to the processors.  The record, 32 ints = 128 bytes, by byte offset:
 *     0  repetition_penalty   float, > 0, 1 = off
 *     4  no_repeat_ngram      0..8, 0 = off
 *     8  min_new_tokens       >= 0: the eos ids are -inf while fewer ids were generated
 *    12  n_eos                0..4
 *    16  eos[4]
 *    32  n_suppress           0..16
 *    36  suppress[16]
 *   100  n_seq                0..64 id sequences of sequence_bias / bad_words_ids in the row's region of the sequence table
 *   104  active               0 = the row is not processed: no logit touched, nothing appended to its history (the other fields are not read)
 *   108  reserved[5]
 * The id sequences of row r are entries [0, n_seq) of region r of a per-row table [max_batch][64][12] ints, each entry as in
 * vz_logits_proc_params.seq.  Same arithmetic, order and limits as vz_llm_decode_logits_proc: bit-identical to it row by row.
 * vz_llm_decode_logits_proc_rows(enable = 1): arms the launch where the call-level one sits - behind the guidance combine and the raw-row
 * recorder, in front of the argmax / the sampler / the per-row tail - with every record inactive and every history empty (stream-ordered).
 * VZ_ERR_ARG together with vz_llm_decode_logits_proc (whichever is armed second); vz_llm_decode_steps refuses it with the beam or the
 * speculative tail; tensor-parallel engines: VZ_ERR_UNSUPPORTED.  enable = 0: off, no launch is added to the step.
 * vz_llm_decode_set_row_logits_proc: stream-ordered like vz_llm_decode_set_row - uploads row `row`'s record and its n_seq (= rec->n_seq)
 * sequences h_seq [n_seq][12] and sets the row's history length and seeded-id count to 0; rec = NULL: the row becomes inactive.  The
 * whole record and the sequences are checked before the device is touched (VZ_ERR_ARG).  The captured step reads the tables through
 * pointers: the call changes no kernel argument and captures nothing (vz_llm_decode_info).
 * vz_op_logits_process_rows: the same kernel on caller-owned fp32 logits [rows <= 64, cols] and histories, row r by h_rows[r]; its
 * sequences are entries [h_nseq_off[r], h_nseq_off[r + 1]) of h_seq [.][12] (h_nseq_off: rows + 1 ints; NULL when no row has any).
 * Nothing is appended (the first token of an admitted request: its prefill logits row with an empty history; tests). */
typedef struct vz_proc_row {
    float repetition_penalty;
    int no_repeat_ngram, min_new_tokens;
    int n_eos, eos[4];
    int n_suppress, suppress[16];
    int n_seq, active;
    int reserved[5];
} vz_proc_row;
int vz_llm_decode_logits_proc_rows(vz_engine* e, int enable, vz_stream stream);
int vz_llm_decode_set_row_logits_proc(vz_engine* e, int row, const vz_proc_row* rec, const int* h_seq, int n_seq, vz_stream stream);
int vz_op_logits_process_rows(float* d_logits, int rows, int cols, int* d_hist, int hist_stride, int* d_hist_len, const vz_proc_row* h_rows,
                              const int* h_seq, const int* h_nseq_off, vz_stream stream);
/* how the last vz_llm_decode_steps ran: *graph = 1 when a captured hipGraph was replayed; *comm_in_graph = 1 when the RCCL
 * collectives of a tensor-parallel engine are part of that graph (0 = eager steps, e.g. after RCCL refused the capture) */
int vz_llm_decode_mode(vz_engine* e, int* graph, int* comm_in_graph);
/* context splits of the last decode-steps call (its context bucket) and the graphs captured since the engine was created */
int vz_llm_decode_info(vz_engine* e, int* nsplit, int* captures);
/* Batch-1 decode on an MI355X (ABI 10): after vz_tune_set(28, 1), with one row, one GPU, bf16 weights and the Zephyr-7B geometry,
 * vz_llm_decode_steps runs every token as ONE resident grid (decode_persist.hip: the 161 launches of a step become phases with
 * in-launch hand-offs; bit-identical logits).  Opt-in: on MI355X it measured slower than the launch chain.  A phase hand-off that expires raises VZ_ASYNC_PERSIST (vz_engine_async_error).
 * vz_test_persist_poke is a test hook: *mode = 1 if the last steps ran that way; word >= 0 presets an arrival counter. */
int vz_test_persist_poke(vz_engine* e, int word, unsigned value, int* mode, vz_stream stream);
/* One-shot all-reduce of the tensor-parallel decode step (ABI 10; comm_oneshot.hip): every rank stores its bf16 vector into every
 * peer's receive area as 8-byte {two bf16, sequence tag} granules (system scope: over xGMI when the areas are peer-mapped) and sums the
 * N vectors it finds in its own area in rank order - one store-and-poll round instead of a ring.  `d_areas[q]` = rank q's receive area
 * (vz_op_oneshot_area_bytes(n_ranks, max_elems) bytes, zero-filled once; peer areas opened through hipIpc by the caller), `d_seq` = two
 * device words {sequence number = 1, ticket = 0} (a zero-filled area carries tag 0 = "nothing yet", so the numbering starts at 1); the launch advances the sequence number itself, so it replays
 * from a hipGraph.  An engine with tp_size > 1 uses it for its decode-step all-reduces after vz_comm_oneshot_attach (RCCL otherwise).
 * Tested in one process (N areas on one GPU, N concurrent launches); unmeasured over xGMI - no multi-GPU box was available. */
size_t vz_op_oneshot_area_bytes(int n_ranks, int max_elems);
int vz_op_allreduce_oneshot(void* const* d_areas, int rank, int n_ranks, int max_elems, const void* d_in, void* d_out, int n, unsigned* d_seq,
                            int* d_err, vz_stream stream);
/* test form: all n_ranks ranks as slices of one grid (one process, one GPU); d_in / d_out / d_seq are arrays of n_ranks pointers */
int vz_test_allreduce_oneshot_all(void* const* d_areas, int n_ranks, int max_elems, const void* const* d_in, void* const* d_out, int n,
                                  unsigned* const* d_seq, int* d_err, vz_stream stream);
/* engine side: this rank's receive area + sequence words (allocated on first call; out_area may be exported with hipIpcGetMemHandle),
 * then the N areas in rank order (own included) - from then on the decode step's [B, hidden] all-reduces take the one-shot kernel */
int vz_comm_oneshot_local(vz_engine* e, void** out_area, size_t* out_bytes);
int vz_comm_oneshot_attach(vz_engine* e, void* const* d_areas, int n_ranks);
/* profiling: s_memrealtime stamps (100 MHz) of workgroup 0's sync wave at the 12 phase edges of every layer of the last token */
int vz_prof_persist_stamps(vz_engine* e, unsigned long long* host_out, int n_layers);
/* batch-1 decode runs QKV GEMV + attention + O GEMV of a layer as ONE launch whose roles hand over through device-side counters;
 * every device-side wait is bounded and raises a word when it expires.  Reads and clears that word (blocking): *err != 0 = the
 * outputs since the previous call are invalid. */
int vz_engine_async_error(vz_engine* e, int* err);
/* The same word for op-level launches (vz_op_linear* whose 256^2 GEMM took the stream-K tail) on `stream`.  Stream-K state
 * (fp32 slots, arrival tickets, error word) exists once per (device, stream): launches that share it are stream-ordered.  A wait
 * that expires raises VZ_ASYNC_STREAMK, leaves the tickets untouched and poisons its tile with NaN; reading the error resets the
 * tickets of that stream. */
int vz_op_async_error(vz_stream stream, int* err);
/* TEST HOOK (tests/test_ops_gpu.py): overwrite the {arrive, ready} ticket pair of stream-K remainder tile `tile` on `stream`. */
int vz_test_corrupt_streamk(vz_stream stream, int tile, int arrive, int ready);
/* weight_fp8 engines: enable = 1 runs the Zephyr prefill linears as e4m3 x e4m3 on the scaled MFMA (inputs quantised per row by
 * vz_op_quant_rows_fp8's kernel, weights = the registered e4m3 copies); 0 (default) = bf16 MFMA on the dequantised bf16 tensors */
int vz_engine_prefill_fp8(vz_engine* e, int enable);
/* forget a registered weight (e.g. the e4m3 copy of a bf16 tensor that has been rewritten) */
int vz_engine_unset_weight(vz_engine* e, const char* name);
/* Continuous batching.  vz_llm_prefill_rows: vz_llm_prefill into KV-cache rows row0 .. row0+B-1;
 * vz_llm_decode_set_row: (re)arm one row of the running decode batch - next input token, rotary position, context length -
 * without touching the others (a finished row is parked with ctx_len 0 until a new request is prefilled into it). */
int vz_llm_prefill_rows(vz_engine* e, int row0, const void* d_embeds, int B, int S, const int* h_seqlens, const int* d_pos,
                        float* d_logits_all, float* d_logits_last, vz_stream stream);
int vz_llm_decode_set_row(vz_engine* e, int row, int token, int next_pos, int ctx_len, vz_stream stream);
/* Append prefill: T new embedding rows per cache row behind what the row already holds.  Cache rows row0 .. row0+B-1 keep their slots
 * [0, h_past[b]); token t < h_new[b] of sample b is appended at slot h_past[b] + t at rotary position d_pos[b, t] and sees the slots
 * <= its own (sliding window as the prefill).  One pass of the prefill's layer loop over the B*T rows; the attention is
 * vz_op_attention_append (or, for more than 256 rows per sample, the prefill's flash kernel once per run of rows with equal past).
 * d_logits_all NULL or fp32 [B,T,vocab] (rows t >= h_new[b] are computed from padding: ignore them), d_logits_last NULL or fp32
 * [B,vocab] = row h_new[b] - 1.  VZ_ERR_ARG unless 1 <= h_new[b] <= T, h_past[b] >= 0, h_past[b] + h_new[b] <= max_ctx and the rotary
 * tables cover max_ctx; tensor-parallel engines: VZ_ERR_UNSUPPORTED. */
int vz_llm_prefill_append(vz_engine* e, int row0, const void* d_embeds, int B, int T, const int* h_new, const int* h_past, const int* d_pos,
                          float* d_logits_all, float* d_logits_last, vz_stream stream);
/* Per-row tail (csrc/sampling.hip: sample_rows_kernel): every row of the decode batch chooses its next token by its own entry of a table
 * in device memory, a vz_sample_params record with its own 64-bit seed and draw counter (the kernel counts it up after every step).
 * A sampled row gets the bits vz_op_sample gives a ONE-row
 * call with the same parameters: its Philox counter is (vocab index, 0, draw counter), so the draws of a request do not depend on the cache
 * row it decodes in.  The captured step reads the table through a pointer: changing an entry changes no kernel argument and captures nothing.
 * vz_llm_decode_sampling_rows(enable=1): arms the tail and keeps the `rows` records h_rows (0..max_batch; the rows behind them greedy)
 * for the NEXT vz_llm_decode_begin to upload; enable = 0: the argmax / the sampler again.  vz_llm_decode_set_row_sampling: one row's entry of the running
 * batch, stream-ordered - the counterpart of vz_llm_decode_set_row.  The logits processors may sit in front of the tail as in front of
 * the sampler; vz_llm_decode_steps refuses it together with the beam or the speculative tail; tensor-parallel engines: VZ_ERR_UNSUPPORTED.
 * vz_op_sample_rows: the same kernel on fp32 logits [rows <= 64, cols] (the first token of each sequence from the prefill logits with
 * counter 0; tests). */
int vz_llm_decode_sampling_rows(vz_engine* e, int enable, int rows, const vz_sample_params* h_rows);
int vz_llm_decode_set_row_sampling(vz_engine* e, int row, const vz_sample_params* p, vz_stream stream);
int vz_op_sample_rows(const float* d_logits, int rows, int cols, const vz_sample_params* h_rows, int* d_ids, vz_stream stream);
/* Step recorder (csrc/sampling.hip: token_scores_kernel): per-token scores and log-probs of a generation, recorded
 * on the device.  After vz_llm_decode_scores(what != 0) every decode step writes, behind its tail (argmax, sampler or per-row tail) and
 * inside the per-token hipGraph, one record of four 32-bit words per row about the token the tail chose:
 *   x_tok    = logits[row, tok] after the logits processors, before temperature (NaN for a token outside the vocabulary)
 *   lse      = log sum_i exp(x_i) over the whole row (fp32, natural log): log-prob at temperature 1 = x_tok - lse
 *   lse_kept = log sum_{i kept} exp(x_i / T) over the tokens the row's sampler keeps for its (T, top_k, top_p) - the sampler's own set;
 *              a greedy row: lse.  x_tok / T - lse_kept = HF's compute_transition_scores(normalize_logits=True) on its warped scores
 *   n_kept   = size of that set (int32; its finite entries); a greedy row: cols
 * what = VZ_SCORE_REC, optionally | VZ_SCORE_WARPED (also the row HF calls scores[t]: x for a greedy row, x / T where kept and -inf
 * elsewhere for a sampled one) | VZ_SCORE_RAW (also logits[t]: the row as the lm_head left it, copied in front of the processors).
 * The buffers are rings of cap_steps steps in device memory: d_rec [slot][B][4], d_warped / d_raw [slot][B][vocab] (null when not asked
 * for); slot = the steps launched since vz_llm_decode_begin (or since this call, whichever is later) modulo cap_steps, counted on the
 * device; vz_llm_decode_set_row leaves it alone.  The pointers, `what` and cap_steps are frozen by a captured step: a change captures
 * again, and with the recorder off no launch is added.  vz_llm_decode_steps refuses n > cap_steps and the recorder together with the beam
 * or the speculative tail; tensor-parallel engines: VZ_ERR_UNSUPPORTED.  what = 0: off.
 * vz_op_token_scores: the same kernel on fp32 logits [rows <= 64, cols] about the tokens d_ids [rows] (int32), row r by the record
 * h_rows[r] as vz_op_sample_rows takes it (seed and counter are checked, not read): d_rec [rows][4], d_warped [rows][cols] or
 * null (the first token of a generation, chosen from the prefill logits; tests). */
#define VZ_SCORE_REC    1u   /* the 16-byte records            */
#define VZ_SCORE_WARPED 2u   /* + processed, warped score rows */
#define VZ_SCORE_RAW    4u   /* + raw logits rows              */
int vz_llm_decode_scores(vz_engine* e, unsigned what, float* d_rec, float* d_warped, float* d_raw, int cap_steps, vz_stream stream);
int vz_op_token_scores(const float* d_logits, int rows, int cols, const int* d_ids, const vz_sample_params* h_rows, float* d_rec,
                       float* d_warped, vz_stream stream);
/* Stop matcher (csrc/stop.hip: stop_match_kernel): stop strings and keyword stops decided on the device.  After
 * vz_llm_decode_stop(enable = 1) every decode step runs, behind its tail (argmax, sampler or per-row tail; behind the step recorder if
 * that is armed) and inside the per-token hipGraph, one 64-lane wave per row over the row's state: n = generated tokens seen, at = -1
 * or the 0-based index of the token at which a stop condition first held (sticky), and a ring of the last VZ_STOP_W ids.  Two rules:
 *   stop strings: HF's StopStringCriteria.__call__ over the tables HF's constructor builds - h_emb = embedding_vec, int32 [emb_rows =
 *     V + 2][vec = n_str * (max_pos + max_end) + 1], max_pos = max_valid_positions, max_end = max_valid_end_lens, window =
 *     maximum_token_len, h_target = target_lens [n_str];
 *   id sequences (KeywordsStoppingCriteria of mm_utils): h_seq int32 [n_seq][VZ_STOP_SEQ_STRIDE] = [len, start, the ids NEWEST FIRST];
 *     sequence k matches when n >= start + len and the last len generated ids equal it.
 * Limits: VZ_STOP_MAX_STR strings, window <= VZ_STOP_W, max_pos <= VZ_STOP_MAX_POS, max_end <= VZ_STOP_MAX_END, VZ_STOP_MAX_SEQ sequences
 * of <= VZ_STOP_MAX_SEQ_LEN ids.  The call copies the tables into engine-owned device memory (never inside a capture); the matcher writes
 * only its own state, never a word the step reads, so arming it changes no id.  Frozen by a captured step: a change captures again, and
 * with the matcher off no launch is added.  Refused with the beam or the speculative tail; tensor-parallel engines: VZ_ERR_UNSUPPORTED.
 * vz_llm_decode_stop_rows: rows [row0, row0 + rows) start clean and their first tokens d_first_ids [rows] (int32, device; chosen from the
 * prefill logits, outside the step) go through the same kernel - call it where vz_llm_decode_begin / vz_llm_decode_set_row are called.
 * Every arming starts with no row watched: a row is matched from this call on, never from what an earlier arming left in its state.  vz_llm_decode_stop_read: at[row0 .. row0 + rows) into d_at (int32, device), stream-ordered.
 * vz_op_stop_match: the kernel on caller-owned state d_state [rows][VZ_STOP_ROW] and device tables, one new id per row d_ids [rows]
 * (reset != 0: the rows start clean first); state word 0 = n, word 1 = at, words 2.. = the ring. */
#define VZ_STOP_W 64
#define VZ_STOP_ROW (2 + VZ_STOP_W)
#define VZ_STOP_MAX_STR 8
#define VZ_STOP_MAX_POS 16
#define VZ_STOP_MAX_END 8
#define VZ_STOP_MAX_SEQ 16
#define VZ_STOP_MAX_SEQ_LEN 32
#define VZ_STOP_SEQ_STRIDE (2 + VZ_STOP_MAX_SEQ_LEN)
#define VZ_STOP_UNARMED (-2)
int vz_llm_decode_stop(vz_engine* e, int enable, const int* h_emb, int emb_rows, int vec, int n_str, int max_pos, int max_end, int window,
                       const int* h_target, const int* h_seq, int n_seq, vz_stream stream);
int vz_llm_decode_stop_rows(vz_engine* e, int row0, int rows, const int* d_first_ids, vz_stream stream);
int vz_llm_decode_stop_read(vz_engine* e, int row0, int rows, int* d_at, vz_stream stream);
/* Per-row stop sequences: the id-sequence rule of the matcher reads row r's sequences from region r of an
 * engine-owned table [max_batch][VZ_STOP_MAX_SEQ][VZ_STOP_SEQ_STRIDE] and their count from a per-row word; the stop strings stay
 * call-level and shared.  vz_llm_decode_stop_row_seqs(enable = 1): arms the mode behind vz_llm_decode_stop, or on its own - no stop
 * string and no call-level sequence at all is allowed here, a row with nothing to match is never a hit.  Every row's region starts as
 * the call-level sequences and, as with every arming, no row is watched.  While the mode is armed vz_llm_decode_stop is VZ_ERR_ARG
 * (disarm the mode first); refusals otherwise as for vz_llm_decode_stop.  enable = 0: off (with the matcher off too, no launch is added).
 * vz_llm_decode_stop_set_row_seqs: stream-ordered - row `row`'s region becomes the call-level sequences followed by its own n_seq
 * sequences h_seq [n_seq][VZ_STOP_SEQ_STRIDE] ([len, start, the ids newest first]); together they must fit VZ_STOP_MAX_SEQ (VZ_ERR_ARG,
 * checked before the device is touched).  It captures nothing.  vz_llm_decode_stop_rows keeps its meaning: the row starts clean and its
 * first token goes through the kernel - call it behind this one. */
int vz_llm_decode_stop_row_seqs(vz_engine* e, int enable, vz_stream stream);
int vz_llm_decode_stop_set_row_seqs(vz_engine* e, int row, const int* h_seq, int n_seq, vz_stream stream);
/* Seeded histories (a generate() call that continues on a kept cache; host ids, stream-ordered; behind the arming, in front of
 * vz_llm_decode_begin / vz_llm_decode_stop_rows).  vz_llm_decode_stop_seed: the last min(n, 63) of the n ids fed before generation begins
 * enter row `row`'s ring in front of its first generated token, so a stop string may begin in them as in the tail of HF's input_ids; the
 * id sequences still match generated ids only and `at` still counts generated tokens.  vz_llm_decode_logits_proc_seed: the n <= max_ctx
 * ids become row `row`'s history - they count for the penalty, the n-grams and the id sequences as a prompt's ids do in HF - while
 * min_new_tokens counts the ids behind them. */
int vz_llm_decode_stop_seed(vz_engine* e, int row, const int* h_ids, int n, vz_stream stream);
int vz_llm_decode_logits_proc_seed(vz_engine* e, int row, const int* h_ids, int n, vz_stream stream);
int vz_op_stop_match(int* d_state, int rows, const int* d_ids, int reset, const int* d_emb, int emb_rows, int vec, int n_str, int max_pos,
                     int max_end, int window, const int* d_target, const int* d_seq, int n_seq, vz_stream stream);
/* Batched admissions: prefill several requests together into spare cache rows (row0 >= the running batch), then move each one's
 * first h_len[i] cache positions from row h_src[i] to the freed row h_dst[i] (every layer, K and V; stream-ordered).  Rows of
 * one call must not overlap (no destination equal to another move's source or destination). */
int vz_llm_kv_move_rows(vz_engine* e, int n, const int* h_src, const int* h_dst, const int* h_len, vz_stream stream);

/* ---- beam search (hf:generation/utils.py `_beam_search`, do_sample=False; csrc/beam.hip; vz_hip/beam.py replays the records) ----
 * K = max(2, 1 + n_eos) * nb candidates per group and step; equal scores go to the smaller flat index beam * V + token.
 * vz_llm_decode_beam(enable=1): the tail of every decode step selects beams on the device.  The running decode batch holds `groups`
 * prompts x `nb` (2..16) beam rows (row g * nb + j); d_scores [groups * nb] = the running beam scores, h_base[g] = prompt length of
 * group g, d_hist = history records int32 [hist_steps][groups][K][3] = {fp32 score bits, token, parent beam}, appended at a
 * device-side step index that restarts at 0 here.  After each selection the cache positions [h_base[g], slot) of every row whose
 * parent is another row become the parent's (in place, bit-exact).  enable = 0: argmax / the sampler again.  tp_size > 1: unsupported.
 * vz_op_beam_select: the same selection on fp32 logits [rows = groups * nb_in, cols] with running scores d_scores_in [rows] (NULL = 0):
 * d_records [groups][K][3] and the next running beams d_next_tok / d_next_score / d_next_parent [groups * nb_out] (the first step:
 * nb_in = 1 on the prefill logits).  vz_llm_kv_beam_reorder: the reorder alone, positions [h_base[g], h_end[g]) of group g, local parent
 * indices d_parent [groups * nb] on the device. */
int vz_llm_decode_beam(vz_engine* e, int enable, int nb, int groups, const int* h_eos, int n_eos, const int* h_base,
                       const float* d_scores, int* d_hist, int hist_steps, vz_stream stream);
int vz_op_beam_select(const float* d_logits, int rows, int cols, int nb_in, int nb_out, const int* h_eos, int n_eos,
                      const float* d_scores_in, int* d_records, int* d_next_tok, float* d_next_score, int* d_next_parent, vz_stream stream);
int vz_llm_kv_beam_reorder(vz_engine* e, int nb, int groups, const int* h_base, const int* h_end, const int* d_parent, vz_stream stream);
/* device-to-device copy of the whole KV cache (bf16 [layer][K|V][max_batch][kv head][max_ctx][head_dim]) into d_out; *bytes = its
 * size (d_out = NULL: the size only).  Tests. */
int vz_llm_kv_copy_out(vz_engine* e, void* d_out, size_t max_bytes, size_t* bytes, vz_stream stream);

/* ---- opt-in e4m3 mirror of the KV cache that the decode attention streams (csrc/attn_decode_kv8.hip; vz_hip/kv8.py) ----
 * The bf16 cache stays: prefill writes it, the prefill and append-prefill attention read it.  Beside it the mirror holds every cache row as OCP
 * e4m3 bytes with ONE fp32 power-of-two scale per (cache row, KV head, slot), for K (after RoPE) and for V, each 128-value row quantised as
 * vz_hip/quant.py::quantize_rows quantises a weight row - +50 % KV memory.  Writers: the prefills (slots [0, past + new) of the rows they touch,
 * every layer), vz_llm_kv_move_rows (slots [0, len) of the destination rows) and the decode step itself (the new token's row).
 * vz_engine_kv_fp8(e, 1) allocates the mirror and marks every row invalid until one of the first two writers has rebuilt it:
 * vz_llm_decode_begin / vz_llm_decode_set_row return VZ_ERR_STATE for a row with ctx_len > 0 whose mirror is invalid.  While on, the decode
 * step runs the kv8 attention for every batch size (no attention + O fusion, no persistent token kernel) and vz_llm_decode_spec,
 * vz_llm_decode_share, vz_llm_decode_beam and vz_llm_kv_beam_reorder return VZ_ERR_UNSUPPORTED.  VZ_ERR_UNSUPPORTED on tp_size > 1.
 * vz_engine_kv_fp8(e, 0) (the default state) frees it: every call is the plain engine's.  Not inside a capture.
 * vz_llm_kv8_copy_out (tests): the mirror's bytes [layer][K|V][max_batch][kv head][max_ctx][head_dim] into d_q and its fp32 scales
 * [layer][K|V][max_batch][kv head][max_ctx] into d_scales; *q_bytes / *scale_floats = the sizes (d_q = d_scales = NULL: the sizes only).
 * vz_op_kv8_mirror_rows: the writer on caller buffers - slots [0, h_len[i]) of rows h_row[i] (n <= 64) of d_kcache / d_vcache bf16
 * [R][Hkv][max_ctx][128] into d_k8 / d_v8 (same shape, bytes) and d_ks / d_vs fp32 [R][Hkv][max_ctx]; other slots are left untouched.
 * vz_op_attention_decode_kv8: vz_op_attention_decode_fused over the mirror - slots < d_slot[b] are read from d_k8 / d_v8 with their scales,
 * the new token's row is used in bf16 and appended to the bf16 caches and, quantised, to the mirror; B <= 64, nsplit <= 32. */
int vz_engine_kv_fp8(vz_engine* e, int enable);
int vz_llm_kv8_copy_out(vz_engine* e, void* d_q, size_t max_q_bytes, float* d_scales, size_t max_scale_floats, size_t* q_bytes,
                        size_t* scale_floats, vz_stream stream);
int vz_op_kv8_mirror_rows(const void* d_kcache, const void* d_vcache, void* d_k8, void* d_v8, float* d_ks, float* d_vs, int n,
                          const int* h_row, const int* h_len, int Hkv, int head_dim, int max_ctx, vz_stream stream);
int vz_op_attention_decode_kv8(const void* d_qkv, void* d_kcache, void* d_vcache, void* d_k8, void* d_v8, float* d_ks, float* d_vs,
                               void* d_o, float* d_workspace, unsigned* d_ticket, const float* d_cos, const float* d_sin,
                               const int* d_pos, const int* d_slot, int B, int Hq, int Hkv, int head_dim, int max_ctx, int nsplit,
                               int window, float scale, vz_stream stream);

/* ---- prompt-lookup speculative decoding of one greedy sequence (hf:generation/candidate_generator.py PromptLookupCandidateGenerator;
 * csrc/spec.hip; vz_hip/spec.py) ----
 * A verify step carries R = D + 1 rows (D in 1..7) of ONE sequence in cache row 0: row 0 = the last emitted token, rows 1..D = guessed
 * continuations.  Row i runs at rotary position p + i, appends its K / V at cache slot L + i and sees keys [.., L + i]; g_i = argmax of
 * row i (the argmax op's tie rule); the step emits g_0 .. g_a for the longest prefix with draft_(i+1) == g_i, stops at the first eos id
 * among them (inclusive) and at `budget` ids, and advances the state by the number emitted.
 * Control words (device int32 [VZ_SPEC_CTL_WORDS]): write index into d_out, history length, done flag (eos emitted / budget reached:
 * later steps emit nothing), ids the current draft holds, steps run; words 8..15 = the last step's argmax ids.
 * Arm it with a decode-begin call of R rows (tokens [t, any..], positions p + i, context lengths L + i), then the decode-spec call
 * (enable=1): d_hist int32 [hist_cap] holds hist_len ids, one per position of the sequence so far INCLUDING the token of row 0 (-1 = a
 * position without a text id: never matches, ends a proposal); d_out int32 [budget]; d_stats int32 [stats_cap][3] = {drafted, draft ids
 * used, emitted} per step (NULL = none); source 0 = drafts by the n-gram rule (max_ngram 1..4), 1 = the step drafts
 * d_stream[w .. w + D) where w = its write index (tests, benchmarks).  L + 1 + budget + D <= max_ctx is required.  The decode-steps call
 * then runs verify steps (its d_out_ids argument is not written); enable = 0: the plain tail again.  tp_size > 1: unsupported.
 * The op-level calls run the pieces on caller-provided buffers: the draft rule for a history (-> d_draft [D], count in
 * d_ctl[VZ_SPEC_CTL_DRAFTED]); argmax + acceptance on logits [R, cols] with d_state = [cur | pos | slot | len] x R (d_stats [3]);
 * RoPE + append of R fresh QKV rows (pos / slot [R]) + the verify attention over cache row [Hkv][max_ctx][D] -> o [R, Hq, D]
 * (q_rot [R, Hq, D] scratch; ws from the part-floats call; ticket [Hkv] zeroed once; key_bound >= slot[0] + R keys, which fixes the
 * absolute split positions: nsplit x 128-key multiples).
 * A query's reduction order is a function of key positions only - and the output therefore bit-independent of the drafts - while a
 * split is exactly 128 keys, i.e. while the context bucket has no more 128-key chunks than splits (<= 32 with the default split limit:
 * max_ctx <= 4096).  Beyond that a split is a larger multiple of 128 that follows the host's worst-case bound, and results agree to
 * bf16 rounding only.
 * Sampled verify steps (HF: do_sample=True with prompt_lookup_num_tokens, `_assisted_decoding` without candidate logits): behind the
 * decode-spec call (enable = 1), vz_llm_decode_spec_sampling with a VZ_ROW_SAMPLE record replaces "argmax of row i" by "the draw of row
 * i": the record's temperature / top-k / top-p / warpers and seed, Philox stream-row word 0 and draw counter w + 1 + i, w =
 * d_ctl[VZ_SPEC_CTL_WRITE] - the index, in the generated sequence, of the token row i would emit (the caller drew token 0 from the
 * prefill logits with counter 0).  The ids are therefore a function of (seed, logits) only, not of the drafts.  The record's `counter`
 * field is IGNORED, whatever its value (it is not checked either): the control words carry the counter.  NULL or a VZ_ROW_GREEDY record: argmax verify; the decode-spec call (either
 * value of enable) and vz_llm_decode_begin clear the record.  The record is part of what a captured step freezes.
 * vz_op_spec_accept_sampled = vz_op_spec_accept with those draws in front instead of the argmax (they land in words 8..15). */
#define VZ_SPEC_CTL_WRITE 0
#define VZ_SPEC_CTL_HIST 1
#define VZ_SPEC_CTL_DONE 2
#define VZ_SPEC_CTL_DRAFTED 3
#define VZ_SPEC_CTL_STEPS 4
#define VZ_SPEC_CTL_IDS 8
#define VZ_SPEC_CTL_WORDS 16
int vz_llm_decode_spec(vz_engine* e, int enable, int D, int max_ngram, int* d_hist, int hist_len, int hist_cap, const int* h_eos, int n_eos,
                       int* d_out, int budget, int* d_ctl, int* d_stats, int stats_cap, int source, const int* d_stream, int stream_len,
                       vz_stream stream);
int vz_op_spec_draft(const int* d_hist, int hist_len, int D, int max_ngram, const int* h_eos, int n_eos, int* d_draft, int* d_ctl,
                     vz_stream stream);
int vz_op_spec_accept(const float* d_logits, int R, int cols, int* d_state, int* d_ctl, int* d_out, int budget, int* d_hist, int hist_cap,
                      const int* h_eos, int n_eos, int* d_stats, int max_ctx, int rope_max, vz_stream stream);
int vz_llm_decode_spec_sampling(vz_engine* e, const vz_sample_params* p);
int vz_op_spec_accept_sampled(const float* d_logits, int R, int cols, const vz_sample_params* p, int* d_state, int* d_ctl, int* d_out, int budget,
                              int* d_hist, int hist_cap, const int* h_eos, int n_eos, int* d_stats, int max_ctx, int rope_max, vz_stream stream);
long vz_op_spec_part_floats(int R, int Hkv, int nsplit);
int vz_op_attention_verify(const void* qkv, void* kc, void* vc, void* o, void* q_rot, float* ws, unsigned* ticket, const float* cosT,
                           const float* sinT, const int* pos, const int* slot, int R, int Hq, int Hkv, int D, int max_ctx, int nsplit,
                           int key_bound, int window, float scale, vz_stream stream);

/* ---- anyres preprocessing on the device (ref:vis_zephyr/model/multi_scale_process.py:70-171) ----
 * vz_op_resample_u8: Pillow's 8-bit LANCZOS `Image.resize` (horizontal pass, 8-bit intermediate, vertical pass) of an
 * [h, w, 3] u8 image to [h2, w2, 3], bit-exact.  bounds int32 [out, 2] = (first tap, tap count), coefs int32 [out, k] at 22
 * fractional bits, computed by the host as Pillow's precompute_coeffs / normalize_coeffs_8bpc do (vz_hip/preprocess.py).
 * d_tmp [h, w2, 3] is needed when both sizes change; equal sizes copy.
 * vz_op_anyres_tiles: the letterbox paste on black + row-major side x side crops + the global view in front + CLIP rescale /
 * normalise through a bf16 LUT [3, 256] -> bf16 [1 + grid_w * grid_h, 3, side, side], what the vision tower takes. */
int vz_op_resample_u8(const void* d_src, int h, int w, void* d_tmp, void* d_dst, int h2, int w2, const int* d_xbounds,
                      const int* d_xcoefs, int kx, const int* d_ybounds, const int* d_ycoefs, int ky, vz_stream stream);
int vz_op_anyres_tiles(const void* d_global, const void* d_resized, int nh, int nw, int paste_x, int paste_y, int grid_w,
                       int grid_h, int side, const void* d_lut, void* d_out, vz_stream stream);

/* ------------------------------------------------------------------------------------------
 * 3. Stage-1 pretrain step
 *
 * ref:vis_zephyr/train/train.py:817-829 freezes everything but `mm_projector`; the loss is HF's causal-LM cross-entropy of
 * ref:vis_zephyr/model/language_model/vis_zephyr.py:51-98 (shift by one, ignore_index -100, mean over the valid targets);
 * ref:vis_zephyr/train/vis_zephyr_trainer.py:224-302 + ref:script/pretrain.sh:39-42: AdamW on the projector parameters,
 * DeepSpeed ZeRO-2 data parallelism.  A trainer belongs to one finalized tp_size 1 engine and owns: W^T copies of the frozen
 * Zephyr linears, fp32 master / Adam moments / gradient arenas of the 165 projector tensors (engine names "qf.*", engine
 * layout - vz_hip/train.py maps them to the reference's parameter names), and an arena of saved activations + scratch.
 *   vz_train_stage1_accumulate  forward (activations kept) + backward of ONE micro-batch; gradients ACCUMULATE.  Stage inputs
 *       as the inference entry points take them (vz_clip_fused_features / vz_qformer / vz_embed_splice / vz_llm_prefill) plus
 *       d_vis_rows int32 [T*32] (row of [B*S] each visual token was spliced into, -1 = cut off), d_labels int32 [B,S] (HF
 *       labels; the shift happens inside) and inv_n = 1 / (valid targets of the whole batch).
 *   vz_train_loss_sum           sum over the rows of the last micro-batch of (logsumexp - target logit)  (blocking)
 *   vz_train_allreduce          RCCL all-reduce (ncclAvg: the mean over the data-parallel ranks of their mean-loss gradients, as
 *                               DeepSpeed / HF Trainer reduce them) of the flat gradient arena, 256 MiB buckets; no-op without vz_train_comm_init
 *   vz_train_adamw_step         torch.optim.AdamW (no amsgrad) on every projector tensor; rewrites the engine's working copies,
 *                               clears the gradients
 *   vz_train_ws_info            bytes of the activation + scratch arena, and the high-water mark of the last
 *                               vz_train_stage1_accumulate in it (equal when that call sized the arena; smaller after a smaller shape)
 * ------------------------------------------------------------------------------------------ */
typedef struct vz_trainer vz_trainer;
int vz_train_create(vz_engine* e, vz_trainer** out, vz_stream stream);
int vz_train_destroy(vz_trainer* t);
int vz_train_set_master(vz_trainer* t, const char* engine_name, const float* d_values, long n, vz_stream stream);
int vz_train_param_count(vz_trainer* t);
int vz_train_param_info(vz_trainer* t, int i, const char** name, long* n, long* offset, int* is_matrix);
int vz_train_arenas(vz_trainer* t, float** d_grad, float** d_master, float** d_m, float** d_v, long* total_floats);
int vz_train_stage1_accumulate(vz_trainer* t, const void* d_images, int T, const void* d_text, int n_samples, int Lmax,
                               const int* h_tile_sample, const int* d_kind, const int* d_idx, const int* d_vis_rows, int B, int S,
                               const int* h_seqlens, const int* d_pos, const int* d_labels, float inv_n, vz_stream stream);
int vz_train_loss_sum(vz_trainer* t, double* out, vz_stream stream);
int vz_train_zero_grad(vz_trainer* t, vz_stream stream);
int vz_train_comm_init(vz_trainer* t, const char* id128, int rank, int world);
int vz_train_allreduce(vz_trainer* t, vz_stream stream);
int vz_train_adamw_step(vz_trainer* t, float lr, float beta1, float beta2, float eps, float weight_decay, vz_stream stream);
int vz_train_ws_info(vz_trainer* t, size_t* arena_bytes, size_t* peak_bytes);

/* ------------------------------------------------------------------------------------------
 * 3b. Stage-2 LoRA finetune step (ref:script/finetune.sh; ref:vis_zephyr/train/train.py:224-243, 933-951)
 *
 * The Stage-1 trainer plus a peft LoRA branch on every decoder linear: y = W x + scaling * B (A dropout(x)), A [r, in],
 * B [out, r], scaling = alpha / r, an independent dropout mask per module.  The frozen weights and the inference engine stay
 * untouched; the branch exists inside the trainer only.  The projector stays trainable (one optimiser group with the factors).
 *   vz_train_lora_enable        adds 2 x 7 x n_layers tensors to the parameter table AFTER the projector tensors (Stage-1
 *       offsets and names unchanged), named "lora.{layer}.{q,k,v,o,gate,up,down}.{A,B}" (row-major A [r, in], B [out, r]),
 *       with fp32 master / moments / gradient in the same arenas (vz_train_arenas: the pointers change) and a bf16 working copy.
 *       Masters start at zero; vz_train_set_master on a LoRA tensor also rewrites its working copy.  r % 64 == 0, 0 <= dropout < 1.
 *       vz_train_zero_grad / vz_train_allreduce / vz_train_adamw_step cover the factors; vz_train_stage1_accumulate runs the branch.
 *   vz_train_lora_set_counter   dropout counter of the following micro-batches: Philox4x32-10, key = seed, counter = (column / 4,
 *       (sample_base + sample in micro-batch) * row_stride + position, layer * 7 + module, optimiser_step), word column % 4; an
 *       element is kept when the word >= floor(p * 2^32).  row_stride >= the micro-batch's S (the longest row of the optimiser
 *       batch keeps every mask independent of the micro-batch split).
 *   vz_op_lora_dropout          the dropout at op level: out = keep * x * scaling / (1 - p) (bf16), rows = B * S of one micro-batch.
 * ------------------------------------------------------------------------------------------ */
int vz_train_lora_enable(vz_trainer* t, int r, float alpha, float dropout, unsigned long long seed, vz_stream stream);
int vz_train_lora_set_counter(vz_trainer* t, int optimiser_step, long sample_base, long row_stride);
int vz_op_lora_dropout(const void* d_x, int ldx, void* d_out, int ldo, int rows, int cols, int S, long sample_base, long row_stride,
                       int tag, int step, unsigned long long seed, float p, float scaling, vz_stream stream);

/* ViP "point" overlay on the device (ref:vis_zephyr/model/vip_processor/conversation_generator.py:143-153,170-175: the
 * `vcr_qa` / `vcr_qar` visual prompt = `ImageDraw.ellipse(box, fill=rgba, outline=rgba)` on a transparent canvas +
 * `Image.alpha_composite` + convert("RGB")): composites one filled ellipse with the INTEGER box (x0, y0, x1, y1) - the
 * reference's float box truncated as Pillow's (int) cast does - and colour rgba (r | g << 8 | b << 16 | a << 24) onto the
 * u8 [h, w, 3] image in place, bit-exact with Pillow (oracle/vip_oracle.py).  Points of one image are applied in call order. */
int vz_op_vip_point(void* d_image_u8, int h, int w, int x0, int y0, int x1, int y1, unsigned rgba, vz_stream stream);

/* argmax over fp32 logits rows: ids int32 [rows] (first maximal index) */
int vz_op_argmax(const float* d_logits, int rows, int cols, int* d_ids, vz_stream stream);

/* A/B hook of the bench tools and the tests (process-wide).  A knob change takes effect on the next vz_llm_decode_steps, which captures
 * its graph again (also when the value set is the one the knob had).  A value outside the knob's range is refused with VZ_ERR_ARG.
 * Defaults and ranges are not repeated here: vz_tune_info enumerates the table (csrc/tune.h).  Knobs (number  name  meaning):
 *   0  gemv_variant          GEMV variant: 0 = production choice; 1..10 = alternatives compiled in (rows per wave, chunks in flight, non-temporal loads, waves per workgroup; tools/bench_kernels.py)
 *   1  gemm_choice           tile GEMM choice: 0 = by grid size; 1 = always 128^2; 2 = always 256^2
 *   2  attn_version          prefill attention generation: 1 = v1 kernel for every head_dim (tests / A-B); 2 = v2 (head_dim 64 / 128) with the classic online-softmax step; 3 = v2 with the deferred-maximum step (production)
 *   3  splitk_mode           split-K of M <= 512 linears: 0 = auto; 1 = never
 *   4  gemm256_streamk       256^2 GEMM stream-K tail: 1 = a last round that fills at most half of the CUs; 0 = whole tiles only; 2 = forced for any tail (tests)
 *   5  gemm256_skew          K-tiles by which even / odd stream-K workgroups lead / lag
 *   6  gemm256_stamps        record 256^2 GEMM phase stamps (vz_prof_gemm_stamps)
 *   7  force_comm            1 = route the collectives of a tp_size == 1 engine holding a one-rank communicator through RCCL (self-test); 2 = shape rehearsal of one rank of a tp_size > 1 engine, collectives skipped
 *   9  skinny_mode           2..64-row linears, SkinnyMode of linear_route.h: 1 = MFMA weight stream; 0 = GEMV / tile GEMM; 5 = ignore the tiled weight copies
 *  10  attn_nsplit           context splits of the fused decode attention: 0 = engine default
 *  11  gemm256_drain         256^2 GEMM workgroups wait for their stores before ending (experiment)
 *  14  decode_tile_rows      rows from which a decode step's linears take the 128^2 tile GEMM (65 = never)
 *  15  decode_sk_short       split-K factor of the K = 4096 decode projections (QKV, O) on that route
 *  16  attn_stamps           record stage stamps of the prefill attention kernel (vz_prof_attn_stamps)
 *  19  wide_mode             gemm_wide.hip for 17..64-row decode steps: 0 = off (they keep the earlier routes)
 *  21  fp8_gemm_choice       fp8 tile GEMM choice: 0 = by grid size; 1 = always the 128^2 kernel; 2 = always the 256^2 pipeline
 *  22  fp8_prefill_min_rows  fewest prefill rows that take the fp8 MFMA path of a prefill_fp8 engine
 *  23  attn_split            key split of few-row head_dim-512 attention: 0 = automatic (every 96 keys); 1 = never; n >= 2 = n splits
 *  24  splitk_cap            most K slices of a weight-streaming (M <= 512) linear; values outside 1..16 are clamped
 *  25  qf_kv_all             Q-Former cross-attention K|V projections of all blocks as one GEMM: 0 = one block at a time (A/B)
 *  26  splitk_mid            K slices for tile-GEMM grids that leave a CU one workgroup (M > 512, < 256 tiles): 0 = whole-K tiles (batch-invariant)
 *  27  wide_fp8_splits       K splits of the e4m3 17..64-row stream: 0 = by shape (A/B)
 *  28  persist_decode        batch-1 decode steps as ONE resident grid per token (decode_persist.hip) instead of the launch chain
 *  29  oneshot               one-shot all-reduce for the TP decode step when peer areas are attached: 0 = keep RCCL
 *  30  attn_o                batch-1 decode attention + O projection as one launch (attn_o_fused.hip): 0 = two launches
 *  31  attn_o_delay          that launch's O role waits n x ~0.21 us before requesting its weights, so that the attention blocks' K / V loads reach the memory system first
 *  32  flash_bwd             training step: tile-resident attention backward for head_dim 128; 0 = the materialising batched-GEMM route (A/B)
 *  33  rope_in_attn          prefill: RoPE of the queries inside the attention's Q load; 0 = a rotated copy of Q from rope_kv_kernel (bit-identical)
 *  34  gemm256_persist       256^2 GEMM: persistent whole-tile workgroups when a launch has more whole tiles than CUs; 0 = one workgroup per tile (bit-identical)
 *  35  skinny_even           3..16-row persistent weight stream: the same number of row groups on every workgroup; 0 = one workgroup per CU (bit-identical)
 *  36  append_flash_min_t    append prefill: more new rows per sample than this run on the prefill's flash kernel, fewer on the key-split kernel of attn_append.hip */
int vz_tune_set(int knob, int value);
/* the knob's current value */
int vz_tune_get(int knob, int* value);
/* entry `index` (0, 1, ...) of the knob table: number, name (static storage), default, lowest and highest accepted value.  VZ_ERR_ARG past
 * the last entry. */
int vz_tune_info(int index, int* knob, const char** name, int* dflt, int* lo, int* hi);

/* per-kernel-class timing of the engine's launches with HIP events on the launch stream (bench.py's roofline
 * leg).  enable=1 disables graph replay and brackets every launch of class `klass` with events.
 * classes: 0 gemm(mfma) 1 gemv 2 attention 3 attn_decode 4 norm 5 other 6 fused attention half 7 RCCL collectives */
int vz_prof_enable(vz_engine* e, int enable, int klass);
/* synchronises the events; returns launches counted and their total milliseconds */
int vz_prof_read(vz_engine* e, long* n_launches, double* total_ms);
/* in-kernel phase stamps (s_memrealtime, 100 MHz) of the last 256^2 GEMM launched with vz_tune_set(6, 1):
 * 16 int64 per workgroup = {start, then per K-slice: loop begin, loop end, fix-up end, epilogue end, (nk<<32 | flags)} */
int vz_prof_gemm_stamps(long long* host_out, int max_wgs, int* n_wgs);
/* stage cycle counts (s_memtime) of one wave of the prefill attention kernel, last launch with vz_tune_set(16, 1): the longest
 * causal workgroup's wave 0 - [issue K/V loads, QK^T, softmax, PV, wait, barrier, -, loop top, tiles] (16 int64), followed by 2048 x 4 int64
 * of per-workgroup schedule: start, end (s_memrealtime, 100 MHz), XCC id << 32 | HW_ID, query block << 32 | tiles.  host buffer: 16 + 8192 int64 */
int vz_prof_attn_stamps(long long* host16);

/* ---- beam search: processors and rows (csrc/beam.hip, csrc/logits_proc.hip) ----
 * vz_llm_decode_logits_proc may be armed together with vz_llm_decode_beam.  HF's `_beam_search` hands the processors the
 * log-softmax row of every running beam and that beam's own ids, so a beam step then runs: log-prob rows in place (the reductions
 * and the fp32 association of the fused select), the processor kernel on them, the select on the rows as they are (s_i = row_i +
 * score[row]), the KV reorder, the reorder of the id histories (a row whose parent is another row takes its parent's history,
 * length included; the processor kernel appends the row's own token at the next step), the history index.  Without processors and
 * without recorded score rows the step is the fused select on the logits, launch for launch.  Log-prob rows followed by the select on
 * rows give the records and next beams of the fused select bit for bit.  The first step runs at op level on the prefill logits:
 * vz_op_beam_logprob_rows, vz_op_logits_process with empty histories, vz_op_beam_select_rows with nb_in = 1.
 * vz_op_beam_logprob_rows: d_lp [rows][cols] = (x - max) - log(sum exp(x - max)) of fp32 logits; d_lp may be d_logits.
 * vz_op_beam_select_rows: vz_op_beam_select on rows that hold scores already (no normalisation).
 * vz_op_hist_beam_reorder: groups x nb (<= 16) histories d_hist [groups * nb][hist_stride] of d_hist_len[row] ids follow d_parent
 *   [groups * nb] (local beam indices), in place; cycles and parents with several children are safe.
 * vz_llm_decode_beam_rows: the beam step also copies its processed log-prob rows (HF's scores[t]) into d_scores and / or its raw logits
 *   rows into d_raw, rings fp32 [cap_steps][groups * nb][vocab] written at (history index of vz_llm_decode_beam) mod cap_steps, inside
 *   the per-token hipGraph (the rings are part of what a captured step freezes); vz_llm_decode_steps refuses n > cap_steps.  Both
 *   NULL: off, nothing is added to the step.  Tensor-parallel engines: VZ_ERR_UNSUPPORTED. */
int vz_op_beam_logprob_rows(const float* d_logits, int rows, int cols, float* d_lp, vz_stream stream);
int vz_op_beam_select_rows(const float* d_rows, int rows, int cols, int nb_in, int nb_out, const int* h_eos, int n_eos,
                           const float* d_scores_in, int* d_records, int* d_next_tok, float* d_next_score, int* d_next_parent,
                           vz_stream stream);
int vz_op_hist_beam_reorder(int* d_hist_len, int* d_hist, int hist_stride, int nb, int groups, const int* d_parent, vz_stream stream);
int vz_llm_decode_beam_rows(vz_engine* e, float* d_scores, float* d_raw, int cap_steps);

/* ---- classifier-free guidance (csrc/guidance.hip) ----
 * hf:generation/logits_process.py UnbatchedClassifierFreeGuidanceLogitsProcessor, the first processor of HF's chain, with the two
 * branches as two rows of one weight sweep.
 * vz_llm_decode_guidance(enable=1, scale, pairs): from the next vz_llm_decode_begin on a decode batch is B = 2 * pairs rows: row r <
 *   pairs is a prompt (the conditional branch), row pairs + r its negative prompt (the unconditional branch, with its own cache row).
 *   Every step runs the model on all B rows; behind the logits, inside the per-token hipGraph: the raw-row recorder, then row r <-
 *   scale * (lc - lu) + lu with lc / lu = log_softmax of row r / row pairs + r in fp32, then the logits processors, the tail (argmax,
 *   sampler or per-row table), the step recorder and the stop matcher on the first `pairs` rows exactly as on a `pairs`-row batch, then
 *   row pairs + r takes the token row r chose and its position / slot / length move on.  d_out_ids of vz_llm_decode_steps is
 *   [pairs][n]; the token ring, the recorder's rings, the matcher's rows and the per-row table describe `pairs` rows.  The
 *   unconditional rows are never recorded.  scale: any finite float (1 changes nothing but costs the step; callers pass enable=0).
 *   vz_llm_decode_steps: VZ_ERR_ARG unless the batch has exactly 2 * pairs rows, VZ_ERR_UNSUPPORTED together with the beam or the
 *   speculative tail.  Tensor-parallel engines: VZ_ERR_UNSUPPORTED.  scale and pairs are part of what a captured step freezes.
 *   enable=0: off - the step is launch for launch what it is without this entry.
 * vz_op_cfg_combine: the same kernel in place on d_logits_cond [pairs][cols] against d_logits_uncond [pairs][cols] (fp32, not
 *   overlapping; only read).  Precondition: the unconditional rows are finite.  -inf in a conditional row stays -inf (scale > 0).
 *   Two calls on equal inputs give equal bits. */
int vz_llm_decode_guidance(vz_engine* e, int enable, float scale, int pairs, vz_stream stream);
int vz_op_cfg_combine(float* d_logits_cond, const float* d_logits_uncond, int pairs, int cols, float scale, vz_stream stream);

/* ---- shared-prefix decode attention (csrc/attn_shared.hip) ----
 * n samples of one prompt read the prompt's K / V once.  Rows come in groups of n adjacent rows, group g = rows g*n .. g*n + n - 1;
 * d_shared[g] (int32, device) leading cache slots of the group live in cache row g*n only.  Row r sees the slots [0, shared[g]) of cache
 * row g*n and the slots [shared[g], slot[r]] of its own row, slot[r] being the slot of the token just appended (window > 0: only the
 * slots > slot[r] - window of that union); a row with slot[r] < shared[g] shares nothing and sees its own slots [0, slot[r]].  No other
 * slot is read.
 * vz_op_attention_shared: d_q_rot rotated bf16 [R][Hq][128], caches [rows >= R][Hkv][max_ctx][128], d_o bf16 [R][Hq][128], d_slot int32 [R].
 *   Two launches: one stacked pass per (group, KV head) over the shared slots, split over nsplit workgroups along the keys (0 = chosen
 *   from shared_max = max_g shared[g], given on the host, 1 <= shared_max <= max_ctx; >= 1 forced, cut to the 64-key tiles of shared_max
 *   and to 64), which leaves fp32 partials in the workspace; then one workgroup per (row, KV head) for the row's own slots and the merge.
 *   2 <= n <= 64, R a multiple of n, head_dim 128.  The workspace needs R * Hq * nsplit * 132 floats;
 *   vz_op_attention_shared_ws_floats(R, n, Hq, Hkv, max_ctx) covers every split the rule can choose for shared_max <= max_ctx (pure host
 *   arithmetic; 0 = a shape the op refuses).
 * vz_llm_decode_share(n, h_shared[groups], groups): arms the NEXT decode batch (vz_llm_decode_begin) as groups x n rows whose attention
 *   is the op above behind the stand-alone RoPE + append launch, for every tail but the speculative one; n = 0 disarms.  2 <= n <= 64,
 *   groups * n <= min(max_batch, 64), 1 <= h_shared[g] <= max_ctx; VZ_ERR_UNSUPPORTED on a tensor-parallel engine.  While armed:
 *   vz_llm_decode_begin with another row count, vz_llm_decode_set_row to a context shorter than the group's shared slots (parking
 *   included), vz_llm_kv_move_rows into a group's first row, and vz_llm_decode_steps with guidance, the speculative tail or the persistent
 *   token kernel are refused.  n, the split and the table's address are part of what a captured step freezes.  With nothing armed the
 *   step is launch for launch what it is without this entry. */
int vz_op_attention_shared(const void* d_q_rot, const void* d_kcache, const void* d_vcache, void* d_o, const int* d_shared, const int* d_slot,
                           int R, int n, int Hq, int Hkv, int head_dim, int max_ctx, int shared_max, float scale, int window, int nsplit,
                           float* d_workspace, long workspace_floats, vz_stream stream);
long vz_op_attention_shared_ws_floats(int R, int n, int Hq, int Hkv, int max_ctx);
int vz_llm_decode_share(vz_engine* e, int n, const int* h_shared, int groups, vz_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VISZEPHYR_H */
