// libviszephyr_hip.so - C ABI (include/viszephyr.h) and the stage engine of the Vision-Zephyr
// forward/generate path on gfx950.  The engine owns workspace + KV cache and sequences the
// hand-written kernels of one stage on the caller's HIP stream:
//
//   vz_clip_fused_features  a8-a10  ref:vis_zephyr/model/vision_encoder/vision_encoder.py:58-117
//   vz_qformer              a11     ref:vis_zephyr/model/multimodal_projector/builder.py:34-92
//   vz_embed_splice         a6/a7   ref:vis_zephyr/model/vis_zephyr_arch.py:236-305,476-530
//   vz_llm_prefill          a12     hf:models/mistral/modeling_mistral.py:202-241,340-466
//   vz_llm_decode_*         a13     hf:generation/utils.py greedy branch, one hipGraph replay per token
//
// Q-Former block 0 (ref builder.py:80-87) keeps only the first 32 rows of a block that ran on
// [32 queries ; L text tokens].  Those rows depend on the other rows only through the self-attention
// keys/values, and both the query rows and the text rows are identical for every tile of a sample,
// so the engine computes block 0's self-attention once per SAMPLE for the 32 query rows (K/V over
// all 32+L rows) and runs cross-attention/FFN per tile on 32 rows - identical results, without the
// rows the reference computes and throws away.
#include <algorithm>
#include <stdarg.h>
#include <stdlib.h>

#include "engine_internal.h"

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
thread_local hipEvent_t g_vz_prof_start = nullptr, g_vz_prof_stop = nullptr;
static thread_local char g_err[1024] = "";
void vz_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* vz_last_error(void) { return g_err; }
extern "C" int vz_abi_version(void) { return 12; }
extern "C" const char* vz_target_arch(void) { return "gfx950"; }

// ------------------------------------------------------------------------------------------------
// operator entry points
// ------------------------------------------------------------------------------------------------
static LinearArgs mk_linear(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                            const float* bias, const void* residual, int ldr, int act, int out_fp32) {
    LinearArgs a;
    a.A = (const bf16_t*)A; a.lda = lda; a.W = (const bf16_t*)W; a.ldw = ldw; a.C = C; a.ldc = ldc;
    a.M = M; a.N = N; a.K = K; a.bias = bias; a.residual = (const bf16_t*)residual; a.ldr = ldr;
    a.act = act; a.out_fp32 = out_fp32; a.norm_w = nullptr; a.norm_eps = 0.f; a.err = nullptr;
    return a;
}


// The op-level linear entry points: each names the kernels it exists for as the routes it admits (include/viszephyr.h: VZ_LINEAR_*); the
// route itself is the planner's.  vz_op_linear_route asks the same function, so what it reports is what the entry point runs.
static int op_plan(int entry, const LinearArgs& a, bool decode, LinPlan* p) {
    const unsigned skinny = lin_bit(LIN_SKINNY) | lin_bit(LIN_SKINNY_PERSIST) | lin_bit(LIN_SKINNY_WIDE);
    const int M = a.M, N = a.N, K = a.K;
    switch (entry) {
    case VZ_LINEAR_ENGINE:          // an engine's own call (route query only): its norm scratch has the linear's K columns
        *p = vz_plan_linear(a, LinCaller{decode ? LIN_ROWS_DECODE : LIN_ROWS_COUPLED, K});
        return VZ_OK;
    case VZ_LINEAR_OP:              // vz_op_linear, vz_op_linear_fp8: 1 row: GEMV; 2..64 rows: MFMA weight stream (gemm_skinny.hip); tile GEMMs beyond
        *p = vz_plan_linear(a, LinCaller{LIN_ROWS_FREE});
        return VZ_OK;
    case VZ_LINEAR_RMSNORM:
        VZ_CHECK_ARG(a.norm_w && M >= 1 && M <= 16, "linear_rmsnorm: needs norm weights and 1 <= M <= 16 (the fused norm lives on the <= 16-row weight-stream kernels)");
        *p = vz_plan_linear(a, LinCaller{LIN_ROWS_FREE, 0, lin_bit(LIN_GEMV) | skinny});
        VZ_CHECK_ARG(p->route != LIN_NONE, "linear_rmsnorm: shape M=%d K=%d not supported by the weight-stream kernels", M, K);
        return VZ_OK;
    case VZ_LINEAR_TILED:           // 17..64 rows: gemm_wide.hip; else the MFMA weight stream on the tiled copy
        VZ_CHECK_ARG(a.Wt && a.ldw == K && (N & 15) == 0, "linear_tiled: needs the tiled copy of a dense [N, K] weight with N %% 16 == 0");
        *p = vz_plan_linear(a, LinCaller{LIN_ROWS_FREE, 0, lin_bit(LIN_WIDE_BF16) | skinny});
        VZ_CHECK_ARG(p->route != LIN_NONE, "linear_tiled: the MFMA weight stream takes 2 <= M <= 64 (fused norm: <= 16), K %% 64 == 0 (M=%d K=%d)", M, K);
        return VZ_OK;
    case VZ_LINEAR_TILED_FP8:
        VZ_CHECK_ARG(a.W8t && a.wscale && (N & 127) == 0, "linear_tiled_fp8: needs the tiled e4m3 copy + row scales of a dense [N, K] weight with N %% 128 == 0");
        *p = vz_plan_linear(a, LinCaller{LIN_ROWS_FREE, 0, lin_bit(LIN_WIDE_E4M3)});
        VZ_CHECK_ARG(p->route != LIN_NONE, "linear_tiled_fp8: needs 17 <= M <= 64, K %% 1024 == 0 (M=%d N=%d K=%d)", M, N, K);
        return VZ_OK;
    // vz_op_linear_impl: the route is forced, the launcher checks what it can take
    case VZ_LINEAR_IMPL + 0: *p = vz_plan_forced(LIN_TILE128, a, false); return VZ_OK;
    case VZ_LINEAR_IMPL + 1: *p = vz_plan_forced(LIN_GEMV, a, false); return VZ_OK;
    case VZ_LINEAR_IMPL + 2: *p = vz_plan_forced(LIN_TILE256, a, false); return VZ_OK;
    case VZ_LINEAR_IMPL + 3: *p = vz_plan_forced(LIN_SKINNY, a, false); return VZ_OK;
    case VZ_LINEAR_IMPL + 4: *p = vz_plan_forced(LIN_TILE128, a, true); return VZ_OK;       // the 29..64-row decode route
    }
    vz_set_error("linear: unknown entry point %d", entry);
    return VZ_ERR_ARG;
}
static int op_linear(int entry, const LinearArgs& a, vz_stream s) {
    LinPlan p;
    const int r = op_plan(entry, a, false, &p);
    return r ? r : vz_run_linear(p, a, nullptr, (hipStream_t)s);
}

extern "C" int vz_op_linear(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                            const float* bias, const void* residual, int ldr, int act, int out_fp32, vz_stream s) {
    return op_linear(VZ_LINEAR_OP, mk_linear(A, lda, W, ldw, C, ldc, M, N, K, bias, residual, ldr, act, out_fp32), s);
}
extern "C" int vz_op_linear_fp8(const void* A, int lda, const void* W8, int ldw, const float* wscale, void* C, int ldc, int M, int N,
                                int K, const float* bias, const void* residual, int ldr, int act, int out_fp32,
                                const float* norm_w, float norm_eps, vz_stream s) {
    VZ_CHECK_ARG(W8 && wscale, "linear_fp8: null weights / scales");
    LinearArgs a = mk_linear(A, lda, (const void*)W8, ldw, C, ldc, M, N, K, bias, residual, ldr, act, out_fp32);
    a.W8 = (const unsigned char*)W8; a.wscale = wscale; a.norm_w = norm_w; a.norm_eps = norm_eps;
    return op_linear(VZ_LINEAR_OP, a, s);
}
extern "C" int vz_op_rmsnorm_quant_fp8(const void* x, int ldx, const float* w, float eps, void* q, int ldq, float* scale, int rows, int cols, vz_stream s) {
    return vz_launch_rmsnorm_quant_fp8((const bf16_t*)x, ldx, w, eps, (unsigned char*)q, ldq, scale, rows, cols, (hipStream_t)s);
}
extern "C" int vz_op_quant_rows_fp8(const void* x, int ldx, void* q, int ldq, float* scale, int rows, int K, vz_stream s) {
    return vz_launch_quant_rows_fp8((const bf16_t*)x, ldx, (unsigned char*)q, ldq, scale, rows, K, (hipStream_t)s);
}
extern "C" int vz_op_linear_fp8_mfma(const void* A8, int lda, const float* ascale, const void* W8, int ldw, const float* wscale, void* C, int ldc,
                                     int M, int N, int K, const float* bias, const void* residual, int ldr, int act, int out_fp32, vz_stream s) {
    Fp8LinearArgs a;
    a.A8 = (const unsigned char*)A8; a.lda = lda; a.ascale = ascale; a.W8 = (const unsigned char*)W8; a.ldw = ldw; a.wscale = wscale;
    a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K; a.bias = bias; a.residual = (const bf16_t*)residual; a.ldr = ldr; a.act = act; a.out_fp32 = out_fp32;
    return vz_launch_gemm_fp8(a, (hipStream_t)s);
}
extern "C" int vz_op_linear_rmsnorm(const void* A, int lda, const float* norm_w, float norm_eps, const void* W, int ldw, void* C, int ldc,
                                    int M, int N, int K, const void* residual, int ldr, int act, int out_fp32, vz_stream s) {
    LinearArgs a = mk_linear(A, lda, W, ldw, C, ldc, M, N, K, nullptr, residual, ldr, act, out_fp32);
    a.norm_w = norm_w; a.norm_eps = norm_eps;
    return op_linear(VZ_LINEAR_RMSNORM, a, s);
}
extern "C" int vz_op_tile_weights(const void* W, int N, int K, int ldw, void* Wt, vz_stream s) {
    return vz_launch_tile_weights((const bf16_t*)W, N, K, ldw, (bf16_t*)Wt, (hipStream_t)s);
}
extern "C" int vz_op_linear_tiled(const void* A, int lda, const void* W, const void* Wt, int ldw, void* C, int ldc, int M, int N, int K,
                                  const float* bias, const void* residual, int ldr, int act, int out_fp32, const float* norm_w,
                                  float norm_eps, vz_stream s) {
    LinearArgs a = mk_linear(A, lda, W, ldw, C, ldc, M, N, K, bias, residual, ldr, act, out_fp32);
    a.Wt = (const bf16_t*)Wt; a.norm_w = norm_w; a.norm_eps = norm_eps;
    return op_linear(VZ_LINEAR_TILED, a, s);
}
extern "C" int vz_op_tile_weights_fp8(const void* W8, int N, int K, int ldw, void* W8t, vz_stream s) {
    return vz_launch_tile_weights_fp8((const unsigned char*)W8, N, K, ldw, (unsigned char*)W8t, (hipStream_t)s);
}
// 17..64 rows on the e4m3 fragment-tiled copy (gemm_wide.hip's W8A16 stream): C = epi((A . dequant(W8)^T)), bf16 activations
extern "C" int vz_op_linear_tiled_fp8(const void* A, int lda, const void* W8t, const float* wscale, void* C, int ldc, int M, int N, int K,
                                      const float* bias, const void* residual, int ldr, int act, int out_fp32, vz_stream s) {
    LinearArgs a = mk_linear(A, lda, W8t, K, C, ldc, M, N, K, bias, residual, ldr, act, out_fp32);      // (W is unused on this route: any aligned pointer)
    a.W8t = (const unsigned char*)W8t; a.wscale = wscale;
    return op_linear(VZ_LINEAR_TILED_FP8, a, s);
}
extern "C" int vz_op_linear_impl(int impl, const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N,
                                 int K, const float* bias, const void* residual, int ldr, int act, int out_fp32,
                                 vz_stream s) {
    VZ_CHECK_ARG(impl >= 0 && impl <= 4, "linear: unknown impl %d", impl);
    return op_linear(VZ_LINEAR_IMPL + impl, mk_linear(A, lda, W, ldw, C, ldc, M, N, K, bias, residual, ldr, act, out_fp32), s);
}
// Which kernel family a linear of this shape runs on (LinRoute of csrc/linear_route.h; -1 = none): `flags` say which copies of W exist and
// what is fused (VZ_ROUTE_*), `entry` whose call it is (VZ_LINEAR_*).  Pointers count as aligned, ldc = the output width.  Touches no device.
extern "C" int vz_op_linear_route(int M, int N, int K, int lda, int ldw, int act, int out_fp32, unsigned flags, int entry,
                                  int* pre_norm, int* splitk_hint) {
    alignas(16) static const float some[4] = {0.f, 0.f, 0.f, 0.f};       // stands for every pointer that exists: nothing is read
    const int n_out = act == VZ_ACT_SWIGLU ? N / 2 : N;
    LinearArgs a = mk_linear(some, lda, some, ldw, (void*)some, n_out, M, N, K, (flags & VZ_ROUTE_BIAS) ? some : nullptr,
                             (flags & VZ_ROUTE_RESIDUAL) ? some : nullptr, n_out, act, out_fp32);
    if (flags & VZ_ROUTE_WT) a.Wt = (const bf16_t*)some;
    if (flags & VZ_ROUTE_W8) a.W8 = (const unsigned char*)some;
    if (flags & VZ_ROUTE_W8T) a.W8t = (const unsigned char*)some;
    if (flags & (VZ_ROUTE_W8 | VZ_ROUTE_W8T)) a.wscale = some;
    if (flags & VZ_ROUTE_NORM) { a.norm_w = some; a.norm_eps = 1e-5f; }
    LinPlan p;
    const std::string err = g_err;          // a query reports through its result: the checks it shares with the launches leave no message behind
    const bool none = vz_linear_check_common(a) || op_plan(entry, a, (flags & VZ_ROUTE_DECODE) != 0, &p) || !vz_route_takes(p, a);
    vz_set_error("%s", err.c_str());
    if (none) return LIN_NONE;
    if (pre_norm) *pre_norm = p.pre_norm;
    if (splitk_hint) *splitk_hint = p.splitk_hint;
    return p.route;
}
extern "C" int vz_op_causal_lm_loss(const float* logits, int B, int S, int V, const int* labels, float* loss_rows, float* out, vz_stream s) {
    return vz_launch_causal_lm_loss(logits, B, S, V, labels, loss_rows, out, (hipStream_t)s);
}
extern "C" int vz_op_layernorm(const void* x, int ldx, void* y, int ldy, const float* w, const float* b, int rows, int cols,
                               float eps, vz_stream s) {
    return vz_launch_layernorm((const bf16_t*)x, ldx, (bf16_t*)y, ldy, w, b, rows, cols, eps, (hipStream_t)s);
}
extern "C" int vz_op_rmsnorm(const void* x, int ldx, void* y, int ldy, const float* w, int rows, int cols, float eps,
                             vz_stream s) {
    return vz_launch_rmsnorm((const bf16_t*)x, ldx, (bf16_t*)y, ldy, w, rows, cols, eps, (hipStream_t)s);
}
extern "C" int vz_op_attention(const void* q, const void* k, const void* v, void* o, int B, int Sq, int Sk, int Hq, int Hkv,
                               int head_dim, long q_bs, long q_ss, long q_hs, long k_bs, long k_ss, long k_hs, long v_bs,
                               long v_ss, long v_hs, long o_bs, long o_ss, long o_hs, float scale, int causal, int q_pos0,
                               int window, const int* kv_len, vz_stream s) {
    // one fill for both forms: without a workspace the launcher never splits
    return vz_op_attention_split(q, k, v, o, B, Sq, Sk, Hq, Hkv, head_dim, q_bs, q_ss, q_hs, k_bs, k_ss, k_hs, v_bs, v_ss, v_hs, o_bs, o_ss, o_hs, scale,
                                 causal, q_pos0, window, kv_len, nullptr, 0, s);
}
extern "C" int vz_op_attention_split(const void* q, const void* k, const void* v, void* o, int B, int Sq, int Sk, int Hq, int Hkv,
                                     int head_dim, long q_bs, long q_ss, long q_hs, long k_bs, long k_ss, long k_hs, long v_bs,
                                     long v_ss, long v_hs, long o_bs, long o_ss, long o_hs, float scale, int causal, int q_pos0,
                                     int window, const int* kv_len, float* ws, long ws_floats, vz_stream s) {
    VZ_CHECK_ARG(ws_floats >= 0 && (ws || ws_floats == 0) && ((uintptr_t)ws & 15) == 0, "attention_split: bad workspace");
    AttnArgs a;
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.o = (bf16_t*)o;
    a.B = B; a.Sq = Sq; a.Sk = Sk; a.Hq = Hq; a.Hkv = Hkv; a.head_dim = head_dim;
    a.q_bs = q_bs; a.q_ss = q_ss; a.q_hs = q_hs; a.k_bs = k_bs; a.k_ss = k_ss; a.k_hs = k_hs;
    a.v_bs = v_bs; a.v_ss = v_ss; a.v_hs = v_hs; a.o_bs = o_bs; a.o_ss = o_ss; a.o_hs = o_hs;
    a.scale = scale; a.causal = causal; a.q_pos0 = q_pos0; a.window = window; a.kv_len = kv_len;
    a.part = ws; a.part_floats = (size_t)ws_floats;
    return vz_launch_attention(a, (hipStream_t)s);
}
extern "C" int vz_op_attention_append(const void* q, const void* kc, const void* vc, void* o, const int* d_past, const int* d_new, int B, int T,
                                      int Hq, int Hkv, int head_dim, int max_ctx, int kv_max, long q_bs, long q_ss, long q_hs, long o_bs,
                                      long o_ss, long o_hs, float scale, int window, int nsplit, float* ws, long ws_floats, vz_stream s) {
    VZ_CHECK_ARG(ws_floats >= 0 && (ws || ws_floats == 0), "attention_append: bad workspace");
    AttnAppendArgs a;
    a.q = (const bf16_t*)q; a.kc = (const bf16_t*)kc; a.vc = (const bf16_t*)vc; a.o = (bf16_t*)o; a.part = ws; a.part_floats = (size_t)ws_floats;
    a.past = d_past; a.nnew = d_new;
    a.B = B; a.T = T; a.Hq = Hq; a.Hkv = Hkv; a.head_dim = head_dim; a.max_ctx = max_ctx; a.window = window; a.kv_max = kv_max; a.nsplit = nsplit;
    a.q_bs = q_bs; a.q_ss = q_ss; a.q_hs = q_hs; a.o_bs = o_bs; a.o_ss = o_ss; a.o_hs = o_hs; a.scale = scale;
    return vz_launch_attention_append(a, (hipStream_t)s);
}
extern "C" long vz_op_attention_append_ws_floats(int B, int T, int Hq, int Hkv, int max_ctx) {
    return (long)vz_attn_append_ws_floats(B, T, Hq, Hkv, max_ctx);
}
extern "C" int vz_op_attention_shared(const void* q, const void* kc, const void* vc, void* o, const int* d_shared, const int* d_slot, int R, int n,
                                      int Hq, int Hkv, int head_dim, int max_ctx, int shared_max, float scale, int window, int nsplit, float* ws,
                                      long ws_floats, vz_stream s) {
    VZ_CHECK_ARG(ws && ws_floats > 0, "attention_shared: bad workspace");
    AttnSharedArgs a;
    a.q = (const bf16_t*)q; a.kc = (const bf16_t*)kc; a.vc = (const bf16_t*)vc; a.o = (bf16_t*)o; a.part = ws; a.part_floats = (size_t)ws_floats;
    a.shared = d_shared; a.slot = d_slot;
    a.R = R; a.n = n; a.Hq = Hq; a.Hkv = Hkv; a.head_dim = head_dim; a.max_ctx = max_ctx; a.window = window; a.shared_max = shared_max; a.nsplit = nsplit;
    a.scale = scale;
    return vz_launch_attention_shared(a, (hipStream_t)s);
}
extern "C" long vz_op_attention_shared_ws_floats(int R, int n, int Hq, int Hkv, int max_ctx) {
    return (long)vz_attn_shared_ws_floats(R, n, Hq, Hkv, max_ctx);
}
// two helpers of the training step at op level (parity tests): dst[c][r] = src[r][c], and out[c] += sum_r y[r][c] through `part`
extern "C" int vz_op_transpose(const void* src, long src_ld, void* dst, long dst_ld, int R, int C, vz_stream s) {
    return vz_launch_transpose((const bf16_t*)src, src_ld, 0, 0, (bf16_t*)dst, dst_ld, 0, 0, R, C, 1, 1, 0, (hipStream_t)s);
}
extern "C" int vz_op_colsum(const void* y, int ld, long rows, int cols, float* part, long part_floats, float* out, vz_stream s) {
    VZ_CHECK_ARG(part_floats >= (long)vz_colsum_groups(rows) * cols, "colsum: scratch of %ld floats, need %ld", part_floats, (long)vz_colsum_groups(rows) * cols);
    return vz_launch_colsum((const bf16_t*)y, ld, rows, cols, part, out, (hipStream_t)s);
}
extern "C" int vz_op_colsum_groups(long rows) { return vz_colsum_groups(rows); }
// the remaining kernels of train.hip at op level (parity tests, tests/test_train_ops_gpu.py): thin casts, every check is the launcher's
extern "C" int vz_op_transpose_batched(const void* src, long src_rs, long src_so, long src_si, void* dst, long dst_rs, long dst_so, long dst_si, int R,
                                       int C, int n_outer, int n_inner, int col0, vz_stream s) {
    return vz_launch_transpose((const bf16_t*)src, src_rs, src_so, src_si, (bf16_t*)dst, dst_rs, dst_so, dst_si, R, C, n_outer, n_inner, col0, (hipStream_t)s);
}
extern "C" int vz_op_softmax_fwd(const float* S, int lds, void* P, int ldp, long rows, int H, int Sq, int Sk, float scale, int causal, int window,
                                 const int* kv_len, vz_stream s) {
    return vz_launch_softmax_fwd(S, lds, (bf16_t*)P, ldp, rows, H, Sq, Sk, scale, causal, window, kv_len, (hipStream_t)s);
}
extern "C" int vz_op_softmax_bwd(const void* P, int ldp, const float* dP, int lddp, void* dS, int ldds, long rows, int Sk, float scale, vz_stream s) {
    return vz_launch_softmax_bwd((const bf16_t*)P, ldp, dP, lddp, (bf16_t*)dS, ldds, rows, Sk, scale, (hipStream_t)s);
}
extern "C" int vz_op_rmsnorm_bwd(const void* x, const float* w, const void* dy, const void* dres, void* dx, long rows, int cols, float eps, vz_stream s) {
    return vz_launch_rmsnorm_bwd((const bf16_t*)x, w, (const bf16_t*)dy, (const bf16_t*)dres, (bf16_t*)dx, rows, cols, eps, (hipStream_t)s);
}
extern "C" long vz_op_layernorm_bwd_scratch_floats(long rows, int cols) {
    return rows > 0 && cols > 0 ? (long)vz_layernorm_bwd_scratch_floats(rows, cols) : 0;
}
extern "C" int vz_op_layernorm_bwd(const void* x, const float* w, const void* dy, const void* dres, void* dx, float* part, long part_floats, float* dw,
                                   float* db, long rows, int cols, float eps, vz_stream s) {
    VZ_CHECK_ARG(rows > 0 && cols > 0 && part_floats >= (long)vz_layernorm_bwd_scratch_floats(rows, cols), "layernorm_bwd: scratch of %ld floats is too small",
                 part_floats);
    return vz_launch_layernorm_bwd((const bf16_t*)x, w, (const bf16_t*)dy, (const bf16_t*)dres, (bf16_t*)dx, part, dw, db, rows, cols, eps, (hipStream_t)s);
}
extern "C" int vz_op_gelu_fwd(const void* h, void* y, long n, vz_stream s) { return vz_launch_gelu_fwd((const bf16_t*)h, (bf16_t*)y, n, (hipStream_t)s); }
extern "C" int vz_op_gelu_bwd(const void* h, const void* dy, void* dh, long n, vz_stream s) {
    return vz_launch_gelu_bwd((const bf16_t*)h, (const bf16_t*)dy, (bf16_t*)dh, n, (hipStream_t)s);
}
extern "C" int vz_op_swiglu_fwd(const void* gu, void* act, long rows, int I, vz_stream s) {
    return vz_launch_swiglu_fwd((const bf16_t*)gu, (bf16_t*)act, rows, I, (hipStream_t)s);
}
extern "C" int vz_op_swiglu_bwd(const void* gu, const void* dact, void* dgu, long rows, int I, vz_stream s) {
    return vz_launch_swiglu_bwd((const bf16_t*)gu, (const bf16_t*)dact, (bf16_t*)dgu, rows, I, (hipStream_t)s);
}
extern "C" int vz_op_rope_bwd_assemble(const void* dq, const float* dk, const float* dv, void* dqkv, const float* cosT, const float* sinT, const int* pos,
                                       int B, int S, int Hq, int Hkv, int head_dim, int Sk_ld, vz_stream s) {
    return vz_launch_rope_bwd_assemble((const bf16_t*)dq, dk, dv, (bf16_t*)dqkv, cosT, sinT, pos, B, S, Hq, Hkv, head_dim, Sk_ld, (hipStream_t)s);
}
extern "C" int vz_op_cross_entropy(const float* logits, int V, const int* labels, long rows, int S, float inv_n, float* loss_rows, void* dlogits, int ldd,
                                   vz_stream s) {
    return vz_launch_cross_entropy(logits, V, labels, rows, S, inv_n, loss_rows, (bf16_t*)dlogits, ldd, (hipStream_t)s);
}
extern "C" int vz_op_gather_rows_idx(const void* src, const int* idx, void* dst, long rows, int cols, vz_stream s) {
    return vz_launch_gather_rows_idx((const bf16_t*)src, idx, (bf16_t*)dst, rows, cols, (hipStream_t)s);
}
extern "C" int vz_op_segment_sum_rows(const void* src, const int* map, int n_src, int rows_per, void* dst, int n_dst, int cols, vz_stream s) {
    return vz_launch_segment_sum_rows((const bf16_t*)src, map, n_src, rows_per, (bf16_t*)dst, n_dst, cols, (hipStream_t)s);
}
extern "C" int vz_op_acc_rows_f32(float* out, const void* src, int n_batches, long stride, int rows, int cols, vz_stream s) {
    return vz_launch_acc_rows_f32(out, (const bf16_t*)src, n_batches, stride, rows, cols, (hipStream_t)s);
}
extern "C" int vz_op_adamw(float* p, float* m, float* v, float* g, void* work, int work_bf16, long n, float lr, float beta1, float beta2, float eps,
                           float weight_decay, int t, vz_stream s) {
    return vz_launch_adamw(p, m, v, g, work, work_bf16, n, lr, beta1, beta2, eps, weight_decay, t, (hipStream_t)s);
}
extern "C" int vz_op_attention_bwd(const void* q, const void* k, const void* v, const void* dO, void* dq, void* dk, void* dv, int dkv_fp32, int B,
                                   int Sq, int Sk, int Hq, int Hkv, int head_dim, float scale, int causal, int window, const int* kv_len,
                                   float* ws, long ws_floats, vz_stream s) {
    VZ_CHECK_ARG(B > 0 && Sq > 0 && Sk > 0 && Hq > 0 && Hkv > 0 && Hq % Hkv == 0, "attention_bwd: bad shape");
    VZ_CHECK_ARG(head_dim == 128, "attention_bwd: the tile-resident backward is built for head_dim 128 (the Zephyr layers), got %d", head_dim);
    AttnBwdArgs f;
    f.q = (const bf16_t*)q; f.k = (const bf16_t*)k; f.v = (const bf16_t*)v; f.dO = (const bf16_t*)dO; f.B = B; f.Sq = Sq; f.Sk = Sk; f.Hq = Hq; f.Hkv = Hkv; f.D = head_dim;
    const long A = (long)Hq * head_dim;
    f.q_bs = f.o_bs = f.dq_bs = (long)Sq * A; f.q_ss = f.o_ss = f.dq_ss = A; f.q_hs = f.o_hs = f.dq_hs = head_dim;
    f.k_bs = f.v_bs = f.dk_bs = (long)Hkv * Sk * head_dim; f.k_ss = f.v_ss = f.dk_ss = head_dim; f.k_hs = f.v_hs = f.dk_hs = (long)Sk * head_dim;
    f.scale = scale; f.causal = causal; f.window = window; f.kv_len = kv_len;
    f.dq = (bf16_t*)dq; f.dk = dk; f.dv = dv; f.dkv_fp32 = dkv_fp32;
    return vz_launch_flash_bwd(f, ws, ws_floats > 0 ? (size_t)ws_floats * 4 : 0, (hipStream_t)s);
}
extern "C" int vz_op_rope_kv(const void* qkv, int ld, void* q_out, void* kc, void* vc, const float* cosT, const float* sinT,
                             const int* pos, const int* slot, int B, int S, int Hq, int Hkv, int D, int max_ctx, vz_stream s) {
    VZ_CHECK_ARG(qkv && q_out && kc && vc && cosT && sinT && pos && slot && B > 0 && S > 0, "rope: bad argument");
    return vz_launch_rope_kv((const bf16_t*)qkv, ld, (bf16_t*)q_out, (bf16_t*)kc, (bf16_t*)vc, cosT, sinT, pos, slot, B, S, Hq,
                             Hkv, D, max_ctx, (hipStream_t)s);
}
extern "C" int vz_op_attention_decode(const void* q, const void* kc, const void* vc, void* o, float* ws, int B, int Hq, int Hkv,
                                      int D, int max_ctx, int nsplit, int window, float scale, const int* ctx_len, vz_stream s) {
    VZ_CHECK_ARG(q && kc && vc && o && ws && ctx_len && B > 0, "attention_decode: bad argument");
    AttnDecodeArgs a;
    a.q = (const bf16_t*)q; a.kc = (const bf16_t*)kc; a.vc = (const bf16_t*)vc; a.o = (bf16_t*)o; a.part = ws;
    a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.D = D; a.max_ctx = max_ctx; a.nsplit = nsplit; a.window = window; a.scale = scale;
    a.ctx_len = ctx_len;
    return vz_launch_attn_decode(a, (hipStream_t)s);
}
extern "C" int vz_op_attention_decode_fused(const void* qkv, void* kc, void* vc, void* o, float* ws, unsigned* ticket,
                                            const float* cosT, const float* sinT, const int* pos, const int* slot, int B, int Hq,
                                            int Hkv, int D, int max_ctx, int nsplit, int window, float scale, vz_stream s) {
    VZ_CHECK_ARG(qkv && kc && vc && o && ws && ticket && cosT && sinT && pos && slot && B > 0, "attention_decode_fused: bad argument");
    AttnDecodeFusedArgs a;
    a.qkv = (const bf16_t*)qkv; a.kc = (bf16_t*)kc; a.vc = (bf16_t*)vc; a.o = (bf16_t*)o; a.part = ws; a.ticket = ticket;
    a.cosT = cosT; a.sinT = sinT; a.pos = pos; a.slot = slot;
    a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.D = D; a.max_ctx = max_ctx; a.nsplit = nsplit; a.window = window; a.scale = scale;
    return vz_launch_attn_decode_fused(a, (hipStream_t)s);
}
extern "C" int vz_op_attention_decode_kv8(const void* qkv, void* kc, void* vc, void* k8, void* v8, float* ks, float* vs, void* o, float* ws, unsigned* ticket,
                                          const float* cosT, const float* sinT, const int* pos, const int* slot, int B, int Hq,
                                          int Hkv, int D, int max_ctx, int nsplit, int window, float scale, vz_stream s) {
    VZ_CHECK_ARG(qkv && kc && vc && k8 && v8 && ks && vs && o && ws && ticket && cosT && sinT && pos && slot && B > 0, "attention_decode_kv8: bad argument");
    AttnDecodeKv8Args a;
    a.qkv = (const bf16_t*)qkv; a.kc = (bf16_t*)kc; a.vc = (bf16_t*)vc; a.k8 = (unsigned char*)k8; a.v8 = (unsigned char*)v8; a.ks = ks; a.vs = vs;
    a.o = (bf16_t*)o; a.part = ws; a.ticket = ticket; a.cosT = cosT; a.sinT = sinT; a.pos = pos; a.slot = slot;
    a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.D = D; a.max_ctx = max_ctx; a.nsplit = nsplit; a.window = window; a.scale = scale;
    return vz_launch_attn_decode_kv8(a, (hipStream_t)s);
}
extern "C" int vz_op_kv8_mirror_rows(const void* kc, const void* vc, void* k8, void* v8, float* ks, float* vs, int n, const int* h_row, const int* h_len,
                                     int Hkv, int D, int max_ctx, vz_stream s) {
    VZ_CHECK_ARG(kc && vc && k8 && v8 && ks && vs && h_row && h_len && n >= 1 && n <= 64 && D == 128, "kv8_mirror_rows: bad argument (1..64 rows, head_dim 128)");
    Kv8MirrorArgs a;
    a.src[0] = (const bf16_t*)kc; a.src[1] = (const bf16_t*)vc; a.q[0] = (unsigned char*)k8; a.q[1] = (unsigned char*)v8; a.sc[0] = ks; a.sc[1] = vs;
    a.layer_elems = 0; a.n_layers = 1; a.Hkv = Hkv; a.max_ctx = max_ctx; a.n = n;
    for (int i = 0; i < n; ++i) { a.row[i] = h_row[i]; a.len[i] = h_len[i]; }
    return vz_launch_kv8_mirror_rows(a, (hipStream_t)s);
}
extern "C" int vz_op_argmax(const float* logits, int rows, int cols, int* ids, vz_stream s) {
    return vz_launch_argmax(logits, rows, cols, ids, {}, (hipStream_t)s);
}

// ------------------------------------------------------------------------------------------------
// engine
// ------------------------------------------------------------------------------------------------
static TailKind tail_kind(const vz_engine* e) {
    return e->spec.on ? TAIL_SPEC : e->beam.on ? TAIL_BEAM : e->rows.on ? TAIL_ROWS : e->samp.on ? TAIL_SAMPLE : TAIL_GREEDY;
}
static bool tail_takes_proc(TailKind t) { return t != TAIL_SPEC; }      // the logits processors may sit in front of it

// One linear C = epi(A . W^T + W.b) of the engine: the route follows the row count, the caller (decode = the rows are the independent
// sequences of a decode step) and what finalize attached to W - vz_plan_linear picks the copy the kernel reads.
static LinearArgs linear_args(vz_engine* e, const bf16_t* A, int lda, const LinW& W, int ldw, void* C, int ldc, int M, int N, int K,
                              const bf16_t* res, int ldr, int act, int out_fp32, const float* norm_w, float norm_eps, int splitk_hint) {
    LinearArgs a = mk_linear(A, lda, W.w, ldw, C, ldc, M, N, K, W.b, res, ldr, act, out_fp32);
    a.W8 = W.w8; a.wscale = W.ws; a.Wt = W.wt; a.W8t = W.w8t;
    a.splitk_hint = splitk_hint;          // 0 = the dispatcher's choice (the Stage-2 trainer's narrow LoRA shapes pass their own)
    a.norm_w = norm_w; a.norm_eps = norm_eps; a.err = e->d_ferr;
    return a;
}
static LinCaller linear_caller(const vz_engine* e, int decode) { return LinCaller{decode ? LIN_ROWS_DECODE : LIN_ROWS_COUPLED, e->c.hidden}; }
int linear(vz_engine* e, int decode, const bf16_t* A, int lda, const LinW& W, int ldw, void* C, int ldc, int M,
           int N, int K, const bf16_t* res, int ldr, int act, int out_fp32, hipStream_t s,
           const float* norm_w, float norm_eps, int splitk_hint) {
    const LinearArgs a = linear_args(e, A, lda, W, ldw, C, ldc, M, N, K, res, ldr, act, out_fp32, norm_w, norm_eps, splitk_hint);
    const LinPlan p = vz_plan_linear(a, linear_caller(e, decode));
    e->last_stream = s;
    if (p.pre_norm) { ProfScope ps(e, K_NORM, s); RC(vz_run_prenorm(a, e->d_xnorm, s)); }
    ProfScope ps(e, p.klass, s);
    return vz_run_route(p, a, e->d_xnorm, s);
}

static int ensure_arena(vz_engine* e, size_t bytes) {
    if (bytes <= e->arena_bytes) return VZ_OK;
    if (e->arena) { VZ_CHECK_HIP(hipDeviceSynchronize()); VZ_CHECK_HIP(hipFree(e->arena)); e->arena = nullptr; e->arena_bytes = 0; }
    VZ_CHECK_HIP(hipMalloc((void**)&e->arena, bytes));
    e->arena_bytes = bytes;
    return VZ_OK;
}

// A stage's workspace: its ONE carve function (carve_clip, carve_qformer, carve_prefill, carve_append, carve_decode below; each takes dimensions, not
// the engine, so vz_op_stage_ws_bytes asks the same function without a device) sizes the arena over a null base and then lays out the
// real one; the mark it reaches is the stage's need (vz_engine_ws_info).
template <typename Ws, typename Carve> static int carve_stage(vz_engine* e, const char* stage, Carve carve, Ws* ws) {
    Carver dry(nullptr, ~(size_t)0);
    carve(dry);
    RC(ensure_arena(e, dry.off));
    Carver m(e->arena, e->arena_bytes);
    *ws = carve(m);
    e->arena_peak = m.off;
    if (!m.ok || m.off != dry.off) { vz_set_error("%s: the carving took %zu bytes of the arena, its sizing pass %zu (internal sizing error)", stage, m.off, dry.off); return VZ_ERR_STATE; }
    return VZ_OK;
}

int upload_ints(vz_engine* e, const int* h, size_t n, int* d, hipStream_t s) {
    // small host arrays go through a pinned staging buffer; the copy is enqueued on the stream
    if (n > e->h_pinned_ints) {
        if (e->h_pinned) { VZ_CHECK_HIP(hipStreamSynchronize(s)); VZ_CHECK_HIP(hipHostFree(e->h_pinned)); }
        VZ_CHECK_HIP(hipHostMalloc((void**)&e->h_pinned, n * sizeof(int)));
        e->h_pinned_ints = n;
    } else {
        VZ_CHECK_HIP(hipStreamSynchronize(s));  // previous use of the staging buffer has drained
    }
    memcpy(e->h_pinned, h, n * sizeof(int));
    VZ_CHECK_HIP(hipMemcpyAsync(d, e->h_pinned, n * sizeof(int), hipMemcpyHostToDevice, s));
    return VZ_OK;
}

// this rank's share of the query heads / KV heads / MLP columns (tp_size 1: everything)
struct Shard { int Hq, Hkv, I; };
static Shard shard_of(const vz_config& c) { return {c.n_heads / c.tp_size, c.n_kv_heads / c.tp_size, c.inter / c.tp_size}; }

static int check_config(const vz_config& c) {
    VZ_CHECK_ARG(c.head_dim == 128 && c.hidden % 512 == 0 && c.inter % 512 == 0 && c.n_heads % c.n_kv_heads == 0 &&
                     c.n_heads * c.head_dim == c.hidden, "engine_create: unsupported Zephyr geometry");
    VZ_CHECK_ARG(c.clip_hidden % 512 == 0 && c.clip_hidden / c.clip_heads == 64 && c.clip_image % c.clip_patch == 0,
                 "engine_create: unsupported CLIP geometry");
    VZ_CHECK_ARG(c.hidden / c.qf_heads == 512 && c.qf_kv_dim == (c.fusion_groups + 1) * c.clip_hidden && c.qf_queries == 32,
                 "engine_create: unsupported Q-Former geometry");
    VZ_CHECK_ARG(c.clip_layers + 1 >= c.fusion_groups * c.fusion_layers_per_group + 1, "engine_create: CLIP too shallow for the fusion");
    VZ_CHECK_ARG(c.max_batch >= 1 && c.max_ctx >= 64 && c.max_tiles >= 1 && c.max_text >= 0, "engine_create: bad capacity");
    VZ_CHECK_ARG(c.tp_size >= 1 && c.tp_rank >= 0 && c.tp_rank < c.tp_size, "engine_create: bad tp_size/tp_rank %d/%d", c.tp_size, c.tp_rank);
    // MLP shard: 16-row gate|up interleave and K %% 64 of the down-proj GEMM (tp 8: 14336 / 8 = 1792 columns; a shard that is not a
    // multiple of 512 takes the tile-GEMM path for the one-row down-proj instead of the GEMV)
    VZ_CHECK_ARG(c.n_kv_heads % c.tp_size == 0 && c.n_heads % c.tp_size == 0 && (c.inter / c.tp_size) % 64 == 0 && c.inter % c.tp_size == 0,
                 "engine_create: tp_size %d must divide the KV heads (%d) and leave MLP shards that are multiples of 64", c.tp_size, c.n_kv_heads);
    VZ_CHECK_ARG((c.n_heads / c.tp_size) == 4 * (c.n_kv_heads / c.tp_size), "engine_create: 4 query heads per KV head expected");
    return VZ_OK;
}

extern "C" int vz_engine_create(const vz_config* cfg, vz_engine** out) {
    VZ_CHECK_ARG(cfg && out, "engine_create: null argument");
    const vz_config& c = *cfg;
    RC(check_config(c));
    { int r = vz_init_gemm_kernels(); if (r) return r; r = vz_init_attention_kernels(); if (r) return r; }
    vz_engine* e = new vz_engine();
    e->c = c;
    e->tp = c.tp_size; e->rank = c.tp_rank;
    const Shard sh = shard_of(c);
    e->Hq_l = sh.Hq; e->Hkv_l = sh.Hkv; e->I_l = sh.I;
    e->Vp = (c.vocab + c.tp_size - 1) / c.tp_size;
    e->kv_layer_elems = (size_t)2 * c.max_batch * e->Hkv_l * c.max_ctx * c.head_dim;
    hipError_t er = hipMalloc((void**)&e->kv, e->kv_layer_elems * c.n_layers * sizeof(bf16_t));
    if (er == hipSuccess) er = hipMalloc((void**)&e->d_state, DecodeState::ints(c.max_batch) * sizeof(int));
    if (er == hipSuccess) er = hipMalloc((void**)&e->d_logits, (size_t)c.max_batch * e->Vp * e->tp * sizeof(float));
    // the partials of whichever decode attention runs: the fused step's records at up to 64 context splits (knob 10; attn_o_fused.hip and
    // decode_persist.hip run the same body on the same records), or the speculative tail's verify attention over its <= 8 rows
    const size_t part_floats = std::max(vz_attn_decode_part_floats(c.max_batch, e->Hkv_l, 64), vz_spec_part_floats(std::min(8, c.max_batch), e->Hkv_l, e->nsplit));
    if (er == hipSuccess) er = hipMalloc((void**)&e->d_part, part_floats * sizeof(float));
    if (er == hipSuccess) er = hipMalloc((void**)&e->d_ticket, 4096);
    if (er == hipSuccess) er = hipMalloc((void**)&e->d_xnorm, (size_t)64 * c.hidden * sizeof(bf16_t));
    if (er == hipSuccess) er = hipMemset(e->d_ticket, 0, 4096);
    if (er == hipSuccess) er = hipMalloc((void**)&e->d_ao_done, 64);
    if (er == hipSuccess) er = hipMemset(e->d_ao_done, 0, 64);
    if (er == hipSuccess) er = hipMalloc((void**)&e->d_ferr, sizeof(int));
    if (er == hipSuccess) er = hipMemset(e->d_ferr, 0, sizeof(int));
    if (er != hipSuccess) {
        vz_set_error("engine_create: hipMalloc failed: %s", hipGetErrorString(er));
        delete e;
        return VZ_ERR_HIP;
    }
    *out = e;
    return VZ_OK;
}

extern "C" int vz_engine_destroy(vz_engine* e) {
    if (!e) return VZ_OK;
    hipDeviceSynchronize();
    if (e->dec_graph) (void)hipGraphExecDestroy(e->dec_graph);
    if (e->cap_stream) (void)hipStreamDestroy(e->cap_stream);
    for (auto& p : e->prof_ev) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    if (e->arena) hipFree(e->arena);
    if (e->kv) hipFree(e->kv);
    if (e->d_state) hipFree(e->d_state);
    if (e->d_logits) hipFree(e->d_logits);
    if (e->d_part) hipFree(e->d_part);
    if (e->d_ticket) hipFree(e->d_ticket);
    if (e->d_ao_done) hipFree(e->d_ao_done);
    if (e->d_ferr) hipFree(e->d_ferr);
    if (e->d_xnorm) hipFree(e->d_xnorm);
    if (e->beam.d) hipFree(e->beam.d);
    if (e->share.d_tab) hipFree(e->share.d_tab);
    if (e->share.q_rot) hipFree(e->share.q_rot);
    if (e->share.ws) hipFree(e->share.ws);
    if (e->kv8.q) hipFree(e->kv8.q);
    if (e->kv8.sc) hipFree(e->kv8.sc);
    if (e->proc.d) hipFree(e->proc.d);
    if (e->proc.d_seq) hipFree(e->proc.d_seq);
    if (e->proc.d_rows) hipFree(e->proc.d_rows);
    if (e->proc.d_rowseq) hipFree(e->proc.d_rowseq);
    if (e->stop.d_rowseq) hipFree(e->stop.d_rowseq);
    if (e->score.d_slot) hipFree(e->score.d_slot);
    if (e->stop.d_state) hipFree(e->stop.d_state);
    if (e->stop.d_tab) hipFree(e->stop.d_tab);
    if (e->d_gather) (void)hipFree(e->d_gather);
    vz_decode_persist_destroy(e->tok);
    if (e->comm) (void)ncclCommDestroy(e->comm);
    if (e->os_area) (void)hipFree(e->os_area);
    if (e->os_seq) (void)hipFree(e->os_seq);
    if (e->h_pinned) hipHostFree(e->h_pinned);
    delete e;
    return VZ_OK;
}

// The captured decode graph freezes every pointer its kernels take (weights, rotary tables, the gathered-logits buffer, the
// workspace): whoever replaces one of them drops the graph, the next vz_llm_decode_steps captures again.
int drop_decode_graph(vz_engine* e) {
    if (e->tok) {                               // the persistent kernel's layer table freezes weight / cache pointers too
        VZ_CHECK_HIP(hipDeviceSynchronize());
        vz_decode_persist_destroy(e->tok);
        e->tok = nullptr;
    }
    if (!e->dec_graph) return VZ_OK;
    VZ_CHECK_HIP(hipDeviceSynchronize());       // a replay may still be running
    (void)hipGraphExecDestroy(e->dec_graph);
    e->dec_graph = nullptr;
    return VZ_OK;
}

extern "C" int vz_engine_set_weight(vz_engine* e, const char* name, const void* d_ptr, int dtype, long n_elems) {
    VZ_CHECK_ARG(e && name && d_ptr && dtype >= 0 && dtype <= 2 && n_elems > 0, "set_weight: bad argument");
    VZ_CHECK_ARG(((uintptr_t)d_ptr & 15) == 0, "set_weight: '%s' must be 16-byte aligned", name);
    RC(drop_decode_graph(e));
    e->w[name] = Weight{d_ptr, dtype, n_elems};
    e->finalized = false;
    return VZ_OK;
}

// forget a registered weight (the e4m3 copy / scales of a bf16 tensor that has been rewritten: finalize must not accept the stale ones)
extern "C" int vz_engine_unset_weight(vz_engine* e, const char* name) {
    VZ_CHECK_ARG(e && name, "unset_weight: bad argument");
    RC(drop_decode_graph(e));
    e->w.erase(name);
    e->finalized = false;
    return VZ_OK;
}

extern "C" int vz_engine_resize_vocab(vz_engine* e, int new_vocab) {
    VZ_CHECK_ARG(e && new_vocab > 0, "resize_vocab: bad argument");
    VZ_CHECK_ARG(e->tp == 1, "resize_vocab: not available on a tensor-parallel engine (rebuild it at the new vocabulary)");
    if (new_vocab == e->c.vocab) return VZ_OK;
    VZ_CHECK_HIP(hipDeviceSynchronize());
    RC(drop_decode_graph(e));     // it holds the old logits width
    if (e->d_logits) { VZ_CHECK_HIP(hipFree(e->d_logits)); e->d_logits = nullptr; }
    e->c.vocab = new_vocab;
    e->Vp = new_vocab;
    VZ_CHECK_HIP(hipMalloc((void**)&e->d_logits, (size_t)e->c.max_batch * e->Vp * sizeof(float)));
    e->w.erase("llm.embed");
    e->w.erase("llm.lm_head");
    e->finalized = false;
    return VZ_OK;
}

static int kpad_patch(const vz_config& c) { return (int)align_up((size_t)3 * c.clip_patch * c.clip_patch, 64); }

extern "C" int vz_engine_finalize(vz_engine* e) {
    VZ_CHECK_ARG(e, "finalize: null engine");
    const vz_config& c = e->c;
    e->finalized = false;
    int rc = VZ_OK;
    // a registered tensor of the expected dtype and element count; the first one that is missing or differs fails the call
    auto get = [&](const std::string& name, int dtype, long n) -> const void* {
        if (rc) return nullptr;
        auto it = e->w.find(name);
        if (it == e->w.end()) { vz_set_error("weight '%s' was never registered", name.c_str()); rc = VZ_ERR_STATE; return nullptr; }
        if (it->second.dtype != dtype || it->second.n != n) {
            vz_set_error("weight '%s': expected dtype %d n %ld, got dtype %d n %ld", name.c_str(), dtype, n, it->second.dtype,
                         it->second.n);
            rc = VZ_ERR_STATE;
            return nullptr;
        }
        return it->second.p;
    };
    // the fragment-tiled copy of a matrix: "<name>t" with the same dtype and element count, else none
    auto tiled = [&](const std::string& name, int dtype, long n) -> const void* {
        auto it = e->w.find(name + "t");
        return it != e->w.end() && it->second.dtype == dtype && it->second.n == n ? it->second.p : nullptr;
    };
    auto vec = [&](const std::string& name, long n) { return (const float*)get(name, 1, n); };
    auto mat = [&](const std::string& name, long n) { return (const bf16_t*)get(name, 0, n); };
    auto norm = [&](const std::string& p, long n) { NormW r; r.w = vec(p + ".w", n); r.b = vec(p + ".b", n); return r; };
    auto lin = [&](const std::string& name, long n) { LinW l; l.w = mat(name, n); l.wt = (const bf16_t*)tiled(name, 0, n); return l; };
    auto lin_b = [&](const std::string& p, long n, long nb) { LinW l = lin(p + ".w", n); l.b = vec(p + ".b", nb); return l; };
    // weight_fp8: the e4m3 copy (and its tiled copy) + the row scales of a decode-side linear
    auto fp8 = [&](LinW& l, const std::string& n8, const std::string& ns, long n, long rows) {
        if (!c.weight_fp8) return;
        l.w8 = (const unsigned char*)get(n8, 2, n); l.w8t = (const unsigned char*)tiled(n8, 2, n); l.ws = vec(ns, rows);
    };
    const long C = c.clip_hidden, H = c.hidden, KD = c.qf_kv_dim, tokens = (c.clip_image / c.clip_patch) * (c.clip_image / c.clip_patch) + 1;
    TopW& t = e->top;
    t.clip_patch_w = mat("clip.patch_w", C * kpad_patch(c)); t.clip_cls = mat("clip.cls", C); t.clip_pos = mat("clip.pos", tokens * C);
    t.clip_pre_ln = norm("clip.pre_ln", C);
    e->clip.assign(c.clip_layers, ClipLayerW());
    for (int i = 0; i < c.clip_layers; ++i) {
        const std::string p = "clip." + std::to_string(i) + ".";
        ClipLayerW& L = e->clip[i];
        L.ln1 = norm(p + "ln1", C); L.qkv = lin_b(p + "qkv", 3 * C * C, 3 * C); L.o = lin_b(p + "o", C * C, C); L.ln2 = norm(p + "ln2", C);
        L.fc1 = lin_b(p + "fc1", c.clip_inter * C, c.clip_inter); L.fc2 = lin_b(p + "fc2", c.clip_inter * C, C);
    }
    t.qf_queries = mat("qf.queries", c.qf_queries * H); t.qf_pre_norm = norm("qf.pre_norm", KD); t.qf_norm = norm("qf.norm", H);
    e->qf.assign(c.qf_blocks, QfBlockW());
    for (int i = 0; i < c.qf_blocks; ++i) {
        const std::string p = "qf." + std::to_string(i) + ".";
        QfBlockW& Q = e->qf[i];
        Q.n1 = norm(p + "n1", H); Q.n2 = norm(p + "n2", H); Q.n3 = norm(p + "n3", H);
        Q.sa_in = lin_b(p + "sa_in", 3 * H * H, 3 * H); Q.sa_out = lin_b(p + "sa_out", H * H, H);
        Q.ca_q = lin_b(p + "ca_q", H * H, H); Q.ca_kv = lin_b(p + "ca_kv", 2 * H * KD, 2 * H); Q.ca_out = lin_b(p + "ca_out", H * H, H);
        Q.ffn1 = lin_b(p + "ffn1", 2 * H * H, 2 * H); Q.ffn2 = lin_b(p + "ffn2", 2 * H * H, H);
    }
    const long qkv_n = (long)(e->Hq_l + 2 * e->Hkv_l) * c.head_dim, A = (long)e->Hq_l * c.head_dim, I = e->I_l;
    t.embed = mat("llm.embed", (long)c.vocab * H); t.norm = vec("llm.norm", H); t.lm_head = lin("llm.lm_head", (long)e->Vp * H);
    fp8(t.lm_head, "llm.lm_head8", "llm.lm_heads", (long)e->Vp * H, e->Vp);
    e->llm.assign(c.n_layers, LlmLayerW());
    for (int i = 0; i < c.n_layers; ++i) {
        const std::string p = "llm." + std::to_string(i) + ".";
        LlmLayerW& L = e->llm[i];
        L.in_norm = vec(p + "in_norm", H); L.post_norm = vec(p + "post_norm", H);
        L.qkv = lin(p + "qkv.w", qkv_n * H); L.o = lin(p + "o.w", H * A); L.gu = lin(p + "gu.w", 2 * I * H); L.down = lin(p + "down.w", I * H);
        fp8(L.qkv, p + "qkv.w8", p + "qkv.ws", qkv_n * H, qkv_n); fp8(L.o, p + "o.w8", p + "o.ws", H * A, H);
        fp8(L.gu, p + "gu.w8", p + "gu.ws", 2 * I * H, 2 * I); fp8(L.down, p + "down.w8", p + "down.ws", I * H, H);
    }
    if (rc) return rc;
    // vz_qformer runs the cross-attention K|V projections of all blocks as one product when their weights and biases are contiguous
    // (vz_hip/engine.py allocates them so; a C-ABI caller may too)
    e->qf_kv_contig = c.qf_blocks > 1;
    for (int i = 1; i < c.qf_blocks && e->qf_kv_contig; ++i)
        e->qf_kv_contig = e->qf[i].ca_kv.w == e->qf[0].ca_kv.w + (size_t)i * 2 * H * KD && e->qf[i].ca_kv.b == e->qf[0].ca_kv.b + (size_t)i * 2 * H;
    e->finalized = true;
    return VZ_OK;
}

extern "C" int vz_engine_set_rope(vz_engine* e, const float* d_cos, const float* d_sin, int max_pos) {
    VZ_CHECK_ARG(e && d_cos && d_sin && max_pos > 0, "set_rope: bad argument");
    RC(drop_decode_graph(e));
    e->cosT = d_cos; e->sinT = d_sin; e->rope_max = max_pos;
    return VZ_OK;
}

// ------------------------------------------------------------------------------------------------
// a8-a10: CLIP tower + fusion
// ------------------------------------------------------------------------------------------------
static int clip_tokens(const vz_config& c) { return (c.clip_image / c.clip_patch) * (c.clip_image / c.clip_patch) + 1; }
static bool clip_shape_ok(const vz_config& c, int T) { return T >= 1 && T <= c.max_tiles; }
struct ClipWs { bf16_t *col, *pe, *hs, *y, *qkv, *att, *mlp; };
// own_hs = false: the caller supplies the buffer of every layer's hidden states (d_hidden_dbg)
static ClipWs carve_clip(Carver& m, const vz_config& c, int T, bool own_hs) {
    const size_t P = clip_tokens(c) - 1, hs_layer = (size_t)T * (P + 1) * c.clip_hidden;
    ClipWs w;
    w.col = m.take<bf16_t>((size_t)T * P * kpad_patch(c));
    w.pe = m.take<bf16_t>((size_t)T * P * c.clip_hidden);
    w.hs = own_hs ? m.take<bf16_t>(hs_layer * (c.clip_layers + 1)) : nullptr;
    w.y = m.take<bf16_t>(hs_layer);
    w.qkv = m.take<bf16_t>(hs_layer * 3);
    w.att = m.take<bf16_t>(hs_layer);
    w.mlp = m.take<bf16_t>((size_t)T * (P + 1) * c.clip_inter);
    return w;
}

extern "C" int vz_clip_fused_features(vz_engine* e, const void* d_images, int T, void* d_out, void* d_hidden_dbg,
                                      vz_stream stream) {
    NEED_READY();
    const vz_config& c = e->c;
    hipStream_t s = (hipStream_t)stream;
    VZ_CHECK_ARG(d_images && d_out && clip_shape_ok(c, T), "clip: T=%d outside [1,%d]", T, c.max_tiles);
    const int C = c.clip_hidden, tokens = clip_tokens(c), P = tokens - 1, kpad = kpad_patch(c);
    const int L = c.clip_layers, rows = T * tokens;
    const size_t hs_layer = (size_t)rows * C;
    ClipWs w;
    RC(carve_stage(e, "clip", [&](Carver& m) { return carve_clip(m, c, T, !d_hidden_dbg); }, &w));
    bf16_t *col = w.col, *pe = w.pe, *hs = d_hidden_dbg ? (bf16_t*)d_hidden_dbg : w.hs, *y = w.y, *qkv = w.qkv, *att = w.att, *mlp = w.mlp;
    const TopW& t = e->top;
    {
        ProfScope ps(e, K_OTHER, s);
        RC(vz_launch_im2col((const bf16_t*)d_images, T, c.clip_image, c.clip_patch, kpad, col, s));
    }
    RC(linear(e, 0, col, kpad, bare(t.clip_patch_w), kpad, pe, C, T * P, C, kpad, nullptr, 0, VZ_ACT_NONE, 0, s));
    {
        ProfScope ps(e, K_OTHER, s);
        RC(vz_launch_clip_assemble(pe, t.clip_cls, t.clip_pos, T, tokens, C, att, s));
    }
    {
        ProfScope ps(e, K_NORM, s);
        RC(vz_launch_layernorm(att, C, hs, C, t.clip_pre_ln.w, t.clip_pre_ln.b, rows, C, c.clip_eps, s));
    }
    for (int i = 0; i < L; ++i) {
        const ClipLayerW& W = e->clip[i];
        bf16_t* x = hs + hs_layer * i;
        bf16_t* xn = hs + hs_layer * (i + 1);
        { ProfScope ps(e, K_NORM, s); RC(vz_launch_layernorm(x, C, y, C, W.ln1.w, W.ln1.b, rows, C, c.clip_eps, s)); }
        RC(linear(e, 0, y, C, W.qkv, C, qkv, 3 * C, rows, 3 * C, C, nullptr, 0, VZ_ACT_NONE, 0, s));
        {
            ProfScope ps(e, K_ATTN, s);
            AttnArgs a;
            a.q = qkv; a.k = qkv + C; a.v = qkv + 2 * C; a.o = att;
            a.B = T; a.Sq = tokens; a.Sk = tokens; a.Hq = c.clip_heads; a.Hkv = c.clip_heads; a.head_dim = 64;
            a.q_bs = a.k_bs = a.v_bs = (long)tokens * 3 * C; a.q_ss = a.k_ss = a.v_ss = 3 * C; a.q_hs = a.k_hs = a.v_hs = 64;
            a.o_bs = (long)tokens * C; a.o_ss = C; a.o_hs = 64;
            a.scale = 0.125f; a.causal = 0; a.q_pos0 = 0; a.window = 0; a.kv_len = nullptr;
            RC(vz_launch_attention(a, s));
        }
        RC(linear(e, 0, att, C, W.o, C, xn, C, rows, C, C, x, C, VZ_ACT_NONE, 0, s));
        { ProfScope ps(e, K_NORM, s); RC(vz_launch_layernorm(xn, C, y, C, W.ln2.w, W.ln2.b, rows, C, c.clip_eps, s)); }
        RC(linear(e, 0, y, C, W.fc1, C, mlp, c.clip_inter, rows, c.clip_inter, C, nullptr, 0, VZ_ACT_QUICK_GELU, 0, s));
        RC(linear(e, 0, mlp, c.clip_inter, W.fc2, c.clip_inter, xn, C, rows, C, c.clip_inter, xn, C, VZ_ACT_NONE, 0, s));
    }
    ProfScope ps(e, K_OTHER, s);
    const int first = L - c.fusion_groups * c.fusion_layers_per_group;
    return vz_launch_fusion(hs, (long)hs_layer, first, c.fusion_groups, c.fusion_layers_per_group, T, tokens, C, c.clip_keep_cls ? 0 : 1, (bf16_t*)d_out, s);
}

// ------------------------------------------------------------------------------------------------
// a11: Q-Former
// ------------------------------------------------------------------------------------------------
int qf_attn(vz_engine* e, const bf16_t* q, long q_bs, long q_ss, const bf16_t* k, const bf16_t* v, long kv_bs, long kv_ss,
            bf16_t* o, int B, int Sq, int Sk, hipStream_t s, float* part, size_t part_floats) {
    ProfScope ps(e, K_ATTN, s);
    AttnArgs a;
    a.part = part; a.part_floats = part_floats;
    a.q = q; a.k = k; a.v = v; a.o = o;
    a.B = B; a.Sq = Sq; a.Sk = Sk; a.Hq = e->c.qf_heads; a.Hkv = e->c.qf_heads; a.head_dim = 512;
    a.q_bs = q_bs; a.q_ss = q_ss; a.q_hs = 512; a.k_bs = a.v_bs = kv_bs; a.k_ss = a.v_ss = kv_ss; a.k_hs = a.v_hs = 512;
    a.o_bs = (long)Sq * e->c.hidden; a.o_ss = e->c.hidden; a.o_hs = 512;
    a.scale = 0.044194173824159216f;  // 512^-0.5
    a.causal = 0; a.q_pos0 = 0; a.window = 0; a.kv_len = nullptr;
    return vz_launch_attention(a, s);
}

static int qf_visual_tokens(const vz_config& c) { return clip_tokens(c) - (c.clip_keep_cls ? 0 : 1); }      // per tile
static bool qf_shape_ok(const vz_config& c, int T, int n_samples, int Lmax) {
    return T >= 1 && T <= c.max_tiles && Lmax >= 0 && Lmax <= c.max_text && n_samples >= 1 && n_samples <= T;
}
// The cross-attention K|V projections of all blocks read the same pre-normed features.  When their weights (and biases) lie back
// to back in memory (`contig` = qf_kv_contig) they run as ONE product over N = blocks * 2H: 256 column tiles per row tile = whole residency
// rounds of the 256^2 kernel, no stream-K tail (8 x 217 us -> one launch).  The [T * P, blocks * 2H] result is capped at 2 GiB;
// larger tile batches fill the chip per block anyway.
static bool qf_kv_all(const vz_config& c, int T, bool contig) {
    return contig && (size_t)T * qf_visual_tokens(c) * c.qf_blocks * 2 * c.hidden * sizeof(bf16_t) <= ((size_t)2 << 30) && vz_knob(VZ_KNOB_QF_KV_ALL);
}
struct QfWs { bf16_t *fn, *ckv, *x0, *y0, *kv0, *q0, *a0, *xs, *x, *y, *qkv, *att, *ff; float* part; size_t part_floats; };
static QfWs carve_qformer(Carver& m, const vz_config& c, int T, int n_samples, int Lmax, bool kv_all) {
    const size_t H = c.hidden, NQ = c.qf_queries, P = qf_visual_tokens(c), N0 = NQ + Lmax, R = (size_t)T * NQ;
    QfWs w;
    w.fn = m.take<bf16_t>((size_t)T * P * c.qf_kv_dim);                               // pre_norm(features)
    w.ckv = m.take<bf16_t>((size_t)T * P * (kv_all ? c.qf_blocks : 1) * 2 * H);        // cross-attention K|V of the current block (kv_all: of every block)
    w.x0 = m.take<bf16_t>((size_t)n_samples * N0 * H);                                // [queries ; text] per sample
    w.y0 = m.take<bf16_t>((size_t)n_samples * N0 * H);
    w.kv0 = m.take<bf16_t>((size_t)n_samples * N0 * 2 * H);
    w.q0 = m.take<bf16_t>(NQ * H);
    w.a0 = m.take<bf16_t>((size_t)n_samples * NQ * H);
    w.xs = m.take<bf16_t>((size_t)n_samples * NQ * H);
    w.x = m.take<bf16_t>(R * H);                                                      // the query rows in flight after block 0's self-attention
    w.y = m.take<bf16_t>(R * H);
    w.qkv = m.take<bf16_t>(R * 3 * H);
    w.att = m.take<bf16_t>(R * H);
    w.ff = m.take<bf16_t>(R * 2 * H);
    // key-split partials: what the launcher asks for the cross-attention over P keys and for block 0's self-attention over [queries ; text]
    w.part_floats = std::max(vz_attn_split_floats(T, c.qf_heads, (int)NQ, (int)P), vz_attn_split_floats(n_samples, c.qf_heads, (int)NQ, (int)N0));
    w.part = m.take<float>(w.part_floats);
    return w;
}

extern "C" int vz_qformer(vz_engine* e, const void* d_feats, int T, const void* d_text, int n_samples, int Lmax,
                          const int* h_tile_sample, void* d_out, vz_stream stream) {
    NEED_READY();
    const vz_config& c = e->c;
    hipStream_t s = (hipStream_t)stream;
    VZ_CHECK_ARG(d_feats && d_out && T >= 1 && T <= c.max_tiles, "qformer: T=%d outside [1,%d]", T, c.max_tiles);
    VZ_CHECK_ARG(Lmax >= 0 && Lmax <= c.max_text, "qformer: Lmax=%d outside [0,%d]", Lmax, c.max_text);
    VZ_CHECK_ARG(qf_shape_ok(c, T, n_samples, Lmax) && h_tile_sample && (Lmax == 0 || d_text), "qformer: bad sample map");
    for (int t = 0; t < T; ++t) VZ_CHECK_ARG(h_tile_sample[t] >= 0 && h_tile_sample[t] < n_samples, "qformer: tile_sample[%d] out of range", t);
    const int H = c.hidden, NQ = c.qf_queries, KD = c.qf_kv_dim;
    const int P = qf_visual_tokens(c), N0 = NQ + Lmax, FF = 2 * H;
    const size_t R = (size_t)T * NQ;  // query rows in flight after block 0's self-attention
    const bool kv_all = qf_kv_all(c, T, e->qf_kv_contig);
    const int kv_ld = kv_all ? c.qf_blocks * 2 * H : 2 * H;
    QfWs w;
    RC(carve_stage(e, "qformer", [&](Carver& m) { return carve_qformer(m, c, T, n_samples, Lmax, kv_all); }, &w));
    bf16_t *fn = w.fn, *ckv = w.ckv, *x0 = w.x0, *y0 = w.y0, *kv0 = w.kv0, *q0 = w.q0, *a0 = w.a0, *xs = w.xs, *x = w.x, *y = w.y, *qkv = w.qkv, *att = w.att, *ff = w.ff;
    { ProfScope ps(e, K_NORM, s); RC(vz_launch_layernorm((const bf16_t*)d_feats, KD, fn, KD, e->top.qf_pre_norm.w, e->top.qf_pre_norm.b, T * P, KD, c.qf_eps, s)); }
    const bf16_t* queries = e->top.qf_queries;
    // ---- block 0 self-attention, once per sample, query rows only ----
    {
        ProfScope ps(e, K_OTHER, s);
        for (int sm = 0; sm < n_samples; ++sm) {
            RC(vz_launch_copy_rows(queries, H, x0 + (size_t)sm * N0 * H, H, NQ, H, s));
            if (Lmax > 0) RC(vz_launch_copy_rows((const bf16_t*)d_text + (size_t)sm * Lmax * H, H, x0 + ((size_t)sm * N0 + NQ) * H, H, Lmax, H, s));
            RC(vz_launch_copy_rows(queries, H, xs + (size_t)sm * NQ * H, H, NQ, H, s));
        }
    }
    {
        const QfBlockW& W = e->qf[0];
        { ProfScope ps(e, K_NORM, s); RC(vz_launch_layernorm(x0, H, y0, H, W.n1.w, W.n1.b, n_samples * N0, H, c.qf_eps, s)); }
        RC(linear(e, 0, y0, H, lin_rows(W.sa_in, H, H), H, kv0, 2 * H, n_samples * N0, 2 * H, H, nullptr, 0, VZ_ACT_NONE, 0, s));
        RC(linear(e, 0, y0, H, W.sa_in, H, q0, H, NQ, H, H, nullptr, 0, VZ_ACT_NONE, 0, s));  // rows 0..31 of sample 0 = LN1(queries)
        RC(qf_attn(e, q0, 0, H, kv0, kv0 + H, (long)N0 * 2 * H, 2 * H, a0, n_samples, NQ, N0, s, w.part, w.part_floats));
        RC(linear(e, 0, a0, H, W.sa_out, H, xs, H, n_samples * NQ, H, H, xs, H, VZ_ACT_NONE, 0, s));
        ProfScope ps(e, K_OTHER, s);
        for (int t = 0; t < T; ++t) RC(vz_launch_copy_rows(xs + (size_t)h_tile_sample[t] * NQ * H, H, x + (size_t)t * NQ * H, H, NQ, H, s));
    }
    for (int i = 0; i < c.qf_blocks; ++i) {
        const QfBlockW& W = e->qf[i];
        if (i > 0) {
            { ProfScope ps(e, K_NORM, s); RC(vz_launch_layernorm(x, H, y, H, W.n1.w, W.n1.b, (int)R, H, c.qf_eps, s)); }
            RC(linear(e, 0, y, H, W.sa_in, H, qkv, 3 * H, (int)R, 3 * H, H, nullptr, 0, VZ_ACT_NONE, 0, s));
            RC(qf_attn(e, qkv, (long)NQ * 3 * H, 3 * H, qkv + H, qkv + 2 * H, (long)NQ * 3 * H, 3 * H, att, T, NQ, NQ, s));
            RC(linear(e, 0, att, H, W.sa_out, H, x, H, (int)R, H, H, x, H, VZ_ACT_NONE, 0, s));
        }
        // cross-attention against the tile's 576 fused visual tokens (kv_all: block 0's ca_kv heads the weights of every block)
        if (!kv_all || i == 0) RC(linear(e, 0, fn, KD, W.ca_kv, KD, ckv, kv_ld, T * P, kv_ld, KD, nullptr, 0, VZ_ACT_NONE, 0, s));
        const bf16_t* ck = kv_all ? ckv + (size_t)i * 2 * H : ckv;
        { ProfScope ps(e, K_NORM, s); RC(vz_launch_layernorm(x, H, y, H, W.n2.w, W.n2.b, (int)R, H, c.qf_eps, s)); }
        RC(linear(e, 0, y, H, W.ca_q, H, qkv, H, (int)R, H, H, nullptr, 0, VZ_ACT_NONE, 0, s));
        RC(qf_attn(e, qkv, (long)NQ * H, H, ck, ck + H, (long)P * kv_ld, kv_ld, att, T, NQ, P, s, w.part, w.part_floats));
        RC(linear(e, 0, att, H, W.ca_out, H, x, H, (int)R, H, H, x, H, VZ_ACT_NONE, 0, s));
        // FFN
        { ProfScope ps(e, K_NORM, s); RC(vz_launch_layernorm(x, H, y, H, W.n3.w, W.n3.b, (int)R, H, c.qf_eps, s)); }
        RC(linear(e, 0, y, H, W.ffn1, H, ff, FF, (int)R, FF, H, nullptr, 0, VZ_ACT_GELU_ERF, 0, s));
        RC(linear(e, 0, ff, FF, W.ffn2, FF, x, H, (int)R, H, FF, x, H, VZ_ACT_NONE, 0, s));
    }
    ProfScope ps(e, K_NORM, s);
    return vz_launch_layernorm(x, H, (bf16_t*)d_out, H, e->top.qf_norm.w, e->top.qf_norm.b, (int)R, H, c.qf_eps, s);
}

// ------------------------------------------------------------------------------------------------
// a6/a7: splice
// ------------------------------------------------------------------------------------------------
extern "C" int vz_embed_splice(vz_engine* e, const int* d_kind, const int* d_idx, int rows, const void* d_visual, void* d_out,
                               vz_stream stream) {
    NEED_READY();
    VZ_CHECK_ARG(d_idx && d_out && rows > 0, "splice: bad argument");
    ProfScope ps(e, K_OTHER, (hipStream_t)stream);
    return vz_launch_gather_rows(d_kind, d_idx, rows, e->c.hidden, e->top.embed, (const bf16_t*)d_visual, (bf16_t*)d_out, (hipStream_t)stream);
}


// ---- tensor-parallel collectives (RCCL over xGMI); no-ops at tp == 1 ----
// Self-test (vz_tune_set(7, 1)): an engine with tp_size == 1 that has been given a one-rank communicator routes the same
// call sites through RCCL (all-reduce over one rank = identity, all-gather = copy), so the collective plumbing - library,
// dtypes, in-place buffers, stream order, the vocab-parallel gather + repack - runs on a single GPU.
static inline bool tp_local(const vz_engine* e) { return e->tp == 1 && !(vz_knob(VZ_KNOB_FORCE_COMM) && e->comm); }

// vz_tune_set(7, 2): shape rehearsal of ONE rank of a tp_size > 1 engine on a single GPU - every collective is skipped (the
// partial sums / vocab shard are left as they are), so all local kernels run with that rank's shard shapes; results are
// meaningless as logits, the point is that nothing on the local path rejects the shapes of tp 2 / 4 / 8.
static inline bool tp_skip(const vz_engine* e) { return e->tp > 1 && vz_knob(VZ_KNOB_FORCE_COMM) == 2; }

static int tp_allreduce_bf16(vz_engine* e, bf16_t* buf, size_t count, hipStream_t s, bool decode = false) {
    if (decode && vz_knob(VZ_KNOB_ONESHOT) && e->os_ranks == e->tp && e->tp > 1 && (int)count <= vz_engine::OS_MAX_ELEMS && (count & 1) == 0 && !tp_skip(e)) {
        ProfScope ps(e, K_COMM, s);
        return vz_launch_allreduce_oneshot(e->os_areas, e->rank, e->tp, vz_engine::OS_MAX_ELEMS, buf, buf, (int)count, e->os_seq, e->d_ferr, s);
    }
    if (tp_local(e) || tp_skip(e)) return VZ_OK;
    if (!e->comm) { vz_set_error("tensor-parallel engine used before vz_comm_init"); return VZ_ERR_STATE; }
    ProfScope ps(e, K_COMM, s);
    ncclResult_t r = ncclAllReduce(buf, buf, count, ncclBfloat16, ncclSum, e->comm, s);
    if (r != ncclSuccess) { vz_set_error("ncclAllReduce failed: %s", ncclGetErrorString(r)); return VZ_ERR_HIP; }
    return VZ_OK;
}

// lm_head over `rows` hidden rows -> fp32 logits [rows, vocab] in `out`.  Vocab-parallel under TP: every rank computes its
// Vp rows of the table, the shards are all-gathered and repacked to the dense [rows, vocab] layout on every rank.
// vocab-parallel lm_head: [tp][rows][Vp] gathered logits + this rank's shard behind them (never grows inside a stream capture:
// vz_llm_decode_steps sizes it before it captures)
static int ensure_gather(vz_engine* e, int rows, hipStream_t s) {
    if (e->tp == 1 && !e->comm) return VZ_OK;
    const size_t local_off = ((size_t)e->tp * rows * e->Vp + 3) & ~(size_t)3;
    const size_t need = local_off + (size_t)rows * e->Vp;
    if (need > e->gather_floats) {
        RC(drop_decode_graph(e));    // its all-gather / repack / lm_head nodes hold the old buffer and the old shard offset
        if (e->d_gather) { VZ_CHECK_HIP(hipStreamSynchronize(s)); VZ_CHECK_HIP(hipFree(e->d_gather)); e->d_gather = nullptr; }
        VZ_CHECK_HIP(hipMalloc((void**)&e->d_gather, need * sizeof(float)));
        e->gather_floats = need;
    }
    return VZ_OK;
}

static int lm_head_logits(vz_engine* e, const bf16_t* h, int rows, float* out, hipStream_t s, const float* norm_w) {
    const vz_config& c = e->c;
    const int H = c.hidden;
    const LinW& lm = e->top.lm_head;
    if (tp_local(e)) return linear(e, norm_w ? 1 : 0, h, H, lm, H, out, c.vocab, rows, c.vocab, H, nullptr, 0, VZ_ACT_NONE, 1, s, norm_w, c.rms_eps);
    const size_t local_off = ((size_t)e->tp * rows * e->Vp + 3) & ~(size_t)3;      // the GEMM wants a 16-byte-aligned output base
    { int r = ensure_gather(e, rows, s); if (r) return r; }
    float* local = e->d_gather + local_off;
    RC(linear(e, norm_w ? 1 : 0, h, H, lm, H, local, e->Vp, rows, e->Vp, H, nullptr, 0, VZ_ACT_NONE, 1, s, norm_w, c.rms_eps));
    if (!e->comm && !tp_skip(e)) { vz_set_error("tensor-parallel engine used before vz_comm_init"); return VZ_ERR_STATE; }
    if (tp_skip(e)) {     // rehearsal: this rank's shard goes to its own chunk, the others stay zero
        VZ_CHECK_HIP(hipMemsetAsync(e->d_gather, 0, (size_t)e->tp * rows * e->Vp * sizeof(float), s));
        VZ_CHECK_HIP(hipMemcpyAsync(e->d_gather + (size_t)e->rank * rows * e->Vp, local, (size_t)rows * e->Vp * sizeof(float), hipMemcpyDeviceToDevice, s));
        return vz_launch_repack_logits(e->d_gather, out, rows, e->Vp, c.vocab, e->tp, s);
    }
    ncclResult_t r;
    { ProfScope ps(e, K_COMM, s); r = ncclAllGather(local, e->d_gather, (size_t)rows * e->Vp, ncclFloat, e->comm, s); }
    if (r != ncclSuccess) { vz_set_error("ncclAllGather failed: %s", ncclGetErrorString(r)); return VZ_ERR_HIP; }
    return vz_launch_repack_logits(e->d_gather, out, rows, e->Vp, c.vocab, e->tp, s);
}

extern "C" int vz_comm_unique_id(char* out128) {
    VZ_CHECK_ARG(out128, "comm_unique_id: null buffer");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) { vz_set_error("ncclGetUniqueId failed: %s", ncclGetErrorString(r)); return VZ_ERR_HIP; }
    memcpy(out128, &id, 128);
    return VZ_OK;
}

extern "C" int vz_comm_init(vz_engine* e, const char* id128) {
    VZ_CHECK_ARG(e && id128, "comm_init: null argument");
    if (e->comm) return VZ_OK;
    ncclUniqueId id;
    memcpy(&id, id128, 128);
    ncclResult_t r = ncclCommInitRank(&e->comm, e->tp, id, e->rank);
    if (r != ncclSuccess) { e->comm = nullptr; vz_set_error("ncclCommInitRank failed: %s", ncclGetErrorString(r)); return VZ_ERR_HIP; }
    return VZ_OK;
}

extern "C" size_t vz_op_oneshot_area_bytes(int n_ranks, int max_elems) { return vz_oneshot_area_bytes(n_ranks, max_elems); }
extern "C" int vz_op_allreduce_oneshot(void* const* d_areas, int rank, int n_ranks, int max_elems, const void* d_in, void* d_out, int n, unsigned* d_seq,
                                       int* d_err, vz_stream stream) {
    return vz_launch_allreduce_oneshot(d_areas, rank, n_ranks, max_elems, (const bf16_t*)d_in, (bf16_t*)d_out, n, d_seq, d_err, (hipStream_t)stream);
}
// TEST FORM: the n_ranks ranks of one all-reduce as slices of ONE grid (one process, one GPU: co-resident whatever the stream / queue mapping)
extern "C" int vz_test_allreduce_oneshot_all(void* const* d_areas, int n_ranks, int max_elems, const void* const* d_in, void* const* d_out, int n,
                                             unsigned* const* d_seq, int* d_err, vz_stream stream) {
    return vz_launch_allreduce_oneshot_all(d_areas, n_ranks, max_elems, (const bf16_t* const*)d_in, (bf16_t* const*)d_out, n, d_seq, d_err, (hipStream_t)stream);
}
extern "C" int vz_comm_oneshot_local(vz_engine* e, void** out_area, size_t* out_bytes) {
    VZ_CHECK_ARG(e && out_area && out_bytes && e->tp >= 1, "comm_oneshot_local: bad argument");
    const size_t bytes = vz_oneshot_area_bytes(e->tp, vz_engine::OS_MAX_ELEMS);
    if (!e->os_area) {
        VZ_CHECK_HIP(hipMalloc(&e->os_area, bytes));
        VZ_CHECK_HIP(hipMemset(e->os_area, 0, bytes));
        VZ_CHECK_HIP(hipMalloc((void**)&e->os_seq, 2 * sizeof(unsigned)));
        const unsigned init[2] = {1u, 0u};                  // sequence numbers start at 1: a zero-filled area carries tag 0 = "nothing yet"
        VZ_CHECK_HIP(hipMemcpy(e->os_seq, init, sizeof(init), hipMemcpyHostToDevice));
    }
    *out_area = e->os_area; *out_bytes = bytes;
    return VZ_OK;
}
extern "C" int vz_comm_oneshot_attach(vz_engine* e, void* const* d_areas, int n_ranks) {
    VZ_CHECK_ARG(e && d_areas && n_ranks == e->tp && n_ranks <= 8 && e->os_area, "comm_oneshot_attach: needs tp_size areas after vz_comm_oneshot_local");
    VZ_CHECK_ARG(d_areas[e->rank] == e->os_area, "comm_oneshot_attach: area %d must be this rank's own", e->rank);
    RC(drop_decode_graph(e));
    for (int q = 0; q < n_ranks; ++q) { VZ_CHECK_ARG(d_areas[q], "comm_oneshot_attach: area %d missing", q); e->os_areas[q] = d_areas[q]; }
    e->os_ranks = n_ranks;
    return VZ_OK;
}

extern "C" int vz_tp_all_gather(vz_engine* e, const void* d_send, void* d_recv, size_t bytes_per_rank, vz_stream stream) {
    VZ_CHECK_ARG(e && d_send && d_recv && bytes_per_rank > 0, "tp_all_gather: bad argument");
    hipStream_t s = (hipStream_t)stream;
    if (tp_local(e)) { VZ_CHECK_HIP(hipMemcpyAsync(d_recv, d_send, bytes_per_rank, hipMemcpyDeviceToDevice, s)); return VZ_OK; }
    if (tp_skip(e)) {     // rehearsal: own chunk only
        VZ_CHECK_HIP(hipMemsetAsync(d_recv, 0, bytes_per_rank * e->tp, s));
        VZ_CHECK_HIP(hipMemcpyAsync((char*)d_recv + bytes_per_rank * e->rank, d_send, bytes_per_rank, hipMemcpyDeviceToDevice, s));
        return VZ_OK;
    }
    if (!e->comm) { vz_set_error("tensor-parallel engine used before vz_comm_init"); return VZ_ERR_STATE; }
    ProfScope ps(e, K_COMM, s);
    ncclResult_t r = ncclAllGather(d_send, d_recv, bytes_per_rank, ncclInt8, e->comm, s);
    if (r != ncclSuccess) { vz_set_error("ncclAllGather failed: %s", ncclGetErrorString(r)); return VZ_ERR_HIP; }
    return VZ_OK;
}

// ------------------------------------------------------------------------------------------------
// a12: Zephyr prefill and append prefill - T rows per sample through the decoder stack (llm_rows_forward)
// ------------------------------------------------------------------------------------------------
static bf16_t* kc_of(vz_engine* e, int layer) { return e->kv + (size_t)layer * e->kv_layer_elems; }
static bf16_t* vc_of(vz_engine* e, int layer) { return kc_of(e, layer) + e->kv_layer_elems / 2; }

// (re)build slots [0, h_len[i]) of cache rows h_row[i] in the e4m3 mirror from the bf16 cache, layers [layer0, layer0 + n_layers), and mark
// the rows valid (attn_decode_kv8.hip: kv8_mirror_rows_kernel, 64 rows per launch)
static int kv8_mirror(vz_engine* e, int layer0, int n_layers, const int* h_row, const int* h_len, int n, hipStream_t s) {
    const vz_config& c = e->c;
    const size_t half = e->kv_layer_elems / 2, l0 = (size_t)layer0 * e->kv_layer_elems;
    for (int i0 = 0; i0 < n; i0 += 64) {
        Kv8MirrorArgs a;
        a.src[0] = e->kv + l0; a.src[1] = e->kv + l0 + half;
        a.q[0] = e->kv8.q + l0; a.q[1] = e->kv8.q + l0 + half;
        a.sc[0] = e->kv8.sc + l0 / c.head_dim; a.sc[1] = e->kv8.sc + (l0 + half) / c.head_dim;
        a.layer_elems = e->kv_layer_elems; a.n_layers = n_layers; a.Hkv = e->Hkv_l; a.max_ctx = c.max_ctx; a.n = std::min(64, n - i0);
        for (int i = 0; i < a.n; ++i) { a.row[i] = h_row[i0 + i]; a.len[i] = h_len[i0 + i]; }
        RC(vz_launch_kv8_mirror_rows(a, s));
    }
    for (int i = 0; i < n; ++i) e->kv8.valid[h_row[i]] = 1;
    return VZ_OK;
}

static bool rows_shape_ok(const vz_config& c, int row0, int B, int T) { return B >= 1 && row0 >= 0 && row0 + B <= c.max_batch && T >= 1 && T <= c.max_ctx; }
// q8, qs: carve_prefill only; part, part_floats: carve_append only
struct RowsWs { bf16_t *x, *y, *qkv, *q, *att, *act; int* ints; bf16_t* ylast; unsigned char* q8 = nullptr; float* qs = nullptr; float* part = nullptr; size_t part_floats = 0; };
// what both carvings begin with; `tables` = the [B] int tables behind slot[rows]
static RowsWs carve_rows_head(Carver& m, const vz_config& c, const Shard& sh, int B, int T, int tables) {
    const size_t rows = (size_t)B * T, H = c.hidden, A = (size_t)sh.Hq * c.head_dim, QKV = (size_t)(sh.Hq + 2 * sh.Hkv) * c.head_dim, I = sh.I;
    RowsWs w;
    w.x = m.take<bf16_t>(rows * H);
    w.y = m.take<bf16_t>(rows * H);
    w.qkv = m.take<bf16_t>(rows * QKV);
    w.q = m.take<bf16_t>(rows * A);
    w.att = m.take<bf16_t>(rows * A);
    w.act = m.take<bf16_t>(rows * I);
    w.ints = m.take<int>(rows + (size_t)tables * B + 16);
    w.ylast = m.take<bf16_t>((size_t)B * H * 2);
    return w;
}
static RowsWs carve_prefill(Carver& m, const vz_config& c, const Shard& sh, int B, int S) {
    const size_t rows = (size_t)B * S, H = c.hidden, A = (size_t)sh.Hq * c.head_dim, I = sh.I;
    RowsWs w = carve_rows_head(m, c, sh, B, S, 1);                            // slot[rows] | kv_len[B]
    w.q8 = m.take<unsigned char>(rows * std::max(std::max(H, A), I));         // e4m3 copy of a linear's input rows + their scales
    w.qs = m.take<float>(rows);                                               // (fp8 MFMA prefill only)
    return w;
}
static RowsWs carve_append(Carver& m, const vz_config& c, const Shard& sh, int B, int T) {
    RowsWs w = carve_rows_head(m, c, sh, B, T, 3);                            // slot[rows] | kv_len[B] | past[B] | new[B]
    w.part_floats = vz_attn_append_ws_floats(B, T, sh.Hq, sh.Hkv, c.max_ctx);
    w.part = m.take<float>(w.part_floats);
    return w;
}

// the checks the two entry points share; `who` and `dim` keep each one's own error text
static int rows_entry_check(vz_engine* e, const char* who, char dim, bool pointers, int row0, int B, int T) {
    const vz_config& c = e->c;
    VZ_CHECK_ARG(pointers && rows_shape_ok(c, row0, B, T), "%s: rows %d..%d, %c=%d outside capacity (max_batch %d, max_ctx %d)", who, row0, row0 + B - 1, dim, T,
                 c.max_batch, c.max_ctx);
    VZ_CHECK_ARG(e->cosT && e->rope_max >= c.max_ctx, "%s: rotary tables not set or shorter than max_ctx", who);
    return VZ_OK;
}

// More new rows per sample than knob 36 (VZ_KNOB_APPEND_FLASH_MIN_T; tune.h has the measurement) run the append on the prefill's flash
// kernel with a scalar q_pos0, once per run of cache rows with equal past; at or below it the key-split kernel of attn_append.hip.

// One call: T embed rows per sample; sample b's first h_new[b] rows are valid and go behind the h_past[b] positions cache row row0 + b
// keeps (slots past + t).  The plain prefill is the call with past = 0 everywhere.
struct RowsCall {
    int row0, B, T;
    const int *h_new, *h_past, *d_pos;
    const void* d_embeds;
    float *d_logits_all, *d_logits_last;
    hipStream_t s;
};

static int llm_rows_forward(vz_engine* e, const RowsWs& w, const RowsCall& k, bool append) {
    const vz_config& c = e->c;
    hipStream_t s = k.s;
    const int B = k.B, T = k.T, rows = B * T;
    const int H = c.hidden, D = c.head_dim, Hq = e->Hq_l, Hkv = e->Hkv_l, QKV = (Hq + 2 * Hkv) * D, I = e->I_l, A = Hq * D;
    const size_t row_elems = (size_t)Hkv * c.max_ctx * D;                         // cache rows are [kv head][max_ctx][128] blocks
    const size_t row_off = (size_t)k.row0 * row_elems;
    const bool lead = e->rank == 0;   // the row-parallel partial sums carry the residual on one rank only
    bf16_t *x = w.x, *y = w.y, *qkv = w.qkv, *q = w.q, *att = w.att, *act = w.act, *ylast = w.ylast;
    // The attention, chosen once: the key-split kernel (short appends), or flash launches over runs of cache rows with equal past.  The
    // plain prefill is one such run at past 0, and the only one whose flash launch may rotate Q in its own load (knob 33; the
    // others read the rotated copy q that rope_kv writes).
    const bool keysplit = append && !(T > vz_knob(VZ_KNOB_APPEND_FLASH_MIN_T));
    const bool rope_q_late = !append && vz_knob(VZ_KNOB_ROPE_IN_ATTN) && D == 128 && vz_knob(VZ_KNOB_ATTN_VERSION) != 1;
    int* d_slot = w.ints;
    int* d_len = w.ints + rows;
    int kv_max = 0;
    bool padded = false;
    std::vector<int> kv8_row(B), kv8_len(B);      // the e4m3 mirror on: every layer rebuilds slots [0, past + new) of the rows this call touches
    for (int b = 0; b < B; ++b) { kv8_row[b] = k.row0 + b; kv8_len[b] = k.h_past[b] + k.h_new[b]; }
    {
        std::vector<int> h(rows + (keysplit ? 3 : 1) * B);          // slot[rows] | kv_len[B], and for the key-split kernel | past[B] | new[B]
        for (int b = 0; b < B; ++b) {
            for (int t = 0; t < T; ++t) h[b * T + t] = t < k.h_new[b] ? k.h_past[b] + t : -1;
            h[rows + b] = k.h_past[b] + k.h_new[b];
            if (keysplit) { h[rows + B + b] = k.h_past[b]; h[rows + 2 * B + b] = k.h_new[b]; }
            kv_max = std::max(kv_max, h[rows + b]);
            padded = padded || k.h_new[b] < T;
        }
        RC(upload_ints(e, h.data(), h.size(), w.ints, s));
    }
    // one linear of the stack: bf16 tile GEMM, or - weight_fp8 engine with vz_engine_prefill_fp8 on - the input rows quantised to e4m3
    // (one power-of-two scale per row) and the product on the fp8 MFMA against the e4m3 weight copy (gemm_fp8.hip)
    // (below ~768 rows the quantiser launches and the shallow grids cost more than the fp8 MFMA saves: 330 rows 20.4 vs 18.6 ms, 1320 rows 37.5 vs 43.6)
    // The plain prefill only: carve_append takes no q8 / qs, and nobody has measured or tested an append on the fp8 route - on a
    // prefill_fp8 engine it keeps the bf16 linears.
    const bool f8 = !append && e->prefill_fp8 && rows >= vz_knob(VZ_KNOB_FP8_PREFILL_MIN_ROWS) && tp_local(e) && vz_gemm_fp8_ok(rows, QKV, H, H, H) && vz_gemm_fp8_ok(rows, H, I, I, I) && vz_gemm_fp8_ok(rows, H, A, A, A);
    // norm_w != null: Ain is the residual stream and the RMSNorm belongs to this linear (fp8: norm + quantiser in one launch)
    auto plin = [&](const bf16_t* Ain, const float* norm_w, const LinW& W, int N, int K, void* Cout, int ldc, const bf16_t* res, int act) -> int {
        if (f8) {
            {
                ProfScope ps(e, K_NORM, s);
                if (norm_w) RC(vz_launch_rmsnorm_quant_fp8(Ain, K, norm_w, c.rms_eps, w.q8, K, w.qs, rows, K, s));
                else RC(vz_launch_quant_rows_fp8(Ain, K, w.q8, K, w.qs, rows, K, s));
            }
            Fp8LinearArgs f;
            f.A8 = w.q8; f.lda = K; f.ascale = w.qs; f.W8 = W.w8; f.ldw = K; f.wscale = W.ws; f.C = Cout; f.ldc = ldc; f.M = rows; f.N = N; f.K = K;
            f.bias = nullptr; f.residual = res; f.ldr = H; f.act = act; f.out_fp32 = 0;
            ProfScope ps(e, K_GEMM, s);
            return vz_launch_gemm_fp8(f, s);
        }
        if (norm_w) { ProfScope ps(e, K_NORM, s); RC(vz_launch_rmsnorm(Ain, K, y, K, norm_w, rows, K, c.rms_eps, s)); }
        return linear(e, 0, norm_w ? y : Ain, K, bare(W.w), K, Cout, ldc, rows, N, K, res, H, act, 0, s);      // (the bf16 matrix only: prefill never streams the e4m3 copy)
    };
    // token rows >= new[b] are never written by the key-split kernel in any layer: keep what the O projection reads of them finite
    if (padded && keysplit) VZ_CHECK_HIP(hipMemsetAsync(att, 0, (size_t)rows * A * sizeof(bf16_t), s));
    { ProfScope ps(e, K_OTHER, s); RC(vz_launch_copy_rows((const bf16_t*)k.d_embeds, H, x, H, rows, H, s)); }
    for (int i = 0; i < c.n_layers; ++i) {
        const LlmLayerW& W = e->llm[i];
        bf16_t *kc = kc_of(e, i) + row_off, *vc = vc_of(e, i) + row_off;
        RC(plin(x, W.in_norm, W.qkv, QKV, H, qkv, QKV, nullptr, VZ_ACT_NONE));
        // RoPE of K + the KV append at slot past + t; the rotated copy q of the queries unless the attention rotates them in its own load
        { ProfScope ps(e, K_OTHER, s); RC(vz_launch_rope_kv(qkv, QKV, rope_q_late ? nullptr : q, kc, vc, e->cosT, e->sinT, k.d_pos, d_slot, B, T, Hq, Hkv, D, c.max_ctx, s)); }
        if (e->kv8.on) { ProfScope ps(e, K_OTHER, s); RC(kv8_mirror(e, i, 1, kv8_row.data(), kv8_len.data(), B, s)); }
        if (keysplit) {
            ProfScope ps(e, K_ATTN, s);
            AttnAppendArgs a;
            a.q = q; a.kc = kc; a.vc = vc; a.o = att; a.part = w.part; a.part_floats = w.part_floats;
            a.past = d_len + B; a.nnew = d_len + 2 * B;
            a.B = B; a.T = T; a.Hq = Hq; a.Hkv = Hkv; a.head_dim = D; a.max_ctx = c.max_ctx; a.window = c.sliding_window; a.kv_max = kv_max; a.nsplit = 0;
            a.q_bs = a.o_bs = (long)T * A; a.q_ss = a.o_ss = A; a.q_hs = a.o_hs = D;
            a.scale = ATTN_SCALE;
            RC(vz_launch_attention_append(a, s));
        } else {
            ProfScope ps(e, K_ATTN, s);
            const bf16_t* qsrc = rope_q_late ? qkv : q;
            const long q_ld = rope_q_late ? QKV : A;
            for (int b0 = 0; b0 < B;) {
                int b1 = b0 + 1;
                while (b1 < B && k.h_past[b1] == k.h_past[b0]) ++b1;
                AttnArgs a;
                a.q = qsrc + (size_t)b0 * T * q_ld; a.k = kc + b0 * row_elems; a.v = vc + b0 * row_elems; a.o = att + (size_t)b0 * T * A;
                a.B = b1 - b0; a.Sq = T; a.Sk = std::min(k.h_past[b0] + T, c.max_ctx); a.Hq = Hq; a.Hkv = Hkv; a.head_dim = D;
                a.q_bs = T * q_ld; a.q_ss = q_ld; a.q_hs = D;
                if (rope_q_late) { a.rope_cos = e->cosT; a.rope_sin = e->sinT; a.rope_pos = k.d_pos; }      // (one run: b0 = 0)
                a.k_bs = a.v_bs = (long)row_elems; a.k_ss = a.v_ss = D; a.k_hs = a.v_hs = (long)c.max_ctx * D;
                a.o_bs = (long)T * A; a.o_ss = A; a.o_hs = D;
                a.scale = ATTN_SCALE;
                a.causal = 1; a.q_pos0 = k.h_past[b0]; a.window = c.sliding_window; a.kv_len = d_len + b0;
                RC(vz_launch_attention(a, s));
                b0 = b1;
            }
        }
        RC(plin(att, nullptr, W.o, H, A, x, H, lead ? x : nullptr, VZ_ACT_NONE));
        RC(tp_allreduce_bf16(e, x, (size_t)rows * H, s));
        RC(plin(x, W.post_norm, W.gu, 2 * I, H, act, I, nullptr, VZ_ACT_SWIGLU));
        RC(plin(act, nullptr, W.down, H, I, x, H, lead ? x : nullptr, VZ_ACT_NONE));
        RC(tp_allreduce_bf16(e, x, (size_t)rows * H, s));
    }
    const float* fn = e->top.norm;
    if (k.d_logits_all) {
        { ProfScope ps(e, K_NORM, s); RC(vz_launch_rmsnorm(x, H, y, H, fn, rows, H, c.rms_eps, s)); }
        RC(lm_head_logits(e, y, rows, k.d_logits_all, s, nullptr));
    }
    if (k.d_logits_last) {
        {
            ProfScope ps(e, K_OTHER, s);
            for (int b = 0; b < B; ++b) RC(vz_launch_copy_rows(x + ((size_t)b * T + k.h_new[b] - 1) * H, H, ylast + (size_t)b * H, H, 1, H, s));
        }
        { ProfScope ps(e, K_NORM, s); RC(vz_launch_rmsnorm(ylast, H, ylast + (size_t)B * H, H, fn, B, H, c.rms_eps, s)); }
        RC(lm_head_logits(e, ylast + (size_t)B * H, B, k.d_logits_last, s, nullptr));
    }
    return VZ_OK;
}

extern "C" int vz_llm_prefill(vz_engine* e, const void* d_embeds, int B, int S, const int* h_seqlens, const int* d_pos,
                              float* d_logits_all, float* d_logits_last, vz_stream stream) {
    return vz_llm_prefill_rows(e, 0, d_embeds, B, S, h_seqlens, d_pos, d_logits_all, d_logits_last, stream);
}

// the same prefill into KV-cache rows row0 .. row0 + B - 1 (continuous batching: a new request enters a free row while the
// other rows keep their context)
extern "C" int vz_llm_prefill_rows(vz_engine* e, int row0, const void* d_embeds, int B, int S, const int* h_seqlens, const int* d_pos,
                                   float* d_logits_all, float* d_logits_last, vz_stream stream) {
    NEED_READY();
    RC(rows_entry_check(e, "prefill", 'S', d_embeds && h_seqlens && d_pos, row0, B, S));
    for (int b = 0; b < B; ++b) VZ_CHECK_ARG(h_seqlens[b] >= 1 && h_seqlens[b] <= S, "prefill: seqlen[%d]=%d outside [1,%d]", b, h_seqlens[b], S);
    const std::vector<int> past(B, 0);
    RowsWs w;
    RC(carve_stage(e, "prefill", [&](Carver& m) { return carve_prefill(m, e->c, Shard{e->Hq_l, e->Hkv_l, e->I_l}, B, S); }, &w));
    return llm_rows_forward(e, w, RowsCall{row0, B, S, h_seqlens, past.data(), d_pos, d_embeds, d_logits_all, d_logits_last, (hipStream_t)stream}, false);
}

// append prefill: T new rows per cache row behind the positions the row keeps
extern "C" int vz_llm_prefill_append(vz_engine* e, int row0, const void* d_embeds, int B, int T, const int* h_new, const int* h_past, const int* d_pos,
                                     float* d_logits_all, float* d_logits_last, vz_stream stream) {
    NEED_READY();
    const vz_config& c = e->c;
    // (llm_rows_forward holds the all-reduces and the lead-rank residual of the plain prefill, but no test has run an append through them)
    if (e->tp > 1) { vz_set_error("prefill_append: the append prefill on a tensor-parallel engine is not built"); return VZ_ERR_UNSUPPORTED; }
    RC(rows_entry_check(e, "prefill_append", 'T', d_embeds && h_new && h_past && d_pos, row0, B, T));
    for (int b = 0; b < B; ++b) {
        VZ_CHECK_ARG(h_new[b] >= 1 && h_new[b] <= T, "prefill_append: new[%d]=%d outside [1,%d]", b, h_new[b], T);
        VZ_CHECK_ARG(h_past[b] >= 0 && h_past[b] <= c.max_ctx - h_new[b], "prefill_append: past[%d]=%d + new %d outside max_ctx %d", b, h_past[b], h_new[b], c.max_ctx);
    }
    RowsWs w;
    RC(carve_stage(e, "prefill_append", [&](Carver& m) { return carve_append(m, c, Shard{e->Hq_l, e->Hkv_l, e->I_l}, B, T); }, &w));
    return llm_rows_forward(e, w, RowsCall{row0, B, T, h_new, h_past, d_pos, d_embeds, d_logits_all, d_logits_last, (hipStream_t)stream}, true);
}

// ------------------------------------------------------------------------------------------------
// a13: greedy decode
// ------------------------------------------------------------------------------------------------
static bool decode_shape_ok(const vz_config& c, int B, bool spec) { return B >= 1 && B <= c.max_batch && B <= 64 && (!spec || (B >= 2 && B <= 8)); }
struct DecodeWs { bf16_t *x, *qkv, *att, *act, *q_rot; };
// spec: the speculative tail's verify steps keep the rotated queries of their R = B rows
static DecodeWs carve_decode(Carver& m, const vz_config& c, const Shard& sh, int B, bool spec) {
    const size_t A = (size_t)sh.Hq * c.head_dim;
    DecodeWs w;
    w.x = m.take<bf16_t>((size_t)B * c.hidden);
    w.qkv = m.take<bf16_t>((size_t)B * (sh.Hq + 2 * sh.Hkv) * c.head_dim);
    w.att = m.take<bf16_t>(B * A);
    w.act = m.take<bf16_t>((size_t)B * sh.I);
    w.q_rot = spec ? m.take<bf16_t>(B * A) : nullptr;
    return w;
}

extern "C" int vz_llm_decode_begin(vz_engine* e, int B, const int* d_first_ids, const int* h_next_pos, const int* h_ctx_len,
                                   vz_stream stream) {
    NEED_READY();
    const vz_config& c = e->c;
    hipStream_t s = (hipStream_t)stream;
    VZ_CHECK_ARG(decode_shape_ok(c, B, false) && d_first_ids && h_next_pos && h_ctx_len, "decode_begin: B=%d unsupported (1..min(64,max_batch))", B);
    VZ_CHECK_ARG(!e->share.on || B == e->share.groups * e->share.n, "decode_begin: the shared-prefix attention (vz_llm_decode_share) is armed for %d x %d rows, "
                 "the batch has %d", e->share.groups, e->share.n, B);
    const int mb = c.max_batch;
    std::vector<int> h(DecodeState::ints(mb), 0);       // host image of the state: everything behind `cur` goes up in one copy
    const DecodeState hs = decode_state(h.data(), mb), ds = decode_state(e->d_state, mb);
    for (int b = 0; b < B; ++b) {
        VZ_CHECK_ARG(h_ctx_len[b] >= 0 && h_ctx_len[b] < c.max_ctx, "decode_begin: ctx_len[%d]=%d outside [0,%d)", b, h_ctx_len[b], c.max_ctx);
        if (e->kv8.on && h_ctx_len[b] > 0 && !e->kv8.valid[b]) {
            vz_set_error("decode_begin: row %d has %d cached positions but no e4m3 mirror of them (vz_engine_kv_fp8 is on: prefill the row, or move KV "
                         "into it, after enabling)", b, h_ctx_len[b]);
            return VZ_ERR_STATE;
        }
        hs.pos[b] = h_next_pos[b];
        hs.slot[b] = h_ctx_len[b];         // slot the next token is written to
        hs.len[b] = h_ctx_len[b] + 1;      // keys visible to the next token
    }
    *hs.ctr = e->samp.rec.ctr; hs.seed[0] = e->samp.rec.seed[0]; hs.seed[1] = e->samp.rec.seed[1];      // (step = 0)
    for (size_t r = 0; r < e->rows.tab.size(); ++r) hs.samp[r] = e->rows.tab[r];            // (never set: zeros = every row greedy)
    RC(upload_ints(e, hs.pos, h.size() - mb, ds.pos, s));
    VZ_CHECK_HIP(hipMemcpyAsync(ds.cur, d_first_ids, B * sizeof(int), hipMemcpyDeviceToDevice, s));
    if (e->score.d_slot) VZ_CHECK_HIP(hipMemsetAsync(e->score.d_slot, 0, sizeof(int), s));      // the step recorder's ring restarts with the batch
    e->dec_B = B;
    e->spec.on = 0;          // a new batch starts with the plain tail: vz_llm_decode_spec is armed AFTER this call
    e->spec.a.samp = ROW_GREEDY;      // ... and its sampling record (vz_llm_decode_spec_sampling) behind that
    e->h_len.assign(B, 0); e->h_pos.assign(B, 0); e->h_parked.assign(B, 0);
    for (int b = 0; b < B; ++b) { e->h_len[b] = h_ctx_len[b] + 1; e->h_pos[b] = h_next_pos[b]; e->h_parked[b] = h_ctx_len[b] == 0 && h_next_pos[b] == 0; }
    return VZ_OK;
}

// Continuous batching: (re)arm ONE row of a running decode batch - its next input token, rotary position and context length -
// without touching the other rows or the step counter.  A finished row is parked the same way (any token, position 0, context
// 0): it keeps stepping harmlessly inside its own cache row until a new request is prefilled into it (vz_llm_prefill_rows).
extern "C" int vz_llm_decode_set_row(vz_engine* e, int row, int token, int next_pos, int ctx_len, vz_stream stream) {
    NEED_READY();
    const vz_config& c = e->c;
    VZ_CHECK_ARG(e->dec_B >= 1 && row >= 0 && row < e->dec_B, "decode_set_row: row %d outside the running batch of %d", row, e->dec_B);
    VZ_CHECK_ARG(ctx_len >= 0 && ctx_len < c.max_ctx && next_pos >= 0, "decode_set_row: ctx_len %d / pos %d outside [0,%d)", ctx_len, next_pos, c.max_ctx);
    // shared-prefix attention armed: the slots [0, shared) of a group are its first row's - a row set in front of them would append into them
    VZ_CHECK_ARG(!e->share.on || (row < e->share.groups * e->share.n && ctx_len >= e->share.h_shared[row / e->share.n]),
                 "decode_set_row: row %d to context %d, in front of the %d slots its group shares (vz_llm_decode_share is armed: a row is neither parked nor "
                 "moved into the shared slots)", row, ctx_len, e->share.on && row < e->share.groups * e->share.n ? e->share.h_shared[row / e->share.n] : 0);
    if (e->kv8.on && ctx_len > 0 && !e->kv8.valid[row]) {
        vz_set_error("decode_set_row: row %d has %d cached positions but no e4m3 mirror of them (vz_engine_kv_fp8 is on: prefill the row, or move KV "
                     "into it, after enabling)", row, ctx_len);
        return VZ_ERR_STATE;
    }
    const DecodeState ds = decode_state(e->d_state, c.max_batch);
    const int h[DecodeState::ROW_ARRAYS] = {token, next_pos, ctx_len, ctx_len + 1};     // cur | pos | slot | len: one int in each of the four state arrays
    e->h_len[row] = ctx_len + 1; e->h_pos[row] = next_pos; e->h_parked[row] = ctx_len == 0 && next_pos == 0;
    hipStream_t s = (hipStream_t)stream;
    VZ_CHECK_ARG(e->h_pinned && e->h_pinned_ints >= DecodeState::ROW_ARRAYS, "decode_set_row: no staging buffer (vz_llm_decode_begin allocates it)");
    VZ_CHECK_HIP(hipStreamSynchronize(s));                        // previous use of the staging buffer has drained
    memcpy(e->h_pinned, h, sizeof(h));
    // a 4-row x 4-byte strided copy: row k lands in state array k at column `row`
    VZ_CHECK_HIP(hipMemcpy2DAsync(ds.cur + row, (size_t)(ds.pos - ds.cur) * sizeof(int), e->h_pinned, sizeof(int), sizeof(int), DecodeState::ROW_ARRAYS,
                                  hipMemcpyHostToDevice, s));
    return VZ_OK;
}

// Batched admissions: several requests are prefilled TOGETHER into spare cache rows (rows the running decode batch does not use,
// vz_llm_prefill_rows with row0 >= the batch size) and then moved to whichever rows have come free - the first h_len[i] cache
// positions of row h_src[i] to row h_dst[i], all layers, one launch per 16 moves, stream-ordered behind the prefill.
extern "C" int vz_llm_kv_move_rows(vz_engine* e, int n, const int* h_src, const int* h_dst, const int* h_len, vz_stream stream) {
    NEED_READY();
    VZ_CHECK_ARG(n >= 1 && h_src && h_dst && h_len, "kv_move_rows: bad argument");
    const vz_config& c = e->c;
    for (int i = 0; i < n; ++i) {
        VZ_CHECK_ARG(h_src[i] >= 0 && h_src[i] < c.max_batch && h_dst[i] >= 0 && h_dst[i] < c.max_batch && h_len[i] >= 0 && h_len[i] <= c.max_ctx,
                     "kv_move_rows: move %d (row %d -> row %d, %d positions) outside the cache (max_batch %d, max_ctx %d)", i, h_src[i], h_dst[i], h_len[i], c.max_batch, c.max_ctx);
        // a row of the running decode batch may only be read or overwritten while it is parked: moving into a live row would replace
        // the keys that row keeps attending to
        VZ_CHECK_ARG(h_src[i] >= e->dec_B || e->h_parked[h_src[i]], "kv_move_rows: source row %d belongs to the running decode batch", h_src[i]);
        VZ_CHECK_ARG(h_dst[i] >= e->dec_B || e->h_parked[h_dst[i]], "kv_move_rows: destination row %d is a live row of the running decode batch (park it first)", h_dst[i]);
        VZ_CHECK_ARG(!e->share.on || h_dst[i] >= e->share.groups * e->share.n || h_dst[i] % e->share.n != 0, "kv_move_rows: destination row %d holds the slots its group "
                     "shares (vz_llm_decode_share is armed)", h_dst[i]);
    }
    for (int i0 = 0; i0 < n; i0 += 16) {
        KvMoves mv;
        mv.n = std::min(16, n - i0);
        for (int i = 0; i < mv.n; ++i) { mv.src[i] = h_src[i0 + i]; mv.dst[i] = h_dst[i0 + i]; mv.len[i] = h_len[i0 + i]; }
        int r = vz_launch_kv_move_rows(e->kv, e->kv_layer_elems, c.n_layers, c.max_batch, e->Hkv_l, c.max_ctx, c.head_dim, mv, (hipStream_t)stream);
        if (r) return r;
        // the e4m3 mirror of the destination rows: re-quantised from the moved bf16 rows, every layer (the mirror is a function of the cache)
        if (e->kv8.on) RC(kv8_mirror(e, 0, c.n_layers, mv.dst, mv.len, mv.n, (hipStream_t)stream));
    }
    return VZ_OK;
}

// the logits processors' buffer (vz_engine::proc.d): the rows' history lengths, how many ids of each history were seeded before generation
// began (vz_llm_decode_logits_proc_seed; 0 otherwise), then the histories [max_batch][max_ctx]
static size_t proc_len_ints(const vz_config& c) { return align_up((size_t)c.max_batch, 64); }
static int* proc_base(const vz_engine* e) { return e->proc.d + proc_len_ints(e->c); }
static int* proc_hist(const vz_engine* e) { return e->proc.d + 2 * proc_len_ints(e->c); }
// the stop matcher's per-row count of ids its ring was seeded with (vz_llm_decode_stop_seed): behind the rows' states
static int* stop_pre(const vz_engine* e) { return e->stop.d_state + (size_t)e->c.max_batch * VZ_STOP_ROW; }
// the per-row stop sequences (vz_llm_decode_stop_row_seqs): the rows' regions, then the rows' counts; null while the mode is off
static constexpr size_t STOP_REGION_INTS = (size_t)VZ_STOP_MAX_SEQ * VZ_STOP_SEQ_STRIDE;
static const int* stop_row_seq(const vz_engine* e, int row0 = 0) { return e->stop.rows_on ? e->stop.d_rowseq + row0 * STOP_REGION_INTS : nullptr; }
static const int* stop_row_nseq(const vz_engine* e, int row0 = 0) { return e->stop.rows_on ? e->stop.d_rowseq + e->c.max_batch * STOP_REGION_INTS + row0 : nullptr; }
static bool stop_armed(const vz_engine* e) { return e->stop.on || e->stop.rows_on; }
// the id-sequence table of sequence_bias / bad_words_ids as the entry points take it (vz_common.h: ProcArgs)
static int proc_seq_check(const int* h_seq, int n_seq) {
    VZ_CHECK_ARG(n_seq >= 0 && n_seq <= VZ_PROC_MAX_SEQ && (n_seq == 0 || h_seq), "logits_proc: 0..%d id sequences expected, got %d", VZ_PROC_MAX_SEQ, n_seq);
    for (int k = 0; k < n_seq; ++k) {
        const int* q = h_seq + (size_t)k * VZ_PROC_SEQ_STRIDE;
        VZ_CHECK_ARG(q[0] >= 1 && q[0] <= VZ_PROC_SEQ_IDS && (q[1] == 0 || q[1] == 1), "logits_proc: id sequence %d of %d ids (1..%d), kind %d (0 = bias, 1 = bad word)",
                     k, q[0], VZ_PROC_SEQ_IDS, q[1]);
        for (int j = 0; j < q[0]; ++j) VZ_CHECK_ARG(q[4 + j] >= 0, "logits_proc: id sequence %d holds the negative id %d", k, q[4 + j]);
    }
    return VZ_OK;
}
// the one check of a processor record (include/viszephyr.h: vz_logits_proc_params), its id-sequence table included: what the kernel
// takes by value (seq_epoch is the business of whoever owns the table's device memory)
static int proc_args_of(const vz_logits_proc_params& p, ProcArgs* out) {
    VZ_CHECK_ARG(p.repetition_penalty > 0.f && p.no_repeat_ngram >= 0 && p.no_repeat_ngram <= 8 && p.min_new_tokens >= 0, "logits_proc: repetition penalty %g > 0, "
                 "0 <= n-gram size %d <= 8, min_new_tokens %d >= 0 expected", (double)p.repetition_penalty, p.no_repeat_ngram, p.min_new_tokens);
    VZ_CHECK_ARG(p.n_eos >= 0 && p.n_eos <= 4 && (p.n_eos == 0 || p.eos), "logits_proc: 0..4 eos ids expected, got %d", p.n_eos);
    VZ_CHECK_ARG(p.n_suppress >= 0 && p.n_suppress <= 16 && (p.n_suppress == 0 || p.suppress), "logits_proc: 0..16 suppressed ids expected, got %d", p.n_suppress);
    RC(proc_seq_check(p.seq, p.n_seq));
    memset(out, 0, sizeof(*out));
    out->penalty = p.repetition_penalty; out->ngram = p.no_repeat_ngram; out->min_new = p.min_new_tokens; out->eos.n = p.n_eos;
    out->n_suppress = p.n_suppress; out->n_seq = p.n_seq;
    for (int i = 0; i < 4; ++i) out->eos.id[i] = i < p.n_eos ? p.eos[i] : -1;
    for (int i = 0; i < 16; ++i) out->suppress[i] = i < p.n_suppress ? p.suppress[i] : -1;
    return VZ_OK;
}

// the accept + draft launch of the armed speculative mode on the step's argmax ids g [R]; g = null: only the first draft (arming)
static int launch_spec_tail(vz_engine* e, const int* g, hipStream_t s) {
    const SpecArgs& a = e->spec.a;
    const DecodeState st = decode_state(e->d_state, e->c.max_batch);
    SpecTailArgs t;
    t.g = g; t.cur = st.cur; t.draft = st.cur + 1; t.pos = st.pos; t.slot = st.slot; t.len = st.len; t.ctl = a.ctl; t.out = a.out; t.budget = a.budget;
    t.hist = a.hist; t.hist_cap = a.hist_cap; t.stats = g ? a.stats : nullptr; t.stats_cap = g ? a.stats_cap : 0;
    t.stream = a.stream; t.stream_len = a.stream_len; t.eos = a.eos; t.R = e->spec.R; t.max_ngram = a.ngram; t.source = a.source;
    t.max_ctx = e->c.max_ctx; t.rope_max = e->rope_max; t.do_accept = g != nullptr; t.do_draft = 1;
    return vz_launch_spec_tail(t, s);
}

// one decode step, all launches on `s`; every quantity that changes between steps lives in device memory.  `w` = carve_decode over the
// arena vz_llm_decode_steps sized with the same function (nothing may grow inside a capture)
static int decode_step_launch(vz_engine* e, const DecodeWs& w, int* d_out_ids, int out_stride, float* d_logits_dbg, hipStream_t s) {
    const vz_config& c = e->c;
    const int B = e->dec_B;
    const int H = c.hidden, D = c.head_dim, Hq = e->Hq_l, Hkv = e->Hkv_l, QKV = (Hq + 2 * Hkv) * D, I = e->I_l, A = Hq * D;
    const bool lead = e->rank == 0;
    const DecodeState st = decode_state(e->d_state, c.max_batch);
    const TailKind tail = tail_kind(e);
    const bool spec = tail == TAIL_SPEC;
    bf16_t *x = w.x, *qkv = w.qkv, *att = w.att, *act = w.act, *q_rot = w.q_rot;
    if (e->use_tok && e->tok) {
        // batch 1 on an MI355X: embedding row -> 32 layers -> logits as the phases of ONE resident grid (decode_persist.hip); same
        // arithmetic as the launches below, bit for bit
        VzTokArgs a;
        a.embed = e->top.embed; a.lm_head = e->top.lm_head.w; a.final_norm = e->top.norm;
        a.cur = st.cur; a.pos = st.pos; a.slot = st.slot; a.step = st.step;
        a.logits = e->d_logits; a.part = e->d_part; a.ticket = e->d_ticket; a.cosT = e->cosT; a.sinT = e->sinT; a.err = e->d_ferr;
        a.vocab = c.vocab; a.max_ctx = c.max_ctx; a.nsplit = e->dec_nsplit; a.window = c.sliding_window; a.scale = ATTN_SCALE; a.eps = c.rms_eps;
        e->last_stream = s;
        ProfScope ps(e, K_GEMV, s);
        RC(vz_launch_decode_token(e->tok, a, s));
    } else {
        { ProfScope ps(e, K_OTHER, s); RC(vz_launch_embed_tokens(st.cur, B, H, e->top.embed, x, s)); }
        for (int i = 0; i < c.n_layers; ++i) {
            const LlmLayerW& W = e->llm[i];
            const bool fuse_ao = !spec && !e->share.on && !e->kv8.on && vz_knob(VZ_KNOB_ATTN_O) && (B == 1 || (B == 2 && vz_knob(VZ_KNOB_ATTN_O) >= 1 && 2 * e->dec_nsplit <= 32)) && e->tp == 1 && tp_local(e) && H == 4096 && A == 4096 && Hq == 32 && Hkv == 8 &&
                                 D == 128 && e->dec_nsplit <= 32 && e->d_ao_done;
            RC(linear(e, 1, x, H, W.qkv, H, qkv, QKV, B, QKV, H, nullptr, 0, VZ_ACT_NONE, 0, s, W.in_norm, c.rms_eps));
            if (spec) {
                // verify step (spec.hip): the B rows are consecutive positions of ONE sequence - RoPE + append of all of them to cache row 0
                // (the stand-alone kernel: its bits), then one pass over that row for all B x 32 query heads
                ProfScope ps(e, K_ATTN_DEC, s);
                RC(vz_launch_rope_kv(qkv, QKV, q_rot, kc_of(e, i), vc_of(e, i), e->cosT, e->sinT, st.pos, st.slot, 1, B, Hq, Hkv, D, c.max_ctx, s));
                SpecVerifyArgs a;
                a.q = q_rot; a.kc = kc_of(e, i); a.vc = vc_of(e, i); a.o = att; a.part = e->d_part; a.ticket = e->d_ticket; a.slot = st.slot;
                a.R = B; a.Hq = Hq; a.Hkv = Hkv; a.max_ctx = c.max_ctx; a.nsplit = e->dec_nsplit; a.key_bound = e->spec.a.key_bound;
                a.window = c.sliding_window; a.scale = ATTN_SCALE;
                RC(vz_launch_spec_verify_attn(a, s));
            } else if (e->share.on) {
                // shared-prefix step (attn_shared.hip): RoPE + append of every row to its own cache row (the stand-alone
                // kernel), one stacked pass per group over the slots its rows share, then each row's own slots and the merge
                ProfScope ps(e, K_ATTN_DEC, s);
                RC(vz_launch_rope_kv(qkv, QKV, e->share.q_rot, kc_of(e, i), vc_of(e, i), e->cosT, e->sinT, st.pos, st.slot, B, 1, Hq, Hkv, D, c.max_ctx, s));
                AttnSharedArgs a;
                a.q = e->share.q_rot; a.kc = kc_of(e, i); a.vc = vc_of(e, i); a.o = att; a.part = e->share.ws; a.part_floats = e->share.ws_floats;
                a.shared = e->share.d_tab; a.slot = st.slot;
                a.R = B; a.n = e->share.n; a.Hq = Hq; a.Hkv = Hkv; a.head_dim = D; a.max_ctx = c.max_ctx; a.window = c.sliding_window;
                a.shared_max = e->share.shared_max; a.nsplit = 0; a.scale = ATTN_SCALE;
                RC(vz_launch_attention_shared(a, s));
            } else if (e->kv8.on) {
                // the e4m3 mirror on (attn_decode_kv8.hip): the same step with the cached slots read from the mirror, for
                // every batch size; the new row goes to the bf16 cache and to the mirror
                ProfScope ps(e, K_ATTN_DEC, s);
                const size_t l0 = (size_t)i * e->kv_layer_elems, half = e->kv_layer_elems / 2;
                AttnDecodeKv8Args a;
                a.qkv = qkv; a.kc = kc_of(e, i); a.vc = vc_of(e, i); a.o = att; a.part = e->d_part; a.ticket = e->d_ticket;
                a.k8 = e->kv8.q + l0; a.v8 = e->kv8.q + l0 + half; a.ks = e->kv8.sc + l0 / D; a.vs = e->kv8.sc + (l0 + half) / D;
                a.cosT = e->cosT; a.sinT = e->sinT; a.pos = st.pos; a.slot = st.slot;
                a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.D = D; a.max_ctx = c.max_ctx; a.nsplit = std::min(e->dec_nsplit, 32); a.window = c.sliding_window;
                a.scale = ATTN_SCALE;
                RC(vz_launch_attn_decode_kv8(a, s));
            } else {
                ProfScope ps(e, K_ATTN_DEC, s);
                AttnDecodeFusedArgs a;
                a.qkv = qkv; a.kc = kc_of(e, i); a.vc = vc_of(e, i); a.o = att; a.part = e->d_part; a.ticket = e->d_ticket;
                a.cosT = e->cosT; a.sinT = e->sinT; a.pos = st.pos; a.slot = st.slot;
                a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.D = D; a.max_ctx = c.max_ctx; a.nsplit = e->dec_nsplit; a.window = c.sliding_window;
                a.scale = ATTN_SCALE;
                if (fuse_ao) {
                    // batch 1 (round 3): the O projection's workgroups ride in the attention's grid and stream their weights under its latency
                    // chain (attn_o_fused.hip); same arithmetic as the two launches, bit for bit (a weight_fp8 engine: the e4m3 rows +
                    // scales, as linear() would take them)
                    RC(vz_launch_attn_o_fused(a, W.o.w, W.o.w8, W.o.ws, att, x, e->d_ao_done, st.step, i, c.n_layers, e->d_ferr, s));
                } else {
                    RC(vz_launch_attn_decode_fused(a, s));
                }
            }
            if (!fuse_ao) RC(linear(e, 1, att, A, W.o, A, x, H, B, H, A, lead ? x : nullptr, H, VZ_ACT_NONE, 0, s));
            RC(tp_allreduce_bf16(e, x, (size_t)B * H, s, true));
            RC(linear(e, 1, x, H, W.gu, H, act, I, B, 2 * I, H, nullptr, 0, VZ_ACT_SWIGLU, 0, s, W.post_norm, c.rms_eps));
            RC(linear(e, 1, act, I, W.down, I, x, H, B, H, I, lead ? x : nullptr, H, VZ_ACT_NONE, 0, s));
            RC(tp_allreduce_bf16(e, x, (size_t)B * H, s, true));
        }
        RC(lm_head_logits(e, x, B, e->d_logits, s, e->top.norm));
    }
    if (d_logits_dbg) {
        // debug copy is indexed by the host (eager mode only)
        VZ_CHECK_HIP(hipMemcpyAsync(d_logits_dbg, e->d_logits, (size_t)B * c.vocab * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    {
        ProfScope ps(e, K_OTHER, s);
        // a guided batch (vz_llm_decode_guidance): the model part above ran on 2 * pairs rows, everything from here on sees the first
        // `pairs` of them - the conditional rows, whose logits cfg_combine turns into the guided scores in front of everything else
        const int rows_model = B;
        const int B = e->cfg.on ? e->cfg.pairs : rows_model;      // (shadows the batch size on purpose: nothing below may touch the other rows)
        // per row: the token into d_out_ids (and the ring), position / slot / length one further
        const RowEmit emit{st.pos, st.slot, st.len, d_out_ids, out_stride, st.step, c.max_ctx, e->rope_max, e->ring.p, e->ring.n};
        if (e->score.what & VZ_SCORE_RAW) RC(vz_launch_score_raw_rows(e->d_logits, B, c.vocab, e->score.raw, e->score.d_slot, e->score.cap, s));
        // guidance.hip: row r <- scale * (log_softmax(row r) - log_softmax(row pairs + r)) + log_softmax(row pairs + r), HF's first processor
        if (e->cfg.on) RC(vz_launch_cfg_combine(e->d_logits, e->d_logits + (size_t)B * c.vocab, B, c.vocab, e->cfg.scale, s));
        // the beam tail with processors or with its processed rows recorded: the logits become log-prob rows in place first, as HF
        // hands log_softmax rows to the processors there; otherwise the fused select takes the logits as they are
        const BeamRowsArgs& br = e->beam.rows;
        const bool beam_lp = tail == TAIL_BEAM && (e->proc.on || br.scores);
        if (tail == TAIL_BEAM && br.raw) RC(vz_launch_score_raw_rows(e->d_logits, B, c.vocab, br.raw, beam_view(e->beam.d).hidx, br.cap, s));
        if (beam_lp) RC(vz_launch_beam_logprob_rows(e->d_logits, B, c.vocab, e->d_logits, s));
        if (e->proc.on && tail_takes_proc(tail)) {
            // logits_proc.hip: st.cur still holds the token the previous tail published - the kernel appends it to the row's history itself
            RC(vz_launch_logits_process(e->d_logits, B, c.vocab, proc_hist(e), c.max_ctx, e->proc.d, st.cur, e->proc.a, e->proc.a.n_seq ? e->proc.d_seq : nullptr, s, proc_base(e)));
        }
        // the per-row form: every row by its own record; a row whose record is inactive is left alone
        if (e->proc.rows_on) RC(vz_launch_logits_process_rows(e->d_logits, B, c.vocab, proc_hist(e), c.max_ctx, e->proc.d, st.cur, e->proc.d_rows, e->proc.d_rowseq, proc_base(e), s));
        if (beam_lp && br.scores) RC(vz_launch_score_raw_rows(e->d_logits, B, c.vocab, br.scores, beam_view(e->beam.d).hidx, br.cap, s));
        switch (tail) {
        case TAIL_SPEC: {
            // spec.hip: per-row argmax - or, with a sampling record armed, per-row draw at the counter of the row's position in the generated
            // sequence (sampling.hip: spec_sample_kernel) - then acceptance + state advance (its own, multi-row rule) + the next step's draft
            // in one small launch
            int* g = e->spec.a.ctl + VZ_SPEC_CTL_IDS;
            if (e->spec.a.samp.mode == VZ_ROW_SAMPLE) RC(vz_launch_spec_sample(e->d_logits, B, c.vocab, e->spec.a.samp, e->spec.a.ctl, g, s));
            else RC(vz_launch_argmax(e->d_logits, B, c.vocab, g, {}, s));
            RC(launch_spec_tail(e, g, s));
            break;
        }
        case TAIL_BEAM: {
            // beam.hip: select, then the KV of rows whose parent is another row follows the parent (and, with processors, the row's id
            // history does: the processor kernel appends the row's own token to it at the next step), then the history index
            const BeamArgs& a = e->beam.a;
            const BeamView v = beam_view(e->beam.d);
            RC(vz_launch_beam_select(e->d_logits, a.nb * a.groups, c.vocab, a.nb, a.nb, a.eos, v.score, v.cand_s, v.cand_t, a.hist, v.hidx, a.hist_cap,
                                     st.cur, v.score, v.parent, emit, beam_lp, s));
            RC(vz_launch_kv_beam_reorder(e->kv, e->kv_layer_elems, c.n_layers, c.max_batch, e->Hkv_l, c.max_ctx, c.head_dim, a.nb, a.groups,
                                         v.parent, v.base, a.nb, st.slot, a.nb, s));
            if (e->proc.on) RC(vz_launch_hist_beam_reorder(e->proc.d, proc_hist(e), c.max_ctx, a.nb, a.groups, v.parent, s));
            RC(vz_launch_beam_advance(v.hidx, s));
            break;
        }
        case TAIL_ROWS:
            RC(vz_launch_sample_rows(e->d_logits, B, c.vocab, st.samp, st.cur, emit, s));
            break;
        case TAIL_SAMPLE:
            RC(vz_launch_sample(e->d_logits, B, c.vocab, e->samp.rec.temp, e->samp.rec.top_k, e->samp.rec.top_p, e->samp.rec.warp, st.seed, st.ctr, 0, st.cur, emit, s));
            break;
        case TAIL_GREEDY:
            RC(vz_launch_argmax(e->d_logits, B, c.vocab, st.cur, emit, s));
            break;
        }
        if (e->score.what) {
            // sampling.hip: the record of the token the tail just left in st.cur, by the parameters the tail took it with
            RC(vz_launch_token_scores(e->d_logits, B, c.vocab, tail == TAIL_ROWS ? st.samp : nullptr, tail == TAIL_SAMPLE ? e->samp.rec : ROW_GREEDY, st.cur, e->score.rec,
                                      (e->score.what & VZ_SCORE_WARPED) ? e->score.warped : nullptr, e->score.d_slot, e->score.cap, s));
        }
        // stop.hip: the token the tail just left in st.cur through the rows' stop conditions (writes its own state only)
        if (stop_armed(e)) { ProfScope pm(e, K_OTHER, s); RC(vz_launch_stop_match(e->stop.a, e->stop.d_state, B, st.cur, 0, s, stop_pre(e), stop_row_seq(e), stop_row_nseq(e))); }      // (its own profiling scope: one more counted launch)
        // guidance.hip: the unconditional rows take the tokens the conditional rows just chose and move on as they did
        if (e->cfg.on) RC(vz_launch_cfg_follow(st.cur, st.pos, st.slot, st.len, B, c.max_ctx, e->rope_max, s));
        RC(vz_launch_step_advance(st.step, e->score.what ? e->score.d_slot : nullptr, s));
    }
    return VZ_OK;
}

// The one check of a sampler record (include/viszephyr.h: vz_sample_params).  The checked, normalised copy is what the kernels read: an entry
// of the per-row table, the sampler's arguments, the recorder's `one`.  A greedy record becomes the canonical greedy entry with its counter,
// its other fields neither checked nor kept.
static int row_sample_of(const vz_sample_params& p, RowSample* out) {
    VZ_CHECK_ARG((p.mode == VZ_ROW_GREEDY || p.mode == VZ_ROW_SAMPLE) && p.counter >= 0, "row sampling: mode %d (0 = greedy, 1 = sample), counter %d >= 0 expected", p.mode, p.counter);
    *out = ROW_GREEDY; out->ctr = p.counter;
    if (p.mode == VZ_ROW_GREEDY) return VZ_OK;
    // (written so that a NaN fails)
    VZ_CHECK_ARG(p.temperature > 0.f && p.top_k >= 0 && p.top_p > 0.f && p.top_p <= 1.f,
                 "row sampling: temperature %g > 0, top_k %d >= 0, 0 < top_p %g <= 1 expected", (double)p.temperature, p.top_k, (double)p.top_p);
    VZ_CHECK_ARG(p.min_p >= 0.f && p.min_p <= 1.f && p.typical_p >= 0.f && p.epsilon_cutoff >= 0.f && p.eta_cutoff >= 0.f,
                 "sampling warpers: 0 <= min_p %g <= 1, typical_p %g >= 0, epsilon_cutoff %g >= 0, eta_cutoff %g >= 0 expected", (double)p.min_p,
                 (double)p.typical_p, (double)p.epsilon_cutoff, (double)p.eta_cutoff);
    // HF's off values arm nothing: typical_p >= 1, a cutoff outside (0, 1)
    const auto off_at_1 = [](float v) { return v < 1.f ? v : 0.f; };
    *out = RowSample{VZ_ROW_SAMPLE, p.temperature, p.top_k, p.top_p, {(unsigned)p.seed, (unsigned)(p.seed >> 32)}, p.counter, 0,
                     {p.min_p, off_at_1(p.typical_p), off_at_1(p.epsilon_cutoff), off_at_1(p.eta_cutoff)}};
    return VZ_OK;
}
// `rows` <= 64 records of an op-level call, checked, as a table in this (device, stream)'s own scratch
static int row_samples_to_device(const char* who, const vz_sample_params* h_rows, int rows, hipStream_t s, RowSample** d_tab) {
    VZ_CHECK_ARG(h_rows, "row sampling: null parameter array");
    RowSample tab[64];
    for (int r = 0; r < rows; ++r) RC(row_sample_of(h_rows[r], tab + r));
    void* p = nullptr; size_t have = 0;
    RC(vz_stream_ws(6, s, sizeof(tab), false, &p, &have));
    VZ_CHECK_ARG(p && have >= sizeof(tab), "%s: first use of a stream inside a capture (call it once before capturing)", who);
    VZ_CHECK_HIP(hipMemcpyAsync(p, tab, (size_t)rows * sizeof(RowSample), hipMemcpyHostToDevice, s));
    VZ_CHECK_HIP(hipStreamSynchronize(s));          // the table is on this frame: it has been read before the call returns
    *d_tab = (RowSample*)p;
    return VZ_OK;
}

// every arming of the matcher starts with no row watched (stream-ordered behind the steps of an earlier arming): a row is matched from its
// vz_llm_decode_stop_rows on, never from what an earlier call left in its state
static int stop_state_unwatched(vz_engine* e, hipStream_t s) {
    const int mb = e->c.max_batch;
    if (!e->stop.d_state) {
        e->stop.h_init.assign((size_t)mb * VZ_STOP_ROW + mb, 0);          // the rows' states, then the rows' seeded-id counts (stop_pre)
        for (int r = 0; r < mb; ++r) e->stop.h_init[(size_t)r * VZ_STOP_ROW + 1] = VZ_STOP_UNARMED;
        VZ_CHECK_HIP(hipMalloc((void**)&e->stop.d_state, e->stop.h_init.size() * sizeof(int)));
    }
    VZ_CHECK_HIP(hipMemcpyAsync(e->stop.d_state, e->stop.h_init.data(), e->stop.h_init.size() * sizeof(int), hipMemcpyHostToDevice, s));
    return VZ_OK;
}
static int stop_seq_check(const char* who, const int* h_seq, int n_seq) {
    VZ_CHECK_ARG(n_seq == 0 || h_seq, "%s: id sequences without their table", who);
    for (int k = 0; k < n_seq; ++k)
        VZ_CHECK_ARG(h_seq[k * VZ_STOP_SEQ_STRIDE] >= 1 && h_seq[k * VZ_STOP_SEQ_STRIDE] <= VZ_STOP_MAX_SEQ_LEN && h_seq[k * VZ_STOP_SEQ_STRIDE + 1] >= 0,
                     "%s: id sequence %d of %d ids from %d (1..%d ids, start >= 0)", who, k, h_seq[k * VZ_STOP_SEQ_STRIDE], h_seq[k * VZ_STOP_SEQ_STRIDE + 1], VZ_STOP_MAX_SEQ_LEN);
    return VZ_OK;
}

// The stop matcher (stop.hip: stop_match_kernel): armed, every decode step whose tail is the argmax, the sampler or the
// per-row tail passes, behind that tail (and the recorder) and inside the per-token hipGraph, the token each row just chose through the
// row's stop conditions and records the index of the token at which one first held.  The tables are copied into the engine's own device
// memory here, outside any capture; a row is watched from vz_llm_decode_stop_rows on.  enable = 0: off.
extern "C" int vz_llm_decode_stop(vz_engine* e, int enable, const int* h_emb, int emb_rows, int vec, int n_str, int max_pos, int max_end, int window,
                                  const int* h_target, const int* h_seq, int n_seq, vz_stream stream) {
    NEED_READY();
    VZ_CHECK_ARG(!e->stop.rows_on, "decode_stop: the per-row stop sequences are armed over the call-level set (vz_llm_decode_stop_row_seqs(0) first)");
    if (!enable) { e->stop.on = 0; memset(&e->stop.a, 0, sizeof(e->stop.a)); return VZ_OK; }
    if (e->tp > 1) { vz_set_error("decode_stop: the stop matcher on a tensor-parallel engine is not built"); return VZ_ERR_UNSUPPORTED; }
    VZ_CHECK_ARG(n_str >= 0 && n_str <= VZ_STOP_MAX_STR && n_seq >= 0 && n_seq <= VZ_STOP_MAX_SEQ && n_str + n_seq >= 1,
                 "decode_stop: %d stop strings (0..%d), %d id sequences (0..%d), at least one of either", n_str, VZ_STOP_MAX_STR, n_seq, VZ_STOP_MAX_SEQ);
    VZ_CHECK_ARG(n_str == 0 || (h_emb && h_target && emb_rows >= 1 && emb_rows <= (1 << 22) && vec == n_str * (max_pos + max_end) + 1 && max_pos >= 1 &&
                                max_pos <= VZ_STOP_MAX_POS && max_end >= 1 && max_end <= VZ_STOP_MAX_END && window >= 1 && window <= VZ_STOP_W),
                 "decode_stop: stop-string tables outside the matcher's limits (rows %d, vec %d, max_valid_positions %d <= %d, max_valid_end_lens %d <= %d, "
                 "maximum_token_len %d <= %d)", emb_rows, vec, max_pos, VZ_STOP_MAX_POS, max_end, VZ_STOP_MAX_END, window, VZ_STOP_W);
    RC(stop_seq_check("decode_stop", h_seq, n_seq));
    hipStream_t s = (hipStream_t)stream;
    RC(stop_state_unwatched(e, s));
    const size_t emb_ints = n_str ? (size_t)emb_rows * vec : 0, tgt_ints = VZ_STOP_MAX_STR, seq_ints = (size_t)VZ_STOP_MAX_SEQ * VZ_STOP_SEQ_STRIDE;
    const size_t need = emb_ints + tgt_ints + seq_ints;
    std::vector<int> tab(need, 0);                  // [emb | target | seq], as the device holds it
    if (emb_ints) memcpy(tab.data(), h_emb, emb_ints * sizeof(int));
    for (int i = 0; i < n_str; ++i) tab[emb_ints + i] = h_target[i];
    if (n_seq) memcpy(tab.data() + emb_ints + tgt_ints, h_seq, (size_t)n_seq * VZ_STOP_SEQ_STRIDE * sizeof(int));
    // the stop set of the previous arming again (a serving loop that calls generate() per request): the device holds these tables already -
    // no synchronise, no upload
    if (!(e->stop.d_tab && tab == e->stop.h_tab)) {
        VZ_CHECK_HIP(hipStreamSynchronize(s));      // steps still in flight read the tables of the previous stop set
        if (need > e->stop.tab_ints) {
            if (e->stop.d_tab) { VZ_CHECK_HIP(hipFree(e->stop.d_tab)); e->stop.d_tab = nullptr; e->stop.tab_ints = 0; e->stop.h_tab.clear(); }
            VZ_CHECK_HIP(hipMalloc((void**)&e->stop.d_tab, need * sizeof(int)));
            e->stop.tab_ints = need;
        }
        VZ_CHECK_HIP(hipMemcpy(e->stop.d_tab, tab.data(), need * sizeof(int), hipMemcpyHostToDevice));
        e->stop.h_tab.swap(tab);
    }
    StopArgs a;
    memset(&a, 0, sizeof(a));
    a.emb = n_str ? e->stop.d_tab : nullptr; a.target = e->stop.d_tab + emb_ints; a.seq = e->stop.d_tab + emb_ints + tgt_ints;
    a.n_str = n_str; a.n_seq = n_seq;
    if (n_str) { a.emb_rows = emb_rows; a.vec = vec; a.max_pos = max_pos; a.max_end = max_end; a.window = window; }
    e->stop.a = a; e->stop.on = 1;
    return VZ_OK;
}

// rows [row0, row0 + rows) start clean and their first tokens (chosen from the prefill logits, outside the step) go through the step's own
// kernel: one implementation, no host mirror
extern "C" int vz_llm_decode_stop_rows(vz_engine* e, int row0, int rows, const int* d_first_ids, vz_stream stream) {
    NEED_READY();
    VZ_CHECK_ARG(stop_armed(e), "decode_stop_rows: the stop matcher is off (vz_llm_decode_stop)");
    VZ_CHECK_ARG(row0 >= 0 && rows >= 1 && row0 + rows <= e->c.max_batch && d_first_ids, "decode_stop_rows: rows [%d, %d) outside max_batch = %d", row0, row0 + rows, e->c.max_batch);
    return vz_launch_stop_match(e->stop.a, e->stop.d_state + (size_t)row0 * VZ_STOP_ROW, rows, d_first_ids, 1, (hipStream_t)stream, stop_pre(e) + row0,
                                stop_row_seq(e, row0), stop_row_nseq(e, row0));
}

// Per-row stop sequences: rule 2 of the matcher by row.  Arming fills every row's region with the call-level
// sequences of the armed matcher (none when it is off) and starts, as every arming does, with no row watched.
extern "C" int vz_llm_decode_stop_row_seqs(vz_engine* e, int enable, vz_stream stream) {
    NEED_READY();
    if (!enable) { e->stop.rows_on = 0; e->stop.h_call.clear(); return VZ_OK; }
    if (e->tp > 1) { vz_set_error("decode_stop_row_seqs: the stop matcher on a tensor-parallel engine is not built"); return VZ_ERR_UNSUPPORTED; }
    hipStream_t s = (hipStream_t)stream;
    const int mb = e->c.max_batch, n_call = e->stop.on ? e->stop.a.n_seq : 0;
    RC(stop_state_unwatched(e, s));
    if (!e->stop.d_rowseq) VZ_CHECK_HIP(hipMalloc((void**)&e->stop.d_rowseq, (mb * STOP_REGION_INTS + mb) * sizeof(int)));
    // the call-level sequences as the armed matcher holds them: the tail of its table image [emb | target | seq]
    e->stop.h_call.assign(STOP_REGION_INTS, 0);
    if (n_call) memcpy(e->stop.h_call.data(), e->stop.h_tab.data() + (e->stop.h_tab.size() - STOP_REGION_INTS), (size_t)n_call * VZ_STOP_SEQ_STRIDE * sizeof(int));
    std::vector<int> img(mb * STOP_REGION_INTS + mb, 0);
    for (int r = 0; r < mb; ++r) {
        memcpy(img.data() + r * STOP_REGION_INTS, e->stop.h_call.data(), STOP_REGION_INTS * sizeof(int));
        img[mb * STOP_REGION_INTS + r] = n_call;
    }
    RC(upload_ints(e, img.data(), img.size(), e->stop.d_rowseq, s));
    e->stop.rows_on = 1;
    return VZ_OK;
}

extern "C" int vz_llm_decode_stop_set_row_seqs(vz_engine* e, int row, const int* h_seq, int n_seq, vz_stream stream) {
    NEED_READY();
    VZ_CHECK_ARG(e->stop.rows_on, "decode_stop_set_row_seqs: the per-row stop sequences are off (vz_llm_decode_stop_row_seqs)");
    const int n_call = e->stop.on ? e->stop.a.n_seq : 0;
    VZ_CHECK_ARG(row >= 0 && row < e->c.max_batch && n_seq >= 0 && n_call + n_seq <= VZ_STOP_MAX_SEQ, "decode_stop_set_row_seqs: row %d outside max_batch = %d, or %d "
                 "call-level + %d own id sequences, more than %d", row, e->c.max_batch, n_call, n_seq, VZ_STOP_MAX_SEQ);
    RC(stop_seq_check("decode_stop_set_row_seqs", h_seq, n_seq));
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> img(e->stop.h_call);                                 // the call-level sequences in front of the row's own
    if (n_seq) memcpy(img.data() + (size_t)n_call * VZ_STOP_SEQ_STRIDE, h_seq, (size_t)n_seq * VZ_STOP_SEQ_STRIDE * sizeof(int));
    const int total = n_call + n_seq;
    RC(upload_ints(e, img.data(), img.size(), e->stop.d_rowseq + row * STOP_REGION_INTS, s));
    return upload_ints(e, &total, 1, e->stop.d_rowseq + e->c.max_batch * STOP_REGION_INTS + row, s);
}

// Seeds row `row`'s ring with the last ids that were fed before generation begins (a call that continues on a kept cache), newest last:
// a stop string may then begin in them, as it may in the tail of HF's input_ids; the id sequences (rule 2) still look at generated ids
// only.  Behind the arming (which clears every row), in front of vz_llm_decode_stop_rows (which keeps the ring); stream-ordered.
extern "C" int vz_llm_decode_stop_seed(vz_engine* e, int row, const int* h_ids, int n, vz_stream stream) {
    NEED_READY();
    VZ_CHECK_ARG(stop_armed(e) && e->stop.d_state, "decode_stop_seed: the stop matcher is off (vz_llm_decode_stop)");
    VZ_CHECK_ARG(row >= 0 && row < e->c.max_batch && n >= 0 && (h_ids || n == 0), "decode_stop_seed: row %d outside max_batch = %d, or %d ids", row, e->c.max_batch, n);
    int img[VZ_STOP_W + 1] = {0};
    const int k = std::min(n, VZ_STOP_W - 1);
    for (int j = 0; j < k; ++j) img[VZ_STOP_W - 1 - j] = h_ids[n - 1 - j];          // the first generated token takes slot 0, its predecessor is slot 63
    img[VZ_STOP_W] = k;
    RC(upload_ints(e, img, VZ_STOP_W, e->stop.d_state + (size_t)row * VZ_STOP_ROW + 2, (hipStream_t)stream));
    return upload_ints(e, img + VZ_STOP_W, 1, stop_pre(e) + row, (hipStream_t)stream);
}

// at[row0 .. row0 + rows) -> d_at (device), stream-ordered behind the steps: rides with the chunk's ids at the host's sync
extern "C" int vz_llm_decode_stop_read(vz_engine* e, int row0, int rows, int* d_at, vz_stream stream) {
    NEED_READY();
    VZ_CHECK_ARG(e->stop.d_state, "decode_stop_read: the stop matcher was never armed (vz_llm_decode_stop)");
    VZ_CHECK_ARG(row0 >= 0 && rows >= 1 && row0 + rows <= e->c.max_batch && d_at, "decode_stop_read: rows [%d, %d) outside max_batch = %d", row0, row0 + rows, e->c.max_batch);
    VZ_CHECK_HIP(hipMemcpy2DAsync(d_at, sizeof(int), e->stop.d_state + (size_t)row0 * VZ_STOP_ROW + 1, VZ_STOP_ROW * sizeof(int), sizeof(int), rows,
                                  hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return VZ_OK;
}

// the kernel on caller-owned state and device tables, one new id per row (tests)
extern "C" int vz_op_stop_match(int* d_state, int rows, const int* d_ids, int reset, const int* d_emb, int emb_rows, int vec, int n_str, int max_pos,
                                int max_end, int window, const int* d_target, const int* d_seq, int n_seq, vz_stream stream) {
    StopArgs a;
    memset(&a, 0, sizeof(a));
    a.emb = d_emb; a.target = d_target; a.seq = d_seq; a.emb_rows = emb_rows; a.vec = vec; a.n_str = n_str; a.max_pos = max_pos; a.max_end = max_end;
    a.window = window; a.n_seq = n_seq;
    return vz_launch_stop_match(a, d_state, rows, d_ids, reset, (hipStream_t)stream);
}

// The step recorder (sampling.hip: token_scores_kernel): armed, every decode step whose tail is the argmax, the
// sampler or the per-row tail writes, behind that tail and inside the per-token hipGraph, one record {x_tok, lse, lse_kept, n_kept} per
// row about the token it chose, and on request the warped score rows and the raw logits rows (copied in front of the processors), into
// rings of cap_steps steps in the caller's device memory.  The slot is a device-side count of the steps launched since
// vz_llm_decode_begin (restarted here too, stream-ordered), so a replayed graph takes no per-step argument.  what = 0: off.
extern "C" int vz_llm_decode_scores(vz_engine* e, unsigned what, float* d_rec, float* d_warped, float* d_raw, int cap_steps, vz_stream stream) {
    NEED_READY();
    if (!what) { e->score.what = 0; e->score.rec = e->score.warped = e->score.raw = nullptr; e->score.cap = 0; return VZ_OK; }
    if (e->tp > 1) { vz_set_error("decode_scores: the step recorder on a tensor-parallel engine is not built"); return VZ_ERR_UNSUPPORTED; }
    VZ_CHECK_ARG((what & VZ_SCORE_REC) && !(what & ~(VZ_SCORE_REC | VZ_SCORE_WARPED | VZ_SCORE_RAW)) && d_rec && cap_steps >= 1,
                 "decode_scores: what = %u needs VZ_SCORE_REC, a record ring and cap_steps %d >= 1", what, cap_steps);
    VZ_CHECK_ARG((!(what & VZ_SCORE_WARPED) || d_warped) && (!(what & VZ_SCORE_RAW) || d_raw), "decode_scores: a requested row output has no ring");
    hipStream_t s = (hipStream_t)stream;
    if (!e->score.d_slot) VZ_CHECK_HIP(hipMalloc((void**)&e->score.d_slot, 64));
    VZ_CHECK_HIP(hipMemsetAsync(e->score.d_slot, 0, sizeof(int), s));
    e->score.what = what; e->score.rec = d_rec; e->score.cap = cap_steps;
    e->score.warped = (what & VZ_SCORE_WARPED) ? d_warped : nullptr; e->score.raw = (what & VZ_SCORE_RAW) ? d_raw : nullptr;
    return VZ_OK;
}

// the same kernel on fp32 logits [rows <= 64, cols] about the tokens d_ids [rows] (int32), row r by the record h_rows[r] as
// vz_op_sample_rows takes it: d_rec [rows][4], d_warped [rows][cols] or null (the first token's record, taken from the prefill logits; tests)
extern "C" int vz_op_token_scores(const float* d_logits, int rows, int cols, const int* d_ids, const vz_sample_params* h_rows, float* d_rec,
                                  float* d_warped, vz_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    VZ_CHECK_ARG(d_logits && d_ids && d_rec && rows >= 1 && rows <= 64 && cols >= 1, "token_scores: bad argument (1..64 rows)");
    RowSample* tab = nullptr;
    RC(row_samples_to_device("token_scores", h_rows, rows, s, &tab));
    return vz_launch_token_scores(d_logits, rows, cols, tab, ROW_GREEDY, d_ids, d_rec, d_warped, nullptr, 0, s);
}

// Sampling instead of argmax as the tail of every decode step (hf:generation/utils.py `_sample`, do_sample=True; see sampling.hip) by a
// VZ_ROW_SAMPLE record: temperature, top_k (HF's default 50 is the caller's business), top_p, the warpers, a 64-bit seed and the draw
// counter the NEXT vz_llm_decode_begin starts from (the caller drew token 0 from the prefill logits with vz_op_sample and counter 0,
// so it passes 1).  A VZ_ROW_GREEDY record: greedy.
extern "C" int vz_llm_decode_sampling(vz_engine* e, const vz_sample_params* p) {
    VZ_CHECK_ARG(e && p, "decode_sampling: null engine / record");
    RowSample r;
    RC(row_sample_of(*p, &r));
    // (the draw counter also indexes the host-visible token ring of a greedy streamer loop)
    if (r.mode == VZ_ROW_GREEDY) { e->samp.on = 0; e->samp.rec.ctr = r.ctr; return VZ_OK; }
    e->samp.on = 1; e->samp.rec = r;
    return VZ_OK;
}

// The per-row tail: every row of the decode batch chooses its next token by its own entry of a table in device memory (sampling.hip:
// sample_rows_kernel) - greedy, or sampled with its own temperature / top-k / top-p, 64-bit seed and draw counter.  Rows are independent
// requests (continuous batching) or the n samples of one prompt.
// enable = 1: the tail of every decode step is the per-row kernel, and the NEXT vz_llm_decode_begin uploads these `rows` entries (the rows
// behind them greedy, rows = 0: every row greedy until vz_llm_decode_set_row_sampling arms it).
// The table is device memory the captured step reads through a pointer: a changed entry needs no new graph.  enable = 0: off.
extern "C" int vz_llm_decode_sampling_rows(vz_engine* e, int enable, int rows, const vz_sample_params* h_rows) {
    VZ_CHECK_ARG(e, "decode_sampling_rows: null engine");
    if (!enable) { e->rows.on = 0; e->rows.tab.clear(); return VZ_OK; }
    if (e->tp > 1) { vz_set_error("decode_sampling_rows: the per-row tail on a tensor-parallel engine is not built"); return VZ_ERR_UNSUPPORTED; }
    VZ_CHECK_ARG(rows >= 0 && rows <= e->c.max_batch, "decode_sampling_rows: %d rows outside [0, max_batch = %d]", rows, e->c.max_batch);
    VZ_CHECK_ARG(rows == 0 || h_rows, "row sampling: null parameter array");
    std::vector<RowSample> tab((size_t)e->c.max_batch, ROW_GREEDY);
    for (int r = 0; r < rows; ++r) RC(row_sample_of(h_rows[r], &tab[r]));
    e->rows.tab.swap(tab);
    e->rows.on = 1;
    return VZ_OK;
}

// The sampling counterpart of vz_llm_decode_set_row: one row's entry of the running batch, stream-ordered, the other rows untouched.
extern "C" int vz_llm_decode_set_row_sampling(vz_engine* e, int row, const vz_sample_params* p, vz_stream stream) {
    NEED_READY();
    VZ_CHECK_ARG(p && e->dec_B >= 1 && row >= 0 && row < e->dec_B, "decode_set_row_sampling: row %d outside the running batch of %d", row, e->dec_B);
    RowSample rs;
    RC(row_sample_of(*p, &rs));
    hipStream_t s = (hipStream_t)stream;
    VZ_CHECK_ARG(e->h_pinned && e->h_pinned_ints >= (size_t)DecodeState::SAMPLE_INTS, "decode_set_row_sampling: no staging buffer (vz_llm_decode_begin allocates it)");
    VZ_CHECK_HIP(hipStreamSynchronize(s));                        // previous use of the staging buffer has drained
    memcpy(e->h_pinned, &rs, sizeof(rs));
    VZ_CHECK_HIP(hipMemcpyAsync(decode_state(e->d_state, e->c.max_batch).samp + row, e->h_pinned, sizeof(rs), hipMemcpyHostToDevice, s));
    return VZ_OK;
}

// one token per row of fp32 logits [rows, cols] with the per-row kernel, rows <= 64 (the first tokens of sampled sequences, drawn from
// the prefill logits with counter 0; tests).  The table goes through this (device, stream)'s own scratch.
extern "C" int vz_op_sample_rows(const float* d_logits, int rows, int cols, const vz_sample_params* h_rows, int* d_ids, vz_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    VZ_CHECK_ARG(d_logits && d_ids && rows >= 1 && rows <= 64 && cols >= 1, "sample_rows: bad argument (1..64 rows)");
    RowSample* tab = nullptr;
    RC(row_samples_to_device("sample_rows", h_rows, rows, s, &tab));
    return vz_launch_sample_rows(d_logits, rows, cols, tab, d_ids, {}, s);
}

// Streamer / stopping-criteria path: besides d_out_ids every step's tail also writes its token to ring[row * ring_n + (draw
// counter mod ring_n)], a DEVICE-VISIBLE HOST buffer (hipHostMalloc / pinned), so the host can keep a step or two in flight and
// read token t as soon as the event recorded behind step t fires, without a device-to-host copy per token.  NULL = off.
extern "C" int vz_llm_decode_ring(vz_engine* e, int* ring, int ring_n, int ring_rows) {
    VZ_CHECK_ARG(e && (!ring || (ring_n >= 2 && ring_rows >= 1)), "decode_ring: ring_n >= 2 slots and ring_rows >= 1 rows expected");
    e->ring.p = ring; e->ring.n = ring ? ring_n : 0; e->ring.rows = ring ? ring_rows : 0;
    return VZ_OK;
}

// one draw per row of fp32 logits [rows, cols] with the sampler's kernel, every row by the one VZ_ROW_SAMPLE record (the first token of a
// sampled generation; tests)
extern "C" int vz_op_sample(const float* d_logits, int rows, int cols, const vz_sample_params* p, int* d_ids, vz_stream stream) {
    // [counter, seed lo, seed hi, -] in this (device, stream)'s own scratch words: launches on other streams or devices have theirs
    hipStream_t s = (hipStream_t)stream;
    VZ_CHECK_ARG(d_logits && d_ids && p && rows >= 1 && cols >= 1, "sample: bad argument");
    RowSample r;
    RC(row_sample_of(*p, &r));
    VZ_CHECK_ARG(r.mode == VZ_ROW_SAMPLE, "sample: a VZ_ROW_SAMPLE record expected (greedy: vz_op_argmax)");
    int* d_scratch = nullptr;
    { void* p = nullptr; size_t have = 0; int r = vz_stream_ws(4, s, 64, true, &p, &have); if (r) return r;
      VZ_CHECK_ARG(p && have >= 16, "sample: first use of a stream inside a capture (call it once before capturing)"); d_scratch = (int*)p; }
    VZ_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)d_scratch, r.ctr, 1, s));
    VZ_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(d_scratch + 1), (int)r.seed[0], 1, s));
    VZ_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(d_scratch + 2), (int)r.seed[1], 1, s));
    return vz_launch_sample(d_logits, rows, cols, r.temp, r.top_k, r.top_p, r.warp, (const unsigned*)(d_scratch + 1), d_scratch, 0, d_ids, {}, s);
}

// Logits processors in the step (hf:generation/logits_process.py; logits_proc.hip): after
// vz_llm_decode_logits_proc(enable=1) every decode step whose tail is the argmax or the sampler first runs repetition penalty (1 = off),
// no-repeat-n-gram (0 = off), min-new-tokens (the eos ids at -inf while fewer ids were generated) and suppress-tokens on its logits, over
// the ids generated so far: each row's history lives on the device, restarts empty here (stream-ordered) and grows by the row's input
// token at every step.  The mode is orthogonal to the tail; vz_llm_decode_steps refuses it together with the speculative tail.  With the
// beam tail the kernel runs on the log-prob rows, as HF's processors do there.  The id sequences of HF's
// sequence_bias / bad_words_ids are copied into the engine's own device memory here, outside any capture; the table of the previous
// arming again: nothing is uploaded.  p = null: off.
extern "C" int vz_llm_decode_logits_proc(vz_engine* e, const vz_logits_proc_params* p, vz_stream stream) {
    NEED_READY();
    if (!p) { e->proc.on = 0; return VZ_OK; }
    const vz_config& c = e->c;
    if (e->tp > 1) { vz_set_error("decode_logits_proc: logits processors on a tensor-parallel engine are not built"); return VZ_ERR_UNSUPPORTED; }
    VZ_CHECK_ARG(!e->proc.rows_on, "decode_logits_proc: the per-row logits processors are armed (vz_llm_decode_logits_proc_rows): one of the two forms at a time");
    ProcArgs a;
    RC(proc_args_of(*p, &a));
    VZ_CHECK_ARG(c.vocab <= 65536, "decode_logits_proc: vocabulary of %d, the kernel's bitmaps hold 65536", c.vocab);
    hipStream_t s = (hipStream_t)stream;
    if (!e->proc.d) VZ_CHECK_HIP(hipMalloc((void**)&e->proc.d, (2 * proc_len_ints(c) + (size_t)c.max_batch * c.max_ctx) * sizeof(int)));
    VZ_CHECK_HIP(hipMemsetAsync(e->proc.d, 0, 2 * proc_len_ints(c) * sizeof(int), s));
    if (a.n_seq) {
        std::vector<int> tab(p->seq, p->seq + (size_t)a.n_seq * VZ_PROC_SEQ_STRIDE);
        if (!(e->proc.d_seq && tab == e->proc.h_seq)) {
            VZ_CHECK_HIP(hipStreamSynchronize(s));      // steps still in flight read the table of the previous arming
            if (!e->proc.d_seq) VZ_CHECK_HIP(hipMalloc((void**)&e->proc.d_seq, (size_t)VZ_PROC_MAX_SEQ * VZ_PROC_SEQ_STRIDE * sizeof(int)));
            VZ_CHECK_HIP(hipMemcpy(e->proc.d_seq, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
            e->proc.h_seq.swap(tab);
            e->proc.seq_epoch += 1;
        }
        a.seq_epoch = e->proc.seq_epoch;
    }
    e->proc.on = 1; e->proc.a = a;
    return VZ_OK;
}

// Seeds row `row`'s history with n ids that were fed before generation begins (a call that continues on a kept cache: the conversation so
// far): they count for the penalty, the n-grams and the id sequences as a prompt's ids do in HF; min_new_tokens counts the ids behind
// them.  Behind the arming (which empties every history), in front of vz_llm_decode_begin; stream-ordered.
extern "C" int vz_llm_decode_logits_proc_seed(vz_engine* e, int row, const int* h_ids, int n, vz_stream stream) {
    NEED_READY();
    const vz_config& c = e->c;
    VZ_CHECK_ARG(e->proc.on && e->proc.d, "decode_logits_proc_seed: the logits processors are off (vz_llm_decode_logits_proc)");
    VZ_CHECK_ARG(row >= 0 && row < c.max_batch && n >= 0 && n <= c.max_ctx && (h_ids || n == 0), "decode_logits_proc_seed: row %d, %d ids outside max_batch %d / max_ctx %d", row, n, c.max_batch, c.max_ctx);
    hipStream_t s = (hipStream_t)stream;
    if (n) RC(upload_ints(e, h_ids, (size_t)n, proc_hist(e) + (size_t)row * c.max_ctx, s));
    const int two[2] = {n, n};
    RC(upload_ints(e, two, 1, e->proc.d + row, s));
    return upload_ints(e, two + 1, 1, proc_base(e) + row, s);
}

// the same kernel on fp32 logits [rows, cols] in place, over the caller's histories d_hist [rows][hist_stride] of d_hist_len[row] ids
// each; nothing is appended (the first token of a generation: the prefill logits and empty histories; tests).  The id-sequence table goes
// through this (device, stream)'s own scratch
extern "C" int vz_op_logits_process(float* d_logits, int rows, int cols, int* d_hist, int hist_stride, int* d_hist_len,
                                    const vz_logits_proc_params* p, vz_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    VZ_CHECK_ARG(p, "logits_process: null record");
    ProcArgs a;
    RC(proc_args_of(*p, &a));
    void* d_seq = nullptr;
    if (a.n_seq) {
        size_t have = 0;
        const size_t need = (size_t)VZ_PROC_MAX_SEQ * VZ_PROC_SEQ_STRIDE * sizeof(int);
        RC(vz_stream_ws(7, s, need, false, &d_seq, &have));
        VZ_CHECK_ARG(d_seq && have >= need, "logits_process: first use of a stream inside a capture (call it once before capturing)");
        VZ_CHECK_HIP(hipStreamSynchronize(s));          // an earlier call's kernel has read its table
        VZ_CHECK_HIP(hipMemcpy(d_seq, p->seq, (size_t)a.n_seq * VZ_PROC_SEQ_STRIDE * sizeof(int), hipMemcpyHostToDevice));
    }
    return vz_launch_logits_process(d_logits, rows, cols, d_hist, hist_stride, d_hist_len, nullptr, a, (const int*)d_seq, s);
}

// Per-row logits processors (logits_proc.hip: logits_process_rows_kernel).  One record per row of the decode batch in
// device memory, every one inactive after the arming; the histories are the call-level form's buffer (the two forms exclude each other).
static constexpr size_t PROC_REGION_INTS = (size_t)VZ_PROC_MAX_SEQ * VZ_PROC_SEQ_STRIDE;
static int proc_row_of(const vz_proc_row* rec, const int* h_seq, int n_seq, ProcRow* out) {
    memset(out, 0, sizeof(*out));
    if (!rec || !rec->active) return VZ_OK;          // inactive: the other fields are neither read nor kept
    memcpy(out, rec, sizeof(*out));
    out->active = 1; memset(out->pad, 0, sizeof(out->pad));
    RC(vz_proc_row_check(*out));
    VZ_CHECK_ARG(n_seq == out->n_seq, "logits_proc rows: the record names %d id sequences, %d were handed over", out->n_seq, n_seq);
    RC(proc_seq_check(h_seq, n_seq));
    for (int i = 0; i < 4; ++i) if (i >= out->eos.n) out->eos.id[i] = -1;
    for (int i = 0; i < 16; ++i) if (i >= out->n_suppress) out->suppress[i] = -1;
    return VZ_OK;
}

extern "C" int vz_llm_decode_logits_proc_rows(vz_engine* e, int enable, vz_stream stream) {
    NEED_READY();
    if (!enable) { e->proc.rows_on = 0; return VZ_OK; }
    const vz_config& c = e->c;
    if (e->tp > 1) { vz_set_error("decode_logits_proc_rows: logits processors on a tensor-parallel engine are not built"); return VZ_ERR_UNSUPPORTED; }
    VZ_CHECK_ARG(!e->proc.on, "decode_logits_proc_rows: the call-level logits processors are armed (vz_llm_decode_logits_proc): one of the two forms at a time");
    VZ_CHECK_ARG(c.vocab <= 65536, "decode_logits_proc_rows: vocabulary of %d, the kernel's bitmaps hold 65536", c.vocab);
    hipStream_t s = (hipStream_t)stream;
    if (!e->proc.d) VZ_CHECK_HIP(hipMalloc((void**)&e->proc.d, (2 * proc_len_ints(c) + (size_t)c.max_batch * c.max_ctx) * sizeof(int)));
    if (!e->proc.d_rows) VZ_CHECK_HIP(hipMalloc((void**)&e->proc.d_rows, (size_t)c.max_batch * sizeof(ProcRow)));
    if (!e->proc.d_rowseq) {          // (zeroed once: the kernel requests a row's whole region before it knows how much of it counts)
        VZ_CHECK_HIP(hipMalloc((void**)&e->proc.d_rowseq, (size_t)c.max_batch * PROC_REGION_INTS * sizeof(int)));
        VZ_CHECK_HIP(hipMemsetAsync(e->proc.d_rowseq, 0, (size_t)c.max_batch * PROC_REGION_INTS * sizeof(int), s));
    }
    VZ_CHECK_HIP(hipMemsetAsync(e->proc.d, 0, 2 * proc_len_ints(c) * sizeof(int), s));
    VZ_CHECK_HIP(hipMemsetAsync(e->proc.d_rows, 0, (size_t)c.max_batch * sizeof(ProcRow), s));      // every record inactive
    e->proc.rows_on = 1;
    return VZ_OK;
}

extern "C" int vz_llm_decode_set_row_logits_proc(vz_engine* e, int row, const vz_proc_row* rec, const int* h_seq, int n_seq, vz_stream stream) {
    NEED_READY();
    const vz_config& c = e->c;
    VZ_CHECK_ARG(e->proc.rows_on, "decode_set_row_logits_proc: the per-row logits processors are off (vz_llm_decode_logits_proc_rows)");
    VZ_CHECK_ARG(row >= 0 && row < c.max_batch, "decode_set_row_logits_proc: row %d outside max_batch = %d", row, c.max_batch);
    ProcRow pr;
    RC(proc_row_of(rec, h_seq, n_seq, &pr));
    hipStream_t s = (hipStream_t)stream;
    // the sequences first, the record behind them (stream order: a step between the two copies cannot be - they are enqueued back to
    // back), then the row's history restarts: length and seeded-id count 0
    if (pr.active && pr.n_seq) RC(upload_ints(e, h_seq, (size_t)pr.n_seq * VZ_PROC_SEQ_STRIDE, e->proc.d_rowseq + row * PROC_REGION_INTS, s));
    RC(upload_ints(e, (const int*)&pr, sizeof(pr) / sizeof(int), (int*)(e->proc.d_rows + row), s));
    VZ_CHECK_HIP(hipMemsetAsync(e->proc.d + row, 0, sizeof(int), s));
    VZ_CHECK_HIP(hipMemsetAsync(proc_base(e) + row, 0, sizeof(int), s));
    return VZ_OK;
}

// the same kernel on caller-owned logits and histories, row r by h_rows[r]; the records and the rows' sequence regions go through this
// (device, stream)'s own scratch.  Nothing is appended.
extern "C" int vz_op_logits_process_rows(float* d_logits, int rows, int cols, int* d_hist, int hist_stride, int* d_hist_len, const vz_proc_row* h_rows,
                                         const int* h_seq, const int* h_nseq_off, vz_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    VZ_CHECK_ARG(d_logits && d_hist && d_hist_len && h_rows && rows >= 1 && rows <= 64 && cols >= 1 && hist_stride >= 1, "logits_process_rows: bad argument (1..64 rows)");
    const size_t rec_ints = sizeof(ProcRow) / sizeof(int);
    std::vector<int> img((rec_ints + PROC_REGION_INTS) * rows, 0);       // [records | regions]
    for (int r = 0; r < rows; ++r) {
        const int k0 = h_nseq_off ? h_nseq_off[r] : 0, k1 = h_nseq_off ? h_nseq_off[r + 1] : 0;
        VZ_CHECK_ARG(k0 >= 0 && k1 >= k0 && (k1 == k0 || h_seq), "logits_process_rows: row %d takes the id sequences [%d, %d) of a table", r, k0, k1);
        const int* q = k1 > k0 ? h_seq + (size_t)k0 * VZ_PROC_SEQ_STRIDE : nullptr;
        ProcRow* pr = (ProcRow*)(img.data() + rec_ints * r);
        RC(proc_row_of(h_rows + r, q, k1 - k0, pr));
        if (pr->active && pr->n_seq) memcpy(img.data() + rec_ints * rows + PROC_REGION_INTS * r, q, (size_t)pr->n_seq * VZ_PROC_SEQ_STRIDE * sizeof(int));
    }
    void* d = nullptr; size_t have = 0;
    const size_t need = (rec_ints + PROC_REGION_INTS) * 64 * sizeof(int);
    RC(vz_stream_ws(8, s, need, false, &d, &have));
    VZ_CHECK_ARG(d && have >= need, "logits_process_rows: first use of a stream inside a capture (call it once before capturing)");
    VZ_CHECK_HIP(hipStreamSynchronize(s));          // an earlier call's kernel has read its tables
    VZ_CHECK_HIP(hipMemcpy(d, img.data(), img.size() * sizeof(int), hipMemcpyHostToDevice));
    return vz_launch_logits_process_rows(d_logits, rows, cols, d_hist, hist_stride, d_hist_len, nullptr, (const ProcRow*)d, (const int*)d + rec_ints * rows, nullptr, s);
}

// Shared-prefix decode attention (attn_shared.hip; include/viszephyr.h has the contract): the next decode batch is
// `groups` groups of n adjacent rows, and the rows of group g read their first h_shared[g] cache slots from cache row g * n.  n = 0: off.
extern "C" int vz_llm_decode_share(vz_engine* e, int n, const int* h_shared, int groups, vz_stream stream) {
    NEED_READY();
    if (n == 0) { e->share.on = 0; e->share.n = 0; e->share.groups = 0; e->share.shared_max = 0; e->share.h_shared.clear(); return VZ_OK; }
    const vz_config& c = e->c;
    if (e->kv8.on) { vz_set_error("decode_share: not available while the e4m3 KV mirror is on (vz_engine_kv_fp8): its attention reads the bf16 cache and its writes would leave the mirror stale"); return VZ_ERR_UNSUPPORTED; }
    if (e->tp > 1) { vz_set_error("decode_share: the shared-prefix attention on a tensor-parallel engine is not built"); return VZ_ERR_UNSUPPORTED; }
    VZ_CHECK_ARG(n >= 2 && n <= 64 && groups >= 1 && h_shared && (long)groups * n <= std::min(c.max_batch, 64), "decode_share: 2 <= n (%d) <= 64 rows per group and "
                 "groups (%d) x n <= min(max_batch = %d, 64) expected", n, groups, c.max_batch);
    VZ_CHECK_ARG(c.head_dim == 128 && vz_attn_shared_ws_floats(groups * n, n, e->Hq_l, e->Hkv_l, c.max_ctx) > 0, "decode_share: head_dim %d, %d query / %d KV heads unsupported",
                 c.head_dim, e->Hq_l, e->Hkv_l);
    int smax = 0;
    for (int g = 0; g < groups; ++g) {
        VZ_CHECK_ARG(h_shared[g] >= 1 && h_shared[g] <= c.max_ctx, "decode_share: shared[%d] = %d outside [1, max_ctx = %d]", g, h_shared[g], c.max_ctx);
        smax = std::max(smax, h_shared[g]);
    }
    hipStream_t s = (hipStream_t)stream;
    if (!e->share.d_tab) {
        // the largest workspace any arming of this engine can ask for: every (groups, n) with groups x n <= min(max_batch, 64)
        size_t ws = 0;
        const int rows_max = std::min(c.max_batch, 64);
        for (int nn = 2; nn <= rows_max; ++nn)
            for (int gg = 1; gg * nn <= rows_max; ++gg) ws = std::max(ws, vz_attn_shared_ws_floats(gg * nn, nn, e->Hq_l, e->Hkv_l, c.max_ctx));
        VZ_CHECK_HIP(hipMalloc((void**)&e->share.ws, ws * sizeof(float)));
        e->share.ws_floats = ws;
        VZ_CHECK_HIP(hipMalloc((void**)&e->share.q_rot, (size_t)64 * e->Hq_l * c.head_dim * sizeof(bf16_t)));
        VZ_CHECK_HIP(hipMalloc((void**)&e->share.d_tab, 64 * sizeof(int)));
    }
    RC(upload_ints(e, h_shared, groups, e->share.d_tab, s));
    e->share.on = 1; e->share.n = n; e->share.groups = groups; e->share.shared_max = smax;
    e->share.h_shared.assign(h_shared, h_shared + groups);
    return VZ_OK;
}

// Classifier-free guidance in the step (hf:generation/logits_process.py UnbatchedClassifierFreeGuidanceLogitsProcessor; guidance.hip;
// DESIGN.md section 6k): after vz_llm_decode_guidance(enable=1) a decode batch is 2 * pairs rows - row r < pairs a prompt, row pairs + r
// its negative prompt - that share every weight sweep; behind the logits, row r's become scale * (lc - lu) + lu (lc / lu = the
// log-softmax of row r / row pairs + r), then the processors, the tail, the recorder and the matcher run on the first `pairs` rows as
// on a `pairs`-row batch (d_out_ids of vz_llm_decode_steps is [pairs, n]), and row pairs + r follows with the token row r chose.
// The mode is orthogonal to the tail kind; vz_llm_decode_steps refuses it with the beam or the speculative tail.
extern "C" int vz_llm_decode_guidance(vz_engine* e, int enable, float scale, int pairs, vz_stream stream) {
    NEED_READY();
    (void)stream;
    if (!enable) { e->cfg.on = 0; e->cfg.pairs = 0; e->cfg.scale = 1.f; return VZ_OK; }
    if (e->tp > 1) { vz_set_error("decode_guidance: guidance on a tensor-parallel engine is not built"); return VZ_ERR_UNSUPPORTED; }
    VZ_CHECK_ARG(std::isfinite(scale) && pairs >= 1 && decode_shape_ok(e->c, 2 * pairs, false), "decode_guidance: a finite scale (%g) and 1 <= pairs (%d) "
                 "with 2 * pairs <= min(64, max_batch = %d) expected", (double)scale, pairs, e->c.max_batch);
    e->cfg.on = 1; e->cfg.pairs = pairs; e->cfg.scale = scale;
    return VZ_OK;
}

// the same kernel at op level, in place on d_logits_cond [pairs, cols] against d_logits_uncond [pairs, cols] (the first token of a guided
// generation: the two branches' prefill logits; one [2 * pairs, cols] buffer: uncond = cond + pairs * cols)
extern "C" int vz_op_cfg_combine(float* d_logits_cond, const float* d_logits_uncond, int pairs, int cols, float scale, vz_stream stream) {
    VZ_CHECK_ARG(std::isfinite(scale), "cfg_combine: the scale %g is not finite", (double)scale);
    return vz_launch_cfg_combine(d_logits_cond, d_logits_uncond, pairs, cols, scale, (hipStream_t)stream);
}

static int ensure_beam_state(vz_engine* e) {
    if (e->beam.d) return VZ_OK;
    VZ_CHECK_HIP(hipMalloc((void**)&e->beam.d, BEAM_INTS * sizeof(int)));
    VZ_CHECK_HIP(hipMemset(e->beam.d, 0, BEAM_INTS * sizeof(int)));
    return VZ_OK;
}

static int beam_eos_of(const int* h_eos, int n_eos, BeamEos* out) {
    VZ_CHECK_ARG(n_eos >= 0 && n_eos <= 4 && (n_eos == 0 || h_eos), "beam: 0..4 eos ids expected, got %d", n_eos);
    out->n = n_eos;
    for (int i = 0; i < 4; ++i) out->id[i] = i < n_eos ? h_eos[i] : -1;
    return VZ_OK;
}

// Beam search (hf:generation/utils.py `_beam_search`, do_sample=False; beam.hip): after vz_llm_decode_beam(enable=1) the tail of every
// decode step chooses beams instead of argmax.  The running batch (vz_llm_decode_begin) holds `groups` prompts x `nb` beam rows, row
// g * nb + j; `d_scores` [groups * nb] are the running beam scores after the first step, h_base[g] the prompt length of group g (the
// cache positions from there on follow the chosen parents), d_hist the history records [hist_steps][groups][K][3] ({score bits, token,
// parent beam}; K = max(2, 1 + n_eos) * nb), written at a device-side index that restarts at 0 here.  enable = 0: the tail is argmax /
// the sampler again.
extern "C" int vz_llm_decode_beam(vz_engine* e, int enable, int nb, int groups, const int* h_eos, int n_eos, const int* h_base,
                                  const float* d_scores, int* d_hist, int hist_steps, vz_stream stream) {
    NEED_READY();
    if (!enable) { e->beam.on = 0; e->beam.a.hist = nullptr; return VZ_OK; }
    const vz_config& c = e->c;
    if (e->kv8.on) { vz_set_error("decode_beam: not available while the e4m3 KV mirror is on (vz_engine_kv_fp8): its attention reads the bf16 cache and its writes would leave the mirror stale"); return VZ_ERR_UNSUPPORTED; }
    if (e->tp > 1) { vz_set_error("decode_beam: beam search on a tensor-parallel engine is not built"); return VZ_ERR_UNSUPPORTED; }
    VZ_CHECK_ARG(nb >= 2 && nb <= 16 && groups >= 1 && nb * groups <= std::min(c.max_batch, BEAM_ROWS) && h_base && d_scores &&
                 d_hist && hist_steps >= 1, "decode_beam: %d groups x %d beams (2..16) must fit min(max_batch %d, 64) rows; base, scores and "
                 "history needed", groups, nb, c.max_batch);
    BeamEos eos;
    RC(beam_eos_of(h_eos, n_eos, &eos));
    for (int g = 0; g < groups; ++g) VZ_CHECK_ARG(h_base[g] >= 0 && h_base[g] < c.max_ctx, "decode_beam: base[%d] = %d outside [0, %d)", g, h_base[g], c.max_ctx);
    RC(ensure_beam_state(e));
    hipStream_t s = (hipStream_t)stream;
    const int rows = nb * groups;
    const BeamView v = beam_view(e->beam.d);
    std::vector<int> h(v.re_base - v.parent, 0);            // [parent | base | hidx, pad] in one copy
    for (int r = 0; r < rows; ++r) { h[r] = r % nb; h[(v.base - v.parent) + r] = h_base[r / nb]; }
    RC(upload_ints(e, h.data(), h.size(), v.parent, s));
    VZ_CHECK_HIP(hipMemcpyAsync(v.score, d_scores, rows * sizeof(float), hipMemcpyDeviceToDevice, s));
    e->beam.on = 1; e->beam.a = BeamArgs{d_hist, nb, groups, hist_steps, eos};
    return VZ_OK;
}

// The beam tail's selection on given fp32 logits [rows, cols] (rows = groups * nb_in beam rows, running scores d_scores_in [rows] or
// NULL = 0): the group's top K candidates -> d_records [groups][K][3] ({score bits, token, parent beam}), the first nb_out non-eos
// ones -> d_next_tok / d_next_score / d_next_parent [groups * nb_out].  The first step of a beam search: nb_in = 1 on the prefill logits.
static int beam_select_op(const float* d_logits, int rows, int cols, int nb_in, int nb_out, const int* h_eos, int n_eos,
                          const float* d_scores_in, int* d_records, int* d_next_tok, float* d_next_score, int* d_next_parent,
                          bool on_rows, vz_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    VZ_CHECK_ARG(d_logits && d_records && d_next_tok && rows >= 1 && cols >= 1 && nb_in >= 1 && nb_in <= 16 && nb_out >= 1 && nb_out <= 16 &&
                 rows % nb_in == 0, "beam_select: bad argument");
    BeamEos eos;
    RC(beam_eos_of(h_eos, n_eos, &eos));
    const int K = vz_beam_k(nb_out, n_eos);
    void* p = nullptr; size_t have = 0;
    RC(vz_stream_ws(5, s, (size_t)rows * K * 2 * sizeof(int), false, &p, &have));
    VZ_CHECK_ARG(p && have >= (size_t)rows * K * 2 * sizeof(int), "beam_select: first use of a stream inside a capture (call it once before capturing)");
    float* cand_s = (float*)p; int* cand_t = (int*)p + (size_t)rows * K;
    return vz_launch_beam_select(d_logits, rows, cols, nb_in, nb_out, eos, d_scores_in, cand_s, cand_t, d_records, nullptr, 1, d_next_tok,
                                 d_next_score, d_next_parent, {}, on_rows, s);
}
extern "C" int vz_op_beam_select(const float* d_logits, int rows, int cols, int nb_in, int nb_out, const int* h_eos, int n_eos,
                                 const float* d_scores_in, int* d_records, int* d_next_tok, float* d_next_score, int* d_next_parent,
                                 vz_stream stream) {
    return beam_select_op(d_logits, rows, cols, nb_in, nb_out, h_eos, n_eos, d_scores_in, d_records, d_next_tok, d_next_score, d_next_parent, false, stream);
}
// ... on rows that hold scores already (vz_op_beam_logprob_rows, then maybe vz_op_logits_process): s_i = row_i + d_scores_in[row],
// no normalisation.  On log-prob rows as they are it gives the records and next beams of vz_op_beam_select on the logits, bit for bit.
extern "C" int vz_op_beam_select_rows(const float* d_rows, int rows, int cols, int nb_in, int nb_out, const int* h_eos, int n_eos,
                                      const float* d_scores_in, int* d_records, int* d_next_tok, float* d_next_score, int* d_next_parent,
                                      vz_stream stream) {
    return beam_select_op(d_rows, rows, cols, nb_in, nb_out, h_eos, n_eos, d_scores_in, d_records, d_next_tok, d_next_score, d_next_parent, true, stream);
}

// HF's log_softmax rows of fp32 logits [rows, cols] with the beam select's own reductions: d_lp[row][i] = (x_i - max) - log(sum_j
// exp(x_j - max)); d_lp may be d_logits.
extern "C" int vz_op_beam_logprob_rows(const float* d_logits, int rows, int cols, float* d_lp, vz_stream stream) {
    return vz_launch_beam_logprob_rows(d_logits, rows, cols, d_lp, (hipStream_t)stream);
}

// The beam tail's history reorder on its own: d_hist_len [groups * nb] and d_hist [groups * nb][hist_stride] (the processors' id
// histories) - row g * nb + j takes the history and the length of row g * nb + d_parent[g * nb + j], in place.
extern "C" int vz_op_hist_beam_reorder(int* d_hist_len, int* d_hist, int hist_stride, int nb, int groups, const int* d_parent, vz_stream stream) {
    return vz_launch_hist_beam_reorder(d_hist_len, d_hist, hist_stride, nb, groups, d_parent, (hipStream_t)stream);
}

// The beam tail's row recorder: after vz_llm_decode_beam_rows every beam step copies, inside the step, its processed log-prob rows (HF's
// scores[t]) into d_scores and / or its raw logits rows into d_raw, rings [cap_steps][groups * nb][vocab] fp32 written at the history
// index of vz_llm_decode_beam mod cap_steps.  Both NULL: off, and nothing is added to the step.
extern "C" int vz_llm_decode_beam_rows(vz_engine* e, float* d_scores, float* d_raw, int cap_steps) {
    NEED_READY();
    if (!d_scores && !d_raw) { e->beam.rows = BeamRowsArgs{}; return VZ_OK; }
    if (e->tp > 1) { vz_set_error("decode_beam_rows: beam search on a tensor-parallel engine is not built"); return VZ_ERR_UNSUPPORTED; }
    VZ_CHECK_ARG(cap_steps >= 1, "decode_beam_rows: cap_steps = %d, at least one step expected", cap_steps);
    e->beam.rows = BeamRowsArgs{d_scores, d_raw, cap_steps, 0};
    return VZ_OK;
}

// The beam tail's KV reorder on its own: for every group g of `nb` rows (row g * nb + j), cache positions [h_base[g], h_end[g]) of row j
// become those of row d_parent[g * nb + j] of the same group (device ints, local beam indices), every layer, K and V, in place.
extern "C" int vz_llm_kv_beam_reorder(vz_engine* e, int nb, int groups, const int* h_base, const int* h_end, const int* d_parent, vz_stream stream) {
    NEED_READY();
    const vz_config& c = e->c;
    if (e->kv8.on) { vz_set_error("kv_beam_reorder: not available while the e4m3 KV mirror is on (vz_engine_kv_fp8): its attention reads the bf16 cache and its writes would leave the mirror stale"); return VZ_ERR_UNSUPPORTED; }
    VZ_CHECK_ARG(nb >= 1 && nb <= 16 && groups >= 1 && nb * groups <= std::min(c.max_batch, BEAM_ROWS) && h_base && h_end && d_parent,
                 "kv_beam_reorder: %d groups x %d rows must fit min(max_batch %d, 64)", groups, nb, c.max_batch);
    for (int g = 0; g < groups; ++g)
        VZ_CHECK_ARG(h_base[g] >= 0 && h_base[g] <= h_end[g] && h_end[g] <= c.max_ctx, "kv_beam_reorder: group %d range [%d, %d) outside [0, %d]", g, h_base[g], h_end[g], c.max_ctx);
    RC(ensure_beam_state(e));
    hipStream_t s = (hipStream_t)stream;
    const BeamView v = beam_view(e->beam.d);
    std::vector<int> h(2 * BEAM_ROWS, 0);       // [base | end] per group in one copy
    for (int g = 0; g < groups; ++g) { h[g] = h_base[g]; h[(v.re_end - v.re_base) + g] = h_end[g]; }
    RC(upload_ints(e, h.data(), h.size(), v.re_base, s));
    return vz_launch_kv_beam_reorder(e->kv, e->kv_layer_elems, c.n_layers, c.max_batch, e->Hkv_l, c.max_ctx, c.head_dim, nb, groups, d_parent,
                                     v.re_base, 1, v.re_end, 1, s);
}

// Prompt-lookup speculative decoding (spec.hip; include/viszephyr.h has the contract): after vz_llm_decode_begin armed R = D + 1 rows of one
// sequence (positions p + i, context lengths L + i), enable = 1 makes every decode step a verify step with the accept + draft tail and
// writes the first draft into rows 1..D.  enable = 0: the plain tail again.
extern "C" int vz_llm_decode_spec(vz_engine* e, int enable, int D, int max_ngram, int* d_hist, int hist_len, int hist_cap, const int* h_eos, int n_eos,
                                  int* d_out, int budget, int* d_ctl, int* d_stats, int stats_cap, int source, const int* d_stream, int stream_len,
                                  vz_stream stream) {
    NEED_READY();
    if (!enable) { e->spec.on = 0; e->spec.a.samp = ROW_GREEDY; return VZ_OK; }
    const vz_config& c = e->c;
    if (e->kv8.on) { vz_set_error("decode_spec: not available while the e4m3 KV mirror is on (vz_engine_kv_fp8): its attention reads the bf16 cache and its writes would leave the mirror stale"); return VZ_ERR_UNSUPPORTED; }
    if (e->tp > 1) { vz_set_error("decode_spec: speculative decoding on a tensor-parallel engine is not built"); return VZ_ERR_UNSUPPORTED; }
    const int R = D + 1;
    VZ_CHECK_ARG(D >= 1 && D <= 7 && R <= c.max_batch && e->dec_B == R, "decode_spec: D = %d draft slots (1..7) need a running decode batch of D + 1 rows "
                 "(it has %d; max_batch %d)", D, e->dec_B, c.max_batch);
    VZ_CHECK_ARG(max_ngram >= 1 && max_ngram <= 4 && (source == 0 || source == 1) && d_out && d_ctl && budget >= 0 && stats_cap >= 0 && (d_stats || stats_cap == 0),
                 "decode_spec: n-gram size 1..4, source 0 / 1, output and control buffers expected");
    VZ_CHECK_ARG(source == 1 ? (d_stream != nullptr && stream_len >= 0) : (d_hist != nullptr && hist_len >= 1 && hist_len <= hist_cap),
                 "decode_spec: source 0 needs a history of 1..hist_cap ids, source 1 an id stream");
    VZ_CHECK_ARG(!d_hist || hist_len + budget <= hist_cap, "decode_spec: the history (%d ids) + %d new ids exceed its capacity %d", hist_len, budget, hist_cap);
    for (int i = 0; i < R; ++i)
        VZ_CHECK_ARG(e->h_len[i] == e->h_len[0] + i && e->h_pos[i] == e->h_pos[0] + i, "decode_spec: row %d must sit %d positions behind row 0 (vz_llm_decode_begin)", i, i);
    VZ_CHECK_ARG(e->h_len[0] + budget + D <= c.max_ctx, "decode_spec: context %d + %d new ids + %d draft slots exceed max_ctx = %d", e->h_len[0], budget, D, c.max_ctx);
    VZ_CHECK_ARG(e->h_pos[0] + budget + D < e->rope_max, "decode_spec: position %d + %d new ids + %d draft slots exceed the rotary tables (%d)", e->h_pos[0], budget, D, e->rope_max);
    BeamEos eos;
    RC(beam_eos_of(h_eos, n_eos, &eos));
    hipStream_t s = (hipStream_t)stream;
    int h[VZ_SPEC_CTL_WORDS] = {0};
    h[VZ_SPEC_CTL_HIST] = d_hist ? hist_len : 0; h[VZ_SPEC_CTL_DONE] = budget == 0;
    RC(upload_ints(e, h, VZ_SPEC_CTL_WORDS, d_ctl, s));
    e->spec.on = 1; e->spec.R = R; e->spec.base_len = e->h_len[0]; e->spec.base_pos = e->h_pos[0];
    e->spec.a = SpecArgs{d_hist, d_out, d_ctl, d_stats, d_stream, max_ngram, source, budget, d_hist ? hist_cap : 0, stats_cap, stream_len, 0, eos, ROW_GREEDY};
    return launch_spec_tail(e, nullptr, s);      // the first draft into rows 1..D
}

// Sampled verify steps: behind vz_llm_decode_spec(enable = 1), a VZ_ROW_SAMPLE record makes every verify step draw its R rows instead of
// taking their argmax - row i with the record's temperature / top-k / top-p / warpers and seed, stream-row word 0 and draw counter
// ctl[VZ_SPEC_CTL_WRITE] + 1 + i, the index of the token that row would emit (sampling.hip: spec_sample_kernel).  The record's own counter
// field is ignored: the control words carry the counter, nothing else does.  The record is a kernel argument, so it is part of what a
// captured step freezes (SpecArgs).  NULL or a VZ_ROW_GREEDY record: argmax verify again.
extern "C" int vz_llm_decode_spec_sampling(vz_engine* e, const vz_sample_params* p) {
    NEED_READY();
    VZ_CHECK_ARG(e->spec.on, "decode_spec_sampling: arm the speculative tail first (vz_llm_decode_spec with enable = 1)");
    RowSample r = ROW_GREEDY;
    if (p) { vz_sample_params q = *p; q.counter = 0; RC(row_sample_of(q, &r)); }      // (the counter is ignored: zeroed in front of the check)
    e->spec.a.samp = r.mode == VZ_ROW_SAMPLE ? r : ROW_GREEDY;
    return VZ_OK;
}

// the draft rule alone on a device history of hist_len ids: d_draft [D] (padded with 0), the count in d_ctl[VZ_SPEC_CTL_DRAFTED]
extern "C" int vz_op_spec_draft(const int* d_hist, int hist_len, int D, int max_ngram, const int* h_eos, int n_eos, int* d_draft, int* d_ctl,
                                vz_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    VZ_CHECK_ARG(d_hist && d_draft && d_ctl && hist_len >= 0 && D >= 1 && D <= 7, "spec_draft: bad argument");
    BeamEos eos;
    RC(beam_eos_of(h_eos, n_eos, &eos));
    VZ_CHECK_HIP(hipMemsetAsync(d_ctl, 0, VZ_SPEC_CTL_WORDS * sizeof(int), s));
    VZ_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(d_ctl + VZ_SPEC_CTL_HIST), hist_len, 1, s));
    SpecTailArgs t;
    t.g = nullptr; t.cur = nullptr; t.draft = d_draft; t.pos = t.slot = t.len = nullptr; t.ctl = d_ctl; t.out = nullptr; t.budget = 0;
    t.hist = (int*)d_hist; t.hist_cap = hist_len; t.stats = nullptr; t.stats_cap = 0; t.stream = nullptr; t.stream_len = 0; t.eos = eos;
    t.R = D + 1; t.max_ngram = max_ngram; t.source = 0; t.max_ctx = 0; t.rope_max = 0; t.do_accept = 0; t.do_draft = 1;
    return vz_launch_spec_tail(t, s);
}

// argmax of R logit rows + the acceptance step on caller-provided state: d_state = [cur | pos | slot | len] x R, d_ctl the control words
// (the argmax ids land in words 8..), d_stats [3] = this step's record (NULL = none; the record index is the ctl step count)
// (samp = null: the argmax; else the checked VZ_ROW_SAMPLE record the rows are drawn by, counters from d_ctl[VZ_SPEC_CTL_WRITE])
static int op_spec_accept(const float* d_logits, int R, int cols, const RowSample* samp, int* d_state, int* d_ctl, int* d_out, int budget, int* d_hist,
                          int hist_cap, const int* h_eos, int n_eos, int* d_stats, int max_ctx, int rope_max, hipStream_t s) {
    VZ_CHECK_ARG(d_logits && d_state && d_ctl && d_out && R >= 2 && R <= 8 && cols >= 1 && budget >= 0 && max_ctx >= 1 && rope_max >= 1, "spec_accept: bad argument");
    BeamEos eos;
    RC(beam_eos_of(h_eos, n_eos, &eos));
    int* g = d_ctl + VZ_SPEC_CTL_IDS;
    if (samp) RC(vz_launch_spec_sample(d_logits, R, cols, *samp, d_ctl, g, s));
    else RC(vz_launch_argmax(d_logits, R, cols, g, {}, s));
    const DecodeState st = decode_state(d_state, R);
    SpecTailArgs t;
    t.g = g; t.cur = st.cur; t.draft = st.cur + 1; t.pos = st.pos; t.slot = st.slot; t.len = st.len; t.ctl = d_ctl; t.out = d_out; t.budget = budget;
    t.hist = d_hist; t.hist_cap = d_hist ? hist_cap : 0; t.stats = d_stats; t.stats_cap = d_stats ? 0x7fffffff / 4 : 0; t.stream = nullptr; t.stream_len = 0; t.eos = eos;
    t.R = R; t.max_ngram = 1; t.source = 0; t.max_ctx = max_ctx; t.rope_max = rope_max; t.do_accept = 1; t.do_draft = 0;
    return vz_launch_spec_tail(t, s);
}

extern "C" int vz_op_spec_accept(const float* d_logits, int R, int cols, int* d_state, int* d_ctl, int* d_out, int budget, int* d_hist, int hist_cap,
                                 const int* h_eos, int n_eos, int* d_stats, int max_ctx, int rope_max, vz_stream stream) {
    return op_spec_accept(d_logits, R, cols, nullptr, d_state, d_ctl, d_out, budget, d_hist, hist_cap, h_eos, n_eos, d_stats, max_ctx, rope_max, (hipStream_t)stream);
}

// vz_op_spec_accept with the draws of a sampled verify step in front instead of the argmax: row i by the VZ_ROW_SAMPLE record `p` (its
// counter ignored) at draw counter d_ctl[VZ_SPEC_CTL_WRITE] + 1 + i; the draws land in d_ctl[VZ_SPEC_CTL_IDS ..]
extern "C" int vz_op_spec_accept_sampled(const float* d_logits, int R, int cols, const vz_sample_params* p, int* d_state, int* d_ctl, int* d_out, int budget,
                                         int* d_hist, int hist_cap, const int* h_eos, int n_eos, int* d_stats, int max_ctx, int rope_max, vz_stream stream) {
    VZ_CHECK_ARG(p, "spec_accept_sampled: null record");
    RowSample r;
    vz_sample_params q = *p;
    q.counter = 0;          // ignored: zeroed in front of the check
    RC(row_sample_of(q, &r));
    VZ_CHECK_ARG(r.mode == VZ_ROW_SAMPLE, "spec_accept_sampled: a VZ_ROW_SAMPLE record expected (greedy: vz_op_spec_accept)");
    return op_spec_accept(d_logits, R, cols, &r, d_state, d_ctl, d_out, budget, d_hist, hist_cap, h_eos, n_eos, d_stats, max_ctx, rope_max, (hipStream_t)stream);
}

extern "C" long vz_op_spec_part_floats(int R, int Hkv, int nsplit) { return (long)vz_spec_part_floats(R, Hkv, nsplit); }

// RoPE + append of R fresh QKV rows of one sequence (the stand-alone kernel) + the verify attention over its cache row
extern "C" int vz_op_attention_verify(const void* qkv, void* kc, void* vc, void* o, void* q_rot, float* ws, unsigned* ticket, const float* cosT,
                                      const float* sinT, const int* pos, const int* slot, int R, int Hq, int Hkv, int D, int max_ctx, int nsplit,
                                      int key_bound, int window, float scale, vz_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    VZ_CHECK_ARG(qkv && kc && vc && o && q_rot && ws && ticket && cosT && sinT && pos && slot && D == 128, "attention_verify: bad argument (head_dim 128)");
    RC(vz_launch_rope_kv((const bf16_t*)qkv, (Hq + 2 * Hkv) * D, (bf16_t*)q_rot, (bf16_t*)kc, (bf16_t*)vc, cosT, sinT, pos, slot, 1, R, Hq, Hkv, D, max_ctx, s));
    SpecVerifyArgs a;
    a.q = (const bf16_t*)q_rot; a.kc = (const bf16_t*)kc; a.vc = (const bf16_t*)vc; a.o = (bf16_t*)o; a.part = ws; a.ticket = ticket; a.slot = slot;
    a.R = R; a.Hq = Hq; a.Hkv = Hkv; a.max_ctx = max_ctx; a.nsplit = nsplit; a.key_bound = key_bound; a.window = window; a.scale = scale;
    return vz_launch_spec_verify_attn(a, s);
}

// A device-to-device copy of the whole KV cache ([layer][K|V][max_batch][kv head][max_ctx][head_dim] bf16) into d_out (tests):
// *bytes receives its size; d_out = NULL only asks for it.
extern "C" int vz_llm_kv_copy_out(vz_engine* e, void* d_out, size_t max_bytes, size_t* bytes, vz_stream stream) {
    NEED_READY();
    VZ_CHECK_ARG(bytes, "kv_copy_out: null size");
    *bytes = e->kv_layer_elems * e->c.n_layers * sizeof(bf16_t);
    if (!d_out) return VZ_OK;
    VZ_CHECK_ARG(max_bytes >= *bytes, "kv_copy_out: %zu bytes do not hold the %zu-byte cache", max_bytes, *bytes);
    VZ_CHECK_HIP(hipMemcpyAsync(d_out, e->kv, *bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return VZ_OK;
}

// The same for the e4m3 mirror (vz_engine_kv_fp8; tests): the bytes [layer][K|V][max_batch][kv head][max_ctx][head_dim] into d_q and the fp32
// scales [layer][K|V][max_batch][kv head][max_ctx] into d_scales; *q_bytes / *scale_floats receive the sizes; d_q = d_scales = NULL only asks.
extern "C" int vz_llm_kv8_copy_out(vz_engine* e, void* d_q, size_t max_q_bytes, float* d_scales, size_t max_scale_floats, size_t* q_bytes, size_t* scale_floats,
                                   vz_stream stream) {
    NEED_READY();
    VZ_CHECK_ARG(q_bytes && scale_floats, "kv8_copy_out: null size");
    if (!e->kv8.on) { vz_set_error("kv8_copy_out: the e4m3 KV mirror is off (vz_engine_kv_fp8)"); return VZ_ERR_STATE; }
    *q_bytes = e->kv_layer_elems * e->c.n_layers;
    *scale_floats = *q_bytes / e->c.head_dim;
    if (!d_q && !d_scales) return VZ_OK;
    VZ_CHECK_ARG(d_q && d_scales && max_q_bytes >= *q_bytes && max_scale_floats >= *scale_floats, "kv8_copy_out: %zu bytes / %zu floats do not hold the %zu-byte mirror and its "
                 "%zu scales", max_q_bytes, max_scale_floats, *q_bytes, *scale_floats);
    VZ_CHECK_HIP(hipMemcpyAsync(d_q, e->kv8.q, *q_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    VZ_CHECK_HIP(hipMemcpyAsync(d_scales, e->kv8.sc, *scale_floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return VZ_OK;
}

// Does a linear of the B-row step decode_step_launch is about to issue (its four projections, the lm_head) leave the <= 16-row
// weight-stream kernels?  Those routes - the tile GEMMs, gemm_wide.hip and the 17..64-row kernel beside them - are the ones whose launches
// may take per-stream split-K scratch, which cannot be allocated inside a capture.
static bool decode_step_past_16_row_kernels(vz_engine* e, int B) {
    const vz_config& c = e->c;
    const int H = c.hidden, QKV = (e->Hq_l + 2 * e->Hkv_l) * c.head_dim, I = e->I_l, A = e->Hq_l * c.head_dim, V = tp_local(e) ? c.vocab : e->Vp;
    const LlmLayerW& W = e->llm[0];
    const bf16_t* x = e->d_xnorm;          // stands for the activations and outputs: nothing is launched
    const LinearArgs step[] = {
        linear_args(e, x, H, W.qkv, H, (void*)x, QKV, B, QKV, H, nullptr, 0, VZ_ACT_NONE, 0, W.in_norm, c.rms_eps, 0),
        linear_args(e, x, A, W.o, A, (void*)x, H, B, H, A, x, H, VZ_ACT_NONE, 0, nullptr, 0.f, 0),
        linear_args(e, x, H, W.gu, H, (void*)x, I, B, 2 * I, H, nullptr, 0, VZ_ACT_SWIGLU, 0, W.post_norm, c.rms_eps, 0),
        linear_args(e, x, I, W.down, I, (void*)x, H, B, H, I, x, H, VZ_ACT_NONE, 0, nullptr, 0.f, 0),
        linear_args(e, x, H, e->top.lm_head, H, (void*)x, V, B, V, H, nullptr, 0, VZ_ACT_NONE, 1, e->top.norm, c.rms_eps, 0),
    };
    for (const LinearArgs& a : step)
        if (vz_plan_linear(a, linear_caller(e, 1)).route >= LIN_SKINNY_WIDE) return true;
    return false;
}

// what the steps vz_llm_decode_steps(n, d_out_ids) is about to launch would freeze in a capture (e->dec_nsplit, use_tok and the
// speculative key bound are those of this call already)
static DecodeGraphKey decode_graph_key(const vz_engine* e, int n, int* d_out_ids) {
    DecodeGraphKey k;
    memset(&k, 0, sizeof(k));          // padding, and the modes that are off, compare equal
    k.B = e->dec_B; k.n = n; k.nsplit = e->dec_nsplit; k.use_tok = e->use_tok; k.kind = tail_kind(e); k.tune_epoch = vz_tune_epoch();
    k.out = d_out_ids; k.arena = e->arena; k.ring = e->ring.p; k.ring_n = e->ring.n;
    switch (k.kind) {
    case TAIL_SPEC: k.spec = e->spec.a; break;
    case TAIL_BEAM: k.beam = e->beam.a; k.beam_rows = e->beam.rows; break;
    case TAIL_SAMPLE: k.samp = SampleArgs{e->samp.rec.top_k, e->samp.rec.temp, e->samp.rec.top_p, e->samp.rec.warp}; break;
    case TAIL_ROWS: case TAIL_GREEDY: break;
    }
    if (e->proc.on) { k.proc_on = 1; k.proc = e->proc.a; k.proc_hist = e->proc.d; k.proc_seq = e->proc.a.n_seq ? e->proc.d_seq : nullptr; }
    if (stop_armed(e)) { k.stop_state = e->stop.d_state; k.stop = e->stop.a; }
    k.proc_rows_on = e->proc.rows_on; k.stop_rows_on = e->stop.rows_on;
    if (e->cfg.on) { k.cfg_scale = e->cfg.scale; k.cfg_pairs = e->cfg.pairs; }
    if (e->share.on) { k.share_n = e->share.n; k.share_nsplit = vz_attn_shared_nsplit(e->share.groups, e->share.n, e->Hq_l, e->Hkv_l, e->share.shared_max); k.share_tab = e->share.d_tab; }
    if (e->kv8.on) k.kv8 = e->kv8.q;
    if (e->score.what) { k.sc_what = e->score.what; k.sc_cap = e->score.cap; k.sc_rec = e->score.rec; k.sc_warped = e->score.warped; k.sc_raw = e->score.raw; }
    return k;
}

extern "C" int vz_llm_decode_steps(vz_engine* e, int n, int* d_out_ids, float* d_logits_dbg, vz_stream stream) {
    NEED_READY();
    const vz_config& c = e->c;
    hipStream_t s = (hipStream_t)stream;
    VZ_CHECK_ARG(e->dec_B >= 1, "decode_steps: call vz_llm_decode_begin first");
    VZ_CHECK_ARG(n >= 1 && d_out_ids, "decode_steps: bad argument");
    const int B = e->dec_B;
    const TailKind tail = tail_kind(e);
    const bool spec = tail == TAIL_SPEC;
    if (e->share.on) {
        VZ_CHECK_ARG(B == e->share.groups * e->share.n, "decode_steps: the shared-prefix attention (vz_llm_decode_share) is armed for %d x %d rows, the batch has %d",
                     e->share.groups, e->share.n, B);
        if (e->cfg.on || tail == TAIL_SPEC) {
            vz_set_error("decode_steps: the shared-prefix attention (vz_llm_decode_share) does not run with guidance or the speculative tail");
            return VZ_ERR_UNSUPPORTED;
        }
    }
    if (e->kv8.on && (e->share.on || tail == TAIL_BEAM || tail == TAIL_SPEC)) {
        vz_set_error("decode_steps: the e4m3 KV mirror (vz_engine_kv_fp8) runs the plain step only, not the shared-prefix attention, the beam or the speculative tail");
        return VZ_ERR_UNSUPPORTED;
    }
    if (e->cfg.on) {
        if (tail == TAIL_BEAM || tail == TAIL_SPEC) {
            vz_set_error("decode_steps: guidance (vz_llm_decode_guidance) runs in front of the argmax, the sampler or the per-row tail only, not with the "
                         "beam or the speculative tail");
            return VZ_ERR_UNSUPPORTED;
        }
        VZ_CHECK_ARG(B == 2 * e->cfg.pairs, "decode_steps: guidance needs a decode batch of exactly 2 x %d rows (it has %d)", e->cfg.pairs, B);
    }
    const int Bt = e->cfg.on ? e->cfg.pairs : B;      // the rows behind the logits: the tail, the token ring, the recorder, the matcher
    VZ_CHECK_ARG(!e->ring.p || Bt <= e->ring.rows, "decode_steps: the token ring holds %d rows, the decode batch has %d", e->ring.rows, Bt);
    VZ_CHECK_ARG(tail != TAIL_BEAM || (B == e->beam.a.nb * e->beam.a.groups && !e->ring.p), "decode_steps: the beam tail needs a decode batch of exactly "
                 "%d x %d rows (it has %d) and no token ring", e->beam.a.groups, e->beam.a.nb, B);
    VZ_CHECK_ARG(tail != TAIL_SPEC || (B == e->spec.R && !e->ring.p && !e->beam.on && !e->samp.on), "decode_steps: the speculative tail needs a decode batch of "
                 "exactly %d rows (it has %d), without the sampler tail (sampled verify steps: vz_llm_decode_spec_sampling), beams or a token ring", e->spec.R, B);
    VZ_CHECK_ARG(!e->proc.on || tail_takes_proc(tail), "decode_steps: the logits processors (vz_llm_decode_logits_proc) run in "
                 "front of the argmax, the sampler or the beam tail, not with the speculative tail");
    VZ_CHECK_ARG(tail != TAIL_BEAM || !(e->beam.rows.scores || e->beam.rows.raw) || n <= e->beam.rows.cap, "decode_steps: %d steps, the beam row "
                 "recorder's rings hold cap_steps = %d", n, e->beam.rows.cap);
    VZ_CHECK_ARG(!e->rows.on || (!e->beam.on && !e->spec.on && e->tp == 1), "decode_steps: the per-row tail (vz_llm_decode_sampling_rows) does not run "
                 "together with the beam or the speculative tail, nor on a tensor-parallel engine");
    VZ_CHECK_ARG(!e->score.what || (tail != TAIL_BEAM && tail != TAIL_SPEC), "decode_steps: the step recorder (vz_llm_decode_scores) runs behind the "
                 "argmax, the sampler or the per-row tail only, not with the beam or the speculative tail");
    VZ_CHECK_ARG(!stop_armed(e) || (tail != TAIL_BEAM && tail != TAIL_SPEC), "decode_steps: the stop matcher (vz_llm_decode_stop) runs behind the "
                 "argmax, the sampler or the per-row tail only, not with the beam or the speculative tail");
    VZ_CHECK_ARG(!e->proc.rows_on || (tail != TAIL_BEAM && tail != TAIL_SPEC), "decode_steps: the per-row logits processors (vz_llm_decode_logits_proc_rows) run in "
                 "front of the argmax, the sampler or the per-row tail only, not with the beam or the speculative tail");
    VZ_CHECK_ARG(!e->score.what || n <= e->score.cap, "decode_steps: %d steps, the step recorder's rings hold cap_steps = %d", n, e->score.cap);
    DecodeWs w;
    RC(carve_stage(e, "decode", [&](Carver& m) { return carve_decode(m, c, Shard{e->Hq_l, e->Hkv_l, e->I_l}, B, spec); }, &w));
    // tensor-parallel steps: the RCCL all-reduces / all-gather are captured with the kernels (one graph launch per token instead of
    // ~230 host launches); if RCCL refuses the capture the engine falls back to eager steps for good
    bool use_graph = !e->prof_on && !d_logits_dbg && getenv("VZ_NO_GRAPH") == nullptr &&
                     (tp_local(e) || (e->comm_graph_ok && getenv("VZ_TP_NO_GRAPH") == nullptr));
    if (!tp_local(e)) RC(ensure_gather(e, B, s));
    VZ_CHECK_HIP(hipMemsetAsync(decode_state(e->d_state, c.max_batch).step, 0, sizeof(int), s));
    VZ_CHECK_HIP(hipMemsetAsync(e->d_ao_done, 0, sizeof(unsigned), s));      // the attention + O launch's arrival word restarts with the step counter
    // vz_tune_set(28, 1) - batch 1, one GPU, bf16 weights, Zephyr-7B geometry on a 256-CU device: the steps run as ONE resident grid
    // per token (decode_persist.hip) instead of the launch chain.  Its pointer table is (re)built here, never inside a capture.
    e->use_tok = false;
    if (vz_knob(VZ_KNOB_PERSIST_DECODE) && !e->kv8.on && B == 1 && e->tp == 1 && tp_local(e) && !c.weight_fp8 && c.hidden == 4096 && c.inter == 14336 && c.n_heads == 32 &&
        c.n_kv_heads == 8 && c.head_dim == 128 && c.vocab >= 256 && vz_decode_persist_supported()) {
        if (!e->tok) {
            std::vector<VzTokLayerHost> lt(c.n_layers);
            for (int i = 0; i < c.n_layers; ++i) {
                const LlmLayerW& W = e->llm[i];
                lt[i].qkv_w = W.qkv.w; lt[i].o_w = W.o.w; lt[i].gu_w = W.gu.w; lt[i].down_w = W.down.w;
                lt[i].in_norm = W.in_norm; lt[i].post_norm = W.post_norm;
                lt[i].kc = kc_of(e, i); lt[i].vc = vc_of(e, i);
            }
            RC(vz_decode_persist_create(lt.data(), c.n_layers, &e->tok));
        }
        RC(vz_decode_persist_reset(e->tok, s));         // arrival counters restart with the step counter
        if (e->tok_poke_word >= 0) { RC(vz_decode_persist_poke(e->tok, e->tok_poke_word, e->tok_poke_value, s)); e->tok_poke_word = -1; }
        e->use_tok = true;
    }
    if (e->share.on && e->use_tok) {      // (an armed batch has >= 2 rows, the resident grid takes one)
        vz_set_error("decode_steps: the shared-prefix attention (vz_llm_decode_share) on the persistent decode-token kernel is not built");
        return VZ_ERR_UNSUPPORTED;
    }
    if (e->cfg.on && e->use_tok) {      // (a guided batch has >= 2 rows, the resident grid takes one: kept so that widening either shows up here)
        vz_set_error("decode_steps: guidance (vz_llm_decode_guidance) on the persistent decode-token kernel is not built");
        return VZ_ERR_UNSUPPORTED;
    }
    // Capacity (the cache append writes slot = len - 1 of the row, the rotary tables are read at pos): every live row must still fit
    // after n steps.  Parked rows (continuous batching) are not checked: the step tail saturates their slot / position on the device.
    int len_max = 0;
    // Verify steps advance by 1..R positions each, decided on the device: the host bounds by the worst case (n steps = n x R positions),
    // itself bounded by the budget the mode was armed with (vz_llm_decode_spec checked base + budget + R against the cache).
    const int spec_len_cap = spec ? e->spec.base_len + e->spec.a.budget : 0;
    for (int b = 0; b < B; ++b) {
        if (spec) { len_max = std::max(len_max, std::min(e->h_len[b], c.max_ctx)); continue; }
        if (!e->h_parked[b]) {
            VZ_CHECK_ARG(e->h_len[b] + n - 1 <= c.max_ctx, "decode_steps: row %d would reach %d keys, the cache holds max_ctx = %d", b, e->h_len[b] + n - 1, c.max_ctx);
            VZ_CHECK_ARG(e->h_pos[b] + n - 1 < e->rope_max, "decode_steps: row %d would reach position %d, the rotary tables hold %d", b, e->h_pos[b] + n - 1, e->rope_max);
        }
        len_max = std::max(len_max, std::min(e->h_len[b], c.max_ctx));
    }
    e->dec_len_max = len_max;
    // Context splits of the decode attention = grid.x: a split takes >= 128 keys and workgroups that find nothing to do still cost
    // a dispatch slot each (measured: 4096 mostly idle workgroups = 59 us per layer at 16 rows), so the grid follows the longest
    // context these n steps can reach - known on the host - in coarse buckets (a new bucket = one re-capture of the graph).
    {
        int keys = std::min(e->dec_len_max + n, c.max_ctx);
        if (c.sliding_window > 0) keys = std::min(keys, c.sliding_window);
        if (spec) {
            // keys the last of these n steps can see: row 0's worst-case length after n - 1 full steps, + R rows; no window cut - the verify
            // attention's splits sit at absolute key positions
            keys = std::min(std::min(e->h_len[0] + (n - 1) * B, spec_len_cap) + B - 1, c.max_ctx);
        }
        const int need = (keys + 127) / 128;
        static const int buckets[] = {1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 24, 28, 32};
        int ns = e->nsplit;
        for (int bk : buckets) if (bk >= need) { ns = std::min(bk, e->nsplit); break; }
        // many rows fill the chip by themselves: splitting their contexts as well only adds dispatch slots and a merge hop per (row, KV head)
        // (config-5 miniature, e4m3, ctx ~330: 64 rows x 3 splits -> x 1: decode 627 -> 597 ms per batch; 32 rows x 3 -> x 2: 459 -> 448) -
        // rows x KV heads x splits is held to ~512 workgroups; 1..2 rows keep every split (batch-1 numbers unchanged)
        if (!spec) ns = std::min(ns, std::max(1, 512 / std::max(1, B * e->Hkv_l)));      // (a verify step's rows share one cache row and its workgroups)
        e->dec_nsplit = vz_knob(VZ_KNOB_ATTN_NSPLIT) > 0 ? vz_knob(VZ_KNOB_ATTN_NSPLIT) : ns;
        if (spec) {
            // the split positions follow the BUCKET, not the exact bound: one graph per bucket, as for the plain step
            int chunks = need;
            for (int bk : buckets) if (bk >= need) { chunks = bk; break; }
            e->spec.a.key_bound = vz_knob(VZ_KNOB_ATTN_NSPLIT) > 0 ? c.max_ctx : std::min(chunks * 128, c.max_ctx);       // (a pinned split count: splits over the whole cache, one graph)
            // worst case of the device-side state after these n steps (the device keeps the exact one): n x R positions, inside the budget
            const int adv = std::min(e->h_len[0] - e->spec.base_len + n * B, e->spec.a.budget);
            for (int b = 0; b < B; ++b) { e->h_len[b] = e->spec.base_len + adv + b; e->h_pos[b] = e->spec.base_pos + adv + b; }
        }
        for (int b = 0; b < B && !spec; ++b) {       // what the device-side state will be after these n steps (the tail saturates, so do we)
            if (e->h_parked[b]) { e->h_len[b] = std::min(e->h_len[b] + n, c.max_ctx); e->h_pos[b] = std::min(e->h_pos[b] + n, e->rope_max - 1); }
            else { e->h_len[b] += n; e->h_pos[b] += n; }      // a live row that is full is refused by the check above on the next call
        }
    }
    if (!use_graph) {
        for (int i = 0; i < n; ++i)
            RC(decode_step_launch(e, w, d_out_ids, n, d_logits_dbg ? d_logits_dbg + (size_t)i * B * c.vocab : nullptr, s));
        return VZ_OK;
    }
    // the captured step is replayed while everything it froze is unchanged (seed, draw counter and the rows' state live in device memory)
    const DecodeGraphKey key = decode_graph_key(e, n, d_out_ids);
    if (!e->dec_graph || memcmp(&e->dec_graph_key, &key, sizeof(key)) != 0) {
        if (e->dec_graph) { hipGraphExecDestroy(e->dec_graph); e->dec_graph = nullptr; }
        hipGraph_t graph;
        if (!e->cap_stream) VZ_CHECK_HIP(hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking));
        if (decode_step_past_16_row_kernels(e, B)) {     // split-K scratch of the capture stream (128^2 tile route, gemm_wide K splits): never allocated inside a capture
            void* p = nullptr; size_t have = 0;
            RC(vz_stream_ws(0, e->cap_stream, (size_t)96 << 20, false, &p, &have));
            RC(vz_wide_reserve(e->cap_stream));
        }
        VZ_CHECK_HIP(hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeThreadLocal));
        int r = decode_step_launch(e, w, d_out_ids, n, nullptr, e->cap_stream);
        graph = nullptr;
        hipError_t er = hipStreamEndCapture(e->cap_stream, &graph);
        if (r == VZ_OK && er == hipSuccess) er = hipGraphInstantiate(&e->dec_graph, graph, nullptr, nullptr, 0);
        if (graph) hipGraphDestroy(graph);
        if (r != VZ_OK || er != hipSuccess) {
            e->dec_graph = nullptr;
            if (tp_local(e)) { if (r) return r; VZ_CHECK_HIP(er); }
            (void)hipGetLastError();            // collectives would not capture: eager steps from now on
            e->comm_graph_ok = false;
            for (int i = 0; i < n; ++i) RC(decode_step_launch(e, w, d_out_ids, n, nullptr, s));
            return VZ_OK;
        }
        e->dec_captures++;
        memcpy(&e->dec_graph_key, &key, sizeof(key));
    }
    for (int i = 0; i < n; ++i) VZ_CHECK_HIP(hipGraphLaunch(e->dec_graph, s));
    return VZ_OK;
}

// weight_fp8 engines: 1 = the Zephyr prefill linears quantise their input rows to e4m3 and run on the fp8 MFMA against the e4m3 weight
// copies (config 5's "fp8 MFMA weights"; gemm_fp8.hip); 0 (default) = bf16 MFMA on the dequantised bf16 tensors.  Decode is untouched.
extern "C" int vz_engine_prefill_fp8(vz_engine* e, int enable) {
    VZ_CHECK_ARG(e && (!enable || e->c.weight_fp8), "prefill_fp8: needs an engine created with weight_fp8 = 1");
    e->prefill_fp8 = enable ? 1 : 0;
    return VZ_OK;
}

// The opt-in e4m3 mirror of the KV cache for the decode attention.  1: allocates the mirror (1 byte per cache element + one
// fp32 scale per 128: +50 % KV memory next to the bf16 cache, which stays) and marks every row's mirror invalid - a row decodes again once a
// prefill (vz_llm_prefill_rows / vz_llm_prefill_append) or vz_llm_kv_move_rows has rebuilt it.  0 (default): frees it; every call is the
// plain engine's.  Never inside a capture: the captured step is dropped.
extern "C" int vz_engine_kv_fp8(vz_engine* e, int enable) {
    VZ_CHECK_ARG(e, "kv_fp8: null engine");
    if (enable && e->tp > 1) { vz_set_error("kv_fp8: the e4m3 KV mirror on a tensor-parallel engine is not built"); return VZ_ERR_UNSUPPORTED; }
    if (enable && (e->share.on || e->beam.on || e->spec.on)) {
        vz_set_error("kv_fp8: disarm the shared-prefix attention, the beam and the speculative tail first (they read and write the bf16 cache only)");
        return VZ_ERR_STATE;
    }
    VZ_CHECK_HIP(hipDeviceSynchronize());
    RC(drop_decode_graph(e));
    if (!enable) {
        if (e->kv8.q) VZ_CHECK_HIP(hipFree(e->kv8.q));
        if (e->kv8.sc) VZ_CHECK_HIP(hipFree(e->kv8.sc));
        e->kv8.q = nullptr; e->kv8.sc = nullptr; e->kv8.on = 0; e->kv8.valid.clear();
        return VZ_OK;
    }
    const size_t bytes = e->kv_layer_elems * e->c.n_layers;
    if (!e->kv8.q) {
        hipError_t er = hipMalloc((void**)&e->kv8.q, bytes);
        if (er == hipSuccess) er = hipMalloc((void**)&e->kv8.sc, bytes / e->c.head_dim * sizeof(float));
        if (er != hipSuccess) {
            if (e->kv8.q) (void)hipFree(e->kv8.q);
            e->kv8.q = nullptr; e->kv8.sc = nullptr; e->kv8.on = 0;
            vz_set_error("kv_fp8: hipMalloc of the %zu-byte mirror failed: %s", bytes + bytes / e->c.head_dim * sizeof(float), hipGetErrorString(er));
            return VZ_ERR_HIP;
        }
    }
    VZ_CHECK_HIP(hipMemset(e->kv8.q, 0, bytes));
    VZ_CHECK_HIP(hipMemset(e->kv8.sc, 0, bytes / e->c.head_dim * sizeof(float)));
    e->kv8.valid.assign(e->c.max_batch, 0);
    e->kv8.on = 1;
    return VZ_OK;
}

// how the last vz_llm_decode_steps ran: *graph = 1 if a captured graph was replayed, *comm_in_graph = 1 if the engine's RCCL
// collectives are part of it (tensor-parallel engines; 0 after a refused capture = eager steps)
extern "C" int vz_llm_decode_mode(vz_engine* e, int* graph, int* comm_in_graph) {
    VZ_CHECK_ARG(e && graph && comm_in_graph, "decode_mode: null argument");
    *graph = e->dec_graph != nullptr;
    *comm_in_graph = e->dec_graph != nullptr && !tp_local(e) && e->comm_graph_ok;
    return VZ_OK;
}

// the last vz_llm_decode_steps call's context splits (the bucket its steps ran in) and the graphs captured so far (tests: a generation that
// crosses a context bucket captures again)
extern "C" int vz_llm_decode_info(vz_engine* e, int* nsplit, int* captures) {
    VZ_CHECK_ARG(e && nsplit && captures, "decode_info: null argument");
    *nsplit = e->dec_nsplit; *captures = e->dec_captures;
    return VZ_OK;
}

// the arena's size and the mark the last stage call's carving reached in it (equal when that call sized the arena)
extern "C" int vz_engine_ws_info(vz_engine* e, size_t* arena_bytes, size_t* peak_bytes) {
    VZ_CHECK_ARG(e && arena_bytes && peak_bytes, "engine_ws_info: bad argument");
    *arena_bytes = e->arena_bytes; *peak_bytes = e->arena_peak;
    return VZ_OK;
}

// The bytes a stage's carving takes for a call of these dimensions on an engine of this config (this rank's shard sizes): the stage's own
// carve function over a null arena.  -1 = a config or shape the stage would refuse.  Touches no device.
extern "C" long vz_op_stage_ws_bytes(const vz_config* cfg, int stage, int n, int n2, int Lmax, unsigned flags) {
    if (!cfg) return -1;
    const vz_config& c = *cfg;
    const std::string err = g_err;          // a query reports through its result: the checks it shares with vz_engine_create leave no message behind
    const bool bad = check_config(c) != VZ_OK;
    vz_set_error("%s", err.c_str());
    if (bad) return -1;
    const bool spec = (flags & VZ_WS_SPEC_TAIL) != 0;
    Carver m(nullptr, ~(size_t)0);
    switch (stage) {
    case VZ_STAGE_CLIP: if (!clip_shape_ok(c, n)) return -1; carve_clip(m, c, n, !(flags & VZ_WS_CALLER_HIDDEN)); break;
    case VZ_STAGE_QFORMER: if (!qf_shape_ok(c, n, n2, Lmax)) return -1; carve_qformer(m, c, n, n2, Lmax, qf_kv_all(c, n, (flags & VZ_WS_QF_KV_CONTIG) != 0)); break;
    case VZ_STAGE_PREFILL: if (!rows_shape_ok(c, 0, n, n2)) return -1; carve_prefill(m, c, shard_of(c), n, n2); break;
    case VZ_STAGE_DECODE: if (!decode_shape_ok(c, n, spec)) return -1; carve_decode(m, c, shard_of(c), n, spec); break;
    case VZ_STAGE_APPEND: if (!rows_shape_ok(c, 0, n, n2)) return -1; carve_append(m, c, shard_of(c), n, n2); break;
    default: return -1;
    }
    return (long)m.off;
}

// Device-side waits of the one-launch attention half are bounded; one that expires raises a word the host reads here (blocking
// 4-byte copy after a stream sync; the word is cleared).  *err != 0 means the ids / logits of the steps since the last call are garbage.
extern "C" int vz_engine_async_error(vz_engine* e, int* err) {
    VZ_CHECK_ARG(e && err, "async_error: null argument");
    *err = 0;
    if (!e->d_ferr) return VZ_OK;
    VZ_CHECK_HIP(hipMemcpy(err, e->d_ferr, sizeof(int), hipMemcpyDeviceToHost));
    if (*err) {
        VZ_CHECK_HIP(hipMemset(e->d_ferr, 0, sizeof(int)));
        // the stream-K tickets that made a wait expire are in an unknown state: start the next launch from zero
        int dummy = 0;
        RC(vz_gemm256_async_error(e->last_stream, &dummy, true));
    }
    return VZ_OK;
}

// the same word for op-level launches on `stream` (vz_op_linear* taking the stream-K path): blocking read + clear
extern "C" int vz_op_async_error(vz_stream stream, int* err) {
    VZ_CHECK_ARG(err, "op_async_error: null argument");
    return vz_gemm256_async_error((hipStream_t)stream, err, false);
}

// TEST HOOK: overwrite the {arrive, ready} pair of stream-K remainder tile `tile` on `stream` (tests/test_ops_gpu.py drives an
// expired fix-up wait with it: the launch must end, raise VZ_ASYNC_STREAMK and write NaN, never a sum of stale slots)
// TEST HOOK: preset arrival-counter shard `word` (0..7; 8 = the abort word) of the persistent decode-token kernel's hand-off state for
// the NEXT vz_llm_decode_steps call - tests/test_persist_gpu.py makes a shard lag so that a wait can never be met: the launch must END,
// raise VZ_ASYNC_PERSIST, and the call after it (which zeroes the counters again) must be clean.  *mode (may be null) receives 1 if the last steps ran on the
// persistent kernel.
extern "C" int vz_test_persist_poke(vz_engine* e, int word, unsigned value, int* mode, vz_stream stream) {
    VZ_CHECK_ARG(e && word <= 8, "persist_poke: bad argument");
    (void)stream;
    if (mode) *mode = e->use_tok && e->tok ? 1 : 0;
    if (word >= 0) { e->tok_poke_word = word; e->tok_poke_value = value; }      // applied by the next vz_llm_decode_steps, behind its counter reset
    return VZ_OK;
}
extern "C" int vz_test_corrupt_streamk(vz_stream stream, int tile, int arrive, int ready) {
    return vz_gemm256_corrupt_tickets((hipStream_t)stream, tile, arrive, ready);
}

int vz_gemm256_read_stamps(long long* host, int max_wgs, int* n_wgs);
int vz_attn_read_stamps(long long* host16);
extern "C" int vz_prof_attn_stamps(long long* host16) { return vz_attn_read_stamps(host16); }
extern "C" int vz_prof_gemm_stamps(long long* host_out, int max_wgs, int* n_wgs) {
    return vz_gemm256_read_stamps(host_out, max_wgs, n_wgs);
}

// phase stamps of the last token the persistent decode-token kernel ran (tools/persist_stamps.py): [n_layers][12] 100 MHz ticks
extern "C" int vz_prof_persist_stamps(vz_engine* e, unsigned long long* host, int n_layers) {
    VZ_CHECK_ARG(e && e->tok, "prof_persist_stamps: the engine has not run a step on the persistent kernel");
    return vz_decode_persist_stamps(e->tok, host, n_layers);
}

extern "C" int vz_prof_enable(vz_engine* e, int enable, int klass) {
    VZ_CHECK_ARG(e, "prof: null engine");
    e->prof_on = enable; e->prof_class = klass; e->prof_used = 0;
    return VZ_OK;
}
extern "C" int vz_prof_read(vz_engine* e, long* n_launches, double* total_ms) {
    VZ_CHECK_ARG(e && n_launches && total_ms, "prof: null argument");
    double tot = 0;
    for (size_t i = 0; i < e->prof_used; ++i) {
        VZ_CHECK_HIP(hipEventSynchronize(e->prof_ev[i].second));
        float ms = 0;
        VZ_CHECK_HIP(hipEventElapsedTime(&ms, e->prof_ev[i].first, e->prof_ev[i].second));
        tot += ms;
    }
    *n_launches = (long)e->prof_used; *total_ms = tot;
    e->prof_used = 0;
    return VZ_OK;
}

