// Weight-streaming GEMV for the decode step (gfx950): C[M<=8, N'] = epi(x[M,K] . W[N,K]^T).
//
// Batch-1 decode reads every one of the 7.2 B bf16 weights once per token (14.2 GB): the kernel is a
// pure HBM stream.  Each wave owns R weight rows at a time and pulls them with 16-byte loads
// straight into VGPRs (64 lanes x 16 B = 1 KiB contiguous per instruction, U x R instructions in
// flight per wave) - no LDS round trip for data that is read exactly once (cdna guide section 5,
// "GEMV / M <= 16" row); optional non-temporal policy so the stream does not evict what IS reused.
// The activation vector(s) are staged once per workgroup in LDS as bf16; with `norm_w` the
// RMSNorm of the residual stream (hf:models/mistral/modeling_mistral.py:182-199) is fused into
// that staging.  Loads, stores and atomics of a wave retire through ONE counter in issue order
// (s_waitcnt vmcnt), so whatever the staging waits for must be requested before the weights:
// for one or two rows the loads of x and norm_w go out first, then half of the wave's first
// batch of weights, and the staging's waits leave those weights in flight (the second norm
// pass reads x from registers).  The wider forms request the first batch first and drain it in
// their staging loops.  The stream itself is a ring of U slots per row: a slot is consumed under
// a counted wait and at once requested again U chunks further on (gemv_step), also across the
// boundary to the wave's next unit (limits: DESIGN.md 6b item 4); residual / bias / scale are
// requested at the start of a unit, not after its reduction.  A launch that has neither bias
// nor residual (bf16 weights, one or two rows: QKV, gate|up, lm_head of the decode step) runs
// gemv_bf16_noepi_kernel, the same stream without that code: nothing is waited for between a
// unit's reduction and its stores, so a looping wave's next unit stays in flight under them, and
// it asks for that unit half a batch at a time (launch_noepi).  Accumulation: v_dot2c_f32_bf16 into fp32, wave
// reduction, then the same epilogues as the tile GEMM (bias / act / SwiGLU pair / residual /
// bf16|fp32 out).  The per-lane order of the sums is the one attn_o_fused.hip and
// decode_persist.hip repeat: chunks ascending, the four fdot2 of dot8 in order.
//
// FP8 weights (W8A16, SURVEY config 5 "fp8 weights"): the same stream at 1 byte per weight.  Rows are OCP e4m3 with one
// power-of-two scale per output row (vz_hip/quant.py), so the dequantised weight 2^e * fp8 is EXACTLY a bf16 number: a
// lane's 16 weights per load are widened to packed bf16 pairs (v_cvt_scalef32_pk_bf16_fp8, exact) and go
// through the same v_dot2c_f32_bf16 as the bf16 stream; the row's 2^e multiplies the fp32 sum once.  The prefill GEMMs
// run on the bf16 copy of the same dequantised weights, so prefill and decode see one and the same model.
#include "vz_common.h"

#include "gemv_kernel.h"

namespace {

// The operand-free form of the stream (gemv_bf16_noepi_kernel): one kernel per K shape, chosen here as gemv_bf16_kernel chooses its body.
template <int MB, int R, int U, bool NT, int NW, int MODE, int G>
int launch_noepi_form(const GemvParams& p, int blocks, hipStream_t s, size_t lds) {
    static VzDeviceOnce attr;
    if (vz_device_first(attr)) {
        VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_noepi_kernel<MB, R, U, NT, NW, MODE, G>, hipFuncAttributeMaxDynamicSharedMemorySize, NW == 4 ? 64 * 1024 : 160 * 1024));
    }
    vz_launch_timed(gemv_bf16_noepi_kernel<MB, R, U, NT, NW, MODE, G>, dim3(blocks), dim3(NW * 64), lds, s, p);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}

template <int MB, int R, int U, bool NT, int NW>
int launch_noepi(const GemvParams& p, int blocks, hipStream_t s, size_t lds) {
    const int nchunk = p.K / 512;
    if (nchunk == U) {
        // looping (some wave walks more than one unit: gate|up, lm_head): the next unit is requested half a batch at a time, 8 loads behind
        // every fourth slot (us per launch, best .. worst of 4 rounds: slot by slot 37.07 .. 37.18 / 39.58 .. 39.81, half batches
        // 36.64 .. 36.72 / 39.64 .. 39.82, one burst of 16 behind the last slot 36.48 .. 36.81 / 39.88 .. 40.06)
        if (p.units > blocks * NW) return launch_noepi_form<MB, R, U, NT, NW, GEMV_K_ONE, 4>(p, blocks, s, lds);
        return launch_noepi_form<MB, R, U, NT, NW, GEMV_K_ONE, 1>(p, blocks, s, lds);
    }
    if (nchunk > U) return launch_noepi_form<MB, R, U, NT, NW, GEMV_K_MANY, 1>(p, blocks, s, lds);
    return launch_noepi_form<MB, R, U, NT, NW, GEMV_K_SHORT, 1>(p, blocks, s, lds);
}

template <int MB, int R, int U, bool NT, bool FP8 = false, int NW = 4>
int launch_variant(const GemvParams& p0, hipStream_t s, size_t lds) {
    GemvParams p = p0;
    p.units = p.act == VZ_ACT_SWIGLU ? p.N / R : (p.N + R - 1) / R;     // SwiGLU: R/2 outputs of N/2 per unit
    int blocks = (p.units + NW - 1) / NW;
    int cap = NW == 4 ? 2048 : 512;
    const int variant = vz_knob(VZ_KNOB_GEMV_VARIANT);
    if (variant >= 7 && variant <= 10) cap = (variant & 1) ? 256 : 512;      // experiments: one / two workgroups per CU
    if (blocks > cap) blocks = cap;
    // neither bias nor residual (QKV, gate|up, lm_head of the decode step): the form without the epilogue's operands; routed forms only
    if constexpr (MB <= 2 && !FP8 && R == 2 && U == 8 && NT) {
        if (!p.bias && !p.residual) return launch_noepi<MB, R, U, NT, NW>(p, blocks, s, lds);
    }
    static VzDeviceOnce attr;
    if (vz_device_first(attr)) {
        VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_kernel<MB, R, U, NT, FP8, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, NW == 4 ? 64 * 1024 : 160 * 1024));
    }
    vz_launch_timed(gemv_bf16_kernel<MB, R, U, NT, FP8, NW>, dim3(blocks), dim3(NW * 64), lds, s, p);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}

template <int MB>
int launch_mb(const GemvParams& p, hipStream_t s, size_t lds) {
    if (lds > 64 * 1024) {        // x does not fit 64 KiB: one 1024-thread workgroup per CU shares one copy (up to 160 KiB)
        if constexpr (MB >= 2) {
            if (p.W8) return launch_variant<MB, 2, 8, true, true, 16>(p, s, lds);
            return launch_variant<MB, 2, 8, true, false, 16>(p, s, lds);
        } else {
            return VZ_ERR_ARG;
        }
    }
    // Batch 1: 8-wave workgroups, at most two per CU (512), where that deals the units evenly over the CUs (O / down: 256 workgroups,
    // gate-up / lm_head: 512 looping); QKV (3072 units = 384 such workgroups = 1.5 per CU) keeps 768 one-unit 4-wave workgroups.
    // Re-measured with the rolling refill, per launch, weights from HBM (profiles/gemv_stream_kernel_stats.txt; us, this rule first):
    //   QKV      768 x 4 waves  9.7 | 384 x 8 waves 10.0 | 256 x 8 looping 10.5
    //   O        256 x 8        7.3 | 512 x 4        7.5
    //   down     256 x 8       19.1 | 512 x 4       19.9
    //   gate|up  512 x 8 loop. 36.9 | 256 x 8 looping 37.2 | 2048 x 4 looping 36.8
    //   lm_head  512 x 8 loop. 40.2 | 256 x 8 looping 40.9 | 2048 x 4 looping 40.8
    // One looping workgroup per CU loses everywhere; the rule stays (gate|up's 0.1 us for 2048 x 4 is inside the spread of 0.4).
    // This rule with the operand-free form where it applies, as the decode step launches them (fused norm; O and down with their residual;
    // profiles/gemv_noepi_ab.txt; best .. worst of 4 rounds, the parent commit's library in the same session behind the bar):
    //   QKV      768 x 4         9.61 ..  9.71 |  9.79 ..  9.98
    //   O        256 x 8         7.29 ..  7.34 |  7.27 ..  7.51      (gemv_bf16_kernel in both)
    //   down     256 x 8        19.19 .. 19.27 | 19.20 .. 19.31      (gemv_bf16_kernel in both)
    //   gate|up  512 x 8 loop.  36.64 .. 36.72 | 37.23 .. 37.63
    //   lm_head  512 x 8 loop.  39.64 .. 39.82 | 40.31 .. 40.53
    bool fat = false;
    if constexpr (MB <= 4) {
        const int units = p.act == VZ_ACT_SWIGLU ? p.N / 2 : (p.N + 1) / 2;
        const int b8 = (units + 7) / 8;
        fat = vz_knob(VZ_KNOB_GEMV_VARIANT) == 0 && (b8 >= 512 || b8 % 256 == 0);
    }
    if (p.W8) {       // 2 rows x up to 8 chunks of 1024 k per wave (measured faster than 4 rows x 4: 13.5 vs 15.3 us on down-proj)
        if (vz_knob(VZ_KNOB_GEMV_VARIANT) == 1) return launch_variant<MB, 4, 4, true, true>(p, s, lds);
        if constexpr (MB <= 4) { if (fat) return launch_variant<MB, 2, 8, true, true, 8>(p, s, lds); }
        return launch_variant<MB, 2, 8, true, true>(p, s, lds);
    }
    if constexpr (MB <= 4) { if (fat) return launch_variant<MB, 2, 8, true, false, 8>(p, s, lds); }
    switch (vz_knob(VZ_KNOB_GEMV_VARIANT)) {
        case 1: return launch_variant<MB, 2, 4, false>(p, s, lds);
        case 2: return launch_variant<MB, 2, 8, false>(p, s, lds);
        case 3: return launch_variant<MB, 2, 8, true>(p, s, lds);
        case 4: return launch_variant<MB, 4, 4, true>(p, s, lds);
        case 5: return launch_variant<MB, 4, 4, false>(p, s, lds);
        case 6: return launch_variant<MB, 2, 4, true>(p, s, lds);
        case 7: case 8: return launch_variant<MB, 2, 8, true, false, 16>(p, s, lds);     // 16 waves, 256 / 512 workgroups
        case 9: case 10: return launch_variant<MB, 2, 8, true, false, 8>(p, s, lds);    // 8 waves, 256 / 512 workgroups
        default: return launch_variant<MB, 2, 8, true>(p, s, lds);
    }
}

}  // namespace

bool vz_gemv_ok(const LinearArgs& a) {
    if (a.M > 8 || (a.K % (a.W8 ? 1024 : 512)) != 0) return false;
    if (a.W8 && (!a.wscale || (a.ldw & 15) != 0 || ((uintptr_t)a.W8 & 15) != 0)) return false;
    if (a.act == VZ_ACT_SWIGLU && (a.N % 64) != 0) return false;
    const int mb = a.M <= 1 ? 1 : a.M <= 2 ? 2 : a.M <= 4 ? 4 : 8;
    return (size_t)mb * a.K * 2 + 256 <= 160 * 1024;
}

int vz_init_gemv_kernels() {
    // every variant sets its own dynamic-LDS limit on first use; make the production ones resident now so the
    // first use never happens inside a stream capture
    static VzDeviceOnce once;
    if (!vz_device_first(once)) return VZ_OK;
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_kernel<1, 2, 8, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_kernel<1, 2, 8, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_kernel<1, 2, 8, true, false, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_kernel<1, 2, 8, true, true, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_kernel<2, 2, 8, true, false, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_kernel<2, 2, 8, true, true, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_kernel<4, 2, 8, true, false, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_kernel<4, 2, 8, true, true, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_kernel<2, 2, 8, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_kernel<2, 2, 8, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_kernel<4, 2, 8, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_kernel<4, 2, 8, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_kernel<8, 2, 8, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_kernel<8, 2, 8, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
#define VZ_NOEPI_ATTR(MB, NW, MODE, G) \
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)gemv_bf16_noepi_kernel<MB, 2, 8, true, NW, MODE, G>, hipFuncAttributeMaxDynamicSharedMemorySize, NW == 4 ? 64 * 1024 : 160 * 1024))
#define VZ_NOEPI_ATTRS(MB, NW) \
    VZ_NOEPI_ATTR(MB, NW, GEMV_K_SHORT, 1); VZ_NOEPI_ATTR(MB, NW, GEMV_K_ONE, 1); VZ_NOEPI_ATTR(MB, NW, GEMV_K_ONE, 4); VZ_NOEPI_ATTR(MB, NW, GEMV_K_MANY, 1)
    VZ_NOEPI_ATTRS(1, 4); VZ_NOEPI_ATTRS(1, 8); VZ_NOEPI_ATTRS(2, 4); VZ_NOEPI_ATTRS(2, 8);
#undef VZ_NOEPI_ATTRS
#undef VZ_NOEPI_ATTR
    return VZ_OK;
}

int vz_launch_gemv(const LinearArgs& a, hipStream_t s) {
    int rc = vz_linear_check_common(a);
    if (rc) return rc;
    VZ_CHECK_ARG(vz_gemv_ok(a), "gemv: needs M <= 8, K %% 512 == 0 (fp8 weights: K %% 1024 == 0, 16-byte-aligned rows, scales) and "
                                "M*K*2 <= 64 KiB (M=%d K=%d)", a.M, a.K);
    GemvParams p;
    p.A = a.A; p.W = a.W; p.C = a.C; p.bias = a.bias; p.residual = a.residual; p.norm_w = a.norm_w;
    p.W8 = a.W8; p.wscale = a.wscale;
    p.M = a.M; p.N = a.N; p.K = a.K; p.lda = a.lda; p.ldw = a.ldw; p.ldc = a.ldc; p.ldr = a.ldr;
    p.act = a.act; p.out_fp32 = a.out_fp32; p.norm_eps = a.norm_eps; p.units = 0;
    const int mb = a.M <= 1 ? 1 : a.M <= 2 ? 2 : a.M <= 4 ? 4 : 8;
    const size_t lds = (size_t)mb * a.K * 2 + 256;
    { int r = vz_init_gemv_kernels(); if (r) return r; }
    switch (mb) {
        case 1: return launch_mb<1>(p, s, lds);
        case 2: return launch_mb<2>(p, s, lds);
        case 4: return launch_mb<4>(p, s, lds);
        default: return launch_mb<8>(p, s, lds);
    }
}
