// gemv_bf16_kernel, gemv_bf16_noepi_kernel and what they are made of: included by gemv.hip (the launchers) and by gemv_audit.hip (the
// batch-1 production instantiations alone, for tests/test_gemv_isa_cpu.py and tests/test_gemv_noepi_isa_cpu.py).  The header of gemv.hip
// describes the kernels.
#pragma once
#include "vz_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

struct GemvParams {
    const bf16_t* A; const bf16_t* W; void* C;
    const unsigned char* W8; const float* wscale;     // FP8 instantiation: e4m3 rows [N][ldw] + fp32 2^e per row
    const float* bias; const bf16_t* residual; const float* norm_w;
    int M, N, K, lda, ldw, ldc, ldr;
    int act, out_fp32, units;
    float norm_eps;
};

// NOTE (hipcc / ROCm 7.2): __builtin_bit_cast applied directly to a vector ELEMENT expression (w[i]) folds every
// use to element 0; the elements are copied to scalars first.
__device__ __forceinline__ float dot8(const u32x4 w, const u32x4 x, float acc) {
    const unsigned w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, w0), __builtin_bit_cast(bf16x2, x0), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, w1), __builtin_bit_cast(bf16x2, x1), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, w2), __builtin_bit_cast(bf16x2, x2), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, w3), __builtin_bit_cast(bf16x2, x3), acc, false);
    return acc;
}

// 16 e4m3 weights of one lane -> 16 bf16 (two u32x4 of packed pairs, k order preserved); exact.
// v_cvt_scalef32_pk_bf16_fp8 widens two fp8 of a dword half to a packed bf16 pair in one instruction (scale 1.0).
__device__ __forceinline__ unsigned fp8x2_to_bf16x2(unsigned w, bool hi_half) {
    return hi_half ? __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true))
                   : __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false));
}
__device__ __forceinline__ void fp8x16_to_bf16(const u32x4 w, u32x4& lo, u32x4& hi) {
    const unsigned w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
    lo = (u32x4){fp8x2_to_bf16x2(w0, false), fp8x2_to_bf16x2(w0, true), fp8x2_to_bf16x2(w1, false), fp8x2_to_bf16x2(w1, true)};
    hi = (u32x4){fp8x2_to_bf16x2(w2, false), fp8x2_to_bf16x2(w2, true), fp8x2_to_bf16x2(w3, false), fp8x2_to_bf16x2(w3, true)};
}

template <bool NT>
__device__ __forceinline__ u32x4 ldw(const void* p) {
    if (NT) return __builtin_nontemporal_load((const u32x4*)p);
    return *(const u32x4*)p;
}

__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == VZ_ACT_QUICK_GELU) return act_quick_gelu(v);
    if (act == VZ_ACT_GELU_ERF) return act_gelu_erf(v);
    return v;
}

// One batch of a wave's stream.  Slot c of the register ring wreg[.][c] holds chunk xc0 + c of the current unit.  The step consumes slots
// 0..nc-1 in ascending chunk order and, as soon as slot c has been consumed, re-issues it (c < nr) from rp[r] + c chunks - the chunk U
// further on in the same unit, or the same slot of the wave's next unit.  NC / NR >= 0 fix the two counts at compile time: the body is then
// straight-line code and the compiler waits vmcnt(in flight behind slot c) per chunk, so the wave keeps its loads in flight from the first
// to the last.  NC = NR = -1 takes them at run time: every load then sits behind a branch of its own and the waits fall back to draining
// (a conditional load may not have been issued, so nothing can be counted behind it) - used for the shapes without a compiled form.
// G: refill granularity.  Slots are requested again G at a time, behind the consumption of the last of the G (1: slot by slot).
template <int MB, int R, int U, bool NT, bool FP8, int NC, int NR, int G = 1>
__device__ __forceinline__ void gemv_step(u32x4 (&wreg)[R][U], float (&acc)[R][MB], const char* smem, int K, int lane, int xc0, int nc, int nr,
                                          const char* const (&rp)[R]) {
    constexpr int EPL = FP8 ? 16 : 8, CH = 64 * EPL, WBYTES = FP8 ? 1 : 2;
#pragma unroll
    for (int c = 0; c < U; ++c) {
        if (NC >= 0 ? c < NC : c < nc) {
            if constexpr (FP8) {
                u32x4 wl[R], wh[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    // The widening is pure, and two forms of the step on the two sides of a branch share it: the optimiser lifts the
                    // whole batch's above the branch, where it waits for every load and takes 128 registers.  Opaque, it stays here.
                    u32x4 w = wreg[r][c];
                    asm volatile("" : "+v"(w));
                    fp8x16_to_bf16(w, wl[r], wh[r]);
                }
#pragma unroll
                for (int m = 0; m < MB; ++m) {
                    const bf16_t* xp = (const bf16_t*)smem + (size_t)m * K + (xc0 + c) * CH + lane * 16;
                    const u32x4 x0 = *(const u32x4*)xp, x1 = *(const u32x4*)(xp + 8);
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[r][m] = dot8(wh[r], x1, dot8(wl[r], x0, acc[r][m]));
                }
            } else {
#pragma unroll
                for (int m = 0; m < MB; ++m) {
                    const u32x4 xv = *(const u32x4*)((const bf16_t*)smem + (size_t)m * K + (xc0 + c) * 512 + lane * 8);
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[r][m] = dot8(wreg[r][c], xv, acc[r][m]);
                }
            }
        }
        // the refill of slot c stays behind its consumption and ahead of the next chunk's: hoisted, it would need a second set of registers
        __builtin_amdgcn_sched_barrier(0);
        if ((c + 1) % G == 0) {
#pragma unroll
            for (int g = c + 1 - G; g <= c; ++g)
                if (NR >= 0 ? g < NR : g < nr) {
#pragma unroll
                    for (int r = 0; r < R; ++r) wreg[r][g] = ldw<NT>(rp[r] + (size_t)g * CH * WBYTES);
                }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The three shapes of a unit's stream, one body each (the branch is taken by the whole grid; each side is a stream whose load counts the
// compiler can follow, with few enough forms of the step for the register ring to stay in one set of registers):
//   K_SHORT  K below one batch of U chunks: every load guarded, the run-time step.
//   K_ONE    K of exactly one batch (4096 in bf16): no loop over batches.  Before a loop that consumes registers loaded ahead of it
//            and loads itself, the compiler drains the counter; here that happens once per wave, before the loop over units.
//   K_MANY   more: a loop of compiled steps <U,U> (refill everything) and <U,0>, then a short last batch on the run-time step (K = 14336
//            is 3.5 batches).  The drain ahead of the batch loop comes once per unit.
// NOEPI: the launch has neither bias nor residual (bf16 weights, one or two rows): the early-operand code does not exist.
// G: refill granularity of the K_ONE stream (gemv_step).
enum { GEMV_K_SHORT = 0, GEMV_K_ONE = 1, GEMV_K_MANY = 2 };
template <int MB, int R, int U, bool NT, bool FP8, int NW, int MODE, bool NOEPI = false, int G = 1>
__device__ __forceinline__ void gemv_body(const GemvParams& p, char* smem) {
    constexpr bool WHOLE = MODE != GEMV_K_SHORT;      // K holds at least one whole batch: the first batch is U x R unconditional loads
    constexpr int NTHR = NW * 64;
    constexpr int EPL = FP8 ? 16 : 8;            // weights per lane per load
    constexpr int CH = 64 * EPL;                 // k per chunk
    constexpr int WBYTES = FP8 ? 1 : 2;
    constexpr size_t CHB = (size_t)CH * WBYTES;  // bytes per chunk of one row
    constexpr int XN = 2, XC = 4;                // 16-byte pieces of x per thread and row the prologue keeps in registers: with / without the norm
    // the wave index through readfirstlane: the compiler then knows that units, their row pointers and every branch on them are wave-uniform
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = p.K;
    float* red = (float*)(smem + (size_t)MB * K * 2);     // NW floats
    const bool swiglu = p.act == VZ_ACT_SWIGLU;
    const int nchunk = K / CH;
    const char* wbase = FP8 ? (const char*)p.W8 : (const char*)p.W;

    auto row_of = [&](int u, int r) -> int {
        if (swiglu) {                                  // outputs j = u*(R/2) + r/2 ; r even = gate, odd = up
            const int j = u * (R / 2) + (r >> 1);
            return (j >> 4) * 32 + (j & 15) + ((r & 1) ? 16 : 0);
        }
        const int n = u * R + r;
        return n < p.N ? n : p.N - 1;
    };
    auto unit_ptr = [&](int u, const char* (&wp)[R]) {
#pragma unroll
        for (int r = 0; r < R; ++r) wp[r] = wbase + ((size_t)row_of(u, r) * p.ldw + lane * EPL) * WBYTES;
    };
    u32x4 wreg[R][U];
    // slots C0 .. C1-1 <- chunks c0 + C0 .. of the unit at wp, slot by slot; `lim` < U guards each chunk (c0 + c < lim)
    auto issue = [&](auto C0, auto C1, const char* const (&wp)[R], int c0, int lim) {
#pragma unroll
        for (int c = decltype(C0)::value; c < decltype(C1)::value; ++c)
            if (lim < 0 || c0 + c < lim) {
#pragma unroll
                for (int r = 0; r < R; ++r) wreg[r][c] = ldw<NT>(wp[r] + (size_t)(c0 + c) * CHB);
                __builtin_amdgcn_sched_barrier(0);      // in this order: slot c is whole once 2 (c + 1) loads have landed
            }
    };
    using I0 = std::integral_constant<int, 0>;
    // 4 and 8 rows keep whole bursts: the first batch goes out whole ahead of the staging and every later one behind the one before it (their
    // register-heavy forms measured 12-21 % slower with the slot-by-slot refill: 8 rows of e4m3 at K = 8192, 27.3 vs 24.3 and 101.5 vs 83.9 us)
    constexpr bool ROLL = MB <= 2;
    using IH = std::integral_constant<int, WHOLE && ROLL ? U / 2 : U>;      // how much of the first batch goes out ahead of the prologue
    using IU = std::integral_constant<int, U>;
    const int lim0 = WHOLE ? -1 : nchunk;

    const int stride = gridDim.x * NW;
    int u = blockIdx.x * NW + wave;
    const bool any = u < p.units;
    const char* wp[R];
    const char* np[R];
    // a wave without a unit loads the last unit's first batch and drops it: a branch round the first batch would leave the compiler
    // nothing to count behind the prologue's loads, and their waits would cover the weights again
    unit_ptr(any ? u : p.units - 1, wp);

    // ---- prologue: x (optionally RMS-normalised) -> LDS as bf16 ----
    // One or two rows whose pieces fit the registers: every global load the prologue waits for (x, norm_w) is issued BEFORE the wave's first
    // weight loads.  Loads retire through one counter in issue order, so the prologue's waits then leave the weight loads in flight, and the
    // second norm pass reads x from the registers of the first.  Pieces past K load piece 0 again and are not used.  Half of the first batch
    // goes out ahead of the staging and half behind it: all 16 loads beside the prologue's registers would cost a wave per SIMD, and half
    // of every wave's first batch is more than the memory system holds in flight.
    bool staged = false;
    if constexpr (MB <= 2 && WHOLE) {
        if (p.norm_w && p.M == MB && K <= XN * NTHR * 8) {
            staged = true;
            u16x8 xv[MB][XN];
            f32x4 nw0[XN], nw1[XN];
#pragma unroll
            for (int i = 0; i < XN; ++i) {
                const int k = tid * 8 + i * NTHR * 8, kc = k < K ? k : 0;
#pragma unroll
                for (int m = 0; m < MB; ++m) xv[m][i] = *(const u16x8*)(p.A + (size_t)m * p.lda + kc);
                nw0[i] = *(const f32x4*)(p.norm_w + kc);
                nw1[i] = *(const f32x4*)(p.norm_w + kc + 4);
            }
            __builtin_amdgcn_sched_barrier(0);
            issue(I0{}, IH{}, wp, 0, lim0);
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                bf16_t* xs = (bf16_t*)smem + (size_t)m * K;
                float ss = 0.f;
#pragma unroll
                for (int i = 0; i < XN; ++i) {
                    if (tid * 8 + i * NTHR * 8 < K) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) { const float f = bf16_to_f32(xv[m][i][j]); ss += f * f; }
                    }
                }
                ss = wave_sum(ss);
                __syncthreads();
                if (lane == 0) red[wave] = ss;
                __syncthreads();
                float tot = 0.f;
#pragma unroll
                for (int w2 = 0; w2 < NW; ++w2) tot += red[w2];
                const float rstd = rsqrtf(tot / (float)K + p.norm_eps);
#pragma unroll
                for (int i = 0; i < XN; ++i) {
                    const int k = tid * 8 + i * NTHR * 8;
                    if (k < K) {
                        u16x8 o;
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float wj = j < 4 ? nw0[i][j] : nw1[i][j - 4];
                            o[j] = f32_to_bf16(wj * (bf16_to_f32(xv[m][i][j]) * rstd));
                        }
                        *(u16x8*)(xs + k) = o;
                    }
                }
            }
            // an unconditional use of every register the prologue loaded (pieces past K were skipped above): none is pending any more,
            // so the loads below may take these registers without a wait that would cover the weights already in flight
#pragma unroll
            for (int i = 0; i < XN; ++i) {
#pragma unroll
                for (int m = 0; m < MB; ++m) asm volatile("" ::"v"(xv[m][i]));
                asm volatile("" ::"v"(nw0[i]), "v"(nw1[i]));
            }
            issue(IH{}, IU{}, wp, 0, -1);
        } else if (!p.norm_w && p.M == MB && K <= XC * NTHR * 8) {
            staged = true;
            u32x4 xv[MB][XC];
#pragma unroll
            for (int i = 0; i < XC; ++i) {
                const int k = tid * 8 + i * NTHR * 8, kc = k < K ? k : 0;
#pragma unroll
                for (int m = 0; m < MB; ++m) xv[m][i] = *(const u32x4*)(p.A + (size_t)m * p.lda + kc);
            }
            __builtin_amdgcn_sched_barrier(0);
            issue(I0{}, IH{}, wp, 0, lim0);
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                bf16_t* xs = (bf16_t*)smem + (size_t)m * K;
#pragma unroll
                for (int i = 0; i < XC; ++i) {
                    const int k = tid * 8 + i * NTHR * 8;
                    if (k < K) *(u32x4*)(xs + k) = xv[m][i];
                }
            }
#pragma unroll
            for (int i = 0; i < XC; ++i)
#pragma unroll
                for (int m = 0; m < MB; ++m) asm volatile("" ::"v"(xv[m][i]));      // as above
            issue(IH{}, IU{}, wp, 0, -1);
        }
    }
    // Four or eight rows, or a K past the registers: the first weight loads go out first and the staging loops' waits cover them.  The first
    // norm pass leaves raw x in LDS and the second normalises it there (each thread re-reads what it wrote itself): x crosses the chip once.
    if (!staged) {
        issue(I0{}, IH{}, wp, 0, lim0);
        if constexpr (MB >= 4) {
            // one wave per activation row (rows m = wave, wave + NW, ...): the sum of squares is a wave reduction, no workgroup barrier
            // per row - with 4 or 8 rows the row-after-row form below costs 4-8x the prologue of a single row
            for (int m = wave; m < MB; m += NW) {
                bf16_t* xs = (bf16_t*)smem + (size_t)m * K;
                if (m >= p.M) {
                    for (int k = lane * 8; k < K; k += 64 * 8) *(uint4*)(xs + k) = make_uint4(0, 0, 0, 0);
                    continue;
                }
                const bf16_t* x = p.A + (size_t)m * p.lda;
                if (p.norm_w) {
                    float ss = 0.f;
                    for (int k = lane * 8; k < K; k += 64 * 8) {
                        const u16x8 v = *(const u16x8*)(x + k);
                        *(u16x8*)(xs + k) = v;
#pragma unroll
                        for (int j = 0; j < 8; ++j) { const float f = bf16_to_f32(v[j]); ss += f * f; }
                    }
                    const float rstd = rsqrtf(wave_sum(ss) / (float)K + p.norm_eps);
                    for (int k = lane * 8; k < K; k += 64 * 8) {
                        const u16x8 v = *(const u16x8*)(xs + k);
                        const f32x4 w0 = *(const f32x4*)(p.norm_w + k), w1 = *(const f32x4*)(p.norm_w + k + 4);
                        u16x8 o;
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float wj = j < 4 ? w0[j] : w1[j - 4];
                            o[j] = f32_to_bf16(wj * (bf16_to_f32(v[j]) * rstd));
                        }
                        *(u16x8*)(xs + k) = o;
                    }
                } else {
                    for (int k = lane * 8; k < K; k += 64 * 8) *(uint4*)(xs + k) = *(const uint4*)(x + k);
                }
            }
        } else {
            for (int m = 0; m < MB; ++m) {
                bf16_t* xs = (bf16_t*)smem + (size_t)m * K;
                if (m >= p.M) {
                    for (int k = tid * 8; k < K; k += NTHR * 8) *(uint4*)(xs + k) = make_uint4(0, 0, 0, 0);
                    continue;
                }
                const bf16_t* x = p.A + (size_t)m * p.lda;
                if (p.norm_w) {
                    float ss = 0.f;
                    for (int k = tid * 8; k < K; k += NTHR * 8) {
                        const u16x8 v = *(const u16x8*)(x + k);
                        *(u16x8*)(xs + k) = v;
#pragma unroll
                        for (int j = 0; j < 8; ++j) { const float f = bf16_to_f32(v[j]); ss += f * f; }
                    }
                    ss = wave_sum(ss);
                    __syncthreads();
                    if (lane == 0) red[wave] = ss;
                    __syncthreads();
                    float tot = 0.f;
#pragma unroll
                    for (int w2 = 0; w2 < NW; ++w2) tot += red[w2];
                    const float rstd = rsqrtf(tot / (float)K + p.norm_eps);
                    for (int k = tid * 8; k < K; k += NTHR * 8) {
                        const u16x8 v = *(const u16x8*)(xs + k);
                        const f32x4 w0 = *(const f32x4*)(p.norm_w + k), w1 = *(const f32x4*)(p.norm_w + k + 4);
                        u16x8 o;
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float wj = j < 4 ? w0[j] : w1[j - 4];
                            o[j] = f32_to_bf16(wj * (bf16_to_f32(v[j]) * rstd));
                        }
                        *(u16x8*)(xs + k) = o;
                    }
                } else {
                    for (int k = tid * 8; k < K; k += NTHR * 8) *(uint4*)(xs + k) = *(const uint4*)(x + k);
                }
            }
        }
        if constexpr (WHOLE) issue(IH{}, IU{}, wp, 0, -1);
    }
    __syncthreads();

    // ---- the stream: this wave's units, stride apart ----
    bool inflight = true;      // the batch about to be consumed has been requested
    while (u < p.units) {
        const int un = u + stride;
        const bool has_next = un < p.units;
        if (has_next) unit_ptr(un, np);
        else {
#pragma unroll
            for (int r = 0; r < R; ++r) np[r] = wp[r];
        }
        float acc[R][MB];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int m = 0; m < MB; ++m) acc[r][m] = 0.f;
        // One or two rows: the epilogue's operands are requested now, ahead of the unit's last weight loads, not after the reduction.
        // Every lane loads what lane 63 will use (one address per wave), and loads and uses are unconditional - an operand that does not
        // exist reads x[0] and is dropped by a select - so that the compiler can count these loads like the weights'.
        // Without operands (NOEPI) nothing is requested: every wait between the reduction and the stores would be a wait for these
        // registers, taken with the count of the step form without a refill - a drain of the next unit's loads, once per unit.
        constexpr bool EARLY = MB <= 2;
        static_assert(!NOEPI || (EARLY && !FP8), "the operand-free form: bf16 weights, one or two rows");
        const bool use_bias = p.bias && !swiglu;
        float e_bias[R], e_scale[R];
        bf16_t e_res[R][MB];
        if constexpr (EARLY && !NOEPI) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int row = row_of(u, r);
                if constexpr (FP8) e_scale[r] = p.wscale[row];
                e_bias[r] = *(use_bias ? p.bias + row : (const float*)p.A);
                const int col = swiglu ? u * (R / 2) + (r >> 1) : row;
#pragma unroll
                for (int m = 0; m < MB; ++m) e_res[r][m] = *(p.residual ? p.residual + (size_t)(m < p.M ? m : 0) * p.ldr + col : p.A);
            }
        }

        if constexpr (MODE == GEMV_K_ONE) {
            // the next unit's first batch rides under this unit's only one: the loads stay in flight across the unit boundary
            if (has_next) gemv_step<MB, R, U, NT, FP8, U, U, G>(wreg, acc, smem, K, lane, 0, U, U, np);
            else gemv_step<MB, R, U, NT, FP8, U, 0, G>(wreg, acc, smem, K, lane, 0, U, 0, np);
        } else {
            int c0 = 0;
            if constexpr (WHOLE) {
                const char* rp[R];
                for (; c0 + U <= nchunk; c0 += U) {
                    if (!inflight) issue(I0{}, IU{}, wp, c0, -1);      // only after a unit that ended in a short batch
                    // what follows this batch: the next whole batch of the unit, or - behind the unit's last - the next unit's first
                    const bool more = ROLL && c0 + 2 * U <= nchunk, cross = ROLL && !more && c0 + U == nchunk && has_next;
#pragma unroll
                    for (int r = 0; r < R; ++r) rp[r] = more ? wp[r] + (size_t)(c0 + U) * CHB : np[r];
                    inflight = more || cross;
                    if (inflight) gemv_step<MB, R, U, NT, FP8, U, U>(wreg, acc, smem, K, lane, c0, U, U, rp);
                    else gemv_step<MB, R, U, NT, FP8, U, 0>(wreg, acc, smem, K, lane, c0, U, 0, rp);
                }
            }
            if (c0 < nchunk) {      // a short last batch (K below one batch: the only one)
                if (!inflight) issue(I0{}, IU{}, wp, c0, nchunk);
                gemv_step<MB, R, U, NT, FP8, -1, -1>(wreg, acc, smem, K, lane, c0, nchunk - c0, 0, wp);
                inflight = false;
            }
        }

#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int m = 0; m < MB; ++m) acc[r][m] = wave_sum_lane63(acc[r][m]);     // R x MB reductions per unit: DPP, not LDS shuffles
        if constexpr (EARLY) {
            // every lane runs the arithmetic on what it holds; lane 63 holds the unit's sums and stores
            const bool last = lane == 63;
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                if (swiglu) {
#pragma unroll
                    for (int h = 0; h < R / 2; ++h) {
                        const int j = u * (R / 2) + h;
                        float g = acc[2 * h][m], v = acc[2 * h + 1][m];
                        if constexpr (FP8) { g *= e_scale[2 * h]; v *= e_scale[2 * h + 1]; }
                        float t = act_silu(g) * v;
                        if constexpr (!NOEPI) {
                            const float tr = t + bf16_to_f32(e_res[2 * h][m]);
                            t = p.residual ? tr : t;
                        }
                        if (last && m < p.M) {
                            if (p.out_fp32) ((float*)p.C)[(size_t)m * p.ldc + j] = t;
                            else ((bf16_t*)p.C)[(size_t)m * p.ldc + j] = f32_to_bf16(t);
                        }
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int n = u * R + r;
                        float t = acc[r][m];
                        if constexpr (FP8) t *= e_scale[r];
                        if constexpr (!NOEPI) {
                            const float tb = t + e_bias[r];
                            t = use_bias ? tb : t;
                        }
                        t = apply_act(t, p.act);
                        if constexpr (!NOEPI) {
                            const float tr = t + bf16_to_f32(e_res[r][m]);
                            t = p.residual ? tr : t;
                        }
                        if (last && m < p.M && n < p.N) {
                            if (p.out_fp32) ((float*)p.C)[(size_t)m * p.ldc + n] = t;
                            else ((bf16_t*)p.C)[(size_t)m * p.ldc + n] = f32_to_bf16(t);
                        }
                    }
                }
            }
        } else if (lane == 63) {
            if constexpr (FP8) {      // the row's power-of-two scale, once per output
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float sc = p.wscale[row_of(u, r)];
#pragma unroll
                    for (int m = 0; m < MB; ++m) acc[r][m] *= sc;
                }
            }
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                if (m >= p.M) break;
                if (swiglu) {
#pragma unroll
                    for (int h = 0; h < R / 2; ++h) {
                        const int j = u * (R / 2) + h;
                        float t = act_silu(acc[2 * h][m]) * acc[2 * h + 1][m];
                        if (p.residual) t += bf16_to_f32(p.residual[(size_t)m * p.ldr + j]);
                        if (p.out_fp32) ((float*)p.C)[(size_t)m * p.ldc + j] = t;
                        else ((bf16_t*)p.C)[(size_t)m * p.ldc + j] = f32_to_bf16(t);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int n = u * R + r;
                        if (n >= p.N) break;
                        float t = acc[r][m];
                        if (p.bias) t += p.bias[n];
                        t = apply_act(t, p.act);
                        if (p.residual) t += bf16_to_f32(p.residual[(size_t)m * p.ldr + n]);
                        if (p.out_fp32) ((float*)p.C)[(size_t)m * p.ldc + n] = t;
                        else ((bf16_t*)p.C)[(size_t)m * p.ldc + n] = f32_to_bf16(t);
                    }
                }
            }
        }
        u = un;
#pragma unroll
        for (int r = 0; r < R; ++r) wp[r] = np[r];
    }
}

// Waves per SIMD the compiler must leave room for: what the kernel had before the register ring (the ring's refills tempt the scheduler
// into a second set of weight registers; with this floor it keeps one).  Only the routed R = 2, U = 8 forms are pinned.
constexpr int gemv_min_waves(int MB, int R, int U, bool FP8, int NW) {
    if (R != 2 || U != 8) return 1;            // tuning variants (tools/bench_kernels.py): the compiler's own choice
    if (MB == 1 && !FP8) return 5;              // batch-1 bf16: 96 registers
    if (MB == 8 && FP8 && NW == 4) return 3;    // 8 rows of e4m3: 16 sums beside the widened weights
    return 4;                                   // every other form: 128 registers
}

// MB: activation rows (1,2,4,8); R: weight rows per wave pass (2 or 4); U: chunks (one 16-byte load per lane: 512 bf16 or
// 1024 fp8 weights of a row) in flight per row; NT: non-temporal weight loads; FP8: 1-byte e4m3 weights + per-row scale.  A "unit" is R consecutive weight rows, or for SwiGLU R/2 outputs
// (gate row g, up row g+16 of the [16 gate | 16 up] interleaved layout).
// NW: waves per workgroup.  4 (256 threads, several workgroups per CU) while the staged activations fit 64 KiB; 16 (one
// 1024-thread workgroup per CU sharing one copy of x, up to 160 KiB) for batched decode through the wide down-projection
// (4 rows x 14336 = 112 KiB).
template <int MB, int R, int U, bool NT, bool FP8, int NW = 4>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(gemv_min_waves(MB, R, U, FP8, NW)))) void gemv_bf16_kernel(GemvParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // xs[MB][K] bf16, then scratch
    const int nchunk = p.K / (64 * (FP8 ? 16 : 8));
    if (MB <= 2 && nchunk == U) gemv_body<MB, R, U, NT, FP8, NW, GEMV_K_ONE>(p, smem);      // (4 and 8 rows: their sums need the registers)
    else if (nchunk >= U) gemv_body<MB, R, U, NT, FP8, NW, GEMV_K_MANY>(p, smem);
    else gemv_body<MB, R, U, NT, FP8, NW, GEMV_K_SHORT>(p, smem);
}

// The same stream for a launch without bias and residual (bf16 weights, one or two rows; in the decode step QKV, gate|up and lm_head):
// gemv_body without its early-operand code.  Same sums, same order, same stores.  The launcher picks the K shape (MODE), so a kernel holds
// one body: with the three bodies behind a branch in one kernel, as in gemv_bf16_kernel, hipcc compiles this form's stream with vmcnt(0) at
// its second slot - one drain per unit again, only earlier (that kernel also holds flat loads, and a pending flat load turns every wait into
// a drain; gemv_bf16_kernel's own drain per unit clears them).  One body per kernel: every slot under a counted wait, 86 registers.
// G: gemv_step's refill granularity where K is one batch.
template <int MB, int R, int U, bool NT, int NW, int MODE, int G = 1>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(gemv_min_waves(MB, R, U, false, NW)))) void gemv_bf16_noepi_kernel(GemvParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // xs[MB][K] bf16, then scratch
    static_assert(G == 1 || MODE == GEMV_K_ONE, "the refill granularity belongs to the one-batch stream");
    gemv_body<MB, R, U, NT, false, NW, MODE, true, G>(p, smem);
}

}  // namespace
