// Device-side sampling tail of a decode step (SURVEY.md section 8a', last Zephyr row; a13):
//   hf:generation/utils.py `_sample` with do_sample=True = logits[:, -1].float() -> TemperatureLogitsWarper (x / T) ->
//   TopKLogitsWarper (keep x >= k-th largest; HF's GenerationConfig default top_k = 50 applies on the reference's CLI path,
//   ref:vis_zephyr/serve/cli.py:171-182 passes only do_sample + temperature) -> TopPLogitsWarper (sort ascending, drop the
//   prefix whose cumulative softmax mass is <= 1 - top_p, keep >= 1) -> softmax -> torch.multinomial(probs, 1).
//
// One 1024-thread workgroup per row; the row (128 KB of fp32 logits) stays in L2 across the passes:
//   1. max of x = logit / T                                   (division, as the warper divides)
//   2. top-k: exact k-th largest by a 4-pass radix select on the order-preserving key of x (256-bin LDS histograms)
//   3. top-p: Z = sum of w_i = floor(exp(x_i - max) * 2^40) over the kept tokens (integer mass: order-independent, so a
//      replayed graph, an eager step and a second run give the same bits), then a 4-pass radix select ASCENDING on the
//      same key with the histogram weighted by w: smallest key t with mass{key <= t} > (1 - top_p) * Z; keep key >= t
//   3b. (opt-in) HF's further warpers in HF's order, each over the set kept so far: min_p, typical_p,
//      epsilon_cutoff, eta_cutoff.  min_p / epsilon / eta raise the lower threshold on x; typical_p keeps a band of log p that may
//      leave out the most likely token, so the kept set is a key interval [lo, hi].  typical_p's cut is the same mass-weighted
//      radix select as top-p's, keyed by |-log p - H|; the float sums (Z, entropy) have a fixed reduction shape.
//   4. draw: token = argmax_i (x_i + G_i) over the kept tokens, G_i = -log(-log(u_i)) (Gumbel race: P[argmax = i] =
//      softmax(x)_i, the distribution torch.multinomial draws from), u_i = Philox4x32-10(key = seed, counter =
//      (i, row, token counter, 0x565a)) word 0 -> ((w >> 9) + 0.5) * 2^-23; ties -> smallest index.
// torch.multinomial's own bit stream is a property of torch's generator, not of the reference; what is pinned is the
// distribution (tests/test_sampling_gpu.py: chi-square against the warped softmax) and the exact draw against the numpy
// restatement oracle/sampling_oracle.py (same Philox stream).
// The same kernel is the step's tail inside the per-token hipGraph: it publishes the token for the next step, appends it
// to the output ids and advances the per-row position / cache slot / length kept on the device (as argmax_kernel does).
#include <algorithm>

#include "vz_common.h"

namespace {

__device__ __forceinline__ unsigned fkey(float x) {          // ascending-order-preserving key of a float
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned philox_word0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    return philox4x32_10(c0, c1, c2, c3, k0, k1).x;
}

struct SampleShared {
    unsigned hist[256];
    unsigned long long mass[256];
    float redf[16];
    int redi[16];
    unsigned long long redm[16];
    unsigned sel;                 // selected radix bin of the current pass
    unsigned long long carry;     // count / mass still to be found inside the selected bin
};

__device__ __forceinline__ float block_max(float v, SampleShared& sh) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) sh.redf[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sh.redf[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) r = fmaxf(r, sh.redf[w]);
    __syncthreads();
    return r;
}

// fixed reduction shape (see the step recorder below): the same bits eager, replayed and on a second run
__device__ __forceinline__ float block_sum(float v, SampleShared& sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh.redf[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sh.redf[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) r += sh.redf[w];
    __syncthreads();
    return r;
}

// REG (cols <= 32768): the tempered row is staged ONCE in LDS (one batch of 32 global loads per thread) and all passes (maximum, the two
// radix selects, the Gumbel race: up to 11 sweeps) read it from there; the loop form re-reads the row from L2 in every sweep, one
// dependent 4-byte load at a time (the streamer path paid ~80 us per token for it).  Same values, same order-independent sums.
// (Keeping the 32 values in registers spills at 1024 threads per workgroup: 128 VGPRs.)
#define VZ_FOR_LOGITS(BODY)                                                                                          \
    if (REG) {                                                                                                       \
        _Pragma("unroll 8") for (int k = tid; k < cols; k += 1024) { const float x = lx[k]; BODY }                    \
    } else {                                                                                                         \
        for (int k = tid; k < cols; k += 1024) { const float x = lr[k] / temperature; BODY }                         \
    }

// the sweeps of the opt-in step 3b: not unrolled, so that the calls that leave the step out keep the registers they had
#define VZ_FOR_LOGITS_1(BODY)                                                                                        \
    if (REG) {                                                                                                       \
        _Pragma("unroll 1") for (int k = tid; k < cols; k += 1024) { const float x = lx[k]; BODY }                    \
    } else {                                                                                                         \
        _Pragma("unroll 1") for (int k = tid; k < cols; k += 1024) { const float x = lr[k] / temperature; BODY }     \
    }

__device__ __forceinline__ float unfkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Z = sum e_i and S = sum e_i * (x_i - m), e_i = exp(x_i - m), over the tokens whose key lies in [lo, hi]: softmax and entropy
// H = log Z - S / Z of the set kept so far (-inf entries have no mass: skipped, as HF's nansum skips them)
template <bool REG>
__device__ __forceinline__ void kept_sums(const float* __restrict__ lr, int cols, float temperature, float m, unsigned lo, unsigned hi,
                                          SampleShared& sh, float& Z, float& S) {
    const int tid = threadIdx.x;
    extern __shared__ float lx[];
    float z = 0.f, sm = 0.f;
    VZ_FOR_LOGITS_1({
        const unsigned key = fkey(x);
        if (key >= lo && key <= hi && x > -INFINITY) { const float d = x - m; const float e = expf(d); z += e; sm += e * d; }
    })
    Z = block_sum(z, sh);
    S = block_sum(sm, sh);
}

// Step 3b: the kept interval [lo, hi] after min_p, typical_p, epsilon_cutoff and eta_cutoff (HF's order; each sees what the one before
// left; each keeps at least the largest score of its input set).  On entry [lo, hi] = [top-k / top-p threshold, all ones]: the row's
// maximum m is inside.
template <bool REG>
__device__ __forceinline__ void sample_row_warp(const float* __restrict__ lr, int cols, float temperature, const SampleWarp& wp, float m,
                                                SampleShared& sh, unsigned& lo, unsigned& hi) {
    const int tid = threadIdx.x;
    extern __shared__ float lx[];
    float top = m;                                   // the largest kept score
    // ---- min_p: drop p_i < min_p * p_max, p_max = exp(0) / Z ----
    if (wp.min_p > 0.f) lo = max(lo, fkey(m + logf(wp.min_p)));
    // ---- typical_p: ascending in s_i = |-log p_i - H|, the shortest prefix with mass >= typical_p ----
    if (wp.typical_p > 0.f && wp.typical_p < 1.f) {
        float Z, S;
        kept_sums<REG>(lr, cols, temperature, m, lo, hi, sh, Z, S);
        const float logZ = logf(Z), H = logZ - S / Z;
        unsigned long long zi = 0;
        VZ_FOR_LOGITS_1({
            const unsigned key = fkey(x);
            if (key >= lo && key <= hi) zi += (unsigned long long)(expf(x - m) * 1099511627776.0f);
        })
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) zi += __shfl_xor(zi, o, 64);
        if ((tid & 63) == 0) sh.redm[tid >> 6] = zi;
        __syncthreads();
        zi = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) zi += sh.redm[w];
        __syncthreads();
        unsigned long long want = (unsigned long long)((double)wp.typical_p * (double)zi);
        if (want < 1) want = 1;
        // smallest s-key t with mass{s <= t} >= want (s >= 0: its bits ascend with it)
        unsigned prefix = 0, pmask = 0;
        unsigned long long below = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) sh.mass[tid] = 0;
            __syncthreads();
            VZ_FOR_LOGITS_1({
                const unsigned key = fkey(x);
                if (key >= lo && key <= hi && x > -INFINITY) {
                    const unsigned sk = __float_as_uint(fabsf((logZ - (x - m)) - H));
                    if ((sk & pmask) == prefix) atomicAdd(&sh.mass[(sk >> shift) & 255], (unsigned long long)(expf(x - m) * 1099511627776.0f));
                }
            })
            __syncthreads();
            if (tid == 0) {
                unsigned long long cum = below;
                int b = 0;
                for (; b < 255; ++b) { if (cum + sh.mass[b] >= want) break; cum += sh.mass[b]; }
                sh.sel = (unsigned)b; sh.carry = cum;
            }
            __syncthreads();
            prefix |= sh.sel << shift; pmask |= 255u << shift; below = sh.carry;
            __syncthreads();
        }
        // s is monotone in |x - c| step by step in fp32, so {s <= t} is an interval of x: its two ends
        unsigned nlo = 0xffffffffu, nhi = 0u;
        VZ_FOR_LOGITS_1({
            const unsigned key = fkey(x);
            if (key >= lo && key <= hi && x > -INFINITY && __float_as_uint(fabsf((logZ - (x - m)) - H)) <= prefix) { nlo = min(nlo, key); nhi = max(nhi, key); }
        })
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { nlo = min(nlo, (unsigned)__shfl_xor((int)nlo, o, 64)); nhi = max(nhi, (unsigned)__shfl_xor((int)nhi, o, 64)); }
        if ((tid & 63) == 0) { sh.redi[tid >> 6] = (int)nlo; sh.hist[tid >> 6] = nhi; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 16; ++w) { nlo = min(nlo, (unsigned)sh.redi[w]); nhi = max(nhi, sh.hist[w]); }
        __syncthreads();
        if (nlo <= nhi) { lo = nlo; hi = nhi; top = unfkey(hi); }
    }
    // ---- epsilon_cutoff: drop p_i < epsilon ----
    if (wp.epsilon > 0.f && wp.epsilon < 1.f) {
        float Z, S;
        kept_sums<REG>(lr, cols, temperature, m, lo, hi, sh, Z, S);
        lo = max(lo, min(fkey(m + logf(wp.epsilon * Z)), fkey(top)));
    }
    // ---- eta_cutoff: drop p_i < min(eta, sqrt(eta) * exp(-H)) ----
    if (wp.eta > 0.f && wp.eta < 1.f) {
        float Z, S;
        kept_sums<REG>(lr, cols, temperature, m, lo, hi, sh, Z, S);
        const float H = logf(Z) - S / Z;
        const float eta = fminf(wp.eta, sqrtf(wp.eta) * expf(-H));
        lo = max(lo, min(fkey(m + logf(eta * Z)), fkey(top)));
    }
}

// One row's kept set, steps 1..3b above: stages the tempered row (REG), returns the interval's lower key and sets its upper key hi_out -
// a token is kept iff lo <= fkey(x) <= hi - and the maximum m of the tempered row.  Shared by the draw (sample_row_race) and the step
// recorder (token_scores_kernel), so the set a record describes is the set the token was drawn from.
template <bool REG>
__device__ __forceinline__ unsigned sample_row_keep(const float* __restrict__ lr, int cols, float temperature, int top_k, float top_p,
                                                    const SampleWarp& wp, SampleShared& sh, float& m_out, unsigned& hi_out,
                                                    const float* have = nullptr) {
    // have (REG only): the caller's registers already hold the row's batch of loads, have[i] = lr[tid + i * 1024] - staged from there
    const int tid = threadIdx.x;
    extern __shared__ float lx[];          // REG: cols floats
    if (REG) {
        if (have) {
#pragma unroll
            for (int i = 0; i < 32; ++i) { const int k = tid + i * 1024; if (k < cols) lx[k] = have[i] / temperature; }
        } else {
            float t[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) { const int k = tid + i * 1024; t[i] = k < cols ? lr[k] : 0.f; }
#pragma unroll
            for (int i = 0; i < 32; ++i) { const int k = tid + i * 1024; if (k < cols) lx[k] = t[i] / temperature; }
        }
        __syncthreads();
    }

    // ---- 1. max of the tempered logits ----
    float m = -INFINITY;
    VZ_FOR_LOGITS({ m = fmaxf(m, x); })
    m = block_max(m, sh);

    // ---- 2. top-k threshold key (0 = keep everything) ----
    unsigned kth = 0;
    if (top_k > 0 && top_k < cols) {
        unsigned prefix = 0, pmask = 0;
        unsigned long long want = (unsigned long long)top_k;          // rank from the top still to be found
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) sh.hist[tid] = 0;
            __syncthreads();
            VZ_FOR_LOGITS({
                const unsigned key = fkey(x);
                if ((key & pmask) == prefix) atomicAdd(&sh.hist[(key >> shift) & 255], 1u);
            })
            __syncthreads();
            if (tid == 0) {
                unsigned long long cum = 0;
                int b = 255;
                for (; b > 0; --b) { if (cum + sh.hist[b] >= want) break; cum += sh.hist[b]; }
                sh.sel = (unsigned)b; sh.carry = want - cum;
            }
            __syncthreads();
            prefix |= sh.sel << shift; pmask |= 255u << shift; want = sh.carry;
            __syncthreads();
        }
        kth = prefix;
    }

    // ---- 3. top-p threshold key ----
    unsigned pth = 0;
    if (top_p < 1.0f) {
        unsigned long long z = 0;
        VZ_FOR_LOGITS({
            if (fkey(x) >= kth) z += (unsigned long long)(expf(x - m) * 1099511627776.0f);
        })
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
        if ((tid & 63) == 0) sh.redm[tid >> 6] = z;
        __syncthreads();
        z = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) z += sh.redm[w];
        __syncthreads();
        // tokens whose cumulative mass (ascending) is <= (1 - top_p) * Z go; the first one beyond that stays
        const unsigned long long drop = (unsigned long long)((1.0 - (double)top_p) * (double)z);
        unsigned prefix = 0, pmask = 0;
        unsigned long long below = 0;                                  // mass of keys strictly below the current prefix range
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) sh.mass[tid] = 0;
            __syncthreads();
            VZ_FOR_LOGITS({
                const unsigned key = fkey(x);
                if (key >= kth && (key & pmask) == prefix)
                    atomicAdd(&sh.mass[(key >> shift) & 255], (unsigned long long)(expf(x - m) * 1099511627776.0f));
            })
            __syncthreads();
            if (tid == 0) {
                unsigned long long cum = below;
                int b = 0;
                for (; b < 255; ++b) { if (cum + sh.mass[b] > drop) break; cum += sh.mass[b]; }
                sh.sel = (unsigned)b; sh.carry = cum;
            }
            __syncthreads();
            prefix |= sh.sel << shift; pmask |= 255u << shift; below = sh.carry;
            __syncthreads();
        }
        pth = prefix;
    }
    m_out = m;
    unsigned lo = kth > pth ? kth : pth, hi = 0xffffffffu;
    if ((wp.min_p > 0.f || wp.typical_p > 0.f || wp.epsilon > 0.f || wp.eta > 0.f) && m > -INFINITY)
        sample_row_warp<REG>(lr, cols, temperature, wp, m, sh, lo, hi);
    hi_out = hi;
    return lo;
}

// One row's draw, steps 1..4 above, up to each thread's own best (value, index) of the race; `stream_row` = the Philox counter's
// row word.  Shared by the two kernels below, so a row gets the same bits from either.
template <bool REG>
__device__ __forceinline__ void sample_row_race(const float* __restrict__ lr, int cols, float temperature, int top_k, float top_p,
                                                const SampleWarp& wp, unsigned k0, unsigned k1, unsigned stream_row, unsigned c2, SampleShared& sh,
                                                float& bv, int& bi) {
    const int tid = threadIdx.x;
    extern __shared__ float lx[];          // REG: cols floats, staged by sample_row_keep
    float m;
    unsigned keep_hi;
    const unsigned keep = sample_row_keep<REG>(lr, cols, temperature, top_k, top_p, wp, sh, m, keep_hi);

    // ---- 4. Gumbel race over the kept tokens ----
    bv = -INFINITY;
    bi = 0x7fffffff;
    VZ_FOR_LOGITS({
        const unsigned key = fkey(x);
        if (key >= keep && key <= keep_hi) {
            const unsigned w = philox_word0((unsigned)k, stream_row, c2, 0x565au, k0, k1);
            const float u = ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f;       // 2^-23; exact in fp32, inside (0, 1)
            const float v = x - logf(-logf(u));
            if (v > bv || (v == bv && k < bi)) { bv = v; bi = k; }
        }
    })
}

// the workgroup's best of the threads' (value, index): larger value, ties to the smaller index; the result is thread 0's
__device__ __forceinline__ int block_first_best(float bv, int bi, SampleShared& sh) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { sh.redf[tid >> 6] = bv; sh.redi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (sh.redf[w] > bv || (sh.redf[w] == bv && sh.redi[w] < bi)) { bv = sh.redf[w]; bi = sh.redi[w]; }
        if (bi == 0x7fffffff) bi = 0;     // all-NaN row
    }
    return bi;
}

template <bool REG>
__global__ __launch_bounds__(1024) void sample_kernel(const float* __restrict__ logits, int cols, float temperature, int top_k,
                                                      float top_p, SampleWarp wp, const unsigned* __restrict__ seed,
                                                      const int* __restrict__ ctr, int ctr_add, int* __restrict__ ids, RowEmit emit) {
    __shared__ SampleShared sh;
    const int row = blockIdx.x;
    const unsigned c2 = (unsigned)(ctr[0] + ctr_add);
    float bv;
    int bi;
    sample_row_race<REG>(logits + (size_t)row * cols, cols, temperature, top_k, top_p, wp, seed[0], seed[1], (unsigned)row, c2, sh, bv, bi);
    bi = block_first_best(bv, bi, sh);
    if (threadIdx.x == 0) {
        ids[row] = bi;
        vz_emit_advance(emit, row, bi, c2);          // ring slot = draw counter
    }
}

// The per-row tail (continuous batching, n samples of one prompt): every row takes its parameters from its own entry of a table in
// device memory, so re-arming a row changes no kernel argument and a captured step stays valid.  A sampled row draws as sample_kernel
// does when called on that row alone - Philox counter (vocab index, 0, the row's draw counter, 0x565a) under the row's own seed: its
// draws do not depend on the cache row it sits in.  A greedy row takes the first maximal index, as argmax_kernel does.  Then the row's
// draw counter moves on by one (parked rows of a continuous batch step for ever: theirs just counts).
template <bool REG>
__global__ __launch_bounds__(1024) void sample_rows_kernel(const float* __restrict__ logits, int cols, RowSample* tab, int* __restrict__ ids,
                                                           RowEmit emit) {
    __shared__ SampleShared sh;
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* lr = logits + (size_t)row * cols;
    // the entry is the same for every lane: one 48-byte read at the top, held in scalar registers from then on
    const int4 e0 = ((const int4*)(tab + row))[0], e1 = ((const int4*)(tab + row))[1], e2 = ((const int4*)(tab + row))[2];
    const int mode = __builtin_amdgcn_readfirstlane(e0.x), top_k = __builtin_amdgcn_readfirstlane(e0.z);
    const float temperature = __int_as_float(__builtin_amdgcn_readfirstlane(e0.y)), top_p = __int_as_float(__builtin_amdgcn_readfirstlane(e0.w));
    const unsigned k0 = (unsigned)__builtin_amdgcn_readfirstlane(e1.x), k1 = (unsigned)__builtin_amdgcn_readfirstlane(e1.y);
    const int ctr = __builtin_amdgcn_readfirstlane(e1.z);
    const SampleWarp wp{__int_as_float(__builtin_amdgcn_readfirstlane(e2.x)), __int_as_float(__builtin_amdgcn_readfirstlane(e2.y)),
                        __int_as_float(__builtin_amdgcn_readfirstlane(e2.z)), __int_as_float(__builtin_amdgcn_readfirstlane(e2.w))};
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    if (mode == VZ_ROW_GREEDY) {
        if (REG) {          // the row as one batch of loads, as the sampled rows stage it
            float t[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) { const int k = tid + i * 1024; t[i] = k < cols ? lr[k] : -INFINITY; }
#pragma unroll
            for (int i = 0; i < 32; ++i) { const int k = tid + i * 1024; if (k < cols && (t[i] > bv || (t[i] == bv && k < bi))) { bv = t[i]; bi = k; } }
        } else {
            for (int k = tid; k < cols; k += 1024) { const float v = lr[k]; if (v > bv || (v == bv && k < bi)) { bv = v; bi = k; } }
        }
    } else {
        sample_row_race<REG>(lr, cols, temperature, top_k, top_p, wp, k0, k1, 0u, (unsigned)ctr, sh, bv, bi);
    }
    bi = block_first_best(bv, bi, sh);
    if (tid == 0) {
        ids[row] = bi;
        vz_emit_advance(emit, row, bi, emit.ring ? (unsigned)emit.step[1] : 0u);      // ring slot = the draws since decode_begin, as the argmax tail
        tab[row].ctr = ctr + 1;
    }
}

// The sampled verify step of prompt-lookup speculation (spec.hip): the R rows are R consecutive positions of ONE
// sequence, and row i draws the token that position would have drawn in a one-row step - Philox counter (vocab index, 0, w + 1 + i,
// 0x565a) under the call's seed, w = ctl[VZ_SPEC_CTL_WRITE] = the ids generated behind the first.  The stream-row word is 0 for every row:
// the row sits in the draw counter, which is the index of the token in the generated sequence, so the draws do not depend on what was
// guessed.  The record comes by value (scalar registers); the kernel leaves the R ids in g and publishes nothing else - acceptance and
// every state advance are spec_tail_kernel's.  The load of w is requested here, in front of the row's staging loads, as a vector
// load in their queue, and w is first used by the race.  Two things keep it there: the load is an atomic one, which the compiler
// leaves where it stands (the plain scalar load was sunk behind the staging's wait: a round trip of its own), and its address goes
// through a zero the compiler cannot see through, so w counts as a per-lane value and stays in a vector register (a load it knows to
// be uniform is waited for and moved to a scalar register at once: the same round trip, at the head).
template <bool REG>
__global__ __launch_bounds__(1024) void spec_sample_kernel(const float* __restrict__ logits, int cols, RowSample rec, const int* __restrict__ ctl,
                                                           int* __restrict__ g) {
    __shared__ SampleShared sh;
    const int row = blockIdx.x;
    int zero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(zero));          // (no memory access: nothing to count or wait for)
    const int w = __hip_atomic_load(ctl + VZ_SPEC_CTL_WRITE + zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    float bv;
    int bi;
    sample_row_race<REG>(logits + (size_t)row * cols, cols, rec.temp, rec.top_k, rec.top_p, rec.warp, rec.seed[0], rec.seed[1], 0u,
                         (unsigned)(w + 1 + row), sh, bv, bi);
    bi = block_first_best(bv, bi, sh);
    if (threadIdx.x == 0) g[row] = bi;
}

// ---- the step recorder -------------------------------------------------------------------------------------------
// Behind the tail: one 16-byte record per row about the token the tail chose, ids[row]:
//   x_tok    = logits[row, tok] as it stands (in a step: after the logits processors, before temperature); NaN if tok is outside [0, cols)
//   lse      = m + log(sum_i exp(x_i - m)) over the whole row, natural log: the log-partition at temperature 1
//   lse_kept = mT + log(sum_{i kept} exp(x_i / T - mT)) over the set the sampler keeps for the row's (T, top_k, top_p, warpers) - sample_row_keep,
//              the sampler's own; a greedy row: lse
//   n_kept   = size of that set (int32), -inf entries not counted; a greedy row: cols
// and, if asked for, the row HF calls scores[t]: x for a greedy row, x / T where kept and -inf elsewhere for a sampled one.
// Fixed reduction shape - each thread sums its stride-1024 elements in index order, the wave's 64 partials go through wave_sum's fixed
// butterfly, the 16 wave partials are added in index order: a replayed graph, an eager step and a second run give the same bits.  The
// maximum is subtracted first; a row of -inf gives lse = -inf without evaluating (-inf) - (-inf).
__device__ __forceinline__ int block_sum_int(int v, SampleShared& sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh.redi[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) r += sh.redi[w];
    __syncthreads();
    return r;
}

// the recording's place in the rings: slot = (*slot_word) mod cap_steps (null: slot 0, the standalone op), rows = gridDim.x
struct ScoreOut { float* rec; float* warped; const int* slot_word; int cap_steps; };

template <bool REG>
__global__ __launch_bounds__(1024) void token_scores_kernel(const float* __restrict__ logits, int cols, const RowSample* __restrict__ tab,
                                                            RowSample one, const int* __restrict__ ids, ScoreOut out) {
    __shared__ SampleShared sh;
    extern __shared__ float lx[];          // REG: cols floats, staged by sample_row_keep
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* lr = logits + (size_t)row * cols;
    int mode = one.mode, top_k = one.top_k;
    float temperature = one.temp, top_p = one.top_p;
    SampleWarp wp = one.warp;
    if (tab) {          // the per-row table, read as sample_rows_kernel reads it
        const int4 e0 = ((const int4*)(tab + row))[0], e2 = ((const int4*)(tab + row))[2];
        wp = SampleWarp{__int_as_float(__builtin_amdgcn_readfirstlane(e2.x)), __int_as_float(__builtin_amdgcn_readfirstlane(e2.y)),
                        __int_as_float(__builtin_amdgcn_readfirstlane(e2.z)), __int_as_float(__builtin_amdgcn_readfirstlane(e2.w))};
        mode = __builtin_amdgcn_readfirstlane(e0.x); top_k = __builtin_amdgcn_readfirstlane(e0.z);
        temperature = __int_as_float(__builtin_amdgcn_readfirstlane(e0.y)); top_p = __int_as_float(__builtin_amdgcn_readfirstlane(e0.w));
    }
    const int slot = out.slot_word ? (int)((unsigned)out.slot_word[0] % (unsigned)out.cap_steps) : 0;
    const size_t orow = (size_t)slot * gridDim.x + row;
    float* wr = out.warped ? out.warped + orow * cols : nullptr;
    const int tok = ids[row];
    const bool greedy = mode == VZ_ROW_GREEDY;

    // ---- the whole row at temperature 1: max, then the sum of exp(x - max) ----
    float m = -INFINITY, sum = 0.f;
    float t[32];        // REG: the row's one batch of 32 loads per thread, held across the two reductions and staged by sample_row_keep
    if (REG) {
#pragma unroll
        for (int i = 0; i < 32; ++i) { const int k = tid + i * 1024; t[i] = k < cols ? lr[k] : -INFINITY; }
#pragma unroll
        for (int i = 0; i < 32; ++i) m = fmaxf(m, t[i]);
        m = block_max(m, sh);
        if (m > -INFINITY) {
#pragma unroll
            for (int i = 0; i < 32; ++i) sum += expf(t[i] - m);          // (a lane behind the row: exp(-inf) = 0)
        }
        if (wr && greedy) {
#pragma unroll
            for (int i = 0; i < 32; ++i) { const int k = tid + i * 1024; if (k < cols) wr[k] = t[i]; }
        }
    } else {            // batches of 8 loads per thread
        for (int k0 = tid; k0 < cols; k0 += 8 * 1024) {
            float u[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) { const int k = k0 + i * 1024; u[i] = k < cols ? lr[k] : -INFINITY; }
#pragma unroll
            for (int i = 0; i < 8; ++i) m = fmaxf(m, u[i]);
        }
        m = block_max(m, sh);
        for (int k0 = tid; k0 < cols; k0 += 8 * 1024) {
            float u[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) { const int k = k0 + i * 1024; u[i] = k < cols ? lr[k] : -INFINITY; }
            if (m > -INFINITY) {
#pragma unroll
                for (int i = 0; i < 8; ++i) sum += expf(u[i] - m);
            }
            if (wr && greedy) {
#pragma unroll
                for (int i = 0; i < 8; ++i) { const int k = k0 + i * 1024; if (k < cols) wr[k] = u[i]; }
            }
        }
    }
    sum = block_sum(sum, sh);
    const float lse = m > -INFINITY ? m + logf(sum) : -INFINITY;

    // ---- the kept set of a sampled row: the sampler's threshold, then the same sum over the kept tempered values ----
    float lse_kept = lse;
    int n_kept = cols;
    if (!greedy) {
        float mT;
        unsigned keep_hi;
        const unsigned keep = sample_row_keep<REG>(lr, cols, temperature, top_k, top_p, wp, sh, mT, keep_hi, REG ? t : nullptr);
        float sk = 0.f;
        int nk = 0;
        VZ_FOR_LOGITS({
            const unsigned key = fkey(x);
            const bool in = key >= keep && key <= keep_hi;
            if (in && x > -INFINITY) { nk += 1; sk += expf(x - mT); }          // (a -inf entry above the threshold has no mass: not counted)
            if (wr) wr[k] = in ? x : -INFINITY;
        })
        sk = block_sum(sk, sh);
        n_kept = block_sum_int(nk, sh);
        lse_kept = mT > -INFINITY ? mT + logf(sk) : -INFINITY;
    }
    if (tid == 0) {
        float4 r;
        r.x = (tok >= 0 && tok < cols) ? lr[tok] : __int_as_float(0x7fc00000);
        r.y = lse; r.z = lse_kept; r.w = __int_as_float(n_kept);
        ((float4*)out.rec)[orow] = r;
    }
}

// a step's logits rows as they leave the lm_head, into the slot the step's record goes to (what HF calls logits[t])
__global__ __launch_bounds__(256) void score_raw_rows_kernel(const float* __restrict__ logits, long n, float* __restrict__ raw,
                                                             const int* __restrict__ slot_word, int cap_steps) {
    float* dst = raw + (size_t)((unsigned)slot_word[0] % (unsigned)cap_steps) * n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = logits[i];
}

}  // namespace

static bool g_sample_lds_ok = false;
// dynamic-LDS limit of the staged kernel (128 KiB for a 32768-wide row), set once and never inside a stream capture
int vz_init_sampling_kernels() {
    static VzDeviceOnce once;
    if (!vz_device_first(once)) return VZ_OK;
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)sample_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * (int)sizeof(float)));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)sample_rows_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * (int)sizeof(float)));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)token_scores_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * (int)sizeof(float)));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)spec_sample_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * (int)sizeof(float)));
    g_sample_lds_ok = true;
    return VZ_OK;
}

int vz_launch_sample(const float* logits, int rows, int cols, float temperature, int top_k, float top_p, const SampleWarp& warp,
                     const unsigned* seed, const int* ctr, int ctr_add, int* ids, const RowEmit& emit, hipStream_t s) {
    VZ_CHECK_ARG(logits && ids && seed && ctr && rows > 0 && cols > 0 && (!emit.ring || emit.ring_n > 0), "sample: bad argument");
    VZ_CHECK_ARG(temperature > 0.f && top_p > 0.f, "sample: temperature %g and top_p %g must be positive (temperature 0 = greedy: use argmax)", (double)temperature, (double)top_p);
    { int r = vz_init_sampling_kernels(); if (r) return r; }
    if (cols <= 32768 && g_sample_lds_ok)
        hipLaunchKernelGGL(sample_kernel<true>, dim3(rows), dim3(1024), (size_t)cols * sizeof(float), s, logits, cols, temperature, top_k, top_p, warp, seed, ctr, ctr_add, ids, emit);
    else
        hipLaunchKernelGGL(sample_kernel<false>, dim3(rows), dim3(1024), 0, s, logits, cols, temperature, top_k, top_p, warp, seed, ctr, ctr_add, ids, emit);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}

// tab: one RowSample per row, in device memory (the host entries were checked by whoever wrote them: row_sample_of, engine.hip)
int vz_launch_sample_rows(const float* logits, int rows, int cols, RowSample* tab, int* ids, const RowEmit& emit, hipStream_t s) {
    VZ_CHECK_ARG(logits && ids && tab && rows > 0 && cols > 0 && (!emit.ring || emit.ring_n > 0), "sample_rows: bad argument");
    { int r = vz_init_sampling_kernels(); if (r) return r; }
    if (cols <= 32768 && g_sample_lds_ok)
        hipLaunchKernelGGL(sample_rows_kernel<true>, dim3(rows), dim3(1024), (size_t)cols * sizeof(float), s, logits, cols, tab, ids, emit);
    else
        hipLaunchKernelGGL(sample_rows_kernel<false>, dim3(rows), dim3(1024), 0, s, logits, cols, tab, ids, emit);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}

// the draws of a sampled verify step: R = 2..8 rows of one sequence by the one checked VZ_ROW_SAMPLE record (its counter is not read: the
// counters come from ctl[VZ_SPEC_CTL_WRITE]), the ids into g [R]
int vz_launch_spec_sample(const float* logits, int R, int cols, const RowSample& rec, const int* ctl, int* g, hipStream_t s) {
    VZ_CHECK_ARG(logits && ctl && g && R >= 2 && R <= 8 && cols > 0, "spec_sample: bad argument (2..8 rows)");
    VZ_CHECK_ARG(rec.mode == VZ_ROW_SAMPLE && rec.temp > 0.f && rec.top_p > 0.f, "spec_sample: a VZ_ROW_SAMPLE record with temperature %g > 0 and top_p %g > 0 expected", (double)rec.temp, (double)rec.top_p);
    { int r = vz_init_sampling_kernels(); if (r) return r; }
    if (cols <= 32768 && g_sample_lds_ok)
        hipLaunchKernelGGL(spec_sample_kernel<true>, dim3(R), dim3(1024), (size_t)cols * sizeof(float), s, logits, cols, rec, ctl, g);
    else
        hipLaunchKernelGGL(spec_sample_kernel<false>, dim3(R), dim3(1024), 0, s, logits, cols, rec, ctl, g);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}

// The step recorder on `rows` rows of fp32 logits about the tokens ids[row]: tab = the rows' entries in device memory (the per-row tail's
// table) or null = every row by `one`.  slot_word / cap_steps: the ring slot (null: slot 0); rec [slots][rows][4], warped [slots][rows][cols] or null.
int vz_launch_token_scores(const float* logits, int rows, int cols, const RowSample* tab, const RowSample& one, const int* ids, float* rec,
                           float* warped, const int* slot_word, int cap_steps, hipStream_t s) {
    VZ_CHECK_ARG(logits && ids && rec && rows > 0 && cols > 0 && (!slot_word || cap_steps > 0), "token_scores: bad argument");
    VZ_CHECK_ARG(tab || one.mode == VZ_ROW_GREEDY || (one.temp > 0.f && one.top_p > 0.f), "token_scores: temperature %g and top_p %g must be positive", (double)one.temp, (double)one.top_p);
    { int r = vz_init_sampling_kernels(); if (r) return r; }
    const ScoreOut out{rec, warped, slot_word, cap_steps};
    if (cols <= 32768 && g_sample_lds_ok)
        hipLaunchKernelGGL(token_scores_kernel<true>, dim3(rows), dim3(1024), (size_t)cols * sizeof(float), s, logits, cols, tab, one, ids, out);
    else
        hipLaunchKernelGGL(token_scores_kernel<false>, dim3(rows), dim3(1024), 0, s, logits, cols, tab, one, ids, out);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}

int vz_launch_score_raw_rows(const float* logits, int rows, int cols, float* raw, const int* slot_word, int cap_steps, hipStream_t s) {
    VZ_CHECK_ARG(logits && raw && slot_word && rows > 0 && cols > 0 && cap_steps > 0, "score_raw_rows: bad argument");
    const long n = (long)rows * cols;
    hipLaunchKernelGGL(score_raw_rows_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 2048)), dim3(256), 0, s, logits, n, raw, slot_word, cap_steps);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}
