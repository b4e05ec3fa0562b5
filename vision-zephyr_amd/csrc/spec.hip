// Prompt-lookup speculative decoding of ONE greedy sequence (hf:generation/candidate_generator.py PromptLookupCandidateGenerator;
// hf:generation/utils.py `_assisted_decoding`, greedy branch): a decode step carries R = D + 1 rows of the same sequence - the last
// emitted token and D guessed continuations - and keeps the longest prefix of guesses that equals the argmax the model produces anyway.
//
//   spec_verify_attn_kernel  R x 32 query heads over ONE cache row.  The R new K / V rows are appended first (rope_kv_kernel, a launch of
//        its own: the bits of the stand-alone RoPE + append), so every key is read from the cache.  One workgroup = (key split, KV head)
//        and serves all R x 4 query rows of that KV head from one pass over its K / V slice: S^T = K Q^T on v_mfma_f32_16x16x32_bf16
//        (keys on the accumulator rows, the queries on the lanes), fp32 online softmax, O += P V on the VALU from an LDS copy of the V
//        chunk.  Splits and 64-key chunks sit at ABSOLUTE key positions (split s = keys [s * per, (s + 1) * per)), masked keys contribute
//        exact zeros, and the partials of a query are merged in split order by the last arriver of the KV head: a query's reduction order
//        is a function of key positions only - not of the row it ran in, nor of what the other rows guessed.
//   spec_tail_kernel         after argmax_kernel has reduced the R logit rows (a sampled sequence: after spec_sample_kernel, sampling.hip,
//        has drawn them - row i the draw its position has anyway; the tail does not care how the ids g were chosen): acceptance scan, eos / budget clamp, append of the emitted
//        ids to the output buffer and the history at device-side indices, advance of cur / pos / slot / len of all R rows, one stats
//        record per step; then the draft of the NEXT step - leftmost earlier occurrence of the last n ids (n = max_ngram .. 1, an
//        atomicMin over match positions), or the ids that follow the step's own position in a caller-provided stream (tests, benchmark).
#include "vz_common.h"

namespace spec {

constexpr int D = 128;        // head_dim
constexpr int G = 4;          // query heads per KV head
constexpr int CK = 64;        // keys per chunk (4 waves x one 16-key MFMA tile)
constexpr int NQ_MAX = 32;    // 8 rows x 4 heads
constexpr int SS = 36;        // floats per key row of the score tile in LDS (32 queries + pad; 16-byte aligned rows)

__device__ __forceinline__ void st_sc1(float* p, float v) {
    __hip_atomic_store((unsigned*)p, __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_sc1(const float* p) {
    return __uint_as_float(__hip_atomic_load((const unsigned*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void st2_sc1(float* p, f32x2 v) {       // 8-byte aligned pair
    __hip_atomic_store((unsigned long long*)p, __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ f32x2 ld2_sc1(const float* p) {
    return __builtin_bit_cast(f32x2, __hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

struct VerifyParams {
    const bf16_t* q;      // [R][Hq][D] rotated queries
    const bf16_t* kc;     // cache row of the sequence: [Hkv][max_ctx][D], the R new rows already appended
    const bf16_t* vc;
    bf16_t* o;            // [R][Hq][D]
    float* part;          // [Hkv][nsplit][R * 4 * D + 64]
    unsigned* ticket;     // [Hkv], zero before the first launch; the last arriver re-zeroes it
    const int* slot;      // slot[0] = L: row i sits at cache slot L + i and sees keys [lo_i, L + i]
    int R, Hq, Hkv, max_ctx, nsplit, per, window;
    float scale;
};

struct Shared {
    __attribute__((aligned(16))) bf16_t v_s[CK][D];     // the chunk's V rows
    __attribute__((aligned(16))) float s_s[CK][SS];     // scores -> probabilities, [key][query]
    unsigned last_flag;
};

__global__ __launch_bounds__(256) void spec_verify_attn_kernel(VerifyParams p) {
    __shared__ Shared sm;
    const int split = blockIdx.x, hk = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int R = p.R, NQ = R * G;
    const int L = p.slot[0];
    const int hi = min(L + R - 1, p.max_ctx - 1);                               // last key any row sees (the host keeps L + R inside the cache)
    const int lo_min = p.window > 0 ? max(0, L + 1 - p.window) : 0;             // first key row 0 sees
    const int s_first = lo_min / p.per, s_last = min(hi / p.per, p.nsplit - 1);      // (nsplit x per covers the host's key bound)
    if (split < s_first || split > s_last) return;
    const int n_active = s_last - s_first + 1;
    const int k_begin = max(split * p.per, lo_min & ~(CK - 1)), k_end = min((split + 1) * p.per, hi + 1);
    const bf16_t* kb = p.kc + (size_t)hk * p.max_ctx * D;
    const bf16_t* vb = p.vc + (size_t)hk * p.max_ctx * D;

    // the queries as the MFMA's second operand: lane (c, g) holds query 16 t + c, dims 32 kk + 8 g .. + 7
    bf16x8 qf[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int qi = 16 * t + c;
        const bf16_t* qp = p.q + ((size_t)(qi >> 2) * p.Hq + hk * G + (qi & 3)) * D + g * 8;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            uint4 raw = make_uint4(0, 0, 0, 0);
            if (qi < NQ) raw = *(const uint4*)(qp + kk * 32);
            qf[t][kk] = __builtin_bit_cast(bf16x8, raw);
        }
    }
    // per lane: which keys its two queries (16 t + c) may see
    int q_hi[2], q_lo[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int qi = 16 * t + c, r = qi >> 2;
        q_hi[t] = qi < NQ ? L + r : -1;
        q_lo[t] = p.window > 0 ? max(0, L + r + 1 - p.window) : 0;
    }

    uint4 kreg[4], vreg[4];
    auto issue = [&](int c0) {
        const int key = c0 + 16 * wave + c;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            kreg[kk] = make_uint4(0, 0, 0, 0);
            if (key < k_end) kreg[kk] = *(const uint4*)(kb + (size_t)key * D + kk * 32 + g * 8);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, vk = c0 + (e >> 4);
            vreg[i] = make_uint4(0, 0, 0, 0);
            if (vk < k_end) vreg[i] = *(const uint4*)(vb + (size_t)vk * D + (e & 15) * 8);
        }
    };
    if (k_begin < k_end) issue(k_begin);

    // wave w owns queries 8 w .. 8 w + 7 in the softmax and in P V; lane = key of the chunk (softmax) / dims 2 lane, 2 lane + 1 (P V)
    float m_run[8], l_run[8];
    f32x2 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { m_run[j] = -INFINITY; l_run[j] = 0.f; acc[j] = (f32x2){0.f, 0.f}; }

    for (int c0 = k_begin; c0 < k_end; c0 += CK) {
        // ---- V chunk -> LDS, S^T = K Q^T -> LDS ----
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            *(uint4*)&sm.v_s[e >> 4][(e & 15) * 8] = vreg[i];
        }
        f32x4 sacc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const bf16x8 kf = __builtin_bit_cast(bf16x8, kreg[kk]);
#pragma unroll
            for (int t = 0; t < 2; ++t) sacc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[t][kk], sacc[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kl = 16 * wave + 4 * g + j, key = c0 + kl;          // accumulator row j of lane group g
                const bool vis = key <= q_hi[t] && key >= q_lo[t];
                sm.s_s[kl][16 * t + c] = vis ? sacc[t][j] * p.scale : -INFINITY;
            }
        if (c0 + CK < k_end) issue(c0 + CK);       // the next chunk's rows travel under this chunk's softmax and P V
        __syncthreads();
        // ---- online softmax: lane = key, eight queries per wave ----
        float alpha[8];
        {
            const f32x4 sa = *(const f32x4*)&sm.s_s[lane][8 * wave], sb = *(const f32x4*)&sm.s_s[lane][8 * wave + 4];
            f32x4 pa, pb;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float s = j < 4 ? sa[j] : sb[j - 4];
                const float m_new = fmaxf(m_run[j], wave_max(s));
                const bool none = m_new == -INFINITY;                  // no visible key so far: nothing to scale, nothing to add
                const float e = none ? 0.f : __expf(s - m_new);
                alpha[j] = none ? 1.f : __expf(m_run[j] - m_new);
                l_run[j] = l_run[j] * alpha[j] + wave_sum(e);
                m_run[j] = m_new;
                if (j < 4) pa[j] = e; else pb[j - 4] = e;
            }
            *(f32x4*)&sm.s_s[lane][8 * wave] = pa;
            *(f32x4*)&sm.s_s[lane][8 * wave + 4] = pb;
        }
        __syncthreads();
        // ---- O += P V ----
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] *= alpha[j];
        const int n = min(CK, k_end - c0);
#pragma unroll 4
        for (int k = 0; k < n; ++k) {
            const unsigned v2 = *(const unsigned*)&sm.v_s[k][2 * lane];
            const f32x2 vv = (f32x2){bf16_to_f32(v2 & 0xFFFF), bf16_to_f32(v2 >> 16)};
            const f32x4 pa = *(const f32x4*)&sm.s_s[k][8 * wave], pb = *(const f32x4*)&sm.s_s[k][8 * wave + 4];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float pj = j < 4 ? pa[j] : pb[j - 4];
                acc[j] += pj * vv;                           // (v_pk_fma_f32: both dims of the lane in one instruction)
            }
        }
        __syncthreads();       // v_s / s_s are rewritten by the next chunk
    }

    const int PW = NQ * D + 2 * NQ_MAX;            // floats per partial record: o[NQ][128] | m[32] | l[32]
    if (n_active == 1) {
        // one split holds every key: the merge below with a single partial multiplies by exp(0) = 1 and by the same 1 / l - these bits
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int qi = 8 * wave + j;
            if (qi < NQ) {
                const float inv = l_run[j] > 0.f ? 1.0f / l_run[j] : 0.f;
                *(unsigned*)(p.o + ((size_t)(qi >> 2) * p.Hq + hk * G + (qi & 3)) * D + 2 * lane) = pack_bf16x2(acc[j][0] * inv, acc[j][1] * inv);
            }
        }
        return;
    }
    // ---- this split's partial record (write-through stores), then ONE lane takes the ticket; the last arriver merges (no wait anywhere) ----
    float* po = p.part + ((size_t)hk * p.nsplit + split) * PW;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int qi = 8 * wave + j;
        if (qi < NQ) {
            st2_sc1(po + (size_t)qi * D + 2 * lane, acc[j]);
            if (lane == 0) { st_sc1(po + NQ * D + qi, m_run[j]); st_sc1(po + NQ * D + NQ_MAX + qi, l_run[j]); }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // every storing wave drains its stores
    __syncthreads();
    if (tid == 0) {
        const unsigned t = __hip_atomic_fetch_add(p.ticket + hk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sm.last_flag = (t == (unsigned)n_active - 1) ? 1u : 0u;
    }
    __syncthreads();
    if (!sm.last_flag) return;
    // The merge reads n_active x (32 queries x 130 floats) written by other workgroups: every phase puts all of its loads in flight
    // before it uses the first one (a load per loop trip would be a memory round trip per trip: measured 99 us per launch).
    const float* pp = p.part + ((size_t)hk * p.nsplit + s_first) * PW;
    float* mb = (float*)&sm.v_s[0][0];             // [split][32] running maxima -> merge weights
    float* lb = mb + 64 * NQ_MAX;                  // [split][32] normalisers
    float* invb = &sm.s_s[0][0];                   // [32] 1 / l of the merged query
    {
        const int n_ent = n_active * NQ_MAX;       // <= 64 x 32
        float mv[8], lv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = tid + 256 * u, s = e >> 5, q = e & 31;
            mv[u] = -INFINITY; lv[u] = 0.f;
            if (e < n_ent && q < NQ) { mv[u] = ld_sc1(pp + (size_t)s * PW + NQ * D + q); lv[u] = ld_sc1(pp + (size_t)s * PW + NQ * D + NQ_MAX + q); }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = tid + 256 * u;
            if (e < n_ent) { mb[e] = mv[u]; lb[e] = lv[u]; }
        }
    }
    __syncthreads();
    if (tid < NQ) {
        float m = -INFINITY;
        for (int s = 0; s < n_active; ++s) m = fmaxf(m, mb[s * NQ_MAX + tid]);
        float l = 0.f;
        for (int s = 0; s < n_active; ++s) {       // split order = key order
            const float ms = mb[s * NQ_MAX + tid];
            const float w = ms == -INFINITY ? 0.f : __expf(ms - m);
            l += w * lb[s * NQ_MAX + tid];
            mb[s * NQ_MAX + tid] = w;
        }
        invb[tid] = l > 0.f ? 1.0f / l : 0.f;
    }
    __syncthreads();
    f32x2 a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = (f32x2){0.f, 0.f};
    for (int s0 = 0; s0 < n_active; s0 += 8) {
        f32x2 v[8][8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int qi = 8 * wave + j;
                v[u][j] = (f32x2){0.f, 0.f};
                if (s0 + u < n_active && qi < NQ) v[u][j] = ld2_sc1(pp + (size_t)(s0 + u) * PW + (size_t)qi * D + 2 * lane);
            }
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float w = s0 + u < n_active ? mb[(s0 + u) * NQ_MAX + 8 * wave + j] : 0.f;
                a[j] += w * v[u][j];
            }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int qi = 8 * wave + j;
        if (qi < NQ) {
            const float inv = invb[qi];
            *(unsigned*)(p.o + ((size_t)(qi >> 2) * p.Hq + hk * G + (qi & 3)) * D + 2 * lane) = pack_bf16x2(a[j][0] * inv, a[j][1] * inv);
        }
    }
    if (tid == 0) __hip_atomic_store(p.ticket + hk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------
// the step tail
// ------------------------------------------------------------------------------------------------
struct TailParams {
    const int* g;          // [R] argmax of the R logit rows
    int* cur; int* pos; int* slot; int* len;      // [R] state arrays: cur[0] = last emitted token (the engine: cur[1 .. D] = the drafts)
    int* draft;            // [D] the guesses rows 1 .. D carry
    int* ctl;              // VZ_SPEC_CTL_* words
    int* out; int budget;  // emitted ids, at most `budget` of them
    int* hist; int hist_cap;
    int* stats; int stats_cap;      // [stats_cap][3] = {drafted, accepted, emitted} per step
    const int* stream; int stream_len;
    BeamEos eos;
    int R, max_ngram, source, max_ctx, rope_max, do_accept, do_draft;
};

__device__ __forceinline__ bool is_eos(const BeamEos& e, int t) {
    return (e.n > 0 && t == e.id[0]) || (e.n > 1 && t == e.id[1]) || (e.n > 2 && t == e.id[2]) || (e.n > 3 && t == e.id[3]);
}

__global__ __launch_bounds__(256) void spec_tail_kernel(TailParams p) {
    __shared__ int found;
    const int tid = threadIdx.x, Dn = p.R - 1;
    if (p.do_accept && tid == 0) {
        const int step = p.ctl[VZ_SPEC_CTL_STEPS];
        int drafted = p.ctl[VZ_SPEC_CTL_DRAFTED], used = 0, n = 0;
        if (!p.ctl[VZ_SPEC_CTL_DONE]) {
            int a = 0;
            while (a < Dn && p.draft[a] == p.g[a]) ++a;
            const int w = p.ctl[VZ_SPEC_CTL_WRITE], hl = p.ctl[VZ_SPEC_CTL_HIST];
            int done = 0;
            for (int j = 0; j <= a; ++j) {
                if (w + n >= p.budget) break;
                const int tok = p.g[j];
                p.out[w + n] = tok;
                if (p.hist && hl + n < p.hist_cap) p.hist[hl + n] = tok;
                ++n;
                if (is_eos(p.eos, tok)) { done = 1; break; }
            }
            if (w + n >= p.budget) done = 1;
            p.ctl[VZ_SPEC_CTL_WRITE] = w + n;
            p.ctl[VZ_SPEC_CTL_HIST] = min(hl + n, p.hist_cap);
            p.ctl[VZ_SPEC_CTL_DONE] = done;
            if (n > 0) {
                used = n - 1;
                p.cur[0] = p.g[n - 1];
                // the host keeps base + budget + R inside the cache and the rotary tables (vz_llm_decode_spec); saturate all the same
                const int p0 = p.pos[0] + n, s0 = p.slot[0] + n;
                for (int i = 0; i < p.R; ++i) {
                    p.pos[i] = min(p0 + i, p.rope_max - 1);
                    p.slot[i] = min(s0 + i, p.max_ctx - 1);
                    p.len[i] = p.slot[i] + 1;
                }
            }
        } else {
            drafted = 0;
        }
        if (p.stats && step < p.stats_cap) { p.stats[3 * step] = drafted; p.stats[3 * step + 1] = used; p.stats[3 * step + 2] = n; }
        p.ctl[VZ_SPEC_CTL_STEPS] = step + 1;
    }
    if (!p.do_draft) return;
    if (tid == 0) found = 0x7fffffff;
    __syncthreads();                  // (also: the accept phase's writes to ctl / hist are visible to the workgroup)
    __threadfence_block();
    if (p.source == 1) {
        if (tid == 0) {
            const int w = p.ctl[VZ_SPEC_CTL_WRITE];
            for (int j = 0; j < Dn; ++j) p.draft[j] = w + j < p.stream_len ? p.stream[w + j] : 0;
            p.ctl[VZ_SPEC_CTL_DRAFTED] = Dn;
        }
        return;
    }
    const int hl = p.ctl[VZ_SPEC_CTL_HIST];
    int n_hit = 0, first = 0x7fffffff;
    for (int n = min(p.max_ngram, hl - 1); n >= 1; --n) {
        // windows [idx, idx + n) with a non-empty continuation: idx + n < hl
        for (int idx = tid; idx < hl - n; idx += 256) {
            bool eq = true;
            for (int j = 0; j < n; ++j) {
                const int a = p.hist[idx + j];
                eq = eq && a >= 0 && a == p.hist[hl - n + j];
            }
            if (eq) { atomicMin(&found, idx); break; }         // this thread's later windows lie to the right of it
        }
        __syncthreads();
        first = found;
        __syncthreads();              // everyone has read it before the next size's atomicMin may change it
        if (first != 0x7fffffff) { n_hit = n; break; }
    }
    if (tid == 0) {
        int cnt = 0;
        if (n_hit) {
            const int start = first + n_hit;
            for (int j = 0; j < Dn && start + j < hl; ++j) {
                const int t = p.hist[start + j];
                if (t < 0 || is_eos(p.eos, t)) break;
                p.draft[cnt++] = t;
            }
        }
        p.ctl[VZ_SPEC_CTL_DRAFTED] = cnt;
        for (int j = cnt; j < Dn; ++j) p.draft[j] = 0;         // padded slots are ordinary guesses
    }
}

}  // namespace spec

int vz_launch_spec_verify_attn(const SpecVerifyArgs& a, hipStream_t s) {
    VZ_CHECK_ARG(a.q && a.kc && a.vc && a.o && a.part && a.ticket && a.slot, "attention_verify: null argument");
    VZ_CHECK_ARG(a.R >= 2 && a.R <= 8 && a.Hq == 4 * a.Hkv && a.Hkv >= 1 && a.max_ctx >= 1, "attention_verify: 2..8 rows, 4 query heads per KV head expected (R=%d Hq=%d Hkv=%d)", a.R, a.Hq, a.Hkv);
    VZ_CHECK_ARG(a.nsplit >= 1 && a.nsplit <= 64 && a.key_bound >= 1 && a.key_bound <= a.max_ctx, "attention_verify: nsplit %d (1..64) / key bound %d (1..max_ctx %d)", a.nsplit, a.key_bound, a.max_ctx);
    spec::VerifyParams p;
    p.q = a.q; p.kc = a.kc; p.vc = a.vc; p.o = a.o; p.part = a.part; p.ticket = a.ticket; p.slot = a.slot;
    p.R = a.R; p.Hq = a.Hq; p.Hkv = a.Hkv; p.max_ctx = a.max_ctx; p.nsplit = a.nsplit; p.window = a.window; p.scale = a.scale;
    const int chunks = (a.key_bound + 127) / 128;
    p.per = 128 * ((chunks + a.nsplit - 1) / a.nsplit);        // splits at absolute key positions; nsplit * per >= key_bound
    hipLaunchKernelGGL(spec::spec_verify_attn_kernel, dim3(a.nsplit, a.Hkv), dim3(256), 0, s, p);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}

size_t vz_spec_part_floats(int R, int Hkv, int nsplit) { return (size_t)Hkv * nsplit * ((size_t)R * spec::G * spec::D + 2 * spec::NQ_MAX); }

int vz_launch_spec_tail(const SpecTailArgs& a, hipStream_t s) {
    VZ_CHECK_ARG(a.R >= 2 && a.R <= 8 && a.draft && a.ctl && a.max_ngram >= 1 && a.max_ngram <= 4 && (a.source == 0 || a.source == 1),
                 "spec tail: 2..8 rows, n-gram 1..4, source 0 / 1 expected");
    VZ_CHECK_ARG(!a.do_accept || (a.g && a.cur && a.pos && a.slot && a.len && a.out && a.budget >= 0), "spec tail: accept needs ids, state and an output buffer");
    VZ_CHECK_ARG(!a.do_draft || (a.source == 1 ? (a.stream != nullptr || a.stream_len == 0) : a.hist != nullptr), "spec tail: draft needs a history / stream");
    spec::TailParams p;
    p.g = a.g; p.cur = a.cur; p.draft = a.draft; p.pos = a.pos; p.slot = a.slot; p.len = a.len; p.ctl = a.ctl; p.out = a.out; p.budget = a.budget;
    p.hist = a.hist; p.hist_cap = a.hist_cap; p.stats = a.stats; p.stats_cap = a.stats_cap; p.stream = a.stream; p.stream_len = a.stream_len;
    p.eos = a.eos; p.R = a.R; p.max_ngram = a.max_ngram; p.source = a.source; p.max_ctx = a.max_ctx; p.rope_max = a.rope_max;
    p.do_accept = a.do_accept; p.do_draft = a.do_draft;
    hipLaunchKernelGGL(spec::spec_tail_kernel, dim3(1), dim3(256), 0, s, p);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}
