// Decode-step attention over the e4m3 mirror of the KV cache (opt-in: vz_engine_kv_fp8), and the mirror's writer.
//
// The mirror holds, next to the bf16 cache [row][kv head][slot][128], the same rows as OCP e4m3 bytes plus ONE fp32 power-of-two scale per
// (row, kv head, slot), for K (after RoPE) and for V - each 128-value row quantised as vz_hip/quant.py::quantize_rows quantises a weight
// row (gemm_fp8.hip: quant_rows_fp8_kernel is the device statement this file repeats): e = the smallest integer with max|x| <= 448 * 2^e
// (0 for an all-zero row), q = e4m3_rne(x * 2^-e), scale = 2^e.  The mirror is a pure function of the bf16 cache.
//
//   kv8_mirror_rows_kernel   (re)builds slots [0, len) of the listed cache rows from the bf16 cache: 16 lanes per slot row.
//   attn_decode_kv8_kernel   the work of attn_decode_body.h - RoPE of the new token's q and k (rounded to bf16 the same way), append of K / V
//                            to the bf16 cache, softmax(q K^T) V over slots [lo, slot], key splits merged by the last arriver - with the
//                            cached slots < slot read from the MIRROR (half the bytes) and the new token's own row used in bf16 as it sits
//                            in LDS; split 0 also appends the new row's quantised form to the mirror.
// One workgroup = (context split, KV head, batch row), 256 threads; 8 lanes per 128-byte key row (16 e4m3 each), 32 key rows per pass, 4 K
// and 4 V rows per lane and 128-key chunk.  The scales never touch the 128 elements: the score is multiplied by ks[key], the probability
// by vs[key] on its way into P V, and the normaliser sums the unscaled probabilities.  e4m3 -> fp32 is v_cvt_pk_f32_fp8 (two values per
// instruction; OCP e4m3 on gfx950 - tests/test_kv8_op_gpu.py holds it against quantize_rows).
// Row indices are clamped to `slot` before the load, never predicated: nothing behind slot[b] is read, and a parked row (slot 0 for ever)
// stays inside its cache row.  Rows a lane loads past the chunk's end are never used (their scores are not stored, P V skips them).
// Partials meet as in attn_decode_body.h (guide section 6 / G16): write-through payload, drained, one relaxed agent-scope ticket per
// workgroup, the last arriver - told by the value its add returned - merges with write-through loads and re-zeroes the ticket.
#include "vz_common.h"

namespace {

constexpr int D = 128;            // head_dim
constexpr int G = 4;              // query heads per KV head
constexpr int CH = 128;           // keys per inner chunk
constexpr int KS = 32;            // key rows per pass (8 lanes each)
constexpr int NR = CH / KS;       // K (and V) rows per lane per chunk
constexpr int PW = G * D + 32;    // floats per partial record: o[4][128] | m[4] l[4] pad (the record of attn_decode_body.h)
constexpr int MAX_SPLITS = 32;

__device__ __forceinline__ void st_sc1(float* p, float v) {
    __hip_atomic_store((unsigned*)p, __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_sc1(const float* p) {
    return __uint_as_float(__hip_atomic_load((const unsigned*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ unsigned long long ld_sc1_x2(const float* p) {
    return __hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the exponent e of a row's scale 2^e from its max |x| (quant_rows_fp8_kernel: 448 = 1.75 * 2^8, no logarithm)
__device__ __forceinline__ int scale_exp(float amax) {
    int e = 0;
    if (amax > 0.f) {
        const unsigned bits = __float_as_uint(amax);
        e = (int)((bits >> 23) & 0xff) - 127 - 8 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
        e = e < -100 ? -100 : (e > 100 ? 100 : e);
    }
    return e;
}
__device__ __forceinline__ float exp2i(int e) { return __uint_as_float((unsigned)(127 + e) << 23); }

// 16 e4m3 (one uint4) -> 16 floats, exact
__device__ __forceinline__ void widen16(const uint4& r, float* f) {
    const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
        const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
        f[4 * i] = lo[0]; f[4 * i + 1] = lo[1]; f[4 * i + 2] = hi[0]; f[4 * i + 3] = hi[1];
    }
}
// 16 bf16 (LDS, 32-byte aligned) -> 16 floats
__device__ __forceinline__ void widen16_bf16(const bf16_t* p, float* f) {
    const u16x8 a = *(const u16x8*)p, b = *(const u16x8*)(p + 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) { f[j] = bf16_to_f32(a[j]); f[8 + j] = bf16_to_f32(b[j]); }
}

// ---- the mirror's writer: slots [0, len[z]) of cache row row[z], every layer of the call, K and V, every KV head ----
// grid (16-slot groups, layers * 2 * Hkv, rows); a DPP row of 16 lanes owns one slot row (8 bf16 per lane).  The byte offset of a mirror
// row equals the element offset of its bf16 row; its scale sits at that offset / 128.
__global__ __launch_bounds__(256) void kv8_mirror_rows_kernel(Kv8MirrorArgs a) {
    const int z = blockIdx.z, y = blockIdx.y;
    const int head = y % a.Hkv, half = (y / a.Hkv) & 1, layer = y / (2 * a.Hkv);
    const int slot = blockIdx.x * 16 + (threadIdx.x >> 4), sub = threadIdx.x & 15;
    if (slot >= a.len[z]) return;          // (a whole DPP row leaves together)
    const size_t off = (size_t)layer * a.layer_elems + (((size_t)a.row[z] * a.Hkv + head) * a.max_ctx + slot) * D;
    const u16x8 v = *(const u16x8*)(a.src[half] + off + sub * 8);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(bf16_to_f32(v[j])));
    amax = fmaxf(amax, dpp_mov<0xb1, 0xf>(amax));
    amax = fmaxf(amax, dpp_mov<0x4e, 0xf>(amax));
    amax = fmaxf(amax, dpp_mov<0x141, 0xf>(amax));
    amax = fmaxf(amax, dpp_mov<0x140, 0xf>(amax));
    const int e = scale_exp(amax);
    const float inv = exp2i(-e);
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf16_to_f32(v[0]) * inv, bf16_to_f32(v[1]) * inv, lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf16_to_f32(v[2]) * inv, bf16_to_f32(v[3]) * inv, lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf16_to_f32(v[4]) * inv, bf16_to_f32(v[5]) * inv, hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf16_to_f32(v[6]) * inv, bf16_to_f32(v[7]) * inv, hi, true);
    *(uint2*)(a.q[half] + off + sub * 8) = make_uint2((unsigned)lo, (unsigned)hi);
    if (sub == 0) a.sc[half][off / D] = exp2i(e);
}

struct Params {
    const bf16_t* qkv; bf16_t *kc, *vc; unsigned char *k8, *v8; float *ks, *vs; bf16_t* o; float* part; unsigned* ticket;
    const float *cosT, *sinT; const int *pos, *slot;
    int B, Hq, Hkv, max_ctx, nsplit, window; float scale;
};

struct Shared {
    __attribute__((aligned(16))) float q_s[G][D];          // rotated, pre-scaled queries
    __attribute__((aligned(32))) bf16_t knew[D], vnew[D];  // the new token's (rotated) K and V
    __attribute__((aligned(16))) float sc[G][CH];          // scores -> probabilities of the chunk
    float stat[3 * G];                                     // per head: alpha | m_run | l_run
    unsigned last_flag;
    __attribute__((aligned(16))) float red[16][G][D];      // P V partial sums per pair of key slots (32 KiB)
};

__global__ __launch_bounds__(256) void attn_decode_kv8_kernel(Params p) {
    __shared__ Shared sm;
    const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int sub = lane & 7, ksl = wave * 8 + (lane >> 3);          // 16-wide d chunk, key slot 0..31
    const int slot = p.slot[b], position = p.pos[b];
    const int len = slot + 1;
    const int lo = p.window > 0 ? max(0, len - p.window) : 0;
    const int span = len - lo;
    // the split rule of attn_decode_body.h: a split takes at least one chunk, the splits beyond that leave at once
    const int per = max(CH, (span + p.nsplit - 1) / p.nsplit);
    const int n_active = (span + per - 1) / per;
    if (split >= n_active) return;
    const int k0 = lo + split * per, k1 = min(len, k0 + per);
    const size_t head_row = ((size_t)b * p.Hkv + hk) * (size_t)p.max_ctx;
    bf16_t* kb = p.kc + head_row * D;
    bf16_t* vb = p.vc + head_row * D;
    unsigned char* k8b = p.k8 + head_row * D;
    unsigned char* v8b = p.v8 + head_row * D;
    float* ksb = p.ks + head_row;
    float* vsb = p.vs + head_row;

    // a chunk's K (V) rows of this lane + their scales; indices clamped to `slot` (row `slot` itself is not in the mirror yet: it is taken
    // from LDS below - reading it while split 0's workgroup appends it is harmless, the value is discarded)
    uint4 kreg[NR], vreg[NR];
    float ksr[NR], vsr[NR];
    auto issue_k = [&](int c0) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int idx = min(c0 + ksl + KS * i, slot);
            kreg[i] = *(const uint4*)(k8b + (size_t)idx * D + sub * 16);
            ksr[i] = ksb[idx];
        }
    };
    auto issue_v = [&](int c0) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int idx = min(c0 + ksl + KS * i, slot);
            vreg[i] = *(const uint4*)(v8b + (size_t)idx * D + sub * 16);
            vsr[i] = vsb[idx];
        }
    };
    // RoPE operands: cos, sin, the q pair (d, d + 64) of head hk*G + wave, and the new token's K pair (wave 0) or V pair (wave 1 uses it)
    const bf16_t* row = p.qkv + (size_t)b * (p.Hq + 2 * p.Hkv) * D;
    const bf16_t* qh = row + (size_t)(hk * G + wave) * D;
    const bf16_t* nh = row + (size_t)(wave == 0 ? p.Hq + hk : p.Hq + p.Hkv + hk) * D;
    const float c = p.cosT[(size_t)position * (D / 2) + lane], s = p.sinT[(size_t)position * (D / 2) + lane];
    const bf16_t qx = qh[lane], qy = qh[lane + 64], nx = nh[lane], ny = nh[lane + 64];
    issue_k(k0);
    issue_v(k0);

    // ---- RoPE: thread (h = wave, pair = lane) rotates (d, d+64) of query head hk*G + h; rounded to bf16 as the stand-alone kernel does ----
    {
        const float x = bf16_to_f32(qx), y = bf16_to_f32(qy);
        sm.q_s[wave][lane] = bf16_to_f32(f32_to_bf16(x * c - y * s)) * p.scale;
        sm.q_s[wave][lane + 64] = bf16_to_f32(f32_to_bf16(y * c + x * s)) * p.scale;
        if (wave == 0) {
            const float kx = bf16_to_f32(nx), ky = bf16_to_f32(ny);
            sm.knew[lane] = f32_to_bf16(kx * c - ky * s);
            sm.knew[lane + 64] = f32_to_bf16(ky * c + kx * s);
        } else if (wave == 1) {
            sm.vnew[lane] = nx;
            sm.vnew[lane + 64] = ny;
        }
    }
    if (tid < G) { sm.stat[G + tid] = -INFINITY; sm.stat[2 * G + tid] = 0.f; }
    __syncthreads();
    if (split == 0) {      // one workgroup per (row, kv head) appends the new row: bf16 to the cache, e4m3 + scale to the mirror
        if (tid < 16) *(uint4*)(kb + (size_t)slot * D + tid * 8) = *(const uint4*)(sm.knew + tid * 8);
        else if (tid < 32) *(uint4*)(vb + (size_t)slot * D + (tid - 16) * 8) = *(const uint4*)(sm.vnew + (tid - 16) * 8);
        if (wave >= 2) {   // wave 2 quantises the K row, wave 3 the V row: lane l holds elements l and l + 64
            const bf16_t* src = wave == 2 ? sm.knew : sm.vnew;
            const float x0 = bf16_to_f32(src[lane]), x1 = bf16_to_f32(src[lane + 64]);
            const int e = scale_exp(wave_max(fmaxf(fabsf(x0), fabsf(x1))));
            const float inv = exp2i(-e);
            const unsigned q2 = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(x0 * inv, x1 * inv, 0, false);
            unsigned char* dst = (wave == 2 ? k8b : v8b) + (size_t)slot * D;
            dst[lane] = (unsigned char)(q2 & 0xffu);
            dst[lane + 64] = (unsigned char)((q2 >> 8) & 0xffu);
            if (lane == 0) (wave == 2 ? ksb : vsb)[slot] = exp2i(e);
        }
    }

    float qr[G][16], acc[G][16];
#pragma unroll
    for (int h = 0; h < G; ++h)
#pragma unroll
        for (int j = 0; j < 16; ++j) { qr[h][j] = sm.q_s[h][sub * 16 + j]; acc[h][j] = 0.f; }

    for (int c0 = k0; c0 < k1; c0 += CH) {
        const int n = min(CH, k1 - c0);
        const int c1 = c0 + CH;
        // ---- scores: s = (q . k8) * ks[key]; the new token's row in bf16 from LDS, scale 1 ----
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int kk = ksl + KS * i;
            const bool is_new = c0 + kk == slot;
            float kf[16];
            if (is_new) widen16_bf16(sm.knew + sub * 16, kf);
            else widen16(kreg[i], kf);
            const float kscale = is_new ? 1.f : ksr[i];
            float sh[G] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 16; ++j)
#pragma unroll
                for (int h = 0; h < G; ++h) sh[h] += qr[h][j] * kf[j];
#pragma unroll
            for (int h = 0; h < G; ++h) {
                // the 8 lanes of a key row hold its 8 d-chunks: quad swaps + half-row mirror, every lane ends with the row's sum
                sh[h] = dpp_add<0xb1, 0xf>(sh[h]); sh[h] = dpp_add<0x4e, 0xf>(sh[h]); sh[h] = dpp_add<0x141, 0xf>(sh[h]);
            }
            if (sub == 0 && kk < n) {
#pragma unroll
                for (int h = 0; h < G; ++h) sm.sc[h][kk] = sh[h] * kscale;
            }
        }
        if (c1 < k1) issue_k(c1);      // the next chunk's K rows pass under the softmax and P V
        __syncthreads();
        // ---- online softmax, wave h owns head h ----
        {
            const float s0 = lane < n ? sm.sc[wave][lane] : -INFINITY;
            const float s1 = lane + 64 < n ? sm.sc[wave][lane + 64] : -INFINITY;
            const float m_old = sm.stat[G + wave];
            const float m_new = fmaxf(m_old, wave_max(fmaxf(s0, s1)));
            const float e0 = __expf(s0 - m_new), e1 = __expf(s1 - m_new);
            if (lane < n) sm.sc[wave][lane] = e0;
            if (lane + 64 < n) sm.sc[wave][lane + 64] = e1;
            const float ps = wave_sum(e0 + e1);
            const float alpha = __expf(m_old - m_new);
            if (lane == 0) { sm.stat[wave] = alpha; sm.stat[G + wave] = m_new; sm.stat[2 * G + wave] = sm.stat[2 * G + wave] * alpha + ps; }
        }
        __syncthreads();
        // ---- O += (P * vs[key]) V ----
        {
            float al[G];
#pragma unroll
            for (int h = 0; h < G; ++h) al[h] = sm.stat[h];
#pragma unroll
            for (int h = 0; h < G; ++h)
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[h][j] *= al[h];
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int kk = ksl + KS * i;
                if (kk < n) {
                    const bool is_new = c0 + kk == slot;
                    float vf[16];
                    if (is_new) widen16_bf16(sm.vnew + sub * 16, vf);
                    else widen16(vreg[i], vf);
                    const float vscale = is_new ? 1.f : vsr[i];
                    float pr[G];
#pragma unroll
                    for (int h = 0; h < G; ++h) pr[h] = sm.sc[h][kk] * vscale;
#pragma unroll
                    for (int j = 0; j < 16; ++j)
#pragma unroll
                        for (int h = 0; h < G; ++h) acc[h][j] += pr[h] * vf[j];
                }
            }
        }
        if (c1 < k1) issue_v(c1);
        __syncthreads();   // sc / stat are rewritten by the next chunk
    }
    // ---- reduce the 32 key slots through LDS in two rounds (slots 0..15 store, slots 16..31 add), write this split's partial ----
    if (ksl < 16) {
#pragma unroll
        for (int h = 0; h < G; ++h)
#pragma unroll
            for (int j = 0; j < 16; j += 4) *(f32x4*)&sm.red[ksl][h][sub * 16 + j] = (f32x4){acc[h][j], acc[h][j + 1], acc[h][j + 2], acc[h][j + 3]};
    }
    __syncthreads();
    if (ksl >= 16) {
#pragma unroll
        for (int h = 0; h < G; ++h)
#pragma unroll
            for (int j = 0; j < 16; j += 4) {
                f32x4* r = (f32x4*)&sm.red[ksl - 16][h][sub * 16 + j];
                *r = *r + (f32x4){acc[h][j], acc[h][j + 1], acc[h][j + 2], acc[h][j + 3]};
            }
    }
    __syncthreads();
    if (n_active == 1) {
        // ONE split covers the row's whole context: nothing to meet - no partial record, no ticket, no re-read
        for (int i = tid; i < G * D; i += 256) {
            const int h = i >> 7, d = i & 127;
            float v = 0.f;
#pragma unroll
            for (int s16 = 0; s16 < 16; ++s16) v += sm.red[s16][h][d];
            const float l = sm.stat[2 * G + h];
            p.o[((size_t)b * p.Hq + hk * G) * D + i] = f32_to_bf16(v * (l > 0.f ? 1.0f / l : 0.f));
        }
        return;
    }
    float* po = p.part + (((size_t)b * p.Hkv + hk) * p.nsplit + split) * PW;
    for (int i = tid; i < G * D; i += 256) {
        const int h = i >> 7, d = i & 127;
        float v = 0.f;
#pragma unroll
        for (int s16 = 0; s16 < 16; ++s16) v += sm.red[s16][h][d];
        st_sc1(po + i, v);
    }
    if (tid < G) { st_sc1(po + G * D + tid, sm.stat[G + tid]); st_sc1(po + G * D + G + tid, sm.stat[2 * G + tid]); }
    // ---- every storing wave drains its stores, then ONE lane takes the ticket; the last arriver merges ----
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const unsigned t = __hip_atomic_fetch_add(p.ticket + (size_t)b * p.Hkv + hk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sm.last_flag = (t == (unsigned)n_active - 1) ? 1u : 0u;
    }
    __syncthreads();   // the wave that added joins this barrier after its add returned; everyone loads behind it
    if (!sm.last_flag) return;
    const float* pp = p.part + ((size_t)b * p.Hkv + hk) * p.nsplit * PW;
    float* wgt = &sm.red[0][0][0];            // [G][64] weights, then [G] 1/l   (red is free again)
    // thread t takes outputs 2t and 2t + 1 (both of head t >> 6): one 8-byte load per split over the compile-time bound, the split index
    // clamped to n_active - 1 instead of a branch around the load; splits >= n_active are left out of the sum by a select
    const int h = tid >> 6;
    unsigned long long pr[MAX_SPLITS];
    {
        const int s2 = tid & 63, scl = min(s2, n_active - 1);
        float ms = ld_sc1(pp + (size_t)scl * PW + G * D + h), ls = ld_sc1(pp + (size_t)scl * PW + G * D + G + h);
#pragma unroll
        for (int s3 = 0; s3 < MAX_SPLITS; ++s3) pr[s3] = ld_sc1_x2(pp + (size_t)min(s3, n_active - 1) * PW + 2 * tid);
        if (s2 >= n_active) { ms = -INFINITY; ls = 0.f; }
        const float m = wave_max(ms);
        const float w = ms == -INFINITY ? 0.f : __expf(ms - m);
        const float l = wave_sum(w * ls);
        wgt[h * 64 + s2] = w;
        if (s2 == 0) wgt[G * 64 + h] = l > 0.f ? 1.0f / l : 0.f;
    }
    __syncthreads();
    {
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int s3 = 0; s3 < MAX_SPLITS; ++s3) {
            const float w = wgt[h * 64 + s3];
            const float t0 = fmaf(w, __uint_as_float((unsigned)pr[s3]), a0), t1 = fmaf(w, __uint_as_float((unsigned)(pr[s3] >> 32)), a1);
            a0 = s3 < n_active ? t0 : a0;
            a1 = s3 < n_active ? t1 : a1;
        }
        const float inv = wgt[G * 64 + h];
        *(unsigned*)(p.o + ((size_t)b * p.Hq + hk * G) * D + 2 * tid) = (unsigned)f32_to_bf16(a0 * inv) | ((unsigned)f32_to_bf16(a1 * inv) << 16);
    }
    if (tid == 0) __hip_atomic_store(p.ticket + (size_t)b * p.Hkv + hk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

int vz_launch_kv8_mirror_rows(const Kv8MirrorArgs& a, hipStream_t s) {
    VZ_CHECK_ARG(a.src[0] && a.src[1] && a.q[0] && a.q[1] && a.sc[0] && a.sc[1] && a.n_layers >= 1 && a.Hkv >= 1 && a.max_ctx >= 1 && a.n >= 1 && a.n <= 64,
                 "kv8_mirror_rows: bad argument (1..64 rows per launch)");
    int len_max = 0;
    for (int i = 0; i < a.n; ++i) {
        VZ_CHECK_ARG(a.row[i] >= 0 && a.len[i] >= 0 && a.len[i] <= a.max_ctx, "kv8_mirror_rows: row %d with %d slots outside the cache (max_ctx %d)", a.row[i], a.len[i], a.max_ctx);
        len_max = std::max(len_max, a.len[i]);
    }
    if (len_max == 0) return VZ_OK;
    hipLaunchKernelGGL(kv8_mirror_rows_kernel, dim3((unsigned)((len_max + 15) / 16), (unsigned)(a.n_layers * 2 * a.Hkv), (unsigned)a.n), dim3(256), 0, s, a);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}

int vz_launch_attn_decode_kv8(const AttnDecodeKv8Args& a, hipStream_t s) {
    VZ_CHECK_ARG(a.D == D && a.Hq == a.Hkv * G, "attn_decode_kv8: needs head_dim 128 and 4 query heads per KV head");
    VZ_CHECK_ARG(a.B >= 1 && a.B <= 64 && a.nsplit >= 1 && a.nsplit <= MAX_SPLITS && a.qkv && a.kc && a.vc && a.k8 && a.v8 && a.ks && a.vs && a.o && a.part && a.ticket &&
                 a.cosT && a.sinT && a.pos && a.slot, "attn_decode_kv8: bad argument (1..64 rows, 1..32 context splits)");
    Params p;
    p.qkv = a.qkv; p.kc = a.kc; p.vc = a.vc; p.k8 = a.k8; p.v8 = a.v8; p.ks = a.ks; p.vs = a.vs; p.o = a.o; p.part = a.part; p.ticket = a.ticket;
    p.cosT = a.cosT; p.sinT = a.sinT; p.pos = a.pos; p.slot = a.slot;
    p.B = a.B; p.Hq = a.Hq; p.Hkv = a.Hkv; p.max_ctx = a.max_ctx; p.nsplit = a.nsplit; p.window = a.window; p.scale = a.scale;
    hipLaunchKernelGGL(attn_decode_kv8_kernel, dim3(a.nsplit, a.Hkv, a.B), dim3(256), 0, s, p);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}
