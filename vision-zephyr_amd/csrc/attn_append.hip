// Append attention (gfx950): new[b] query tokens of cache row b against that row's KV cache, whose slots
// past[b] .. past[b] + new[b] - 1 already hold the new tokens' keys and values.
//
//   * past / new are int32 [B] in device memory: rows of a batch may have different cached lengths.  Token i of row b sees the
//     slots j <= past[b] + i (and j > past[b] + i - window with a sliding window) - the rule of the flash kernels with a per-row
//     q_pos0.  Token rows i >= new[b] write nothing; no slot at or behind past[b] + new[b] is read (row indices are clamped to
//     the last valid slot before the load, as flash_attn_kernel clamps to kv_len - 1).
//   * GQA stacking: the Hq / Hkv query heads of one KV head form ONE query tile - stacked row s = token * G + head-in-group, 64
//     stacked rows (4 waves x 16) per workgroup - so a K or V byte is loaded once per KV head, not once per query head.
//   * key split: blockIdx.x cuts the 64-key tiles of the visible range over nsplit workgroups; each leaves un-normalised fp32
//     (O, m, l) in the caller's workspace and attn_append_combine merges them, as attn_decode_combine / flash_split_combine do.
//     nsplit is chosen on the host from max(past + new) and T so that a short append over a long context fills the chip.
// The tile arithmetic is flash_attn_kernel<128, 64>'s: S^T = K Q^T and O^T += V^T P^T on v_mfma_f32_16x16x32_bf16, fp32 online
// softmax per lane column, P rounded to bf16 for the MFMA, the normaliser summed from the unrounded exponentials.
#include <algorithm>

#include "vz_common.h"

namespace {

constexpr int AP_D = 128;            // head_dim
constexpr int AP_KT = 64;            // keys per tile
constexpr int AP_ROWS = 64;          // stacked query rows per workgroup
constexpr int AP_PART = AP_D + 4;    // floats per partial row: o[128], m, l, pad
constexpr int AP_MAX_SPLIT = 64;
constexpr int AP_TARGET_WGS = 512;   // two workgroups per CU

struct AppendParams {
    const bf16_t *q, *kc, *vc;
    bf16_t* o;
    float* part;             // [B][Hq][nsplit][T] x AP_PART
    const int *past, *nnew;
    int B, T, Hq, Hkv, max_ctx, nsplit, window;
    long q_bs, q_ss, q_hs, o_bs, o_ss, o_hs;
    float scale;
};

// grid (nsplit, ceil(T * G / 64) * Hkv, B)
__global__ __launch_bounds__(256, 1) void attn_append_kernel(AppendParams p) {
    constexpr int KS_STRIDE = AP_D * 2 + 16;   // bytes per K row in LDS (+16: spreads the 16 rows of a fragment read)
    constexpr int VT_STRIDE = AP_KT * 2 + 8;   // bytes per V^T row (d) in LDS
    constexpr int NT = AP_KT / 16, DS = AP_D / 32, DT = AP_D / 16, CPK = AP_D / 8;
    __shared__ __attribute__((aligned(16))) char Ks[AP_KT * KS_STRIDE];
    __shared__ __attribute__((aligned(16))) char Vt[AP_D * VT_STRIDE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int G = p.Hq / p.Hkv;
    const int b = blockIdx.z, hk = blockIdx.y % p.Hkv, qt = blockIdx.y / p.Hkv;
    const int past = max(p.past[b], 0);
    const int nw = min(min(p.nnew[b], p.T), p.max_ctx - past);
    const int i0 = (qt * AP_ROWS) / G;                 // first token of this workgroup's stacked rows
    if (nw <= 0 || i0 >= nw) return;                   // (uniform over the workgroup)
    const int i1 = min((qt * AP_ROWS + AP_ROWS - 1) / G, nw - 1);
    const int kv_len = past + nw;

    // ---- this lane's stacked query row (B operand of S^T = K Q^T): Q[tok][h][ds*32 + 8g .. +7] ----
    const int srow = qt * AP_ROWS + wave * 16 + c;
    int tok = srow / G;
    const int h = hk * G + srow % G;
    const bool q_valid = tok < nw;
    if (!q_valid) tok = nw - 1;
    const bf16_t* qp = p.q + (size_t)b * p.q_bs + (size_t)tok * p.q_ss + (size_t)h * p.q_hs;
    bf16x8 qf[DS];
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) qf[ds] = *(const bf16x8*)(qp + ds * 32 + g * 8);
    const int hi_key = past + tok;                                             // last visible slot
    const int lo_key = p.window > 0 ? hi_key - p.window + 1 : 0;               // first visible slot

    f32x4 oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) oacc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    // key tiles this workgroup's tokens i0 .. i1 can see, cut over the splits
    const int k_end = past + i1 + 1;
    const int k_begin = p.window > 0 ? max(0, past + i0 - p.window + 1) : 0;
    int t_begin = k_begin / AP_KT, t_end = (k_end + AP_KT - 1) / AP_KT;
    {
        const int per = (t_end - t_begin + p.nsplit - 1) / p.nsplit;
        t_begin += (int)blockIdx.x * per;
        t_end = min(t_end, t_begin + per);
    }

    const bf16_t* kbase = p.kc + ((size_t)b * p.Hkv + hk) * (size_t)p.max_ctx * AP_D;
    const bf16_t* vbase = p.vc + ((size_t)b * p.Hkv + hk) * (size_t)p.max_ctx * AP_D;
    const int last_key = kv_len - 1;

    for (int t = t_begin; t < t_end; ++t) {
        const int key0 = t * AP_KT;
        __syncthreads();  // every wave has finished reading the previous tile
        // ---- stage K row-major ----
#pragma unroll
        for (int i = 0; i < (AP_KT * CPK) / 256; ++i) {
            const int ch = i * 256 + tid;
            const int kr = ch / CPK, dc = ch % CPK;
            const int krow = min(key0 + kr, last_key);
            const uint4 val = *(const uint4*)(kbase + (size_t)krow * AP_D + dc * 8);
            *(uint4*)(Ks + kr * KS_STRIDE + dc * 16) = val;
        }
        // ---- stage V transposed: unit = (key pair, 8-wide d chunk) -> 8 packed 32-bit LDS writes ----
#pragma unroll
        for (int i = 0; i < ((AP_KT / 2) * CPK) / 256; ++i) {
            const int u = i * 256 + tid;
            const int kp = u % (AP_KT / 2), dc = u / (AP_KT / 2);
            const int r0 = min(key0 + 2 * kp, last_key), r1 = min(key0 + 2 * kp + 1, last_key);
            const u16x8 a = *(const u16x8*)(vbase + (size_t)r0 * AP_D + dc * 8);
            const u16x8 bb = *(const u16x8*)(vbase + (size_t)r1 * AP_D + dc * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                *(unsigned*)(Vt + (dc * 8 + j) * VT_STRIDE + kp * 4) = (unsigned)a[j] | ((unsigned)bb[j] << 16);
        }
        __syncthreads();

        // ---- S^T tiles: sacc[nt][r] = S[key = key0 + nt*16 + 4g + r][q = this lane's stacked row] ----
        f32x4 sacc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            sacc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ds = 0; ds < DS; ++ds) {
                const bf16x8 kf = *(const bf16x8*)(Ks + (nt * 16 + c) * KS_STRIDE + ds * 64 + g * 16);
                sacc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ds], sacc[nt], 0, 0, 0);
            }
        }
        // ---- slot mask + online softmax (per lane column) ----
        float m_tile = -INFINITY;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kidx = key0 + nt * 16 + 4 * g + r;
                const bool ok = (kidx >= lo_key) & (kidx <= hi_key);
                const float s = ok ? sacc[nt][r] * p.scale : -INFINITY;
                sacc[nt][r] = s;
                m_tile = fmaxf(m_tile, s);
            }
        m_tile = rows_max(m_tile);
        const float m_new = fmaxf(m_run, m_tile);
        const float m_safe = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __expf(m_run - m_safe);  // m_run = -inf -> 0
        float psum = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __expf(sacc[nt][r] - m_safe);
                sacc[nt][r] = e;
                psum += e;
            }
        psum = rows_sum(psum);
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            oacc[dt][0] *= alpha; oacc[dt][1] *= alpha; oacc[dt][2] *= alpha; oacc[dt][3] *= alpha;
        }
        // ---- O^T += V^T P^T.  k-slot j of lane group g in k-step s is key  (2s + (j>>2))*16 + 4g + (j&3) ----
#pragma unroll
        for (int s = 0; s < NT / 2; ++s) {
            bf16x8 pf;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pf[r] = (__bf16)sacc[2 * s][r];
                pf[4 + r] = (__bf16)sacc[2 * s + 1][r];
            }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const char* vrow = Vt + (dt * 16 + c) * VT_STRIDE + g * 8;
                const bf16x4 v0 = *(const bf16x4*)(vrow + (2 * s) * 32);
                const bf16x4 v1 = *(const bf16x4*)(vrow + (2 * s + 1) * 32);
                const bf16x8 vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, oacc[dt], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: oacc[dt][r] = O[this lane's stacked row][d = dt*16 + 4g + r] ----
    if (!q_valid) return;
    if (p.nsplit > 1) {      // an empty split leaves (0, -inf, 0): weight 0 in the combine
        float* pp = p.part + ((((size_t)b * p.Hq + h) * p.nsplit + blockIdx.x) * p.T + tok) * AP_PART;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) *(f32x4*)(pp + dt * 16 + 4 * g) = oacc[dt];
        if (g == 0) *(float2*)(pp + AP_D) = make_float2(m_run, l_run);
        return;
    }
    const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
    bf16_t* op = p.o + (size_t)b * p.o_bs + (size_t)tok * p.o_ss + (size_t)h * p.o_hs;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        uint2 pk;
        pk.x = pack_bf16x2(oacc[dt][0] * inv, oacc[dt][1] * inv);
        pk.y = pack_bf16x2(oacc[dt][2] * inv, oacc[dt][3] * inv);
        *(uint2*)(op + dt * 16 + 4 * g) = pk;
    }
}

// grid (T, Hq, B), 256 threads = 8 groups x 32 threads (4 output columns each): group g merges the splits g, g + 8, .. of one
// (token, head) - a chain of ceil(nsplit / 8) dependent iterations instead of nsplit - and group 0 merges the eight through LDS
__global__ __launch_bounds__(256) void attn_append_combine(AppendParams p) {
    __shared__ float gm[8], gl[8];
    __shared__ f32x4 go[8][32];
    const int tok = blockIdx.x, h = blockIdx.y, b = blockIdx.z, grp = threadIdx.x >> 5, col = threadIdx.x & 31, d = col * 4;
    if (tok >= min(min(p.nnew[b], p.T), p.max_ctx - max(p.past[b], 0))) return;      // (uniform over the block)
    const float* pp = p.part + ((((size_t)b * p.Hq + h) * p.nsplit) * p.T + tok) * AP_PART;
    const size_t sstride = (size_t)p.T * AP_PART;
    float m = -INFINITY;
    for (int s = grp; s < p.nsplit; s += 8) m = fmaxf(m, pp[s * sstride + AP_D]);
    float l = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = grp; s < p.nsplit; s += 8) {
        const float ms = pp[s * sstride + AP_D];
        const float w = ms == -INFINITY ? 0.f : __expf(ms - m);
        l += w * pp[s * sstride + AP_D + 1];
        const f32x4 o = *(const f32x4*)(pp + s * sstride + d);
        acc[0] += w * o[0]; acc[1] += w * o[1]; acc[2] += w * o[2]; acc[3] += w * o[3];
    }
    if (col == 0) { gm[grp] = m; gl[grp] = l; }
    go[grp][col] = acc;
    __syncthreads();
    if (grp != 0) return;
    float mm = -INFINITY;
#pragma unroll
    for (int g = 0; g < 8; ++g) mm = fmaxf(mm, gm[g]);
    l = 0.f;
    acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const float w = gm[g] == -INFINITY ? 0.f : __expf(gm[g] - mm);
        const f32x4 o = go[g][col];
        l += w * gl[g];
        acc[0] += w * o[0]; acc[1] += w * o[1]; acc[2] += w * o[2]; acc[3] += w * o[3];
    }
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    uint2 pk;
    pk.x = pack_bf16x2(acc[0] * inv, acc[1] * inv);
    pk.y = pack_bf16x2(acc[2] * inv, acc[3] * inv);
    *(uint2*)(p.o + (size_t)b * p.o_bs + (size_t)tok * p.o_ss + (size_t)h * p.o_hs + d) = pk;
}

int key_tiles(int keys) { return (keys + AP_KT - 1) / AP_KT; }

}  // namespace

// Key splits of an append of T token rows per cache row whose longest row ends at slot kv_max: enough workgroups for two per CU,
// never more than the key tiles (a split without a tile is wasted) or AP_MAX_SPLIT.
int vz_attn_append_nsplit(int B, int T, int Hq, int Hkv, int kv_max) {
    const int G = Hq / Hkv;
    const long base = (long)B * Hkv * ((T * G + AP_ROWS - 1) / AP_ROWS);
    const int want = (int)std::max<long>(1, AP_TARGET_WGS / base);
    return std::max(1, std::min(std::min(want, key_tiles(kv_max)), AP_MAX_SPLIT));
}

// fp32 workspace of the largest split the rule above can choose for any context up to max_ctx.  T * nsplit is bounded by
// T * min(tiles, AP_MAX_SPLIT) and by max(T, AP_TARGET_WGS * (64 / G) / (B * Hkv)) (want <= AP_TARGET_WGS / (B * Hkv * T / (64 / G))):
// both non-decreasing in T and max_ctx, unlike T * nsplit itself.
size_t vz_attn_append_ws_floats(int B, int T, int Hq, int Hkv, int max_ctx) {
    if (B < 1 || T < 1 || Hkv < 1 || Hq < Hkv || Hq % Hkv || AP_ROWS % (Hq / Hkv) || max_ctx < 1) return 0;
    const long tpt = AP_ROWS / (Hq / Hkv);
    const long by_tiles = (long)T * std::min(key_tiles(max_ctx), AP_MAX_SPLIT);
    const long by_wgs = std::max<long>(T, (AP_TARGET_WGS * tpt + (long)B * Hkv - 1) / ((long)B * Hkv));
    return (size_t)B * Hq * (size_t)std::min(by_tiles, by_wgs) * AP_PART;
}

int vz_launch_attention_append(const AttnAppendArgs& a, hipStream_t s) {
    VZ_CHECK_ARG(a.q && a.kc && a.vc && a.o && a.past && a.nnew, "attention_append: null pointer");
    VZ_CHECK_ARG(a.head_dim == AP_D, "attention_append: head_dim %d unsupported (128)", a.head_dim);
    VZ_CHECK_ARG(a.B > 0 && a.T > 0 && a.Hq > 0 && a.Hkv > 0 && a.Hq % a.Hkv == 0 && AP_ROWS % (a.Hq / a.Hkv) == 0 && a.max_ctx > 0 &&
                     a.kv_max >= 1 && a.kv_max <= a.max_ctx,
                 "attention_append: bad shape B=%d T=%d Hq=%d Hkv=%d max_ctx=%d kv_max=%d", a.B, a.T, a.Hq, a.Hkv, a.max_ctx, a.kv_max);
    const long tiles_q = ((long)a.T * (a.Hq / a.Hkv) + AP_ROWS - 1) / AP_ROWS;
    VZ_CHECK_ARG(tiles_q * a.Hkv <= 65535 && a.B <= 65535 && a.Hq <= 65535, "attention_append: grid too large");
    const long strides[] = {a.q_bs, a.q_ss, a.q_hs, a.o_bs, a.o_ss, a.o_hs};
    for (long st : strides) VZ_CHECK_ARG(st % 8 == 0, "attention_append: strides must be multiples of 8 elements");
    VZ_CHECK_ARG(((uintptr_t)a.q & 15) == 0 && ((uintptr_t)a.kc & 15) == 0 && ((uintptr_t)a.vc & 15) == 0 && ((uintptr_t)a.o & 15) == 0 &&
                     ((uintptr_t)a.part & 15) == 0, "attention_append: pointers must be 16-byte aligned");
    VZ_CHECK_ARG(a.nsplit >= 0, "attention_append: nsplit %d", a.nsplit);
    // nsplit 0: the host rule; n >= 1: forced (tests, A/B), cut to the key tiles and to AP_MAX_SPLIT
    const int nsplit = a.nsplit ? std::min(std::min(a.nsplit, key_tiles(a.kv_max)), AP_MAX_SPLIT) : vz_attn_append_nsplit(a.B, a.T, a.Hq, a.Hkv, a.kv_max);
    const size_t need = nsplit > 1 ? (size_t)a.B * a.Hq * nsplit * a.T * AP_PART : 0;
    VZ_CHECK_ARG(need == 0 || (a.part && need <= a.part_floats), "attention_append: workspace of %zu floats, %d splits need %zu", a.part_floats, nsplit, need);
    AppendParams p;
    p.q = a.q; p.kc = a.kc; p.vc = a.vc; p.o = a.o; p.part = a.part; p.past = a.past; p.nnew = a.nnew;
    p.B = a.B; p.T = a.T; p.Hq = a.Hq; p.Hkv = a.Hkv; p.max_ctx = a.max_ctx; p.nsplit = nsplit; p.window = a.window;
    p.q_bs = a.q_bs; p.q_ss = a.q_ss; p.q_hs = a.q_hs; p.o_bs = a.o_bs; p.o_ss = a.o_ss; p.o_hs = a.o_hs;
    p.scale = a.scale;
    hipLaunchKernelGGL(attn_append_kernel, dim3(nsplit, (unsigned)(tiles_q * a.Hkv), a.B), dim3(256), 0, s, p);
    VZ_LAUNCH_CHECK();
    if (nsplit > 1) {
        hipLaunchKernelGGL(attn_append_combine, dim3(a.T, a.Hq, a.B), dim3(256), 0, s, p);
        VZ_LAUNCH_CHECK();
    }
    return VZ_OK;
}
