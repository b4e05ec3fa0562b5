// Shared-prefix decode attention (gfx950): the n adjacent rows of a group - n samples of one prompt - read the
// prompt's K / V once, from the one cache row that holds it, instead of each row streaming its own copy.
//
//   * rows come in groups of n: group g is rows g*n .. g*n + n - 1; shared[g] (int32, device) leading cache slots of the group live in
//     cache row g*n only.  Row r sees the slots [0, shared[g]) of row g*n and the slots [shared[g], slot[r]] of its OWN row (slot[r]
//     holds the token just appended); with a sliding window only the slots > slot[r] - window of that union.  A row with
//     slot[r] < shared[g] shares nothing this step: it sees its own slots [0, slot[r]].  No other slot is read: key indices are
//     clamped into the visible range of the row they are read from before the load, as attn_append.hip clamps to its last valid slot.
//   * attn_shared_prefix_kernel, grid (nsplit, Hkv * ceil(n * G / 64), groups): the n * G queries of one KV head and group are the
//     stacked rows of attn_append_kernel's query tile (stacked row s = row-in-group * G + head-in-group), 64 per workgroup; each
//     workgroup takes one key split of [0, shared[g]) of row g*n and leaves un-normalised fp32 (O[128], m, l) per (row, q head, split)
//     in the workspace - (0, -inf, 0) where it saw no key.  The window is masked per stacked row.
//   * attn_shared_tail_kernel, grid (Hkv, R), one wave: the row's own slots for its G query heads on the same tile, then the prefix
//     partials merged in - the 16 / G column groups of the tile take every (16 / G)-th split each - normalised, bf16 o[r][h][:].
// Both launches are plain: a workgroup reads only what an earlier launch wrote.  The tile arithmetic (ap_tile) is attn_append_kernel's:
// S^T = K Q^T and O^T += V^T P^T on v_mfma_f32_16x16x32_bf16, fp32 online softmax per lane column, P rounded to bf16 for the MFMA, the
// normaliser summed from the unrounded exponentials.
#include <algorithm>

#include "vz_common.h"

namespace {

constexpr int AP_D = 128;            // head_dim
constexpr int AP_KT = 64;            // keys per tile
constexpr int AP_ROWS = 64;          // stacked query rows per prefix workgroup
constexpr int AP_PART = AP_D + 4;    // floats per partial row: o[128], m, l, pad
constexpr int AP_MAX_SPLIT = 64;
constexpr int AP_TARGET_WGS = 512;   // two workgroups per CU
constexpr int KS_STRIDE = AP_D * 2 + 16;   // bytes per K row in LDS (+16: spreads the 16 rows of a fragment read)
constexpr int VT_STRIDE = AP_KT * 2 + 8;   // bytes per V^T row (d) in LDS
constexpr int NT = AP_KT / 16, DS = AP_D / 32, DT = AP_D / 16, CPK = AP_D / 8;

struct SharedParams {
    const bf16_t *q, *kc, *vc;   // q [R][Hq][128]
    bf16_t* o;                   // [R][Hq][128]
    float* part;                 // [R][Hq][nsplit] x AP_PART
    const int *shared, *slot;
    int R, n, Hq, Hkv, max_ctx, nsplit, window;
    float scale;
};

// One 64-key tile of the cache rows at kbase / vbase, keys key0 .. key0 + 63 (row indices clamped to last_key), against the query
// fragments qf of this lane's stacked row, which sees the keys lo_key .. hi_key: online-softmax update of (oacc, m_run, l_run).
// Every thread of the THREADS-wide workgroup calls it (two barriers); oacc[dt][r] = O[stacked row][d = dt*16 + 4g + r].
template <int THREADS>
__device__ __forceinline__ void ap_tile(char* Ks, char* Vt, const bf16_t* kbase, const bf16_t* vbase, int key0, int last_key,
                                        const bf16x8 (&qf)[DS], int lo_key, int hi_key, float scale, f32x4 (&oacc)[DT], float& m_run,
                                        float& l_run) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int c = lane & 15, g = lane >> 4;
    __syncthreads();  // every wave has finished reading the previous tile
    // ---- stage K row-major ----
#pragma unroll
    for (int i = 0; i < (AP_KT * CPK) / THREADS; ++i) {
        const int ch = i * THREADS + tid;
        const int kr = ch / CPK, dc = ch % CPK;
        const int krow = min(key0 + kr, last_key);
        const uint4 val = *(const uint4*)(kbase + (size_t)krow * AP_D + dc * 8);
        *(uint4*)(Ks + kr * KS_STRIDE + dc * 16) = val;
    }
    // ---- stage V transposed: unit = (key pair, 8-wide d chunk) -> 8 packed 32-bit LDS writes ----
#pragma unroll
    for (int i = 0; i < ((AP_KT / 2) * CPK) / THREADS; ++i) {
        const int u = i * THREADS + tid;
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
            const float s = ok ? sacc[nt][r] * scale : -INFINITY;
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

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// grid (nsplit, ceil(n * G / 64) * Hkv, groups)
__global__ __launch_bounds__(256, 1) void attn_shared_prefix_kernel(SharedParams p) {
    __shared__ __attribute__((aligned(16))) char Ks[AP_KT * KS_STRIDE];
    __shared__ __attribute__((aligned(16))) char Vt[AP_D * VT_STRIDE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int G = p.Hq / p.Hkv;
    const int grp = blockIdx.z, hk = blockIdx.y % p.Hkv, qt = blockIdx.y / p.Hkv;
    const int row0 = grp * p.n;                                    // the cache row that holds the shared slots
    const int shared = clampi(p.shared[grp], 0, p.max_ctx);
    const int nrows = p.n * G;                                     // stacked rows of the group

    // ---- this lane's stacked query row (B operand of S^T = K Q^T): Q[row][h][ds*32 + 8g .. +7] ----
    int srow = qt * AP_ROWS + wave * 16 + c;
    const bool q_valid = srow < nrows;
    if (!q_valid) srow = nrows - 1;
    const int r = row0 + srow / G, h = hk * G + srow % G;
    const bf16_t* qp = p.q + ((size_t)r * p.Hq + h) * AP_D;
    bf16x8 qf[DS];
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) qf[ds] = *(const bf16x8*)(qp + ds * 32 + g * 8);
    const int slot = clampi(p.slot[r], 0, p.max_ctx - 1);
    const int hi_key = slot >= shared ? shared - 1 : -1;                       // last visible shared slot (none: the row shares nothing)
    const int lo_key = p.window > 0 ? slot - p.window + 1 : 0;                 // first visible slot

    // first shared slot any row of this workgroup sees (uniform over the workgroup); shared = none.  Lane l of every wave looks at row
    // j0 + l of the tile - one batch of loads and a wave reduction instead of a loop of dependent ones
    int wg_lo = shared;
    {
        const int j = (qt * AP_ROWS) / G + lane;
        if (lane < AP_ROWS / G && j < p.n) {
            const int sl = clampi(p.slot[row0 + j], 0, p.max_ctx - 1);
            if (sl >= shared) wg_lo = p.window > 0 ? max(0, sl - p.window + 1) : 0;
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) wg_lo = min(wg_lo, __shfl_xor(wg_lo, off, 64));
        wg_lo = __builtin_amdgcn_readfirstlane(wg_lo);
    }
    int t_begin = wg_lo / AP_KT, t_end = wg_lo < shared ? (shared + AP_KT - 1) / AP_KT : t_begin;
    {
        const int per = (t_end - t_begin + p.nsplit - 1) / p.nsplit;
        t_begin += (int)blockIdx.x * per;
        t_end = min(t_end, t_begin + per);
    }

    f32x4 oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) oacc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    const bf16_t* kbase = p.kc + ((size_t)row0 * p.Hkv + hk) * (size_t)p.max_ctx * AP_D;
    const bf16_t* vbase = p.vc + ((size_t)row0 * p.Hkv + hk) * (size_t)p.max_ctx * AP_D;
    for (int t = t_begin; t < t_end; ++t)
        ap_tile<256>(Ks, Vt, kbase, vbase, t * AP_KT, shared - 1, qf, lo_key, hi_key, p.scale, oacc, m_run, l_run);

    // ---- the partial of (row, q head, split); a split or a row without a visible key leaves (0, -inf, 0): weight 0 in the merge ----
    if (!q_valid) return;
    float* pp = p.part + (((size_t)r * p.Hq + h) * p.nsplit + blockIdx.x) * AP_PART;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) *(f32x4*)(pp + dt * 16 + 4 * g) = oacc[dt];
    if (g == 0) *(float2*)(pp + AP_D) = make_float2(m_run, l_run);
}

// grid (Hkv, R), one wave: stacked row c < G is query head hk * G + c of row r; the columns behind them repeat those heads (and share the merge)
__global__ __launch_bounds__(64) void attn_shared_tail_kernel(SharedParams p) {
    __shared__ __attribute__((aligned(16))) char Ks[AP_KT * KS_STRIDE];
    __shared__ __attribute__((aligned(16))) char Vt[AP_D * VT_STRIDE];

    const int lane = threadIdx.x & 63;
    const int c = lane & 15, g = lane >> 4;
    const int G = p.Hq / p.Hkv;
    const int r = blockIdx.y, hk = blockIdx.x;
    const int shared = clampi(p.shared[r / p.n], 0, p.max_ctx);
    const int slot = clampi(p.slot[r], 0, p.max_ctx - 1);
    const int h = hk * G + c % G;
    const bf16_t* qp = p.q + ((size_t)r * p.Hq + h) * AP_D;
    bf16x8 qf[DS];
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) qf[ds] = *(const bf16x8*)(qp + ds * 32 + g * 8);
    const int lo = p.window > 0 ? max(0, slot - p.window + 1) : 0;
    const bool sees = slot >= shared;                              // else: the row shares nothing, its own slots [lo, slot]
    const int start = sees ? max(shared, lo) : lo;                 // (<= slot: the token just appended is always visible)

    f32x4 oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) oacc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    const bf16_t* kbase = p.kc + ((size_t)r * p.Hkv + hk) * (size_t)p.max_ctx * AP_D;
    const bf16_t* vbase = p.vc + ((size_t)r * p.Hkv + hk) * (size_t)p.max_ctx * AP_D;
    for (int key0 = start; key0 <= slot; key0 += AP_KT)
        ap_tile<64>(Ks, Vt, kbase, vbase, key0, slot, qf, start, slot, p.scale, oacc, m_run, l_run);

    // ---- merge the prefix partials of (r, h).  The 16 / G column groups hold the same own result; group `sub` takes the splits sub,
    // sub + 16 / G, .. (group 0 the own slots too) and the groups meet through lane shuffles.  Loads go out MB at a time with the split
    // index clamped, the surplus dropped by a select: no load sits behind a branch.  An empty partial holds m = -inf and takes weight 0
    // (never exp(-inf - -inf)); its O and l are zeros ----
    constexpr int MB = 4;
    const int nsub = 16 / G, sub = c / G;
    const float* pp = p.part + (((size_t)r * p.Hq + h) * p.nsplit) * AP_PART;
    const int last = p.nsplit - 1;
    float m = sub == 0 ? m_run : -INFINITY;
    for (int s0 = sub; s0 < p.nsplit; s0 += MB * nsub) {
        float ms[MB];
#pragma unroll
        for (int i = 0; i < MB; ++i) ms[i] = pp[(size_t)min(s0 + i * nsub, last) * AP_PART + AP_D];
#pragma unroll
        for (int i = 0; i < MB; ++i) m = fmaxf(m, ms[i]);          // (a clamped index repeats a split: the maximum does not mind)
    }
    for (int off = G; off < 16; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    const float w0 = (sub == 0 && m_run != -INFINITY) ? __expf(m_run - m) : 0.f;
    float l = l_run * w0;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { oacc[dt][0] *= w0; oacc[dt][1] *= w0; oacc[dt][2] *= w0; oacc[dt][3] *= w0; }
    for (int s0 = sub; s0 < p.nsplit; s0 += MB * nsub) {
        float2 ml[MB];
        f32x4 o[MB][DT];
#pragma unroll
        for (int i = 0; i < MB; ++i) {
            const float* ps = pp + (size_t)min(s0 + i * nsub, last) * AP_PART;
            ml[i] = *(const float2*)(ps + AP_D);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[i][dt] = *(const f32x4*)(ps + dt * 16 + 4 * g);
        }
#pragma unroll
        for (int i = 0; i < MB; ++i) {
            const float w = (s0 + i * nsub <= last && ml[i].x != -INFINITY) ? __expf(ml[i].x - m) : 0.f;
            l += w * ml[i].y;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                oacc[dt][0] += w * o[i][dt][0]; oacc[dt][1] += w * o[i][dt][1]; oacc[dt][2] += w * o[i][dt][2]; oacc[dt][3] += w * o[i][dt][3];
            }
        }
    }
    for (int off = G; off < 16; off <<= 1) {
        l += __shfl_xor(l, off, 64);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int k = 0; k < 4; ++k) oacc[dt][k] += __shfl_xor(oacc[dt][k], off, 64);
    }
    if (sub != 0) return;
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    bf16_t* op = p.o + ((size_t)r * p.Hq + h) * AP_D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        uint2 pk;
        pk.x = pack_bf16x2(oacc[dt][0] * inv, oacc[dt][1] * inv);
        pk.y = pack_bf16x2(oacc[dt][2] * inv, oacc[dt][3] * inv);
        *(uint2*)(op + dt * 16 + 4 * g) = pk;
    }
}

int key_tiles(int keys) { return (keys + AP_KT - 1) / AP_KT; }

bool shape_ok(int R, int n, int Hq, int Hkv, int max_ctx) {
    return R >= 1 && n >= 2 && n <= 64 && R % n == 0 && R <= 65535 && Hkv >= 1 && Hq >= Hkv && Hq % Hkv == 0 && 16 % (Hq / Hkv) == 0 && Hq <= 65535 &&      // (the tail kernel's 16 columns hold whole head groups)
          
           max_ctx >= 1;
}

}  // namespace

// Key splits of the prefix launch for `groups` groups of n rows whose longest shared prefix is shared_max slots: enough workgroups for
// two per CU, never more than the key tiles (a split without a tile is wasted) or AP_MAX_SPLIT.
int vz_attn_shared_nsplit(int groups, int n, int Hq, int Hkv, int shared_max) {
    const int G = Hq / Hkv;
    const long base = (long)groups * Hkv * ((n * G + AP_ROWS - 1) / AP_ROWS);
    const int want = (int)std::max<long>(1, AP_TARGET_WGS / base);
    return std::max(1, std::min(std::min(want, key_tiles(shared_max)), AP_MAX_SPLIT));
}

// fp32 workspace of the largest split the rule above can choose for any shared prefix up to max_ctx (the rule is non-decreasing in it)
size_t vz_attn_shared_ws_floats(int R, int n, int Hq, int Hkv, int max_ctx) {
    if (!shape_ok(R, n, Hq, Hkv, max_ctx)) return 0;
    return (size_t)R * Hq * vz_attn_shared_nsplit(R / n, n, Hq, Hkv, max_ctx) * AP_PART;
}

int vz_launch_attention_shared(const AttnSharedArgs& a, hipStream_t s) {
    VZ_CHECK_ARG(a.q && a.kc && a.vc && a.o && a.shared && a.slot && a.part, "attention_shared: null pointer");
    VZ_CHECK_ARG(a.head_dim == AP_D, "attention_shared: head_dim %d unsupported (128)", a.head_dim);
    VZ_CHECK_ARG(shape_ok(a.R, a.n, a.Hq, a.Hkv, a.max_ctx), "attention_shared: bad shape R=%d n=%d (2..64 rows per group, R a multiple of it) Hq=%d Hkv=%d max_ctx=%d",
                 a.R, a.n, a.Hq, a.Hkv, a.max_ctx);
    VZ_CHECK_ARG(a.shared_max >= 1 && a.shared_max <= a.max_ctx, "attention_shared: shared_max %d outside [1, max_ctx = %d]", a.shared_max, a.max_ctx);
    const int groups = a.R / a.n;
    const long tiles_q = ((long)a.n * (a.Hq / a.Hkv) + AP_ROWS - 1) / AP_ROWS;
    VZ_CHECK_ARG(tiles_q * a.Hkv <= 65535 && groups <= 65535, "attention_shared: grid too large");
    VZ_CHECK_ARG(((uintptr_t)a.q & 15) == 0 && ((uintptr_t)a.kc & 15) == 0 && ((uintptr_t)a.vc & 15) == 0 && ((uintptr_t)a.o & 15) == 0 &&
                     ((uintptr_t)a.part & 15) == 0, "attention_shared: pointers must be 16-byte aligned");
    VZ_CHECK_ARG(a.nsplit >= 0 && a.window >= 0, "attention_shared: nsplit %d, window %d", a.nsplit, a.window);
    // nsplit 0: the host rule; n >= 1: forced (tests, A/B), cut to the key tiles and to AP_MAX_SPLIT
    const int nsplit = a.nsplit ? std::min(std::min(a.nsplit, key_tiles(a.shared_max)), AP_MAX_SPLIT) : vz_attn_shared_nsplit(groups, a.n, a.Hq, a.Hkv, a.shared_max);
    const size_t need = (size_t)a.R * a.Hq * nsplit * AP_PART;
    VZ_CHECK_ARG(need <= a.part_floats, "attention_shared: workspace of %zu floats, %d splits need %zu", a.part_floats, nsplit, need);
    SharedParams p;
    p.q = a.q; p.kc = a.kc; p.vc = a.vc; p.o = a.o; p.part = a.part; p.shared = a.shared; p.slot = a.slot;
    p.R = a.R; p.n = a.n; p.Hq = a.Hq; p.Hkv = a.Hkv; p.max_ctx = a.max_ctx; p.nsplit = nsplit; p.window = a.window; p.scale = a.scale;
    hipLaunchKernelGGL(attn_shared_prefix_kernel, dim3(nsplit, (unsigned)(tiles_q * a.Hkv), groups), dim3(256), 0, s, p);
    VZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(attn_shared_tail_kernel, dim3(a.Hkv, a.R), dim3(64), 0, s, p);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}
