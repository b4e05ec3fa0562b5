// Classifier-free guidance behind the logits (hf:generation/logits_process.py UnbatchedClassifierFreeGuidanceLogitsProcessor; DESIGN.md
// section 6k).  A guided decode batch holds 2G rows: row r < G is a prompt (the conditional branch), row G + r its negative prompt
// followed by the same generated tokens (the unconditional branch).  cfg_combine_kernel turns the conditional row's logits into HF's
// guided scores in front of the processors and the tail; cfg_follow_kernel, behind the tail, hands the token the conditional row chose to
// its unconditional row and moves that row on.  Both take rows, counts and base pointers only: a captured step stays valid as the
// sequences grow.
#include "vz_common.h"

namespace {

constexpr int CFG_THREADS = 1024, CFG_BATCH = 4;      // per thread and pass step: CFG_BATCH loads of either row in flight together

// four consecutive floats: one 16-byte access where the row's base allows it, four 4-byte ones otherwise
__device__ __forceinline__ f32x4 cfg_load4(const float* p, bool wide) {
    if (wide) return *(const f32x4*)p;
    return (f32x4){p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ void cfg_store4(float* p, f32x4 v, bool wide) {
    if (wide) { *(f32x4*)p = v; return; }
    p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
}

// f(xc, xu) over the elements of a pair of rows.  A thread always takes the same elements in the same order - the quads tid, tid + 1024,
// ... of the first 4 * (cols / 4) elements, then the tail one by one - whether a row's base lets its quads go as 16-byte words (wide_c /
// wide_u) or not: the reductions add the same numbers in the same order for any placement of the rows.  In either part the loads of
// BOTH rows of a step are issued before the first is used (row after row, each load would wait for the one before it).
// STORE: f's value goes back over the conditional element.
template <bool STORE, typename F>
__device__ __forceinline__ void cfg_sweep(float* __restrict__ c, const float* __restrict__ u, int cols, bool wide_c, bool wide_u, int tid, F f) {
    const int nvec = cols >> 2;
    for (int q0 = tid; q0 < nvec; q0 += CFG_BATCH * CFG_THREADS) {
        f32x4 a[CFG_BATCH], b[CFG_BATCH];
#pragma unroll
        for (int i = 0; i < CFG_BATCH; ++i) {
            const int q = q0 + i * CFG_THREADS;
            if (q < nvec) a[i] = cfg_load4(c + (size_t)q * 4, wide_c);
        }
#pragma unroll
        for (int i = 0; i < CFG_BATCH; ++i) {
            const int q = q0 + i * CFG_THREADS;
            if (q < nvec) b[i] = cfg_load4(u + (size_t)q * 4, wide_u);
        }
#pragma unroll
        for (int i = 0; i < CFG_BATCH; ++i) {
            const int q = q0 + i * CFG_THREADS;
            if (q >= nvec) continue;
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = f(a[i][j], b[i][j]);
            if (STORE) cfg_store4(c + (size_t)q * 4, o, wide_c);
        }
    }
    for (int k0 = nvec * 4 + tid; k0 < cols; k0 += CFG_BATCH * CFG_THREADS) {
        float a[CFG_BATCH], b[CFG_BATCH];
#pragma unroll
        for (int i = 0; i < CFG_BATCH; ++i) {
            const int k = k0 + i * CFG_THREADS;
            if (k < cols) a[i] = c[k];
        }
#pragma unroll
        for (int i = 0; i < CFG_BATCH; ++i) {
            const int k = k0 + i * CFG_THREADS;
            if (k < cols) b[i] = u[k];
        }
#pragma unroll
        for (int i = 0; i < CFG_BATCH; ++i) {
            const int k = k0 + i * CFG_THREADS;
            if (k >= cols) continue;
            const float o = f(a[i], b[i]);
            if (STORE) c[k] = o;
        }
    }
}

// A pair of rows of up to CFG_REG_COLS columns held in registers: this thread's quads tid + i * 1024 of either row and its tail element.
constexpr int CFG_REG_QUADS = 8, CFG_REG_COLS = CFG_REG_QUADS * CFG_THREADS * 4;
struct CfgRegs { f32x4 a[CFG_REG_QUADS], b[CFG_REG_QUADS]; float ta, tb; };

// all of it as ONE batch of loads (16 quads and the tail in flight together); the three sweeps then run on registers
__device__ __forceinline__ void cfg_load_rows(CfgRegs& r, const float* __restrict__ c, const float* __restrict__ u, int cols, bool wide_c, bool wide_u, int tid) {
    const int nvec = cols >> 2, kt = nvec * 4 + tid;
#pragma unroll
    for (int i = 0; i < CFG_REG_QUADS; ++i) {
        const int q = tid + i * CFG_THREADS;
        if (q < nvec) r.a[i] = cfg_load4(c + (size_t)q * 4, wide_c);
    }
#pragma unroll
    for (int i = 0; i < CFG_REG_QUADS; ++i) {
        const int q = tid + i * CFG_THREADS;
        if (q < nvec) r.b[i] = cfg_load4(u + (size_t)q * 4, wide_u);
    }
    if (kt < cols) { r.ta = c[kt]; r.tb = u[kt]; }
}

// cfg_sweep over the registers: the same elements in the same order
template <bool STORE, typename F>
__device__ __forceinline__ void cfg_sweep_regs(const CfgRegs& r, float* __restrict__ c, int cols, bool wide_c, int tid, F f) {
    const int nvec = cols >> 2, kt = nvec * 4 + tid;
#pragma unroll
    for (int i = 0; i < CFG_REG_QUADS; ++i) {
        const int q = tid + i * CFG_THREADS;
        if (q >= nvec) continue;
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = f(r.a[i][j], r.b[i][j]);
        if (STORE) cfg_store4(c + (size_t)q * 4, o, wide_c);
    }
    if (kt < cols) {
        const float o = f(r.ta, r.tb);
        if (STORE) c[kt] = o;
    }
}

// both values over the workgroup, in one fixed order: the wave's butterfly, then the 16 wave results in wave order (every thread adds
// the same 16 numbers in the same order, so every thread holds the same bits)
template <bool MAX>
__device__ __forceinline__ void cfg_reduce2(float& x, float& y, float (*sh)[16], int tid) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ox = __shfl_xor(x, o, 64), oy = __shfl_xor(y, o, 64);
        x = MAX ? fmaxf(x, ox) : x + ox;
        y = MAX ? fmaxf(y, oy) : y + oy;
    }
    __syncthreads();          // the previous reduction's readers are done with sh
    if (lane == 0) { sh[0][wave] = x; sh[1][wave] = y; }
    __syncthreads();
    x = sh[0][0]; y = sh[1][0];
#pragma unroll
    for (int w = 1; w < 16; ++w) {
        x = MAX ? fmaxf(x, sh[0][w]) : x + sh[0][w];
        y = MAX ? fmaxf(y, sh[1][w]) : y + sh[1][w];
    }
}

// One workgroup per pair r: cond[r] <- s * (lc - lu) + lu with l = log_softmax of the row, all in fp32 as HF writes it:
// l = (x - max) - log(sum exp(x - max)).  Three sweeps over the two rows (max, sum, write).  REG (cols <= CFG_REG_COLS = 32768): the rows are
// loaded once, as one batch, and the sweeps run on registers; otherwise every sweep reads them again (L2-resident after the first).
// Precondition: the unconditional row is finite (raw model logits).  -inf in the conditional row gives -inf (for s > 0).
template <bool REG>
__global__ __launch_bounds__(CFG_THREADS) void cfg_combine_kernel(float* __restrict__ cond, const float* __restrict__ uncond, int cols, float scale) {
    __shared__ float sh[2][16];
    const int tid = threadIdx.x;
    float* c = cond + (size_t)blockIdx.x * cols;
    const float* u = uncond + (size_t)blockIdx.x * cols;
    const bool wide_c = (((uintptr_t)c) & 15) == 0, wide_u = (((uintptr_t)u) & 15) == 0;
    float mc = -INFINITY, mu = -INFINITY, sc = 0.f, su = 0.f, lsc = 0.f, lsu = 0.f;
    auto f_max = [&](float xc, float xu) { mc = fmaxf(mc, xc); mu = fmaxf(mu, xu); return 0.f; };
    auto f_sum = [&](float xc, float xu) { sc += expf(xc - mc); su += expf(xu - mu); return 0.f; };
    auto f_out = [&](float xc, float xu) {
        const float lc = (xc - mc) - lsc, lu = (xu - mu) - lsu;
        return scale * (lc - lu) + lu;
    };
    CfgRegs r;
    if (REG) cfg_load_rows(r, c, u, cols, wide_c, wide_u, tid);
    if (REG) cfg_sweep_regs<false>(r, c, cols, wide_c, tid, f_max); else cfg_sweep<false>(c, u, cols, wide_c, wide_u, tid, f_max);
    cfg_reduce2<true>(mc, mu, sh, tid);
    if (REG) cfg_sweep_regs<false>(r, c, cols, wide_c, tid, f_sum); else cfg_sweep<false>(c, u, cols, wide_c, wide_u, tid, f_sum);
    cfg_reduce2<false>(sc, su, sh, tid);
    lsc = logf(sc); lsu = logf(su);
    if (REG) cfg_sweep_regs<true>(r, c, cols, wide_c, tid, f_out); else cfg_sweep<true>(c, u, cols, wide_c, wide_u, tid, f_out);
}

// Behind the tail: the unconditional row G + r takes the token row r chose and moves on by the tail's own saturating rule; nothing of it
// goes to the output ids or the token ring.
__global__ void cfg_follow_kernel(int* cur, int* pos, int* slot, int* len, int pairs, int max_ctx, int rope_max) {
    RowEmit t;
    t.pos = pos; t.slot = slot; t.len = len; t.max_ctx = max_ctx; t.rope_max = rope_max;
    for (int r = threadIdx.x; r < pairs; r += blockDim.x) {
        const int tok = cur[r];
        cur[pairs + r] = tok;
        vz_emit_advance(t, pairs + r, tok, 0u);
    }
}

}  // namespace

int vz_launch_cfg_combine(float* cond, const float* uncond, int pairs, int cols, float scale, hipStream_t s) {
    VZ_CHECK_ARG(cond && uncond && pairs > 0 && cols > 0, "cfg_combine: bad argument");
    if (cols <= CFG_REG_COLS) hipLaunchKernelGGL(cfg_combine_kernel<true>, dim3(pairs), dim3(CFG_THREADS), 0, s, cond, uncond, cols, scale);
    else hipLaunchKernelGGL(cfg_combine_kernel<false>, dim3(pairs), dim3(CFG_THREADS), 0, s, cond, uncond, cols, scale);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}

int vz_launch_cfg_follow(int* cur, int* pos, int* slot, int* len, int pairs, int max_ctx, int rope_max, hipStream_t s) {
    VZ_CHECK_ARG(cur && pos && slot && len && pairs > 0 && pairs <= 32, "cfg_follow: bad argument");
    hipLaunchKernelGGL(cfg_follow_kernel, dim3(1), dim3(64), 0, s, cur, pos, slot, len, pairs, max_ctx, rope_max);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}
