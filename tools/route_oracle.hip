// The linear dispatch as it was BEFORE csrc/linear_route.hip existed, kept as an oracle for the planner: linear() of engine.hip,
// vz_launch_linear of gemm.hip, the form choice and the knob-9 = 5 rule of vz_launch_skinny, vz_wide_engine_ok, and the bodies of
// vz_op_linear / _fp8 / _rmsnorm / _tiled / _tiled_fp8 / _impl - transcribed with every launch replaced by "return what would have been
// launched".  What a kernel can take (vz_gemv_ok, vz_skinny_ok, vz_skinny_fused_norm_ok, vz_wide_ok, vz_linear_check_common) and the two
// helpers whose bodies only changed name (vz_wide_splits = wide_splits, vz_gemm_use256 = the condition of vz_launch_gemm) come from the
// library.  Host code only; touches no device.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Ivision-zephyr_amd/csrc -Iinclude tools/route_oracle.hip -o route_oracle \
//         -Lvision-zephyr_amd/lib -lviszephyr_hip -Wl,-rpath,$PWD/vision-zephyr_amd/lib          (tools/route_sweep.py oracle does this)
//   route_oracle grid     every combination of the grids below: old dispatch vs vz_plan_linear / vz_op_linear_route, prints the differences
//   route_oracle table    stdin: "k9 k14 k19 entry flags M N K lda ldw act out_fp32" per line; stdout: the old dispatch's route per line
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "linear_route.h"
#include "viszephyr.h"

struct Old { int route, weights, pre_norm, splitk, klass; };
struct Copies { bool wt, w8, w8t; };
alignas(16) static const float some[4] = {0, 0, 0, 0};       // stands for every pointer that exists
static const Old REFUSED{LIN_NONE, 0, 0, 0, 0};

static int old_decode_splitk(int N, int K, int act) {
    if (N & 7) return 0;
    const int tiles_n = (N + 127) / 128;
    if (act == VZ_ACT_SWIGLU) return tiles_n < 384 ? 2 : 0;
    if (K < 8192) return vz_knob(VZ_KNOB_DECODE_SK_SHORT);
    int sk = (512 + tiles_n - 1) / tiles_n;
    if (sk > 16) sk = 16;
    return sk < 1 ? 1 : sk;
}
// vz_launch_skinny: which kernel, which weights
static bool old_persist_ok(const LinearArgs& a) {
    if (!a.norm_w) return false;
    const int steps = a.K >> 6, U = 8;
    return steps % 8 == 0 && (steps / 8) % U == 0 && (size_t)a.M * (a.K + 8) * 2 + (size_t)8 * 2 * 64 * 4 * sizeof(float) <= 160 * 1024;
}
static Old old_skinny(const LinearArgs& a, int pre, int klass) {
    if (!vz_skinny_ok(a)) return REFUSED;
    const int w = a.W8 ? LIN_W_E4M3 : (a.N & 15) == 0 && vz_knob(VZ_KNOB_SKINNY_MODE) != 5 && a.Wt ? LIN_W_BF16_TILED : LIN_W_BF16;
    if (a.M > 16) return Old{LIN_SKINNY_WIDE, w, pre, a.splitk_hint, klass};
    if (vz_knob(VZ_KNOB_SKINNY_MODE) != 2 && old_persist_ok(a) && (a.M >= 3 || vz_knob(VZ_KNOB_SKINNY_MODE) == 3)) return Old{LIN_SKINNY_PERSIST, w, pre, a.splitk_hint, klass};
    return Old{LIN_SKINNY, w, pre, a.splitk_hint, klass};
}
static Old old_tile(LinRoute r, const LinearArgs& a, int pre, int splitk, int klass) {
    return a.norm_w ? REFUSED : Old{r, LIN_W_BF16, pre, splitk, klass};       // "fused RMSNorm prologue exists on the GEMV path only"
}
static Old old_launch_linear(const LinearArgs& a, int pre, int klass) {
    if (vz_knob(VZ_KNOB_SKINNY_MODE) && vz_skinny_ok(a) && !(a.M == 2 && vz_knob(VZ_KNOB_SKINNY_MODE) != 7 && vz_gemv_ok(a))) return old_skinny(a, pre, klass);
    if (vz_gemv_ok(a)) return Old{LIN_GEMV, a.W8 ? LIN_W_E4M3 : LIN_W_BF16, pre, a.splitk_hint, klass};
    if (a.W8) return REFUSED;
    return old_tile(vz_gemm_use256(a) ? LIN_TILE256 : LIN_TILE128, a, pre, a.splitk_hint, klass);
}
// linear() of engine.hip; `a` arrives without any copy attached, W says which copies finalize attached
static Old old_engine_linear(int klass_hint, LinearArgs a, Copies W, int hidden) {
    const int M = a.M, N = a.N, K = a.K;
    const bool norm = a.norm_w != nullptr, fp8 = W.w8;
    if (klass_hint == 1 && M >= 2 && a.ldw == K) {
        a.Wt = W.wt ? (const bf16_t*)some : nullptr;
        if (fp8 && M >= 17 && M <= 64 && W.w8t) {
            LinearArgs t = a;
            t.W8t = (const unsigned char*)some; t.wscale = some; t.W8 = nullptr; t.Wt = nullptr; t.rows_free = true;
            if (norm) { t.lda = K; t.norm_w = nullptr; }
            if (vz_wide_ok(t)) return Old{LIN_WIDE_E4M3, LIN_W_E4M3_TILED, norm, a.splitk_hint, K_GEMV};
        }
    }
    a.rows_free = klass_hint == 1;
    if (fp8) {
        a.W8 = (const unsigned char*)some; a.wscale = some;
        LinearArgs t = a;
        if (M > 16) t.norm_w = nullptr;
        if (!vz_gemv_ok(t) && !(vz_knob(VZ_KNOB_SKINNY_MODE) && vz_skinny_ok(t))) { a.W8 = nullptr; a.wscale = nullptr; }
    }
    if (klass_hint == 1 && M >= 17 && M <= 64 && a.Wt && (!fp8 || M >= std::max(vz_knob(VZ_KNOB_DECODE_TILE_ROWS), 33))) {
        LinearArgs t = a;
        t.W8 = nullptr; t.wscale = nullptr;
        if (norm) { t.lda = K; t.norm_w = nullptr; }
        if (vz_wide_ok(t) && vz_wide_splits(t) == 1) return Old{LIN_WIDE_BF16, LIN_W_BF16_TILED, norm, a.splitk_hint, K_GEMV};
    }
    if (klass_hint == 1 && M >= (fp8 ? std::max(vz_knob(VZ_KNOB_DECODE_TILE_ROWS), 33) : vz_knob(VZ_KNOB_DECODE_TILE_ROWS)) && M <= 64 && vz_knob(VZ_KNOB_SKINNY_MODE) && (K & 63) == 0)
        return Old{LIN_TILE128, LIN_W_BF16, norm, old_decode_splitk(N, K, a.act), K_GEMV};
    if (norm && M > 4 && M <= 64 && K == hidden && vz_knob(VZ_KNOB_SKINNY_MODE) && !(vz_skinny_ok(a) && vz_skinny_fused_norm_ok(a))) {
        LinearArgs t = a;
        t.lda = K; t.norm_w = nullptr;
        if (vz_skinny_ok(t)) return old_skinny(t, 1, K_GEMV);
    }
    if (norm) return old_launch_linear(a, 0, K_GEMV);
    return old_launch_linear(a, 0, vz_gemv_ok(a) || (vz_knob(VZ_KNOB_SKINNY_MODE) && vz_skinny_ok(a)) ? K_GEMV : K_GEMM);
}
// the op-level entry points (entry = VZ_LINEAR_*); `a` carries what the caller passed
static Old old_op(int entry, LinearArgs a) {
    const int M = a.M, N = a.N, K = a.K;
    switch (entry) {
    case VZ_LINEAR_OP: return (a.W8 && !a.wscale) ? REFUSED : old_launch_linear(a, 0, 0);
    case VZ_LINEAR_RMSNORM:
        if (!(a.norm_w && M >= 1 && M <= 16) || !((vz_knob(VZ_KNOB_SKINNY_MODE) && vz_skinny_ok(a)) || vz_gemv_ok(a))) return REFUSED;
        return old_launch_linear(a, 0, 0);
    case VZ_LINEAR_TILED:
        if (!(a.Wt && a.ldw == K && (N & 15) == 0)) return REFUSED;
        if (M >= 17 && vz_wide_ok(a)) return Old{LIN_WIDE_BF16, LIN_W_BF16_TILED, 0, 0, 0};
        return vz_knob(VZ_KNOB_SKINNY_MODE) ? old_skinny(a, 0, 0) : REFUSED;
    case VZ_LINEAR_TILED_FP8:
        if (!(a.W8t && a.wscale && (N & 127) == 0) || !vz_wide_ok(a)) return REFUSED;
        return Old{LIN_WIDE_E4M3, LIN_W_E4M3_TILED, 0, 0, 0};
    case VZ_LINEAR_IMPL + 0: return old_tile(LIN_TILE128, a, 0, 0, 0);
    case VZ_LINEAR_IMPL + 1: return vz_gemv_ok(a) ? Old{LIN_GEMV, LIN_W_BF16, 0, 0, 0} : REFUSED;
    case VZ_LINEAR_IMPL + 2: return old_tile(LIN_TILE256, a, 0, 0, 0);
    case VZ_LINEAR_IMPL + 3: return old_skinny(a, 0, 0);
    case VZ_LINEAR_IMPL + 4: return old_tile(LIN_TILE128, a, 0, old_decode_splitk(N, K, a.act), 0);
    }
    return REFUSED;
}

static LinearArgs mk(int M, int N, int K, int lda, int ldw, int act, int f32, unsigned flags) {
    LinearArgs a;
    const int no = act == VZ_ACT_SWIGLU ? N / 2 : N;
    a.A = (const bf16_t*)some; a.lda = lda; a.W = (const bf16_t*)some; a.ldw = ldw; a.C = (void*)some; a.ldc = no; a.M = M; a.N = N; a.K = K;
    a.bias = (flags & VZ_ROUTE_BIAS) ? some : nullptr; a.residual = (flags & VZ_ROUTE_RESIDUAL) ? (const bf16_t*)some : nullptr; a.ldr = no;
    a.act = act; a.out_fp32 = f32; a.norm_w = (flags & VZ_ROUTE_NORM) ? some : nullptr; a.norm_eps = 1e-5f; a.err = nullptr;
    return a;
}
// the old dispatch's answer in the terms of vz_op_linear_route; for an engine linear the norm scratch has `hidden` columns
static Old old_route(int entry, unsigned flags, int M, int N, int K, int lda, int ldw, int act, int f32, int hidden, int splitk_hint) {
    LinearArgs a = mk(M, N, K, lda, ldw, act, f32, flags);
    a.splitk_hint = splitk_hint;
    if (vz_linear_check_common(a) != VZ_OK) return REFUSED;
    if (entry == VZ_LINEAR_ENGINE)
        return old_engine_linear((flags & VZ_ROUTE_DECODE) ? 1 : 0, a, Copies{(flags & VZ_ROUTE_WT) != 0, (flags & VZ_ROUTE_W8) != 0, (flags & VZ_ROUTE_W8T) != 0}, hidden);
    if (flags & VZ_ROUTE_WT) a.Wt = (const bf16_t*)some;
    if (flags & VZ_ROUTE_W8) a.W8 = (const unsigned char*)some;
    if (flags & VZ_ROUTE_W8T) a.W8t = (const unsigned char*)some;
    if (flags & (VZ_ROUTE_W8 | VZ_ROUTE_W8T)) a.wscale = some;
    return old_op(entry, a);
}

static bool set_knobs(int k9, int k14, int k19) {       // a refused value is reported by the caller's exit status
    return vz_tune_set(VZ_KNOB_SKINNY_MODE, k9) == VZ_OK && vz_tune_set(VZ_KNOB_DECODE_TILE_ROWS, k14) == VZ_OK && vz_tune_set(VZ_KNOB_WIDE_MODE, k19) == VZ_OK;
}

static int table() {
    int k9, k14, k19, entry, flags, M, N, K, lda, ldw, act, f32;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d", &k9, &k14, &k19, &entry, &flags, &M, &N, &K, &lda, &ldw, &act, &f32) == 12) {
        if (!set_knobs(k9, k14, k19)) return 1;
        printf("%s\n", vz_route_name((LinRoute)old_route(entry, flags, M, N, K, lda, ldw, act, f32, K, 0).route));
    }
    return 0;
}

static int grid() {
    const int Ns[] = {6144, 4096, 28672, 32000, 32001, 4000, 3584, 1024, 257, 48, 65536, 12288};
    const int Ks[] = {4096, 14336, 1024, 2048, 512, 576, 5120, 8192, 1536, 100};
    const unsigned copies[] = {0, VZ_ROUTE_WT, VZ_ROUTE_W8, VZ_ROUTE_W8 | VZ_ROUTE_W8T, VZ_ROUTE_W8 | VZ_ROUTE_W8T | VZ_ROUTE_WT, VZ_ROUTE_W8 | VZ_ROUTE_WT};
    const int hidden = 4096;
    long n_engine = 0, n_op = 0, bad = 0;
    for (int k9 = 0; k9 < 8; ++k9) for (int k14 : {29, 17, 65, 40, 8, 1}) for (int k19 : {1, 0}) {
        if (!set_knobs(k9, k14, k19)) return 1;
        for (int N : Ns) for (int K : Ks) for (int act : {0, 1, 3}) for (int M = 1; M <= 700; M += (M < 70 ? 1 : 61)) for (int norm : {0, 1}) {
            if (act == VZ_ACT_SWIGLU && (N & 31)) continue;
            const unsigned base = (norm ? VZ_ROUTE_NORM : VZ_ROUTE_RESIDUAL) | (act != VZ_ACT_SWIGLU && N % 3 == 0 ? VZ_ROUTE_BIAS : 0);
            // engine callers: the plan against what linear() launched (route, copy read, stand-alone norm, split-K hint, profile class)
            for (int decode : {0, 1}) for (unsigned cp : copies) for (int sk : {0, 3}) {
                const unsigned fl = base | cp | (decode ? VZ_ROUTE_DECODE : 0);
                const Old want = old_route(VZ_LINEAR_ENGINE, fl, M, N, K, K, K, act, 0, hidden, sk);
                LinearArgs a = mk(M, N, K, K, K, act, 0, fl);
                a.splitk_hint = sk;
                if (cp & VZ_ROUTE_WT) a.Wt = (const bf16_t*)some;
                if (cp & VZ_ROUTE_W8) { a.W8 = (const unsigned char*)some; a.wscale = some; }
                if (cp & VZ_ROUTE_W8T) a.W8t = (const unsigned char*)some;
                LinPlan p = vz_plan_linear(a, LinCaller{decode ? LIN_ROWS_DECODE : LIN_ROWS_COUPLED, hidden});
                if (vz_linear_check_common(a) != VZ_OK || !vz_route_takes(p, a)) p.route = LIN_NONE;
                ++n_engine;
                bool same = p.route == want.route;
                if (same && p.route != LIN_NONE) {
                    same = p.pre_norm == (want.pre_norm != 0) && p.klass == want.klass && (p.route != LIN_TILE128 || p.splitk_hint == want.splitk);
                    const bool reads_copy = p.route >= LIN_SKINNY && p.route <= LIN_WIDE_E4M3;       // the GEMV and the tile GEMMs read row-major weights only
                    same = same && (reads_copy ? p.weights == want.weights : (p.weights == LIN_W_E4M3) == (want.weights == LIN_W_E4M3));
                }
                if (!same && ++bad <= 20)
                    printf("DIFF engine k9=%d k14=%d k19=%d M=%d N=%d K=%d act=%d flags=%u hint=%d: old %s w%d pre%d sk%d class%d | plan %s w%d pre%d sk%d class%d\n", k9, k14, k19, M, N, K,
                           act, fl, sk, vz_route_name((LinRoute)want.route), want.weights, want.pre_norm, want.splitk, want.klass, vz_route_name(p.route), p.weights, p.pre_norm, p.splitk_hint, p.klass);
            }
            // op-level entry points: the route query against what the entry point launched
            if (k14 != 29) continue;
            for (int entry : {VZ_LINEAR_OP, VZ_LINEAR_RMSNORM, VZ_LINEAR_TILED, VZ_LINEAR_TILED_FP8, VZ_LINEAR_IMPL, VZ_LINEAR_IMPL + 1, VZ_LINEAR_IMPL + 2, VZ_LINEAR_IMPL + 3, VZ_LINEAR_IMPL + 4})
            for (int w8 : {0, 1}) {
                if (w8 && entry != VZ_LINEAR_OP) continue;
                if (norm && entry >= VZ_LINEAR_TILED_FP8) continue;          // these entry points take no norm
                const unsigned fl = base | VZ_ROUTE_RESIDUAL | (w8 ? VZ_ROUTE_W8 : 0) | (entry == VZ_LINEAR_TILED ? VZ_ROUTE_WT : 0) | (entry == VZ_LINEAR_TILED_FP8 ? VZ_ROUTE_W8T : 0);
                if (entry == VZ_LINEAR_RMSNORM && (fl & VZ_ROUTE_BIAS)) continue;
                const int want = old_route(entry, fl, M, N, K, K, K, act, 0, hidden, 0).route;
                const int got = vz_op_linear_route(M, N, K, K, K, act, 0, fl, entry, nullptr, nullptr);
                ++n_op;
                if (got != want && ++bad <= 20)
                    printf("DIFF op entry=%d k9=%d k19=%d M=%d N=%d K=%d act=%d flags=%u: old %s | query %s\n", entry, k9, k19, M, N, K, act, fl, vz_route_name((LinRoute)want), vz_route_name((LinRoute)got));
            }
        }
    }
    printf("%ld engine cases, %ld op-level cases, %ld differ\n", n_engine, n_op, bad);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "grid")) return grid();
    if (argc == 2 && !strcmp(argv[1], "table")) return table();
    fprintf(stderr, "usage: route_oracle grid | table\n");
    return 2;
}
