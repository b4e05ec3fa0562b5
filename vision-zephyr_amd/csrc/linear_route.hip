// The route plan of every linear (linear_route.h): one cascade of row-count ranges, then the launch of what it chose.  Host code only.
#include <algorithm>

#include "linear_route.h"

const char* vz_route_name(LinRoute r) {
    static const char* const names[] = {"GEMV", "SKINNY", "SKINNY_PERSIST", "SKINNY_WIDE", "WIDE_BF16", "WIDE_E4M3", "TILE128", "TILE256"};
    return r >= LIN_GEMV && r <= LIN_TILE256 ? names[r] : "NONE";
}

static int vz_decode_splitk(int N, int K, int act) {
    // In situ (rocprofv3 of a 64-row step, profiles/r02_rows.txt) the 128^2 kernel is bound by the bytes its workgroups keep in flight
    // (32 KiB each): gate|up with 224 workgroups ran at 3.3 TB/s, down with 512 (split 16) at 4.4.  So every projection is cut along K
    // until ~2 workgroups per CU are streaming: gate|up x2 (the SwiGLU pairs are formed by the finalize kernel), QKV / O x8, down x16.
    if (N & 7) return 0;
    const int tiles_n = (N + 127) / 128;
    if (act == VZ_ACT_SWIGLU) return tiles_n < 384 ? 2 : 0;
    if (K < 8192) return vz_knob(VZ_KNOB_DECODE_SK_SHORT);
    int sk = (512 + tiles_n - 1) / tiles_n;
    if (sk > 16) sk = 16;
    return sk < 1 ? 1 : sk;
}

// the arguments a launcher sees: only the weight copy the plan reads, the norm gone (and A = the scratch) where it runs as its own launch
static LinearArgs as_launched(const LinearArgs& a, const LinPlan& p, const bf16_t* xnorm) {
    LinearArgs t = a;
    if (p.weights != LIN_W_E4M3) t.W8 = nullptr;
    if (p.weights != LIN_W_BF16_TILED) t.Wt = nullptr;
    if (p.weights != LIN_W_E4M3_TILED) t.W8t = nullptr;
    if (p.weights == LIN_W_BF16 || p.weights == LIN_W_BF16_TILED) t.wscale = nullptr;
    t.rows_free = p.rows_free; t.splitk_hint = p.splitk_hint;
    if (p.pre_norm) { t.A = xnorm; t.lda = a.K; t.norm_w = nullptr; }
    return t;
}

static bool is_skinny(LinRoute r) { return r == LIN_SKINNY || r == LIN_SKINNY_PERSIST || r == LIN_SKINNY_WIDE; }

bool vz_route_takes(const LinPlan& p, const LinearArgs& a) {
    const LinearArgs t = as_launched(a, p, a.A);
    if (p.route == LIN_GEMV) return vz_gemv_ok(t);
    if (is_skinny(p.route)) return vz_skinny_ok(t);
    if (p.route == LIN_WIDE_BF16 || p.route == LIN_WIDE_E4M3) return vz_wide_ok(t);
    return p.route != LIN_NONE && !t.norm_w;       // the tile GEMMs have no norm prologue
}

LinPlan vz_plan_forced(LinRoute family, const LinearArgs& a, bool decode_splitk) {
    LinPlan p{family, a.W8t ? LIN_W_E4M3_TILED : a.W8 ? LIN_W_E4M3 : a.Wt ? LIN_W_BF16_TILED : LIN_W_BF16, false,
              decode_splitk ? vz_decode_splitk(a.N, a.K, a.act) : a.splitk_hint, family >= LIN_TILE128 && !decode_splitk ? K_GEMM : K_GEMV, true};
    if (is_skinny(family)) p.route = vz_skinny_route(as_launched(a, p, a.A));
    return p;
}

LinPlan vz_plan_linear(const LinearArgs& a, LinCaller c) {
    const bool decode = c.rows == LIN_ROWS_DECODE, rows_free = c.rows != LIN_ROWS_COUPLED;
    // the norm CAN run as its own launch into the caller's scratch: a decode step's scratch is taken to hold its normed linears' K
    // columns (they all have K = hidden); below 17 rows the stand-alone norm is only tried where the columns are known to match
    const bool pre = a.norm_w && (c.rows == LIN_ROWS_DECODE ? c.xnorm_cols > 0 : c.xnorm_cols == a.K);
    const bool pre_k = a.norm_w && c.xnorm_cols == a.K;
    const bool stream = vz_knob(VZ_KNOB_SKINNY_MODE) != SKINNY_OFF;
    auto plan = [&](LinRoute r, LinWeights w, bool pre_norm, int splitk, int klass) { return LinPlan{r, w, pre_norm, splitk, klass, rows_free}; };
    auto probe = [&](LinWeights w, bool pre_norm) { return as_launched(a, plan(LIN_NONE, w, pre_norm, a.splitk_hint, K_GEMV), a.A); };
    auto allowed = [&](LinRoute r) { return (c.allow & lin_bit(r)) != 0; };
    const LinPlan none = plan(LIN_NONE, LIN_W_BF16, false, a.splitk_hint, K_GEMV);

    // ---- which copies of W this caller may read ----
    // The tiled copies belong to independent rows on dense [N, K] weights: a decode step reads what finalize attached, an op-level caller
    // what it passed.  Prefill keeps the row-major tensor even at 2..16 rows.
    const bool tiled = rows_free && a.ldw == a.K;
    const bool has_wt = tiled && a.Wt, has_w8t = tiled && a.W8t && a.wscale;
    // The row-major e4m3 copy holds the same values as the bf16 tensor; only the weight-stream kernels (GEMV, MFMA stream: M <= 64) read
    // it.  Above 16 rows those run behind a stand-alone norm, so the probe drops it.  An engine falls back to its bf16 tensor; an
    // op-level caller passed the e4m3 rows alone.
    const bool e4m3 = a.W8 && a.wscale;
    bool use8 = e4m3;
    if (e4m3 && c.rows != LIN_ROWS_FREE) {
        LinearArgs t = probe(LIN_W_E4M3, false);
        if (a.M > 16) t.norm_w = nullptr;
        use8 = vz_gemv_ok(t) || (stream && vz_skinny_ok(t));
    }
    // what a GEMV / MFMA-stream launch reads (knob 9 = 5: the row-major weights although a tiled copy exists, A/B)
    const LinWeights ws = use8 ? LIN_W_E4M3 : has_wt && (a.N & 15) == 0 && vz_knob(VZ_KNOB_SKINNY_MODE) != SKINNY_IGNORE_TILED ? LIN_W_BF16_TILED : LIN_W_BF16;

    // e4m3 engines leave the e4m3 streams for the bf16 tile route where the row-major e4m3 stream stops being ahead (32 rows); bf16
    // engines at the measured cross-over of knob 14
    const int tile_rows = e4m3 ? std::max(vz_knob(VZ_KNOB_DECODE_TILE_ROWS), 33) : vz_knob(VZ_KNOB_DECODE_TILE_ROWS);

    // ---- 17..64 independent rows: the tiled streams of gemm_wide.hip ----
    if (rows_free && a.M >= 17 && a.M <= 64) {
        // 17..64-row step of an e4m3-weight engine: every projection streams the e4m3 fragment-tiled copy (gemm_wide.hip, round 3) -
        // half the bytes of the bf16 routes these row counts took before (the row-major e4m3 stream of gemm_skinny.hip was slower than
        // bf16 at 17..32 rows and unused beyond).  The RMSNorm runs as its own launch.
        if (has_w8t && allowed(LIN_WIDE_E4M3) && vz_wide_ok(probe(LIN_W_E4M3_TILED, pre)))
            return plan(LIN_WIDE_E4M3, LIN_W_E4M3_TILED, pre, a.splitk_hint, K_GEMV);
        // 17..64 rows on the tiled bf16 copy (gemm_wide.hip): weights straight to registers, the activations of a 512-k chunk staged once
        // per 128 weight rows.  A decode step takes it for the projections whose row blocks fill the chip without a K split (gate|up,
        // lm_head: measured 52.7 vs 62 us and 55 vs 91 us at 64 rows; the split shapes - down P = 7: 38.5 vs 28.9 + 6.2 us, O: 22.9 vs
        // 14.2 + 6.2, QKV: 22.2 vs 17.0 + 4.9 - stay on the tile GEMM).  The RMSNorm runs as its own launch.  (A weight_fp8 engine's bf16
        // tensors - and their tiled copies - hold the same dequantised values.)
        if (has_wt && allowed(LIN_WIDE_BF16) && (!e4m3 || a.M >= tile_rows)) {
            const LinearArgs t = probe(LIN_W_BF16_TILED, pre);
            if (vz_wide_ok(t) && (!decode || vz_wide_splits(t) == 1)) return plan(LIN_WIDE_BF16, LIN_W_BF16_TILED, pre, a.splitk_hint, K_GEMV);
        }
    }

    // ---- a decode step from knob 14's row count on (29; any value, also below 17), up to 64 rows ----
    // Decode step as a TILE GEMM: the 128^2 MFMA kernel streams every weight once at the rate its workgroups can pull (gate-up 48 us =
    // 4.9 TB/s whatever the row count), where the MFMA weight stream of gemm_skinny.hip re-reads the activations per 16-row group and
    // falls to 2.7 TB/s at 64 rows (tools/bench_rows.py, profiles/r02_rows.txt).  Projections with few column tiles (QKV 48, O / down
    // 32) are cut along K until ~512 workgroups are in flight (vz_decode_splitk).  The RMSNorm runs as its own launch.
    if (decode && a.M >= tile_rows && a.M <= 64 && stream && (a.K & 63) == 0 && (!a.norm_w || pre) && allowed(LIN_TILE128))
        return plan(LIN_TILE128, LIN_W_BF16, pre, vz_decode_splitk(a.N, a.K, a.act), K_GEMV);

    // ---- 5..64 rows whose norm cannot ride in the kernel ----
    // Without the persistent fused-norm kernel (knob 9 = 2, a K it does not take, more than 16 rows): normalise once into an L2-resident
    // scratch and let the MFMA weight stream take its B fragments from there.
    const LinearArgs a0 = probe(ws, false);
    if (pre_k && a.M > 4 && a.M <= 64 && stream && !(vz_skinny_ok(a0) && vz_skinny_fused_norm_ok(a0))) {
        const LinearArgs t = probe(ws, true);
        if (vz_skinny_ok(t) && allowed(vz_skinny_route(t))) return plan(vz_skinny_route(t), ws, true, a.splitk_hint, K_GEMV);
    }

    // ---- every row count: the kernels by eligibility ----
    // 2 rows: the GEMV with both rows in LDS streams the weights like the 1-row launch (3.12 vs 3.48 ms per 2-row step; knob 9 = 7: the
    // MFMA stream); 3..64 independent rows: one MFMA per KiB of weights.  Both fuse the norm.
    const bool gemv = vz_gemv_ok(a0) && allowed(LIN_GEMV);
    if (stream && vz_skinny_ok(a0) && allowed(vz_skinny_route(a0)) && !(a.M == 2 && vz_knob(VZ_KNOB_SKINNY_MODE) != SKINNY_2_ROWS && gemv))
        return plan(vz_skinny_route(a0), ws, false, a.splitk_hint, K_GEMV);
    if (gemv) return plan(LIN_GEMV, use8 ? LIN_W_E4M3 : LIN_W_BF16, false, a.splitk_hint, K_GEMV);
    if (use8) return none;                                     // e4m3 rows and no weight-stream kernel for them
    const LinRoute tile = vz_gemm_use256(a0) ? LIN_TILE256 : LIN_TILE128;
    if (!allowed(tile)) return none;
    return plan(tile, LIN_W_BF16, false, a.splitk_hint, a.norm_w ? K_GEMV : K_GEMM);
}

int vz_run_prenorm(const LinearArgs& a, bf16_t* xnorm, hipStream_t s) {
    return vz_launch_rmsnorm(a.A, a.lda, xnorm, a.K, a.norm_w, a.M, a.K, a.norm_eps, s);
}

int vz_run_route(const LinPlan& p, const LinearArgs& a, const bf16_t* xnorm, hipStream_t s) {
    const LinearArgs t = as_launched(a, p, xnorm);
    switch (p.route) {
    case LIN_GEMV: return vz_launch_gemv(t, s);
    case LIN_SKINNY: case LIN_SKINNY_PERSIST: case LIN_SKINNY_WIDE: return vz_launch_skinny(t, s);
    case LIN_WIDE_BF16: case LIN_WIDE_E4M3: return vz_launch_wide(t, s);
    case LIN_TILE128: return vz_launch_gemm128(t, s);
    case LIN_TILE256: return vz_launch_gemm256(t, s);
    case LIN_NONE: break;
    }
    VZ_CHECK_ARG(!a.W8, "linear: e4m3 weights are streamed by the M <= 16 kernels only (M=%d K=%d)", a.M, a.K);
    vz_set_error("linear: no admitted kernel takes M=%d N=%d K=%d", a.M, a.N, a.K);
    return VZ_ERR_ARG;
}

int vz_run_linear(const LinPlan& p, const LinearArgs& a, bf16_t* xnorm, hipStream_t s) {
    if (p.pre_norm) { int r = vz_run_prenorm(a, xnorm, s); if (r) return r; }
    return vz_run_route(p, a, xnorm, s);
}
