// Which kernel runs a linear C = epi(A . W^T): vz_plan_linear() chooses once, vz_run_linear() launches what the plan says.
// The planner (linear_route.hip) is host-only and pure: a function of the arguments, the caller and the tune knobs.  What a kernel can
// take stays with the kernel (vz_gemv_ok, vz_skinny_ok, vz_wide_ok, vz_wide_splits, vz_gemm_use256); which of the eligible ones is
// taken - the measured cross-overs - is written down in vz_plan_linear and nowhere else.
#pragma once
#include "vz_common.h"

// one value per kernel family a launch can end in
enum LinRoute {
    LIN_NONE = -1,              // no admitted kernel takes the arguments: vz_run_linear returns VZ_ERR_ARG
    LIN_GEMV = 0,               // gemv.hip: 1..8 rows in LDS, fused RMSNorm, bf16 or e4m3 rows
    LIN_SKINNY = 1,             // gemm_skinny.hip: 2..16 rows, one 16-row weight group per workgroup
    LIN_SKINNY_PERSIST = 2,     // gemm_skinny.hip: the persistent form, one workgroup per CU, RMSNorm fused
    LIN_SKINNY_WIDE = 3,        // gemm_skinny.hip: 17..64 rows, two / four B operands per weight fragment
    LIN_WIDE_BF16 = 4,          // gemm_wide.hip on the tiled bf16 copy
    LIN_WIDE_E4M3 = 5,          // gemm_wide.hip on the tiled e4m3 copy
    LIN_TILE128 = 6,            // gemm.hip: 128^2 tiles, with or without split-K
    LIN_TILE256 = 7,            // gemm256.hip: the 256^2 pipeline
};
const char* vz_route_name(LinRoute r);
constexpr unsigned lin_bit(LinRoute r) { return 1u << r; }

// the representation of W the kernel reads
enum LinWeights { LIN_W_BF16, LIN_W_BF16_TILED, LIN_W_E4M3, LIN_W_E4M3_TILED };

// the values of knob 9 (VZ_KNOB_SKINNY_MODE)
enum SkinnyMode {
    SKINNY_OFF = 0,              // no MFMA weight stream: GEMV up to 8 rows, tile GEMMs beyond (the routes before gemm_skinny.hip)
    SKINNY_ON = 1,               // default: 2..64 independent rows stream the weights through MFMAs; persistent fused-norm form from 3 rows
    SKINNY_NO_PERSIST = 2,       // never the persistent form: the one-group-per-workgroup kernel, above 4 rows behind a stand-alone RMSNorm
    SKINNY_PERSIST_FROM_2 = 3,   // the persistent form takes 2-row launches as well
    SKINNY_PERSIST_2_PER_CU = 4, // the persistent form with two workgroups per CU where LDS holds them (A/B)
    SKINNY_IGNORE_TILED = 5,     // the weight stream reads the row-major weights although a tiled copy exists (A/B)
    SKINNY_MODE_6 = 6,           // no reader: behaves as SKINNY_ON
    SKINNY_2_ROWS = 7,           // 2-row linears take the weight stream too (default: the GEMV with both rows in LDS)
};

// what the rows of A are to the caller
enum LinRows {
    LIN_ROWS_COUPLED,   // prefill, CLIP, Q-Former, trainer: a row's result must not depend on how many rows sit beside it (the tile GEMM's
                        // split-K is a function of N and K only; tests/test_stages_gpu.py::test_qformer) - above 16 rows only tile GEMMs
    LIN_ROWS_FREE,      // op-level entry points: independent rows, kernels by eligibility alone (weight streams up to 64 rows)
    LIN_ROWS_DECODE,    // an engine's decode step: independent sequences, and the measured 17..64-row cascade on the copies finalize attached
};
struct LinCaller {
    LinRows rows;
    int xnorm_cols = 0;         // columns of the RMSNorm scratch the caller hands to vz_run_linear (0 = none: the norm can only run fused)
    unsigned allow = ~0u;       // lin_bit(r) set: the caller admits route r (op-level entry points name the kernels they exist for)
};

struct LinPlan {
    LinRoute route;
    LinWeights weights;
    bool pre_norm;              // the RMSNorm runs as its own launch into the caller's scratch, the linear reads that scratch
    int splitk_hint;            // LinearArgs::splitk_hint of the launch: vz_decode_splitk on the decode tile route, else the caller's own
    int klass;                  // profile class of the launch: K_GEMV (weight-streaming, decode) or K_GEMM
    bool rows_free;             // LinCaller::rows != LIN_ROWS_COUPLED, for the launchers' own checks
};

LinPlan vz_plan_linear(const LinearArgs& a, LinCaller c);
// the plan of a caller that names its kernel family (vz_op_linear_impl): any of the gemm_skinny.hip routes stands for the one
// vz_skinny_route picks; decode_splitk = the TILE128 plan of a decode step.  Eligibility is the launcher's own check (vz_route_takes).
LinPlan vz_plan_forced(LinRoute family, const LinearArgs& a, bool decode_splitk);
bool vz_route_takes(const LinPlan& p, const LinearArgs& a);
// launches exactly what the plan says: vz_run_prenorm (if p.pre_norm) then vz_run_route.  Callers that bracket the two launches
// separately (the engine's profile scopes) call the halves themselves.
int vz_run_linear(const LinPlan& p, const LinearArgs& a, bf16_t* xnorm, hipStream_t s);
int vz_run_prenorm(const LinearArgs& a, bf16_t* xnorm, hipStream_t s);
int vz_run_route(const LinPlan& p, const LinearArgs& a, const bf16_t* xnorm, hipStream_t s);

// gemm_skinny.hip: which of its three forms takes these arguments (the launcher and the planner both ask here)
LinRoute vz_skinny_route(const LinearArgs& a);
