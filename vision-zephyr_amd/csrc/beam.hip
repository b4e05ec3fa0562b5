// Beam search on the device (hf:generation/utils.py `_beam_search`, do_sample=False; DESIGN.md "Beam search"):
//
// 1. beam_row_topk_kernel - one 1024-thread workgroup per beam row of fp32 logits [groups * nb_in, V]:
//      s_i = ((x_i - max) - log(sum_j exp(x_j - max))) + score[row]        (HF: log_softmax(logits) + running_beam_scores)
//    the max and the sum are reduced in a fixed order (same bits in a graph replay, an eager step and a second run); then the
//    exact top K of s by a 4-pass radix select on the order-preserving key (as sample_kernel's top-k), the candidates strictly
//    above the K-th key plus, of those equal to it, the smallest token indices; sorted, written to a per-row scratch list.
// 2. beam_merge_kernel - one workgroup per group (= prompt): the nb_in sorted lists merged into the group's sorted top K
//    (rank of a candidate = its place in its own list + a binary search in every other list).  TIES: equal scores go to the
//    smaller flat index beam * V + token (torch.topk leaves their order unspecified; vz_hip/beam.py follows the same rule).
//    The K candidates {score, token, parent beam} are appended to the history record hist[hidx][group] (hidx = a device word);
//    the next running beams are the first nb_out candidates whose token is not an eos id: their token, score and parent beam
//    are written per row, and as the decode step's tail the row's output id / position / cache slot / length advance exactly as
//    argmax_kernel advances them.
// 3. kv_beam_reorder_kernel - after the tail, cache positions [base, slot) of every beam row whose parent is another row become
//    those of its parent (every layer, K and V).  A workgroup takes one (group, layer, K|V, KV head, 8-position chunk) piece,
//    stages the chunk of every row that is some changed row's parent in LDS, then writes the changed rows: cycles and parents
//    with several children are safe, the copy is bit-exact, and a group whose parents are all the identity costs nothing.
//    The piece count follows the device-side slot, so a replayed graph copies only the positions generated so far.
#include "vz_common.h"

namespace {

constexpr int BEAM_KMAX = 128;          // K = max(2, 1 + n_eos) * nb <= 5 * 16 = 80
constexpr int REORDER_CH = 8;           // positions per reorder piece (16 rows x 8 positions x 128 x 2 B = 32 KiB of LDS)

__device__ __forceinline__ unsigned bkey(float x) {          // ascending-order-preserving key of a float
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct RowShared {
    unsigned hist[256];
    float redf[16];
    unsigned wcnt[16];
    unsigned sel, carry, n_above;
    unsigned ckey[BEAM_KMAX];
    float cs[BEAM_KMAX];
    int ci[BEAM_KMAX];
};

#define BEAM_FOR_ROW(BODY)                                                                                            \
    if (REG) {                                                                                                        \
        _Pragma("unroll 8") for (int k = tid; k < cols; k += 1024) { const float x = lx[k]; BODY }                     \
    } else {                                                                                                          \
        for (int k = tid; k < cols; k += 1024) { const float x = lr[k]; BODY }                                        \
    }

// MODE: BEAM_FUSED = select on logits (the parent's step); BEAM_ON_ROWS = select on rows that are log-probs already (s_i = lp_i +
// score[row], no reduction); BEAM_LOGPROB = write the log-prob rows lp_i = (x_i - max) - log(sum) to lp_out (may be `logits`: every
// element is read and written by the same thread, behind the reductions) and select nothing.
enum { BEAM_FUSED = 0, BEAM_ON_ROWS = 1, BEAM_LOGPROB = 2 };

template <bool REG, int MODE>
__global__ __launch_bounds__(1024) void beam_row_topk_kernel(const float* logits, int cols, int K,
                                                             const float* __restrict__ scores_in, float* __restrict__ cand_s,
                                                             int* __restrict__ cand_t, float* lp_out) {
    __shared__ RowShared sh;
    extern __shared__ float lx[];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* lr = logits + (size_t)row * cols;
    if (REG) {
        for (int k = tid; k < cols; k += 1024) lx[k] = lr[k];
        __syncthreads();
    }
    const float bs = scores_in ? scores_in[row] : 0.f;

    // ---- max and sum of exp, fixed reduction order ----
    float m = 0.f, lse = 0.f;
    if (MODE != BEAM_ON_ROWS) {
        m = -INFINITY;
        BEAM_FOR_ROW({ m = fmaxf(m, x); })
        m = wave_max(m);
        if (lane == 0) sh.redf[wv] = m;
        __syncthreads();
        m = sh.redf[0];
        for (int w = 1; w < 16; ++w) m = fmaxf(m, sh.redf[w]);
        __syncthreads();
        float z = 0.f;
        BEAM_FOR_ROW({ z += expf(x - m); })
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
        if (lane == 0) sh.redf[wv] = z;
        __syncthreads();
        z = 0.f;
        for (int w = 0; w < 16; ++w) z += sh.redf[w];
        lse = logf(z);
        __syncthreads();
    }
    if (MODE == BEAM_LOGPROB) {
        float* out = lp_out + (size_t)row * cols;
        BEAM_FOR_ROW({ out[k] = (x - m) - lse; })
        return;
    }
#define BEAM_S(x) (MODE == BEAM_ON_ROWS ? (x) + bs : ((x) - m) - lse + bs)

    // ---- key of the K-th largest s: 4-pass radix select ----
    unsigned prefix = 0, pmask = 0, want = (unsigned)K;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) sh.hist[tid] = 0;
        __syncthreads();
        BEAM_FOR_ROW({
            const unsigned key = bkey(BEAM_S(x));
            if ((key & pmask) == prefix) atomicAdd(&sh.hist[(key >> shift) & 255], 1u);
        })
        __syncthreads();
        if (tid == 0) {
            unsigned cum = 0;
            int b = 255;
            for (; b > 0; --b) { if (cum + sh.hist[b] >= want) break; cum += sh.hist[b]; }
            sh.sel = (unsigned)b; sh.carry = want - cum;
        }
        __syncthreads();
        prefix |= sh.sel << shift; pmask |= 255u << shift; want = sh.carry;
        __syncthreads();
    }
    const unsigned kth = prefix;          // `want` candidates with key == kth complete the K

    // ---- the candidates above the K-th key (any order; sorted below) ----
    if (tid == 0) sh.n_above = 0;
    __syncthreads();
    BEAM_FOR_ROW({
        const float sv = BEAM_S(x);
        const unsigned key = bkey(sv);
        if (key > kth) { const unsigned p = atomicAdd(&sh.n_above, 1u); if (p < BEAM_KMAX) { sh.cs[p] = sv; sh.ckey[p] = key; sh.ci[p] = k; } }
    })
    __syncthreads();
    // ---- of the candidates equal to it, the `want` smallest token indices: an ordered scan, 1024 indices at a time ----
    const unsigned above = sh.n_above;
    unsigned taken = 0;
    for (int k0 = 0; k0 < cols && taken < want; k0 += 1024) {
        const int k = k0 + tid;
        float sv = 0.f;
        bool f = false;
        if (k < cols) { sv = BEAM_S(REG ? lx[k] : lr[k]); f = bkey(sv) == kth; }
        const unsigned long long bal = __ballot(f);
        if (lane == 0) sh.wcnt[wv] = (unsigned)__popcll(bal);
        __syncthreads();
        unsigned before = 0, total = 0;
        for (int w = 0; w < 16; ++w) { if (w < wv) before += sh.wcnt[w]; total += sh.wcnt[w]; }
        const unsigned r = taken + before + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
        if (f && r < want) { const unsigned p = above + r; if (p < BEAM_KMAX) { sh.cs[p] = sv; sh.ckey[p] = kth; sh.ci[p] = k; } }
        taken += total;
        __syncthreads();
    }
#undef BEAM_S
    // ---- sort the K: rank by (key descending, token ascending) ----
    if (tid < K) {
        const unsigned ka = sh.ckey[tid];
        const int ia = sh.ci[tid];
        int rank = 0;
        for (int j = 0; j < K; ++j) rank += (sh.ckey[j] > ka) || (sh.ckey[j] == ka && sh.ci[j] < ia);
        cand_s[(size_t)row * K + rank] = sh.cs[tid];
        cand_t[(size_t)row * K + rank] = ia;
    }
}

// number of entries of a sorted (descending) list better than (key, flat) - entries of an earlier row win equal keys
__device__ __forceinline__ int count_better(const float* s, int K, unsigned key, bool ties_win) {
    int lo = 0, hi = K;                   // first index whose entry is NOT better
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const unsigned km = bkey(s[mid]);
        const bool better = ties_win ? km >= key : km > key;
        if (better) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void beam_merge_kernel(const float* __restrict__ cand_s, const int* __restrict__ cand_t, int cols,
                                                         int nb_in, int nb_out, int K, BeamEos eos, int groups,
                                                         int* __restrict__ hist, const int* __restrict__ hidx, int hist_cap,
                                                         int* __restrict__ next_tok, float* __restrict__ next_score,
                                                         int* __restrict__ next_parent, RowEmit emit) {
    __shared__ float ts[BEAM_KMAX];
    __shared__ int tt[BEAM_KMAX], tb[BEAM_KMAX];
    const int g = blockIdx.x, tid = threadIdx.x;
    const float* gs = cand_s + (size_t)g * nb_in * K;
    const int* gt = cand_t + (size_t)g * nb_in * K;
    for (int c = tid; c < nb_in * K; c += 256) {
        const int r = c / K, p = c % K;
        const unsigned key = bkey(gs[c]);
        int rank = p;
        for (int r2 = 0; r2 < nb_in && rank < K; ++r2)
            if (r2 != r) rank += count_better(gs + (size_t)r2 * K, K, key, r2 < r);
        if (rank < K) { ts[rank] = gs[c]; tt[rank] = gt[c]; tb[rank] = r; }
    }
    __syncthreads();
    const int h = hidx ? *hidx : 0;
    if (hist && h < hist_cap) {
        int* rec = hist + ((size_t)h * groups + g) * K * 3;
        for (int i = tid; i < K; i += 256) { rec[3 * i] = __float_as_int(ts[i]); rec[3 * i + 1] = tt[i]; rec[3 * i + 2] = tb[i]; }
    }
    if (tid == 0) {
        int j = 0;
        for (int i = 0; i < K && j < nb_out; ++i) {
            bool is_eos = false;
            for (int q = 0; q < eos.n; ++q) is_eos |= tt[i] == eos.id[q];
            if (is_eos) continue;
            const int row = g * nb_out + j++;
            next_tok[row] = tt[i];
            if (next_score) next_score[row] = ts[i];
            if (next_parent) next_parent[row] = tb[i];
            vz_emit_advance(emit, row, tt[i], 0u);          // (the beam tail runs without a token ring)
        }
    }
}

__global__ void beam_advance_kernel(int* hidx) { hidx[0] += 1; }

// The processors' id histories (logits_proc.hip: lens[row], ids[row][stride]) follow the beams: the history of every row whose parent
// is another row becomes its parent's, length included.  One workgroup per group; like the KV reorder it stages the piece of every
// row that is some changed row's parent in LDS before it writes the changed rows, HIST_CH ids at a time, so cycles and parents with
// several children are safe; the lengths are read before anything is written and written last.
constexpr int HIST_CH = 512;            // 16 rows x 512 ids x 4 B = 32 KiB of LDS

__global__ __launch_bounds__(1024) void hist_beam_reorder_kernel(int* __restrict__ lens, int* __restrict__ ids, int stride, int nb,
                                                                 const int* __restrict__ parent) {
    __shared__ int stage[16 * HIST_CH];
    __shared__ int par[16], slot_of[16], srcs[16], dsts[16], len0[16];
    __shared__ int n_src, n_dst, n_max;
    const int tid = threadIdx.x, r0 = blockIdx.x * nb;
    if (tid == 0) {
        int ns = 0, nd = 0, mx = 0;
        for (int j = 0; j < nb; ++j) {
            const int p = parent[r0 + j];
            par[j] = (p >= 0 && p < nb) ? p : j; slot_of[j] = -1; len0[j] = min(max(lens[r0 + j], 0), stride);
        }
        for (int j = 0; j < nb; ++j)
            if (par[j] != j) {
                dsts[nd++] = j;
                if (slot_of[par[j]] < 0) { slot_of[par[j]] = ns; srcs[ns++] = par[j]; mx = max(mx, len0[par[j]]); }
            }
        n_src = ns; n_dst = nd; n_max = mx;
    }
    __syncthreads();
    const int ns = n_src, nd = n_dst, nm = n_max;
    if (nd == 0) return;
    for (int p0 = 0; p0 < nm; p0 += HIST_CH) {
        const int np = min(HIST_CH, nm - p0);
        for (int i = tid; i < ns * np; i += 1024) {
            const int q = i / np, v = i % np;
            stage[q * HIST_CH + v] = ids[(size_t)(r0 + srcs[q]) * stride + p0 + v];
        }
        __syncthreads();
        for (int i = tid; i < nd * np; i += 1024) {
            const int d = i / np, v = i % np;
            const int j = dsts[d];
            if (p0 + v < len0[par[j]]) ids[(size_t)(r0 + j) * stride + p0 + v] = stage[slot_of[par[j]] * HIST_CH + v];
        }
        __syncthreads();
    }
    if (tid < nd) lens[r0 + dsts[tid]] = len0[par[dsts[tid]]];
}

__global__ __launch_bounds__(256) void kv_beam_reorder_kernel(bf16_t* __restrict__ kv, size_t layer_elems, int n_layers, int max_batch,
                                                              int Hkv, int max_ctx, int D, int nb, int groups, const int* __restrict__ parent,
                                                              const int* __restrict__ base, int base_stride, const int* __restrict__ end,
                                                              int end_stride) {
    __shared__ uint4 stage[16 * REORDER_CH * 128 / 8];
    __shared__ int par[16], slot_of[16], srcs[16], dsts[16];
    __shared__ int n_src, n_dst;
    const int tid = threadIdx.x;
    const int vec = D / 8;                                     // 16-byte vectors per position
    const size_t row_elems = (size_t)Hkv * max_ctx * D;
    const int per_pos_piece = n_layers * 2 * Hkv;
    long off = 0;                                             // first piece index of group g
    for (int g = 0; g < groups; ++g) {
        const int r0 = g * nb;
        const int P = base[(size_t)g * base_stride], E = min(end[(size_t)g * end_stride], max_ctx);
        const int nch = E > P && P >= 0 ? (E - P + REORDER_CH - 1) / REORDER_CH : 0;
        const long pieces = (long)per_pos_piece * nch;
        if (pieces == 0) continue;
        __syncthreads();
        if (tid == 0) {
            int ns = 0, nd = 0;
            for (int j = 0; j < nb; ++j) { const int p = parent[r0 + j]; par[j] = (p >= 0 && p < nb) ? p : j; slot_of[j] = -1; }
            for (int j = 0; j < nb; ++j)
                if (par[j] != j) {
                    dsts[nd++] = j;
                    if (slot_of[par[j]] < 0) { slot_of[par[j]] = ns; srcs[ns++] = par[j]; }
                }
            n_src = ns; n_dst = nd;
        }
        __syncthreads();
        if (n_dst == 0) { off += pieces; continue; }
        const int ns = n_src, nd = n_dst;
        long first = ((long)blockIdx.x - off) % (long)gridDim.x;
        if (first < 0) first += gridDim.x;
        for (long pc = first; pc < pieces; pc += gridDim.x) {
            const int ch = (int)(pc / per_pos_piece), y = (int)(pc % per_pos_piece);
            const int head = y % Hkv, half = (y / Hkv) & 1, layer = y / (2 * Hkv);
            const int p0 = P + ch * REORDER_CH, np = min(REORDER_CH, E - p0);
            const bf16_t* hb = kv + (size_t)layer * layer_elems + (size_t)half * (layer_elems / 2) + (size_t)head * max_ctx * D + (size_t)p0 * D;
            const int nv = np * vec;                           // vectors of one row's chunk
            for (int i = tid; i < ns * nv; i += 256) {
                const int s = i / nv, v = i % nv;
                stage[s * REORDER_CH * 16 + v] = *(const uint4*)(hb + (size_t)(r0 + srcs[s]) * row_elems + (size_t)v * 8);
            }
            __syncthreads();
            for (int i = tid; i < nd * nv; i += 256) {
                const int d = i / nv, v = i % nv;
                const int j = dsts[d];
                *(uint4*)((bf16_t*)hb + (size_t)(r0 + j) * row_elems + (size_t)v * 8) = stage[slot_of[par[j]] * REORDER_CH * 16 + v];
            }
            __syncthreads();
        }
        off += pieces;
    }
}

}  // namespace

static bool g_beam_lds_ok = false;
static int init_beam_kernels() {
    static VzDeviceOnce once;
    if (!vz_device_first(once)) return VZ_OK;
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)beam_row_topk_kernel<true, BEAM_FUSED>, hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * (int)sizeof(float)));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)beam_row_topk_kernel<true, BEAM_ON_ROWS>, hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * (int)sizeof(float)));
    VZ_CHECK_HIP(hipFuncSetAttribute((const void*)beam_row_topk_kernel<true, BEAM_LOGPROB>, hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * (int)sizeof(float)));
    g_beam_lds_ok = true;
    return VZ_OK;
}

int vz_beam_k(int nb, int n_eos) { return (n_eos + 1 > 2 ? n_eos + 1 : 2) * nb; }

int vz_launch_beam_select(const float* logits, int rows, int cols, int nb_in, int nb_out, const BeamEos& eos, const float* scores_in,
                          float* cand_s, int* cand_t, int* hist, const int* hidx, int hist_cap, int* next_tok, float* next_score,
                          int* next_parent, const RowEmit& emit, bool on_rows, hipStream_t s) {
    const int K = vz_beam_k(nb_out, eos.n);
    VZ_CHECK_ARG(logits && cand_s && cand_t && next_tok && rows >= 1 && cols >= 1 && nb_in >= 1 && nb_in <= 16 && nb_out >= 1 &&
                 nb_out <= 16 && rows % nb_in == 0 && eos.n >= 0 && eos.n <= 4 && K <= BEAM_KMAX && !emit.ring,
                 "beam_select: bad argument (rows %d, nb_in %d, nb_out %d, %d eos ids)", rows, nb_in, nb_out, eos.n);
    VZ_CHECK_ARG(cols >= K, "beam_select: %d candidates per row exceed the vocabulary of %d", K, cols);
    { int r = init_beam_kernels(); if (r) return r; }
    const bool reg = cols <= 32768 && g_beam_lds_ok;
    const size_t lds = reg ? (size_t)cols * sizeof(float) : 0;
    float* const none = nullptr;
    if (on_rows) {          // the rows are log-probs already (vz_launch_beam_logprob_rows, then maybe the processors)
        if (reg) hipLaunchKernelGGL((beam_row_topk_kernel<true, BEAM_ON_ROWS>), dim3(rows), dim3(1024), lds, s, logits, cols, K, scores_in, cand_s, cand_t, none);
        else hipLaunchKernelGGL((beam_row_topk_kernel<false, BEAM_ON_ROWS>), dim3(rows), dim3(1024), lds, s, logits, cols, K, scores_in, cand_s, cand_t, none);
    } else {
        if (reg) hipLaunchKernelGGL((beam_row_topk_kernel<true, BEAM_FUSED>), dim3(rows), dim3(1024), lds, s, logits, cols, K, scores_in, cand_s, cand_t, none);
        else hipLaunchKernelGGL((beam_row_topk_kernel<false, BEAM_FUSED>), dim3(rows), dim3(1024), lds, s, logits, cols, K, scores_in, cand_s, cand_t, none);
    }
    VZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(beam_merge_kernel, dim3(rows / nb_in), dim3(256), 0, s, cand_s, cand_t, cols, nb_in, nb_out, K, eos, rows / nb_in,
                       hist, hidx, hist_cap, next_tok, next_score, next_parent, emit);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}

// lp[row][i] = (x_i - max) - log(sum_j exp(x_j - max)) with the reductions and the association of the fused select; lp may be `logits`
int vz_launch_beam_logprob_rows(const float* logits, int rows, int cols, float* lp, hipStream_t s) {
    VZ_CHECK_ARG(logits && lp && rows >= 1 && cols >= 1, "beam_logprob_rows: bad argument (rows %d, cols %d)", rows, cols);
    { int r = init_beam_kernels(); if (r) return r; }
    float* const nof = nullptr; int* const noi = nullptr;
    if (cols <= 32768 && g_beam_lds_ok)
        hipLaunchKernelGGL((beam_row_topk_kernel<true, BEAM_LOGPROB>), dim3(rows), dim3(1024), (size_t)cols * sizeof(float), s, logits, cols, 0, nof, nof, noi, lp);
    else
        hipLaunchKernelGGL((beam_row_topk_kernel<false, BEAM_LOGPROB>), dim3(rows), dim3(1024), 0, s, logits, cols, 0, nof, nof, noi, lp);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}

int vz_launch_hist_beam_reorder(int* lens, int* ids, int stride, int nb, int groups, const int* parent, hipStream_t s) {
    VZ_CHECK_ARG(lens && ids && parent && stride >= 1 && nb >= 1 && nb <= 16 && groups >= 1, "hist_beam_reorder: bad argument (nb %d, groups %d)", nb, groups);
    hipLaunchKernelGGL(hist_beam_reorder_kernel, dim3(groups), dim3(1024), 0, s, lens, ids, stride, nb, parent);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}

int vz_launch_beam_advance(int* hidx, hipStream_t s) {
    hipLaunchKernelGGL(beam_advance_kernel, dim3(1), dim3(1), 0, s, hidx);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}

int vz_launch_kv_beam_reorder(bf16_t* kv, size_t layer_elems, int n_layers, int max_batch, int Hkv, int max_ctx, int D, int nb, int groups,
                              const int* parent, const int* base, int base_stride, const int* end, int end_stride, hipStream_t s) {
    VZ_CHECK_ARG(kv && parent && base && end && nb >= 1 && nb <= 16 && groups >= 1 && groups * nb <= max_batch && D % 8 == 0 && D <= 128,
                 "kv_beam_reorder: bad argument (nb %d, groups %d, head_dim %d)", nb, groups, D);
    // a fixed grid (the piece count lives on the device): 2 workgroups per CU of a 256-CU part, or fewer for a small cache
    const long most = (long)n_layers * 2 * Hkv * ((max_ctx + REORDER_CH - 1) / REORDER_CH) * groups;
    const int grid = (int)std::min<long>(512, most);
    hipLaunchKernelGGL(kv_beam_reorder_kernel, dim3(grid), dim3(256), 0, s, kv, layer_elems, n_layers, max_batch, Hkv, max_ctx, D, nb, groups,
                       parent, base, base_stride, end, end_stride);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}
