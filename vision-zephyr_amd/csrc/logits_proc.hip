// HF's logits processors as one device-side filter between the lm_head and the step's tail:
//   hf:generation/logits_process.py RepetitionPenaltyLogitsProcessor -> NoRepeatNGramLogitsProcessor ->
//   MinNewTokensLengthLogitsProcessor(prompt_length_to_skip = 0) -> SuppressTokensLogitsProcessor, the order of
//   hf:generation/utils.py `_get_logits_processor`; the warpers (sampling.hip) come after them.
// The reference generates from inputs_embeds, so HF's processors see only the ids generated so far: the history h[0..n) of a row.
//   penalty : every DISTINCT token of h: x < 0 ? x * p : x / p       (HF gathers, then scatters: once per token)
//   n-gram g: ban h[i + g - 1] for every i with h[i .. i + g - 2] == h[n - g + 1 .. n); nothing while n < g; g = 1 bans all of h
//   min-new : while n < min_new every eos id is -inf
//   suppress: the listed ids are -inf
// The last three only write -inf and -inf * p = -inf, so ONE pass applies all four: two bitmaps of `cols` bits in LDS, `seen` (tokens of
// h) and `ban`; the history is marked with LDS atomics, then the bitmap WORDS are swept and only set bits touch a logit - penalty
// first, then -inf; a logit has exactly one writer, the rest of the row is neither read nor written.  Plain fp32 * and / (correctly
// rounded, no fast-math): bit-identical to torch on the CPU.
// In front of them, opt-in: HF's SequenceBiasLogitsProcessor (first in HF's chain) and NoBadWordsLogitsProcessor
// (behind the n-gram ban) from one table of id sequences in device memory, seq[k] = [len 1..8 | bad | bias (fp32 bits) | - | ids[8]]:
//   a one-id sequence acts at every step; a longer one acts on its last id when h ends in its first len - 1 ids - and, as HF's length
//   check has it, only once len <= n.  bad = 1 (a bad word): the id is banned, no arithmetic.  Else the id is marked in a third bitmap,
//   `biased`, and the sweep adds, in fp32 and in table order, the biases of the acting sequences that end in it: x + (((0 + b1) + b2) ...),
//   HF's zero-initialised bias row - then the penalty, which acts on the biased score, then -inf.  Still one writer per logit.
// One 1024-thread workgroup per row, in place.  Inside a decode step the kernel first appends cur[row] - the token the previous tail
// published - to the row's history (saturating at hist_stride), so no tail kernel has to know about the history.  base (optional): per
// row, how many ids of the history were seeded before generation began; min-new counts the ids behind them.
#include "vz_common.h"

namespace {

constexpr int PROC_MAX_COLS = 65536, PROC_WORDS = PROC_MAX_COLS / 32, PROC_G = 8;

__device__ __forceinline__ void mark(unsigned* bm, int tok, int cols) {
    if ((unsigned)tok < (unsigned)cols) atomicOr(&bm[tok >> 5], 1u << (tok & 31));
}

__global__ __launch_bounds__(1024) void logits_process_kernel(float* __restrict__ logits, int cols, int* __restrict__ hist, int hist_stride,
                                                              int* __restrict__ hist_len, const int* __restrict__ cur, ProcArgs a,
                                                              const int* __restrict__ seqtab, const int* __restrict__ base) {
    __shared__ unsigned seen[PROC_WORDS], ban[PROC_WORDS], biased[PROC_WORDS];
    __shared__ int s_tok[VZ_PROC_MAX_SEQ];          // the id sequence k biases in this row, -1: none (it does not act, or it bans)
    __shared__ float s_bias[VZ_PROC_MAX_SEQ];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int W = (cols + 31) >> 5;
    int* h = hist + (size_t)row * hist_stride;
    float* lr = logits + (size_t)row * cols;

    // every thread reads the length and the token to append BEFORE the barrier; thread 0 writes both behind it
    const int n0 = min(max(hist_len[row], 0), hist_stride);
    const bool app = cur != nullptr && n0 < hist_stride;
    const int c = cur ? cur[row] : -1;
    const int n_seq = seqtab ? a.n_seq : 0;
    // ids the history was seeded with before the first generated one (a call that continues on a kept cache: the cached conversation);
    // they count for the penalty, the n-grams and the id sequences, as a prompt's ids do in HF, but not as NEW tokens
    const int n_base = base ? min(max(base[row], 0), n0) : 0;
    for (int w = tid; w < W; w += 1024) { seen[w] = 0; ban[w] = 0; if (n_seq) biased[w] = 0; }
    __syncthreads();
    if (app && tid == 0) { h[n0] = c; hist_len[row] = n0 + 1; }
    const int n = app ? n0 + 1 : n0;                     // entries the processors see; h[n0] = c is taken from the register
    const int g = a.ngram;

    if (n > 0 && (a.penalty != 1.f || g > 0)) {
        // the tail h[n - g + 1 .. n) the n-grams are compared with: g - 1 <= 7 tokens, once, in registers
        const bool grams = g > 0 && n >= g;
        int tail[PROC_G - 1];
#pragma unroll
        for (int j = 0; j < PROC_G - 1; ++j) {
            const int k = min(max(n - g + 1 + j, 0), n - 1);
            const int v = h[k];
            tail[j] = (app && k == n0) ? c : v;
        }
        // position i: its token is seen; if an n-gram starts there (i + g - 1 < n) and its first g - 1 tokens equal the tail, its last
        // token is banned.  The 8 loads of a position are independent (clamped addresses, no branch): one wait for the batch.
        for (int i0 = 0; i0 < n; i0 += 1024) {
            const int i = i0 + tid;
            int w[PROC_G];
#pragma unroll
            for (int j = 0; j < PROC_G; ++j) {
                const int k = min(i + (j < g ? j : 0), n - 1);
                const int v = h[k];
                w[j] = (app && k == n0) ? c : v;
            }
            if (i < n) {
                if (a.penalty != 1.f) mark(seen, w[0], cols);
                if (grams && i + g - 1 < n) {
                    bool eq = true;
                    int last = w[0];
#pragma unroll
                    for (int j = 0; j < PROC_G; ++j) {
                        if (j < g - 1) eq = eq && w[j] == tail[j];
                        if (j == g - 1) last = w[j];
                    }
                    if (eq) mark(ban, last, cols);
                }
            }
        }
    }
    if (tid < 4 && tid < a.eos.n && n - n_base < a.min_new) mark(ban, a.eos.id[tid], cols);
    if (tid >= 64 && tid < 64 + 16 && tid - 64 < a.n_suppress) mark(ban, a.suppress[tid - 64], cols);
    if (tid >= 128 && tid - 128 < n_seq) {          // one thread per sequence of the table
        const int* q = seqtab + (tid - 128) * VZ_PROC_SEQ_STRIDE;
        const int L = min(max(q[0], 1), VZ_PROC_SEQ_IDS);
        bool hit = L == 1 || n >= L;                     // HF skips a sequence while len(sequence) > ids generated (not len - 1)
        for (int j = 0; j + 1 < L && hit; ++j) {
            const int k = n - (L - 1) + j;               // >= 1 here
            const int v = h[k];
            hit = ((app && k == n0) ? c : v) == q[4 + j];
        }
        const int last = q[4 + L - 1];
        int act = -1;
        if (hit && (unsigned)last < (unsigned)cols) {
            if (q[1]) mark(ban, last, cols);
            else { mark(biased, last, cols); act = last; }
        }
        s_tok[tid - 128] = act;
        s_bias[tid - 128] = __int_as_float(q[2]);
    }
    __syncthreads();

    const float p = a.penalty;
    for (int w = tid; w < W; w += 1024) {
        const unsigned b = ban[w], sn = seen[w], bs = n_seq ? biased[w] : 0u;
        unsigned m = sn | b | bs;
        while (m) {
            const int bit = __ffs(m) - 1;
            m &= m - 1;
            const int k = (w << 5) + bit;                // < cols: only ids inside [0, cols) set a bit
            if ((b >> bit) & 1u) {
                lr[k] = -INFINITY;
            } else {
                float x = lr[k];
                if ((bs >> bit) & 1u) {
                    float s = 0.f;
                    for (int i = 0; i < n_seq; ++i) if (s_tok[i] == k) s += s_bias[i];
                    x = x + s;
                }
                if ((sn >> bit) & 1u) x = x < 0.f ? x * p : x / p;
                lr[k] = x;
            }
        }
    }
}

}  // namespace

int vz_launch_logits_process(float* logits, int rows, int cols, int* hist, int hist_stride, int* hist_len, const int* cur,
                             const ProcArgs& a, const int* seqtab, hipStream_t s, const int* base) {
    VZ_CHECK_ARG(logits && hist && hist_len && rows > 0 && cols > 0 && hist_stride >= 1, "logits_process: bad argument");
    VZ_CHECK_ARG(cols <= PROC_MAX_COLS, "logits_process: %d columns, the LDS bitmaps hold %d", cols, PROC_MAX_COLS);
    VZ_CHECK_ARG(a.penalty > 0.f && a.ngram >= 0 && a.ngram <= PROC_G && a.min_new >= 0 && a.eos.n >= 0 && a.eos.n <= 4 && a.n_suppress >= 0 &&
                 a.n_suppress <= 16, "logits_process: penalty %g > 0, 0 <= ngram %d <= 8, min_new %d >= 0, <= 4 eos ids (%d), <= 16 suppressed ids (%d) expected",
                 (double)a.penalty, a.ngram, a.min_new, a.eos.n, a.n_suppress);
    VZ_CHECK_ARG(a.n_seq >= 0 && a.n_seq <= VZ_PROC_MAX_SEQ && (a.n_seq == 0 || seqtab), "logits_process: %d id sequences, 0..%d with their table expected", a.n_seq, VZ_PROC_MAX_SEQ);
    hipLaunchKernelGGL(logits_process_kernel, dim3(rows), dim3(1024), 0, s, logits, cols, hist, hist_stride, hist_len, cur, a, seqtab, base);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}

// The per-row form: the same filter, but row r takes its parameters from record r of a table in device memory
// (ProcRow, vz_common.h = vz_proc_row of the C ABI) and its id sequences from region r of a per-row sequence table
// [rows][VZ_PROC_MAX_SEQ][VZ_PROC_SEQ_STRIDE] - the rows of a continuous batch are independent requests.  A captured step reads both
// through pointers: a changed record changes no kernel argument.  A row whose record is inactive leaves on a workgroup-uniform branch
// right behind the record: no LDS cleared, no logit touched, nothing appended.  Same algorithm, operation order and plain fp32 * and / as
// logits_process_kernel above: bit-identical to it row by row.
// Everything whose address is known at entry - the record (uniform: scalar loads), the row's length / token / base, the first batch of
// 8 history ids per thread (clamped to the buffer, not to the length: what lies behind the length is never used), the thread's word of
// the eos / suppress lists and its sequence entry - is requested before anything is waited for: one memory round trip in front of the
// marking pass however many of the processors the record arms.
namespace {

// STEP: inside a decode step - cur and base are there (cur[row] is appended); else neither is (an op-level call: nothing is appended)
template <bool STEP>
__global__ __launch_bounds__(1024) void logits_process_rows_kernel(float* logits, int cols, int* hist, int hist_stride, int* hist_len, const int* cur,
                                                                   const ProcRow* tab, const int* seqtab, const int* base) {
    __shared__ unsigned seen[PROC_WORDS], ban[PROC_WORDS], biased[PROC_WORDS];
    __shared__ int s_tok[VZ_PROC_MAX_SEQ];
    __shared__ float s_bias[VZ_PROC_MAX_SEQ];
    const int row = blockIdx.x, tid = threadIdx.x;
    const ProcRow* rp = tab + row;
    int* h = hist + (size_t)row * hist_stride;
    float* lr = logits + (size_t)row * cols;

    const int active = rp->active;
    const float p = rp->penalty;
    const int g = rp->ngram, min_new = rp->min_new, n_eos = rp->eos.n, n_suppress = rp->n_suppress, n_seq = rp->n_seq;
    const int len_raw = hist_len[row];
    const int c = STEP ? cur[row] : -1;
    const int base_raw = STEP ? base[row] : 0;
    // thread t < 4: eos id t; thread 64 + t, t < 16: suppressed id t (words of the record: no indexed copy of it in registers)
    const int list_word = tid < 4 ? (int)(offsetof(ProcRow, eos.id) / 4) + tid
                                  : (int)(offsetof(ProcRow, suppress) / 4) + min(max(tid - 64, 0), 15);
    const int list_id = ((const int*)rp)[list_word];
    int w0[PROC_G];
#pragma unroll
    for (int j = 0; j < PROC_G; ++j) w0[j] = h[min(tid + j, hist_stride - 1)];
    // thread 128 + k: entry k of the row's region (every thread loads a clamped one: no branch around the loads)
    const int4* qp = (const int4*)(seqtab + ((size_t)row * VZ_PROC_MAX_SEQ + min(max(tid - 128, 0), VZ_PROC_MAX_SEQ - 1)) * VZ_PROC_SEQ_STRIDE);
    const int4 q0 = qp[0], q1 = qp[1], q2 = qp[2];       // [len | bad | bias | - ] [ids 0..3] [ids 4..7]

    asm volatile("" ::: "memory");          // the requests above stay above the branch: in flight while the record decides
    if (!__builtin_amdgcn_readfirstlane(active)) return;

    const int W = (cols + 31) >> 5;
    const int n0 = min(max(len_raw, 0), hist_stride);
    const bool app = STEP && n0 < hist_stride;
    const int n_base = min(max(base_raw, 0), n0);
    for (int w = tid; w < W; w += 1024) { seen[w] = 0; ban[w] = 0; if (n_seq) biased[w] = 0; }
    __syncthreads();
    if (app && tid == 0) { h[n0] = c; hist_len[row] = n0 + 1; }
    const int n = app ? n0 + 1 : n0;

    if (n > 0 && (p != 1.f || g > 0)) {
        const bool grams = g > 0 && n >= g;
        int tail[PROC_G - 1];
#pragma unroll
        for (int j = 0; j < PROC_G - 1; ++j) {
            const int k = min(max(n - g + 1 + j, 0), n - 1);
            const int v = h[k];
            tail[j] = (app && k == n0) ? c : v;
        }
        for (int i0 = 0; i0 < n; i0 += 1024) {
            const int i = i0 + tid;
            int w[PROC_G];
#pragma unroll
            for (int j = 0; j < PROC_G; ++j) {
                const int k = i + j;                     // used only while k < n (j < g and the n-gram fits), so the clamp is never seen
                const int v = i0 == 0 ? w0[j] : h[min(k, hist_stride - 1)];
                w[j] = (app && k == n0) ? c : v;
            }
            if (i < n) {
                if (p != 1.f) mark(seen, w[0], cols);
                if (grams && i + g - 1 < n) {
                    bool eq = true;
                    int last = w[0];
#pragma unroll
                    for (int j = 0; j < PROC_G; ++j) {
                        if (j < g - 1) eq = eq && w[j] == tail[j];
                        if (j == g - 1) last = w[j];
                    }
                    if (eq) mark(ban, last, cols);
                }
            }
        }
    }
    if (tid < 4 && tid < n_eos && n - n_base < min_new) mark(ban, list_id, cols);
    if (tid >= 64 && tid < 64 + 16 && tid - 64 < n_suppress) mark(ban, list_id, cols);
    if (tid >= 128 && tid - 128 < n_seq) {
        const int ids[VZ_PROC_SEQ_IDS] = {q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
        const int L = min(max(q0.x, 1), VZ_PROC_SEQ_IDS);
        bool hit = L == 1 || n >= L;
        int last = ids[0];
#pragma unroll
        for (int j = 0; j < VZ_PROC_SEQ_IDS; ++j) {
            if (j + 1 < L && hit) {
                const int k = n - (L - 1) + j;           // >= 1 here
                const int v = h[k];
                hit = ((app && k == n0) ? c : v) == ids[j];
            }
            if (j == L - 1) last = ids[j];
        }
        int act = -1;
        if (hit && (unsigned)last < (unsigned)cols) {
            if (q0.y) mark(ban, last, cols);
            else { mark(biased, last, cols); act = last; }
        }
        s_tok[tid - 128] = act;
        s_bias[tid - 128] = __int_as_float(q0.z);
    }
    __syncthreads();

    for (int w = tid; w < W; w += 1024) {
        const unsigned b = ban[w], sn = seen[w], bs = n_seq ? biased[w] : 0u;
        unsigned m = sn | b | bs;
        while (m) {
            const int bit = __ffs(m) - 1;
            m &= m - 1;
            const int k = (w << 5) + bit;
            if ((b >> bit) & 1u) {
                lr[k] = -INFINITY;
            } else {
                float x = lr[k];
                if ((bs >> bit) & 1u) {
                    float s = 0.f;
                    for (int i = 0; i < n_seq; ++i) if (s_tok[i] == k) s += s_bias[i];
                    x = x + s;
                }
                if ((sn >> bit) & 1u) x = x < 0.f ? x * p : x / p;
                lr[k] = x;
            }
        }
    }
}

}  // namespace

// the check of one record (every entry point that takes a vz_proc_row runs it before it touches the device): vz_launch_logits_process's limits
int vz_proc_row_check(const ProcRow& a) {
    if (!a.active) return VZ_OK;
    VZ_CHECK_ARG(a.penalty > 0.f && a.ngram >= 0 && a.ngram <= PROC_G && a.min_new >= 0 && a.eos.n >= 0 && a.eos.n <= 4 && a.n_suppress >= 0 &&
                 a.n_suppress <= 16, "logits_process_rows: penalty %g > 0, 0 <= ngram %d <= 8, min_new %d >= 0, <= 4 eos ids (%d), <= 16 suppressed ids (%d) expected",
                 (double)a.penalty, a.ngram, a.min_new, a.eos.n, a.n_suppress);
    VZ_CHECK_ARG(a.n_seq >= 0 && a.n_seq <= VZ_PROC_MAX_SEQ, "logits_process_rows: %d id sequences, 0..%d expected", a.n_seq, VZ_PROC_MAX_SEQ);
    return VZ_OK;
}

int vz_launch_logits_process_rows(float* logits, int rows, int cols, int* hist, int hist_stride, int* hist_len, const int* cur,
                                  const ProcRow* d_records, const int* d_seqtab, const int* base, hipStream_t s) {
    VZ_CHECK_ARG(logits && hist && hist_len && d_records && d_seqtab && rows > 0 && cols > 0 && hist_stride >= 1, "logits_process_rows: bad argument");
    VZ_CHECK_ARG(cols <= PROC_MAX_COLS, "logits_process_rows: %d columns, the LDS bitmaps hold %d", cols, PROC_MAX_COLS);
    VZ_CHECK_ARG((cur == nullptr) == (base == nullptr), "logits_process_rows: a step hands over the rows' tokens and seeded-id counts, an op-level call neither");
    if (cur) hipLaunchKernelGGL(logits_process_rows_kernel<true>, dim3(rows), dim3(1024), 0, s, logits, cols, hist, hist_stride, hist_len, cur, d_records, d_seqtab, base);
    else hipLaunchKernelGGL(logits_process_rows_kernel<false>, dim3(rows), dim3(1024), 0, s, logits, cols, hist, hist_stride, hist_len, cur, d_records, d_seqtab, base);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}
