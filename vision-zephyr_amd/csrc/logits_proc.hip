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
