// Stop strings and keyword stops, matched on the device behind the decode step's tail.
//
// stop_match_kernel: one 64-lane wave per row.  The row's state is VZ_STOP_ROW ints: n (generated tokens seen), at (-1, or the 0-based
// index of the token at which a stop condition first held - sticky; VZ_STOP_UNARMED: the row is not watched) and a ring of the last
// VZ_STOP_W ids, one per lane.  A call appends one id and decides two rules on the row's tail:
//   rule 1 (hf:generation/stopping_criteria.py StopStringCriteria.__call__, over the tables HF's own constructor builds): lane p <
//     n_str * max_end is the pair (stop string p / max_end, end-length candidate p % max_end) of the newest token; its walk starts if
//     that end length is > 0, an older token continues it if the running sum is one of the token's valid positions for the string
//     (then its length is added), the first token that does not ends it; the row matches if a walk's sum reaches the string's length.
//   rule 2 (ref:vis_zephyr/model/mm_utils.py KeywordsStoppingCriteria): lane k < n_seq is an id sequence: it matches when
//     n >= start_k + len_k and the last len_k ids equal it.
// The common step - no stop string can end in the new token, no sequence ends in it - is two memory round trips: the new token with the
// state, then the token's table entry with the target lengths and the sequences' heads; the ring slot and n are written, done.  When a walk is needed the table
// rows of all older window tokens are requested as batches of 8 independent loads per lane into LDS and the walks then run in LDS.
// Per-row mode: rule 2 takes row r's sequences and their count from region r of a per-row table instead of the shared
// one - the call-level sequences are copied in front of every row's own by whoever fills it; rule 1 stays shared.
// The kernel writes the state only: never a word the step reads.
#include "vz_common.h"

#define STOP_MAX_VEC (VZ_STOP_MAX_STR * (VZ_STOP_MAX_POS + VZ_STOP_MAX_END) + 1)

__global__ __launch_bounds__(64) void stop_match_kernel(StopArgs a, int* __restrict__ state, const int* __restrict__ ids, int reset,
                                                        const int* __restrict__ pre, const int* __restrict__ row_seq,
                                                        const int* __restrict__ row_nseq) {
    __shared__ int rowsL[(VZ_STOP_W - 1) * STOP_MAX_VEC];
    const int lane = threadIdx.x;
    int* st = state + (size_t)blockIdx.x * VZ_STOP_ROW;
    // everything the common step reads, requested before the first use
    const int tok = ids[blockIdx.x];
    int n = st[0], at = st[1], ringv = st[2 + lane];        // (read unconditionally: no branch between the loads; a reset row ignores them)
    if (reset) { n = 0; at = -1; }
    const int V1 = a.emb_rows - 1;                          // HF's dummy row: ids past the vocabulary are clamped to it
    const int ct = (tok < 0 || tok > V1) ? V1 : tok;
    const int npair = a.n_str * a.max_end;
    int end_len = -1, target = 0, s_idx = 0;
    if (lane < npair) {
        s_idx = lane / a.max_end;
        end_len = a.emb[(size_t)ct * a.vec + a.n_str * a.max_pos + lane];
        target = a.target[s_idx];
    }
    // per-row mode (row_seq): the row's own region and count; the count is requested beside the heads, not in front of them - the region
    // holds VZ_STOP_MAX_SEQ entries whatever the count is
    const int* sq = (row_seq ? row_seq + (size_t)blockIdx.x * VZ_STOP_MAX_SEQ * VZ_STOP_SEQ_STRIDE : a.seq) + lane * VZ_STOP_SEQ_STRIDE;      // [len, start, ids newest first]
    int len = 0, start = 0, head = 0;
    int n_seq = row_seq ? row_nseq[blockIdx.x] : a.n_seq;
    if (lane < (row_seq ? VZ_STOP_MAX_SEQ : a.n_seq)) { len = sq[0]; start = sq[1]; head = sq[2]; }
    n_seq = min(max(__builtin_amdgcn_readfirstlane(n_seq), 0), VZ_STOP_MAX_SEQ);
    n = __builtin_amdgcn_readfirstlane(n);
    at = __builtin_amdgcn_readfirstlane(at);
    if (at != -1) return;                                   // stopped already (sticky), or not armed
    const int n1 = n + 1;
    if (lane == (n & (VZ_STOP_W - 1))) { ringv = tok; st[2 + lane] = tok; }

    // rule 2: the newest id first, the rest only for a sequence that ends in it
    bool ok2 = lane < n_seq && len >= 1 && len <= VZ_STOP_MAX_SEQ_LEN && n1 >= start + len && head == tok;
    if (__any(ok2)) {
        // the older ids of every sequence whose head matched, requested as one batch (the table row holds VZ_STOP_MAX_SEQ_LEN ids whatever
        // len is), then compared in registers against ring values moved by __shfl: no dependent load per id
        int q[VZ_STOP_MAX_SEQ_LEN - 1];
#pragma unroll
        for (int j = 1; j < VZ_STOP_MAX_SEQ_LEN; ++j) q[j - 1] = ok2 ? sq[2 + j] : 0;
#pragma unroll
        for (int j = 1; j < VZ_STOP_MAX_SEQ_LEN; ++j) {
            const int rv = __shfl(ringv, (n1 - 1 - j) & (VZ_STOP_W - 1));
            if (j < len && q[j - 1] != rv) ok2 = false;
        }
    }

    // rule 1
    const bool live = end_len > 0;
    bool hit1 = live && end_len >= target;
    // window: the newest token and L - 1 older ones.  pre (optional): ids the ring was seeded with in front of the first generated token,
    // slots 63, 62, .. = the newest first (a call that continues on a kept cache): HF's criterion sees them as the tail of its input_ids,
    // so a stop string may begin in them; rule 2 looks at generated ids only, as the reference's criterion does behind its start length
    const int n_seen = n1 + (pre ? min(max(pre[blockIdx.x], 0), VZ_STOP_W - 1) : 0);
    const int L = n_seen < a.window ? n_seen : a.window;
    if (L > 1 && __any(live && !hit1)) {
        const int total = (L - 1) * a.vec;
        for (int base = 0; base < total; base += 64 * 8) {
            int v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int el = base + u * 64 + lane, ec = el < total ? el : total - 1;
                const int i = ec / a.vec, col = ec - i * a.vec;
                int id = __shfl(ringv, (n1 - 2 - i) & (VZ_STOP_W - 1));
                id = (id < 0 || id > V1) ? V1 : id;
                v[u] = a.emb[(size_t)id * a.vec + col];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int el = base + u * 64 + lane;
                if (el < total) rowsL[el] = v[u];
            }
        }
        __syncthreads();
        if (live && !hit1) {
            int sum = end_len;
            for (int i = 0; i < L - 1; ++i) {
                const int* row = rowsL + i * a.vec;
                bool cont = false;
                for (int q = 0; q < a.max_pos; ++q) cont |= row[s_idx * a.max_pos + q] == sum;      // (sum > 0: a -1 entry never matches)
                if (!cont) break;
                sum += row[a.vec - 1];
                if (sum >= target) { hit1 = true; break; }
            }
        }
    }
    const bool hit = __any(hit1 || ok2);
    if (lane == 0) {
        st[0] = n1;
        if (hit) st[1] = n1 - 1;
        else if (reset) st[1] = -1;
    }
}

static int stop_args_ok(const StopArgs& a, bool per_row) {
    VZ_CHECK_ARG(a.n_str >= 0 && a.n_str <= VZ_STOP_MAX_STR && a.n_seq >= 0 && a.n_seq <= VZ_STOP_MAX_SEQ && (per_row || a.n_str + a.n_seq >= 1),
                 "stop_match: %d stop strings (0..%d), %d id sequences (0..%d), at least one of either", a.n_str, VZ_STOP_MAX_STR, a.n_seq, VZ_STOP_MAX_SEQ);
    if (a.n_str) {
        VZ_CHECK_ARG(a.emb && a.target && a.emb_rows >= 1, "stop_match: stop strings without their tables");
        VZ_CHECK_ARG(a.max_pos >= 1 && a.max_pos <= VZ_STOP_MAX_POS && a.max_end >= 1 && a.max_end <= VZ_STOP_MAX_END && a.window >= 1 && a.window <= VZ_STOP_W,
                     "stop_match: max_valid_positions %d (1..%d), max_valid_end_lens %d (1..%d), maximum_token_len %d (1..%d)", a.max_pos, VZ_STOP_MAX_POS,
                     a.max_end, VZ_STOP_MAX_END, a.window, VZ_STOP_W);
        VZ_CHECK_ARG(a.vec == a.n_str * (a.max_pos + a.max_end) + 1, "stop_match: table rows of %d words, %d x (%d + %d) + 1 expected", a.vec, a.n_str,
                     a.max_pos, a.max_end);
    }
    VZ_CHECK_ARG(a.n_seq == 0 || a.seq, "stop_match: id sequences without their table");
    return VZ_OK;
}

int vz_launch_stop_match(const StopArgs& a, int* state, int rows, const int* ids, int reset, hipStream_t s, const int* pre, const int* row_seq,
                         const int* row_nseq) {
    VZ_CHECK_ARG(state && ids && rows >= 1 && (row_seq == nullptr) == (row_nseq == nullptr), "stop_match: bad argument");
    { int r = stop_args_ok(a, row_seq != nullptr); if (r) return r; }
    hipLaunchKernelGGL(stop_match_kernel, dim3(rows), dim3(64), 0, s, a, state, ids, reset, pre, row_seq, row_nseq);
    VZ_LAUNCH_CHECK();
    return VZ_OK;
}
