// Engine internals shared by engine.hip and train_engine.hip: the engine object with its weight tables, the arena carver, the profiling
// scope and the few engine functions the training step calls.  Nothing here is part of the C ABI (include/viszephyr.h).
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include <rccl/rccl.h>

#include "linear_route.h"

struct Weight { const void* p; int dtype; long n; };

// The weight tables the stages read, filled by vz_engine_finalize from the name registry.  A linear: the bf16 matrix [N, K] and its
// fragment-tiled copy ("<name>t" if registered: the 2..64-row decode streams read it), the e4m3 copy + fp32 row scales (weight_fp8
// engines only) and the e4m3 copy's tiled copy, the fp32 bias; null = absent.
struct LinW {
    const bf16_t* w = nullptr; const bf16_t* wt = nullptr;
    const unsigned char* w8 = nullptr; const unsigned char* w8t = nullptr; const float* ws = nullptr;
    const float* b = nullptr;
};
static LinW bare(const bf16_t* w) { LinW l; l.w = w; return l; }      // a matrix with nothing attached (trainer operands)
// rows r0.. of a linear's matrix [., K] and bias (Q-Former block 0 runs the K|V rows of sa_in on their own)
static LinW lin_rows(const LinW& l, long r0, int K) { LinW s = bare(l.w + r0 * K); s.b = l.b + r0; return s; }
struct NormW { const float* w = nullptr; const float* b = nullptr; };      // LayerNorm scale + shift
struct ClipLayerW { NormW ln1, ln2; LinW qkv, o, fc1, fc2; };
struct QfBlockW { NormW n1, n2, n3; LinW sa_in, sa_out, ca_q, ca_kv, ca_out, ffn1, ffn2; };
struct LlmLayerW { const float* in_norm = nullptr; const float* post_norm = nullptr; LinW qkv, o, gu, down; };
struct TopW {
    const bf16_t *clip_patch_w = nullptr, *clip_cls = nullptr, *clip_pos = nullptr; NormW clip_pre_ln;
    const bf16_t* qf_queries = nullptr; NormW qf_pre_norm, qf_norm;
    const bf16_t* embed = nullptr; const float* norm = nullptr; LinW lm_head;
};

static constexpr float ATTN_SCALE = 0.08838834764831845f;      // 128^-0.5 (vz_engine_create takes head_dim 128 only)

// The device-side state of a decode batch of max_batch = mb rows: [cur | pos | slot | len], mb ints each (the row's input token, its
// rotary position, the cache slot its keys are appended to, the keys it sees), then WORDS ints: the step index inside the running
// vz_llm_decode_steps call, the draws since vz_llm_decode_begin, the sampler's seed (lo, hi); then the per-row tail's table, one
// RowSample per row (16-byte aligned: 4 * (mb + 1) ints precede it).
struct DecodeState {
    static constexpr int ROW_ARRAYS = 4, WORDS = 4, SAMPLE_INTS = sizeof(RowSample) / sizeof(int);
    int *cur, *pos, *slot, *len, *step, *ctr; unsigned* seed; RowSample* samp;
    static size_t ints(int mb) { return (size_t)(ROW_ARRAYS + SAMPLE_INTS) * mb + WORDS; }
};
static DecodeState decode_state(int* base, int mb) {
    int* w = base + DecodeState::ROW_ARRAYS * mb;
    return {base, base + mb, base + 2 * mb, base + 3 * mb, w, w + 1, (unsigned*)(w + 2), (RowSample*)(w + DecodeState::WORDS)};
}

// The tail of a decode step turns the logits into the next tokens: speculative verify > beam select > per-row table > sampler > argmax,
// whichever armed mode comes first (tail_kind).  The *Args of a mode are what its kernels take by value - a captured step freezes them, so
// they go into the graph key as they are; they are laid out without padding (the key is compared with memcmp).
enum TailKind { TAIL_GREEDY = 0, TAIL_SAMPLE, TAIL_BEAM, TAIL_SPEC, TAIL_ROWS };      // TAIL_ROWS takes nothing by value: its table is device memory
struct SampleArgs { int top_k; float temp, top_p; SampleWarp warp; };
static constexpr RowSample ROW_GREEDY{VZ_ROW_GREEDY, 1.f, 0, 1.f, {0u, 0u}, 0, 0, {0.f, 0.f, 0.f, 0.f}};      // the canonical greedy entry (row_sample_of)
struct BeamArgs { int* hist; int nb, groups, hist_cap; BeamEos eos; };      // hist = the caller's history records, hist_cap steps
// the beam tail's row recorder (vz_llm_decode_beam_rows): rings of `cap` steps x (groups * nb) rows x vocab fp32, written at the beam
// tail's history index mod cap - scores = the processed log-prob rows (HF's scores[t]), raw = the logits rows; null = not recorded
struct BeamRowsArgs { float *scores, *raw; int cap, pad; };
struct SpecArgs {
    int *hist, *out, *ctl, *stats; const int* stream;
    int ngram, source, budget, hist_cap, stats_cap, stream_len;
    int key_bound;      // keys the steps being launched can reach (fixes the verify attention's absolute splits)
    BeamEos eos;
    RowSample samp;     // ROW_GREEDY: argmax verify; a VZ_ROW_SAMPLE record (vz_llm_decode_spec_sampling; its ctr 0): spec_sample_kernel draws the rows
};
// Everything decode_step_launch hands to a kernel that can differ between two vz_llm_decode_steps calls: a replayed graph is only
// valid while all of it is unchanged.  The *Args of the modes that are off stay zero.
struct DecodeGraphKey {
    int B, n, nsplit, use_tok, kind; unsigned tune_epoch;
    int* out; char* arena; int* ring; int ring_n;
    SampleArgs samp; BeamArgs beam; SpecArgs spec;
    int* proc_hist; const int* proc_seq; ProcArgs proc; int proc_on;      // the logits processors in front of the tail, their history buffer and sequence table (zero when off)
    float *sc_rec, *sc_warped, *sc_raw; unsigned sc_what; int sc_cap;      // the step recorder behind the tail and its rings (zero when off)
    int* stop_state; StopArgs stop;      // the stop matcher behind the tail: its state, tables and dims (zero when off)
    BeamRowsArgs beam_rows;              // the beam tail's row recorder: its rings (zero when off)
    float cfg_scale; int cfg_pairs;      // classifier-free guidance between the logits and the processors (zero when off)
    int proc_rows_on, stop_rows_on;      // the per-row processors / per-row stop sequences: mode bits only - their tables are engine-owned, stable device memory read through pointers
    int share_n, share_nsplit; const int* share_tab;      // the shared-prefix attention (vz_llm_decode_share): rows per group, key splits, the `shared` table (zero when off)
    const unsigned char* kv8;            // the e4m3 KV mirror the decode attention streams (vz_engine_kv_fp8; null when off)
};
static_assert(sizeof(DecodeGraphKey) == 6 * 4 + 3 * 8 + 4 + sizeof(SampleArgs) + sizeof(BeamArgs) + sizeof(SpecArgs) + 2 * 8 + sizeof(ProcArgs) + 4 + 3 * 8 + 2 * 4 + 8 + sizeof(StopArgs) + sizeof(BeamRowsArgs) + 2 * 4 + 2 * 4 + 2 * 4 + 8 + 8 &&
              sizeof(BeamRowsArgs) == 2 * 8 + 2 * 4 &&
              sizeof(BeamArgs) == 8 + 3 * 4 + sizeof(BeamEos) && sizeof(SpecArgs) == 5 * 8 + 7 * 4 + sizeof(BeamEos) + sizeof(RowSample), "padding in the graph key");

// The beam tail's device state, BEAM_ROWS rows: [score (fp32) | parent | base | hidx, pad | base, end of a standalone reorder | candidate
// scores | candidate tokens (BEAM_K per row)]
static constexpr int BEAM_ROWS = 64, BEAM_K = 80;
static constexpr size_t BEAM_INTS = 4 + 5 * (size_t)BEAM_ROWS + 2 * (size_t)BEAM_ROWS * BEAM_K;
struct BeamView { float* score; int *parent, *base, *hidx, *re_base, *re_end; float* cand_s; int* cand_t; };
static BeamView beam_view(int* d) {
    const int R = BEAM_ROWS;
    int* cand = d + 5 * R + 4;
    return {(float*)d, d + R, d + 2 * R, d + 3 * R, d + 3 * R + 4, d + 4 * R + 4, (float*)cand, cand + R * BEAM_K};
}

struct vz_engine {
    vz_config c;
    // tensor parallelism: this rank's share of the 32 query heads / 8 KV heads / 14336 MLP columns and
    // of the vocabulary (Vp = ceil(vocab / tp) rows of lm_head, zero padded); tp == 1: everything.
    int tp = 1, rank = 0, Hq_l = 0, Hkv_l = 0, I_l = 0, Vp = 0;
    ncclComm_t comm = nullptr;
    // one-shot all-reduce of the decode step (comm_oneshot.hip): this rank's receive area, every rank's area (peer-mapped), sequence words
    void* os_area = nullptr; void* os_areas[8] = {nullptr}; int os_ranks = 0; unsigned* os_seq = nullptr;
    static constexpr int OS_MAX_ELEMS = 64 * 4096;       // up to 64 decode rows of hidden 4096
    float* d_gather = nullptr;     // [tp][rows][Vp] all-gathered logits before the repack
    size_t gather_floats = 0;
    std::unordered_map<std::string, Weight> w;     // by name (vz_engine_set_weight); only vz_engine_finalize reads it
    // resolved by vz_engine_finalize; valid while `finalized`
    TopW top; std::vector<ClipLayerW> clip; std::vector<QfBlockW> qf; std::vector<LlmLayerW> llm;
    bool qf_kv_contig = false;     // > 1 Q-Former block and their ca_kv weights + biases lie back to back (block-major)
    bool finalized = false;
    // rope
    const float* cosT = nullptr; const float* sinT = nullptr; int rope_max = 0;
    // workspace (one arena, carved per stage; stages never overlap in time on a stream); arena_peak = the mark of the last stage's carving
    char* arena = nullptr; size_t arena_bytes = 0, arena_peak = 0;
    // kv cache: [layer][2][B][Hkv][max_ctx][D]
    bf16_t* kv = nullptr; size_t kv_layer_elems = 0;
    // decode state (device)
    int* d_state = nullptr;  // DecodeState of max_batch rows
    int dec_B = 0;
    int prefill_fp8 = 0;         // vz_engine_prefill_fp8: the Zephyr prefill linears run e4m3 x e4m3 on the scaled MFMA (weight_fp8 engines)
    bool comm_graph_ok = true;   // RCCL collectives captured into the decode graph (cleared if a capture is refused -> eager steps)
    int dec_len_max = 0;         // host-side bound on the longest row's visible keys (grows by one per launched step)
    // host mirror of the device-side decode state, per row: keys visible to the NEXT step, its rotary position, and whether the
    // row is parked (continuous batching: ctx_len 0, steps harmlessly, never checked against the capacity)
    std::vector<int> h_len, h_pos; std::vector<char> h_parked;
    // the step's tail (tail_kind): each mode is armed on its own, so disarming one falls back to the next armed one
    // sampling (vz_llm_decode_sampling): the checked record; its ctr / seed = the draw counter and the key the next vz_llm_decode_begin uploads
    struct { int on = 0; RowSample rec = ROW_GREEDY; } samp;
    // per-row table (vz_llm_decode_sampling_rows): tab = the max_batch entries the next vz_llm_decode_begin uploads (all greedy until set)
    struct { int on = 0; std::vector<RowSample> tab; } rows;
    // beam search (vz_llm_decode_beam): a.groups x a.nb rows; d = the device state (beam_view)
    // rows = the row recorder of the beam tail (zero: off)
    struct { int on = 0; BeamArgs a{}; int* d = nullptr; BeamRowsArgs rows{}; } beam;
    // prompt-lookup speculation (vz_llm_decode_spec; spec.hip): R = D + 1 rows of one sequence in cache row 0; base_len / base_pos = keys visible
    // to row 0 and its position when the mode was armed
    struct { int on = 0, R = 0, base_len = 0, base_pos = 0; SpecArgs a{}; } spec;
    // logits processors (vz_llm_decode_logits_proc; logits_proc.hip): orthogonal to the tail - armed, they run on the step's logits in front
    // of the argmax / the sampler.  d = [hist_len: max_batch ints, padded to 64 | hist: max_batch x max_ctx ints], its own allocation
    // d_seq / h_seq = the id-sequence table of sequence_bias / bad_words_ids (VZ_PROC_MAX_SEQ entries) and its host image: an arming
    // with an equal table uploads nothing; seq_epoch counts the uploads
    // rows_on (vz_llm_decode_logits_proc_rows): the per-row launch instead, over the same histories - d_rows = max_batch
    // records, d_rowseq = max_batch regions of VZ_PROC_MAX_SEQ sequence entries; allocated once, never moved
    struct { int on = 0; ProcArgs a{}; int* d = nullptr; int* d_seq = nullptr; std::vector<int> h_seq; int seq_epoch = 0;
             int rows_on = 0; ProcRow* d_rows = nullptr; int* d_rowseq = nullptr; } proc;
    // step recorder (vz_llm_decode_scores; sampling.hip: token_scores_kernel): behind the tail, a record per row and step into the caller's
    // rings of `cap` steps; d_slot = the steps launched since vz_llm_decode_begin (one word of its own, counted by the step-advance launch)
    struct { unsigned what = 0; float *rec = nullptr, *warped = nullptr, *raw = nullptr; int cap = 0; int* d_slot = nullptr; } score;
    // stop matcher (vz_llm_decode_stop; stop.hip: stop_match_kernel): behind the tail and the recorder.  d_state = max_batch rows of VZ_STOP_ROW
    // ints [n | at | ring]; d_tab = the tables of the armed stop set [emb | target | seq] (a.emb / a.target / a.seq point into it)
    // h_tab = the host image of d_tab (an arming with the same stop set uploads nothing); h_init = the state with no row watched
    // rows_on (vz_llm_decode_stop_row_seqs): rule 2 reads d_rowseq = max_batch regions of VZ_STOP_MAX_SEQ entries, then
    // max_batch counts; h_call = the call-level sequences every region starts with (a.n_seq entries; the matcher may be off: none)
    struct { int on = 0; StopArgs a{}; int* d_state = nullptr; int* d_tab = nullptr; size_t tab_ints = 0; std::vector<int> h_tab, h_init;
             int rows_on = 0; int* d_rowseq = nullptr; std::vector<int> h_call; } stop;
    // classifier-free guidance (vz_llm_decode_guidance; guidance.hip): orthogonal to the tail - armed, the decode batch is 2 * pairs rows
    // (row r < pairs a prompt, row pairs + r its negative prompt) and everything behind the logits runs on the first `pairs` rows
    struct { int on = 0, pairs = 0; float scale = 1.f; } cfg;
    // shared-prefix decode attention (vz_llm_decode_share; attn_shared.hip): the decode batch is groups x n rows and
    // the rows of a group read h_shared[g] leading slots from cache row g * n.  d_tab = the `shared` table (64 ints), q_rot = the rotated
    // queries [64][Hq][D], ws = the prefix partials - the engine's own allocations, made on the first arming, never carved from the arena
    struct { int on = 0, n = 0, groups = 0, shared_max = 0; std::vector<int> h_shared; int* d_tab = nullptr; bf16_t* q_rot = nullptr;
             float* ws = nullptr; size_t ws_floats = 0; } share;
    // e4m3 mirror of the KV cache for the decode attention (vz_engine_kv_fp8; attn_decode_kv8.hip): q = the cache's rows
    // as bytes at the bf16 cache's element offsets, sc = one fp32 power-of-two scale per 128-value row (offset / 128); the engine's own
    // allocations.  valid[row] = the row's mirror was (re)built by a prefill or a kv_move since the mirror was enabled
    struct { int on = 0; unsigned char* q = nullptr; float* sc = nullptr; std::vector<char> valid; } kv8;
    struct { int* p = nullptr; int n = 0, rows = 0; } ring;   // host-visible token ring of the streamer path (vz_llm_decode_ring): [rows][n]
    hipStream_t last_stream = nullptr;   // stream of the last stage call (vz_engine_async_error resets that stream's stream-K tickets)
    int dec_captures = 0;        // graphs captured since the engine was created (vz_llm_decode_info)
    int dec_nsplit = 1;          // context splits of the decode attention for the steps being launched
    float* d_logits = nullptr;   // [max_batch, vocab] fp32
    bf16_t* d_xnorm = nullptr;   // [64, hidden]: normalised rows of a 5..16-row decode batch (the MFMA weight stream reads them from L2)
    float* d_part = nullptr;     // decode attention partials
    unsigned* d_ticket = nullptr; // arrival counters of the fused decode attention
    unsigned* d_ao_done = nullptr; // arrival word of the attention + O-projection launch (attn_o_fused.hip); zeroed with the step counter
    int* d_ferr = nullptr;        // raised by a bounded device-side wait that expired
    int nsplit = 32;                 // upper bound: a split takes >= 128 keys, the splits beyond ceil(len / 128) leave at once
    VzTokState* tok = nullptr;          // persistent decode-token kernel (decode_persist.hip): per-layer pointer table + hand-off vectors + arrival counters
    bool use_tok = false;               // the steps being launched run on it (decided per vz_llm_decode_steps call)
    int tok_poke_word = -1; unsigned tok_poke_value = 0;      // TEST HOOK (vz_test_persist_poke): applied once, behind the next counter reset
    hipStream_t cap_stream = nullptr;   // stream capture is not allowed on the legacy null stream torch hands us
    hipGraphExec_t dec_graph = nullptr; DecodeGraphKey dec_graph_key{};      // the captured step and what it froze
    int* h_pinned = nullptr;     // pinned staging for small host->device uploads
    size_t h_pinned_ints = 0;
    // profiling
    int prof_on = 0, prof_class = -1;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev; size_t prof_used = 0;
};

#define RC(expr) do { int _r = (expr); if (_r) return _r; } while (0)

struct ProfScope {
    vz_engine* e; hipStream_t s; bool on; size_t idx; bool ext = false;
    ProfScope(vz_engine* e_, int klass, hipStream_t s_) : e(e_), s(s_), on(false), idx(0) {
        if (e->prof_on && klass == e->prof_class) {
            if (e->prof_used == e->prof_ev.size()) {
                hipEvent_t a, b;
                if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
                e->prof_ev.push_back({a, b});
            }
            idx = e->prof_used++;
            on = true;
            if (klass == K_GEMM || klass == K_GEMV) {      // stamped by the launch itself (kernel-only duration)
                g_vz_prof_start = e->prof_ev[idx].first;
                g_vz_prof_stop = e->prof_ev[idx].second;
                ext = true;
            } else {
                (void)hipEventRecord(e->prof_ev[idx].first, s);
            }
        }
    }
    ~ProfScope() {
        if (!on) return;
        if (ext) {
            if (g_vz_prof_start) { g_vz_prof_start = nullptr; g_vz_prof_stop = nullptr; e->prof_used--; }   // launch never happened
        } else {
            (void)hipEventRecord(e->prof_ev[idx].second, s);
        }
    }
};

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Carver {
    char* base; size_t off, cap; bool ok;
    size_t peak = 0;        // high-water mark of `off`: it survives a caller rewinding `off` to reuse scratch
    Carver(char* b, size_t c) : base(b), off(0), cap(c), ok(true) {}
    template <typename T> T* take(size_t n) {
        off = align_up(off, 256);
        T* p = (T*)(base + off);
        off += n * sizeof(T);
        if (off > cap) ok = false;
        if (off > peak) peak = off;
        return p;
    }
};

#define NEED_READY()                                                                                         \
    do {                                                                                                     \
        if (!e || !e->finalized) { vz_set_error("engine not finalized (register every weight, then vz_engine_finalize)"); return VZ_ERR_STATE; } \
    } while (0)

// engine.hip
int linear(vz_engine* e, int decode, const bf16_t* A, int lda, const LinW& W, int ldw, void* C, int ldc, int M,
           int N, int K, const bf16_t* res, int ldr, int act, int out_fp32, hipStream_t s,
           const float* norm_w = nullptr, float norm_eps = 0.f, int splitk_hint = 0);
int upload_ints(vz_engine* e, const int* h, size_t n, int* d, hipStream_t s);
int qf_attn(vz_engine* e, const bf16_t* q, long q_bs, long q_ss, const bf16_t* k, const bf16_t* v, long kv_bs, long kv_ss,
            bf16_t* o, int B, int Sq, int Sk, hipStream_t s, float* part = nullptr, size_t part_floats = 0);
int drop_decode_graph(vz_engine* e);
