// Stage-1 pretrain step on the engine and the Stage-2 LoRA step on top of it - a translation unit of its own
// over the engine's internals (engine_internal.h: the weight tables, `linear()` dispatch, arena carver; the stage kernels through vz_common.h).
// What the reference does (ref:vis_zephyr/train/train.py:817-829: freeze
// everything, re-enable `mm_projector`; ref:vis_zephyr/model/language_model/vis_zephyr.py:51-98 -> HF ForCausalLMLoss;
// ref:script/pretrain.sh:39-42 -> AdamW lr 2e-5 / cosine / warm-up 3 %, DeepSpeed ZeRO-2 data parallelism):
//
//   forward  tiles -> CLIP (no grad) -> fusion -> Q-Former (activations kept) -> splice -> 32 frozen Zephyr layers (activations
//            kept) -> lm_head on every position -> shifted cross-entropy, mean over the valid targets
//   backward dlogits -> lm_head^T -> final RMSNorm -> per layer (reverse): down^T, SwiGLU', gate|up^T, RMSNorm', o^T, attention
//            backward (causal GQA, head 128), RoPE^T, qkv^T, RMSNorm' (INPUT gradients only: Zephyr is frozen) -> rows of
//            d(inputs_embeds) that hold visual tokens -> Q-Former backward with all 165 parameter gradients (attention backward
//            head 512, LayerNorm / exact-GELU backward, weight gradients with the row dimension as the contraction)
//   update   fused AdamW over the projector tensors (fp32 master + moments; bf16 / fp32 working copies = the engine's weights),
//            after an RCCL all-reduce of the flat fp32 gradient arena when a data-parallel communicator is attached.
//
// Contractions: see train.hip's header (everything on the forward's MFMA tile GEMMs through transposed operands).
// Memory: one bump arena per trainer (saved activations + scratch).  The step's own carving sizes it: the step runs once without launches
// to find its high-water mark, then for real ("the step's memory" below).  vz_train_stage1_accumulate = argument checks, sizing, four phases.
#include <math.h>

#include <algorithm>

#include "engine_internal.h"


struct ProjParam { std::string name; int dtype; long n; size_t off; void* work; };

// Stage-2 LoRA adapters (ref:vis_zephyr/train/train.py:933-951, peft LoraConfig; see the block before vz_train_lora_enable)
constexpr int LORA_MODS = 7;                                    // q k v o gate up down
static const char* const LORA_MOD_NAMES[LORA_MODS] = {"q", "k", "v", "o", "gate", "up", "down"};
struct LoraState {
    int r = 0; float alpha = 0.f, p = 0.f, scaling = 0.f; unsigned long long seed = 0;
    int first = -1;                                             // table index of lora.0.q.A; A / B of (layer, module) follow in order
    bf16_t* work = nullptr;                                     // bf16 working copies of every factor (one block)
    int step = 0; long sample_base = 0, row_stride = 0;         // dropout counter of the next micro-batch
};

// gradients of the projector tensors in the trainer's flat fp32 arena, by block: parallel to the engine's Q-Former table
struct GradWB { float* w = nullptr; float* b = nullptr; };          // a linear's weight + bias, or a LayerNorm's scale + shift
struct QfBlockG { GradWB n1, n2, n3, sa_in, sa_out, ca_q, ca_kv, ca_out, ffn1, ffn2; };

struct vz_trainer {
    vz_engine* e = nullptr;
    std::vector<bf16_t*> t_qkv, t_o, t_gu, t_down;     // W^T of the frozen Zephyr linears: [H,QKV] [A,H] [H,2I] [I,H]
    bf16_t* t_lm = nullptr; int Vpad = 0;               // [H, Vpad]
    std::vector<ProjParam> params; std::unordered_map<std::string, int> index;
    float *master = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr; size_t total = 0;
    char* ws = nullptr; size_t ws_bytes = 0, ws_peak = 0;     // the step arena; high-water mark of the last step in it
    float* d_loss_rows = nullptr; size_t loss_rows_cap = 0; long loss_rows_n = 0;
    int adam_t = 0;
    ncclComm_t dp_comm = nullptr; int dp_world = 1;
    LoraState lora;
    std::vector<QfBlockG> g_qf; GradWB g_pre_norm, g_norm; float* g_queries = nullptr;     // into `grad` (bind_grads)
};

// points the projector gradient table into the current `grad` arena (vz_train_create; again when LoRA moves the arenas)
static int bind_grads(vz_trainer* tr) {
    const vz_config& c = tr->e->c;
    const long H = c.hidden, KD = c.qf_kv_dim;
    int rc = VZ_OK;
    auto g = [&](const std::string& name, long n) -> float* {
        auto it = tr->index.find(name);
        if (it != tr->index.end() && tr->params[it->second].n == n) return tr->grad + tr->params[it->second].off;
        if (!rc) vz_set_error("trainer: no projector tensor '%s' of %ld elements", name.c_str(), n);
        rc = VZ_ERR_STATE;
        return nullptr;
    };
    auto wb = [&](const std::string& p, long n, long nb) { GradWB r; r.w = g(p + ".w", n); r.b = g(p + ".b", nb); return r; };
    tr->g_queries = g("qf.queries", c.qf_queries * H); tr->g_pre_norm = wb("qf.pre_norm", KD, KD); tr->g_norm = wb("qf.norm", H, H);
    tr->g_qf.assign(c.qf_blocks, QfBlockG());
    for (int i = 0; i < c.qf_blocks; ++i) {
        const std::string p = "qf." + std::to_string(i) + ".";
        QfBlockG& G = tr->g_qf[i];
        G.n1 = wb(p + "n1", H, H); G.n2 = wb(p + "n2", H, H); G.n3 = wb(p + "n3", H, H);
        G.sa_in = wb(p + "sa_in", 3 * H * H, 3 * H); G.sa_out = wb(p + "sa_out", H * H, H);
        G.ca_q = wb(p + "ca_q", H * H, H); G.ca_kv = wb(p + "ca_kv", 2 * H * KD, 2 * H); G.ca_out = wb(p + "ca_out", H * H, H);
        G.ffn1 = wb(p + "ffn1", 2 * H * H, 2 * H); G.ffn2 = wb(p + "ffn2", 2 * H * H, H);
    }
    return rc;
}

static int pad64(int v) { return (v + 63) & ~63; }

static int transpose2d(const bf16_t* src, int R, int C, bf16_t* dst, int dst_rs, hipStream_t s) {
    return vz_launch_transpose(src, C, 0, 0, dst, dst_rs, 0, 0, R, C, 1, 1, 0, s);
}

extern "C" int vz_train_destroy(vz_trainer* tr) {
    if (!tr) return VZ_OK;
    (void)hipDeviceSynchronize();
    for (auto* v : {&tr->t_qkv, &tr->t_o, &tr->t_gu, &tr->t_down}) for (bf16_t* p : *v) if (p) (void)hipFree(p);
    for (void* p : {(void*)tr->t_lm, (void*)tr->master, (void*)tr->m, (void*)tr->v, (void*)tr->grad, (void*)tr->ws, (void*)tr->d_loss_rows,
                    (void*)tr->lora.work}) if (p) (void)hipFree(p);
    if (tr->dp_comm) (void)ncclCommDestroy(tr->dp_comm);
    delete tr;
    return VZ_OK;
}

// Builds the trainer of a finalized, single-GPU (tp_size 1) engine: W^T copies of the frozen Zephyr linears (+14.5 GB at 32 layers),
// fp32 master / Adam moments / gradient arenas for the projector (4 x 6.7 GB), masters initialised from the engine's working copies.
extern "C" int vz_train_create(vz_engine* e, vz_trainer** out, vz_stream stream) {
    NEED_READY();
    VZ_CHECK_ARG(out && e->tp == 1 && !e->c.weight_fp8, "train_create: needs a tp_size 1, bf16-weight engine");
    hipStream_t s = (hipStream_t)stream;
    const vz_config& c = e->c;
    const int H = c.hidden, D = c.head_dim, QKV = (c.n_heads + 2 * c.n_kv_heads) * D, A = c.n_heads * D, I = c.inter;
    vz_trainer* tr = new vz_trainer();
    tr->e = e;
    auto fail = [&](int r) { vz_train_destroy(tr); return r; };
    for (int i = 0; i < c.n_layers; ++i) {
        const LlmLayerW& W = e->llm[i];
        bf16_t *a = nullptr, *b = nullptr, *g = nullptr, *d = nullptr;
        if (hipMalloc((void**)&a, (size_t)H * QKV * 2) != hipSuccess || hipMalloc((void**)&b, (size_t)A * H * 2) != hipSuccess ||
            hipMalloc((void**)&g, (size_t)H * 2 * I * 2) != hipSuccess || hipMalloc((void**)&d, (size_t)I * H * 2) != hipSuccess) {
            vz_set_error("train_create: out of memory for the transposed Zephyr weights");
            return fail(VZ_ERR_HIP);
        }
        tr->t_qkv.push_back(a); tr->t_o.push_back(b); tr->t_gu.push_back(g); tr->t_down.push_back(d);
        int r = transpose2d(W.qkv.w, QKV, H, a, QKV, s);
        if (!r) r = transpose2d(W.o.w, H, A, b, H, s);
        if (!r) r = transpose2d(W.gu.w, 2 * I, H, g, 2 * I, s);
        if (!r) r = transpose2d(W.down.w, H, I, d, H, s);
        if (r) return fail(r);
    }
    tr->Vpad = pad64(c.vocab);
    if (hipMalloc((void**)&tr->t_lm, (size_t)H * tr->Vpad * 2) != hipSuccess) { vz_set_error("train_create: out of memory"); return fail(VZ_ERR_HIP); }
    (void)hipMemsetAsync(tr->t_lm, 0, (size_t)H * tr->Vpad * 2, s);
    { int r = transpose2d(e->top.lm_head.w, c.vocab, H, tr->t_lm, tr->Vpad, s); if (r) return fail(r); }
    // projector tensors in a fixed order (sorted names): the flat arenas follow it
    std::vector<std::string> names;
    for (auto& kv : e->w) if (kv.first.rfind("qf.", 0) == 0) names.push_back(kv.first);
    std::sort(names.begin(), names.end());
    size_t off = 0;
    for (auto& n : names) {
        const Weight& w = e->w[n];
        tr->index[n] = (int)tr->params.size();
        tr->params.push_back(ProjParam{n, w.dtype, w.n, off, const_cast<void*>(w.p)});
        off += (size_t)((w.n + 63) & ~63L);
    }
    tr->total = off;
    for (float** p : {&tr->master, &tr->m, &tr->v, &tr->grad}) {
        if (hipMalloc((void**)p, off * sizeof(float)) != hipSuccess) { vz_set_error("train_create: out of memory for the optimiser arenas"); return fail(VZ_ERR_HIP); }
        (void)hipMemsetAsync(*p, 0, off * sizeof(float), s);
    }
    { int r = bind_grads(tr); if (r) return fail(r); }
    for (auto& pp : tr->params) {       // master <- working copy (exact for fp32 vectors; matrices: see vz_train_set_master)
        if (pp.dtype == 1) (void)hipMemcpyAsync(tr->master + pp.off, pp.work, pp.n * sizeof(float), hipMemcpyDeviceToDevice, s);
        else {
            // bf16 -> fp32 by a widening copy: reuse the AdamW kernel's inverse is overkill; a one-off tiny kernel is not worth a symbol,
            // so go through the host-independent path: f32_to_bf16's counterpart is a plain shift, done by vz_launch_bf16_to_f32 below
            int r = vz_launch_bf16_to_f32((const bf16_t*)pp.work, tr->master + pp.off, pp.n, s);
            if (r) return fail(r);
        }
    }
    *out = tr;
    return VZ_OK;
}

// fp32 master of one projector tensor from the caller's fp32 values (a checkpoint's fp32 weights / the oracle's): the working copy
// keeps its rounded value, the optimiser continues from the exact one.  Engine tensor names ("qf.3.ffn1.w"); n elements, device pointer.
extern "C" int vz_train_set_master(vz_trainer* tr, const char* name, const float* d_values, long n, vz_stream stream) {
    VZ_CHECK_ARG(tr && name && d_values, "train_set_master: bad argument");
    auto it = tr->index.find(name);
    VZ_CHECK_ARG(it != tr->index.end() && tr->params[it->second].n == n, "train_set_master: no projector tensor '%s' of %ld elements", name, n);
    const ProjParam& pp = tr->params[it->second];
    VZ_CHECK_HIP(hipMemcpyAsync(tr->master + pp.off, d_values, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    // a LoRA factor's working copy is the trainer's own: it follows the master at once (RNE, as vz_train_adamw_step writes it)
    if (tr->lora.first >= 0 && it->second >= tr->lora.first) RC(vz_launch_f32_to_bf16(tr->master + pp.off, (bf16_t*)pp.work, n, (hipStream_t)stream));
    return VZ_OK;
}

// ---- Stage-2 LoRA (ref:vis_zephyr/train/train.py:224-243 find_all_linear_names, :933-951 LoraConfig; ref:script/finetune.sh) ----
// Every decoder linear gets an adapter: y = W x + scaling * B (A dropout(x)), A [r, in], B [out, r], scaling = alpha / r, dropout p
// per module (peft's Linear.forward).  The factors join the parameter table AFTER the projector tensors - Stage-1 offsets, names and
// results stay as they were - as lora.{layer}.{q,k,v,o,gate,up,down}.{A,B}, with fp32 master / moments / gradient in the same flat
// arenas (so zero_grad / allreduce / adamw cover them) and a bf16 working copy owned here.  Masters start at zero (the branch adds
// exactly nothing); the host writes peft's initial values (or a saved adapter) through vz_train_set_master.
static void lora_dims(const vz_config& c, int mod, int* in, int* out) {
    const int H = c.hidden, D = c.head_dim, A = c.n_heads * D, KV = c.n_kv_heads * D, I = c.inter;
    static const int ins[LORA_MODS] = {0, 0, 0, 1, 0, 0, 2};
    const int in_dims[3] = {H, A, I};
    const int out_dims[LORA_MODS] = {A, KV, KV, H, I, I, H};
    *in = in_dims[ins[mod]]; *out = out_dims[mod];
}

extern "C" int vz_train_lora_enable(vz_trainer* tr, int r, float alpha, float dropout, unsigned long long seed, vz_stream stream) {
    VZ_CHECK_ARG(tr && tr->e, "train_lora_enable: null trainer");
    VZ_CHECK_ARG(tr->lora.r == 0, "train_lora_enable: LoRA is already enabled on this trainer");
    VZ_CHECK_ARG(r >= 64 && r % 64 == 0 && alpha > 0.f && dropout >= 0.f && dropout < 1.f,
                 "train_lora_enable: r=%d (a multiple of 64: the rank is a GEMM contraction), alpha=%g, dropout=%g in [0, 1)", r, (double)alpha, (double)dropout);
    hipStream_t s = (hipStream_t)stream;
    const vz_config& c = tr->e->c;
    const size_t old_total = tr->total;
    size_t off = old_total, woff = 0;
    std::vector<ProjParam> add;
    std::vector<size_t> wo;
    for (int i = 0; i < c.n_layers; ++i)
        for (int mod = 0; mod < LORA_MODS; ++mod) {
            int in, out;
            lora_dims(c, mod, &in, &out);
            for (int ab = 0; ab < 2; ++ab) {
                const long n = (long)r * (ab == 0 ? in : out);
                add.push_back(ProjParam{"lora." + std::to_string(i) + "." + LORA_MOD_NAMES[mod] + (ab == 0 ? ".A" : ".B"), 0, n, off, nullptr});
                wo.push_back(woff);
                off += (size_t)((n + 63) & ~63L); woff += (size_t)((n + 63) & ~63L);
            }
        }
    bf16_t* work = nullptr;
    float* fresh[4] = {nullptr, nullptr, nullptr, nullptr};
    auto release = [&]() {
        if (work) (void)hipFree(work);
        for (float* p : fresh) if (p) (void)hipFree(p);
    };
    bool ok = hipMalloc((void**)&work, woff * sizeof(bf16_t)) == hipSuccess;
    for (int k = 0; k < 4 && ok; ++k) ok = hipMalloc((void**)&fresh[k], off * sizeof(float)) == hipSuccess;
    if (!ok) {
        release();
        vz_set_error("train_lora_enable: out of memory for %zu MiB of LoRA arenas", (off - old_total) * 16 >> 20);
        return VZ_ERR_HIP;
    }
    float** arenas[4] = {&tr->master, &tr->m, &tr->v, &tr->grad};
    hipError_t he = hipSuccess;
    for (int k = 0; k < 4 && he == hipSuccess; ++k) {
        he = hipMemcpyAsync(fresh[k], *arenas[k], old_total * sizeof(float), hipMemcpyDeviceToDevice, s);
        if (he == hipSuccess) he = hipMemsetAsync(fresh[k] + old_total, 0, (off - old_total) * sizeof(float), s);
    }
    if (he == hipSuccess) he = hipMemsetAsync(work, 0, woff * sizeof(bf16_t), s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he != hipSuccess) {             // the trainer keeps its Stage-1 arenas; nothing of the new ones survives
        (void)hipStreamSynchronize(s);
        release();
        vz_set_error("train_lora_enable: %s", hipGetErrorString(he));
        return VZ_ERR_HIP;
    }
    for (int k = 0; k < 4; ++k) { (void)hipFree(*arenas[k]); *arenas[k] = fresh[k]; }
    RC(bind_grads(tr));                 // the projector tensors keep their offsets in the new gradient arena
    tr->lora.first = (int)tr->params.size();
    for (size_t k = 0; k < add.size(); ++k) {
        add[k].work = work + wo[k];
        tr->index[add[k].name] = (int)tr->params.size();
        tr->params.push_back(add[k]);
    }
    tr->total = off;
    tr->lora.work = work; tr->lora.r = r; tr->lora.alpha = alpha; tr->lora.p = dropout; tr->lora.scaling = alpha / (float)r; tr->lora.seed = seed;
    return VZ_OK;
}

// dropout counter of the following micro-batches: the optimiser step, the index of the micro-batch's first sample within the optimiser
// batch, and the row stride of the counter (>= every micro-batch's S: the longest spliced row of the optimiser batch)
extern "C" int vz_train_lora_set_counter(vz_trainer* tr, int optimiser_step, long sample_base, long row_stride) {
    VZ_CHECK_ARG(tr && tr->lora.r > 0, "train_lora_set_counter: LoRA is not enabled");
    VZ_CHECK_ARG(optimiser_step >= 0 && sample_base >= 0 && row_stride >= 1, "train_lora_set_counter: bad argument");
    tr->lora.step = optimiser_step; tr->lora.sample_base = sample_base; tr->lora.row_stride = row_stride;
    return VZ_OK;
}

// tensor table for the host: count, then per index name / element count / offset into the flat arenas
extern "C" int vz_train_param_count(vz_trainer* tr) { return tr ? (int)tr->params.size() : 0; }
extern "C" int vz_train_param_info(vz_trainer* tr, int i, const char** name, long* n, long* offset, int* is_matrix) {
    VZ_CHECK_ARG(tr && i >= 0 && i < (int)tr->params.size() && name && n && offset && is_matrix, "train_param_info: bad argument");
    *name = tr->params[i].name.c_str(); *n = tr->params[i].n; *offset = (long)tr->params[i].off; *is_matrix = tr->params[i].dtype == 0;
    return VZ_OK;
}
// device pointers of the flat fp32 arenas (gradient, master, m, v) and their length in floats
extern "C" int vz_train_arenas(vz_trainer* tr, float** grad, float** master, float** m, float** v, long* total) {
    VZ_CHECK_ARG(tr, "train_arenas: null trainer");
    if (grad) *grad = tr->grad; if (master) *master = tr->master; if (m) *m = tr->m; if (v) *v = tr->v; if (total) *total = (long)tr->total;
    return VZ_OK;
}

// ---- the step's memory ------------------------------------------------------------------------------------------------------
// Everything a step touches is carved from the trainer's one arena by the step's own code, which runs twice per call (run_step): first
// as a sizing pass over a null-based Carver, with every launch and every host-to-device effect skipped (RUN / `if (cx.dry)`), then for
// real.  The sizing pass's high-water mark is the arena's need; after the real pass the two marks must agree.  So no size is written
// twice, and no branch of the step may depend on the arena's capacity (both passes must take the same branches).
// The one rule of the layout: the saved activations come first (carve_saved); a phase's buffers start where the saved activations end
// (phase_begin); a helper's scratch starts where its caller's buffers end, and is released when the helper returns (Frame).
#define RUN(expr) do { if (!cx.dry) RC(expr); } while (0)
#define RUN_AS(klass, expr) do { if (!cx.dry) { ProfScope ps_(cx.e, klass, cx.s); RC(expr); } } while (0)

struct Frame {
    Carver& m; const size_t mark;
    explicit Frame(Carver& c) : m(c), mark(c.off) {}
    ~Frame() { m.off = mark; }
};

struct Blk { bf16_t *x_in, *y1, *qkv, *att_s, *x_a, *y2, *qc, *ckv, *att_c, *x_b, *y3, *ffh, *ff; };
struct Lay { bf16_t *x_in, *y, *qrot, *att, *x_mid, *y2, *gu, *act; };
struct TrainPlan {
    bf16_t* lora_u;         // Stage 2: u = drop(x) A^T of every adapted module, [layer][module][B*S, r]
    bf16_t *feats, *fn, *x0, *y0, *kv0, *q0, *a0, *xs, *x_fin, *proj, *emb, *x_last, *y_last, *dlogits;
    bf16_t* demb;           // d(inputs_embeds) [B*S, H]: what the Zephyr backward hands to the projector backward
    float* logits; int* tile_map; int* zero_map; int* seq;
    std::vector<Blk> blk; std::vector<Lay> lay;
    bf16_t *kc, *vc;        // K/V of the micro-batch, cache layout [layer][B][Hkv][S][D]
    size_t scratch_off;
};

// one micro-batch: the caller's arguments, the dimensions, the arena cursor and the saved activations
struct Step {
    vz_trainer* tr; vz_engine* e; hipStream_t s;
    const void* d_images; const bf16_t* d_text; const int *h_tile_sample, *d_kind, *d_idx, *d_vis_rows, *h_seqlens, *d_pos, *d_labels; float inv_n;
    int T, n_samples, Lmax, B, S;
    int H, D, Hq, Hkv, QKV, I, A, V, NQ, KD, FF, NB, L, QH, QD, Pv, N0, lr;
    long R, TP, rows, R0, RS; size_t kvl;
    float qscale, lscale;
    bool dry; Carver m{nullptr, 0};
    TrainPlan pl;
    int* d_slot() const { return pl.seq; }
    int* d_len() const { return pl.seq + rows; }
    void phase_begin() { m.off = pl.scratch_off; }
};

static void carve_saved(Step& cx) {
    TrainPlan& pl = cx.pl; Carver& m = cx.m;
    const long R = cx.R, TP = cx.TP, rows = cx.rows, R0 = cx.R0, RS = cx.RS;
    const int H = cx.H, KD = cx.KD, FF = cx.FF, A = cx.A, I = cx.I;
    pl.feats = m.take<bf16_t>(TP * KD); pl.fn = m.take<bf16_t>(TP * KD);
    pl.x0 = m.take<bf16_t>(R0 * H); pl.y0 = m.take<bf16_t>(R0 * H); pl.kv0 = m.take<bf16_t>(R0 * 2 * H); pl.q0 = m.take<bf16_t>((size_t)cx.NQ * H);
    pl.a0 = m.take<bf16_t>(RS * H); pl.xs = m.take<bf16_t>(RS * H);
    pl.blk.assign(cx.NB, Blk());
    for (Blk& b : pl.blk) {
        b.x_in = m.take<bf16_t>(R * H); b.y1 = m.take<bf16_t>(R * H); b.qkv = m.take<bf16_t>(R * 3 * H); b.att_s = m.take<bf16_t>(R * H);
        b.x_a = m.take<bf16_t>(R * H); b.y2 = m.take<bf16_t>(R * H); b.qc = m.take<bf16_t>(R * H); b.ckv = m.take<bf16_t>(TP * 2 * H);
        b.att_c = m.take<bf16_t>(R * H); b.x_b = m.take<bf16_t>(R * H); b.y3 = m.take<bf16_t>(R * H); b.ffh = m.take<bf16_t>(R * FF); b.ff = m.take<bf16_t>(R * FF);
    }
    pl.x_fin = m.take<bf16_t>(R * H); pl.proj = m.take<bf16_t>(R * H); pl.emb = m.take<bf16_t>(rows * H);
    pl.lay.assign(cx.L, Lay());
    for (Lay& l : pl.lay) {
        l.x_in = m.take<bf16_t>(rows * H); l.y = m.take<bf16_t>(rows * H); l.qrot = m.take<bf16_t>(rows * A); l.att = m.take<bf16_t>(rows * A);
        l.x_mid = m.take<bf16_t>(rows * H); l.y2 = m.take<bf16_t>(rows * H); l.gu = m.take<bf16_t>(rows * 2 * I); l.act = m.take<bf16_t>(rows * I);
    }
    pl.kc = m.take<bf16_t>(cx.L * cx.kvl); pl.vc = m.take<bf16_t>(cx.L * cx.kvl);
    pl.x_last = m.take<bf16_t>(rows * H); pl.y_last = m.take<bf16_t>(rows * H);
    pl.logits = m.take<float>(rows * cx.V); pl.dlogits = m.take<bf16_t>(rows * cx.tr->Vpad);
    pl.demb = m.take<bf16_t>(rows * H);
    pl.lora_u = cx.lr ? m.take<bf16_t>((size_t)cx.L * LORA_MODS * rows * cx.lr) : nullptr;
    pl.tile_map = m.take<int>(cx.T + 16); pl.zero_map = m.take<int>(cx.n_samples + 16); pl.seq = m.take<int>(rows + cx.B + 16);
    pl.scratch_off = m.off;
}

// ---- attention: the step's five stride set-ups come from two layouts ----------------------------------------------------------
// packed rows: q / o (and dO / dq) [B, S, Hq*D]; K / V (and dK / dV) in the cache layout [B, Hkv, S, D] - the Zephyr layers, forward and backward
template <typename Args> static void packed_strides(Args& a, int S, int Hq, int Hkv, int D) {
    a.q_bs = a.o_bs = (long)S * Hq * D; a.q_ss = a.o_ss = (long)Hq * D; a.q_hs = a.o_hs = D;
    a.k_bs = a.v_bs = (long)Hkv * S * D; a.k_ss = a.v_ss = D; a.k_hs = a.v_hs = (long)S * D;
}
static AttnBwdArgs attn_bwd_packed(const bf16_t* q, const bf16_t* k, const bf16_t* v, const bf16_t* dO, bf16_t* dq, float* dk, float* dv, int B, int S,
                                   int Hq, int Hkv, int D, float scale, int window, const int* kv_len) {
    AttnBwdArgs a;
    a.q = q; a.k = k; a.v = v; a.dO = dO; a.B = B; a.Sq = a.Sk = S; a.Hq = Hq; a.Hkv = Hkv; a.D = D;
    packed_strides(a, S, Hq, Hkv, D);
    a.scale = scale; a.causal = 1; a.window = window; a.kv_len = kv_len;
    a.dq = dq; a.dq_bs = a.q_bs; a.dq_ss = a.q_ss; a.dq_hs = a.q_hs;
    a.dk = dk; a.dv = dv; a.dkv_fp32 = 1; a.dk_bs = a.k_bs; a.dk_ss = a.k_ss; a.dk_hs = a.k_hs;
    return a;
}
// interleaved rows (the Q-Former): head h of a row is its columns h*D.. in a row-major buffer of leading dimension ld (H, 2H or 3H: q, k | v
// or q | k | v column blocks of one projection); sample b starts S * ld further.  A gradient is laid out like its primal, dO like the
// attention output [B, Sq, Hq*D].
static AttnBwdArgs attn_bwd_rows(const bf16_t* q, int ldq, const bf16_t* k, const bf16_t* v, int ldkv, const bf16_t* dO, bf16_t* dq, bf16_t* dk,
                                 bf16_t* dv, int B, int Sq, int Sk, int Hq, int D, float scale) {
    AttnBwdArgs a;
    a.q = q; a.k = k; a.v = v; a.dO = dO; a.B = B; a.Sq = Sq; a.Sk = Sk; a.Hq = a.Hkv = Hq; a.D = D;
    a.q_bs = (long)Sq * ldq; a.q_ss = ldq; a.k_bs = a.v_bs = (long)Sk * ldkv; a.k_ss = a.v_ss = ldkv; a.o_bs = (long)Sq * Hq * D; a.o_ss = (long)Hq * D;
    a.q_hs = a.k_hs = a.v_hs = a.o_hs = D;
    a.scale = scale; a.causal = 0; a.window = 0; a.kv_len = nullptr;
    a.dq = dq; a.dq_bs = a.q_bs; a.dq_ss = a.q_ss; a.dq_hs = D;
    a.dk = dk; a.dv = dv; a.dkv_fp32 = 0; a.dk_bs = a.k_bs; a.dk_ss = a.k_ss; a.dk_hs = D;
    return a;
}

// ---- attention backward ---------------------------------------------------------------------------------------------------
// head_dim 128 (the Zephyr layers): the tile-resident form of attn_bwd_flash.hip - no S x S tensor in memory, the whole batch in two launches.
// Otherwise (the Q-Former's head_dim 512; vz_tune_set(32, 0)) by batched tile GEMMs (train.hip header).  That route RECOMPUTES the
// probabilities from Q and K (nothing of the forward's attention is kept), but a call materialises S, P and dS of all the (sample, head) pairs
// it is given: 8 bytes x B x Hq x Sq x Sk.  At the Stage-1 shape (S = 199, 16 samples) that is 160 MB; at the length the reference trains up to
// (ref:script/pretrain.sh:44 --model_max_length 2048) it would be 17 GB for the same 16 samples.  Samples are independent here, so the call
// walks the batch in groups whose scratch stays under ATTN_BWD_CAP: the scratch does not grow with the batch, and S = 2048 needs 1.1 GB per sample.
constexpr size_t ATTN_BWD_CAP = (size_t)1536 << 20;
struct AttnBwdWs { float* Sf; bf16_t *P, *dS, *Kt, *Xt, *Yt; };
static AttnBwdWs attn_bwd_carve(Carver& m, int B, const AttnBwdArgs& a) {
    const size_t Skp = pad64(a.Sk), Sqp = pad64(a.Sq), g = a.Hq / a.Hkv;
    AttnBwdWs w;
    w.Sf = m.take<float>((size_t)B * a.Hq * a.Sq * Skp);
    w.P = m.take<bf16_t>((size_t)B * a.Hq * a.Sq * Skp);
    w.dS = m.take<bf16_t>((size_t)B * a.Hq * a.Sq * Skp);
    w.Kt = m.take<bf16_t>((size_t)B * a.Hkv * a.D * Skp);            // K^T, later V is not needed transposed
    w.Xt = m.take<bf16_t>((size_t)B * a.Hkv * a.Sk * g * Sqp);       // dS^T, then P^T
    w.Yt = m.take<bf16_t>((size_t)B * a.Hkv * a.D * g * Sqp);        // Q^T, then dO^T
    return w;
}
static int attn_bwd_group(const Carver& at, const AttnBwdArgs& a) {       // samples per pass: the launcher's own carving, tried from where it will start
    for (int gB = a.B;; gB = (gB + 1) / 2) {
        Carver probe = at;
        attn_bwd_carve(probe, gB, a);
        if (gB == 1 || probe.off - at.off <= ATTN_BWD_CAP) return gB;
    }
}
static int attn_bwd_one(Step& cx, const AttnBwdArgs& a) {
    vz_engine* e = cx.e; hipStream_t s = cx.s;
    const int B = a.B, Sq = a.Sq, Sk = a.Sk, Hq = a.Hq, Hkv = a.Hkv, D = a.D, g = Hq / Hkv;
    const int Skp = pad64(Sk), Sqp = pad64(Sq);
    Frame fr(cx.m);
    const AttnBwdWs w = attn_bwd_carve(cx.m, B, a);
    if (cx.dry) return VZ_OK;
    float* Sf = w.Sf; bf16_t *P = w.P, *dS = w.dS, *Kt = w.Kt, *Xt = w.Xt, *Yt = w.Yt;
    ProfScope ps(e, K_ATTN, s);
    const long rows = (long)B * Hq * Sq, blk = (long)Sq * Skp;
    BatchedGemmArgs b;
    // S = Q K^T (fp32)
    b.A = a.q; b.lda = (int)a.q_ss; b.W = a.k; b.ldw = (int)a.k_ss; b.C = Sf; b.ldc = Skp; b.M = Sq; b.N = Sk; b.K = D; b.out_fp32 = 1;
    b.n_outer = B; b.n_inner = Hq; b.a_div = 1; b.w_div = g; b.a_so = a.q_bs; b.a_si = a.q_hs; b.w_so = a.k_bs; b.w_si = a.k_hs; b.c_so = Hq * blk; b.c_si = blk;
    RC(vz_launch_gemm_batched(b, s));
    RC(vz_launch_softmax_fwd(Sf, Skp, P, Skp, rows, Hq, Sq, Sk, a.scale, a.causal, a.window, a.kv_len, s));
    // dP = dO V^T (fp32, over S's buffer), dS = P o (dP - rowsum(P o dP)) scale
    b.A = a.dO; b.lda = (int)a.o_ss; b.W = a.v; b.ldw = (int)a.v_ss; b.a_so = a.o_bs; b.a_si = a.o_hs; b.w_so = a.v_bs; b.w_si = a.v_hs;
    RC(vz_launch_gemm_batched(b, s));
    RC(vz_launch_softmax_bwd(P, Skp, Sf, Skp, dS, Skp, rows, Sk, a.scale, s));
    // dQ = dS K   ("W" = K^T [D, Skp])
    VZ_CHECK_HIP(hipMemsetAsync(Kt, 0, (size_t)B * Hkv * D * Skp * 2, s));
    RC(vz_launch_transpose(a.k, a.k_ss, a.k_bs, a.k_hs, Kt, Skp, (long)Hkv * D * Skp, (long)D * Skp, Sk, D, B, Hkv, 0, s));
    b.A = dS; b.lda = Skp; b.W = Kt; b.ldw = Skp; b.C = a.dq; b.ldc = (int)a.dq_ss; b.M = Sq; b.N = D; b.K = Skp; b.out_fp32 = 0;
    b.a_so = Hq * blk; b.a_si = blk; b.w_so = (long)Hkv * D * Skp; b.w_si = (long)D * Skp; b.c_so = a.dq_bs; b.c_si = a.dq_hs;
    RC(vz_launch_gemm_batched(b, s));
    // dK = sum over the g query heads of a KV head of dS_h^T Q_h: the heads are concatenated along the contraction
    const long xt_blk = (long)Sk * g * Sqp, yt_blk = (long)D * g * Sqp;
    auto stack = [&](const bf16_t* rowsrc, long r_bs, long r_hs, long r_ss, const bf16_t* mat) -> int {
        // Xt[(b,kvh)][sk][j*Sqp + sq] = mat[(b, kvh*g + j)][sq][sk];   Yt[(b,kvh)][d][j*Sqp + sq] = rowsrc[(b, sq, kvh*g + j)][d]
        VZ_CHECK_HIP(hipMemsetAsync(Xt, 0, (size_t)B * Hkv * xt_blk * 2, s));
        VZ_CHECK_HIP(hipMemsetAsync(Yt, 0, (size_t)B * Hkv * yt_blk * 2, s));
        for (int j = 0; j < g; ++j) {
            RC(vz_launch_transpose(mat + (size_t)j * blk, Skp, Hq * blk, g * blk, Xt, (long)g * Sqp, Hkv * xt_blk, xt_blk, Sq, Sk, B, Hkv, j * Sqp, s));
            RC(vz_launch_transpose(rowsrc + (size_t)j * r_hs, r_ss, r_bs, g * r_hs, Yt, (long)g * Sqp, Hkv * yt_blk, yt_blk, Sq, D, B, Hkv, j * Sqp, s));
        }
        return VZ_OK;
    };
    RC(stack(a.q, a.q_bs, a.q_hs, a.q_ss, dS));
    b.A = Xt; b.lda = g * Sqp; b.W = Yt; b.ldw = g * Sqp; b.C = a.dk; b.ldc = (int)a.dk_ss; b.M = Sk; b.N = D; b.K = g * Sqp; b.out_fp32 = a.dkv_fp32;
    b.n_outer = B; b.n_inner = Hkv; b.a_div = 1; b.w_div = 1; b.a_so = Hkv * xt_blk; b.a_si = xt_blk; b.w_so = Hkv * yt_blk; b.w_si = yt_blk;
    b.c_so = a.dk_bs; b.c_si = a.dk_hs;
    RC(vz_launch_gemm_batched(b, s));
    // dV = sum_h P_h^T dO_h
    RC(stack(a.dO, a.o_bs, a.o_hs, a.o_ss, P));
    b.C = a.dv;
    RC(vz_launch_gemm_batched(b, s));
    return VZ_OK;
}
static int attn_bwd(Step& cx, const AttnBwdArgs& a0) {
    if (vz_knob(VZ_KNOB_FLASH_BWD) && vz_flash_bwd_ok(a0)) {
        Frame fr(cx.m);
        const size_t bytes = vz_flash_bwd_scratch_bytes(a0.B, a0.Sq, a0.Hq);
        char* ws = cx.m.take<char>(bytes);
        RUN_AS(K_ATTN, vz_launch_flash_bwd(a0, ws, bytes, cx.s));
        return VZ_OK;
    }
    const int gB = attn_bwd_group(cx.m, a0);
    for (int b0 = 0; b0 < a0.B; b0 += gB) {
        AttnBwdArgs a = a0;
        a.B = std::min(gB, a0.B - b0);
        a.q += (size_t)b0 * a0.q_bs; a.k += (size_t)b0 * a0.k_bs; a.v += (size_t)b0 * a0.v_bs; a.dO += (size_t)b0 * a0.o_bs;
        a.dq += (size_t)b0 * a0.dq_bs;
        const size_t esz = a0.dkv_fp32 ? 4 : 2;
        a.dk = (char*)a0.dk + (size_t)b0 * a0.dk_bs * esz; a.dv = (char*)a0.dv + (size_t)b0 * a0.dk_bs * esz;
        if (a0.kv_len) a.kv_len = a0.kv_len + b0;
        RC(attn_bwd_one(cx, a));
    }
    return VZ_OK;
}

// dW[N,K] (+)= dY^T X  and  db[N] += colsum(dY):  dY [R,N] bf16 (ld ldy), X [R,K] bf16 (ld ldx)
static int weight_grad(Step& cx, const bf16_t* dY, int ldy, const bf16_t* X, int ldx, long R, int N, int K, float* dW, float* db, int splitk_hint = 0) {
    vz_engine* e = cx.e; hipStream_t s = cx.s;
    Frame fr(cx.m);
    const int Rp = pad64((int)R);
    bf16_t* dYt = cx.m.take<bf16_t>((size_t)N * Rp);
    bf16_t* Xt = cx.m.take<bf16_t>((size_t)K * Rp);
    float* tmp = cx.m.take<float>((size_t)N * K);
    float* part = cx.m.take<float>((size_t)vz_colsum_groups(R) * N);
    if (cx.dry) return VZ_OK;
    if (Rp != R) {
        VZ_CHECK_HIP(hipMemsetAsync(dYt, 0, (size_t)N * Rp * 2, s));
        VZ_CHECK_HIP(hipMemsetAsync(Xt, 0, (size_t)K * Rp * 2, s));
    }
    { ProfScope ps(e, K_OTHER, s);
      RC(vz_launch_transpose(dY, ldy, 0, 0, dYt, Rp, 0, 0, (int)R, N, 1, 1, 0, s));
      RC(vz_launch_transpose(X, ldx, 0, 0, Xt, Rp, 0, 0, (int)R, K, 1, 1, 0, s)); }
    RC(linear(e, 0, dYt, Rp, bare(Xt), Rp, tmp, K, N, K, Rp, nullptr, 0, VZ_ACT_NONE, 1, s, nullptr, 0.f, splitk_hint));
    { ProfScope ps(e, K_OTHER, s);
      RC(vz_launch_axpy_f32(dW, tmp, (long)N * K, s));
      if (db) RC(vz_launch_colsum(dY, ldy, R, N, part, db, s)); }
    return VZ_OK;
}

// dX[R,K] = dY[R,N] . W[N,K] (+ res): transposes the (trainable, so per-step) weight into scratch first
static int input_grad(Step& cx, const bf16_t* dY, int ldy, const bf16_t* W, long R, int N, int K, bf16_t* dX, int ldx, const bf16_t* res) {
    Frame fr(cx.m);
    bf16_t* Wt = cx.m.take<bf16_t>((size_t)K * N);
    RUN_AS(K_OTHER, transpose2d(W, N, K, Wt, N, cx.s));
    RUN(linear(cx.e, 0, dY, ldy, bare(Wt), N, dX, ldx, (int)R, K, N, res, ldx, VZ_ACT_NONE, 0, cx.s));
    return VZ_OK;
}

// ---- the LoRA branch of one adapted module (Stage 2) ----
// forward:  xd = drop(x) * scaling / (1 - p) (lora.hip, mask from the counter);  u = xd A^T [rows, r], kept;  y += u B^T (the GEMM's
//           residual epilogue, in place).  The scaling rides on xd, so neither GEMM needs a scale epilogue.
// backward: v = g B [rows, r];  dX += drop(v A) (same mask and factor);  dB += g^T u;  dA += v^T xd (xd rebuilt from the counter).
// Weight operands are the bf16 working copies; the backward's B^T / A^T are transposed into scratch per call (r x in, small).
static int lora_call(const vz_trainer* tr, int layer, int mod, const bf16_t* x, long ldx, bf16_t* out, long ldo, const bf16_t* res, int B, int S,
                     hipStream_t s) {
    const LoraState& lo = tr->lora;
    int in, outd;
    lora_dims(tr->e->c, mod, &in, &outd);
    ProfScope ps(tr->e, K_OTHER, s);
    return vz_launch_lora_dropout(x, ldx, out, ldo, res, ldo, B * S, in, S, lo.sample_base, lo.row_stride, layer * LORA_MODS + mod, lo.step, lo.seed,
                                  lo.p, lo.scaling, s);
}
// K-split of the LoRA contractions with N = r (x A^T, g B, dB = g^T u): a 128-column output has one column tile, so the dispatcher's own
// split (4 slices when M > 512) leaves half of the 256 CUs idle at 4096 rows; cut K until ~512 workgroups exist, keeping >= 8 K-tiles per slice
static int lora_splitk(int M, int N, int K) {
    const int tiles = ((M + 127) / 128) * ((N + 127) / 128), nk = K / 64;
    int sk = std::min(16, std::max(1, 512 / tiles));
    while (sk > 1 && nk / sk < 8) --sk;
    return sk;
}
static const ProjParam& lora_param(const vz_trainer* tr, int layer, int mod, int ab) { return tr->params[tr->lora.first + (layer * LORA_MODS + mod) * 2 + ab]; }

static int lora_fwd(Step& cx, int layer, int mod, const bf16_t* x, int ldx, bf16_t* y, int ldy) {
    vz_trainer* tr = cx.tr; vz_engine* e = cx.e; hipStream_t s = cx.s;
    const int r = cx.lr;
    const long rows = cx.rows;
    int in, out;
    lora_dims(e->c, mod, &in, &out);
    Frame fr(cx.m);
    bf16_t* xd = cx.m.take<bf16_t>(rows * in);
    if (cx.dry) return VZ_OK;
    bf16_t* u = cx.pl.lora_u + ((size_t)layer * LORA_MODS + mod) * rows * r;
    RC(lora_call(tr, layer, mod, x, ldx, xd, in, nullptr, cx.B, cx.S, s));
    RC(linear(e, 0, xd, in, bare((const bf16_t*)lora_param(tr, layer, mod, 0).work), in, u, r, (int)rows, r, in, nullptr, 0, VZ_ACT_NONE, 0, s,
              nullptr, 0.f, lora_splitk((int)rows, r, in)));
    return linear(e, 0, u, r, bare((const bf16_t*)lora_param(tr, layer, mod, 1).work), r, y, ldy, (int)rows, out, r, y, ldy, VZ_ACT_NONE, 0, s);
}

static int lora_bwd(Step& cx, int layer, int mod, const bf16_t* g, int ldg, const bf16_t* x, int ldx, bf16_t* dX, int lddx) {
    vz_trainer* tr = cx.tr; vz_engine* e = cx.e; hipStream_t s = cx.s;
    const int r = cx.lr, B = cx.B, S = cx.S;
    const long rows = cx.rows;
    int in, out;
    lora_dims(e->c, mod, &in, &out);
    const ProjParam &pa = lora_param(tr, layer, mod, 0), &pb = lora_param(tr, layer, mod, 1);
    const bf16_t* u = cx.pl.lora_u + ((size_t)layer * LORA_MODS + mod) * rows * r;
    Frame fr(cx.m);
    bf16_t* bt = cx.m.take<bf16_t>((size_t)r * out);
    bf16_t* at = cx.m.take<bf16_t>((size_t)in * r);
    bf16_t* v = cx.m.take<bf16_t>(rows * r);
    bf16_t* t = cx.m.take<bf16_t>(rows * in);                // v A, later xd
    if (!cx.dry) {
        ProfScope ps(e, K_OTHER, s);
        RC(transpose2d((const bf16_t*)pb.work, out, r, bt, out, s));
        RC(transpose2d((const bf16_t*)pa.work, r, in, at, r, s));
    }
    RUN(linear(e, 0, g, ldg, bare(bt), out, v, r, (int)rows, r, out, nullptr, 0, VZ_ACT_NONE, 0, s, nullptr, 0.f, lora_splitk((int)rows, r, out)));
    RUN(linear(e, 0, v, r, bare(at), r, t, in, (int)rows, in, r, nullptr, 0, VZ_ACT_NONE, 0, s));
    RUN(lora_call(tr, layer, mod, t, in, dX, lddx, dX, B, S, s));
    RC(weight_grad(cx, g, ldg, u, r, rows, out, r, tr->grad + pb.off, nullptr, lora_splitk(out, r, pad64((int)rows))));
    RUN(lora_call(tr, layer, mod, x, ldx, t, in, nullptr, B, S, s));
    return weight_grad(cx, v, r, t, in, rows, r, in, tr->grad + pa.off, nullptr);
}

// ---- the four phases of a step ------------------------------------------------------------------------------------------------
// small host tables -> device; K / V start as zeros
static int upload_tables(Step& cx) {
    if (cx.dry) return VZ_OK;
    vz_engine* e = cx.e; hipStream_t s = cx.s; const TrainPlan& pl = cx.pl;
    const int B = cx.B, S = cx.S; const long rows = cx.rows;
    RC(upload_ints(e, cx.h_tile_sample, cx.T, pl.tile_map, s));
    std::vector<int> q(rows + B);
    for (int b = 0; b < B; ++b) {
        for (int t = 0; t < S; ++t) q[(size_t)b * S + t] = t < cx.h_seqlens[b] ? t : -1;
        q[rows + b] = cx.h_seqlens[b];
    }
    RC(upload_ints(e, q.data(), q.size(), pl.seq, s));
    VZ_CHECK_HIP(hipMemsetAsync(pl.zero_map, 0, (cx.n_samples + 16) * sizeof(int), s));
    // padded positions are never written by the RoPE / append kernel; the backward GEMMs multiply them by exact zeros, so they must be finite
    VZ_CHECK_HIP(hipMemsetAsync(pl.kc, 0, cx.L * cx.kvl * 2, s));
    VZ_CHECK_HIP(hipMemsetAsync(pl.vc, 0, cx.L * cx.kvl * 2, s));
    return VZ_OK;
}

// block 0's self-attention: once per SAMPLE on the 32 query rows, keys / values over [queries ; text] (engine.hip's header)
static int block0_self_attn(Step& cx) {
    vz_engine* e = cx.e; hipStream_t s = cx.s; const TrainPlan& pl = cx.pl;
    const int H = cx.H, NQ = cx.NQ, N0 = cx.N0, Lmax = cx.Lmax;
    const bf16_t* queries = e->top.qf_queries;
    for (int sm = 0; sm < cx.n_samples; ++sm) {
        RUN(vz_launch_copy_rows(queries, H, pl.x0 + (size_t)sm * N0 * H, H, NQ, H, s));
        if (Lmax > 0) RUN(vz_launch_copy_rows(cx.d_text + (size_t)sm * Lmax * H, H, pl.x0 + ((size_t)sm * N0 + NQ) * H, H, Lmax, H, s));
        RUN(vz_launch_copy_rows(queries, H, pl.xs + (size_t)sm * NQ * H, H, NQ, H, s));
    }
    const QfBlockW& W = e->qf[0];
    RUN(vz_launch_layernorm(pl.x0, H, pl.y0, H, W.n1.w, W.n1.b, (int)cx.R0, H, e->c.qf_eps, s));
    RUN(linear(e, 0, pl.y0, H, lin_rows(W.sa_in, H, H), H, pl.kv0, 2 * H, (int)cx.R0, 2 * H, H, nullptr, 0, VZ_ACT_NONE, 0, s));
    RUN(linear(e, 0, pl.y0, H, W.sa_in, H, pl.q0, H, NQ, H, H, nullptr, 0, VZ_ACT_NONE, 0, s));
    RUN(qf_attn(e, pl.q0, 0, H, pl.kv0, pl.kv0 + H, (long)N0 * 2 * H, 2 * H, pl.a0, cx.n_samples, NQ, N0, s));
    RUN(linear(e, 0, pl.a0, H, W.sa_out, H, pl.xs, H, (int)cx.RS, H, H, pl.xs, H, VZ_ACT_NONE, 0, s));
    for (int t = 0; t < cx.T; ++t) RUN(vz_launch_copy_rows(pl.xs + (size_t)cx.h_tile_sample[t] * NQ * H, H, pl.blk[0].x_a + (size_t)t * NQ * H, H, NQ, H, s));
    return VZ_OK;
}

// tiles -> CLIP (no grad) -> fusion -> Q-Former, activations kept
static int projector_forward(Step& cx) {
    vz_engine* e = cx.e; hipStream_t s = cx.s; const vz_config& c = e->c; TrainPlan& pl = cx.pl;
    const int H = cx.H, NQ = cx.NQ, KD = cx.KD, FF = cx.FF, NB = cx.NB, Pv = cx.Pv, T = cx.T;
    const long R = cx.R, TP = cx.TP;
    RUN(vz_clip_fused_features(e, cx.d_images, T, pl.feats, nullptr, (vz_stream)s));
    RUN_AS(K_NORM, vz_launch_layernorm(pl.feats, KD, pl.fn, KD, e->top.qf_pre_norm.w, e->top.qf_pre_norm.b, (int)TP, KD, c.qf_eps, s));
    RC(block0_self_attn(cx));
    for (int i = 0; i < NB; ++i) {
        const QfBlockW& W = e->qf[i];
        Blk& b = pl.blk[i];
        if (i > 0) {
            RUN(vz_launch_layernorm(b.x_in, H, b.y1, H, W.n1.w, W.n1.b, (int)R, H, c.qf_eps, s));
            RUN(linear(e, 0, b.y1, H, W.sa_in, H, b.qkv, 3 * H, (int)R, 3 * H, H, nullptr, 0, VZ_ACT_NONE, 0, s));
            RUN(qf_attn(e, b.qkv, (long)NQ * 3 * H, 3 * H, b.qkv + H, b.qkv + 2 * H, (long)NQ * 3 * H, 3 * H, b.att_s, T, NQ, NQ, s));
            RUN(linear(e, 0, b.att_s, H, W.sa_out, H, b.x_a, H, (int)R, H, H, b.x_in, H, VZ_ACT_NONE, 0, s));
        }
        RUN(linear(e, 0, pl.fn, KD, W.ca_kv, KD, b.ckv, 2 * H, (int)TP, 2 * H, KD, nullptr, 0, VZ_ACT_NONE, 0, s));
        RUN(vz_launch_layernorm(b.x_a, H, b.y2, H, W.n2.w, W.n2.b, (int)R, H, c.qf_eps, s));
        RUN(linear(e, 0, b.y2, H, W.ca_q, H, b.qc, H, (int)R, H, H, nullptr, 0, VZ_ACT_NONE, 0, s));
        RUN(qf_attn(e, b.qc, (long)NQ * H, H, b.ckv, b.ckv + H, (long)Pv * 2 * H, 2 * H, b.att_c, T, NQ, Pv, s));
        RUN(linear(e, 0, b.att_c, H, W.ca_out, H, b.x_b, H, (int)R, H, H, b.x_a, H, VZ_ACT_NONE, 0, s));
        RUN(vz_launch_layernorm(b.x_b, H, b.y3, H, W.n3.w, W.n3.b, (int)R, H, c.qf_eps, s));
        RUN(linear(e, 0, b.y3, H, W.ffn1, H, b.ffh, FF, (int)R, FF, H, nullptr, 0, VZ_ACT_NONE, 0, s));
        RUN(vz_launch_gelu_fwd(b.ffh, b.ff, R * FF, s));
        bf16_t* x_next = i + 1 < NB ? pl.blk[i + 1].x_in : pl.x_fin;
        RUN(linear(e, 0, b.ff, FF, W.ffn2, FF, x_next, H, (int)R, H, FF, b.x_b, H, VZ_ACT_NONE, 0, s));
    }
    RUN(vz_launch_layernorm(pl.x_fin, H, pl.proj, H, e->top.qf_norm.w, e->top.qf_norm.b, (int)R, H, c.qf_eps, s));
    return VZ_OK;
}

// splice -> the frozen Zephyr layers (activations kept; Stage 2: + the LoRA branches) -> lm_head on every position -> shifted cross-entropy
static int zephyr_forward_loss(Step& cx) {
    vz_trainer* tr = cx.tr; vz_engine* e = cx.e; hipStream_t s = cx.s; const vz_config& c = e->c; TrainPlan& pl = cx.pl;
    const int H = cx.H, D = cx.D, Hq = cx.Hq, Hkv = cx.Hkv, QKV = cx.QKV, I = cx.I, A = cx.A, V = cx.V, L = cx.L, B = cx.B, S = cx.S, lr = cx.lr;
    const long rows = cx.rows;
    cx.phase_begin();
    bf16_t* qkv = cx.m.take<bf16_t>(rows * QKV);              // [rows, QKV] un-rotated projection of the layer at hand
    RUN(vz_embed_splice(e, cx.d_kind, cx.d_idx, (int)rows, pl.proj, pl.emb, (vz_stream)s));
    for (int i = 0; i < L; ++i) {
        const LlmLayerW& W = e->llm[i];
        Lay& l = pl.lay[i];
        if (i == 0) RUN(vz_launch_copy_rows(pl.emb, H, l.x_in, H, (int)rows, H, s));
        RUN(vz_launch_rmsnorm(l.x_in, H, l.y, H, W.in_norm, (int)rows, H, c.rms_eps, s));
        RUN(linear(e, 0, l.y, H, W.qkv, H, qkv, QKV, (int)rows, QKV, H, nullptr, 0, VZ_ACT_NONE, 0, s));
        if (lr) for (int mod = 0; mod < 3; ++mod) RC(lora_fwd(cx, i, mod, l.y, H, qkv + (mod == 0 ? 0 : mod == 1 ? A : A + Hkv * D), QKV));
        bf16_t* kc = pl.kc + (size_t)i * cx.kvl; bf16_t* vc = pl.vc + (size_t)i * cx.kvl;
        RUN(vz_launch_rope_kv(qkv, QKV, l.qrot, kc, vc, e->cosT, e->sinT, cx.d_pos, cx.d_slot(), B, S, Hq, Hkv, D, S, s));
        {
            AttnArgs a;
            a.q = l.qrot; a.k = kc; a.v = vc; a.o = l.att;
            a.B = B; a.Sq = S; a.Sk = S; a.Hq = Hq; a.Hkv = Hkv; a.head_dim = D;
            packed_strides(a, S, Hq, Hkv, D);
            a.scale = cx.lscale; a.causal = 1; a.q_pos0 = 0; a.window = c.sliding_window; a.kv_len = cx.d_len();
            RUN_AS(K_ATTN, vz_launch_attention(a, s));
        }
        RUN(linear(e, 0, l.att, A, W.o, A, l.x_mid, H, (int)rows, H, A, l.x_in, H, VZ_ACT_NONE, 0, s));
        if (lr) RC(lora_fwd(cx, i, 3, l.att, A, l.x_mid, H));
        RUN(vz_launch_rmsnorm(l.x_mid, H, l.y2, H, W.post_norm, (int)rows, H, c.rms_eps, s));
        // gate|up pre-activations are kept (SwiGLU backward needs both): N = 2I plain columns, then the SwiGLU as its own kernel
        RUN(linear(e, 0, l.y2, H, W.gu, H, l.gu, 2 * I, (int)rows, 2 * I, H, nullptr, 0, VZ_ACT_NONE, 0, s));
        if (lr) {
            // the fused output interleaves gate and up in 16-column groups: add the two branches on a [gate | up] copy, then put it back
            Frame fr(cx.m);
            bf16_t* z = cx.m.take<bf16_t>(rows * 2 * I);
            RUN_AS(K_OTHER, vz_launch_gu_permute(l.gu, z, rows, I, 1, s));
            RC(lora_fwd(cx, i, 4, l.y2, H, z, 2 * I));
            RC(lora_fwd(cx, i, 5, l.y2, H, z + I, 2 * I));
            RUN_AS(K_OTHER, vz_launch_gu_permute(z, l.gu, rows, I, 0, s));
        }
        RUN(vz_launch_swiglu_fwd(l.gu, l.act, rows, I, s));
        bf16_t* x_next = i + 1 < L ? pl.lay[i + 1].x_in : pl.x_last;
        RUN(linear(e, 0, l.act, I, W.down, I, x_next, H, (int)rows, H, I, l.x_mid, H, VZ_ACT_NONE, 0, s));
        if (lr) RC(lora_fwd(cx, i, 6, l.act, I, x_next, H));
    }
    RUN(vz_launch_rmsnorm(pl.x_last, H, pl.y_last, H, e->top.norm, (int)rows, H, c.rms_eps, s));
    RUN(linear(e, 0, pl.y_last, H, e->top.lm_head, H, pl.logits, V, (int)rows, V, H, nullptr, 0, VZ_ACT_NONE, 1, s));
    RUN(vz_launch_cross_entropy(pl.logits, V, cx.d_labels, rows, S, cx.inv_n, tr->d_loss_rows, pl.dlogits, tr->Vpad, s));
    if (!cx.dry) tr->loss_rows_n = rows;
    return VZ_OK;
}

// dlogits -> d(inputs_embeds) through the frozen Zephyr layers (input gradients only; Stage 2: + the LoRA factors' gradients)
static int zephyr_backward(Step& cx) {
    vz_trainer* tr = cx.tr; vz_engine* e = cx.e; hipStream_t s = cx.s; const vz_config& c = e->c; TrainPlan& pl = cx.pl; Carver& m = cx.m;
    const int H = cx.H, D = cx.D, Hq = cx.Hq, Hkv = cx.Hkv, QKV = cx.QKV, I = cx.I, A = cx.A, L = cx.L, B = cx.B, S = cx.S, lr = cx.lr;
    const long rows = cx.rows;
    cx.phase_begin();
    bf16_t* dx = pl.demb; bf16_t* dy = m.take<bf16_t>(rows * H); bf16_t* dx2 = m.take<bf16_t>(rows * H);
    bf16_t* datt = m.take<bf16_t>(rows * A); bf16_t* dact = m.take<bf16_t>(rows * I); bf16_t* dgu = m.take<bf16_t>(rows * 2 * I);
    bf16_t* dqkv = m.take<bf16_t>(rows * QKV); bf16_t* dq = m.take<bf16_t>(rows * A);
    float* dk = m.take<float>(cx.kvl); float* dv = m.take<float>(cx.kvl);
    RUN(linear(e, 0, pl.dlogits, tr->Vpad, bare(tr->t_lm), tr->Vpad, dy, H, (int)rows, H, tr->Vpad, nullptr, 0, VZ_ACT_NONE, 0, s));
    RUN(vz_launch_rmsnorm_bwd(pl.x_last, e->top.norm, dy, nullptr, dx, rows, H, c.rms_eps, s));
    for (int i = L - 1; i >= 0; --i) {
        const LlmLayerW& W = e->llm[i];
        Lay& l = pl.lay[i];
        // x_out = x_mid + down(act):  dact = dx . W_down
        RUN(linear(e, 0, dx, H, bare(tr->t_down[i]), H, dact, I, (int)rows, I, H, nullptr, 0, VZ_ACT_NONE, 0, s));
        if (lr) RC(lora_bwd(cx, i, 6, dx, H, l.act, I, dact, I));
        RUN(vz_launch_swiglu_bwd(l.gu, dact, dgu, rows, I, s));
        RUN(linear(e, 0, dgu, 2 * I, bare(tr->t_gu[i]), 2 * I, dy, H, (int)rows, H, 2 * I, nullptr, 0, VZ_ACT_NONE, 0, s));
        if (lr) {
            Frame fr(m);
            bf16_t* g = m.take<bf16_t>(rows * 2 * I);          // d(gate | up) in [gate | up] halves
            RUN_AS(K_OTHER, vz_launch_gu_permute(dgu, g, rows, I, 1, s));
            RC(lora_bwd(cx, i, 4, g, 2 * I, l.y2, H, dy, H));
            RC(lora_bwd(cx, i, 5, g + I, 2 * I, l.y2, H, dy, H));
        }
        RUN(vz_launch_rmsnorm_bwd(l.x_mid, W.post_norm, dy, dx, dx2, rows, H, c.rms_eps, s));       // dx2 = d x_mid
        // x_mid = x_in + o(att):  datt = dx2 . W_o
        RUN(linear(e, 0, dx2, H, bare(tr->t_o[i]), H, datt, A, (int)rows, A, H, nullptr, 0, VZ_ACT_NONE, 0, s));
        if (lr) RC(lora_bwd(cx, i, 3, dx2, H, l.att, A, datt, A));
        RC(attn_bwd(cx, attn_bwd_packed(l.qrot, pl.kc + (size_t)i * cx.kvl, pl.vc + (size_t)i * cx.kvl, datt, dq, dk, dv, B, S, Hq, Hkv, D, cx.lscale,
                                        c.sliding_window, cx.d_len())));
        RUN(vz_launch_rope_bwd_assemble(dq, dk, dv, dqkv, e->cosT, e->sinT, cx.d_pos, B, S, Hq, Hkv, D, S, s));
        RUN(linear(e, 0, dqkv, QKV, bare(tr->t_qkv[i]), QKV, dy, H, (int)rows, H, QKV, nullptr, 0, VZ_ACT_NONE, 0, s));
        if (lr) for (int mod = 0; mod < 3; ++mod) RC(lora_bwd(cx, i, mod, dqkv + (mod == 0 ? 0 : mod == 1 ? A : A + Hkv * D), QKV, l.y, H, dy, H));
        RUN(vz_launch_rmsnorm_bwd(l.x_in, W.in_norm, dy, dx2, dx, rows, H, c.rms_eps, s));          // dx = d x_in
    }
    return VZ_OK;
}

// the projector backward's own buffers
struct QfBwd {
    bf16_t *dxq, *dtmp, *dy, *datt, *dqc, *dproj, *dff, *dffh, *dqkv3, *dckv, *dfn;
    bf16_t *dkv0, *dy0, *dx0, *dxs, *da0, *dq0, *dq0sum;       // block 0's self-attention (per sample)
    float* lnpart;
};
static int ln_bwd(Step& cx, const QfBwd& q, const bf16_t* x, const NormW& w, const GradWB& g, const bf16_t* dy, const bf16_t* dres, bf16_t* dx, long nrows, int cols) {
    RUN_AS(K_NORM, vz_launch_layernorm_bwd(x, w.w, dy, dres, dx, q.lnpart, g.w, g.b, nrows, cols, cx.e->c.qf_eps, cx.s));
    return VZ_OK;
}

// backward of block0_self_attn, from q.dxq = d x_a of block 0 [R, H]: the gradient of a sample's rows is the sum over its tiles, and
// everything below is linear in that gradient
static int block0_self_attn_bwd(Step& cx, const QfBwd& q) {
    vz_trainer* tr = cx.tr; vz_engine* e = cx.e; hipStream_t s = cx.s; const TrainPlan& pl = cx.pl;
    const int H = cx.H, NQ = cx.NQ, N0 = cx.N0, n_samples = cx.n_samples;
    const long RS = cx.RS, R0 = cx.R0;
    const QfBlockW& W = e->qf[0];
    const QfBlockG& G = tr->g_qf[0];
    RUN_AS(K_OTHER, vz_launch_segment_sum_rows(q.dxq, pl.tile_map, cx.T, NQ, q.dxs, n_samples, H, s));
    RC(weight_grad(cx, q.dxs, H, pl.a0, H, RS, H, H, G.sa_out.w, G.sa_out.b));
    RC(input_grad(cx, q.dxs, H, W.sa_out.w, RS, H, H, q.da0, H, nullptr));
    AttnBwdArgs ab = attn_bwd_rows(pl.q0, H, pl.kv0, pl.kv0 + H, 2 * H, q.da0, q.dq0, q.dkv0, q.dkv0 + H, n_samples, NQ, N0, cx.QH, cx.QD, cx.qscale);
    ab.q_bs = 0;            // the query projection was computed once (rows 0..31 of sample 0 = LN1(queries), the same for every sample)
    RC(attn_bwd(cx, ab));
    RUN_AS(K_OTHER, vz_launch_segment_sum_rows(q.dq0, pl.zero_map, n_samples, NQ, q.dq0sum, 1, H, s));
    RC(weight_grad(cx, q.dq0sum, H, pl.y0, H, NQ, H, H, G.sa_in.w, G.sa_in.b));
    RC(weight_grad(cx, q.dkv0, 2 * H, pl.y0, H, R0, 2 * H, H, G.sa_in.w + (size_t)H * H, G.sa_in.b + H));
    RC(input_grad(cx, q.dkv0, 2 * H, W.sa_in.w + (size_t)H * H, R0, 2 * H, H, q.dy0, H, nullptr));
    RC(input_grad(cx, q.dq0sum, H, W.sa_in.w, NQ, H, H, q.dy0, H, q.dy0));           // + dq . Wq into the query rows of sample 0
    RC(ln_bwd(cx, q, pl.x0, W.n1, G.n1, q.dy0, nullptr, q.dx0, R0, H));
    // learned_queries: residual path of every sample (xs = queries + ...) + the query rows of every sample's [queries ; text]
    if (!cx.dry) {
        ProfScope ps(e, K_OTHER, s);
        RC(vz_launch_acc_rows_f32(tr->g_queries, q.dxs, n_samples, (long)NQ * H, NQ, H, s));
        RC(vz_launch_acc_rows_f32(tr->g_queries, q.dx0, n_samples, (long)N0 * H, NQ, H, s));
    }
    return VZ_OK;
}

// rows of d(inputs_embeds) that hold visual tokens -> Q-Former backward with all 165 parameter gradients
static int projector_backward(Step& cx) {
    vz_trainer* tr = cx.tr; vz_engine* e = cx.e; hipStream_t s = cx.s; TrainPlan& pl = cx.pl; Carver& m = cx.m;
    const int H = cx.H, NQ = cx.NQ, KD = cx.KD, FF = cx.FF, NB = cx.NB, QH = cx.QH, QD = cx.QD, Pv = cx.Pv, T = cx.T;
    const long R = cx.R, TP = cx.TP, R0 = cx.R0, RS = cx.RS;
    cx.phase_begin();
    QfBwd q;
    q.dxq = m.take<bf16_t>(R * H); q.dtmp = m.take<bf16_t>(R * H); q.dy = m.take<bf16_t>(R * H); q.datt = m.take<bf16_t>(R * H);
    q.dqc = m.take<bf16_t>(R * H); q.dproj = m.take<bf16_t>(R * H);
    q.dff = m.take<bf16_t>(R * FF); q.dffh = m.take<bf16_t>(R * FF); q.dqkv3 = m.take<bf16_t>(R * 3 * H);
    q.dckv = m.take<bf16_t>(TP * 2 * H); q.dfn = m.take<bf16_t>(TP * KD);
    q.dkv0 = m.take<bf16_t>(R0 * 2 * H); q.dy0 = m.take<bf16_t>(R0 * H); q.dx0 = m.take<bf16_t>(R0 * H);
    q.dxs = m.take<bf16_t>(RS * H); q.da0 = m.take<bf16_t>(RS * H); q.dq0 = m.take<bf16_t>(RS * H); q.dq0sum = m.take<bf16_t>((size_t)NQ * H);
    q.lnpart = m.take<float>(std::max(vz_layernorm_bwd_scratch_floats(TP, KD), vz_layernorm_bwd_scratch_floats(std::max(R, R0), H)));
    RUN_AS(K_OTHER, vz_launch_gather_rows_idx(pl.demb, cx.d_vis_rows, q.dproj, R, H, s));
    RC(ln_bwd(cx, q, pl.x_fin, e->top.qf_norm, tr->g_norm, q.dproj, nullptr, q.dxq, R, H));
    bool have_dfn = false;
    for (int i = NB - 1; i >= 0; --i) {
        const QfBlockW& W = e->qf[i];
        const QfBlockG& G = tr->g_qf[i];
        Blk& b = pl.blk[i];
        // FFN
        RC(weight_grad(cx, q.dxq, H, b.ff, FF, R, H, FF, G.ffn2.w, G.ffn2.b));
        RC(input_grad(cx, q.dxq, H, W.ffn2.w, R, H, FF, q.dff, FF, nullptr));
        RUN_AS(K_OTHER, vz_launch_gelu_bwd(b.ffh, q.dff, q.dffh, R * FF, s));
        RC(weight_grad(cx, q.dffh, FF, b.y3, H, R, FF, H, G.ffn1.w, G.ffn1.b));
        RC(input_grad(cx, q.dffh, FF, W.ffn1.w, R, FF, H, q.dy, H, nullptr));
        RC(ln_bwd(cx, q, b.x_b, W.n3, G.n3, q.dy, q.dxq, q.dtmp, R, H));
        std::swap(q.dxq, q.dtmp);                               // dxq = d x_b
        // cross-attention
        RC(weight_grad(cx, q.dxq, H, b.att_c, H, R, H, H, G.ca_out.w, G.ca_out.b));
        RC(input_grad(cx, q.dxq, H, W.ca_out.w, R, H, H, q.datt, H, nullptr));
        RC(attn_bwd(cx, attn_bwd_rows(b.qc, H, b.ckv, b.ckv + H, 2 * H, q.datt, q.dqc, q.dckv, q.dckv + H, T, NQ, Pv, QH, QD, cx.qscale)));
        RC(weight_grad(cx, q.dqc, H, b.y2, H, R, H, H, G.ca_q.w, G.ca_q.b));
        RC(input_grad(cx, q.dqc, H, W.ca_q.w, R, H, H, q.dy, H, nullptr));
        RC(weight_grad(cx, q.dckv, 2 * H, pl.fn, KD, TP, 2 * H, KD, G.ca_kv.w, G.ca_kv.b));
        RC(input_grad(cx, q.dckv, 2 * H, W.ca_kv.w, TP, 2 * H, KD, q.dfn, KD, have_dfn ? q.dfn : nullptr));
        have_dfn = true;
        RC(ln_bwd(cx, q, b.x_a, W.n2, G.n2, q.dy, q.dxq, q.dtmp, R, H));
        std::swap(q.dxq, q.dtmp);                               // dxq = d x_a
        if (i == 0) { RC(block0_self_attn_bwd(cx, q)); break; }
        RC(weight_grad(cx, q.dxq, H, b.att_s, H, R, H, H, G.sa_out.w, G.sa_out.b));
        RC(input_grad(cx, q.dxq, H, W.sa_out.w, R, H, H, q.datt, H, nullptr));
        RC(attn_bwd(cx, attn_bwd_rows(b.qkv, 3 * H, b.qkv + H, b.qkv + 2 * H, 3 * H, q.datt, q.dqkv3, q.dqkv3 + H, q.dqkv3 + 2 * H, T, NQ, NQ, QH, QD, cx.qscale)));
        RC(weight_grad(cx, q.dqkv3, 3 * H, b.y1, H, R, 3 * H, H, G.sa_in.w, G.sa_in.b));
        RC(input_grad(cx, q.dqkv3, 3 * H, W.sa_in.w, R, 3 * H, H, q.dy, H, nullptr));
        RC(ln_bwd(cx, q, b.x_in, W.n1, G.n1, q.dy, q.dxq, q.dtmp, R, H));
        std::swap(q.dxq, q.dtmp);                               // dxq = d x_in = d(output of block i - 1)
    }
    // pre_norm (LayerNorm 5120 of the fused visual features): parameter gradients only - the features are constants (CLIP runs under no_grad)
    return ln_bwd(cx, q, pl.feats, e->top.qf_pre_norm, tr->g_pre_norm, q.dfn, nullptr, nullptr, TP, KD);
}

// the step's body: once to size the arena (cx.dry), once for real
static int run_step(Step& cx) {
    carve_saved(cx);
    RC(upload_tables(cx));
    RC(projector_forward(cx));
    RC(zephyr_forward_loss(cx));
    RC(zephyr_backward(cx));
    return projector_backward(cx);
}

// Accumulates the gradients of ONE micro-batch into the trainer's gradient arena and the micro-batch's row losses (x inv_n) into
// the loss buffer.  Inputs as the inference stages take them: d_images bf16 [T,3,336,336]; d_text bf16 [n_samples,Lmax,H] +
// h_tile_sample[T] (vz_qformer); d_kind / d_idx int32 [B*S] row map of the splice (vz_embed_splice; kind 1 rows = visual token idx);
// d_vis_rows int32 [T*32]: the row of [B*S] that visual token (tile, query) was spliced into, -1 if it was cut off;
// h_seqlens[B], d_pos int32 [B,S] (vz_llm_prefill); d_labels int32 [B,S] (HF labels, -100 = ignore; the shift by one happens
// here); inv_n = 1 / (valid targets of the WHOLE batch, all micro-batches and ranks).
extern "C" int vz_train_stage1_accumulate(vz_trainer* tr, const void* d_images, int T, const void* d_text, int n_samples, int Lmax,
                                          const int* h_tile_sample, const int* d_kind, const int* d_idx, const int* d_vis_rows, int B, int S,
                                          const int* h_seqlens, const int* d_pos, const int* d_labels, float inv_n, vz_stream stream) {
    VZ_CHECK_ARG(tr && tr->e, "train: null trainer");
    vz_engine* e = tr->e;
    NEED_READY();
    const vz_config& c = e->c;
    VZ_CHECK_ARG(d_images && d_kind && d_idx && d_vis_rows && h_tile_sample && h_seqlens && d_pos && d_labels && T >= 1 && B >= 1 && S >= 2 && n_samples >= 1 &&
                 n_samples <= T && Lmax >= 0 && (Lmax == 0 || d_text), "train: bad argument");
    VZ_CHECK_ARG(e->cosT && e->rope_max >= S, "train: rotary tables shorter than S");
    for (int t = 0; t < T; ++t) VZ_CHECK_ARG(h_tile_sample[t] >= 0 && h_tile_sample[t] < n_samples, "train: tile_sample[%d] out of range", t);
    for (int b = 0; b < B; ++b) VZ_CHECK_ARG(h_seqlens[b] >= 1 && h_seqlens[b] <= S, "train: seqlen[%d]=%d outside [1,%d]", b, h_seqlens[b], S);
    const LoraState& lo = tr->lora;
    VZ_CHECK_ARG(!lo.r || lo.row_stride >= S, "train: LoRA dropout row stride %ld < S=%d (vz_train_lora_set_counter)", lo.row_stride, S);

    Step cx;
    cx.tr = tr; cx.e = e; cx.s = (hipStream_t)stream;
    cx.d_images = d_images; cx.d_text = (const bf16_t*)d_text; cx.h_tile_sample = h_tile_sample; cx.d_kind = d_kind; cx.d_idx = d_idx; cx.d_vis_rows = d_vis_rows;
    cx.h_seqlens = h_seqlens; cx.d_pos = d_pos; cx.d_labels = d_labels; cx.inv_n = inv_n;
    cx.T = T; cx.n_samples = n_samples; cx.Lmax = Lmax; cx.B = B; cx.S = S;
    cx.H = c.hidden; cx.D = c.head_dim; cx.Hq = c.n_heads; cx.Hkv = c.n_kv_heads; cx.QKV = (cx.Hq + 2 * cx.Hkv) * cx.D; cx.I = c.inter; cx.A = cx.Hq * cx.D; cx.V = c.vocab;
    cx.NQ = c.qf_queries; cx.KD = c.qf_kv_dim; cx.FF = 2 * cx.H; cx.NB = c.qf_blocks; cx.L = c.n_layers; cx.QH = c.qf_heads; cx.QD = cx.H / cx.QH;
    cx.Pv = (c.clip_image / c.clip_patch) * (c.clip_image / c.clip_patch) + (c.clip_keep_cls ? 1 : 0);
    cx.N0 = cx.NQ + Lmax; cx.lr = lo.r;
    cx.R = (long)T * cx.NQ; cx.TP = (long)T * cx.Pv; cx.rows = (long)B * S; cx.R0 = (long)n_samples * cx.N0; cx.RS = (long)n_samples * cx.NQ;
    cx.kvl = (size_t)B * cx.Hkv * S * cx.D;
    cx.qscale = 1.0f / sqrtf((float)cx.QD); cx.lscale = 1.0f / sqrtf((float)cx.D);

    // sizing: the step itself over a null arena; its high-water mark is the need
    cx.dry = true; cx.m = Carver(nullptr, ~(size_t)0);
    RC(run_step(cx));
    const size_t need = cx.m.peak;
    if (need > tr->ws_bytes) {
        if (tr->ws) { VZ_CHECK_HIP(hipDeviceSynchronize()); VZ_CHECK_HIP(hipFree(tr->ws)); tr->ws = nullptr; tr->ws_bytes = 0; }
        if (hipMalloc((void**)&tr->ws, need) != hipSuccess) { vz_set_error("train: cannot allocate %zu MiB of activations + scratch (use smaller micro-batches)", need >> 20); return VZ_ERR_HIP; }
        tr->ws_bytes = need;
    }
    if ((size_t)cx.rows > tr->loss_rows_cap) {
        if (tr->d_loss_rows) { VZ_CHECK_HIP(hipDeviceSynchronize()); VZ_CHECK_HIP(hipFree(tr->d_loss_rows)); tr->d_loss_rows = nullptr; tr->loss_rows_cap = 0; }
        VZ_CHECK_HIP(hipMalloc((void**)&tr->d_loss_rows, cx.rows * sizeof(float)));
        tr->loss_rows_cap = cx.rows;
    }
    cx.dry = false; cx.m = Carver(tr->ws, tr->ws_bytes);
    RC(run_step(cx));
    tr->ws_peak = cx.m.peak;
    if (cx.m.peak != need) { vz_set_error("train: the step took %zu bytes of the arena, its sizing pass %zu (internal sizing error)", cx.m.peak, need); return VZ_ERR_STATE; }
    return VZ_OK;
}

// the arena's size and the high-water mark of the last step in it (equal when that step sized the arena)
extern "C" int vz_train_ws_info(vz_trainer* tr, size_t* arena_bytes, size_t* peak_bytes) {
    VZ_CHECK_ARG(tr && arena_bytes && peak_bytes, "train_ws_info: bad argument");
    *arena_bytes = tr->ws_bytes; *peak_bytes = tr->ws_peak;
    return VZ_OK;
}

// sum over the rows of the last micro-batch of (logsumexp - target logit): the caller multiplies by inv_n and adds micro-batches
extern "C" int vz_train_loss_sum(vz_trainer* tr, double* out, vz_stream stream) {
    VZ_CHECK_ARG(tr && out, "train_loss_sum: bad argument");
    std::vector<float> h(tr->loss_rows_n);
    VZ_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (tr->loss_rows_n) VZ_CHECK_HIP(hipMemcpy(h.data(), tr->d_loss_rows, h.size() * sizeof(float), hipMemcpyDeviceToHost));
    double s2 = 0;
    for (float v : h) s2 += v;
    *out = s2;
    return VZ_OK;
}

extern "C" int vz_train_zero_grad(vz_trainer* tr, vz_stream stream) {
    VZ_CHECK_ARG(tr, "train_zero_grad: null trainer");
    VZ_CHECK_HIP(hipMemsetAsync(tr->grad, 0, tr->total * sizeof(float), (hipStream_t)stream));
    return VZ_OK;
}

// Data parallelism over RCCL (the reference: DeepSpeed ZeRO-2, ref:script/pretrain.sh:7 - every rank back-propagates the MEAN loss of
// its own batch, the gradients are AVERAGED across ranks, every rank applies the same update): one communicator per trainer, the flat
// fp32 gradient arena all-reduced with ncclAvg in 256 MiB buckets.  (Round 2 summed: world x the reference's gradient.)
extern "C" int vz_train_comm_init(vz_trainer* tr, const char* id128, int rank, int world) {
    VZ_CHECK_ARG(tr && id128 && world >= 1 && rank >= 0 && rank < world, "train_comm_init: bad argument");
    if (tr->dp_comm) return VZ_OK;
    ncclUniqueId id;
    memcpy(&id, id128, 128);
    ncclResult_t r = ncclCommInitRank(&tr->dp_comm, world, id, rank);
    if (r != ncclSuccess) { tr->dp_comm = nullptr; vz_set_error("ncclCommInitRank failed: %s", ncclGetErrorString(r)); return VZ_ERR_HIP; }
    tr->dp_world = world;
    return VZ_OK;
}
extern "C" int vz_train_allreduce(vz_trainer* tr, vz_stream stream) {
    VZ_CHECK_ARG(tr, "train_allreduce: null trainer");
    if (!tr->dp_comm) return VZ_OK;
    const size_t bucket = (size_t)64 << 20;      // floats
    ProfScope ps(tr->e, K_COMM, (hipStream_t)stream);
    for (size_t o = 0; o < tr->total; o += bucket) {
        const size_t n = std::min(bucket, tr->total - o);
        ncclResult_t r = ncclAllReduce(tr->grad + o, tr->grad + o, n, ncclFloat, ncclAvg, tr->dp_comm, (hipStream_t)stream);
        if (r != ncclSuccess) { vz_set_error("ncclAllReduce failed: %s", ncclGetErrorString(r)); return VZ_ERR_HIP; }
    }
    return VZ_OK;
}

// torch.optim.AdamW on every projector tensor (fp32 master / moments), writing the engine's working copies and clearing the gradients
extern "C" int vz_train_adamw_step(vz_trainer* tr, float lr, float beta1, float beta2, float eps, float weight_decay, vz_stream stream) {
    VZ_CHECK_ARG(tr && lr >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps > 0.f, "train_adamw: bad argument");
    hipStream_t s = (hipStream_t)stream;
    RC(drop_decode_graph(tr->e));               // the weights a captured decode graph reads are about to change (same pointers, new values: harmless, but keep the rule simple)
    const int t = ++tr->adam_t;
    ProfScope ps(tr->e, K_OTHER, s);
    for (auto& pp : tr->params)
        RC(vz_launch_adamw(tr->master + pp.off, tr->m + pp.off, tr->v + pp.off, tr->grad + pp.off, pp.work, pp.dtype == 0, pp.n, lr, beta1, beta2, eps, weight_decay, t, s));
    return VZ_OK;
}
