// The tune knobs of vz_tune_set / vz_tune_get / vz_tune_info: ONE table of numbers, names, defaults and accepted ranges, one int array
// behind it, one reader (vz_knob).  Host code only.  The numbers are ABI (bench.py, profiles/ and DESIGN.md refer to them) and never
// change; include/viszephyr.h lists `number  name  meaning` in the order of this table (tests/test_tune_cpu.py compares the two).
#pragma once

// X(number, IDENT, name, default, lowest, highest, meaning).  A range is what the knob's read sites can take: an enumeration's values,
// 0 / 1 for a switch, and for a count the bound the reader itself applies.
#define VZ_KNOBS(X) \
    X(0, GEMV_VARIANT, gemv_variant, 0, 0, 10, "GEMV variant: 0 = production choice; 1..10 = alternatives compiled in (rows per wave, chunks in flight, non-temporal loads, waves per workgroup; tools/bench_kernels.py)") \
    X(1, GEMM_CHOICE, gemm_choice, 0, 0, 2, "tile GEMM choice: 0 = by grid size; 1 = always 128^2; 2 = always 256^2") \
    X(2, ATTN_VERSION, attn_version, 3, 1, 3, "prefill attention generation: 1 = v1 kernel for every head_dim (tests / A-B); 2 = v2 (head_dim 64 / 128) with the classic online-softmax step; 3 = v2 with the deferred-maximum step (production)") \
    X(3, SPLITK_MODE, splitk_mode, 0, 0, 1, "split-K of M <= 512 linears: 0 = auto; 1 = never") \
    X(4, GEMM256_STREAMK, gemm256_streamk, 1, 0, 2, "256^2 GEMM stream-K tail: 1 = a last round that fills at most half of the CUs; 0 = whole tiles only; 2 = forced for any tail (tests)") \
    /* the skew applies to stream-K workgroups of >= 24 units: 12 leaves the short (odd) ones half of theirs */ \
    X(5, GEMM256_SKEW, gemm256_skew, 2, 0, 12, "K-tiles by which even / odd stream-K workgroups lead / lag") \
    X(6, GEMM256_STAMPS, gemm256_stamps, 0, 0, 1, "record 256^2 GEMM phase stamps (vz_prof_gemm_stamps)") \
    X(7, FORCE_COMM, force_comm, 0, 0, 2, "1 = route the collectives of a tp_size == 1 engine holding a one-rank communicator through RCCL (self-test); 2 = shape rehearsal of one rank of a tp_size > 1 engine, collectives skipped") \
    X(9, SKINNY_MODE, skinny_mode, 1, 0, 7, "2..64-row linears, SkinnyMode of linear_route.h: 1 = MFMA weight stream; 0 = GEMV / tile GEMM; 5 = ignore the tiled weight copies") \
    X(10, ATTN_NSPLIT, attn_nsplit, 0, 0, 64, "context splits of the fused decode attention: 0 = engine default") \
    X(11, GEMM256_DRAIN, gemm256_drain, 0, 0, 1, "256^2 GEMM workgroups wait for their stores before ending (experiment)") \
    /* measured cross-over on the tiled weight copies (profiles/r02_rows.txt): MFMA weight stream 4.42 ms per step at 25 rows, 4.74 at 32; \
       tile route 4.56 / 4.64 */ \
    X(14, DECODE_TILE_ROWS, decode_tile_rows, 29, 1, 65, "rows from which a decode step's linears take the 128^2 tile GEMM (65 = never)") \
    /* 0 = no hint; the launch lowers the factor until a slice keeps 4 K-tiles, and 16 is the most vz_decode_splitk gives any projection */ \
    X(15, DECODE_SK_SHORT, decode_sk_short, 8, 0, 16, "split-K factor of the K = 4096 decode projections (QKV, O) on that route") \
    X(16, ATTN_STAMPS, attn_stamps, 0, 0, 1, "record stage stamps of the prefill attention kernel (vz_prof_attn_stamps)") \
    X(19, WIDE_MODE, wide_mode, 1, 0, 1, "gemm_wide.hip for 17..64-row decode steps: 0 = off (they keep the earlier routes)") \
    X(21, FP8_GEMM_CHOICE, fp8_gemm_choice, 0, 0, 2, "fp8 tile GEMM choice: 0 = by grid size; 1 = always the 128^2 kernel; 2 = always the 256^2 pipeline") \
    X(22, FP8_PREFILL_MIN_ROWS, fp8_prefill_min_rows, 768, 0, 0x7fffffff, "fewest prefill rows that take the fp8 MFMA path of a prefill_fp8 engine") \
    /* split512 (attention.hip) takes at most 1024 splits */ \
    X(23, ATTN_SPLIT, attn_split, 0, 0, 1024, "key split of few-row head_dim-512 attention: 0 = automatic (every 96 keys); 1 = never; n >= 2 = n splits") \
    /* 4 -> 8: Q-Former 3.87 -> 3.80 ms.  The one knob whose setter CLAMPS a value outside its range instead of refusing it (the tools' sweeps rely on it) */ \
    X(24, SPLITK_CAP, splitk_cap, 8, 1, 16, "most K slices of a weight-streaming (M <= 512) linear; values outside 1..16 are clamped") \
    X(25, QF_KV_ALL, qf_kv_all, 1, 0, 1, "Q-Former cross-attention K|V projections of all blocks as one GEMM: 0 = one block at a time (A/B)") \
    X(26, SPLITK_MID, splitk_mid, 1, 0, 1, "K slices for tile-GEMM grids that leave a CU one workgroup (M > 512, < 256 tiles): 0 = whole-K tiles (batch-invariant)") \
    /* taken only where it divides the K chunks into an even count per split (gemm_wide.hip); K = 14336 has 112 chunks */ \
    X(27, WIDE_FP8_SPLITS, wide_fp8_splits, 0, 0, 64, "K splits of the e4m3 17..64-row stream: 0 = by shape (A/B)") \
    /* off by default: measured 282 vs 339 tok/s (profiles/r03_persist_stamps.txt: the phase edges + the attention phase leave HBM idle longer than the \
       launch boundaries they replace) */ \
    X(28, PERSIST_DECODE, persist_decode, 0, 0, 1, "batch-1 decode steps as ONE resident grid per token (decode_persist.hip) instead of the launch chain") \
    X(29, ONESHOT, oneshot, 1, 0, 1, "one-shot all-reduce for the TP decode step when peer areas are attached: 0 = keep RCCL") \
    X(30, ATTN_O, attn_o, 1, 0, 1, "batch-1 decode attention + O projection as one launch (attn_o_fused.hip): 0 = two launches") \
    /* scan at ctx 2048 with the two-trip head, two runs each: 0 -> 372.5-372.7, 4 -> 375.4-377.4, 8 -> 376.5-377.0, 12 -> 373.0-373.6, \
       16 -> 368.8-370.0 tok/s; against the four-trip head it was 12: 0 -> 344, 8 -> 346, 12 -> 357, 16 -> 352, 24 -> 348.  The units are \
       spent in a loop of s_sleep 8: 64 (~13 us, a whole fused launch) bounds it */ \
    X(31, ATTN_O_DELAY, attn_o_delay, 8, 0, 64, "that launch's O role waits n x ~0.21 us before requesting its weights, so that the attention blocks' K / V loads reach the memory system first") \
    X(32, FLASH_BWD, flash_bwd, 1, 0, 1, "training step: tile-resident attention backward for head_dim 128; 0 = the materialising batched-GEMM route (A/B)") \
    X(33, ROPE_IN_ATTN, rope_in_attn, 1, 0, 1, "prefill: RoPE of the queries inside the attention's Q load; 0 = a rotated copy of Q from rope_kv_kernel (bit-identical)") \
    X(34, GEMM256_PERSIST, gemm256_persist, 1, 0, 1, "256^2 GEMM: persistent whole-tile workgroups when a launch has more whole tiles than CUs; 0 = one workgroup per tile (bit-identical)") \
    X(35, SKINNY_EVEN, skinny_even, 1, 0, 1, "3..16-row persistent weight stream: the same number of row groups on every workgroup; 0 = one workgroup per CU (bit-identical)") \
    /* measured behind 2048 cached positions (profiles/append.txt): the key-split kernel + combine take 48 us against 67 at T = 256, 61 against 68 \
       at 320, 76 against 71 at 384 and 87 against 74 at 512: the crossover lies between 320 and 384, and 256 sits inside the range it wins by a \
       clear margin */ \
    X(36, APPEND_FLASH_MIN_T, append_flash_min_t, 256, 0, 0x7fffffff, "append prefill: more new rows per sample than this run on the prefill's flash kernel, fewer on the key-split kernel of attn_append.hip")

enum VzKnob {
#define X(num, id, name, dflt, lo, hi, doc) VZ_KNOB_##id = num,
    VZ_KNOBS(X)
#undef X
    VZ_KNOB_SLOTS = 37        // array length: the highest number + 1 (8, 12, 13, 17, 18 and 20 are numbers no knob has)
};

struct VzKnobValues { int v[VZ_KNOB_SLOTS]; };
extern VzKnobValues g_vz_knobs;      // tune.hip; written by vz_tune_set alone
inline int vz_knob(VzKnob k) { return g_vz_knobs.v[k]; }

// successful vz_tune_set calls so far: a captured decode step froze the routes the knobs chose, so it is part of the graph key
unsigned vz_tune_epoch();
