#!/usr/bin/env python
"""Which kernel runs which linear: a sweep over every route the linear dispatch can take, for comparing two builds.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o sweep -- python tools/route_sweep.py run --log LOG.json
    python tools/route_sweep.py summarise DIR/**/sweep_kernel_trace.csv LOG.json > SUMMARY.txt
    python tools/route_sweep.py golden    DIR/**/sweep_kernel_trace.csv LOG.json > tests/golden/linear_routes.json
    python tools/route_sweep.py diff SUMMARY_A.txt SUMMARY_B.txt
    python tools/route_sweep.py run --dry --log LOG.json      (no GPU: only the case list)
    python tools/route_sweep.py oracle grid                   (no GPU: tools/route_oracle.hip, the dispatch code from before the planner,
                                                               against the planner over its whole grid)
    python tools/route_sweep.py oracle golden LOG.json > tests/golden/linear_routes.json      (the same table from that code's answers)

`run` (MI355X) drives
  * a 2-layer full-width synth engine through EAGER decode steps at 1..64 rows - bf16 with tiled weight copies, bf16 without, e4m3 with
    tiled e4m3 copies - under the default knobs and under knob 9 in {0, 2, 3, 5, 7}, knob 19 = 0, knob 14 in {8, 17, 65}; prefill at
    199 / 512 / 2048 positions; the vision stage at 1 and 5 tiles;
  * the op-level entry points (linear_tiled, linear_tiled_fp8, linear_rmsnorm, linear_fp8, linear_impl 0..4) over the shape grids of
    tests/test_ops_gpu.py,
and writes LOG.json: per case the linears it issued (shape, flags of vz_op_linear_route, knobs) and a sha256 of every output.  Every case
starts with a marker launch: a one-row RMSNorm over 64 columns, i.e. a single workgroup of the generic `norm_kernel<true>`.  The sweep's
own RMSNorms are 4096 columns wide and take `norm_rows_kernel`, so no other launch looks like it - an engine of another hidden size with
1-row steps would, and the tool then stops with a count mismatch.  A kernel trace of the run is cut into cases at the markers.
On a shared GPU give every run its own limit: `timeout -k 10 540 rocprofv3 ... -- python tools/route_sweep.py run ...`.

`summarise` prints, per case, the linear-family launches (kernel, grid, workgroup, LDS) in order, a sha256 over ALL launches of the case
and the output digests; two builds route alike iff their summaries are equal (`diff`).  `golden` maps each linear of the log to the
route its kernel belongs to: the table tests/test_linear_route_cpu.py pins vz_op_linear_route against."""
import csv
import hashlib
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# flags / entries of vz_op_linear_route (include/viszephyr.h)
F_WT, F_W8, F_W8T, F_NORM, F_BIAS, F_RES, F_DECODE = 1, 2, 4, 8, 16, 32, 64
E_ENGINE, E_LINEAR, E_RMSNORM, E_TILED, E_TILED_FP8, E_IMPL0 = 0, 1, 2, 3, 4, 8

ROWS = (1, 2, 3, 4, 5, 8, 12, 16, 17, 24, 28, 29, 32, 33, 48, 64)
ROUTE_KNOBS = (9, 14, 19)      # skinny_mode, decode_tile_rows, wide_mode: what the planner reads; every case sets all three
KNOB_SETS = [{}] + [{9: v} for v in (0, 2, 3, 5, 7)] + [{19: 0}] + [{14: v} for v in (8, 17, 65)]

# kernel name -> route name of csrc/linear_route.h (splitk_finalize_kernel belongs to the TILE128 launch before it)
ROUTE_OF_KERNEL = [("gemv_bf16_kernel", "GEMV"), ("gemv_bf16_noepi_kernel", "GEMV"), ("skinny_persist_kernel", "SKINNY_PERSIST"), ("skinny_wide_kernel", "SKINNY_WIDE"),
                   ("skinny_kernel", "SKINNY"), ("wide_tiled_fp8_kernel", "WIDE_E4M3"), ("wide_tiled_kernel", "WIDE_BF16"),
                   ("gemm256_bf16_kernel", "TILE256"), ("gemm_bf16_kernel", "TILE128")]


def route_of(kernel_name):
    for key, route in ROUTE_OF_KERNEL:
        if re.search(r"\b" + key + r"\b", kernel_name):
            return route
    return None


def lin(name, M, N, K, act=0, out_fp32=0, flags=0, entry=E_ENGINE, ldw=None):
    return {"name": name, "M": M, "N": N, "K": K, "lda": K, "ldw": K if ldw is None else ldw, "act": act, "out_fp32": out_fp32,
            "flags": flags, "entry": entry}


# ------------------------------------------------------------------------------------------------------------------------------------
# run
# ------------------------------------------------------------------------------------------------------------------------------------
def run(log_path, quick, dry=False):
    """dry: only enumerate the cases and their linears into the log (no GPU, nothing launched)"""
    sys.path.insert(0, os.path.join(REPO, "vision-zephyr_amd"))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    from vz_hip import binding as B
    from vz_hip import quant, synth
    from vz_hip.engine import Engine
    B.load_library()
    dev = "cuda:0"
    cases = []
    base = {k: B.tune_get(k) for k in ROUTE_KNOBS}          # the values the sweep starts from: a case's knobs are these but for what it names
    if not dry:
        mark_x = torch.ones(1, 64, dtype=torch.bfloat16, device=dev)
        mark_w = torch.ones(64, dtype=torch.float32, device=dev)

    def sha(t):
        return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()

    def begin(label, knobs, linears):
        for k, v in {**base, **knobs}.items():
            B.tune(k, v)
        case = {"id": len(cases), "label": label, "knobs": {str(k): v for k, v in {**base, **knobs}.items()}, "named": sorted(knobs),
                "linears": linears, "digests": {}}
        cases.append(case)
        if not dry:
            B.rmsnorm(mark_x, mark_w, 1e-5)          # the marker launch
        return case

    def rnd(shape, std, seed, dtype=torch.bfloat16):
        if dry:
            return None
        g = torch.Generator(device=dev).manual_seed(seed)
        return (torch.randn(*shape, generator=g, device=dev) * std).to(dtype)

    # ---- engine sweep ----
    cfg = synth.ArchConfig(n_layers=2)
    H, I, V, QKV = cfg.hidden, cfg.inter, cfg.vocab, (cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim
    engines = [("bf16-tiled", False, "1", F_WT), ("bf16-plain", False, "0", 0), ("e4m3-tiled", True, "1", F_W8 | F_W8T)]
    S0 = 24
    for ename, fp8, tiled, wflags in engines[:1] if quick else engines:
        os.environ["VZ_DECODE_TILED"] = tiled
        eng = None if dry else Engine(cfg, device=dev, max_batch=64, max_ctx=2176, max_tiles=5, max_text=64, weight_fp8=fp8)
        if eng:
            eng.load_synthetic(0)
            eng.finalize()
            ids = torch.stack([synth.synth_ids(S0 + 1, V, image_pos=-1, seed=500 + b) for b in range(64)])
            emb = eng.embed_tokens(ids[:, :S0])
            eng.prefill(emb, [S0] * 64, all_logits=False, last_logits=True)
            first = ids[:, S0].to(torch.int32)

        def step_linears(M):
            d = wflags | F_DECODE
            layer = [lin("qkv", M, QKV, H, flags=d | F_NORM), lin("o", M, H, H, flags=d | F_RES),
                     lin("gate_up", M, 2 * I, H, act=3, flags=d | F_NORM), lin("down", M, H, I, flags=d | F_RES)]
            return layer * cfg.n_layers + [lin("lm_head", M, V, H, out_fp32=1, flags=d | F_NORM)]

        for knobs in KNOB_SETS[:2] if quick else KNOB_SETS:
            for M in ROWS:
                case = begin(f"decode {ename} rows={M}", knobs, step_linears(M))
                if dry:
                    continue
                eng.decode_begin(first[:M], [S0] * M, [S0] * M)
                try:
                    toks, lg = eng.decode_steps(1, return_logits=True)          # (debug logits = an eager step, never a graph replay)
                    case["digests"] = {"ids": sha(toks), "logits": sha(lg)}
                except ValueError as ex:          # (knob 9 = 0 above 8 rows: no kernel fuses the norm - the step stops at that linear)
                    case["digests"] = {"step": "rejected: " + str(ex)}
                eng.check_async()
        for S in (199,) if quick else (199, 512, 2048):
            # prefill: every Zephyr linear is a non-decode caller on the bf16 matrix; the last-position lm_head (1 row) may stream the e4m3 copy
            layer = [lin("qkv", S, QKV, H), lin("o", S, H, H, flags=F_RES), lin("gate_up", S, 2 * I, H, act=3), lin("down", S, H, I, flags=F_RES)]
            case = begin(f"prefill {ename} S={S}", {}, layer * cfg.n_layers + [lin("lm_head", 1, V, H, out_fp32=1, flags=F_W8 if fp8 else 0)])
            if dry:
                continue
            pids = synth.synth_ids(S, V, image_pos=-1, seed=900 + S).unsqueeze(0)
            _, last = eng.prefill(eng.embed_tokens(pids), [S], all_logits=False, last_logits=True)
            case["digests"] = {"last_logits": sha(last)}
        for T in (1,) if quick else (1, 5):
            C, CI, P, NQ, KD, FF, nb = cfg.clip_hidden, cfg.clip_inter, cfg.clip_patches, cfg.qf_queries, cfg.qf_kv_dim, cfg.qf_ffn, cfg.qf_blocks
            rows, R, bias = T * cfg.clip_tokens, T * NQ, F_BIAS
            clip = [lin("clip.patch", T * P, C, 640)]
            for _ in range(cfg.clip_layers):
                clip += [lin("clip.qkv", rows, 3 * C, C, flags=bias), lin("clip.o", rows, C, C, flags=bias | F_RES),
                         lin("clip.fc1", rows, CI, C, act=1, flags=bias), lin("clip.fc2", rows, C, CI, flags=bias | F_RES)]
            case = begin(f"clip {ename} tiles={T}", {}, clip)
            feats = None if dry else eng.clip_fused_features(synth.synth_tiles(T, seed=1).to(dev))
            case["digests"] = {} if dry else {"features": sha(feats)}
            qf = [lin("qf0.sa_kv", NQ, 2 * H, H, flags=bias), lin("qf0.sa_q", NQ, H, H, flags=bias), lin("qf0.sa_out", NQ, H, H, flags=bias | F_RES)]
            for i in range(nb):
                if i > 0:
                    qf += [lin("qf.sa_in", R, 3 * H, H, flags=bias), lin("qf.sa_out", R, H, H, flags=bias | F_RES)]
                if i == 0:
                    qf += [lin("qf.ca_kv_all", T * P, nb * 2 * H, KD, flags=bias)]
                qf += [lin("qf.ca_q", R, H, H, flags=bias), lin("qf.ca_out", R, H, H, flags=bias | F_RES),
                       lin("qf.ffn1", R, FF, H, act=2, flags=bias), lin("qf.ffn2", R, H, FF, flags=bias | F_RES)]
            case = begin(f"qformer {ename} tiles={T}", {}, qf)
            if not dry:
                case["digests"] = {"queries": sha(eng.qformer(feats, None, [0] * T))}
        if eng:
            eng.check_async()
            eng.close()
            del eng
            torch.cuda.empty_cache()

    # ---- op-level sweep: the grids tests/test_ops_gpu.py uses ----
    import test_ops_gpu as T_

    def grid(fn):
        return [m for m in fn.pytestmark if m.name == "parametrize"][0].args[1]

    def op(case, name, fn):
        if dry:
            return
        try:
            case["digests"][name] = sha(fn())
        except (ValueError, NotImplementedError, B.VzError) as ex:
            case["digests"][name] = "rejected: " + str(ex)

    def operands(M, N, K, act, seed):
        n_out = N // 2 if act == 3 else N
        nw = rnd((K,), 0.2, seed + 4, torch.float32)
        return (rnd((M, K), 1.0, seed), rnd((N, K), K ** -0.5, seed + 1), rnd((M, n_out), 0.5, seed + 2),
                None if act == 3 else (True if dry else rnd((N,), 0.1, seed + 3, torch.float32)), nw if dry else nw + 1.0)

    tiled = [(g, {19: 0}) for g in grid(T_.test_skinny_tiled_weights_bit_identical)] + [(g + (False,), {}) for g in grid(T_.test_wide_tiled_gemm)]
    for (M, N, K, act, norm), knobs in tiled[:3] if quick else tiled:
        x, w, res, bias, nw = operands(M, N, K, act, 11)
        wt = None if dry else B.tile_weights(w)
        use_norm = norm and M <= 16
        fl = F_WT | F_RES | (F_NORM if use_norm else 0) | (F_BIAS if bias is not None and not use_norm else 0)
        case = begin(f"linear_tiled {M}x{N}x{K} act{act} norm{int(use_norm)}", knobs, [lin("op", M, N, K, act=act, out_fp32=1, flags=fl, entry=E_TILED)])
        op(case, "out", lambda: B.linear_tiled(x, w, wt, bias=None if use_norm else bias, residual=res, act=act, out_fp32=True,
                                                norm_w=nw if use_norm else None, norm_eps=1e-5))
    for M, N, K, act in grid(T_.test_wide_tiled_gemm_fp8)[:2 if quick else None]:
        x, w, res, bias, nw = operands(M, N, K, act, 21)
        w8, ws = (None, None) if dry else quant.quantize_rows(w)
        w8t = None if dry else B.tile_weights_fp8(w8)
        case = begin(f"linear_tiled_fp8 {M}x{N}x{K} act{act}", {}, [lin("op", M, N, K, act=act, out_fp32=1, entry=E_TILED_FP8,
                                                                        flags=F_W8T | F_RES | (F_BIAS if bias is not None else 0))])
        op(case, "out", lambda: B.linear_tiled_fp8(x, w8t, ws, N, bias=bias, residual=res, act=act, out_fp32=True))
    fused = [(M, 6144, act) for M, act in grid(T_.test_skinny_gemm_fused_rmsnorm)] + list(grid(T_.test_skinny_persistent_fused_norm))
    for M, N, act in fused[:2] if quick else fused:
        x, w, res, bias, nw = operands(M, N, 4096, act, 31)
        for knobs in ({}, {9: 0}, {9: 2}):
            case = begin(f"linear_rmsnorm {M}x{N}x4096 act{act}", knobs, [lin("op", M, N, 4096, act=act, out_fp32=1, flags=F_NORM | F_RES, entry=E_RMSNORM)])
            op(case, "out", lambda: B.linear_rmsnorm(x, nw, 1e-5, w, residual=res, act=act, out_fp32=True))
    fp8 = ([g + (False,) for g in grid(T_.test_gemv_fp8_weights)] + [(M, 6144, 4096, 0, True) for M in grid(T_.test_gemv_fp8_fused_rmsnorm)] +
           [g + (False,) for g in grid(T_.test_skinny_wide_rows) if g[2] % 1024 == 0 and (g[3] != 3 or g[1] % 64 == 0)] +
           [(M, N, 4096, act, True) for M, N, act in grid(T_.test_skinny_persistent_fused_norm) if act != 3 or N % 64 == 0] + [(65, 64, 2048, 0, False)])
    for M, N, K, act, norm in fp8[:3] if quick else fp8:
        x, w, res, bias, nw = operands(M, N, K, act, 41)
        w8, ws = (None, None) if dry else quant.quantize_rows(w)
        for knobs in ({}, {9: 0}):
            fl = F_W8 | F_RES | (F_NORM if norm else 0) | (F_BIAS if bias is not None else 0)
            case = begin(f"linear_fp8 {M}x{N}x{K} act{act} norm{int(norm)}", knobs, [lin("op", M, N, K, act=act, out_fp32=1, flags=fl, entry=E_LINEAR)])
            op(case, "out", lambda: B.linear_fp8(x, w8, ws, bias=bias, residual=res, act=act, out_fp32=True, norm_w=nw if norm else None, norm_eps=1e-5))
    shapes = []
    for g in (list(grid(T_.test_skinny_gemm)) + list(grid(T_.test_skinny_wide_rows)) + list(grid(T_.test_decode_tile_route_splitk)) +
              list(grid(T_.test_gemv)) + [s + (0,) for s in T_.GEMM_SHAPES]):
        g = tuple(g[:4]) if len(g) >= 4 else tuple(g[:3]) + (0,)
        if g not in shapes:
            shapes.append(g)
    for M, N, K, act in shapes[:4] if quick else shapes:
        x, w, res, bias, nw = operands(M, N, K, act, 51)
        for impl in range(5):
            fl = F_RES | (F_BIAS if bias is not None else 0)
            case = begin(f"linear_impl{impl} {M}x{N}x{K} act{act}", {}, [lin("op", M, N, K, act=act, out_fp32=1, flags=fl, entry=E_IMPL0 + impl)])
            op(case, "out", lambda: B.linear(x, w, bias=bias, residual=res, act=act, out_fp32=True, impl=impl))
    begin("end", {}, [])
    if not dry:
        torch.cuda.synchronize()
    with open(log_path, "w") as f:
        json.dump({"cases": cases}, f, indent=0)
    print(f"route_sweep: {len(cases) - 1} cases -> {log_path}")


# ------------------------------------------------------------------------------------------------------------------------------------
# trace -> cases
# ------------------------------------------------------------------------------------------------------------------------------------
def short(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    return re.sub(r"\(.*\)$", "", name)


def launches_per_case(trace_csv, n_cases):
    """[[(kernel, grid, workgroup, lds)] per case] - the trace cut at the marker launches"""
    with open(trace_csv) as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0))))
    out, cur = [], None
    for r in rows:
        name = short(r["Kernel_Name"])
        rec = (name, "x".join(r[f"Grid_Size_{a}"] for a in "XYZ"), "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ"), r.get("LDS_Block_Size") or r.get("Group_Segment_Size") or "?")
        if name.startswith("norm_kernel<true>") and rec[1].split("x")[0] in (rec[2].split("x")[0], "1"):          # the marker: ONE workgroup of the generic RMSNorm kernel
            cur = []
            out.append(cur)
        elif cur is not None:
            cur.append(rec)
    if len(out) != n_cases:
        sys.exit(f"route_sweep: the trace holds {len(out)} marker launches, the log {n_cases} cases")
    return out


def linear_launches(recs):
    return [(route_of(r[0]),) + r for r in recs if route_of(r[0])]


def summarise(trace_csv, log_json):
    cases = json.load(open(log_json))["cases"]
    per_case = launches_per_case(trace_csv, len(cases))
    total = hashlib.sha256()
    for case, recs in zip(cases, per_case):
        h = hashlib.sha256("\n".join(" ".join(r) for r in recs).encode()).hexdigest()
        total.update(h.encode())
        knobs = " ".join(f"k{k}={case['knobs'][str(k)]}" for k in case["named"])
        print(f"== case {case['id']}: {case['label']} {knobs}".rstrip())
        print(f"   launches {len(recs)} sha256 {h}")
        prev, count = None, 0
        for rec in linear_launches(recs) + [None]:
            if rec == prev:
                count += 1
                continue
            if prev:
                print(f"   {prev[0]:14s} {prev[1]} grid {prev[2]} wg {prev[3]} lds {prev[4]}" + (f"  x{count}" if count > 1 else ""))
            prev, count = rec, 1
        for k, v in sorted(case["digests"].items()):
            print(f"   digest {k} {v}")
    print(f"== all launches sha256 {total.hexdigest()}")


GOLDEN_COLUMNS = ("k9", "k14", "k19", "entry", "flags", "M", "N", "K", "lda", "ldw", "act", "out_fp32", "route")


def write_table(table):
    """one row per distinct (knobs, entry, flags, shape): compact JSON, columns named once"""
    rows = [[t["knobs"]["9"], t["knobs"]["14"], t["knobs"]["19"]] + [t[c] for c in GOLDEN_COLUMNS[3:]] for t in table]
    print('{"columns": ' + json.dumps(list(GOLDEN_COLUMNS)) + ', "rows": [')
    print(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
    print("]}")


def golden(trace_csv, log_json):
    cases = json.load(open(log_json))["cases"]
    per_case = launches_per_case(trace_csv, len(cases))
    table, seen = [], set()
    for case, recs in zip(cases, per_case):
        routes = [r[0] for r in linear_launches(recs)]
        want = list(case["linears"])
        if any("attn_o_fused" in r[0] for r in recs):          # 1..2-row steps: the O projection rides in the attention launch
            want = [l for l in want if l["name"] != "o"]
        if any(str(v).startswith("rejected") for v in case["digests"].values()) and len(routes) < len(want):
            want = want[:len(routes) + 1]          # the call stopped at the first linear nothing takes
            routes = routes + ["NONE"]
        if len(routes) != len(want):
            sys.exit(f"route_sweep: case {case['id']} ({case['label']}) issued {len(want)} linears, the trace shows {len(routes)} linear launches")
        for l, route in zip(want, routes):
            entry = {k: l[k] for k in ("M", "N", "K", "lda", "ldw", "act", "out_fp32", "flags", "entry")}
            entry["knobs"] = case["knobs"]
            key = json.dumps(entry, sort_keys=True)
            if key in seen:
                prior = next(t for t in table if json.dumps({k: t[k] for k in entry}, sort_keys=True) == key)
                if prior["route"] != route:
                    sys.exit(f"route_sweep: {key} ran on {prior['route']} and on {route}")
                continue
            seen.add(key)
            table.append({**entry, "route": route})
    write_table(table)



def oracle_build(out_dir):
    """compile tools/route_oracle.hip (the dispatch code from before the planner) against the built library; returns the program's path"""
    import subprocess
    lib_dir = os.path.join(REPO, "vision-zephyr_amd", "lib")
    exe = os.path.join(out_dir, "route_oracle")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2", "-std=c++17",
                           "-I" + os.path.join(REPO, "vision-zephyr_amd", "csrc"), "-I" + os.path.join(REPO, "include"),
                           os.path.join(REPO, "tools", "route_oracle.hip"), "-o", exe, "-L" + lib_dir, "-lviszephyr_hip", "-Wl,-rpath," + lib_dir])
    return exe


def oracle_table(exe, log_json):
    """the golden table from the OLD dispatch code's answers for every linear of a log (`run --dry` writes one without a GPU)"""
    import subprocess
    table, seen, lines = [], set(), []
    for case in json.load(open(log_json))["cases"]:
        for l in case["linears"]:
            entry = {k: l[k] for k in ("M", "N", "K", "lda", "ldw", "act", "out_fp32", "flags", "entry")}
            entry["knobs"] = case["knobs"]
            key = json.dumps(entry, sort_keys=True)
            if key not in seen:
                seen.add(key)
                table.append(entry)
                lines.append(" ".join(str(v) for v in [case["knobs"]["9"], case["knobs"]["14"], case["knobs"]["19"]] + [l[c] for c in GOLDEN_COLUMNS[3:-1]]))
    routes = subprocess.run([exe, "table"], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
    assert len(routes) == len(table)
    write_table([{**t, "route": r} for t, r in zip(table, routes)])


def diff(a, b):
    la, lb = open(a).read().splitlines(), open(b).read().splitlines()
    bad, case = [], ""
    for i in range(max(len(la), len(lb))):
        x, y = (la[i] if i < len(la) else "<missing>"), (lb[i] if i < len(lb) else "<missing>")
        if x.startswith("== case"):
            case = x
        if x != y:
            bad.append(f"{case}\n  - {x}\n  + {y}")
    print(f"{a} vs {b}: {len(la)} / {len(lb)} lines, {len(bad)} differ")
    for d in bad[:200]:
        print(d)
    return 1 if bad else 0


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "run":
        run(sys.argv[sys.argv.index("--log") + 1], "--quick" in sys.argv, "--dry" in sys.argv)
    elif cmd == "summarise":
        summarise(sys.argv[2], sys.argv[3])
    elif cmd == "golden":
        golden(sys.argv[2], sys.argv[3])
    elif cmd == "oracle":          # oracle grid | oracle golden LOG.json
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            exe = oracle_build(tmp)
            if sys.argv[2] == "golden":
                oracle_table(exe, sys.argv[3])
            else:
                import subprocess
                sys.exit(subprocess.call([exe, "grid"]))
    elif cmd == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
