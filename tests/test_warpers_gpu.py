"""HF's warpers behind top-p on the device (csrc/sampling.hip step 3b): the kept set of the op-level calls against
tests/warpers_ref.py (itself pinned to HF's classes by tests/test_warpers_cpu.py), the exact draw, the distribution, and the keywords in
generate() / generate_stream.

Every parameter of the op-level tests is chosen away from any token (warpers_ref.build_row): the geometric midpoint between two adjacent
decision values at least 1 % apart (an fp32 sum of up to 65536 terms is off by 0.4 % at the worst), typical_p at the midpoint between
two cumulative masses whose token holds at least 1 % of the mass with neighbouring shifted values at least 1e-3 apart.  So kept sets must
be EQUAL, n_kept too; lse_kept at the tolerance of tests/test_scores_gpu.py: 2e-5 + 2^-22 * max|x / T|."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warpers_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu

NEG = float("-inf")
NAMES = list(WR.CASES)


def _tol(x):
    f = np.abs(x[np.isfinite(x)])
    return 2e-5 + 2.0 ** -22 * (float(f.max()) if f.size else 0.0)


def _tables(R, V):
    """lists of (case name, logits, RowParams): one row per case for R = 1, a greedy and two sampled rows side by side for R = 3, the cases
    in turn for R = 64"""
    if R == 1:
        return [[(n,) + WR.build_row(n, V, V % 89 + 3 * i)] for i, n in enumerate(NAMES)]
    if R == 3:
        return [[(n,) + WR.build_row(n, V, V % 89 + 40 + i) for i, n in enumerate(t)]
                for t in (("greedy", "all", "typical_drops_top"), ("min_p", "epsilon_keeps_one", "no_top_k"))]
    return [[(NAMES[r % len(NAMES)],) + WR.build_row(NAMES[r % len(NAMES)], V, V % 89 + 100 + 5 * r) for r in range(R)]]


# ---- 4. the kept set against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1000, 32001, 40000])          # 40000 > 32768: the loop form
@pytest.mark.parametrize("R", [1, 3, 64])
def test_kept_set_equals_restatement(R, V):
    from vz_hip import binding as B
    from vz_hip import scores as SC
    for table in _tables(R, V):
        x = np.stack([t[1] for t in table])
        params = [t[2] for t in table]
        ref = [WR.warp_params(x[r], params[r]) for r in range(len(table))]
        toks = torch.tensor([WR.draw(x[r], params[r]) for r in range(len(table))], dtype=torch.int32)
        xd = torch.from_numpy(x).cuda()
        rec, warped = B.token_scores(xd, toks.cuda(), params, warped=True)
        _, _, lk, nk = (t.cpu().numpy() for t in SC.unpack(rec))
        warped = warped.cpu().numpy()
        for r, (name, xr, p) in enumerate(table):
            kept, want = np.isfinite(warped[r]), np.isfinite(ref[r])
            print(f"R {R} V {V} row {r} {name}: T {p.temperature} k {p.top_k} p {p.top_p} warp {p.warp}: n_kept {nk[r]} vs {int(want.sum())}, lse_kept {lk[r]!r}")
            if not p.sample:
                assert np.array_equal(warped[r], xr) and nk[r] == V
                continue
            assert np.array_equal(kept, want), (name, r, np.nonzero(kept != want)[0].tolist())
            assert int(nk[r]) == int(want.sum())
            assert np.array_equal(warped[r].view(np.uint32), ref[r].view(np.uint32))          # x / T where kept, -inf elsewhere
            assert abs(float(lk[r]) - WR.lse(ref[r])) <= _tol(ref[r]), (name, r, lk[r], WR.lse(ref[r]))
            if name == "typical_drops_top":
                assert not kept[int(np.argmax(xr))] and nk[r] >= 1
            if name == "epsilon_keeps_one":
                assert nk[r] == 1 and kept[int(np.argmax(xr))]
        again = B.token_scores(xd, toks.cuda(), params, warped=True)[0]
        assert torch.equal(again.view(torch.int32), rec.view(torch.int32))          # a second run: the same bits


# ---- 5. the exact draw ------------------------------------------------------------------------------------------------------------------
def _race_margin(x, p, row):
    s = (WR.warp_params(x, p) + WR.SO.gumbel(x.shape[0], row, p.counter, p.seed)).astype(np.float32)
    two = np.partition(s[np.isfinite(s)], -2)[-2:] if np.isfinite(s).sum() > 1 else np.array([0.0, 1.0])
    return float(two[1] - two[0])


@pytest.mark.parametrize("V", [1000, 32001, 40000])
def test_draw_equals_restatement(V):
    """the per-row kernel and the one-sequence kernel (on the row alone, and as row r of a batch that shares the row's parameters) draw the
    restatement's token; as in tests/test_sampling_gpu.py a draw may differ only where the two best race scores are closer than 1e-3"""
    from vz_hip import binding as B
    table = [(n,) + WR.build_row(n, V, V % 89 + 300 + 7 * i + j) for i, n in enumerate(NAMES) for j in range(2)]
    x = np.stack([t[1] for t in table])
    params = [t[2] for t in table]
    xd = torch.from_numpy(x).cuda()
    got = B.sample_rows(xd, params).cpu().tolist()
    bad = 0
    for r, (name, xr, p) in enumerate(table):
        want = WR.draw(xr, p)
        one = int(B.sample(xd[r:r + 1], p.temperature, p.top_k, p.top_p, p.seed, p.counter, warp=p.warp)[0]) if p.sample else want
        assert one == got[r], (name, r, one, got[r])          # the two kernels: the same bits
        assert np.isfinite(WR.warp_params(xr, p)[got[r]]), f"row {r} ({name}) drew token {got[r]}, which the warpers filter"
        if got[r] != want:
            assert _race_margin(xr, p, 0) < 1e-3, (name, r, got[r], want)
            bad += 1
    # row r of a batch under one set of parameters: the Philox row word is r
    name, xr, p = table[NAMES.index("all") * 2]
    ids = B.sample(torch.from_numpy(xr).expand(16, V).contiguous().cuda(), p.temperature, p.top_k, p.top_p, p.seed, p.counter, warp=p.warp).cpu().tolist()
    for r in range(16):
        want = WR.draw(xr, p, row=r)
        if ids[r] != want:
            assert _race_margin(xr, p, r) < 1e-3, (r, ids[r], want)
            bad += 1
    assert bad <= 2, f"{bad} draws differ from the restatement"


# ---- 6. the distribution ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["min_p", "typical", "all"])
def test_distribution_chi_square(case):
    """draw count and significance level of tests/test_sampling_gpu.py::test_distribution_chi_square, one row at V = 1000"""
    from vz_hip import binding as B
    V, rows = 1000, 8192
    xr, p = WR.build_row(case, V, 21)
    w = WR.warp_params(xr, p).astype(np.float64)
    pr = np.exp(w - w.max())
    pr /= pr.sum()
    x = torch.from_numpy(xr).expand(rows, V).contiguous().cuda()
    cnt = np.zeros(V)
    n = 0
    for counter in range(4):
        ids = B.sample(x, p.temperature, p.top_k, p.top_p, 99, counter, warp=p.warp).cpu().numpy()
        np.add.at(cnt, ids, 1)
        n += rows
    assert cnt[pr == 0].sum() == 0, "a filtered token was drawn"
    big = pr * n >= 5
    chi2 = float(((cnt[big] - pr[big] * n) ** 2 / (pr[big] * n)).sum())
    dof = int(big.sum()) - 1
    print(f"{case}: {int((pr > 0).sum())} kept, chi2 {chi2:.2f}, dof {dof}")
    assert dof >= 1 and chi2 < dof + 5 * np.sqrt(2 * dof), (chi2, dof)


def test_op_refuses_bad_warpers():
    from vz_hip import binding as B
    from vz_hip.sample_rows import RowParams
    x = torch.randn(2, 1000).cuda()
    ok = RowParams(True, 0.7, 50, 0.9, 1, 0, min_p=0.1)
    for bad in (RowParams(True, 0.7, 50, 0.9, 1, 0, min_p=1.5), RowParams(True, 0.7, 50, 0.9, 1, 0, min_p=float("nan"))):
        with pytest.raises(ValueError):
            B.sample_rows(x, [ok, bad])
        with pytest.raises(ValueError):
            B.sample(x, 0.7, 50, 0.9, 1, 0, warp=bad.warp)
        with pytest.raises(ValueError):
            B.token_scores(x, torch.zeros(2, dtype=torch.int32).cuda(), [ok, bad])
    with pytest.raises(ValueError):
        B.sample(x, 0.7, 50, 0.9, 1, 0, warp=(0.1, -0.5, 0.0, 0.0))


# ---- 8. generate() and generate_stream -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from vz_hip import synth
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    cfg = synth.ArchConfig(n_layers=2)
    hf = VisZephyrConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=2, num_attention_heads=32,
                         num_key_value_heads=8, vocab_size=cfg.vocab, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    return VisZephyrForCausalLM.from_synthetic(hf, seed=0, max_batch=6, max_ctx=256, max_tiles=1, max_text=32)


@pytest.fixture()
def pinned_routes():
    """whole tiles only and no row-count-dependent K slices: rows of different batches get the same bits (tests/test_sample_rows_gpu.py)"""
    from vz_hip import binding as B
    with B.tuned(gemm256_streamk=0, splitk_mid=0):
        yield


def _prompt(n, seed):
    from vz_hip import synth
    return synth.synth_ids(n, 32000, image_pos=-1, seed=seed).unsqueeze(0)


def _pick(B, row_logits, p, counter):
    """the row's token by the op-level call of the one-sequence kernel on that row alone (Philox row word 0): int32 [1] on the device"""
    if not p.sample:
        return B.argmax(row_logits)
    return B.sample(row_logits, p.temperature, p.top_k, p.top_p, p.seed, counter, warp=p.warp)


def _host_steps(eng, first, next_pos, ctx, params, steps, switch=None):
    """the host-driven loop of tests/test_sample_rows_gpu.py: eager steps with the logits handed back, every row's token chosen by the
    op-level call; switch = {step: {row: params}} re-arms a row from that step on.  Returns [rows][steps] ids."""
    from vz_hip import binding as B
    R = len(params)
    params = list(params)
    ctr = [p.counter for p in params]
    eng.set_sampling_rows(None)
    eng.decode_begin(first, next_pos, ctx)
    out = [[] for _ in range(R)]
    for t in range(steps):
        for r, p in (switch or {}).get(t, {}).items():
            params[r], ctr[r] = p, p.counter
        _, lg = eng.decode_steps(1, return_logits=True)
        toks = torch.cat([_pick(B, lg[0, r:r + 1].contiguous(), params[r], ctr[r]) for r in range(R)]).tolist()
        for r in range(R):
            out[r].append(int(toks[r]))
            ctr[r] += 1
            eng.decode_set_row(r, toks[r], next_pos[r] + t + 1, ctx[r] + t + 1)
    return out


def _host_generate(model, ids, params, max_new):
    from vz_hip import binding as B
    eng = model.engine
    R, L = len(params), ids.shape[1]
    emb = eng.embed_tokens(ids.to(model.device).repeat(R, 1))
    _, last = eng.prefill(emb, [L] * R)
    first = torch.cat([_pick(B, last[r:r + 1].contiguous(), params[r], 0) for r in range(R)])
    rest = _host_steps(eng, first, [L] * R, [L] * R, [p.at(1) for p in params], max_new - 1) if max_new > 1 else [[] for _ in range(R)]
    return [[int(first[r])] + rest[r] for r in range(R)]


ALL4 = dict(min_p=0.02, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=2e-3)


def test_generate_equals_host_loop(model):
    from vz_hip import binding as B
    from vz_hip.sample_rows import RowParams
    eng = model.engine
    ids = _prompt(19, 60)
    kw = dict(do_sample=True, temperature=1.1, seed=777, max_new_tokens=8, eos_token_id=[])
    plain = model.generate(input_ids=ids, **kw)
    c0 = eng.decode_info()[1]
    assert model.generate(input_ids=ids, **kw).tolist() == plain.tolist()
    same = eng.decode_info()[1] - c0          # what a repeated call captures
    for warp in (dict(min_p=0.5), ALL4):
        out = model.generate(input_ids=ids, **kw, **warp)
        want = _host_generate(model, ids, [RowParams(True, 1.1, 50, 1.0, 777, 0, **warp)], 8)
        assert out.tolist() == want, (warp, out.tolist(), want)
    # output_scores rows hold -inf exactly outside the new kept set: the rows the op-level recorder gives on the step's own logits
    par = RowParams(True, 1.1, 50, 1.0, 777, 0, min_p=0.5)
    o = model.generate(input_ids=ids, **kw, min_p=0.5, return_dict_in_generate=True, output_scores=True, output_logits=True)
    base = model.generate(input_ids=ids, **kw, return_dict_in_generate=True, output_scores=True)
    assert o.sequences.tolist() == model.generate(input_ids=ids, **kw, min_p=0.5).tolist()
    for t in range(8):
        rec, w = B.token_scores(o.logits[t].contiguous(), o.sequences[:, t].to(torch.int32), [par], warped=True)
        assert torch.equal(o.scores[t].view(torch.int32), w.view(torch.int32)), t
        assert bool(torch.isfinite(o.scores[t][0, o.sequences[0, t]]))
    n_with, n_without = int(torch.isfinite(o.scores[0]).sum()), int(torch.isfinite(base.scores[0]).sum())
    print(f"first token: {n_with} tokens kept with min_p = 0.5, {n_without} without")
    assert 1 <= n_with < n_without == 50          # the keyword bites (the first token's logits are the same prefill logits)
    # a call without the keywords - or with HF's off values - runs what it ran: the same ids, and captures what a repeated call captures
    c1 = eng.decode_info()[1]
    assert model.generate(input_ids=ids, **kw).tolist() == plain.tolist()
    c2 = eng.decode_info()[1]
    assert model.generate(input_ids=ids, **kw, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0).tolist() == plain.tolist()
    assert eng.decode_info()[1] - c2 == same, (c0, c1, c2, eng.decode_info()[1], same)
    # greedy calls ignore the warpers, as HF does
    g = model.generate(input_ids=ids, do_sample=False, max_new_tokens=6, eos_token_id=[])
    assert model.generate(input_ids=ids, do_sample=False, max_new_tokens=6, eos_token_id=[], min_p=0.5, typical_p=0.3).tolist() == g.tolist()
    with pytest.raises(ValueError, match="min_p"):
        model.generate(input_ids=ids, **kw, min_p=1.5)
    with pytest.raises(ValueError, match="typical_p"):
        model.generate(input_ids=ids, **kw, typical_p=0.0)


def test_streamer_path_takes_the_warpers(model):
    """the one-sequence sampler inside the step, on the streamer route (one step in flight, tokens through the host-visible ring)"""
    from vz_hip.sample_rows import RowParams
    ids = _prompt(19, 60)
    kw = dict(do_sample=True, temperature=1.1, seed=777, max_new_tokens=8, eos_token_id=[], **ALL4)
    want = _host_generate(model, ids, [RowParams(True, 1.1, 50, 1.0, 777, 0, **ALL4)], 8)

    class _St:
        def __init__(self):
            self.got = []

        def put(self, v):
            self.got += v.reshape(-1).tolist()

        def end(self):
            pass
    st = _St()
    assert model.generate(input_ids=ids, streamer=st, **kw).tolist() == want and st.got == want[0]


def test_step_tail_rearm_captures_nothing(model):
    from vz_hip import binding as B
    from vz_hip.sample_rows import GREEDY, RowParams
    eng = model.engine
    lens = [9, 30, 17]
    ids = torch.full((3, max(lens)), 2, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = _prompt(n, 80 + b)[0]
    _, last = eng.prefill(eng.embed_tokens(ids.to(model.device)), lens)
    first = B.argmax(last)
    params = [RowParams(True, 0.9, 50, 0.95, 4242, 1, min_p=0.3), GREEDY.at(5), RowParams(True, 1.2, 0, 1.0, 77, 77, typical_p=0.5, eta_cutoff=3e-3)]
    other = RowParams(True, 1.2, 0, 0.9, 31337, 3, min_p=0.1, epsilon_cutoff=2e-3)
    want = _host_steps(eng, first, lens, lens, params, 6)
    want_sw = _host_steps(eng, first, lens, lens, params, 6, switch={3: {1: other}})

    def run(n_calls, rearm=None):
        buf = torch.empty(3, 6 // n_calls, dtype=torch.int32, device=model.device)
        eng.set_sampling_rows(params)
        try:
            eng.decode_begin(first, lens, lens)
            parts, caps = [], []
            for c in range(n_calls):
                if c and rearm is not None:
                    eng.decode_set_row_sampling(*rearm)
                parts.append(eng.decode_steps(6 // n_calls, out=buf).cpu().clone())
                caps.append(eng.decode_info()[1])
            return torch.cat(parts, 1).tolist(), caps
        finally:
            eng.set_sampling_rows(None)

    got, _ = run(1)
    assert got == want, (got, want)
    os.environ["VZ_NO_GRAPH"] = "1"
    try:
        eager, _ = run(1)
    finally:
        del os.environ["VZ_NO_GRAPH"]
    assert eager == got
    sw, caps = run(2, rearm=(1, other))
    assert sw == want_sw and caps[1] == caps[0], (sw, want_sw, caps)
    assert sw[0] == got[0] and sw[2] == got[2] and sw[1][:3] == got[1][:3]


def test_stream_and_return_sequences(model, pinned_routes):
    from vz_hip.sample_rows import RowParams, parse_request
    lens, budgets = [9, 30, 17, 44, 12], [6, 11, 9, 10, 7]
    samp = [dict(do_sample=True, temperature=0.9, seed=11, min_p=0.2), None, dict(do_sample=True, temperature=1.2, top_k=0, seed=12, typical_p=0.6),
            dict(do_sample=True, temperature=1.0, seed=13, min_p=0.05, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=2e-3), None]
    reqs = [{"input_ids": _prompt(n, 70 + i), "max_new_tokens": bud, **(samp[i] or {})} for i, (n, bud) in enumerate(zip(lens, budgets))]
    pars = [parse_request(r, model.generation_config, None) for r in reqs]
    assert [p.warp is not None for p in pars] == [True, False, True, True, False]
    free_run = []
    for i, p in enumerate(pars):          # the request alone: row 0 of a 2-row batch (same kernels as the stream's rows)
        two = _host_generate(model, reqs[i]["input_ids"], [p, p], budgets[i])
        assert two[0] == two[1]
        free_run.append(two[0])
    got = dict(model.generate_stream(reqs, eos_token_id=None, rows=3, sync_every=4))
    assert [got[i].tolist() for i in range(len(reqs))] == free_run
    # num_return_sequences = 3: row j under seed s + j
    ids, s = _prompt(21, 90), 4242
    kw = dict(do_sample=True, temperature=0.9, top_p=0.95, seed=s, max_new_tokens=8, eos_token_id=[], min_p=0.1, typical_p=0.8)
    out = model.generate(input_ids=ids, num_return_sequences=3, **kw)
    want = _host_generate(model, ids, [RowParams(True, 0.9, 50, 0.95, s + j, 0, min_p=0.1, typical_p=0.8) for j in range(3)], 8)
    assert out.tolist() == want, (out.tolist(), want)
