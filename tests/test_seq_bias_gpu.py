"""sequence_bias and bad_words_ids on the device (csrc/logits_proc.hip): the kernel against tests/seq_bias_ref.py bit
for bit (itself pinned to HF's classes by tests/test_seq_bias_cpu.py), and generate() with the two keywords against a host loop over the
same engine calls, un-armed, with the restatement applied to the logits on the host."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seq_bias_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NEW = 12


# ---- 7. the kernel ---------------------------------------------------------------------------------------------------------------------
def _alphabet(cols):
    return np.concatenate([[0], np.linspace(1, cols - 2, 14).astype(np.int64), [cols - 1]])


def _logit_rows(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, cols, generator=g) * 3).float()
    a = _alphabet(cols)
    x[:, a[1]] = 0.0                     # biased and penalised ids reach an exact zero, a negative and a -inf logit
    x[:, a[3]] = -2.25
    x[:, a[4]] = float("-inf")
    return x


def _configs(cols):
    from vz_hip.logits_proc import ProcConfig
    a = [int(t) for t in _alphabet(cols)]
    inf = float("-inf")
    return [
        ProcConfig(seq=(((a[1],), 2.5, False),)),
        # one-id sequences, longer ones, two sequences and a one-id sequence that bias one id (a[5]), a -inf bias
        ProcConfig(seq=(((a[5],), -0.3, False), ((a[3],), 4.0, False), ((a[2], a[5]), 2.0, False), ((a[6], a[5]), 0.7, False),
                        ((a[7], a[8], a[9]), 4.0, False), ((a[2], a[10]), inf, False))),
        # bias on ids the penalty also touches, either sign, and bad words beside them
        ProcConfig(penalty=1.3, seq=(((a[1],), -2.0, False), ((a[3],), 4.0, False), ((a[7],), 6.0, False), ((a[2], a[3]), -9.5, False),
                                     ((a[9],), inf, True), ((a[2], a[6]), inf, True), ((a[7], a[8], a[11]), inf, True))),
        ProcConfig(penalty=0.7, ngram=2, min_new=5, eos=(a[15],), suppress=(a[12],),
                   seq=(((a[3],), 4.0, False), ((a[7],), -6.0, False), ((a[2], a[7]), 1e8, False), ((a[6], a[7]), -1e8, False),
                        (tuple(a[2:10]), 3.0, False), ((a[13],), inf, True), (tuple(a[3:11]), inf, True))),
        # the table full: 64 sequences
        ProcConfig(penalty=1.3, seq=tuple(((a[i % 16],), 0.25 * i, False) for i in range(16)) + tuple(((a[i % 16], a[(i * 5 + 1) % 16]), 1.0 + i, False) for i in range(32))
                   + tuple(((a[(i + 1) % 16], a[i % 16], a[(i + 2) % 16]), inf, True) for i in range(16))),
    ]


def _histories(rows, cols, shift, rng):
    """shorter than, as long as and longer than the sequences, and ends that match the configs' prefixes"""
    a = [int(t) for t in _alphabet(cols)]
    ends = [[], [a[2]], [a[6]], [a[7], a[8]], [a[0], a[2]], [a[0], a[6]], a[2:9], a[3:10], [a[1]] + a[2:9], [a[0], a[7], a[8]]]
    out = []
    for r in range(rows):
        e = ends[(r + shift) % len(ends)]
        n = (0, 0, 3, 40, 1500)[(r + shift) % 5] if e else 0
        out.append([a[i] for i in rng.integers(0, 16, size=n)] + e if (r + shift) % 3 else list(e))
    return out


def _run_kernel(x, hists, cfg):
    from vz_hip import binding as B
    rows = x.shape[0]
    stride = 2048 if max(len(h) for h in hists) > 64 else 64
    hist = torch.full((rows, stride), -7, dtype=torch.int32)
    for r, h in enumerate(hists):
        hist[r, :len(h)] = torch.tensor(h, dtype=torch.int32)
    hl = torch.tensor([len(h) for h in hists], dtype=torch.int32)
    y = x.clone().cuda()
    hd, hld = hist.cuda(), hl.cuda()
    B.logits_process(y, cfg, hd, hld)
    assert torch.equal(hd.cpu(), hist) and torch.equal(hld.cpu(), hl), "the op-level form appends nothing"
    return y.cpu().numpy()


@pytest.mark.parametrize("rows,cols", [(1, 1000), (5, 1000), (1, 32001), (5, 32001)])
def test_kernel_equals_reference_bitwise(rows, cols):
    rng = np.random.default_rng(cols + rows)
    x = _logit_rows(rows, cols, seed=cols)
    changed = 0
    for i, cfg in enumerate(_configs(cols)):
        for shift in range(10 if rows == 1 else 2):
            hists = _histories(rows, cols, shift + 3 * i, rng)
            got = _run_kernel(x, hists, cfg)
            for r in range(rows):
                want = R.process(x[r].numpy(), hists[r], cfg)
                assert np.array_equal(got[r].view(np.int32), want.view(np.int32)), (i, shift, r, hists[r][-9:], np.nonzero(got[r].view(np.int32) != want.view(np.int32))[0])
                changed += int((want.view(np.int32) != x[r].numpy().view(np.int32)).sum())
    assert changed > 20


def test_kernel_ignores_ids_outside_the_row():
    from vz_hip.logits_proc import ProcConfig
    cols = 1000
    x = _logit_rows(2, cols, seed=3)
    cfg = ProcConfig(seq=(((cols,), 5.0, False), ((5, cols + 7), 2.0, False), ((2 ** 30,), float("-inf"), True), ((5, 9), 1.5, False),
                          ((cols, 11), 1.0, False)))
    hists = [[3, 5], [cols, 4, cols]]          # row 1: an id outside the row in the history matches a prefix outside the row
    got = _run_kernel(x, hists, cfg)
    for r in range(2):
        assert np.array_equal(got[r].view(np.int32), R.process(x[r].numpy(), hists[r], cfg).view(np.int32))
    assert got[0][9] == x[0, 9] + np.float32(1.5) and got[1][11] == x[1, 11] + np.float32(1.0)
    assert int((got != x.numpy()).sum()) == 2


def test_op_refuses_what_the_table_cannot_hold():
    from vz_hip import binding as B
    x = torch.zeros(1, 1000).cuda()
    h, hl = torch.zeros(1, 8, dtype=torch.int32).cuda(), torch.zeros(1, dtype=torch.int32).cuda()

    def call(tab, n):
        arr = (B.C.c_int * len(tab))(*tab)
        rec = B.VzLogitsProcParams(1.0, 0, 0, 0, 0, n, None, None, arr)
        B.check(B.lib().vz_op_logits_process(B.ptr(x), 1, 1000, B.ptr(h), 8, B.ptr(hl), B.C.byref(rec), B.stream_ptr(x.device)))

    one = [1, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0]
    call(one * 64, 64)
    for tab, n in ((one * 65, 65), ([9] + one[1:], 1), ([0] + one[1:], 1), ([1, 2] + one[2:], 1), ([1, 0, 0, 0, -5] + one[5:], 1)):
        with pytest.raises(ValueError):
            call(tab, n)


# ---- 8. generate() -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    """the 2-layer synthetic model of tests/test_sample_rows_gpu.py"""
    from vz_hip import synth
    from vis_zephyr.model import VisZephyrConfig, VisZephyrForCausalLM
    cfg = synth.ArchConfig(n_layers=2)
    hf = VisZephyrConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=2, num_attention_heads=32,
                         num_key_value_heads=8, vocab_size=cfg.vocab, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    return VisZephyrForCausalLM.from_synthetic(hf, seed=0, max_batch=6, max_ctx=256, max_tiles=1, max_text=32)


def _parse(kw, eos):
    from vz_hip import logits_proc as LP
    return LP.parse(kw.get("repetition_penalty"), kw.get("no_repeat_ngram_size"), kw.get("min_new_tokens"), kw.get("suppress_tokens"), eos,
                    kw.get("sequence_bias"), kw.get("bad_words_ids"), 32000)


def _host_loop(model, ids, seqlens, cfg, max_new=NEW):
    """tests/test_logits_proc_gpu.py's host loop with the six processors: un-armed engine calls, the raw logits read back at every step, the
    processors on the host (seq_bias_ref), the first maximal index"""
    eng = model.engine
    Bn = ids.shape[0]
    emb = model.get_model().embed_tokens(ids.to(model.device))
    _, last = eng.prefill(emb, seqlens, None, all_logits=False, last_logits=True)
    out = [[] for _ in range(Bn)]
    raw = [[] for _ in range(Bn)]

    def choose(lg):
        toks = []
        for b in range(Bn):
            x = lg[b].cpu().numpy()
            raw[b].append(x)
            if cfg is not None:
                x = R.process(x, out[b], cfg)
            toks.append(int(np.argmax(x)))
            out[b].append(toks[-1])
        return toks

    toks = choose(last)
    for t in range(1, max_new):
        eng.decode_begin(torch.tensor(toks, dtype=torch.int32), [l + t - 1 for l in seqlens], [l + t - 1 for l in seqlens])
        _, lg = eng.decode_steps(1, return_logits=True)
        toks = choose(lg[0])
    return out, raw


def _prompts(lens, seed0):
    from vz_hip import synth
    ids = torch.full((len(lens), max(lens)), 5, dtype=torch.long)
    mask = torch.zeros(len(lens), max(lens), dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = synth.synth_ids(n, 32000, image_pos=-1, seed=seed0 + b)
        mask[b, :n] = 1
    return ids, mask


class _Streamer:
    def __init__(self):
        self.got = []

    def put(self, v):
        self.got += v.reshape(-1).tolist()

    def end(self):
        pass


def test_generate_equals_host_loop(model):
    eng = model.engine
    ids, _ = _prompts([12], 21)
    kw0 = dict(input_ids=ids, do_sample=False, max_new_tokens=NEW, eos_token_id=[])
    (plain,), (raw,) = _host_loop(model, ids, [12], None)
    assert model.generate(**kw0)[0].tolist() == plain and len(set(plain)) == NEW
    # a one-id bad word (the free run's first id: only one-id sequences can act on the prefill logits), a two-id and a three-id bad word
    # the free run emits, and a bias that lifts the runner-up of step 6 over everything once the free run's ids 4, 5 stand in front of it
    second = int(np.argsort(raw[6])[-2])
    lift = float(raw[6].max() - raw[6][second]) + 1.0
    kw = dict(bad_words_ids=[[plain[0]], [plain[2], plain[3]], [plain[7], plain[8], plain[9]]],
              sequence_bias={(plain[4], plain[5], second): lift, (plain[1],): -0.25})
    cfg = _parse(kw, [])
    (want,), _ = _host_loop(model, ids, [12], cfg)
    bans_only = model.generate(**kw0, bad_words_ids=kw["bad_words_ids"])[0].tolist()
    (want_bans,), _ = _host_loop(model, ids, [12], _parse(dict(bad_words_ids=kw["bad_words_ids"]), []))
    print("plain", plain, "bans", want_bans, "bans + bias", want)
    assert bans_only == want_bans and want_bans[0] != plain[0]          # the bans bite: the free run's first id is gone
    got = model.generate(**kw0, **kw)[0].tolist()
    assert got == want and want != plain
    # a multi-id bad word of the run with the first id free again: the run keeps the word's prefix and leaves it at its last id
    (w2,), _ = _host_loop(model, ids, [12], _parse(dict(bad_words_ids=[[plain[2], plain[3]]]), []))
    g2 = model.generate(**kw0, bad_words_ids=[[plain[2], plain[3]]])[0].tolist()
    assert g2 == w2 and g2[:3] == plain[:3] and g2[3] != plain[3]
    (w3,), _ = _host_loop(model, ids, [12], _parse(dict(sequence_bias={(plain[4], plain[5], second): lift}), []))
    g3 = model.generate(**kw0, sequence_bias={(plain[4], plain[5], second): lift})[0].tolist()
    assert g3 == w3 and g3[:6] == plain[:6] and g3[6] == second != plain[6]
    # the streamer route (one step in flight) and the sampled route take the same filter
    st = _Streamer()
    assert model.generate(**kw0, **kw, streamer=st)[0].tolist() == want and st.got == want
    s = model.generate(input_ids=ids, do_sample=True, temperature=0.9, seed=5, max_new_tokens=NEW, eos_token_id=[], bad_words_ids=[[plain[0]]],
                       sequence_bias={(t,): float("-inf") for t in plain[1:4]})[0].tolist()
    assert not set(s) & set(plain[:4])
    # prompt lookup with the keywords: the plain greedy path, the same ids
    assert model.generate(**kw0, **kw, prompt_lookup_num_tokens=3)[0].tolist() == want
    # the table is part of what a captured step freezes: a changed one captures again
    c0 = eng.decode_info()[1]
    model.generate(**kw0, **dict(kw, sequence_bias={(plain[4], plain[5], second): lift, (plain[1],): -0.5}))
    assert eng.decode_info()[1] > c0
    # disarmed afterwards: the plain call is the plain run
    assert model.generate(**kw0)[0].tolist() == plain


def test_batched_generate_equals_host_loop(model):
    lens = [12, 9, 5]
    ids, mask = _prompts(lens, 30)
    kw0 = dict(input_ids=ids, attention_mask=mask, do_sample=False, max_new_tokens=NEW, eos_token_id=[])
    base, _ = _host_loop(model, ids, lens, None)
    assert model.generate(**kw0).tolist() == base
    # every row's free run loses a two-id word, row 0's also its first id; a bias on row 1's second id
    kw = dict(bad_words_ids=[[base[0][0]]] + [[base[b][3], base[b][4]] for b in range(3)], sequence_bias={(base[1][1],): -30.0},
              repetition_penalty=1.3)
    want, _ = _host_loop(model, ids, lens, _parse(kw, []))
    got = model.generate(**kw0, **kw).tolist()
    assert got == want
    assert got[0][0] != base[0][0] and got[1][:1] == base[1][:1] and got[1][1] != base[1][1] and got[2][:4] == base[2][:4] and got[2][4] != base[2][4]


def test_equal_table_uploads_and_captures_nothing(model):
    """the engine keeps the table: arming with the table of the previous arming replays the captured step, a table that differs in one
    bias captures again - and the step follows it"""
    from vz_hip import binding as B
    from vz_hip.logits_proc import ProcConfig
    eng = model.engine
    ids, _ = _prompts([12], 21)
    _, last = eng.prefill(model.get_model().embed_tokens(ids.to(model.device)), [12], None, all_logits=False, last_logits=True)
    first = B.argmax(last)
    buf = torch.empty(1, 4, dtype=torch.int32, device=model.device)

    def run(cfg):
        eng.set_logits_proc(cfg)
        try:
            eng.decode_begin(first, [12], [12])
            return eng.decode_steps(4, out=buf).cpu().tolist()[0], eng.decode_info()[1]
        finally:
            eng.set_logits_proc(None)

    free, _ = run(None)
    cfg = ProcConfig(seq=(((free[1],), -50.0, False), ((free[0], free[1]), float("-inf"), True)))
    a, c1 = run(cfg)
    b, c2 = run(ProcConfig(seq=cfg.seq))
    assert a == b and c2 == c1 and a[0] == free[0] and a[1] != free[1]
    c, c3 = run(ProcConfig(seq=(((free[1],), 0.0, False), ((free[0], free[0]), float("-inf"), True))))
    assert c3 == c2 + 1 and c == free


def test_refusals(model):
    ids, _ = _prompts([12], 21)
    for kw in (dict(bad_words_ids=[[5, 6]]), dict(sequence_bias={(5, 6): 1.0})):
        with pytest.raises(NotImplementedError):
            model.generate(input_ids=ids, num_beams=2, max_new_tokens=4, **kw)
        with pytest.raises(NotImplementedError):
            next(model.generate_stream([{"input_ids": ids, "max_new_tokens": 4, **kw}], rows=3))
    with pytest.raises(NotImplementedError):
        model.generate(input_ids=ids, max_new_tokens=4, bad_words_ids=[[i + 10] for i in range(65)])
    with pytest.raises(NotImplementedError):
        model.generate(input_ids=ids, max_new_tokens=4, sequence_bias={tuple(range(1, 10)): 1.0})
    with pytest.raises(ValueError):
        model.generate(input_ids=ids, max_new_tokens=4, bad_words_ids=[[5, 32000]])
    with pytest.raises(ValueError):
        model.generate(input_ids=ids, max_new_tokens=4, sequence_bias={(5,): 1})
    # the engine checks what it is armed with itself
    from vz_hip import binding as B
    eng = model.engine
    bad = (B.C.c_int * 12)(9, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8)
    with pytest.raises(ValueError):
        B.check(eng.lib.vz_llm_decode_logits_proc(eng.h, B.C.byref(B.VzLogitsProcParams(1.0, 0, 0, 0, 0, 1, None, None, bad)), None))
    with pytest.raises(ValueError):
        B.check(eng.lib.vz_llm_decode_logits_proc(eng.h, B.C.byref(B.VzLogitsProcParams(1.0, 0, 0, 0, 0, 65, None, None, None)), None))
    eng.set_logits_proc(None)
