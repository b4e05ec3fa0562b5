"""The device-side logits processors (csrc/logits_proc.hip): the kernel against tests/logits_proc_ref.py bit for bit, and generate()
with `repetition_penalty`, `no_repeat_ngram_size`, `min_new_tokens`, `suppress_tokens` against a host loop over the same engine calls,
un-armed, with the reference applied to the logits on the host."""
import numpy as np
import pytest
import torch

import logits_proc_ref as R

pytestmark = pytest.mark.gpu

NEW = 32


# ---- kernel ------------------------------------------------------------------------------------------------------------------

def _alphabet(cols):
    mid = np.linspace(1, cols - 2, 14).astype(np.int64)
    return np.concatenate([[0], mid, [cols - 1]])


def _logit_rows(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, cols, generator=g) * 3).float()
    a = _alphabet(cols)
    x[:, a[1]] = 0.0                     # the history reaches an exact zero, a negative zero, a negative and a -inf logit
    x[:, a[2]] = -0.0
    x[:, a[3]] = -2.25
    x[:, a[4]] = float("-inf")
    return x


# penalty in {1, 1.3, 0.7}; g in {0, 1, 2, 3, 8}; min_new above / below the lengths; 0, 1 and 16 suppressed ids; 1 and 4 eos ids
def _param_sets(cols):
    from vz_hip.logits_proc import ProcConfig
    a = _alphabet(cols).tolist()
    sup16 = tuple(a[::2] + list(range(100, 108)))
    return [
        ProcConfig(penalty=1.3),
        ProcConfig(penalty=0.7, ngram=1),
        ProcConfig(ngram=2, suppress=(a[5],)),
        ProcConfig(penalty=1.3, ngram=3, min_new=5, eos=(a[0],)),
        ProcConfig(ngram=8, min_new=2000, eos=(a[15], a[1], 17, a[7])),
        ProcConfig(penalty=0.7, ngram=2, min_new=5, eos=(a[15], a[1], 17, a[7]), suppress=sup16),
        ProcConfig(penalty=1.3, ngram=8, min_new=2000, eos=(3,), suppress=sup16),
        ProcConfig(min_new=1, eos=(a[15],)),
        ProcConfig(suppress=sup16),
    ]


def _histories(rows, cols, g, shift, rng):
    g = max(g, 2)
    lens = [0, 1, g - 1, g, 37, 1500]
    a = _alphabet(cols)
    out = []
    for r in range(rows):
        n = lens[(r + shift) % len(lens)]
        out.append(a[rng.integers(0, 16, size=n)].tolist())
    return out


def _run_kernel(x, hists, cfg):
    from vz_hip import binding as B
    rows = x.shape[0]
    stride = 2048 if max(len(h) for h in hists) > 64 else 64          # the 1500-id rows: more ids than the workgroup has threads
    hist = torch.full((rows, stride), -7, dtype=torch.int32)
    for r, h in enumerate(hists):
        hist[r, :len(h)] = torch.tensor(h, dtype=torch.int32)
    hl = torch.tensor([len(h) for h in hists], dtype=torch.int32)
    y = x.clone().cuda()
    hd, hld = hist.cuda(), hl.cuda()
    out = B.logits_process(y, cfg, hd, hld)
    assert out.data_ptr() == y.data_ptr()
    assert torch.equal(hd.cpu(), hist) and torch.equal(hld.cpu(), hl), "the op-level form appends nothing"
    return y.cpu().numpy()


@pytest.mark.parametrize("rows,cols", [(1, 1000), (3, 32000), (5, 32001), (64, 4096)])
def test_kernel_equals_reference_bitwise(rows, cols):
    rng = np.random.default_rng(cols + rows)
    x = _logit_rows(rows, cols, seed=cols)
    for i, cfg in enumerate(_param_sets(cols)):
        hists = _histories(rows, cols, cfg.ngram, i, rng)
        got = _run_kernel(x, hists, cfg)
        want = np.stack([R.process(x[r].numpy(), hists[r], cfg) for r in range(rows)])
        bad = np.nonzero(got.view(np.int32) != want.view(np.int32))
        assert bad[0].size == 0, (cfg, [len(h) for h in hists], bad[0][:8], bad[1][:8], got[bad][:8], want[bad][:8])
        again = _run_kernel(x, hists, cfg)
        assert np.array_equal(again.view(np.int32), got.view(np.int32)), "a second call gives other bits"


def test_kernel_ignores_ids_outside_the_row():
    from vz_hip.logits_proc import ProcConfig
    cols = 1000
    x = _logit_rows(2, cols, seed=3)
    hists = [[5, cols, -1, 5, 2 ** 30, cols, -1, 5], [cols + 31, 999, -2 ** 31, 999]]
    cfg = ProcConfig(penalty=1.3, ngram=2, min_new=50, eos=(cols, 4), suppress=(-1, cols, 1023, 7))
    got = _run_kernel(x, hists, cfg)
    want = np.stack([R.process(x[r].numpy(), hists[r], cfg) for r in range(2)])
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_op_refuses_what_the_kernel_cannot_hold():
    from vz_hip import binding as B
    from vz_hip.logits_proc import ProcConfig
    with pytest.raises(ValueError):
        B.logits_process(torch.zeros(1, 65537, device="cuda"), ProcConfig(penalty=1.3))
    with pytest.raises(ValueError):
        B.logits_process(torch.zeros(1, 100, device="cuda"), ProcConfig(ngram=9))


# ---- generate ----------------------------------------------------------------------------------------------------------------

def _hf_config():
    from vz_hip import synth
    from vis_zephyr.model import VisZephyrConfig
    cfg = synth.ArchConfig(n_layers=2)
    hf = VisZephyrConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=2, num_attention_heads=32,
                         num_key_value_heads=8, vocab_size=cfg.vocab, rms_norm_eps=1e-5, sliding_window=4096, eos_token_id=2, pad_token_id=2)
    hf.mm_vision_tower = "openai/clip-vit-large-patch14-336"
    hf.mm_patch_merge_type = "flat"
    return cfg, hf


@pytest.fixture(scope="module")
def random_model():
    """the 2-layer synthetic model of tests/test_sampling_gpu.py (with 4 cache rows)"""
    from vis_zephyr.model import VisZephyrForCausalLM
    return VisZephyrForCausalLM.from_synthetic(_hf_config()[1], seed=0, max_batch=4, max_ctx=256, max_tiles=1, max_text=32)


@pytest.fixture(scope="module")
def model():
    """The same synthetic model with an lm_head that makes greedy decoding LOOP, as a trained chat model does.  The penalty and the
    n-gram processor can only change a run that repeats itself, and the plain greedy runs of the random-weight model never do: measured
    for the synthetic seeds 0, 1, 2, 3 and four prompts each, 32 new tokens hold 32 distinct ids every time (a random function of a
    32000-token vocabulary).  So: the embedding rows are scaled by 8 (the current token dominates the residual stream) and lm_head row v =
    0.02 * (E[pi^-1(v)] + 0.85 * E[rho^-1(v)]) with pi = the 4-cycle inside every aligned block of four ids and rho(c) = c + 28: after
    token c the best next id is pi(c), the runner-up rho(c) at 0.85 of its logit.  The plain run therefore cycles with period 4 (repeated
    tokens and bigrams from the fifth id on); a penalty of 1.3 (1 / 1.3 < 0.85) or a banned bigram sends the run to rho(c)."""
    from vz_hip import synth
    from vis_zephyr.model import VisZephyrForCausalLM
    cfg, hf = _hf_config()
    m = VisZephyrForCausalLM(hf, max_batch=4, max_ctx=256, max_tiles=1, max_text=32)

    def named():
        E = None
        for name, t in synth.iter_state_dict(cfg, 0, device=m.engine.device):
            if name == "model.embed_tokens.weight":
                E = t.float()
                t = t * 8
            elif name == "lm_head.weight":
                v = torch.arange(cfg.vocab, device=t.device)
                t = 0.02 * (E[(v & ~3) | ((v + 3) & 3)] + 0.85 * E[(v - 28) % cfg.vocab])
            yield name, t

    m.engine.load_weights(named())
    m.engine.init_comm()
    if m.get_vision_tower() is not None:
        m.get_vision_tower().is_loaded = True
    return m


@pytest.fixture(scope="module")
def prompt():
    from vz_hip import synth
    return synth.synth_ids(12, 32000, image_pos=-1, seed=21).unsqueeze(0)


def _parse(kw, eos):
    from vz_hip import logits_proc as LP
    return LP.parse(kw.get("repetition_penalty"), kw.get("no_repeat_ngram_size"), kw.get("min_new_tokens"), kw.get("suppress_tokens"), eos)


def _host_loop(model, ids, seqlens, cfg, eos=(), max_new=NEW):
    """greedy ids of the rows of `ids` [B, S] (right-padded to seqlens) from un-armed engine calls: prefill, then one eager decode step per
    token with its raw logits read back; the processors run on the host (logits_proc_ref)."""
    eng = model.engine
    Bn = ids.shape[0]
    emb = model.get_model().embed_tokens(ids.to(model.device))
    _, last = eng.prefill(emb, seqlens, None, all_logits=False, last_logits=True)
    out = [[] for _ in range(Bn)]

    def choose(lg):
        toks = []
        for b in range(Bn):
            x = lg[b].cpu().numpy()
            if cfg is not None:
                x = R.process(x, out[b], cfg)
            toks.append(int(np.argmax(x)))          # first maximal index, as the argmax kernel
            out[b].append(toks[-1])
        return toks

    toks = choose(last)
    for t in range(1, max_new):
        if Bn == 1 and toks[0] in eos:
            break
        eng.decode_begin(torch.tensor(toks, dtype=torch.int32), [l + t - 1 for l in seqlens], [l + t - 1 for l in seqlens])
        _, lg = eng.decode_steps(1, return_logits=True)
        toks = choose(lg[0])
    return out


@pytest.fixture(scope="module")
def plain(model, prompt):
    """the plain greedy run; the penalty case needs a repeated token in it, the n-gram case a repeated bigram"""
    ids = model.generate(input_ids=prompt, do_sample=False, max_new_tokens=NEW, eos_token_id=[])[0].tolist()
    assert len(ids) == NEW and ids == _host_loop(model, prompt, [12], None)[0]
    bigrams = list(zip(ids, ids[1:]))
    assert len(set(ids)) < len(ids), f"no repeated token in {ids}"
    assert len(set(bigrams)) < len(bigrams), f"no repeated bigram in {ids}"
    return ids


def _cases(plain):
    return {
        "penalty": (dict(repetition_penalty=1.3), []),
        "ngram": (dict(no_repeat_ngram_size=2), []),
        "min_new": (dict(min_new_tokens=8), [plain[1]]),
        "suppress": (dict(suppress_tokens=[plain[0]]), []),
        "all": (dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=8, suppress_tokens=[plain[0]]), [plain[1]]),
    }


@pytest.fixture(scope="module")
def refs(model, prompt, plain):
    """the host-loop ids of every keyword set, computed once"""
    out = {}
    for name, (kw, eos) in _cases(plain).items():
        out[name] = _host_loop(model, prompt, [12], _parse(kw, eos), eos)[0]
    return out


def _plain_with(plain, eos):
    return plain if not eos else plain[:plain.index(eos[0]) + 1]


class _Streamer:
    def __init__(self):
        self.puts, self.ended = [], False

    def put(self, v):
        self.puts.append(v.reshape(-1).tolist())

    def end(self):
        self.ended = True


@pytest.mark.parametrize("name", ["penalty", "ngram", "min_new", "suppress", "all"])
def test_generate_equals_host_loop(model, prompt, plain, refs, name):
    kw, eos = _cases(plain)[name]
    want = refs[name]
    assert want != _plain_with(plain, eos), f"{name}: the processors do not change the plain run {plain}"
    if name == "min_new":
        assert len(_plain_with(plain, eos)) == 2 and len(want) >= 8 and plain[1] not in want[:8]
    got = model.generate(input_ids=prompt, do_sample=False, max_new_tokens=NEW, eos_token_id=eos, **kw)[0].tolist()
    print(name, "plain", plain, "reference", want, "generate", got)
    assert got == want
    # streamer + stopping criteria: one step in flight, tokens through the host-visible ring
    st = _Streamer()
    seen = []
    s = model.generate(input_ids=prompt, do_sample=False, max_new_tokens=NEW, eos_token_id=eos, streamer=st,
                       stopping_criteria=[lambda i, sc, **k: seen.append(i.shape[1]) or False], **kw)[0].tolist()
    assert s == want and st.ended and st.puts[0] == [] and [p[0] for p in st.puts[1:]] == want


def test_prompt_lookup_with_processors_takes_the_plain_path(model, prompt, plain, refs):
    got = model.generate(input_ids=prompt, do_sample=False, max_new_tokens=NEW, eos_token_id=[], prompt_lookup_num_tokens=3,
                         repetition_penalty=1.3)[0].tolist()
    assert got == refs["penalty"]


def test_batched_generate_equals_host_loop(model):
    from vz_hip import synth
    lens = [12, 9, 5]
    ids = torch.full((3, 12), 5, dtype=torch.long)
    mask = torch.zeros(3, 12, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = synth.synth_ids(n, 32000, image_pos=-1, seed=30 + b)
        mask[b, :n] = 1
    base = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, max_new_tokens=NEW, eos_token_id=[]).tolist()
    assert base == _host_loop(model, ids, lens, None)
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[base[0][0], base[1][0], base[2][0]])
    want = _host_loop(model, ids, lens, _parse(kw, []))
    got = model.generate(input_ids=ids, attention_mask=mask, do_sample=False, max_new_tokens=NEW, eos_token_id=[], **kw).tolist()
    assert got == want
    for b in range(3):
        assert got[b] != base[b] and got[b][0] != base[b][0]


def test_sampled_generate_honours_the_processors(random_model, prompt):
    model = random_model
    kw = dict(input_ids=prompt, do_sample=True, temperature=0.8, max_new_tokens=NEW, eos_token_id=[])
    base = model.generate(seed=1000, **kw)[0].tolist()
    t0 = base[0]
    for seed in range(1000, 1004):
        ids = model.generate(seed=seed, suppress_tokens=[t0], **kw)[0].tolist()
        assert len(ids) == NEW and t0 not in ids
        if seed == 1000:
            assert ids[0] != t0
    eos = list(dict.fromkeys(base[:8]))[:4]          # ids the plain sampled run emits among its first 8
    ids = model.generate(**{**kw, "eos_token_id": eos}, seed=1000, min_new_tokens=8)[0].tolist()
    assert len(ids) >= 8 and not set(eos) & set(ids[:8])
    assert len(model.generate(**{**kw, "eos_token_id": eos}, seed=1000)[0].tolist()) == 1


def test_parameters_are_part_of_the_graph_key(model, prompt, plain):
    eng = model.engine
    kw = dict(input_ids=prompt, do_sample=False, max_new_tokens=NEW, eos_token_id=[])
    a = model.generate(repetition_penalty=1.3, **kw)[0].tolist()
    c0 = eng.decode_info()[1]
    b = model.generate(repetition_penalty=1.7, **kw)[0].tolist()
    c1 = eng.decode_info()[1]
    assert c1 > c0, "another penalty must capture the step again"
    assert a == _host_loop(model, prompt, [12], _parse(dict(repetition_penalty=1.3), []))[0]
    assert b == _host_loop(model, prompt, [12], _parse(dict(repetition_penalty=1.7), []))[0]
    # disarmed afterwards: the plain call is the plain run, the history is not consulted
    assert model.generate(**kw)[0].tolist() == plain


def test_refusals(model, prompt):
    with pytest.raises(NotImplementedError):
        model.generate(input_ids=prompt, num_beams=2, repetition_penalty=1.2, max_new_tokens=4)
    with pytest.raises(ValueError):
        model.generate(input_ids=prompt, repetition_penalty=2, max_new_tokens=4)
    # the engine checks what it is armed with itself
    from vz_hip import binding as B
    eng = model.engine
    for bad in ((0.0, 0, 0), (1.2, 9, 0), (1.2, -1, 0), (1.2, 0, -1)):
        with pytest.raises(ValueError):
            B.check(eng.lib.vz_llm_decode_logits_proc(eng.h, B.C.byref(B.VzLogitsProcParams(bad[0], bad[1], bad[2], 0, 0, 0, None, None, None)), None))
    ids = (B.C.c_int * 17)(*range(17))
    with pytest.raises(ValueError):
        B.check(eng.lib.vz_llm_decode_logits_proc(eng.h, B.C.byref(B.VzLogitsProcParams(1.2, 0, 0, 5, 0, 0, ids, None, None)), None))
    with pytest.raises(ValueError):
        B.check(eng.lib.vz_llm_decode_logits_proc(eng.h, B.C.byref(B.VzLogitsProcParams(1.2, 0, 0, 0, 17, 0, None, ids, None)), None))
