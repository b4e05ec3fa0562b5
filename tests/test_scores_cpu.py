"""The host side of the step recorder (vz_hip/scores.py): records of chunks and rings put together as [rows, T], positions behind a row's
eos masked, `transition_scores` against HF's own `compute_transition_scores`, and how generate() / generate_stream read their keywords."""
import pytest
import torch

from vz_hip import scores as SC


def _rec(n, rows, seed):
    """records [n, rows, 4] with distinct values: x_tok, lse, lse_kept random, n_kept = an int32 in the fourth word"""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(n, rows, 4, generator=g)
    r.view(torch.int32)[..., 3] = torch.randint(1, 32000, (n, rows), generator=g, dtype=torch.int32)
    return r


def test_unpack_reads_the_count_as_int():
    r = _rec(3, 2, 0)
    x, lse, lk, nk = SC.unpack(r)
    assert nk.dtype == torch.int32 and int(nk.min()) >= 1 and torch.equal(x, r[..., 0]) and torch.equal(lse, r[..., 1]) and torch.equal(lk, r[..., 2])


def test_assemble_chunks_of_unequal_length():
    chunks = [_rec(1, 3, 1), _rec(4, 3, 2), _rec(2, 3, 3)]
    full = torch.cat(chunks, 0)                       # [7, 3, 4]
    got = SC.assemble(chunks)
    assert tuple(got.shape) == (3, 7, 4) and torch.equal(got, full.transpose(0, 1))
    assert torch.equal(SC.assemble(chunks, T=5), full[:5].transpose(0, 1))          # steps behind the end of the generation are cut
    padded = SC.assemble(chunks, T=9)
    assert tuple(padded.shape) == (3, 9, 4) and torch.equal(padded[:, :7], full.transpose(0, 1)) and not bool(padded[:, 7:].any())


def test_ring_wrap():
    cap, rows = 5, 2
    steps = _rec(12, rows, 4)
    ring = torch.zeros(cap, rows, 4)
    for t in range(12):
        ring[t % cap] = steps[t]
    assert torch.equal(SC.ring_order(ring, 12, 5), steps[7:12])
    assert torch.equal(SC.ring_order(ring, 12, 3), steps[9:12])
    assert torch.equal(SC.ring_order(ring, 12, 2, first=8), steps[8:10])
    assert SC.ring_order(ring, 12, 0).shape[0] == 0
    with pytest.raises(ValueError):
        SC.ring_order(ring, 12, 6)                    # step 6 was overwritten
    with pytest.raises(ValueError):
        SC.ring_order(ring, 3, 4)                     # more than were written
    # before the ring has wrapped
    assert torch.equal(SC.ring_order(ring[:], 4, 4)[3], ring[3])


def test_eos_mask_and_logprobs():
    ids = torch.tensor([[2, 9, 9, 9],        # ends on its first token
                        [5, 6, 2, 2],        # eos in the middle (the pad id is the eos id)
                        [5, 6, 4, 8],        # never ends
                        [5, 7, 6, 2]])       # ends on its last token; 7 is the second eos id
    m = SC.behind_eos(ids, {2, 7})
    assert m.tolist() == [[False, True, True, True], [False, False, False, True], [False] * 4, [False, False, True, True]]
    assert not bool(SC.behind_eos(ids, set()).any())
    rec = _rec(4, 4, 5).transpose(0, 1).contiguous()          # [rows, T, 4]
    temps = torch.tensor([1.0, 0.7, 1.3, 0.2])
    lp, lpw = SC.logprobs(rec, temps, m)
    x, lse, lk, _ = SC.unpack(rec)
    assert torch.equal(lp[~m], (x - lse)[~m]) and torch.equal(lpw[~m], (x / temps.view(4, 1) - lk)[~m])
    assert not bool(lp[m].any()) and not bool(lpw[m].any()) and lp.dtype == torch.float32
    lp1, _ = SC.logprobs(rec, 1.0)
    assert torch.equal(lp1, x - lse)


def test_sink_puts_blocks_together():
    """two blocks: three rows that decoded together (first token + chunks of 2 and 3 steps, one more step than the ids show) and one row
    that decoded alone and stopped after 2 tokens"""
    V = 11
    g = torch.Generator().manual_seed(6)
    sink = SC.Sink(SC.SCORE_REC | SC.SCORE_WARPED)
    assert sink.warped and not sink.raw
    a = sink.block(3, 1.0)
    ra, wa = [_rec(n, 3, 10 + n) for n in (1, 2, 3)], [torch.randn(n, 3, V, generator=g) for n in (1, 2, 3)]
    for r, w in zip(ra, wa):
        a.add(r, w)
    b = sink.block(1, 0.5)
    rb, wb = [_rec(n, 1, 20 + n) for n in (1, 1)], [torch.randn(n, 1, V, generator=g) for n in (1, 1)]
    for r, w in zip(rb, wb):
        b.add(r, w)
    ids = torch.tensor([[5, 6, 7, 8, 9], [5, 2, 2, 2, 2], [2, 2, 2, 2, 2], [4, 3, 2, 2, 2]])
    out = sink.finish(ids, {2})
    assert out["logits"] is None and len(out["scores"]) == 5 and all(tuple(s.shape) == (4, V) for s in out["scores"])
    full_a, full_b = torch.cat(ra, 0)[:5], torch.cat(rb, 0)
    lp = out["token_logprobs"]
    assert tuple(lp.shape) == (4, 5)
    assert torch.equal(lp[0], full_a[:, 0, 0] - full_a[:, 0, 1])
    assert lp[1, :2].tolist() == (full_a[:2, 1, 0] - full_a[:2, 1, 1]).tolist() and lp[1, 2:].tolist() == [0.0] * 3
    assert lp[2, 0] == full_a[0, 2, 0] - full_a[0, 2, 1] and lp[2, 1:].tolist() == [0.0] * 4          # ended on its first token
    assert lp[3, :2].tolist() == (full_b[:, 0, 0] - full_b[:, 0, 1]).tolist() and lp[3, 2:].tolist() == [0.0] * 3
    lpw = out["token_logprobs_warped"]
    assert lpw[3, :2].tolist() == (full_b[:, 0, 0] / 0.5 - full_b[:, 0, 2]).tolist() and lpw[0].tolist() == (full_a[:, 0, 0] - full_a[:, 0, 2]).tolist()
    sa = torch.cat(wa, 0)
    for t in range(5):
        assert torch.equal(out["scores"][t][:3], sa[t])
    assert torch.equal(out["scores"][1][3], torch.cat(wb, 0)[1, 0]) and not bool(out["scores"][3][3].any())


@pytest.mark.parametrize("normalize", [False, True])
def test_transition_scores_equal_hf(normalize):
    from transformers import GenerationMixin
    T, Bn, V = 7, 3, 50
    g = torch.Generator().manual_seed(7)
    scores = []
    for t in range(T):
        s = torch.randn(Bn, V, generator=g) * 3
        s[torch.rand(Bn, V, generator=g) < 0.3] = float("-inf")
        scores.append(s)
    seq = torch.stack([torch.stack([torch.nonzero(torch.isfinite(scores[t][b]))[t % 3, 0] for t in range(T)]) for b in range(Bn)])
    seq = torch.cat([torch.randint(0, V, (Bn, 4), generator=g), seq], 1)          # HF takes the last len(scores) columns

    class _M(GenerationMixin):
        class config:
            vocab_size = V
            is_encoder_decoder = False

            @staticmethod
            def get_text_config(decoder=False):
                return _M.config

    want = GenerationMixin.compute_transition_scores(_M(), seq, tuple(scores), normalize_logits=normalize)
    got = SC.transition_scores(seq, tuple(scores), normalize_logits=normalize)
    assert got.dtype == torch.float32 and tuple(got.shape) == (Bn, T) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
    assert torch.equal(SC.transition_scores(seq[:, 4:], tuple(scores), normalize_logits=normalize), want)
    with pytest.raises(NotImplementedError):
        SC.transition_scores(seq, tuple(scores), beam_indices=torch.zeros(Bn, T, dtype=torch.long))


def test_keywords():
    # as in HF, the output_* keywords without return_dict_in_generate return the plain tensor: nothing is recorded
    assert SC.check_outputs(False, True, True, True) == 0
    assert SC.check_outputs(True, False, False, False) == 0
    assert SC.check_outputs(True, False, False, True) == SC.SCORE_REC
    assert SC.check_outputs(True, True, False, False) == SC.SCORE_REC | SC.SCORE_WARPED
    assert SC.check_outputs(True, True, True, True) == SC.SCORE_REC | SC.SCORE_WARPED | SC.SCORE_RAW
    assert SC.check_outputs(True, False, False, False, num_beams=3) == 0
    for kw in ((True, False, False), (False, True, False), (False, False, True)):
        with pytest.raises(NotImplementedError):
            SC.check_outputs(True, *kw, num_beams=3)
    assert (SC.SCORE_REC, SC.SCORE_WARPED, SC.SCORE_RAW) == (1, 2, 4)
    from vz_hip import binding
    assert (binding.SCORE_REC, binding.SCORE_WARPED, binding.SCORE_RAW) == (1, 2, 4)


def test_request_parsing():
    assert SC.wants_logprobs({"logprobs": True}) and SC.wants_logprobs({"logprobs": 1})
    assert not SC.wants_logprobs({}) and not SC.wants_logprobs({"logprobs": False}) and not SC.wants_logprobs({"logprobs": None})
    for bad in (5, "yes", 0.5):
        with pytest.raises(ValueError):
            SC.wants_logprobs({"logprobs": bad})


def test_output_objects():
    from transformers.generation.utils import GenerateBeamDecoderOnlyOutput, GenerateDecoderOnlyOutput
    Scored, Beam = SC.output_classes()
    assert issubclass(Scored, GenerateDecoderOnlyOutput) and Beam is GenerateBeamDecoderOnlyOutput
    ids = torch.zeros(2, 3, dtype=torch.long)
    o = Scored(sequences=ids, token_logprobs=torch.zeros(2, 3))
    assert o.sequences is ids and o.scores is None and o.token_logprobs_warped is None and "token_logprobs" in o.keys()
    assert SC.output_classes()[0] is Scored
