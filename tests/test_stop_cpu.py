"""The host side of the stop matcher (vz_hip/stop.py): what `parse` hands to the device and what it leaves on the host, and the checks
downstream of it that ask "are there stopping criteria?" (they see the host's remainder only)."""
import pytest
import torch

import stop_ref as R
from vz_hip import stop as ST


def _hf(tok, strings):
    from transformers.generation.stopping_criteria import StopStringCriteria
    return StopStringCriteria(tok, strings)


def test_standin_tokenizer_gives_the_documented_tables():
    tok = R.small_tokenizer()
    c = _hf(tok, R.STOPS)
    assert len(R.VOCAB) == 46 and c.maximum_token_len == 8 and c.max_valid_positions == 3 and c.max_valid_end_lens == 2
    assert tuple(c.embedding_vec.shape) == (47, 26) and c.num_stop_strings == 5


def test_parse_nothing_asked():
    assert ST.parse(None, None, None) == (None, None)
    assert ST.parse(None, R.small_tokenizer(), []) == (None, None)
    assert ST.parse([], None, None) == (None, None)


def test_parse_raises_without_tokenizer():
    from types import SimpleNamespace
    with pytest.raises(ValueError, match="tokenizer"):
        ST.parse(["abc"], None, None)
    with pytest.raises(ValueError, match="tokenizer"):
        ST.parse(None, None, None, SimpleNamespace(stop_strings=["abc"]))          # HF's fallback to the generation config


def test_parse_tables_are_hfs_verbatim():
    tok = R.small_tokenizer()
    c = _hf(tok, R.STOPS)
    for plan, host in (ST.parse(R.STOPS, tok, None), ST.parse(None, None, [c]), ST.parse("abc", tok, None)):
        assert host is None and plan is not None and not plan.seqs
    plan, _ = ST.parse(R.STOPS, tok, None)
    assert plan.emb.dtype == torch.int32 and torch.equal(plan.emb, c.embedding_vec.to(torch.int32)) and torch.equal(plan.target, c.target_lens)
    assert (plan.n_str, plan.max_pos, plan.max_end, plan.window, plan.vec) == (5, c.max_valid_positions, c.max_valid_end_lens, c.maximum_token_len, 26)
    one, _ = ST.parse("abc", tok, None)
    assert one.n_str == 1 and one.window == 3


def test_parse_keywords_become_id_sequences():
    from vis_zephyr.model.mm_utils import KeywordsStoppingCriteria
    tok = R.small_tokenizer()
    k = KeywordsStoppingCriteria(["xy", "ab"], tok, torch.zeros(1, 3, dtype=torch.long))
    plan, host = ST.parse(None, None, [k])
    assert host is None and plan.n_str == 0 and plan.emb is None
    assert plan.seqs == [(tok.ids("x", "y"), 3), (tok.ids("ab"), 3)]
    t = plan.seq_table()
    assert t.dtype == torch.int32 and tuple(t.shape) == (2, ST.SEQ_STRIDE)
    assert t[0, :4].tolist() == [2, 3] + tok.ids("y", "x") and t[1, :3].tolist() == [1, 3] + tok.ids("ab")          # newest id first
    both, host = ST.parse(R.STOPS, tok, [k])
    assert host is None and both.n_str == 5 and len(both.seqs) == 2
    seqs, host = ST.parse(None, None, None, token_sequences=[[5, 6, 7]])
    assert host is None and seqs.seqs == [([5, 6, 7], 0)]


def test_parse_unknown_criterion_keeps_everything_on_the_host():
    tok = R.small_tokenizer()
    k = R.keyword_criterion([[4, 5]], 0)
    lam = lambda ids, scores, **kw: False      # noqa: E731
    plan, host = ST.parse(None, None, [k, lam])
    assert plan is None and host == [k, lam]
    plan, host = ST.parse(None, None, lam)          # a bare callable, as generate() has always taken
    assert plan is None and host == [lam]
    plan, host = ST.parse(["abc"], tok, [lam])      # stop strings by keyword join the host list: never dropped
    assert plan is None and host[0] is lam and len(host) == 2 and type(host[1]).__name__ == "StopStringCriteria"
    plan, host = ST.parse(["abc"], tok, [k], device_stop=False)
    assert plan is None and host[0] is k and len(host) == 2


def test_parse_falls_back_at_each_limit():
    tok = R.small_tokenizer()
    ok = lambda *a, **kw: ST.parse(*a, **kw)[0] is not None      # noqa: E731
    # 8 stop strings
    eight = ["abc", "ab", "bc", "cd", "def", "user", "us", "er"]
    assert ok(eight, tok, None) and not ok(eight + ["aa"], tok, None)
    # maximum_token_len <= 64
    s64 = "abcdef" * 10 + "abcd"
    assert len(s64) == 64 and ok([s64], tok, None) and ST.parse([s64], tok, None)[0].window == 64
    c = _hf(tok, ["abcdef" * 11])
    assert c.maximum_token_len == 66 and c.max_valid_positions <= ST.MAX_POS and c.max_valid_end_lens <= ST.MAX_END and not ok(["abcdef" * 11], tok, None)
    # max_valid_positions <= 16: a one-character token that fits 20 places of the string
    c = _hf(tok, ["a" * 21])
    assert c.max_valid_positions > ST.MAX_POS and not ok(["a" * 21], tok, None)
    assert ok(["a" * 17], tok, None) and _hf(tok, ["a" * 17]).max_valid_positions == 16
    # max_valid_end_lens <= 8: nine tokens that are a run of one character
    runs = R.SelfTokenizer(["abcdef", "x"] + ["a" * n for n in range(1, 11)])
    c = _hf(runs, ["a" * 10])
    assert c.max_valid_end_lens > ST.MAX_END and not ok(["a" * 10], runs, None)
    # 16 id sequences of at most 32 ids
    k16 = R.keyword_criterion([[i, i + 1] for i in range(16)], 0)
    k17 = R.keyword_criterion([[i, i + 1] for i in range(17)], 0)
    assert ok(None, None, [k16]) and not ok(None, None, [k17])
    assert ok(None, None, [R.keyword_criterion([list(range(32))], 0)]) and not ok(None, None, [R.keyword_criterion([list(range(33))], 0)])
    # two sets of stop strings: one table on the device
    assert not ok(["abc"], tok, [_hf(tok, ["def"])])
    # and the fallback is the host list, complete
    plan, host = ST.parse(None, None, [k17])
    assert plan is None and host == [k17]


def test_downstream_checks_see_the_host_remainder():
    from vz_hip import sample_rows, spec
    lam = lambda ids, scores, **kw: False      # noqa: E731
    kw = dict(n_seq=1, greedy=True, num_beams=1, streamer=None, tp_size=1, max_batch=6, prompt_len=10, max_new=16, max_ctx=256)
    _, host = ST.parse(None, None, [lam])
    with pytest.raises(NotImplementedError):
        sample_rows.check_return_sequences(3, False, 6, None, host)
    assert spec.draft_slots(4, 2, stopping_criteria=host, **kw) == 0
    plan, host = ST.parse(None, None, [R.keyword_criterion([[4, 5]], 0)])
    assert plan is not None and host is None
    assert sample_rows.check_return_sequences(3, False, 6, None, host) == 3
    assert spec.draft_slots(4, 2, stopping_criteria=host, **kw) > 0


def test_oracle_first_hits_of_the_scripted_rows():
    """the table of the issue: HF's first hits on the scripted token rows (behind the quiet prefix `x yz`)"""
    tok = R.small_tokenizer()
    c = _hf(tok, R.STOPS)
    rows = {("<|", "user", "|>"): 2, ("<", "|", "u", "s", "e", "r", "|", ">"): 7, ("<", "|user|", ">\n"): 2, ("<|", "us", "e", "r|>x"): 3,
            ("<", "/", "s", ">"): 3, ("</", "s>"): 1, ("</s>",): 0, ("ab", "ab", "ab"): 2, ("aba", "bab"): 1, ("aa", "bab", "ab"): 2,
            ("ab", "ab", "abc"): 2, ("abcdef",): 0}
    for toks, want in rows.items():
        assert R.first_hit(c, tok.ids("x", "yz", *toks)) == want + 2, toks
    for toks in (("ab", "ab", "x", "ab"), ("<|", "user", "|", "x", ">"), ("</", "x", "s>"), ("ab", "ab", "a"), ("<", "|", "u", "s", "e", "r", "|", "y", ">")):
        assert R.first_hit(c, tok.ids("x", "yz", *toks)) == -1, toks


def test_token_sequences_are_never_dropped():
    """id lists have no host criterion to fall back to: what the device cannot take raises instead of returning (None, None)"""
    tok = R.small_tokenizer()
    plan, host = ST.parse(None, None, None, None, True, [[1, 2]] * 16)
    assert host is None and len(plan.seqs) == 16
    with pytest.raises(ValueError, match="16"):
        ST.parse(None, None, None, None, True, [[1, 2]] * 17)
    with pytest.raises(ValueError):
        ST.parse(None, None, None, None, True, [list(range(33))])
    with pytest.raises(ValueError):
        ST.parse(None, None, None, None, True, [[]])
    # together with a stop set that stays on the host (beyond a limit, or a keyword criterion that fills the 16 slots)
    with pytest.raises(NotImplementedError):
        ST.parse(["a" * 21], tok, None, None, True, [[1, 2]])
    with pytest.raises(NotImplementedError):
        ST.parse(None, None, [R.keyword_criterion([[i, i + 1] for i in range(16)], 0)], None, True, [[1, 2]])
    with pytest.raises(NotImplementedError):
        ST.parse(None, None, None, None, False, [[1, 2]])


def test_subclasses_stay_on_the_host():
    """a subclass may override __call__: only the two classes themselves are re-expressed on the device"""
    from transformers.generation.stopping_criteria import StopStringCriteria
    from vis_zephyr.model.mm_utils import KeywordsStoppingCriteria
    tok = R.small_tokenizer()

    class Mine(KeywordsStoppingCriteria):
        def __call__(self, output_ids, scores=None, **kw):
            return False

    class Theirs(StopStringCriteria):
        pass

    for c in (Mine(["ab"], tok, torch.zeros(1, 0, dtype=torch.long)), Theirs(tok, ["abc"])):
        plan, host = ST.parse(None, None, [c])
        assert plan is None and host == [c]
