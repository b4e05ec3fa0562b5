"""Per-row sampling without a GPU (vz_hip/sample_rows.py): how a generate_stream request's sampling parameters are read, the defaults,
the seed of sample j of prompt b, the chunking and the refusals - the host half of csrc/sampling.hip's per-row tail."""
import types

import pytest

from vz_hip import sample_rows as SR


GEN = types.SimpleNamespace(top_k=50, top_p=1.0)          # the model's generation config, as far as sampling reads it


def _never():
    raise AssertionError("a seed was drawn for a request that needs none")


def test_request_defaults_are_generates():
    """no sampling key = greedy; do_sample with only a temperature = the generation config's top_k (50) and top_p (1.0)"""
    assert SR.parse_request({"input_ids": None}, GEN, _never) == SR.GREEDY
    assert not SR.GREEDY.sample and SR.GREEDY.counter == 0
    p = SR.parse_request({"do_sample": True, "temperature": 0.2, "seed": 7}, GEN, _never)
    assert p == SR.RowParams(True, 0.2, 50, 1.0, 7, 0)
    # temperature defaults to 1.0, as generate's keyword does
    assert SR.parse_request({"do_sample": True, "seed": 1}, GEN, _never).temperature == 1.0
    # the generation config's values are the caller's: another config, other defaults
    q = SR.parse_request({"do_sample": True, "seed": 1}, types.SimpleNamespace(top_k=20, top_p=0.8), _never)
    assert (q.top_k, q.top_p) == (20, 0.8)


@pytest.mark.parametrize("req", [{"do_sample": False, "temperature": 0.7, "seed": 3}, {"do_sample": True, "temperature": 0.0},
                                 {"do_sample": True, "temperature": None}, {"do_sample": True, "temperature": -1.0},
                                 {"temperature": 0.7, "top_p": 0.9}])
def test_requests_that_mean_greedy(req):
    assert SR.parse_request(req, GEN, _never) == SR.GREEDY


def test_named_top_k_and_top_p():
    base = {"do_sample": True, "temperature": 0.7, "seed": 5}
    assert SR.parse_request({**base, "top_k": 5, "top_p": 0.3}, GEN, _never) == SR.RowParams(True, 0.7, 5, 0.3, 5, 0)
    # top_k None / 0 = no filter (0 in the table); top_p None = the generation config's
    assert SR.parse_request({**base, "top_k": None}, GEN, _never).top_k == 0
    assert SR.parse_request({**base, "top_k": 0}, GEN, _never).top_k == 0
    assert SR.parse_request({**base, "top_p": None}, types.SimpleNamespace(top_k=50, top_p=0.9), _never).top_p == 0.9
    for bad in ({"top_k": -2}, {"top_p": 0.0}, {"top_p": 1.5}):
        with pytest.raises(ValueError):
            SR.parse_request({**base, **bad}, GEN, _never)


def test_missing_seed_is_drawn_once_per_sampled_request():
    drawn = []

    def draw():
        drawn.append(1)
        return 1234 + len(drawn)
    a = SR.parse_request({"do_sample": True, "temperature": 0.5}, GEN, draw)
    b = SR.parse_request({"do_sample": True, "temperature": 0.5}, GEN, draw)
    assert (a.seed, b.seed) == (1235, 1236) and len(drawn) == 2
    SR.parse_request({"do_sample": True, "temperature": 0.5, "seed": 9}, GEN, _never)      # a named seed draws nothing


@pytest.mark.parametrize("key,val", [("repetition_penalty", 1.2), ("no_repeat_ngram_size", 2), ("min_new_tokens", 3), ("suppress_tokens", [5])])
def test_processors_in_a_request_are_refused(key, val):
    with pytest.raises(NotImplementedError, match=key):
        SR.parse_request({"do_sample": True, "temperature": 0.7, "seed": 1, key: val}, GEN, _never)
    assert SR.parse_request({key: None}, None, _never) == SR.GREEDY            # named but empty: nothing asked for; greedy reads no config


def test_counter_steps_with_the_row():
    p = SR.RowParams(True, 0.7, 50, 0.9, 11, 0)
    assert p.at(1) == SR.RowParams(True, 0.7, 50, 0.9, 11, 1) and p.counter == 0


def test_seed_rule():
    """row j of prompt b: seed + b * n + j; n = 1 is the sequential sampled batch's seed + b"""
    assert [SR.row_seed(100, b, 1, 0) for b in range(3)] == [100, 101, 102]
    assert [SR.row_seed(100, b, 4, j) for b in range(2) for j in range(4)] == list(range(100, 108))
    seeds = {SR.row_seed(7, b, 3, j) for b in range(5) for j in range(3)}
    assert len(seeds) == 15


def test_return_sequences_refusals():
    assert SR.check_return_sequences(1, True, 4) == 1                     # n = 1: every existing path, greedy included
    assert SR.check_return_sequences(1, False, 4, streamer=object()) == 1
    assert SR.check_return_sequences(None, True, 4) == 1                  # not named
    assert SR.check_return_sequences(4, False, 4) == 4
    with pytest.raises(ValueError, match="Greedy methods without beam search do not support `num_return_sequences` different than 1"):
        SR.check_return_sequences(2, True, 4)
    with pytest.raises(NotImplementedError):
        SR.check_return_sequences(2, False, 4, streamer=object())
    with pytest.raises(NotImplementedError):
        SR.check_return_sequences(2, False, 4, stopping_criteria=[lambda *a: False])
    with pytest.raises(ValueError, match="exceeds"):
        SR.check_return_sequences(5, False, 4)
    with pytest.raises(ValueError, match="exceeds"):
        SR.check_return_sequences(65, False, 128)                          # 64 rows decode together at the most
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            SR.check_return_sequences(bad, False, 4)


def test_prompts_per_chunk():
    """chunk * n <= min(max_batch, 64)"""
    assert SR.prompts_per_chunk(4, 4) == 1 and SR.prompts_per_chunk(2, 4) == 2 and SR.prompts_per_chunk(3, 8) == 2
    assert SR.prompts_per_chunk(4, 128) == 16 and SR.prompts_per_chunk(64, 128) == 1
    for n in range(1, 65):
        for cap in (1, 6, 64, 100):
            if n <= min(cap, 64):
                assert 1 <= SR.prompts_per_chunk(n, cap) * n <= min(cap, 64)
