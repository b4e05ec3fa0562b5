"""generate_stream(per_request=True) without a GPU: what a request may carry with and without the flag, the
vz_proc_row record byte by byte against the offsets include/viszephyr.h documents, the row's sequence region, and the limit the call's and a
request's stop sequences share."""
import struct
import types

import pytest

from vz_hip import logits_proc as LP
from vz_hip import sample_rows as SR
from vz_hip import stop as ST

GEN = types.SimpleNamespace(top_k=50, top_p=1.0)
_never = lambda: (_ for _ in ()).throw(AssertionError("no seed is drawn"))      # noqa: E731

PROC_KEYS = {"repetition_penalty": 1.3, "no_repeat_ngram_size": 2, "min_new_tokens": 3, "suppress_tokens": [5], "sequence_bias": {(7,): 2.0},
             "bad_words_ids": [[4, 9]]}


@pytest.mark.parametrize("key", list(PROC_KEYS) + ["stop_token_sequences"])
def test_without_the_flag_every_key_still_raises(key):
    val = PROC_KEYS.get(key, [[3, 4]])
    with pytest.raises(NotImplementedError):
        SR.parse_request({key: val}, GEN, _never)
    with pytest.raises(NotImplementedError):
        SR.parse_request({key: val}, GEN, _never, per_request=False)
    assert SR.parse_request({key: None}, GEN, _never) == SR.GREEDY           # named but empty: nothing asked for
    assert SR.parse_request({key: val}, GEN, _never, per_request=True) == SR.GREEDY      # with it the sampling side reads past them


def test_with_the_flag_a_request_parses_to_its_config():
    req = {"input_ids": None, "do_sample": True, "seed": 3, **PROC_KEYS}
    got = LP.parse_request(req, eos=[2, 11], vocab=32000)
    want = LP.parse(1.3, 2, 3, [5], [2, 11], {(7,): 2.0}, [[4, 9]], 32000)
    assert got == want and got is not None
    assert got.eos == (2, 11) and got.seq == (((7,), 2.0, False), ((4, 9), float("-inf"), True))
    assert SR.parse_request(req, GEN, _never, per_request=True).sample
    # a request that names none of the keys: an inactive record
    assert LP.parse_request({"input_ids": None, "do_sample": True, "temperature": 0.5}, eos=[2], vocab=32000) is None
    assert LP.parse_request({"repetition_penalty": 1.0, "no_repeat_ngram_size": 0}, eos=[2], vocab=32000) is None
    assert LP.parse_request({"min_new_tokens": 4}, eos=[], vocab=32000) is None          # HF builds that processor only with an eos id
    # HF's ValueErrors and the kernel's limits are `parse`'s
    with pytest.raises(ValueError, match="strictly positive float"):
        LP.parse_request({"repetition_penalty": 0.0}, eos=[2], vocab=32000)
    with pytest.raises(ValueError, match="vocabulary size"):
        LP.parse_request({"bad_words_ids": [[32000]]}, eos=[2], vocab=32000)
    with pytest.raises(NotImplementedError):
        LP.parse_request({"no_repeat_ngram_size": 9}, eos=[2], vocab=32000)
    with pytest.raises(NotImplementedError):
        LP.parse_request({"suppress_tokens": list(range(17))}, eos=[2], vocab=32000)


def test_record_bytes_at_the_documented_offsets():
    cfg = LP.ProcConfig(penalty=1.25, ngram=3, min_new=7, eos=(2, 11, 13), suppress=(5, 6), seq=(((7,), 2.0, False), ((4, 9), float("-inf"), True)))
    rec = LP.pack_row(cfg)
    assert len(rec) == LP.ROW_RECORD_BYTES == 128
    word = lambda off: struct.unpack_from("<i", rec, off)[0]      # noqa: E731
    assert struct.unpack_from("<f", rec, 0)[0] == 1.25            # 0   repetition_penalty
    assert word(4) == 3                                           # 4   no_repeat_ngram
    assert word(8) == 7                                           # 8   min_new_tokens
    assert word(12) == 3                                          # 12  n_eos
    assert [word(16 + 4 * i) for i in range(4)] == [2, 11, 13, -1]                  # 16  eos[4]
    assert word(32) == 2                                          # 32  n_suppress
    assert [word(36 + 4 * i) for i in range(16)] == [5, 6] + [-1] * 14              # 36  suppress[16]
    assert word(100) == 2                                         # 100 n_seq
    assert word(104) == 1                                         # 104 active
    assert rec[108:] == bytes(20)                                 # 108 reserved[5]
    assert LP.pack_row(None) == bytes(128)                        # an inactive record: active = 0
    # the ctypes record of the binding is the same 128 bytes, field by field
    from vz_hip import binding as B
    r = B.proc_row(cfg)
    assert B.C.sizeof(B.VzProcRow) == 128 and bytes(r) == rec
    assert (B.VzProcRow.repetition_penalty.offset, B.VzProcRow.no_repeat_ngram.offset, B.VzProcRow.min_new_tokens.offset, B.VzProcRow.n_eos.offset,
            B.VzProcRow.eos.offset, B.VzProcRow.n_suppress.offset, B.VzProcRow.suppress.offset, B.VzProcRow.n_seq.offset, B.VzProcRow.active.offset,
            B.VzProcRow.reserved.offset) == (0, 4, 8, 12, 16, 32, 36, 100, 104, 108)
    assert (r.no_repeat_ngram, r.min_new_tokens, r.n_eos, r.n_suppress, r.n_seq, r.active) == (3, 7, 3, 2, 2, 1)
    assert bytes(B.proc_row(None)) == bytes(128)


def test_row_sequence_region_is_the_configs_table():
    cfg = LP.parse(sequence_bias={(7,): 2.0, (3, 8): -1.5}, bad_words_ids=[[4, 9, 1]], eos=[2], vocab=100)
    region = LP.pack_row_seqs(cfg)
    assert region == cfg.seq_table() and len(region) == 3 * LP.SEQ_STRIDE
    assert region[:LP.SEQ_STRIDE] == [1, 0, struct.unpack("<i", struct.pack("<f", 2.0))[0], 0, 7, 0, 0, 0, 0, 0, 0, 0]
    assert region[2 * LP.SEQ_STRIDE:] == [3, 1, 0, 0, 4, 9, 1, 0, 0, 0, 0, 0]
    assert LP.pack_row_seqs(None) == [] and LP.pack_row_seqs(LP.ProcConfig(penalty=1.2)) == []


def test_stop_sequences_of_call_and_request_share_sixteen():
    assert ST.parse_row_sequences(None, 16) == [] and ST.parse_row_sequences([], 3) == []
    assert ST.parse_row_sequences([[3, 4], (5,)], 14) == [[3, 4], [5]]
    with pytest.raises(ValueError, match="at most 16"):
        ST.parse_row_sequences([[3, 4], [5], [6]], 14)
    with pytest.raises(ValueError, match="at most 16"):
        ST.parse_row_sequences([[t] for t in range(17)], 0)
    for bad in ([[]], [list(range(33))]):
        with pytest.raises(ValueError, match="1..32 ids"):
            ST.parse_row_sequences(bad, 0)
    # a request's own sequences as the per-row table takes them: [len, start 0, the ids newest first]
    t = ST.row_seq_table([[3, 4, 5], [9]])
    assert tuple(t.shape) == (2, ST.SEQ_STRIDE) and t[0, :5].tolist() == [3, 0, 5, 4, 3] and t[1, :3].tolist() == [1, 0, 9]
