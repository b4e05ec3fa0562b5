"""The two parameter records of the C ABI (include/viszephyr.h: vz_sample_params, vz_logits_proc_params) and their one checker each
(csrc/engine.hip: row_sample_of, proc_args_of), without a GPU.

(a) the ctypes mirror of vz_sample_params has the layout the header lists - the layout of the per-row table's entry in device memory.
(b) every op-level entry point checks its record before it touches the device: without a GPU a refused record is VZ_ERR_ARG (ValueError
    through binding.check) and an accepted one VZ_ERR_HIP from the first device call (binding.VzError).  Host buffers stand in for the
    device pointers, so a wrongly accepted record would fault on a machine that has a GPU: (b) runs only where there is none.
vz_op_sample takes one record for all rows, which has to be VZ_ROW_SAMPLE (the header: a greedy call is vz_op_argmax): the greedy
records the other two accept are a refusal there."""
import ctypes as C
import math

import pytest
import torch

from vz_hip import binding as B

NAN = float("nan")
ROWS, COLS = 2, 64


def rec(mode=B.ROW_SAMPLE, temperature=0.7, top_k=5, top_p=0.9, seed=0x123456789ABCDEF0, counter=3, min_p=0.0, typical_p=0.0,
        epsilon_cutoff=0.0, eta_cutoff=0.0):
    return B.VzSampleParams(mode, temperature, top_k, top_p, seed, counter, 0, min_p, typical_p, epsilon_cutoff, eta_cutoff)


REFUSED = {
    "temperature 0": rec(temperature=0.0),
    "temperature NaN": rec(temperature=NAN),
    "top_p 1.5": rec(top_p=1.5),
    "top_k -1": rec(top_k=-1),
    "counter -1": rec(counter=-1),
    "mode 2": rec(mode=2),
    "min_p 1.5": rec(min_p=1.5),
    "min_p NaN": rec(min_p=NAN),
    "typical_p -0.5": rec(typical_p=-0.5),
}
ACCEPTED = {
    "sampled": rec(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3),
    "off values": rec(typical_p=1.0, epsilon_cutoff=1.0, eta_cutoff=1.0),
}
GREEDY = {
    "greedy": rec(mode=B.ROW_GREEDY, temperature=1.0, top_k=0, top_p=1.0, seed=0, counter=0),
    "greedy, garbage elsewhere": rec(mode=B.ROW_GREEDY, temperature=NAN, top_k=-7, top_p=-2.0, seed=2 ** 64 - 1, counter=5, min_p=NAN,
                                     typical_p=-1.0, epsilon_cutoff=-math.inf, eta_cutoff=NAN),
}


def test_record_layout():
    assert C.sizeof(B.VzSampleParams) == 48
    offsets = {name: getattr(B.VzSampleParams, name).offset for name, _ in B.VzSampleParams._fields_}
    assert offsets == {"mode": 0, "temperature": 4, "top_k": 8, "top_p": 12, "seed": 16, "counter": 24, "reserved": 28, "min_p": 32,
                       "typical_p": 36, "epsilon_cutoff": 40, "eta_cutoff": 44}
    r = rec(seed=0x1122334455667788)          # the seed's low word first
    words = (C.c_uint * 12).from_buffer_copy(r)
    assert (words[4], words[5]) == (0x55667788, 0x11223344)
    # what sample_params writes for a RowParams: its own fields and its `warp` column
    from vz_hip.sample_rows import GREEDY as ROW_GREEDY, RowParams
    p = RowParams(True, 0.5, 7, 0.8, 2 ** 64 + 9, 4, min_p=0.1, typical_p=1.0, epsilon_cutoff=0.25, eta_cutoff=2.0)
    got = B.sample_params([p, ROW_GREEDY])
    assert len(got) == 2 and (got[0].mode, got[0].top_k, got[0].seed, got[0].counter, got[0].reserved) == (1, 7, 9, 4, 0)
    assert [got[0].temperature, got[0].top_p, got[0].min_p, got[0].typical_p, got[0].epsilon_cutoff, got[0].eta_cutoff] == \
        [C.c_float(v).value for v in (0.5, 0.8, 0.1, 0.0, 0.25, 0.0)]
    assert (got[1].mode, got[1].counter, got[1].min_p, got[1].typical_p) == (0, 0, 0.0, 0.0)


needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="host buffers stand in for device pointers")


class Host:
    """host buffers in the places of the device pointers"""

    def __init__(self):
        self.logits = (C.c_float * (ROWS * COLS))()
        self.ids = (C.c_int * ROWS)()
        self.rec = (C.c_float * (ROWS * 4))()
        self.hist = (C.c_int * (ROWS * 8))()
        self.hist_len = (C.c_int * ROWS)()

    def sample(self, r):
        B.check(B.lib().vz_op_sample(self.logits, ROWS, COLS, C.byref(r), self.ids, None))

    def rows_of(self, r):
        """the record as row 1 of a two-row table behind a valid row"""
        tab = (B.VzSampleParams * ROWS)()
        tab[0], tab[1] = rec(), r
        return tab

    def sample_rows(self, r):
        B.check(B.lib().vz_op_sample_rows(self.logits, ROWS, COLS, self.rows_of(r), self.ids, None))

    def token_scores(self, r):
        B.check(B.lib().vz_op_token_scores(self.logits, ROWS, COLS, self.ids, self.rows_of(r), self.rec, None, None))

    def logits_process(self, p):
        B.check(B.lib().vz_op_logits_process(self.logits, ROWS, COLS, self.hist, 8, self.hist_len, C.byref(p), None))


def passes_the_check(call, arg):
    with pytest.raises(B.VzError, match=f"error {B.VZ_ERR_HIP}:"):
        call(arg)


@needs_no_gpu
@pytest.mark.parametrize("op", ["sample", "sample_rows", "token_scores"])
@pytest.mark.parametrize("what", list(REFUSED))
def test_sampler_refusals(op, what):
    with pytest.raises(ValueError):
        getattr(Host(), op)(REFUSED[what])


@needs_no_gpu
@pytest.mark.parametrize("op", ["sample", "sample_rows", "token_scores"])
@pytest.mark.parametrize("what", list(ACCEPTED))
def test_sampler_acceptances(op, what):
    passes_the_check(getattr(Host(), op), ACCEPTED[what])


@needs_no_gpu
@pytest.mark.parametrize("what", list(GREEDY))
def test_greedy_records(what):
    h = Host()
    passes_the_check(h.sample_rows, GREEDY[what])
    passes_the_check(h.token_scores, GREEDY[what])
    with pytest.raises(ValueError, match="VZ_ROW_SAMPLE"):
        h.sample(GREEDY[what])


def proc(penalty=1.2, ngram=2, min_new=3, eos=(2,), suppress=(5, 6), seq=()):
    """seq: entries of 12 ints"""
    arr = lambda v: (C.c_int * max(1, len(v)))(*v)      # noqa: E731
    flat = [x for q in seq for x in q]
    return B.VzLogitsProcParams(penalty, ngram, min_new, len(eos), len(suppress), len(seq), arr(eos), arr(suppress), arr(flat) if seq else None)


ONE_SEQ = [1, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0]


@needs_no_gpu
@pytest.mark.parametrize("what,p", [
    ("penalty 0", dict(penalty=0.0)), ("n-gram 9", dict(ngram=9)), ("min_new -1", dict(min_new=-1)), ("5 eos ids", dict(eos=range(5))),
    ("17 suppressed ids", dict(suppress=range(17))), ("65 id sequences", dict(seq=[ONE_SEQ] * 65)),
])
def test_processor_refusals(what, p):
    with pytest.raises(ValueError):
        Host().logits_process(proc(**p))


@needs_no_gpu
@pytest.mark.parametrize("seq", [[], [ONE_SEQ] * 64])
def test_processor_acceptance(seq):
    passes_the_check(Host().logits_process, proc(seq=seq))
