"""The per-row logits processors at op level (csrc/logits_proc.hip: logits_process_rows_kernel): a different config in
every row, bit for bit against the call-level kernel run on each row alone with that row's config and against tests/seq_bias_ref.py, the
numpy restatement of HF's chain; inactive rows are left alone; a bad record is refused before anything is launched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seq_bias_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("-inf")


def _alphabet(V):
    """16 ids spread over the row: the first, the last (V = 97: a bit of the partial last bitmap word), ids above 32768 when there are any"""
    return [int(t) for t in np.concatenate([[0], np.linspace(1, V - 2, 14).astype(np.int64), [V - 1]])]


def _pool(a):
    """every processor, alone and together; trigger = ids a history has to end in for the config's sequences to act"""
    from vz_hip.logits_proc import ProcConfig as P
    return [
        (P(penalty=1.3, ngram=1), []),                                                         # n-gram 1: every id of the history is banned
        (P(penalty=0.8, ngram=8), []),                                                         # n-gram 8
        (P(seq=(((a[5],), -0.3, False), ((a[2], a[5]), 2.0, False), ((a[6], a[5]), 0.75, False))), [a[2]]),      # two (three) biases land on a[5]
        (P(penalty=1.2, seq=((tuple(a[2:10]), INF, True),)), a[2:9]),                             # a bad word of 8 ids
        (P(seq=(((a[3],), 4.0, False), ((a[7], a[3]), 1.5, False), ((a[3],), INF, True))), [a[7]]),              # a bias on an id that is also banned
        (P(min_new=40, eos=(a[15], a[14], a[13], a[12])), []),                                    # min_new with 4 eos ids
        (P(penalty=1.5, ngram=2, min_new=2, eos=(a[15],), suppress=(a[11], a[0]),
           seq=(((a[1],), 2.5, False), ((a[4], a[8]), -1e8, False), ((a[9],), INF, True), ((a[4], a[10]), INF, True))), [a[4]]),
        (P(ngram=3, suppress=tuple(a[:16])), []),                                                 # 16 suppressed ids
    ]


def _case(rows, V, seed):
    """logits, per-row configs, per-row histories: lengths from {0, 1, g - 1, g, 37} (g = the row's n-gram size, 2 without one), ids from the
    alphabet with a short period so that n-grams repeat, ends that arm the row's sequences"""
    rng = np.random.default_rng(seed)
    a = _alphabet(V)
    g0 = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, V, generator=g0) * 3).float()
    x[:, a[1]], x[:, a[3]], x[:, a[4]] = 0.0, -2.25, INF           # an exact zero, a negative and a -inf logit under bias and penalty
    pool = _pool(a)
    cfgs, hists = [], []
    for r in range(rows):
        cfg, trig = pool[(r + seed) % len(pool)]
        g = cfg.ngram or 2
        n = (0, 1, g - 1, g, 37)[(r // len(pool) + r + seed) % 5]
        period = (3, 5, 16)[r % 3]
        off = int(rng.integers(0, 16))
        h = [a[(off + i) % period] if r % 2 else a[int(rng.integers(0, 16))] for i in range(n)]
        if trig and n >= len(trig):
            h[n - len(trig):] = trig
        cfgs.append(cfg)
        hists.append(h)
    return x, cfgs, hists


def _device_hist(hists, stride=64):
    hist = torch.full((len(hists), stride), -7, dtype=torch.int32)
    for r, h in enumerate(hists):
        hist[r, :len(h)] = torch.tensor(h, dtype=torch.int32)
    return hist, torch.tensor([len(h) for h in hists], dtype=torch.int32)


@pytest.mark.parametrize("V", [97, 32000, 40000])
@pytest.mark.parametrize("rows", [1, 3, 64])
def test_rows_equal_the_call_level_kernel_and_the_restatement(rows, V):
    from vz_hip import binding as B
    changed = acting = 0
    for seed in ((0, 3, 5, 6) if rows < 64 else (1,)):            # few rows: several draws, so that every config of the pool is met
        x, cfgs, hists = _case(rows, V, seed)
        hist, hl = _device_hist(hists)
        y, hd, hld = x.clone().cuda(), hist.cuda(), hl.cuda()
        B.logits_process_rows(y, cfgs, hd, hld)
        assert torch.equal(hd.cpu(), hist) and torch.equal(hld.cpu(), hl), "the op-level form appends nothing"
        for r in range(rows):
            one, h1, l1 = x[r:r + 1].clone().cuda(), hist[r:r + 1].clone().cuda(), hl[r:r + 1].clone().cuda()
            B.logits_process(one, cfgs[r], h1, l1)                 # the call-level kernel on the row alone, with the row's config
            assert torch.equal(y[r].view(torch.int32), one[0].view(torch.int32)), (seed, r, cfgs[r], hists[r][-9:])
            assert torch.equal(h1.cpu(), hist[r:r + 1]) and torch.equal(l1.cpu(), hl[r:r + 1])
        got = y.cpu().numpy()
        for r in range(rows):
            want = R.process(x[r].numpy(), hists[r], cfgs[r])
            assert np.array_equal(got[r].view(np.int32), want.view(np.int32)), (seed, r, cfgs[r], np.nonzero(got[r].view(np.int32) != want.view(np.int32))[0])
            d = int((want.view(np.int32) != x[r].numpy().view(np.int32)).sum())
            changed += d
            acting += d > 0
    assert acting >= (1 if rows == 1 else 2) and changed >= acting


def test_inactive_rows_are_left_alone():
    from vz_hip import binding as B
    V = 32000
    x, cfgs, hists = _case(3, V, 0)
    cfgs[1] = None
    hists[1] = [5, 6, 7]
    x[1] = float("nan")                                           # poisoned: the bits must survive
    x[1, 7] = torch.tensor([0x7FC01234], dtype=torch.int32).view(torch.float32)[0]      # a NaN with a payload
    hist, hl = _device_hist(hists)
    y, hd, hld = x.clone().cuda(), hist.cuda(), hl.cuda()
    B.logits_process_rows(y, cfgs, hd, hld)
    assert torch.equal(y[1].cpu().view(torch.int32), x[1].view(torch.int32))
    assert torch.equal(hd.cpu(), hist) and torch.equal(hld.cpu(), hl)
    for r in (0, 2):
        want = R.process(x[r].numpy(), hists[r], cfgs[r])
        assert np.array_equal(y[r].cpu().numpy().view(np.int32), want.view(np.int32))
    # every row inactive: nothing moves at all
    z = x.clone().cuda()
    B.logits_process_rows(z, [None, None, None], hd, hld)
    assert torch.equal(z.cpu().view(torch.int32), x.view(torch.int32))


def test_bad_records_are_refused_before_any_launch():
    from vz_hip import binding as B
    from vz_hip.logits_proc import ProcConfig as P
    good = P(penalty=1.3, ngram=1)
    x = torch.randn(3, 1000, generator=torch.Generator().manual_seed(1)).float()
    hist, hl = _device_hist([[1, 2, 3]] * 3)
    one = ((5,), 1.0, False)
    for bad in (P(penalty=0.0), P(penalty=-1.5), P(ngram=9), P(suppress=tuple(range(17))), P(seq=(one,) * 65)):
        y, hd, hld = x.clone().cuda(), hist.cuda(), hl.cuda()
        with pytest.raises(ValueError):
            B.logits_process_rows(y, [good, good, bad], hd, hld)
        torch.cuda.synchronize()
        assert torch.equal(y.cpu().view(torch.int32), x.view(torch.int32)), "a refused call launched its good rows"
    y = x.clone().cuda()
    B.logits_process_rows(y, [good, P(seq=(one,) * 64), P(ngram=8, suppress=tuple(range(16)))], hist.cuda(), hl.cuda())      # the limits themselves pass
    assert not torch.equal(y.cpu(), x)
