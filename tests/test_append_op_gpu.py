"""vz_op_attention_append (csrc/attn_append.hip) on its own buffers against the fp32 reference of tests/append_ref.py, at the tolerances
every attention-op test of tests/test_ops_gpu.py holds its kernel to (max-norm 8e-3, relative L2 4e-3).  The cache behind past + new and
the unused token rows are NaN: a single read of either poisons the output."""
import pytest
import torch

from append_ref import NAN, append_attention_ref, poisoned_case
from util import check_close, errs, record

pytestmark = pytest.mark.gpu

HQ, HKV, D, MAX_CTX = 32, 8, 128, 512
SCALE = D ** -0.5
MAX_TOL, L2_TOL = 8e-3, 4e-3


@pytest.fixture(scope="module")
def B():
    from vz_hip import binding
    binding.load_library()
    return binding


def _run(B, name, T, past, new, window=0, nsplit=0, seed=0):
    Bn = len(past)
    q, kc, vc = poisoned_case(Bn, T, HQ, HKV, D, MAX_CTX, past, new, seed)
    dev = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")      # noqa: E731
    out = torch.full((Bn, T, HQ, D), NAN, dtype=torch.bfloat16, device="cuda")
    kv_max = max(p + n for p, n in zip(past, new))
    got = B.attention_append(q, kc, vc, dev(past), dev(new), SCALE, kv_max, window=window, nsplit=nsplit, out=out)
    assert got is out
    ref = append_attention_ref(q, kc, vc, past, new, SCALE, window)
    old = torch.full_like(ref, NAN)
    for b in range(Bn):          # the existing kernel with a scalar q_pos0, one cache row at a time
        n, kv = new[b], past[b] + new[b]
        k1 = kc[b, :, :kv].permute(1, 0, 2).unsqueeze(0)
        v1 = vc[b, :, :kv].permute(1, 0, 2).unsqueeze(0)
        old[b, :n] = B.attention(q[b:b + 1, :n], k1, v1, SCALE, True, past[b], window)[0].float()
        assert torch.isnan(out[b, n:].float()).all(), f"{name}: token rows >= new[{b}] were written"
    live = ~torch.isnan(ref)
    e_old = errs(old[live], ref[live])
    record(f"attention_append old kernel {name}", max_err=e_old[0], l2_err=e_old[1])
    check_close(f"attention_append {name}", out.float()[live], ref[live], MAX_TOL, L2_TOL)
    return out, ref, live


# T x past: every 64-key tile boundary, one / several query tiles (16 tokens x 4 heads each), one / several splits, the end of the cache
CASES = [(1, 0), (1, 1), (1, 63), (1, 64), (1, 380), (3, 0), (3, 65), (3, 127), (3, 200), (17, 0), (17, 63), (17, 64), (17, 127),
         (17, 380), (33, 0), (33, 1), (33, 65), (33, 200), (33, 380), (130, 0), (130, 65), (130, 200), (130, 382)]


@pytest.mark.parametrize("T,past", CASES, ids=lambda v: str(v))
def test_append_attention(B, T, past):
    assert past + T <= MAX_CTX
    _run(B, f"T={T} past={past}", T, [past], [T], seed=100 + T + past)


def test_append_attention_rows_of_different_length(B):
    _run(B, "B=2 past=(65,200) new=(17,5)", 17, [65, 200], [17, 5], seed=7)


def test_append_attention_window(B):
    _run(B, "window=48 T=33 past=100", 33, [100], [33], window=48, seed=8)


def test_append_attention_forced_splits(B):
    """one split (no workspace, direct store) and the most the host rule can choose (one per 64-key tile): same result at the tolerance"""
    one, ref, live = _run(B, "nsplit=1 T=33 past=380", 33, [380], [33], nsplit=1, seed=9)
    most, _, _ = _run(B, "nsplit=max T=33 past=380", 33, [380], [33], nsplit=64, seed=9)
    check_close("attention_append nsplit=1 vs max", most.float()[live], one.float()[live], MAX_TOL, L2_TOL)
