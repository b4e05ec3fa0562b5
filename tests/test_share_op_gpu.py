"""vz_op_attention_shared (csrc/attn_shared.hip) on its own buffers against the fp32 reference of tests/share_ref.py, at the tolerances
every attention-op test of this project holds its kernel to (max-norm 8e-3, relative L2 4e-3).  The shared slots of every non-first row of
a group, the cache behind slot[r] and the output buffer are NaN: a single read of the wrong row or slot, or an unwritten output row,
poisons the result."""
import pytest
import torch

from share_ref import NAN, copied_cache, poisoned_case, shared_attention_ref
from util import check_close, errs, record

pytestmark = pytest.mark.gpu

HQ, HKV, D, MAX_CTX = 32, 8, 128, 512
SCALE = D ** -0.5
MAX_TOL, L2_TOL = 8e-3, 4e-3
SUFFIX = [1, 2, 64, 65, 100]          # own slots of a row, the new token included


@pytest.fixture(scope="module")
def B():
    from vz_hip import binding
    binding.load_library()
    return binding


def _run(B, name, n, shared, slot, window=0, nsplit=0, seed=0, old=True):
    R = len(slot)
    assert R == n * len(shared) and max(slot) < MAX_CTX
    q, kc, vc, out = poisoned_case(R, n, HQ, HKV, D, MAX_CTX, shared, slot, seed)
    dev = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")      # noqa: E731
    got = B.attention_shared(q, kc, vc, dev(shared), dev(slot), n, SCALE, max(shared), window=window, nsplit=nsplit, out=out)
    assert got is out
    ref = shared_attention_ref(q, kc, vc, n, shared, slot, SCALE, window)
    if old and all(s >= shared[r // n] for r, s in enumerate(slot)):
        # the existing decode-attention op on the copy route's cache (the prefix copied into every row), next to the new kernel's error
        kcc, vcc = (torch.nan_to_num(t.float(), nan=0.0).bfloat16() for t in copied_cache(kc, vc, n, shared))
        e_old = errs(B.attention_decode(q, kcc, vcc, dev([s + 1 for s in slot]), SCALE, window=window).float(), ref)
        record(f"attention_shared old kernel {name}", max_err=e_old[0], l2_err=e_old[1])
    check_close(f"attention_shared {name}", out.float(), ref, MAX_TOL, L2_TOL)
    return out, ref


def _slots(n, shared, first=0):
    """rows of one group with different own lengths: row j of group g takes SUFFIX[(first + g + j) % 5]"""
    return [sh + SUFFIX[(first + g + j) % len(SUFFIX)] - 1 for g, sh in enumerate(shared) for j in range(n)]


# n rows per group: 8, 16, 64, 68 and 256 stacked rows - a partial tile, one exact tile, a ragged second tile, four tiles
@pytest.mark.parametrize("shared", [1, 63, 64, 65, 200, 380])
@pytest.mark.parametrize("n", [2, 4, 16, 17, 64])
def test_shared_attention(B, n, shared):
    _run(B, f"n={n} shared={shared}", n, [shared], _slots(n, [shared], first=shared), seed=1000 + 7 * n + shared)


@pytest.mark.parametrize("suffix", SUFFIX)
def test_shared_attention_every_suffix_length(B, suffix):
    """every row of a group with the same own length (1 = only the new token)"""
    _run(B, f"n=4 shared=65 suffix={suffix}", 4, [65], [65 + suffix - 1] * 4, seed=50 + suffix)


def test_shared_attention_two_groups(B):
    _run(B, "n=4 shared=(65,200)", 4, [65, 200], _slots(4, [65, 200]), seed=3)
    _run(B, "n=17 shared=(380,1)", 17, [380, 1], _slots(17, [380, 1], first=2), seed=4)


def test_shared_attention_row_in_front_of_the_shared_slots(B):
    """a row with slot < shared shares nothing this step: its own slots [0, slot]"""
    _run(B, "n=4 shared=100 slot=(104,37,100,163)", 4, [100], [104, 37, 100, 163], seed=5)
    _run(B, "n=2 shared=(100,64) slot=(99,120,64,0)", 2, [100, 64], [99, 120, 64, 0], seed=6)


@pytest.mark.parametrize("window,what", [(48, "prefix partly visible"), (8, "prefix wholly masked"), (10, "exactly the suffix"), (11, "one shared slot")])
def test_shared_attention_window(B, window, what):
    """shared 100, 10 own slots: window 8 leaves every prefix partial empty (m = -inf in the merge), window 10 covers exactly the own slots"""
    _run(B, f"window={window} ({what})", 4, [100], [109] * 4, window=window, seed=8)


def test_shared_attention_window_per_row(B):
    """rows of one stacked tile with different windows' starts: masked per stacked row"""
    _run(B, "window=48 n=16 shared=200", 16, [200], _slots(16, [200]), window=48, seed=9)


def test_shared_attention_forced_splits(B):
    """one split and the most a call can take (one per 64-key tile): same result at the tolerance"""
    slot = _slots(16, [380])
    one, ref = _run(B, "nsplit=1 n=16 shared=380", 16, [380], slot, nsplit=1, seed=10)
    most, _ = _run(B, "nsplit=max n=16 shared=380", 16, [380], slot, nsplit=64, seed=10, old=False)
    check_close("attention_shared nsplit=1 vs max", most.float(), one.float(), MAX_TOL, L2_TOL)


def test_shared_attention_refusals(B):
    dev = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")      # noqa: E731

    def call(R, n, shared, shared_max, ws=None):
        q = torch.zeros(R, HQ, D, dtype=torch.bfloat16, device="cuda")
        kc = torch.zeros(R, HKV, 64, D, dtype=torch.bfloat16, device="cuda")
        return B.attention_shared(q, kc, kc.clone(), dev(shared), dev([s for s in shared for _ in range(n)]), n, SCALE, shared_max, ws=ws)

    call(4, 2, [3, 5], 5)                                              # (the shape the refusals below vary)
    with pytest.raises(ValueError, match="bad shape"):
        call(2, 1, [3, 5], 5)                                          # n = 1
    with pytest.raises(ValueError, match="bad shape"):
        call(65, 65, [3], 3)                                           # n = 65
    with pytest.raises(ValueError, match="shared_max"):
        call(4, 2, [3, 5], 65)                                         # shared > max_ctx
    with pytest.raises(ValueError, match="workspace"):
        call(4, 2, [3, 5], 5, ws=torch.empty(4 * HQ * (D + 4) - 1, dtype=torch.float32, device="cuda"))
    assert B.attention_shared_ws_floats(2, 1, HQ, HKV, 64) == 0 and B.attention_shared_ws_floats(65, 65, HQ, HKV, 64) == 0
