"""Helpers of the Stage-1 training step at op level (train.hip): the 64 x 64 transposition through the hardware transposing LDS read (the
dY^T / X^T / W^T copies of the weight- and input-gradient GEMMs) and the column sums (bias gradients).  Exact: a transposition moves
bits; the column sums are compared with a float64 sum (fp32 accumulation in a fixed order: 1e-6 relative).

Below those two: every other kernel of train.hip on its own against the float64 restatements of tests/train_ref.py (held to autograd by
tests/test_train_ref_cpu.py), at the tails, boundaries and kernel choices the whole-step tests never reach.  Bounds, per element and over
ALL elements of an output (padding and guard rows included):
    bf16 output   |hip - ref| <= 2^-8 |ref| + delta     2^-8 = bf16's unit roundoff; delta = 8 x the largest distance between the
                                                        unrounded fp32 CPU evaluation of the same reference and the float64 one on this
                                                        test's inputs (8: __expf / rsqrtf at a few ulp, another summation order)
    fp32 output   the same without the bf16 term, both sides divided by the sum of absolute terms of the element's reduction; on an output of
                  fewer than 16 elements the measured distance counts as at least fp32's unit roundoff 2^-24 (see check_f32)
    moves (gather, transposition, the V part of the RoPE re-assembly, AdamW's working copy of its master): bitwise
Outputs are pre-filled with a sentinel and sit inside guard elements, so an unwritten or over-written element shows.  Each delta and each
measured error goes to util.record."""
import math

import pytest
import torch

import train_ref as R
from util import record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from vz_hip import binding
    binding.load_library()
    return binding


@pytest.mark.parametrize("R,C", [(64, 64), (2560, 4096), (200, 136), (8, 8), (10240, 1024), (33, 47), (64, 72)])
def test_transpose_is_exact(B, R, C):
    x = torch.randn(R, C, generator=torch.Generator().manual_seed(R + C)).to("cuda", torch.bfloat16)
    y = B.transpose(x)
    assert torch.equal(y, x.t().contiguous())
    # a strided source (leading dimension wider than C)
    wide = torch.randn(R, C + 16, generator=torch.Generator().manual_seed(1)).to("cuda", torch.bfloat16)
    assert torch.equal(B.transpose(wide[:, :C]), wide[:, :C].t().contiguous())


@pytest.mark.parametrize("rows,cols", [(37, 64), (2560, 4096), (10240, 12288), (5000, 100), (4096, 1024)])
def test_colsum_adds_into_the_output(B, rows, cols):
    y = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows)).to("cuda", torch.bfloat16)
    out = torch.full((cols,), 0.5, dtype=torch.float32, device="cuda")
    B.colsum(y, out)
    ref = y.double().sum(0) + 0.5
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    assert err <= 1e-6, err
    out2 = torch.full((cols,), 0.5, dtype=torch.float32, device="cuda")
    B.colsum(y, out2)
    assert torch.equal(out, out2)          # fixed order: reproducible


# ------------------------------------------------------------------------------------------------------------------------------------
# plumbing of the per-kernel blocks
# ------------------------------------------------------------------------------------------------------------------------------------
SENT = -7.5                 # bf16-exact, far from anything the kernels produce here
GUARD = 64                  # sentinel elements before and after every output
WRAP = 8192 * 256           # grid_for() caps the grid at 8192 workgroups of 256: above this many work items the grid-stride loop wraps
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=_gen(seed), dtype=F32)


def _cuda(t):
    return None if t is None else t.to("cuda")


class Out:
    """a device output of `n` elements between two guards, all pre-filled with a sentinel (an accumulator copies its start value over the body);
    `off` (elements) shifts it off 16-byte alignment"""

    def __init__(self, n, dtype=BF, off=0, fill=SENT):
        self.n, self.lo, self.fill = n, GUARD + off, fill
        self.base = torch.full((n + 2 * GUARD + off,), fill, dtype=dtype, device="cuda")
        self.t = self.base[self.lo:self.lo + n]

    def host(self):
        """the output on the host, after checking that the guards still hold the sentinel"""
        torch.cuda.synchronize()
        h = self.base.cpu()
        assert (h[:self.lo] == self.fill).all() and (h[self.lo + self.n:] == self.fill).all(), "wrote outside its output"
        return h[self.lo:self.lo + self.n]


def _shifted(t, off):
    """a device copy of `t` whose base sits `off` elements past a 16-byte boundary"""
    base = torch.empty(t.numel() + off + 8, dtype=t.dtype, device="cuda")
    v = base[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (off * t.element_size()) % 16
    return v


def check_bf16(name, hip, ref64, ref32):
    """every element of a bf16 output inside 2^-8 |ref| + delta; returns the worst err / bound"""
    hip, ref64 = hip.reshape(-1).to(F64), ref64.reshape(-1)
    assert hip.shape == ref64.shape, (hip.shape, ref64.shape)
    delta = R.delta_of(ref32.reshape(-1), ref64)
    err, bound = (hip - ref64).abs(), R.bound_bf16(ref64, delta)
    finite = bool(torch.isfinite(hip).all())
    worst = float((err / bound.clamp_min(1e-300)).nan_to_num(nan=math.inf).max()) if hip.numel() else 0.0
    excess = float((err - bound).nan_to_num(nan=math.inf).max())
    print(f"{name}: delta {delta:.3e}  max err {float(err.nan_to_num(nan=math.inf).max()):.3e}  worst err/bound {worst:.3f}  n {hip.numel()}")
    record("train_ops/" + name, kind="bf16", delta=delta, max_err=float(err.nan_to_num(nan=math.inf).max()), worst_ratio=worst, n=hip.numel())
    assert finite, f"{name}: non-finite output"
    assert excess <= 0.0, f"{name}: {int((err > bound).sum())} of {hip.numel()} elements outside 2^-8|ref| + {delta:.3e}; worst err/bound {worst:.3f}"
    return worst


FEW = 16                    # outputs of fewer elements than this take the floor of check_f32


def check_f32(name, hip, ref64, ref32, terms):
    """every element of an fp32 output: |hip - ref| / terms <= delta = 8 x max(|fp32 evaluation - ref| / terms).  The maximum over an output of
    fewer than FEW elements (one row's statistics, nine loss rows) is no measure of fp32 arithmetic: the CPU evaluation lands on the float64
    value, or within a fraction of a rounding of it, by accident there (one element: exactly, for a single add).  Only for those outputs the
    maximum counts as no less than fp32's unit roundoff 2^-24, the one rounding of a partial result of the size of `terms`; `floor` in the
    record says whether that was the operative bound"""
    hip, ref64, terms = hip.reshape(-1).to(F64), ref64.reshape(-1), terms.reshape(-1).to(F64)
    assert hip.shape == ref64.shape == terms.shape, (hip.shape, ref64.shape, terms.shape)
    measured = R.delta_of(ref32.reshape(-1), ref64, terms)
    floor = hip.numel() < FEW and measured < R.FP32_FACTOR * R.U_FP32
    delta = R.FP32_FACTOR * R.U_FP32 if floor else measured
    err = ((hip - ref64).abs() / terms.clamp_min(1e-300)).nan_to_num(nan=math.inf)
    mx = float(err.max())
    print(f"{name}: delta(normalised) {delta:.3e}{' (floor)' if floor else ''}  max err(normalised) {mx:.3e}  n {hip.numel()}")
    record("train_ops/" + name, kind="fp32", delta=delta, floor=bool(floor), max_err=mx,
           worst_ratio=mx / delta if delta > 0 else (0.0 if mx == 0 else math.inf), n=hip.numel())
    assert bool(torch.isfinite(hip).all()), f"{name}: non-finite output"
    assert mx <= delta, f"{name}: normalised error {mx:.3e} above {delta:.3e}"


# ------------------------------------------------------------------------------------------------------------------------------------
# masked softmax
# ------------------------------------------------------------------------------------------------------------------------------------
# (Bn, H, Sq, Sk, causal, window, kv_len, spikes): rows 1 / 3 / 4 / 5 / 1027 (one wave per row, four rows per workgroup); Sk around the 64-lane
# stride; Bn > 1 with H and Sq coprime so that a wrong b / i decomposition lands on another kv_len / another diagonal; windows of 1, below Sk
# and above Sk; kv_len of 0 and above Sk
SOFTMAX = [
    (1, 1, 1, 1, False, 0, None, False),
    (1, 1, 3, 63, True, 0, None, False),
    (1, 2, 2, 64, False, 0, [70], False),
    (1, 1, 5, 65, True, 1, None, False),
    (1, 1, 1027, 1059, True, 100, None, True),
    (3, 2, 7, 200, False, 0, [0, 150, 300], True),
    (2, 3, 5, 200, True, 4096, [3, 200], False),
    (2, 2, 9, 65, True, 3, [65, 4], False),
    (3, 3, 67, 65, True, 64, [65, 0, 33], True),
]
SM_SCALE = R.f32(1.0 / math.sqrt(128.0))


def _softmax_inputs(case):
    Bn, H, Sq, Sk, causal, window, kv, spikes = case
    rows = Bn * H * Sq
    kv_len = None if kv is None else torch.tensor(kv, dtype=torch.int32)
    vis = R.softmax_visible(rows, H, Sq, Sk, causal, window, kv_len)
    S = _randn(rows + Sk, rows, Sk) * 8
    if spikes:                      # one +1e4 and one -1e4 score per row, on visible keys where the row has any
        for r in range(0, rows, 3):
            js = vis[r].nonzero()[:, 0]
            if js.numel():
                S[r, js[(r * 7) % js.numel()]] = 1e4
                S[r, js[(r * 11 + 1) % js.numel()]] = -1e4
    return rows, kv_len, vis, S


@pytest.mark.parametrize("case", SOFTMAX, ids=lambda c: f"B{c[0]}H{c[1]}Sq{c[2]}Sk{c[3]}c{int(c[4])}w{c[5]}kv{c[6]}")
def test_softmax_fwd(B, case):
    Bn, H, Sq, Sk, causal, window, kv, _ = case
    rows, kv_len, vis, S = _softmax_inputs(case)
    ldp = R.pad64(Sk)
    # what a masked score holds is nobody's business (the step computes it from cache rows nobody wrote): NaN there and in S's padding
    Sd = torch.full((rows, ldp + 64), math.nan, dtype=F32)
    Sd[:, :Sk] = torch.where(vis, S, torch.full_like(S, math.nan))
    Sd = _cuda(Sd)
    P = Out(rows * ldp)
    B.softmax_fwd(Sd, P.t.view(rows, ldp), rows, H, Sq, Sk, SM_SCALE, causal, window, _cuda(kv_len))
    got = P.host().view(rows, ldp)
    assert (got[:, Sk:] == 0).all(), "padding columns must be exactly 0"
    assert (got[:, :Sk][~vis] == 0).all(), "masked entries must be exactly 0"
    ref64 = torch.zeros(rows, ldp, dtype=F64)
    ref32 = torch.zeros(rows, ldp, dtype=F32)
    ref64[:, :Sk] = R.softmax_fwd(S, vis, SM_SCALE, F64)
    ref32[:, :Sk] = R.softmax_fwd(S, vis, SM_SCALE, F32)
    check_bf16(f"softmax_fwd/{Bn}x{H}x{Sq}x{Sk}", got, ref64, ref32)
    live = vis.any(1)
    assert ((got[:, :Sk].double().sum(1) - 1).abs()[live] <= Sk * R.U_BF16).all() and (got[~live] == 0).all()


@pytest.mark.parametrize("case", SOFTMAX, ids=lambda c: f"B{c[0]}H{c[1]}Sq{c[2]}Sk{c[3]}c{int(c[4])}w{c[5]}kv{c[6]}")
def test_softmax_bwd(B, case):
    Bn, H, Sq, Sk, causal, window, kv, _ = case
    rows, kv_len, vis, S = _softmax_inputs(case)
    ldp, lddp, ldds = R.pad64(Sk), R.pad64(Sk) + 64, R.pad64(Sk) + 64
    P = torch.zeros(rows, ldp, dtype=BF)
    P[:, :Sk] = R.softmax_fwd(S, vis, SM_SCALE, F64).to(BF)
    dP = torch.full((rows, lddp), math.nan, dtype=F32)                 # NaN wherever P == 0 and in the padding: must not be read
    vals = _randn(rows + 1, rows, Sk) * 3
    dP[:, :Sk] = torch.where(P[:, :Sk] != 0, vals, torch.full_like(vals, math.nan))
    dS = Out(rows * ldds)
    B.softmax_bwd(_cuda(P), _cuda(dP), dS.t.view(rows, ldds), rows, Sk, SM_SCALE)
    got = dS.host().view(rows, ldds)
    assert torch.isfinite(got.float()).all()
    assert (got[:, Sk:] == 0).all(), "padding columns up to ldds must be exactly 0"
    assert (got[:, :Sk][P[:, :Sk] == 0] == 0).all(), "dS must be exactly 0 where P == 0"
    ref64 = torch.zeros(rows, ldds, dtype=F64)
    ref32 = torch.zeros(rows, ldds, dtype=F32)
    ref64[:, :Sk] = R.softmax_bwd(P[:, :Sk], dP[:, :Sk], SM_SCALE, F64)
    ref32[:, :Sk] = R.softmax_bwd(P[:, :Sk], dP[:, :Sk], SM_SCALE, F32)
    check_bf16(f"softmax_bwd/{Bn}x{H}x{Sq}x{Sk}", got, ref64, ref32)
    # rows of dS sum to (about) zero: as near as the reference's own rows (bf16 P does not sum to exactly 1) plus the elements' bounds
    slack = R.bound_bf16(ref64, R.delta_of(ref32, ref64)).sum(1)
    assert (got.double().sum(1).abs() <= ref64.sum(1).abs() + slack).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# RMSNorm backward: the 4096-column register kernel (aligned bases) and the generic one (everything else, and 4096 columns on a view 4 elements
# off alignment) against the same float64
# ------------------------------------------------------------------------------------------------------------------------------------
RMS_EPS = R.f32(1e-5)
# (rows, cols, dres, offset elements, ill-conditioned)
RMSNORM = [
    (1, 48, False, 0, False), (3, 1000, True, 0, False), (4, 1024, False, 0, False), (5, 8192, True, 0, False), (1027, 1024, True, 0, False),
    (1, 4096, True, 0, False), (3, 4096, False, 0, False), (4, 4096, True, 0, False), (5, 4096, False, 0, False), (1027, 4096, True, 0, False),
    (1, 4096, True, 4, False), (3, 4096, False, 4, False), (4, 4096, True, 4, False), (5, 4096, False, 4, False), (1027, 4096, True, 4, False),
    (37, 4096, True, 0, True), (37, 4096, True, 4, True), (129, 1000, False, 0, True), (5, 48, True, 4, True),
]


@pytest.mark.parametrize("rows,cols,with_res,off,ill", RMSNORM)
def test_rmsnorm_bwd(B, rows, cols, with_res, off, ill):
    x = (_randn(rows * 3 + cols, rows, cols) + (100.0 if ill else 0.0)).to(BF)          # ill: mean(x) ~ 100, dy ~ 1e-4 - the two terms of dx cancel
    dy = (_randn(rows + 7, rows, cols) * (1e-4 if ill else 1.0)).to(BF)
    w = 1.0 + 0.1 * _randn(cols, cols)
    dres = (_randn(rows + 9, rows, cols) * (1e-4 if ill else 1.0)).to(BF) if with_res else None
    dx = Out(rows * cols, off=off)
    xd, dyd, dresd = _shifted(x, off), _shifted(dy, off), (_shifted(dres, off) if with_res else None)
    assert dx.t.data_ptr() % 16 == 2 * off and xd.data_ptr() % 16 == 2 * off          # 0: the register kernel's precondition at 4096 columns; 8: generic
    B.rmsnorm_bwd(xd, _cuda(w), dyd, dresd, dx.t, rows, cols, RMS_EPS)
    got = dx.host().view(rows, cols)
    check_bf16(f"rmsnorm_bwd/{rows}x{cols}{'+res' if with_res else ''}{'/off4' if off else ''}{'/ill' if ill else ''}", got,
               R.rmsnorm_bwd(x, w, dy, dres, RMS_EPS, F64), R.rmsnorm_bwd(x, w, dy, dres, RMS_EPS, F32))


@pytest.mark.parametrize("rows", [5, 1027])
def test_rmsnorm_bwd_generic_and_register_kernels_agree(B, rows):
    """the same 4096-column problem through both kernels: each within its bound of float64 above, and within the two bounds of each other here"""
    cols = 4096
    x, dy, w = _randn(1, rows, cols).to(BF), _randn(2, rows, cols).to(BF), 1.0 + 0.1 * _randn(3, cols)
    outs = []
    for off in (0, 4):
        dx = Out(rows * cols, off=off)
        B.rmsnorm_bwd(_shifted(x, off), _cuda(w), _shifted(dy, off), None, dx.t, rows, cols, RMS_EPS)
        outs.append(dx.host().double())
    ref64, ref32 = R.rmsnorm_bwd(x, w, dy, None, RMS_EPS, F64).reshape(-1), R.rmsnorm_bwd(x, w, dy, None, RMS_EPS, F32).reshape(-1)
    bound = R.bound_bf16(ref64, R.delta_of(ref32, ref64))
    assert ((outs[0] - outs[1]).abs() <= 2 * bound).all()
    record("train_ops/rmsnorm_bwd/kernels_agree", rows=rows, differing=int((outs[0] != outs[1]).sum()), n=rows * cols)


# ------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward: dx, the (mean, rstd) statistics, dw / db added into what the buffers hold; rows around the 128-group boundary of the
# partial sums; cols off the 512-column stride of a wave
# ------------------------------------------------------------------------------------------------------------------------------------
LN_EPS = R.f32(1e-6)
# (rows, cols, dres, shifted x)
LAYERNORM = [(1, 8, False, False), (127, 520, True, False), (128, 1024, False, False), (129, 1408, True, True), (1000, 4096, True, False),
             (129, 8, False, False), (1000, 1408, False, True), (128, 520, True, True), (127, 4096, False, False), (1, 1024, True, False)]


def _ln_inputs(rows, cols, with_res, shifted):
    x = (_randn(rows + cols, rows, cols) * 0.5 + 50.0 if shifted else _randn(rows + cols, rows, cols)).to(BF)
    dy = _randn(rows + 11, rows, cols).to(BF)
    w, dres = 1.0 + 0.2 * _randn(cols + 1, cols), (_randn(rows + 13, rows, cols).to(BF) if with_res else None)
    dw0, db0 = _randn(cols + 2, cols), _randn(cols + 3, cols)
    return x, dy, w, dres, dw0, db0


def _ln_check(name, x, dy, w, dres, dw0, db0, stats, dw, db):
    r64, r32 = R.layernorm_bwd(x, w, dy, dres, LN_EPS, F64), R.layernorm_bwd(x, w, dy, dres, LN_EPS, F32)
    check_f32(name + "/mean", stats[:, 0], r64[3], r32[3], x.double().abs().mean(-1))
    check_f32(name + "/rstd", stats[:, 1], r64[4], r32[4], r64[4])
    check_f32(name + "/dw", dw, dw0.double() + r64[1], dw0 + r32[1], dw0.double().abs() + r64[5])
    check_f32(name + "/db", db, db0.double() + r64[2], db0 + r32[2], db0.double().abs() + r64[6])
    return r64[0], r32[0]


@pytest.mark.parametrize("rows,cols,with_res,shifted", LAYERNORM)
def test_layernorm_bwd(B, rows, cols, with_res, shifted):
    x, dy, w, dres, dw0, db0 = _ln_inputs(rows, cols, with_res, shifted)
    name = f"layernorm_bwd/{rows}x{cols}{'+res' if with_res else ''}{'/mean50' if shifted else ''}"
    runs = []
    for _ in range(2):
        dx, dw, db = Out(rows * cols), Out(cols, F32), Out(cols, F32)
        dw.t.copy_(dw0)
        db.t.copy_(db0)
        stats = B.layernorm_bwd(_cuda(x), _cuda(w), _cuda(dy), _cuda(dres), dx.t, dw.t, db.t, rows, cols, LN_EPS)
        runs.append((dx.host(), dw.host(), db.host(), stats.cpu()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), "two runs must be bit-identical (fixed summation order)"
    got_dx, got_dw, got_db, stats = runs[0]
    dx64, dx32 = _ln_check(name, x, dy, w, dres, dw0, db0, stats, got_dw, got_db)
    check_bf16(name + "/dx", got_dx, dx64, dx32)


@pytest.mark.parametrize("rows,cols", [(129, 520), (4, 1408), (1000, 1024)])
def test_layernorm_bwd_without_dx(B, rows, cols):
    """dx == NULL: the statistics and dw / db only (the frozen-input LayerNorm of the projector)"""
    x, dy, w, _, dw0, db0 = _ln_inputs(rows, cols, False, True)
    dw, db = Out(cols, F32), Out(cols, F32)
    dw.t.copy_(dw0)
    db.t.copy_(db0)
    stats = B.layernorm_bwd(_cuda(x), _cuda(w), _cuda(dy), None, None, dw.t, db.t, rows, cols, LN_EPS)
    _ln_check(f"layernorm_bwd/no_dx/{rows}x{cols}", x, dy, w, None, dw0, db0, stats.cpu(), dw.host(), db.host())


def test_layernorm_bwd_and_gather_refuse_misaligned_views(B):
    x = torch.zeros(4 * 64 + 8, dtype=BF, device="cuda")
    ok, bad = x[:256].view(4, 64), x[4:260].view(4, 64)
    w, dw, db = (torch.zeros(64, dtype=F32, device="cuda") for _ in range(3))
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    for args in ((bad, w, ok, None, ok), (ok, w, bad, None, ok), (ok, w, ok, bad, ok), (ok, w, ok, None, bad)):
        with pytest.raises(ValueError, match="16-byte"):
            B.layernorm_bwd(*args, dw, db, 4, 64, LN_EPS)
    for src, dst in ((bad, ok), (ok, bad)):
        with pytest.raises(ValueError, match="16-byte"):
            B.gather_rows_idx(src, idx, dst, 4, 64)
    with pytest.raises(ValueError, match="I % 16"):
        B.swiglu_fwd(ok, ok, 4, 24)
    with pytest.raises(ValueError, match="odd head_dim"):
        B.rope_bwd_assemble(ok, w, w, ok, w, w, idx, 1, 1, 1, 1, 7, 1)
    # empty and ineligible sizes, on allocations large enough for what the call names
    lg, big = torch.zeros(4 * 128, dtype=F32, device="cuda"), torch.zeros(4, 128, dtype=BF, device="cuda")
    for word, call in (
            ("gelu_fwd", lambda: B.gelu_fwd(ok, ok, 0)), ("gelu_bwd", lambda: B.gelu_bwd(ok, ok, ok, -1)),
            ("swiglu_fwd", lambda: B.swiglu_fwd(ok, ok, 0, 16)), ("swiglu_bwd", lambda: B.swiglu_bwd(ok, ok, ok, 2, 24)),
            ("cols % 8", lambda: B.gather_rows_idx(ok, idx, ok, 4, 60)), ("gather_rows_idx", lambda: B.gather_rows_idx(ok, idx, ok, 0, 64)),
            ("segment_sum_rows", lambda: B.segment_sum_rows(ok, idx, 0, 2, ok, 2, 8)), ("acc_rows_f32", lambda: B.acc_rows_f32(w, ok, 0, 64, 2, 8)),
            ("rope_bwd_assemble", lambda: B.rope_bwd_assemble(ok, w, w, ok, w, w, idx, 1, 2, 1, 1, 8, 1)),          # cache rows shorter than S
            ("cross_entropy", lambda: B.cross_entropy(lg, idx, 4, 0, 128, 1.0, dw)),                                 # row % S on the device
            ("cross_entropy", lambda: B.cross_entropy(lg, idx, 4, 2, 0, 1.0, dw)),
            ("cross_entropy", lambda: B.cross_entropy(lg, idx, 4, 2, 128, 1.0, dw, ok)),                             # ldd 64 < V
            ("softmax_fwd", lambda: B.softmax_fwd(lg.view(4, 128), ok, 4, 1, 4, 65, 1.0)),                           # Sk > ldp
            ("softmax_bwd", lambda: B.softmax_bwd(big, lg.view(4, 128), ok, 4, 65, 1.0)),                            # Sk > ldds
            ("adamw", lambda: B.adamw(w, w, w, w, w, 64, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0)),
            ("transpose", lambda: B.transpose_batched(ok, 64, 0, 0, ok, 64, 0, 0, 4, 64, 300, 300, 0))):
        with pytest.raises(ValueError, match=word):
            call()
    torch.cuda.synchronize()
    assert (x == 0).all() and (dw == 0).all() and (w == 0).all()          # refused means not launched


# ------------------------------------------------------------------------------------------------------------------------------------
# GELU / SwiGLU, forward and backward
# ------------------------------------------------------------------------------------------------------------------------------------
def _args(seed, n):
    """pre-activations across [-8, 8], an exact 0, and a normal bulk"""
    h = _randn(seed, n) * 2.5
    k = min(n, 4001)
    h[:k] = torch.linspace(-8.0, 8.0, k)
    h[n // 2] = 0.0
    return h


@pytest.mark.parametrize("n", [100, 1000, WRAP + 77])
def test_gelu_fwd_bwd(B, n):
    h, dy = _args(n, n).to(BF), _randn(n + 1, n).to(BF)
    y, dh = Out(n), Out(n)
    B.gelu_fwd(_cuda(h), y.t, n)
    B.gelu_bwd(_cuda(h), _cuda(dy), dh.t, n)
    check_bf16(f"gelu_fwd/{n}", y.host(), R.gelu_fwd(h, F64), R.gelu_fwd(h, F32))
    check_bf16(f"gelu_bwd/{n}", dh.host(), R.gelu_bwd(h, dy, F64), R.gelu_bwd(h, dy, F32))


@pytest.mark.parametrize("rows,I", [(3, 16), (7, 48), (147, 14336), (1, 14336)])
def test_swiglu_fwd_bwd(B, rows, I):
    """rows * I: 48 (< 256), 336 (not a multiple of 256), 2107392 (> 8192 * 256).  The kernels read the interleaved [16 g | 16 u] layout; the
    reference de-interleaves by reshape and is held to an index-by-index statement of the layout in tests/test_train_ref_cpu.py"""
    assert (rows, I) != (147, 14336) or rows * I > WRAP
    g, u = _args(rows + I, rows * I).view(rows, I).clone(), _randn(rows + I + 1, rows, I) * 2
    g.view(-1)[1::37] = 90.0          # exp(90) overflows fp32: sigmoid must saturate, not turn into NaN
    g.view(-1)[2::41] = -90.0
    u.view(-1)[5::43] = 0.0
    gu = R.interleave(g, u).to(BF)
    dact = _randn(rows + I + 2, rows, I).to(BF)
    act, dgu = Out(rows * I), Out(rows * 2 * I)
    B.swiglu_fwd(_cuda(gu), act.t, rows, I)
    B.swiglu_bwd(_cuda(gu), _cuda(dact), dgu.t, rows, I)
    check_bf16(f"swiglu_fwd/{rows}x{I}", act.host(), R.swiglu_fwd(gu, I, F64), R.swiglu_fwd(gu, I, F32))
    check_bf16(f"swiglu_bwd/{rows}x{I}", dgu.host(), R.swiglu_bwd(gu, dact, I, F64), R.swiglu_bwd(gu, dact, I, F32))


# ------------------------------------------------------------------------------------------------------------------------------------
# RoPE backward + re-assembly of the fused-QKV gradient
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hq,Hkv,D,S", [(32, 8, 128, 5), (8, 8, 64, 7), (4, 1, 128, 9), (32, 8, 128, 400)])
def test_rope_bwd_assemble(B, Hq, Hkv, D, S):
    """Bn = 2, cache rows longer than the sequence (Sk_ld > S), arbitrary non-monotone positions; S = 400 at (32, 8, 128) is above 8192 * 256 work items"""
    Bn, Sk_ld, n_pos = 2, S + 3, 600
    assert S != 400 or Bn * S * (Hq + 2 * Hkv) * (D // 2) > WRAP
    pos = torch.randint(0, n_pos, (Bn * S,), generator=_gen(S), dtype=torch.int32)
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=F64) / D))
    ang = torch.arange(n_pos, dtype=F64)[:, None] * inv_freq[None, :]
    cosT, sinT = ang.cos().float(), ang.sin().float()
    dq = _randn(S + 1, Bn * S, Hq, D).to(BF)
    dk, dv = _randn(S + 2, Bn, Hkv, Sk_ld, D), _randn(S + 3, Bn, Hkv, Sk_ld, D)
    QKV = (Hq + 2 * Hkv) * D
    out = Out(Bn * S * QKV)
    B.rope_bwd_assemble(_cuda(dq), _cuda(dk), _cuda(dv), out.t, _cuda(cosT), _cuda(sinT), _cuda(pos), Bn, S, Hq, Hkv, D, Sk_ld)
    got = out.host().view(Bn * S, QKV)
    check_bf16(f"rope_bwd_assemble/{Hq}-{Hkv}-{D}/S{S}", got, R.rope_bwd_assemble(dq, dk, dv, cosT, sinT, pos, Bn, S, Hq, Hkv, D, F64),
               R.rope_bwd_assemble(dq, dk, dv, cosT, sinT, pos, Bn, S, Hq, Hkv, D, F32))
    v_rows = dv[:, :, :S].permute(0, 2, 1, 3).reshape(Bn * S, Hkv * D)
    assert torch.equal(got[:, (Hq + Hkv) * D:], v_rows.to(BF)), "the V part is a pure fp32 -> bf16 copy"


# ------------------------------------------------------------------------------------------------------------------------------------
# cross-entropy: loss rows + dlogits
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ldd", [(1000, 1024), (32000, 32064), (32003, 32064), (255, 256), (257, 320)])
def test_cross_entropy(B, V, ldd):
    """Bn = 3 sequences of 5: the last position of every sequence is ignored even though the next sequence starts with a valid label (a kernel
    that reads labels[row + 1] across the boundary would score it); -100 labels; a label >= V counts as ignored (torch raises on it: see
    tests/train_ref.py); one row with a 1e4 logit on its target and one with it elsewhere; inv_n = 1/7"""
    Bn, S = 3, 5
    rows, inv_n = Bn * S, R.f32(1.0 / 7.0)
    logits = _randn(V, Bn, S, V) * 3
    labels = torch.randint(0, V, (Bn, S), generator=_gen(V + 1), dtype=torch.int32)
    labels[0, 2] = -100
    labels[2, 1] = -100
    labels[1, 4] = V + 5
    assert (labels[1:, 0] >= 0).all()
    logits[0, 0, labels[0, 1]] = 1e4
    logits[2, 2, (int(labels[2, 3]) + 1) % V] = 1e4
    loss, d = Out(rows, F32), Out(rows * ldd)
    B.cross_entropy(_cuda(logits.view(rows, V)), _cuda(labels.view(-1)), rows, S, V, inv_n, loss.t, d.t.view(rows, ldd))
    got_loss, got_d = loss.host(), d.host().view(rows, ldd)
    l64, d64, terms = R.cross_entropy(logits, labels, inv_n, F64)
    l32, d32, _ = R.cross_entropy(logits, labels, inv_n, F32)
    ignored = (R.ce_targets(labels.long(), V).reshape(-1) < 0)
    assert ignored.view(Bn, S)[:, -1].all() and int(ignored.sum()) == Bn + 3
    assert (got_loss[ignored] == 0).all() and (got_d[ignored] == 0).all(), "an ignored row is exactly 0"
    assert (got_d[:, V:] == 0).all(), "padding columns up to ldd must be exactly 0"
    ref64, ref32 = torch.zeros(rows, ldd, dtype=F64), torch.zeros(rows, ldd, dtype=F32)
    ref64[:, :V], ref32[:, :V] = d64, d32
    check_bf16(f"cross_entropy/dlogits/V{V}", got_d, ref64, ref32)
    check_f32(f"cross_entropy/loss_rows/V{V}", got_loss, l64, l32, terms)
    # loss only (dlogits == NULL)
    loss2 = Out(rows, F32)
    B.cross_entropy(_cuda(logits.view(rows, V)), _cuda(labels.view(-1)), rows, S, V, inv_n, loss2.t, None)
    assert torch.equal(loss2.host(), got_loss)


# ------------------------------------------------------------------------------------------------------------------------------------
# row movers
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,n_src,cols", [(5, 3, 8), (300, 77, 4096), (4200, 500, 4096)])
def test_gather_rows_idx_is_exact(B, rows, n_src, cols):
    assert rows != 4200 or rows * (cols // 8) > WRAP
    src = _randn(rows, n_src, cols).to(BF)
    idx = torch.randint(-2, n_src, (rows,), generator=_gen(rows + 1), dtype=torch.int32)          # negative (-> zeros) and repeated
    idx[0], idx[-1] = -1, idx[rows // 2]
    dst = Out(rows * cols)
    B.gather_rows_idx(_cuda(src), _cuda(idx), dst.t, rows, cols)
    assert torch.equal(dst.host().view(rows, cols), R.gather_rows_idx(src, idx))


@pytest.mark.parametrize("n_src,rows_per,cols,n_dst,seg", [(6, 5, 72, 4, [2, 0, 2, 2, -1, 0]), (1, 1, 1, 1, [0]), (3, 32, 4096, 2, [5, -1, 7]),
                                                            (25, 32, 4096, 17, None)])
def test_segment_sum_rows(B, n_src, rows_per, cols, n_dst, seg):
    """repeated, negative and out-of-range segment numbers; empty segments give zeros; 17 x 32 x 4096 is above 8192 * 256 elements"""
    assert seg is not None or n_dst * rows_per * cols > WRAP
    seg = torch.tensor(seg, dtype=torch.int32) if seg is not None else torch.randint(0, n_dst - 2, (n_src,), generator=_gen(3), dtype=torch.int32)
    src = _randn(n_src + cols, n_src * rows_per, cols).to(BF)
    dst = Out(n_dst * rows_per * cols)
    B.segment_sum_rows(_cuda(src), _cuda(seg), n_src, rows_per, dst.t, n_dst, cols)
    got = dst.host().view(n_dst * rows_per, cols)
    ref64 = R.segment_sum_rows(src, seg, rows_per, n_dst, F64)
    check_bf16(f"segment_sum_rows/{n_src}x{rows_per}x{cols}->{n_dst}", got, ref64, R.segment_sum_rows(src, seg, rows_per, n_dst, F32))
    empty = [r for r in range(n_dst) if r not in seg.tolist()]
    assert all((got.view(n_dst, rows_per, cols)[r] == 0).all() for r in empty)


@pytest.mark.parametrize("rows,cols,n_batches,pad", [(3, 10, 2, 34), (1, 1, 1, 0), (32, 4096, 5, 4096 * 200), (600, 4096, 3, 128)])
def test_acc_rows_f32_adds_into_the_output(B, rows, cols, n_batches, pad):
    n, stride = rows * cols, rows * cols + pad
    assert rows != 600 or n > WRAP
    src = _randn(rows + cols, n_batches * stride).to(BF)
    out0 = _randn(rows + cols + 1, n)
    out = Out(n, F32)
    out.t.copy_(out0)
    B.acc_rows_f32(out.t, _cuda(src), n_batches, stride, rows, cols)
    ref64, terms = R.acc_rows(out0, src, n_batches, stride, n, F64)
    check_f32(f"acc_rows_f32/{rows}x{cols}x{n_batches}", out.host(), ref64, R.acc_rows(out0, src, n_batches, stride, n, F32)[0], terms)


# ------------------------------------------------------------------------------------------------------------------------------------
# fused AdamW
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t,wd,work_bf16", [(1000, 1, 0.0, True), (1000, 2, 0.01, False), (1000, 1000, 0.01, True), (77, 1000, 0.0, False),
                                              (WRAP + 77, 2, 0.01, True), (WRAP + 77, 1000, 0.0, False)])
def test_adamw(B, n, t, wd, work_bf16):
    from oracle import train_oracle as TO
    lr, b1, b2, eps, wd = R.f32(1e-3), R.f32(0.9), R.f32(0.999), R.f32(1e-8), R.f32(wd)          # the floats the C ABI delivers
    p0, g0 = _randn(n, n), _randn(n + 1, n)
    g0[::5] = 0.0
    m0 = 0.1 * _randn(n + 2, n) if t > 1 else torch.zeros(n)
    # t = 1 starts from zero moments (g = 0 there: 0 / (0 + eps), no NaN); later steps keep v away from 0, where one element's step is
    # ill-conditioned (sqrt(v) ~ eps) and, delta being a maximum over the output, would alone set the bound of all n
    v0 = 1e-3 + 0.01 * torch.rand(n, generator=_gen(n + 3)) if t > 1 else torch.zeros(n)
    outs = [Out(n, F32) for _ in range(4)]
    for o, init in zip(outs, (p0, m0, v0, g0)):
        o.t.copy_(init)
    work = Out(n, BF if work_bf16 else F32)
    B.adamw(*(o.t for o in outs), work.t, n, lr, b1, b2, eps, wd, t)
    p, m, v, g = (o.host() for o in outs)
    r64 = TO.adamw_step(p0.double(), g0.double(), m0.double(), v0.double(), t, lr, b1, b2, eps, wd)
    r32 = TO.adamw_step(p0, g0, m0, v0, t, lr, b1, b2, eps, wd)
    name = f"adamw/n{n}/t{t}/wd{wd:.2g}"
    step = (p0.double() * (1.0 - lr * wd) - r64[0]).abs()
    check_f32(name + "/p", p, r64[0], r32[0], p0.double().abs() + step)
    check_f32(name + "/m", m, r64[1], r32[1], (b1 * m0.double()).abs() + ((1.0 - b1) * g0.double()).abs())
    check_f32(name + "/v", v, r64[2], r32[2], (b2 * v0.double()).abs() + (1.0 - b2) * g0.double() ** 2)
    assert (g == 0).all(), "the gradient is cleared for the next accumulation"
    got_work = work.host()
    assert torch.equal(got_work, p.to(BF) if work_bf16 else p), "the working copy is the (bf16 of the) master, bitwise"


# ------------------------------------------------------------------------------------------------------------------------------------
# batched, col0-offset transposition: dst[o][i][c][col0 + r] = src[o][i][r][c]
# ------------------------------------------------------------------------------------------------------------------------------------
# (R, C, n_outer, n_inner, col0, stride padding, kernel the launcher takes)
TRANSPOSE = [
    (40, 24, 2, 3, 8, 8, "64"), (200, 136, 3, 2, 64, 16, "64"), (64, 64, 1, 1, 0, 0, "64"),
    (33, 47, 2, 3, 5, 3, "32"), (40, 24, 2, 3, 3, 8, "32"), (1024, 1024, 1, 2, 3, 8, "32"),
    (1024, 1032, 2, 2, 16, 8, "128"), (1160, 1024, 1, 3, 1024, 24, "128"),
]


@pytest.mark.parametrize("R_,C_,n_outer,n_inner,col0,pad,kernel", TRANSPOSE)
def test_transpose_batched_is_exact_and_stays_inside(B, R_, C_, n_outer, n_inner, col0, pad, kernel):
    """all three kernels in their batched forms: 128^2 tiles (everything a multiple of 8, R and C >= 1024), 64^2 tiles (multiples of 8), 32^2 (the
    rest: a col0 or a stride off the multiple of 8).  The whole destination buffer is compared, so nothing outside the addressed blocks may change"""
    src_rs, dst_rs = C_ + pad, col0 + R_ + pad
    src_si, dst_si = R_ * src_rs + 8 * pad, C_ * dst_rs + 8 * pad
    src_so, dst_so = n_inner * src_si + 16 * pad, n_inner * dst_si + 16 * pad
    wide = all(v % 8 == 0 for v in (src_rs, src_so, src_si, dst_rs, dst_so, dst_si, R_, C_, col0))
    assert {"128": wide and R_ >= 1024 and C_ >= 1024, "64": wide and not (R_ >= 1024 and C_ >= 1024), "32": not wide}[kernel]
    src = _randn(R_ + C_, n_outer * src_so).to(BF)
    dst = Out(n_outer * dst_so)
    B.transpose_batched(_cuda(src), src_rs, src_so, src_si, dst.t, dst_rs, dst_so, dst_si, R_, C_, n_outer, n_inner, col0)
    want = torch.full((n_outer * dst_so,), SENT, dtype=BF)
    for o in range(n_outer):
        for i in range(n_inner):
            block = src.as_strided((R_, C_), (src_rs, 1), o * src_so + i * src_si)
            want.as_strided((C_, R_), (dst_rs, 1), o * dst_so + i * dst_si + col0).copy_(block.t())
    assert torch.equal(dst.host(), want)
