"""The route plan of the linears (csrc/linear_route.hip) through vz_op_linear_route - no GPU needed: the library's CU-count defaults
are the MI355X's 256.

tests/golden/linear_routes.json holds, for every linear of tools/route_sweep.py's case list, the route the dispatch code from BEFORE
the planner took: the answers of tools/route_oracle.hip, which keeps that code (`route_sweep.py oracle golden`), not the planner's own.
`route_sweep.py golden` derives the same table from a kernel trace of the sweep on an MI355X."""
import json
import os

import pytest

from util import REPO

ROUTE_KNOBS = (9, 14, 19)      # skinny_mode, decode_tile_rows, wide_mode: the golden table's k9 / k14 / k19 columns


@pytest.fixture(scope="module")
def B():
    from test_abi_cpu import _ensure_built
    from vz_hip import binding
    binding.load_library(_ensure_built())
    with binding.tuned(*[(k, binding.tune_get(k)) for k in ROUTE_KNOBS]):       # whatever a test leaves, the module puts back what it found
        yield binding


def _zephyr_decode_shapes():
    """(name, N, K, act, out_fp32, flags): QKV, O, gate|up, down, lm_head of BASELINE.json's model (Zephyr-7B)"""
    cfg = json.load(open(os.path.join(REPO, "BASELINE.json"))).get("model", {})
    H, I, V = cfg.get("hidden", 4096), cfg.get("inter", 14336), cfg.get("vocab", 32000)
    nh, nkv, hd = cfg.get("n_heads", 32), cfg.get("n_kv_heads", 8), cfg.get("head_dim", 128)
    NORM, RES = 8, 32
    return [("qkv", (nh + 2 * nkv) * hd, H, 0, 0, NORM), ("o", H, nh * hd, 0, 0, RES), ("gate_up", 2 * I, H, 3, 0, NORM),
            ("down", H, I, 0, 0, RES), ("lm_head", V, H, 0, 1, NORM)]


def test_zephyr_shapes_are_the_issue_s():
    assert [(n, N, K) for n, N, K, _, _, _ in _zephyr_decode_shapes()] == [("qkv", 6144, 4096), ("o", 4096, 4096), ("gate_up", 28672, 4096),
                                                                          ("down", 4096, 14336), ("lm_head", 32000, 4096)]


def test_route_table_is_the_one_from_before_the_planner(B):
    doc = json.load(open(os.path.join(REPO, "tests", "golden", "linear_routes.json")))
    table = [dict(zip(doc["columns"], row)) for row in doc["rows"]]
    assert len(table) >= 2000
    assert {t["route"] for t in table} >= set(B.LIN_ROUTES)          # the sweep reached every kernel family
    wrong = []
    for t in table:
        with B.tuned(*[(k, t[f"k{k}"]) for k in ROUTE_KNOBS]):
            got = B.linear_route(t["M"], t["N"], t["K"], t["lda"], t["ldw"], t["act"], t["out_fp32"], t["flags"], t["entry"])[0]
        if got != t["route"]:
            wrong.append((t, got))
    assert not wrong, f"{len(wrong)} of {len(table)} routes differ, first: {wrong[:5]}"


def test_planner_equals_the_dispatch_code_it_replaced(B, tmp_path):
    """tools/route_oracle.hip keeps the dispatch code from before the planner (linear(), vz_launch_linear, the vz_launch_skinny form
    choice, vz_wide_engine_ok, the op entry points) with its launches turned into return values.  Against vz_plan_linear and
    vz_op_linear_route over knob 9 in 0..7, knob 14 in {29, 17, 65, 40, 8, 1}, knob 19, 12 N x 10 K x 3 activations, 1..700 rows, decode or
    not, norm or not, six sets of weight copies, two caller split-K hints: route, copy read, stand-alone norm, split-K hint and profile
    class must all agree (the program prints the first differences and their count)."""
    import subprocess
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import route_sweep
    exe = route_sweep.oracle_build(str(tmp_path))
    run = subprocess.run([exe, "grid"], capture_output=True, text=True)
    tail = run.stdout[-3000:]
    assert run.returncode == 0 and " 0 differ" in tail, tail


@pytest.mark.parametrize("wflags", [0, 1, 2, 2 | 4], ids=["bf16", "bf16+tiled", "e4m3", "e4m3+tiled"])
def test_every_decode_row_count_has_a_route(B, wflags):
    for M in range(1, 65):
        for name, N, K, act, f32, flags in _zephyr_decode_shapes():
            route, pre, sk = B.linear_route(M, N, K, act=act, out_fp32=f32, flags=wflags | flags | B.ROUTE_DECODE)
            assert route in B.LIN_ROUTES, (M, name, route)
            # a norm that cannot ride in the kernel ran before it, and only a normed linear has one
            assert not pre or flags & B.ROUTE_NORM, (M, name)
            assert sk == 0 or route == "TILE128", (M, name, sk)


def test_non_decode_plan_does_not_depend_on_rows_within_17_512(B):
    """the batch invariance tests/test_stages_gpu.py::test_qformer relies on (block 0's self-attention runs once per sample on 32 rows, the
    per-tile blocks on 32 x tiles): route, split-K hint and pre-norm of a non-decode caller are the same for every M in 17..512 - for every
    Q-Former linear (hidden 4096: sa_in, sa_out / ca_q / ca_out, block 0's K|V rows, ffn1, ffn2) and for the Zephyr QKV / O / down shapes.
    Zephyr's gate|up and lm_head are the exception the tile GEMMs have always had (gemm.hip: the 128^2 / 256^2 choice follows the tile
    count, i.e. M - 112 and 125 column tiles reach the 256^2 kernel's 160 from 257 rows on): no Q-Former shape is near it, and for those
    two only the tile size may change."""
    H = 4096
    invariant = [(3 * H, H, 0), (H, H, 0), (2 * H, H, 0), (2 * H, H, 2), (H, 2 * H, 0), (6144, 4096, 0), (4096, 14336, 0)]
    tile_size_only = [(28672, 4096, 3), (32000, 4096, 0)]
    for N, K, act in invariant + tile_size_only:
        for wflags in (0, 1, 2):
            plans = {B.linear_route(M, N, K, act=act, flags=wflags | B.ROUTE_BIAS * (act != 3)) for M in range(17, 513)}
            assert {p[0] for p in plans} <= {"TILE128", "TILE256"} and {p[1:] for p in plans} == {(False, 0)}, (N, K, act, wflags, plans)
            if (N, K, act) in invariant:
                assert len(plans) == 1, (N, K, act, wflags, plans)
