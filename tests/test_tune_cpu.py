"""The tune knobs (csrc/tune.h: one table of numbers, names, defaults and ranges) through vz_tune_set / vz_tune_get / vz_tune_info and the
binding's names and scopes - no GPU needed."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

from util import REPO

NUMBERS = set(range(0, 8)) | {9, 10, 11, 14, 15, 16, 19} | set(range(21, 37))       # ABI: bench.py, profiles/ and DESIGN.md refer to them
CLAMPS = {24}            # the one knob whose setter clamps a value outside its range instead of refusing it


@pytest.fixture(scope="module")
def B():
    from test_abi_cpu import _ensure_built
    from vz_hip import binding
    binding.load_library(_ensure_built())
    return binding


def _set(B, knob, value):
    return B.lib().vz_tune_set(knob, value)


def test_every_knob_reads_back_its_default_in_a_fresh_process(B):
    code = ("import json, sys; sys.path.insert(0, sys.argv[2]); from vz_hip import binding as B; B.load_library(sys.argv[1]); "
            "print(json.dumps({n: [d, B.tune_get(n), B.tune_get(k)] for n, (k, d, lo, hi) in B.knobs().items()}))")
    out = subprocess.run([sys.executable, "-c", code, B.LIB_PATH, os.path.join(REPO, "vision-zephyr_amd")], capture_output=True, text=True, check=True)
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert set(got) == set(B.knobs()) and len(got) == len(NUMBERS)
    for name, (dflt, by_name, by_number) in got.items():
        assert dflt == by_name == by_number == B.knobs()[name][1], name


def test_numbers_are_the_abi_s_and_names_are_unique(B):
    rows, i = [], 0
    k, name, d, lo, hi = C.c_int(), C.c_char_p(), C.c_int(), C.c_int(), C.c_int()
    while B.lib().vz_tune_info(i, C.byref(k), C.byref(name), C.byref(d), C.byref(lo), C.byref(hi)) == B.VZ_OK:
        rows.append((k.value, name.value.decode(), d.value, lo.value, hi.value))
        i += 1
    out = [C.byref(x) for x in (k, name, d, lo, hi)]
    assert B.lib().vz_tune_info(i, *out) == B.lib().vz_tune_info(-1, *out) == B.lib().vz_tune_info(0, None, *out[1:]) == B.VZ_ERR_ARG
    assert sorted(r[0] for r in rows) == sorted(NUMBERS) and len({r[1] for r in rows}) == len(rows) == len(NUMBERS)
    assert all(lo <= d <= hi for _, _, d, lo, hi in rows), rows
    assert B.knobs() == {n: (k, d, lo, hi) for k, n, d, lo, hi in rows}


def test_set_get_round_trips_and_the_range_is_enforced(B):
    for name, (k, d, lo, hi) in B.knobs().items():
        was = B.tune_get(k)
        try:
            for v in (lo, hi):
                assert _set(B, k, v) == B.VZ_OK and B.tune_get(k) == B.tune_get(name) == v, (name, v)
            for v, edge in ((lo - 1, lo), (hi + 1, hi)):
                if not -2 ** 31 <= v < 2 ** 31:
                    continue                    # the range ends where int does
                assert _set(B, k, edge) == B.VZ_OK
                if k in CLAMPS:
                    assert _set(B, k, v) == B.VZ_OK and B.tune_get(k) == edge, (name, v)
                    assert _set(B, k, v + (v - edge) * 100) == B.VZ_OK and B.tune_get(k) == edge, (name, v)
                else:
                    assert _set(B, k, v) == B.VZ_ERR_ARG and B.tune_get(k) == edge, (name, v)
                    msg = B.lib().vz_last_error().decode()
                    assert name in msg and str(k) in msg, msg            # the refusal names the knob
                    with pytest.raises(ValueError):
                        B.tune(name, v)
        finally:
            B.tune(k, was)
    assert all(B.tune_get(n) == d for n, (_, d, _, _) in B.knobs().items())


def test_unknown_knobs_are_refused(B):
    v = C.c_int(-7)
    for k in sorted(set(range(-2, 40)) - NUMBERS) + [1000]:
        assert _set(B, k, 0) == B.VZ_ERR_ARG and B.lib().vz_tune_get(k, C.byref(v)) == B.VZ_ERR_ARG and v.value == -7, k
        with pytest.raises(ValueError):
            B.tune(k, 0)
    assert B.lib().vz_tune_get(0, None) == B.VZ_ERR_ARG
    for call in (lambda: B.tune("no_such_knob", 1), lambda: B.tune_get("no_such_knob"), lambda: B.tuned(no_such_knob=1).__enter__(),
                 lambda: B.tuned_from_args(["no_such_knob=1"]).__enter__()):
        with pytest.raises(KeyError, match="skinny_mode"):          # the message lists the known names
            call()


def test_tuned_restores_on_exit_on_error_and_nested(B):
    d = {n: v[1] for n, v in B.knobs().items()}
    with B.tuned(skinny_mode=0, gemm256_streamk=2):
        assert (B.tune_get("skinny_mode"), B.tune_get(9), B.tune_get("gemm256_streamk")) == (0, 0, 2)
        with B.tuned(skinny_mode=5, splitk_mid=0):
            assert (B.tune_get("skinny_mode"), B.tune_get("splitk_mid"), B.tune_get("gemm256_streamk")) == (5, 0, 2)
            with pytest.raises(ZeroDivisionError):
                with B.tuned((9, 7), ("decode_tile_rows", 65)):
                    assert (B.tune_get(9), B.tune_get(14)) == (7, 65)
                    1 / 0
            assert (B.tune_get("skinny_mode"), B.tune_get("decode_tile_rows")) == (5, d["decode_tile_rows"])
        assert (B.tune_get("skinny_mode"), B.tune_get("splitk_mid")) == (0, d["splitk_mid"])
    assert all(B.tune_get(n) == v for n, v in d.items())
    # a value the library refuses: what the scope had already set is put back, the refusal reaches the caller
    with pytest.raises(ValueError):
        with B.tuned(wide_mode=0, gemm_choice=3):
            pytest.fail("the scope was entered")
    assert all(B.tune_get(n) == v for n, v in d.items())
    # the same knob twice in one scope: restored in reverse order, so the first value read wins
    with B.tuned((9, 2), ("skinny_mode", 3)):
        assert B.tune_get(9) == 3
    assert B.tune_get(9) == d["skinny_mode"]


def test_a_scope_restores_the_value_it_found_not_the_default(B):
    assert B.knobs()["decode_tile_rows"][1] != 40
    B.tune("decode_tile_rows", 40)
    try:
        with B.tuned(decode_tile_rows=17):
            assert B.tune_get(14) == 17
        assert B.tune_get(14) == 40
        with B.tuned_from_args(["14=8", "wide_mode=0"]):
            assert (B.tune_get(14), B.tune_get("wide_mode")) == (8, 0)
        with B.tuned_from_args("decode_tile_rows=65,19=0,"):
            assert (B.tune_get(14), B.tune_get(19)) == (65, 0)
        assert (B.tune_get(14), B.tune_get(19)) == (40, B.knobs()["wide_mode"][1])
    finally:
        B.tune("decode_tile_rows", B.knobs()["decode_tile_rows"][1])


def test_header_lists_the_table_s_numbers_and_names(B):
    hdr = open(os.path.join(REPO, "include", "viszephyr.h")).read()
    block = hdr[hdr.index("Knobs (number  name  meaning):"):hdr.index("int vz_tune_set(")]
    listed = [(int(k), n) for k, n in re.findall(r"^ \*\s+(\d+)  (\w+) {2,}\S", block, flags=re.M)]
    assert listed == [(k, n) for n, (k, _, _, _) in B.knobs().items()]            # same pairs, same (table) order
