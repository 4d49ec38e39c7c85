"""How an LM pass picks its attention route, host side (no device work): the pure part of the pass plan
(engine.cpp lm_attn_route, exported as vv_diag_lm_attn_route) swept against the rule include/vibevoice_hip.h
states for the four per-context options, and the one options check of the Python side
(weights.check_lm_options) against the separate checks it calls.
"""
import ctypes
import itertools
import os
import re

import pytest

from vibevoice_amd import _lib
from vibevoice_amd.weights import (check_kv_dtype, check_lm_attn_kv8, check_lm_attn_max_keys, check_lm_attn_max_rows,
                                   check_lm_attn_w8, check_lm_options, check_weight_dtype)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8 = "fp8_e4m3"
BF16, W8, MIXED = 0, 1, 2   # how every layer's qkv_w / o_w are bound

# vibevoice_hip.h, vv_set_lm_attn_w8: all FP8 pairs run the W8 form with the option, the three launches without
# it; all bf16 runs the bf16 form whatever the option; a mix runs the three launches.
# (binding, option) -> the kernel's weight form, None = the three launches
WEIGHTS = {(BF16, 0): "bf16", (BF16, 1): "bf16", (W8, 0): None, (W8, 1): "w8", (MIXED, 0): None, (MIXED, 1): None}
# vv_set_kv_dtype / vv_set_lm_attn_kv8: under FP8 KV the kernel is off unless the option; without an FP8 KV cache
# the option has no effect.  (kv_dtype, option) -> (the kernel may run, its rows are quantised in the launch)
KV = {(0, 0): (True, False), (0, 1): (True, False), (1, 0): (False, True), (1, 1): (True, True)}


def test_export_and_header():
    L = _lib.lib()
    assert len(L.vv_diag_lm_attn_route.argtypes) == 12
    product = open(os.path.join(ROOT, "include", "vibevoice_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "vibevoice_hip_diag.h")).read()
    assert re.search(r"^int vv_diag_lm_attn_route\(int attn_form, int kv_dtype, int w8, int kv8, int max_keys, "
                     r"int max_rows, int max_ctx,\n\s+int kvround, int staged, int rows, int keys, int\* out\);",
                     diag, re.M)
    assert "vv_diag_lm_attn_route" not in product
    assert L.vv_diag_lm_attn_route(0, 0, 0, 0, 4096, 16, 4096, 0, 1, 1, 1, None) != 0


def test_route_follows_the_headers_rule():
    L = _lib.lib()
    out = (ctypes.c_int * 3)()
    built = (ctypes.c_int * 4)()
    max_ctx, n = 8192, 0
    for form, kv_dtype, w8, kv8, kvround, max_keys, max_rows, rows, keys in itertools.product(
            (BF16, W8, MIXED), (0, 1), (0, 1), (0, 1), (0, 1), (4096, 8192), (16, 32), (1, 16, 17, 32),
            (1, 4096, 4097, 8192)):
        weights = WEIGHTS[form, w8]
        kv_ok, quantised = KV[kv_dtype, kv8]
        # kvq: 1 the FP8 cache's quantiser; 2 the diagnostic round trip (vv_lm_attn_kvround: a bf16-weight,
        # bf16-KV context only); else 0
        kvq = 1 if quantised else 2 if kvround and form == BF16 else 0
        # vv_set_lm_attn_max_keys: <= 4,096 keys, or <= the option (itself <= max_ctx);
        # vv_set_lm_attn_max_rows: <= 16 rows, or <= the option with raw rows into a bf16 cache
        keys_ok = keys <= 4096 or keys <= min(max_keys, max_ctx)
        rows_ok = rows <= 16 or (rows <= max_rows and kvq == 0)
        one = weights is not None and kv_ok and keys_ok and rows_ok
        out[:] = [-1] * 3
        args = (form, kv_dtype, w8, kv8, max_keys, max_rows, max_ctx, kvround, 1, rows, keys)
        assert L.vv_diag_lm_attn_route(*args, out) == 0
        assert tuple(out) == (int(one), int(weights == "w8"), kvq), (args, tuple(out))
        # ... and with the form table (which forms are built): an FP8-KV context keeps its launches past
        # 4,096 keys and above 16 rows whatever the values
        runs = one and L.vv_diag_lm_attn_form_rows(out[1], out[2], keys, rows, built) == 0
        if kv_dtype and (keys > 4096 or rows > 16):
            assert not runs, args
        if kvq == 0 and one:
            assert runs, args
        n += 1
    assert n == 3 * 2 * 2 * 2 * 2 * 2 * 2 * 4 * 4
    # max_ctx bounds the option; without a staging cache there is no round trip
    assert L.vv_diag_lm_attn_route(BF16, 0, 0, 0, 8192, 16, 4096, 0, 1, 2, 4097, out) == 0 and out[0] == 0
    assert L.vv_diag_lm_attn_route(BF16, 0, 0, 0, 4096, 16, 4096, 1, 0, 2, 64, out) == 0 and tuple(out) == (1, 0, 0)
    assert L.vv_diag_lm_attn_route(BF16, 0, 0, 0, 4096, 16, 4096, 1, 1, 2, 64, out) == 0 and tuple(out) == (1, 0, 2)


def test_check_lm_options_returns_what_the_separate_checks_return():
    for wd, kd, w8, kv8, keys, rows in itertools.product((None, FP8), (None, FP8), (False, True, 0, 1), (False, True),
                                                         (None, 4096, 8192), (None, 16, 32)):
        def separate():
            return dict(lm_attn_max_keys=check_lm_attn_max_keys(keys, 8192, 1),
                        lm_attn_max_rows=check_lm_attn_max_rows(rows, 1),
                        weight_dtype=check_weight_dtype(wd, 1), kv_dtype=check_kv_dtype(kd, 1),
                        lm_attn_kv8=check_lm_attn_kv8(kv8, kd, 1),
                        lm_attn_w8=check_lm_attn_w8(w8, wd, kd, 1, lm_attn_kv8=kv8))
        try:
            want = separate()
        except ValueError as e:
            with pytest.raises(ValueError, match=re.escape(str(e))):
                check_lm_options(wd, kd, w8, kv8, keys, rows, max_ctx=8192)
            continue
        got = check_lm_options(wd, kd, w8, kv8, keys, rows, max_ctx=8192)
        assert got == want and type(got["lm_attn_w8"]) is bool
    # packed: the weight format is the packed weights', whatever weight_dtype says
    assert check_lm_options(None, None, True, False, None, None, max_ctx=64,
                            packed={"lm.0.qkv_w8": None})["weight_dtype"] == FP8
    with pytest.raises(ValueError, match="FP8 weights"):
        check_lm_options(FP8, None, True, False, None, None, max_ctx=64, packed={"lm.0.qkv_w": None})


def test_check_lm_options_raises_the_first_check_in_engine_order():
    """Engine's order: lm_attn_max_keys, lm_attn_max_rows, weight_dtype, kv_dtype, lm_attn_kv8, lm_attn_w8."""
    bad = dict(lm_attn_max_keys=(100, "lm_attn_max_keys=100 is outside"), lm_attn_max_rows=(33, "lm_attn_max_rows=33 is outside"),
               weight_dtype=("int4", "weight_dtype='int4' is not supported"), kv_dtype=("int4", "kv_dtype='int4' is not supported"),
               lm_attn_kv8=("yes", "lm_attn_kv8='yes'"), lm_attn_w8=("yes", "lm_attn_w8='yes'"))
    order = list(bad)
    ok = dict(weight_dtype=None, kv_dtype=None, lm_attn_w8=False, lm_attn_kv8=False, lm_attn_max_keys=None,
              lm_attn_max_rows=None)
    for i, j in itertools.combinations(range(len(order)), 2):
        kw = dict(ok, **{order[i]: bad[order[i]][0], order[j]: bad[order[j]][0]})
        with pytest.raises(ValueError, match=re.escape(bad[order[i]][1])):
            check_lm_options(kw["weight_dtype"], kw["kv_dtype"], kw["lm_attn_w8"], kw["lm_attn_kv8"],
                             kw["lm_attn_max_keys"], kw["lm_attn_max_rows"], max_ctx=8192)
    # tensor parallelism: every option refuses it, the first in that order names itself
    with pytest.raises(ValueError, match="lm_attn_max_keys is not supported with tensor parallelism"):
        check_lm_options(FP8, FP8, True, True, 4096, 32, max_ctx=8192, tp_size=2)
    with pytest.raises(ValueError, match="weight_dtype='fp8_e4m3' is not supported with tensor parallelism"):
        check_lm_options(FP8, FP8, True, True, None, None, max_ctx=8192, tp_size=2)


def test_check_lm_options_types_only_without_max_ctx():
    for keys in (4096, 8192, 1 << 20, 1 << 40):
        assert check_lm_options(None, None, False, False, keys, None, max_ctx=None)["lm_attn_max_keys"] == keys
    with pytest.raises(ValueError, match="outside"):
        check_lm_options(None, None, False, False, 8192, None, max_ctx=4096)
    with pytest.raises(ValueError, match="outside"):
        check_lm_options(None, None, False, False, 4095, None, max_ctx=None)
    for wrong in (True, 4096.0, "all"):
        with pytest.raises(ValueError, match="expected None or an int"):
            check_lm_options(None, None, False, False, wrong, None, max_ctx=None)
    with pytest.raises(ValueError, match="expected None or an int"):
        check_lm_options(None, None, False, False, None, "32", max_ctx=None)
