"""The one-launch LM attention kernel at 17 to 32 rows, host side (no device work): the
option's validation (weights.check_lm_attn_max_rows, Engine), the new exports, and the
form table with the row count (vv_diag_lm_attn_form_rows = lm_attn.hip la_form): eleven
forms, the seven of 1 .. 16 rows and, at 17 .. 32 rows, raw bf16 KV rows with bf16 or FP8
weights, short or long.
"""
import ctypes
import os
import re

import pytest

from tiny import tiny_config
from vibevoice_amd import _lib
from vibevoice_amd.engine import Engine
from vibevoice_amd.weights import check_lm_attn_max_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_and_headers():
    L = _lib.lib()
    assert len(L.vv_set_lm_attn_max_rows.argtypes) == 2 and len(L.vv_lm_attn_max_rows.argtypes) == 1
    assert len(L.vv_diag_lm_attn_form_rows.argtypes) == 5
    product = open(os.path.join(ROOT, "include", "vibevoice_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "vibevoice_hip_diag.h")).read()
    assert re.search(r"^int vv_set_lm_attn_max_rows\(vv_ctx\* ctx, int rows\);", product, re.M)
    assert re.search(r"^int vv_lm_attn_max_rows\(vv_ctx\* ctx\);", product, re.M)
    assert "an FP8-KV context keeps its\n * launches above 16 rows" in product
    assert re.search(r"^int vv_diag_lm_attn_form_rows\(int w8, int kvq, int keys, int rows, int\* out\);", diag, re.M)
    assert "vv_diag_lm_attn_form_rows" not in product
    assert L.vv_set_lm_attn_max_rows(None, 32) != 0
    assert b"vv_set_lm_attn_max_rows: null context" in L.vv_last_error()
    assert L.vv_lm_attn_max_rows(None) == 0


def test_check_lm_attn_max_rows():
    assert check_lm_attn_max_rows(None) is None and check_lm_attn_max_rows(None, 2) is None
    assert check_lm_attn_max_rows(16) == 16 and check_lm_attn_max_rows(32) == 32 and check_lm_attn_max_rows(24, 1) == 24
    for bad in (15, 33):
        with pytest.raises(ValueError, match="outside"):
            check_lm_attn_max_rows(bad)
    for bad in (True, 16.0, "32"):
        with pytest.raises(ValueError, match="expected None or an int"):
            check_lm_attn_max_rows(bad)
    with pytest.raises(ValueError, match="tensor parallelism"):
        check_lm_attn_max_rows(32, tp_size=2)


def test_form_table_with_rows():
    L = _lib.lib()
    f, f16 = L.vv_diag_lm_attn_form_rows, L.vv_diag_lm_attn_form
    out, out16 = (ctypes.c_int * 4)(), (ctypes.c_int * 3)()
    built = set()
    for w8 in (0, 1):
        for kvq in (0, 1, 2):
            for keys in (1, 4096, 4097, 1 << 20):
                for rows in (1, 16, 17, 32):
                    lng, mt = int(keys > 4096), 1 if rows <= 16 else 2
                    exists = not (kvq == 2 and w8) and not (kvq != 0 and lng) and not (kvq != 0 and mt == 2)
                    out[:] = [-1] * 4
                    rc = f(w8, kvq, keys, rows, out)
                    assert (rc == 0) == exists, (w8, kvq, keys, rows, rc)
                    if exists:
                        assert tuple(out) == (w8, kvq, lng, mt), (w8, kvq, keys, rows, tuple(out))
                        built.add(tuple(out))
                    else:
                        assert tuple(out) == (-1, -1, -1, -1)
                    if rows <= 16:   # the table of 16 rows or fewer is vv_diag_lm_attn_form's
                        out16[:] = [-1] * 3
                        assert (f16(w8, kvq, keys, out16) == 0) == exists
                        assert tuple(out16) == tuple(out)[:3]
                for rows in (0, 33, -1):
                    assert f(w8, kvq, keys, rows, out) != 0
                assert f(w8, kvq, keys, 16, None) != 0 and f(w8, kvq, keys, 32, None) != 0
            assert f(w8, kvq, 0, 32, out) != 0 and f(w8, kvq, (1 << 20) + 1, 32, out) != 0
    old = {(0, 0, 0, 1), (1, 0, 0, 1), (0, 1, 0, 1), (1, 1, 0, 1), (0, 2, 0, 1), (0, 0, 1, 1), (1, 0, 1, 1)}
    assert built == old | {(0, 0, 0, 2), (1, 0, 0, 2), (0, 0, 1, 2), (1, 0, 1, 2)} and len(built) == 11
    assert f(2, 0, 1, 17, out) != 0 and f(0, 3, 1, 17, out) != 0 and f(0, -1, 1, 17, out) != 0


def test_engine_keyword():
    cfg = tiny_config()
    with pytest.raises(ValueError, match="outside"):
        Engine(cfg, None, "cpu", lm_attn_max_rows=33)
    with pytest.raises(ValueError, match="tensor parallelism"):
        Engine(cfg, None, "cpu", tp_size=2, lm_attn_max_rows=32)
    # an accepted value gets past the validation: the next refusal is the device's
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        Engine(cfg, None, "cpu", max_batch=16, lm_attn_max_rows=32)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        Engine(cfg, None, "cpu", max_ctx=8192, lm_attn_max_keys=8192, lm_attn_max_rows=32)
