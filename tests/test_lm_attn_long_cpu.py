"""The one-launch LM attention kernel past 4,096 keys, host side (no device work):
the option's validation (weights.check_lm_attn_max_keys, Engine, the model class),
the new exports, and the unit plan the kernel evaluates per row
(vv_diag_lm_attn_plan = kernels.h la_unit_steps / la_unit_count): s = 1 up to 4,096
keys (the short form's units), the units tile [0, len) exactly, at most 128 units
per (row, kv head) -- the merge wave holds two (m, l) per lane."""
import ctypes
import os
import re

import pytest

from tiny import tiny_config
from vibevoice_amd import _lib
from vibevoice_amd.engine import Engine
from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference as M
from vibevoice_amd.weights import check_lm_attn_max_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT_CAP = 128


def test_exports_and_headers():
    L = _lib.lib()
    assert len(L.vv_set_lm_attn_max_keys.argtypes) == 2 and len(L.vv_lm_attn_max_keys.argtypes) == 1
    assert len(L.vv_diag_lm_attn_plan.argtypes) == 2
    product = open(os.path.join(ROOT, "include", "vibevoice_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "vibevoice_hip_diag.h")).read()
    assert re.search(r"^int vv_set_lm_attn_max_keys\(vv_ctx\* ctx, int keys\);", product, re.M)
    assert re.search(r"^int vv_lm_attn_max_keys\(vv_ctx\* ctx\);", product, re.M)
    assert re.search(r"^int vv_diag_lm_attn_plan\(int len, int\* out\);", diag, re.M)
    assert L.vv_set_lm_attn_max_keys(None, 8192) != 0
    assert b"vv_set_lm_attn_max_keys: null context" in L.vv_last_error()
    assert L.vv_lm_attn_max_keys(None) == 0
    out = (ctypes.c_int * 2)()
    assert L.vv_diag_lm_attn_plan(0, out) != 0 and L.vv_diag_lm_attn_plan(1, None) != 0


def test_check_lm_attn_max_keys():
    assert check_lm_attn_max_keys(None) is None and check_lm_attn_max_keys(None, 64, 2) is None
    assert check_lm_attn_max_keys(4096, 4096) == 4096 and check_lm_attn_max_keys(8192, 8192) == 8192
    assert check_lm_attn_max_keys(5000, 65536, 1) == 5000
    for bad, ctx in ((4095, 8192), (8193, 8192), (0, 8192), (-1, 8192), (4096, 64)):
        with pytest.raises(ValueError, match="outside"):
            check_lm_attn_max_keys(bad, ctx)
    for bad in (True, 8192.0, "8192"):
        with pytest.raises(ValueError, match="expected None or an int"):
            check_lm_attn_max_keys(bad, 8192)
    with pytest.raises(ValueError, match="tensor parallelism"):
        check_lm_attn_max_keys(8192, 8192, 2)


def test_engine_and_model_validate_before_touching_a_device():
    cfg = tiny_config()
    with pytest.raises(ValueError, match="outside"):
        Engine(cfg, None, "cpu", max_ctx=8192, lm_attn_max_keys=8193)
    with pytest.raises(ValueError, match="tensor parallelism"):
        Engine(cfg, None, "cpu", max_ctx=8192, tp_size=2, lm_attn_max_keys=8192)
    with pytest.raises(ValueError, match="outside"):
        M(cfg, None, "cpu", max_ctx=8192, lm_attn_max_keys=4000)
    with pytest.raises(ValueError, match="expected None or an int"):
        M.from_pretrained("synthetic:1.5B", lm_attn_max_keys="all")


def test_unit_plan_every_length():
    L = _lib.lib()
    out = (ctypes.c_int * 2)()
    seen = set()
    for n in range(1, 65537):
        assert L.vv_diag_lm_attn_plan(n, out) == 0
        s, units = out[0], out[1]
        if n <= 4096:
            assert s == 1 and units == (n + 31) // 32, n
        assert s >= 1 and 1 <= units <= UNIT_CAP, (n, s, units)
        # units of 32 s keys tile [0, n): the last one starts inside the row and ends at or past its end
        assert (units - 1) * 32 * s < n <= units * 32 * s, (n, s, units)
        seen.add(s)
    assert seen == set(range(1, 17))
