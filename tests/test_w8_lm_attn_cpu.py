"""The per-context option that runs the one-launch LM attention kernel on FP8
weights (host only, no device work): vv_set_lm_attn_w8 / vv_lm_attn_w8 are
exported, bound by _lib.py and declared in the product header; the C setter
rejects values other than 0 / 1 by name; and Engine / the model class refuse the
option without FP8 weights, with an FP8 KV cache and with tensor parallelism
before any device is touched."""
import re
from pathlib import Path

import pytest

from tiny import tiny_config
from vibevoice_amd import _lib
from vibevoice_amd.engine import Engine
from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference
from vibevoice_amd.weights import W8_CODES, check_lm_attn_w8

ROOT = Path(__file__).resolve().parent.parent
FP8 = "fp8_e4m3"


def test_symbols_are_exported_bound_and_declared():
    L = _lib.lib()   # raises if the library does not load
    names = {n: a for n, _, a in _lib.EXPORTS}
    assert len(names["vv_set_lm_attn_w8"]) == 2 and len(names["vv_lm_attn_w8"]) == 1
    assert len(L.vv_set_lm_attn_w8.argtypes) == 2 and len(L.vv_lm_attn_w8.argtypes) == 1
    product = (ROOT / "include" / "vibevoice_hip.h").read_text()
    diag = (ROOT / "include" / "vibevoice_hip_diag.h").read_text()
    assert re.search(r"^int vv_set_lm_attn_w8\(vv_ctx\* ctx, int on\);", product, re.M)
    assert re.search(r"^int vv_lm_attn_w8\(vv_ctx\* ctx\);", product, re.M)
    assert "vv_set_lm_attn_w8(" not in diag
    assert product.index("int vv_set_kv_dtype(") < product.index("int vv_set_lm_attn_w8(")
    assert "off unless vv_set_lm_attn_w8" in " ".join(product.replace("*", " ").split())


def test_setter_rejects_other_values_by_name():
    L = _lib.lib()
    for bad in (2, -1, 256):
        assert L.vv_set_lm_attn_w8(None, bad) != 0, bad
        err = L.vv_last_error()
        assert b"vv_set_lm_attn_w8" in err and str(bad).encode() in err, err
    for ok in (0, 1):                                   # an accepted value, no context: named too
        assert L.vv_set_lm_attn_w8(None, ok) != 0
        assert b"vv_set_lm_attn_w8" in L.vv_last_error()
    assert L.vv_lm_attn_w8(None) == 0


def test_check_lm_attn_w8():
    assert check_lm_attn_w8(False) is False and check_lm_attn_w8(False, None, FP8, 2) is False
    assert check_lm_attn_w8(True, FP8) is True
    with pytest.raises(ValueError, match="FP8 weights"):
        check_lm_attn_w8(True, None)
    with pytest.raises(ValueError, match="kv_dtype"):
        check_lm_attn_w8(True, FP8, FP8)
    with pytest.raises(ValueError, match="tensor parallel"):
        check_lm_attn_w8(True, FP8, None, tp_size=2)
    with pytest.raises(ValueError, match="True or False"):
        check_lm_attn_w8("yes", FP8)


def test_engine_refuses_the_option_before_touching_a_device():
    """Every case raises in Engine's argument validation: no weights are packed and no
    context is created (state_dict None, device 'cpu')."""
    cfg = tiny_config()
    with pytest.raises(ValueError, match="FP8 weights"):
        Engine(cfg, None, "cpu", lm_attn_w8=True)
    with pytest.raises(ValueError, match="kv_dtype"):
        Engine(cfg, None, "cpu", weight_dtype=FP8, kv_dtype=FP8, lm_attn_w8=True)
    with pytest.raises(ValueError, match="lm_attn_w8=True is not supported with tensor parallel"):
        Engine(cfg, None, "cpu", packed={"lm.0.qkv_w" + W8_CODES: None}, tp_size=2, lm_attn_w8=True)
    # packed=: "FP8 weights" is the format those weights were packed in, whatever weight_dtype says
    with pytest.raises(ValueError, match="FP8 weights"):
        Engine(cfg, None, "cpu", packed={"lm.0.qkv_w": None}, weight_dtype=FP8, lm_attn_w8=True)
    with pytest.raises(ValueError, match="kv_dtype"):
        Engine(cfg, None, "cpu", packed={"lm.0.qkv_w" + W8_CODES: None}, kv_dtype=FP8, lm_attn_w8=True)
    # accepted arguments get past the validation: the next refusal is the device's
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        Engine(cfg, None, "cpu", packed={"lm.0.qkv_w" + W8_CODES: None}, lm_attn_w8=True)


def test_model_class_refuses_the_option_the_same_way():
    cfg = tiny_config()
    M = VibeVoiceForConditionalGenerationInference
    with pytest.raises(ValueError, match="FP8 weights"):
        M(cfg, None, "cpu", lm_attn_w8=True)
    with pytest.raises(ValueError, match="kv_dtype"):
        M(cfg, None, "cpu", weight_dtype=FP8, kv_dtype=FP8, lm_attn_w8=True)
    with pytest.raises(ValueError, match="FP8 weights"):
        M.from_pretrained("synthetic:1.5B", lm_attn_w8=True)
