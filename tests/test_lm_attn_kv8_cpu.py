"""The per-context option that runs the one-launch LM attention kernel on an FP8
KV cache (host only, no device work): vv_set_lm_attn_kv8 / vv_lm_attn_kv8 are
exported, bound by _lib.py and declared in the product header after
vv_set_lm_attn_w8, which states that the option is off unless set; the
diagnostic vv_lm_attn_kvround is declared in the diagnostic header only; the C
setter names itself in its null-context and bad-value errors; check_lm_attn_kv8
and the new keyword of check_lm_attn_w8; and Engine / the model class raise the
option's errors before their device error."""
import re
from pathlib import Path

import pytest

from tiny import tiny_config
from vibevoice_amd import _lib
from vibevoice_amd.engine import Engine
from vibevoice_amd.modeling_vibevoice_inference import VibeVoiceForConditionalGenerationInference
from vibevoice_amd.weights import W8_CODES, check_lm_attn_kv8, check_lm_attn_w8

ROOT = Path(__file__).resolve().parent.parent
FP8 = "fp8_e4m3"


def test_symbols_are_exported_bound_and_declared():
    L = _lib.lib()   # raises if the library does not load
    names = {n: a for n, _, a in _lib.EXPORTS}
    assert len(names["vv_set_lm_attn_kv8"]) == 2 and len(names["vv_lm_attn_kv8"]) == 1
    assert len(L.vv_set_lm_attn_kv8.argtypes) == 2 and len(L.vv_lm_attn_kv8.argtypes) == 1
    assert len(names["vv_lm_attn_kvround"]) == 1 and len(L.vv_lm_attn_kvround.argtypes) == 1
    product = (ROOT / "include" / "vibevoice_hip.h").read_text()
    diag = (ROOT / "include" / "vibevoice_hip_diag.h").read_text()
    assert re.search(r"^int vv_set_lm_attn_kv8\(vv_ctx\* ctx, int on\);", product, re.M)
    assert re.search(r"^int vv_lm_attn_kv8\(vv_ctx\* ctx\);", product, re.M)
    assert "vv_set_lm_attn_kv8(" not in diag and "vv_lm_attn_kv8(" not in diag
    assert product.index("int vv_set_lm_attn_w8(") < product.index("int vv_set_lm_attn_kv8(")
    # the comment above the declaration says that the option is off unless set
    flat = " ".join(product.replace("*", " ").split())
    comment = flat[flat.index("int vv_lm_attn_w8(vv_ctx ctx);"):flat.index("int vv_set_lm_attn_kv8(")]
    assert "off unless set" in comment and "the default" in comment
    assert "unless vv_set_lm_attn_kv8" in flat          # ... and vv_set_kv_dtype's comment points at it
    assert re.search(r"^int vv_lm_attn_kvround\(int on\);", diag, re.M) and "vv_lm_attn_kvround" not in product


def test_setter_names_itself_in_its_errors():
    L = _lib.lib()
    for bad in (2, -1, 256):
        assert L.vv_set_lm_attn_kv8(None, bad) != 0, bad
        err = L.vv_last_error()
        assert b"vv_set_lm_attn_kv8" in err and b"unsupported value" in err and str(bad).encode() in err, err
    for ok in (0, 1):
        assert L.vv_set_lm_attn_kv8(None, ok) != 0
        assert b"vv_set_lm_attn_kv8: null context" in L.vv_last_error()
    assert L.vv_lm_attn_kv8(None) == 0


def test_check_lm_attn_kv8():
    assert check_lm_attn_kv8(False) is False and check_lm_attn_kv8(False, None, 2) is False
    assert check_lm_attn_kv8(False, FP8) is False and check_lm_attn_kv8(True, FP8) is True
    assert check_lm_attn_kv8(True, FP8, 1) is True
    with pytest.raises(ValueError, match="kv_dtype"):
        check_lm_attn_kv8(True)
    with pytest.raises(ValueError, match="kv_dtype"):
        check_lm_attn_kv8(True, None, 2)
    with pytest.raises(ValueError, match="tensor parallel"):
        check_lm_attn_kv8(True, FP8, 2)
    for bad in ("yes", 1, 0, None):
        with pytest.raises(ValueError, match="True or False"):
            check_lm_attn_kv8(bad, FP8)


def test_check_lm_attn_w8_keyword():
    assert check_lm_attn_w8(True, FP8, FP8, lm_attn_kv8=True) is True
    assert check_lm_attn_w8(True, FP8, FP8, 1, lm_attn_kv8=True) is True
    with pytest.raises(ValueError, match="kv_dtype"):
        check_lm_attn_w8(True, FP8, FP8)
    with pytest.raises(ValueError, match="kv_dtype"):
        check_lm_attn_w8(True, FP8, FP8, lm_attn_kv8=False)
    with pytest.raises(ValueError, match="tensor parallel"):
        check_lm_attn_w8(True, FP8, FP8, 2, lm_attn_kv8=True)
    with pytest.raises(ValueError, match="FP8 weights"):
        check_lm_attn_w8(True, None, FP8, lm_attn_kv8=True)
    with pytest.raises(TypeError):
        check_lm_attn_w8(True, FP8, FP8, 1, True)          # keyword only


def test_engine_raises_the_option_errors_before_its_device_error():
    cfg = tiny_config()
    with pytest.raises(ValueError, match="lm_attn_kv8=True needs an FP8 KV cache"):
        Engine(cfg, None, "cpu", lm_attn_kv8=True)
    with pytest.raises(ValueError, match="True or False"):
        Engine(cfg, None, "cpu", kv_dtype=FP8, lm_attn_kv8="on")
    with pytest.raises(ValueError, match="tensor parallel"):
        Engine(cfg, None, "cpu", kv_dtype=FP8, tp_size=2, lm_attn_kv8=True)
    # FP8 weights + FP8 KV: lm_attn_w8 alone still raises on kv_dtype; with both options the device is next
    with pytest.raises(ValueError, match="kv_dtype"):
        Engine(cfg, None, "cpu", weight_dtype=FP8, kv_dtype=FP8, lm_attn_w8=True)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        Engine(cfg, None, "cpu", packed={"lm.0.qkv_w" + W8_CODES: None}, kv_dtype=FP8, lm_attn_w8=True,
               lm_attn_kv8=True)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        Engine(cfg, None, "cpu", packed={"lm.0.qkv_w": None}, kv_dtype=FP8, lm_attn_kv8=True)


def test_model_class_raises_the_same_way():
    cfg = tiny_config()
    M = VibeVoiceForConditionalGenerationInference
    with pytest.raises(ValueError, match="lm_attn_kv8=True needs an FP8 KV cache"):
        M(cfg, None, "cpu", lm_attn_kv8=True)
    with pytest.raises(ValueError, match="True or False"):
        M(cfg, None, "cpu", kv_dtype=FP8, lm_attn_kv8=1)
    with pytest.raises(ValueError, match="lm_attn_kv8=True needs an FP8 KV cache"):
        M.from_pretrained("synthetic:1.5B", lm_attn_kv8=True)
    with pytest.raises(ValueError, match="kv_dtype"):
        M.from_pretrained("synthetic:1.5B", weight_dtype=FP8, kv_dtype=FP8, lm_attn_w8=True)
