"""FP8 (OCP e4m3) KV-cache storage, host side: fake_quantize_kv (the CPU statement
of the format csrc/kv_fp8.hip stores), option validation, the header's new
exports, and kv8_ref pinned to the oracle (no GPU compute here)."""
import os
import re

import pytest
import torch

import kv8_ref
from oracle import lm as olm
from tiny import tiny_config
from vibevoice_amd.weights import (check_kv_dtype, dequantize_rows, fake_quantize_kv, quantize_rows_e4m3,
                                   synthetic_state_dict)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows():
    """[3, 40, 128] bf16 rows scaled by 2^-12 .. 2^6; one all-zero row, one single-element row."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 40, 128, generator=g)
    ex = (torch.arange(120) % 19 - 12).reshape(3, 40, 1)
    x = torch.ldexp(x, ex).bfloat16()
    x[1, 5] = 0
    x[2, 7] = 0
    x[2, 7, 100] = -3.0
    return x


def test_fake_quantize_kv_format():
    x = _rows()
    y = fake_quantize_kv(x)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape
    assert torch.equal(fake_quantize_kv(y), y)                                   # idempotent
    assert (y[1, 5] == 0).all() and torch.equal(y[2, 7], x[2, 7])               # zero row; one element: exact
    xf, yf = x.float().reshape(-1, 128), y.float().reshape(-1, 128)
    nz = xf.abs().amax(1) > 0
    rel = (yf - xf).norm(dim=1)[nz] / xf.norm(dim=1)[nz]
    assert rel.max() <= 2.0 ** -4, rel.max()                                     # half an e4m3 ulp
    # it is the weights' row quantiser, row by row
    codes, e = quantize_rows_e4m3(x.reshape(-1, 128))
    assert torch.equal(dequantize_rows(codes, e).reshape(x.shape), y)
    assert ((codes.view(torch.uint8) & 0x7f) != 0x7f).all()                      # no NaN code
    with pytest.raises(AssertionError):
        fake_quantize_kv(x.float())


def test_fake_quantize_kv_round_trips_every_code():
    """Every finite e4m3 value times 2^e, in rows whose amax code is the top binade
    (so the row's exponent is e), comes back unchanged."""
    c = torch.arange(256, dtype=torch.uint8)
    c = c[(c & 0x7f) != 0x7f]
    vals = c.view(torch.float8_e4m3fn).float()                                   # 254 values
    for e in (-20, -3, 0, 5, 40):
        rows = torch.zeros(2, 128)
        rows[0, :127] = vals[:127]
        rows[1, :127] = vals[127:]
        rows[:, 127] = 448.0                                                     # pins the row exponent to e
        x = torch.ldexp(rows, torch.tensor(e)).bfloat16()
        assert torch.equal(x.float(), torch.ldexp(rows, torch.tensor(e)))        # exact in bf16
        assert torch.equal(fake_quantize_kv(x), x), e


def test_check_kv_dtype():
    assert check_kv_dtype(None) is None and check_kv_dtype("fp8_e4m3") == "fp8_e4m3"
    for bad in ("fp8", "int8", "bf16", 1, "FP8_E4M3"):
        with pytest.raises(ValueError, match="fp8_e4m3"):
            check_kv_dtype(bad)
    with pytest.raises(ValueError, match="tensor parallel"):
        check_kv_dtype("fp8_e4m3", tp_size=2)
    assert check_kv_dtype(None, tp_size=2) is None


def test_headers_declare_kv_exports():
    product = open(os.path.join(ROOT, "include", "vibevoice_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "vibevoice_hip_diag.h")).read()
    assert re.search(r"^int vv_set_kv_dtype\(vv_ctx\* ctx, int dtype\);", product, re.M)
    assert re.search(r"^int vv_kv_dtype\(vv_ctx\* ctx\);", product, re.M)
    assert re.search(r"^int vv_kv_bytes\(vv_ctx\* ctx, long long\* bytes\);", product, re.M)
    for n in ("vv_diag_kv_read", "vv_diag_kv_write", "vv_diag_attn_ctx"):
        assert re.search(rf"^int {n}\(", diag, re.M) and n + "(" not in product, n
    from vibevoice_amd import _lib
    names = {n for n, _, _ in _lib.EXPORTS}
    assert {"vv_set_kv_dtype", "vv_kv_dtype", "vv_kv_bytes", "vv_diag_kv_read", "vv_diag_kv_write",
            "vv_diag_attn_ctx"} <= names
    L = _lib.lib()
    for n in names:
        assert hasattr(L, n), n


@pytest.mark.parametrize("heads,kv_heads", [(6, 1), (7, 1)])
def test_kv8_ref_identity_is_the_oracle(heads, kv_heads):
    cfg = tiny_config(hidden=128 * heads, layers=2, heads=heads, kv_heads=kv_heads, inter=256)
    sd = synthetic_state_dict(cfg, seed=5, device="cpu", mode="test", with_acoustic_encoder=False)
    pre = "model.language_model."
    osd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
    lcfg = dict(cfg.decoder_config)
    g = torch.Generator().manual_seed(1)
    H = cfg.decoder_config.hidden_size
    ka, kb = [olm.RowKV(2) for _ in range(2)], [olm.RowKV(2) for _ in range(2)]
    for T in (5, 1, 1):
        x = torch.randn(2, T, H, generator=g).bfloat16()
        a = olm.forward_rows(osd, lcfg, x, ka)
        b = kv8_ref.forward_rows(osd, lcfg, x, kb)
        assert torch.equal(a, b)
        for r in range(2):
            for li in range(2):
                assert torch.equal(ka[r].k[li], kb[r].k[li]) and torch.equal(ka[r].v[li], kb[r].v[li])
    # the hook changes the result (the test would pass vacuously if it were never called)
    c = kv8_ref.forward_rows(osd, lcfg, x, [olm.RowKV(2) for _ in range(2)], kv_hook=fake_quantize_kv)
    assert not torch.equal(c, olm.forward_rows(osd, lcfg, x, [olm.RowKV(2) for _ in range(2)]))
