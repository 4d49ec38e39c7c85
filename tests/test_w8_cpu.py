"""FP8 (OCP e4m3fn) weight-only storage, host side: the row quantiser, the
packed byte layout of the FP8 GEMV, pack(weight_dtype="fp8_e4m3") against
pack() of the fake-quantised state dict, option validation, and Engine's
`persistent` normalisation (no GPU compute here)."""
import pytest
import torch

from tiny import tiny_config
from vibevoice_amd.engine import normalize_persistent
from vibevoice_amd.weights import (LM_QUANTIZED, W8_CODES, W8_EXPS, check_weight_dtype, dequantize_rows,
                                   fake_quantize_state_dict, mfma_pack8, mfma_unpack, mfma_unpack8, pack,
                                   quantize_rows_e4m3, synthetic_state_dict)


def _weights():
    """[48, 192] bf16 rows scaled by 2^-12 .. 2^6, row 5 all zero, row 7 a single +-max element."""
    g = torch.Generator().manual_seed(0)
    w = torch.randn(48, 192, generator=g)
    ex = torch.arange(48) % 19 - 12                      # -12 .. 6
    w = torch.ldexp(w, ex[:, None]).bfloat16()
    w[5] = 0
    w[7] = 0
    w[7, 100] = -3.0
    return w


def test_quantize_rows_e4m3():
    w = _weights()
    codes, e = quantize_rows_e4m3(w)
    assert codes.dtype == torch.float8_e4m3fn and codes.shape == w.shape
    assert e.dtype == torch.int8 and e.shape == (48,)
    cf = codes.float()
    assert torch.isfinite(cf).all() and cf.abs().max() <= 448
    assert ((codes.view(torch.uint8) & 0x7f) != 0x7f).all()          # no NaN code (0x7f / 0xff)
    dq = dequantize_rows(codes, e)
    assert dq.dtype == torch.bfloat16
    exact = torch.ldexp(cf.double(), e.to(torch.int32)[:, None].double())
    assert torch.equal(dq.double(), exact)                            # bf16 holds code * 2^e exactly
    assert torch.equal(dq.float().bfloat16(), dq)
    wf = w.float()
    nz = wf.abs().amax(1) > 0
    rel = (dq.float() - wf).norm(dim=1)[nz] / wf.norm(dim=1)[nz]
    assert rel.max() <= 2.0 ** -4, rel.max()
    top = cf.abs().amax(1)
    assert ((top[nz] > 224) & (top[nz] <= 448)).all(), top
    assert e[5] == 0 and (cf[5] == 0).all()
    assert torch.equal(dq[7], w[7])                                   # one element: exactly representable


@pytest.mark.parametrize("K", [64, 192, 3584])
@pytest.mark.parametrize("N", [16, 48])
def test_mfma_pack8_round_trip(N, K):
    g = torch.Generator().manual_seed(N + K)
    c = torch.randint(0, 256, (N, K), generator=g, dtype=torch.uint8)
    p = mfma_pack8(c)
    assert p.shape == c.shape and torch.equal(mfma_unpack8(p), c)
    f = c.view(torch.float8_e4m3fn)
    assert torch.equal(mfma_unpack8(mfma_pack8(f)).view(torch.uint8), c)
    # the documented layout: block (t, p) is 1 KB, lane l holds 8 + 8 columns of row 16t + (l & 15)
    t, pr, l = N // 16 - 1, K // 64 - 1, 37
    off = (t * (K // 64) + pr) * 1024 + l * 16
    row = c[16 * t + (l & 15)]
    want = torch.cat([row[64 * pr + 8 * (l >> 4):][:8], row[64 * pr + 32 + 8 * (l >> 4):][:8]])
    assert torch.equal(p.reshape(-1)[off:off + 16], want)


def test_pack_fp8_equals_pack_of_fake_quantized():
    cfg = tiny_config()
    sd = synthetic_state_dict(cfg, seed=3, device="cpu", mode="test", with_acoustic_encoder=False)
    q = pack(sd, cfg, "cpu", weight_dtype="fp8_e4m3")
    f = pack(fake_quantize_state_dict(sd, cfg), cfg, "cpu")
    plain = pack(sd, cfg, "cpu")
    for l in range(cfg.decoder_config.num_hidden_layers):
        for n in LM_QUANTIZED:
            k = f"lm.{l}.{n}"
            assert k not in q                                          # no bf16 copy of a quantised matrix
            codes, ex = q[k + W8_CODES], q[k + W8_EXPS]
            assert codes.dtype == torch.float8_e4m3fn and ex.dtype == torch.int8
            assert codes.shape == plain[k].shape and ex.shape == (plain[k].shape[0],)
            assert torch.equal(dequantize_rows(mfma_unpack8(codes), ex), mfma_unpack(f[k])), k
    lmq = {f"lm.{l}.{n}" for l in range(cfg.decoder_config.num_hidden_layers) for n in LM_QUANTIZED}
    for k, v in q.items():
        if v.dtype == torch.bfloat16:
            assert k not in lmq and torch.equal(v, plain[k]), k       # everything else untouched
    assert set(plain) - set(q) == lmq
    # unset: today's pack, bit for bit
    again = pack(sd, cfg, "cpu", weight_dtype=None)
    assert set(again) == set(plain) and all(torch.equal(again[k], plain[k]) for k in plain)


def test_weight_dtype_validation():
    cfg = tiny_config(hidden=256, heads=2, kv_heads=2, inter=512)
    sd = synthetic_state_dict(cfg, seed=3, device="meta", mode="test", with_acoustic_encoder=False)
    with pytest.raises(ValueError, match="fp8_e4m3"):
        pack(sd, cfg, "cpu", weight_dtype="int4")
    with pytest.raises(ValueError, match="tensor parallel"):
        pack(sd, cfg, "cpu", tp_rank=0, tp_size=2, weight_dtype="fp8_e4m3")
    with pytest.raises(ValueError):
        check_weight_dtype("fp8")
    assert check_weight_dtype(None) is None and check_weight_dtype("fp8_e4m3") == "fp8_e4m3"


def test_persistent_normalisation():
    assert normalize_persistent(True) is True and normalize_persistent(1) is True
    assert normalize_persistent(False) is False and normalize_persistent(0) is False
    assert normalize_persistent("follow") == "follow"
    for bad in ("on", "Follow", 2, None, 1.0, "1"):
        with pytest.raises(ValueError):
            normalize_persistent(bad)
