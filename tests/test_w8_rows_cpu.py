"""Where an FP8 weight-only operand goes above 16 rows (host only, no device
work): vv_gemm_plan_w8 is vv_gemm_plan for a quantised GemmArgs plus one word,
0 = the FP8 GEMV (k_gemv_w8), 1 = the chosen bf16 kernel's own W8
instantiation (reads the codes, no dequantise pass), 2 = dequantise into the
scratch first.  The bf16 decision itself must not move."""
import ctypes

import pytest

from vibevoice_amd import _lib

CUS = 256
NONE, NORM = 0, 1
SHAPES = [(48, 192), (4608, 1536), (8192, 2048), (1024, 4096)]
GEMV, GEMVW, GEMM64, GEMM32, BIG2, XL = 1, 2, 4, 5, 7, 8


def plan_w8(M, N, K, xf=NONE, w=False, mod=False, epi=0, keep=0, cus=CUS):
    out = (ctypes.c_int * 12)()
    assert _lib.lib().vv_gemm_plan_w8(M, N, K, xf, int(w), int(mod), epi, keep, cus, out, 12) == 0
    return list(out)


def plan(M, N, K, xf=NONE, w=False, mod=False, epi=0, keep=0, cus=CUS):
    out = (ctypes.c_int * 11)()
    assert _lib.lib().vv_gemm_plan(M, N, K, xf, int(w), int(mod), epi, keep, cus, out, 11) == 0
    return list(out)


@pytest.mark.parametrize("xf", [NONE, NORM])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [17, 40, 64])
def test_gemv_rows_are_native(M, N, K, xf):
    p = plan_w8(M, N, K, xf)
    assert p[11] == 1, p
    assert p[:11] == plan(M, N, K, xf)
    assert p[0] in (GEMV, GEMVW) and p[1] == (M + 15) // 16


# (above 64 rows no kernel, bf16 or FP8, serves N % 32 != 0: N = 96 stands in for N = 48 there)
@pytest.mark.parametrize("N,K", [(96, 192)] + SHAPES[1:])
@pytest.mark.parametrize("M,xf", [(65, NONE), (65, NORM), (200, NONE), (200, NORM), (300, NORM)])
def test_tiled_rows_are_native(M, N, K, xf):
    p = plan_w8(M, N, K, xf)
    assert p[11] == 1, p
    assert p[:11] == plan(M, N, K, xf)
    assert p[0] in (GEMM64, GEMM32)


def test_rejected_shape_stays_rejected():
    assert plan(65, 48, 192)[0] == 9 and plan_w8(65, 48, 192)[:11] == plan(65, 48, 192)


@pytest.mark.parametrize("xf", [NONE, NORM])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("M", [1, 8, 16])
def test_decode_rows_keep_the_fp8_gemv(M, N, K, xf):
    p = plan_w8(M, N, K, xf)
    assert p[11] == 0, p
    assert p[:11] == plan(M, N, K, xf)


def test_what_still_dequantises():
    p = plan_w8(512, 4608, 1536)                       # k_gemm_big: one dequantise over 512 rows
    assert p[11] == 2 and p[0] == BIG2 and p[:11] == plan(512, 4608, 1536)
    p = plan_w8(4096, 4608, 1536)                      # k_gemm_xl
    assert p[11] == 2 and p[0] == XL
    for M in (2, 40, 200):                             # K = 96: a row is not whole chunk pairs
        p = plan_w8(M, 48, 96)
        assert p[11] == 2 and p[:11] == plan(M, 48, 96), (M, p)
    p = plan_w8(16, 4608, 1536, xf=2)                  # SiLU-add rows at M <= 16: k_gemv1, not k_gemv_w8's form
    assert p[11] == 2 and p[:11] == plan(16, 4608, 1536, xf=2)
    assert plan_w8(40, 4608, 1536, xf=2)[11] == 1      # ... above 16 rows k_gemv is built for it


def test_switch_forces_the_fallback_at_every_row_count():
    L = _lib.lib()
    L.vv_gemv_w8(0)
    try:
        for M in (1, 16, 17, 40, 64, 65, 200):
            for N, K in SHAPES:
                p = plan_w8(M, N, K)
                assert p[11] == 2 and p[:11] == plan(M, N, K), (M, N, K, p)
    finally:
        L.vv_gemv_w8(1)
    assert plan_w8(40, 48, 192)[11] == 1


def test_capacity_and_counter_are_host_only():
    L = _lib.lib()
    assert L.vv_gemm_plan_w8(40, 48, 192, 0, 0, 0, 0, 0, CUS, (ctypes.c_int * 11)(), 11) != 0   # out[] too short
    assert L.vv_gemm_plan_w8(40, 48, 100, 0, 0, 0, 0, 0, CUS, (ctypes.c_int * 12)(), 12) != 0   # K % 32
    n = L.vv_w8_dequant_launches()
    plan_w8(40, 48, 96)
    assert L.vv_w8_dequant_launches() == n >= 0
