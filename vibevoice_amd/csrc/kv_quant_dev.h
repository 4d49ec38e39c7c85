// The e4m3 row quantiser of the FP8 KV cache (format: kv_fp8.hip's header;
// vibevoice_amd/weights.py quantize_rows_e4m3), one copy for every kernel that
// appends to the cache or writes its rows: k_kv_quant, k_kv_rows (kv_fp8.hip)
// and k_lm_attn's FP8-KV forms (lm_attn.hip).  A pure function of the row.
#pragma once
#include "common.h"

constexpr int KVQ_E_MIN = -100;   // weights.py _E_MIN

// the row exponent of amax (>= 0, finite): amax = m * 2^x, m in [0.5, 1), and
// 448 * 2^e = 0.875 * 2^(e + 9), so e = x - 9 when m <= 0.875, else x - 8
DEV int row_exp(float amax) {
  if (amax == 0.f) return 0;
  int x;
  const float m = __builtin_frexpf(amax, &x);
  const int e = m <= 0.875f ? x - 9 : x - 8;
  return min(max(e, KVQ_E_MIN), 127);
}

// round-to-nearest-even e4m3 code of y, |y| <= 448.  Below the smallest normal
// (2^-6) the codes 0 .. 8 count steps of 2^-9 (8 is the smallest normal itself);
// above, the fp32 mantissa is rounded to 3 bits (a carry moves into the exponent).
DEV unsigned enc_e4m3(float y) {
  const unsigned s = (__float_as_uint(y) >> 24) & 0x80u;
  const float a = fabsf(y);
  unsigned c;
  if (a < 0.015625f) {
    c = (unsigned)__builtin_rintf(a * 512.f);
  } else {
    unsigned u = __float_as_uint(a);
    u += 0x7FFFFu + ((u >> 20) & 1u);
    c = (u >> 20) - (120u << 3);
  }
  return s | c;
}

// one wave, one row: the lane's two values (dims 2 lane, 2 lane + 1) -> their codes and the row exponent
DEV int quant_row(float x0, float x1, unsigned& c0, unsigned& c1) {
  const int e = row_exp(wave_max(fmaxf(fabsf(x0), fabsf(x1))));
  c0 = enc_e4m3(ldexpf(x0, -e));
  c1 = enc_e4m3(ldexpf(x1, -e));
  return e;
}

// one e4m3 code -> fp32 (exact)
DEV float dec_e4m3(unsigned c) { return __builtin_amdgcn_cvt_f32_fp8((int)c, 0); }
