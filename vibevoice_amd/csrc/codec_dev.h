// The σ-VAE codec Block1D (modular_vibevoice_tokenizer.py:667-684, streaming conv
// :327-382) as every kernel form computes it, one frame of rows t per sample:
//   n_t = ConvRMSNorm(x_t)                        -> conv buffer (next steps' history)
//   y_t = x_t + bf16(bf16(dwconv_k7(n)_t + b) * gamma)
//   a_t = ConvRMSNorm_ffn(y_t)
//   out_t = y_t + bf16(ffn_gamma * bf16(fc2(GELU(fc1(a_t)))))
// Where an rb() sits below IS the parity contract with the reference (common.h):
// the cb_* helpers are the only place it is written.  They are pure functions of
// registers (no loads, stores or barriers); every form -- mix_rows (k_mix,
// k_block), XF_MIX (gemm.hip), k_codec_stage, k_codec_stage_s, k_codec_tile,
// k_codec_wide -- brings its own data movement, row-sum reduction and fc1 / fc2
// work split.  A chunk is 8 consecutive channels of one row (16 bytes); the taps
// of a chunk are summed k = 0 .. 6 in order, one fp32 accumulator per channel.
//
// The rounding chains (cb_norm, cb_y, cb_gelu, cb_ffn_res) are per element, and
// the callers keep the loop over a chunk's 8 (or a tile's 4) elements: hipcc
// optimises a force-inlined callee before it inlines it, so a chunk-wide helper
// with the loop inside converts and schedules the block's loop-invariant
// operands in another order than the same loop written in the kernel, and the
// kernels' registers and waits moved with it ("One copy of the
// Block1D arithmetic").  The chunk-wide helpers below are the ones that left
// every kernel's loads, waits, barriers and registers where they were.
#pragma once
#include "gemv_dev.h"

// ---------------------------------------------------------------- element arithmetic
// sum of squares of a chunk, ascending element order (a row's sum adds its chunks' sums)
DEV float cb_ss8(bf16x8 v) { return ss8(v); }
// ConvRMSNorm of an element, inv = rsqrt(mean square + eps): the mixer norm and the FFN norm
DEV bf16 cb_norm(bf16 v, float inv, bf16 w) { return tobf(rb(rb(bf(v) * inv) * bf(w))); }
// The depthwise weights are [C][7]: a chunk's 56 values in 7 registers wk, tap k
// of the chunk's channel q at flat index q * 7 + k.
DEV bf16 cb_tap(const bf16x8 (&wk)[7], int q, int k) {
  const int f = q * 7 + k;
  return wk[f >> 3][f & 7];
}
DEV bf16x8 cb_taps8(const bf16x8 (&wk)[7], int k) {   // tap k of the 8 channels
  bf16x8 o;
#pragma unroll
  for (int q = 0; q < 8; ++q) o[q] = cb_tap(wk, q, k);
  return o;
}
// one tap into the 8 sums: gathered taps w, conv input row v (cb_conv8's body; k_codec_stage
// parks tap 6 with cb_taps8 and adds it to the new row with the same multiply-add)
DEV void cb_mac8(float (&acc)[8], bf16x8 w, bf16x8 v) {
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] += bf(w[q]) * bf(v[q]);
}
DEV void cb_conv8(float (&acc)[8], const bf16x8 (&wk)[7], bf16x8 v, int k) { cb_mac8(acc, cb_taps8(wk, k), v); }
// gamma residual y of an element.  The caller sums y's squares for the FFN norm in the same
// loop (ss += bf(y) * bf(y)): cb_ss8(y8) after the loop gives the same sum but moved code
// (k_codec_wide<256> lost a wait, the tile kernels 4 .. 10 instructions), so it stays there.
DEV bf16 cb_y(bf16 x, float acc, bf16 bb, bf16 gv) { return tobf(bf(x) + rb(rb(acc + bf(bb)) * bf(gv))); }
// fc1's epilogue.  FAST: erf by gelu_fast (common.h: |error| <= 1.5e-7 before the
// bf16 rounding) in the one-launch tile / cluster stages, whose epilogues are
// VALU-bound over many rows; otherwise ocml's erff (k_block, the persistent
// stages, the GEMMs' EPI_GELU).  The two are not bit-identical; the choice per
// form is part of that form's parity record (tests/test_gpu_codec*.py).
template <bool FAST>
DEV bf16 cb_gelu(float acc, bf16 b1) {
  const float h = rb(acc + bf(b1));
  return tobf(FAST ? gelu_fast(h) : gelu_f(h));
}
template <bool FAST>
DEV bf16x4 cb_gelu4(f32x4 acc, bf16x4 b1) {
  bf16x4 o;
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = cb_gelu<FAST>(acc[q], b1[q]);
  return o;
}
// fc2's epilogue: the ffn_gamma residual
DEV bf16 cb_ffn_res(bf16 y, float acc, bf16 b2, bf16 g2) { return tobf(bf(y) + rb(bf(g2) * rb(acc + bf(b2)))); }
DEV bf16x4 cb_ffn_res4(bf16x4 y, f32x4 acc, bf16x4 b2, bf16x4 g2) {
  bf16x4 o;
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = cb_ffn_res(y[q], acc[q], b2[q], g2[q]);
  return o;
}


// ---------------------------------------------------------------- time-tile stages
// What k_codec_tile and k_codec_wide share: a workgroup of ctm::NTH threads over a
// time tile's rows in LDS, thread tid on chunk tid % N8 of row-in-pass tid / N8.
namespace ctm {
constexpr int NTH = 512, NW = 8;   // 8 waves
template <int C>
struct Geo {
  static constexpr int N8 = C / 8;               // 16-byte chunks per row
  static constexpr int RPP = NTH / N8;           // rows per elementwise pass
  static constexpr int F = 4 * C;                // hidden width
  static constexpr int XLD = C + 8;              // LDS row stride (+16 B against bank conflicts)
  static_assert(NTH % N8 == 0 && 64 % N8 == 0, "a row's chunks in one lane group");
};
}  // namespace ctm

// A block's per-channel operands for this thread's chunk and its history row: one
// set in registers, block j+1's overwrites block j's once its mixer is done.
template <int C>
struct TileMix {
  bf16x8 wn, bb, gv, wf, wk[7], hv;
};

// The record's loads and the two mixer phases are macros, not functions: hipcc
// optimises a callee before it inlines it, and as functions -- the record by
// reference or its members by value -- these cost both kernels 2 .. 4 VGPRs and
// moved their waits; as source text they compile to what each kernel
// held before.  c2 / rp are the kernel's own tid % N8 and tid / N8: recomputed
// here they changed the code too.  G: the kernel's Geo; m: a TileMix<C> lvalue;
// blk: the Block1D; rows t live at xs + (t - L0) * XLD, conv input rows at ns 6
// rows further down.
#define CB_TILE_MIX_LOAD(G, C, m, blk, slot, tid, c2_)                                                     \
  do {                                                                                                     \
    (m).wn = *(const bf16x8*)((blk).norm + c2_ * 8);                                                       \
    (m).bb = *(const bf16x8*)((blk).dw_b + c2_ * 8);                                                       \
    (m).gv = *(const bf16x8*)((blk).gamma + c2_ * 8);                                                      \
    (m).wf = *(const bf16x8*)((blk).ffn_norm + c2_ * 8);                                                   \
    _Pragma("unroll") for (int k_ = 0; k_ < 7; ++k_)                                                       \
        (m).wk[k_] = *(const bf16x8*)((blk).dw_w + (size_t)c2_ * 56 + k_ * 8);                             \
    const int h_ = min((tid) / G::N8, 5); /* history row (threads >= 6 * N8 load a copy of row 5) */       \
    (m).hv = *(const bf16x8*)((blk).mix + (slot) * (blk).mix_sB + (long long)h_ * (C) + c2_ * 8);          \
  } while (0)
// M1: conv input rows [lo - 6, B) = norm(x) (history rows t < 0 from m.hv); `append`: this
// workgroup writes the frame's last 6 rows to the block's history buffer
#define CB_TILE_MIX_NORM(G, C, m, blk, slot, eps, xs, ns, L0, lo, B, T, append, tid, c2_, rp_)                 \
  do {                                                                                                     \
    const int cs_ = (lo) - 6;                                                                              \
    if ((tid) < 6 * G::N8) {                                                                               \
      const int t_ = (tid) / G::N8 - 6;                                                                    \
      if (t_ >= cs_) *(bf16x8*)((ns) + (t_ - (L0) + 6) * G::XLD + c2_ * 8) = (m).hv;                       \
    }                                                                                                      \
    for (int p_ = max(cs_, 0); p_ < (B); p_ += G::RPP) {                                                   \
      const int t_ = p_ + rp_, tc_ = min(t_, (B) - 1);                                                     \
      const bf16x8 v_ = *(const bf16x8*)((xs) + (tc_ - (L0)) * G::XLD + c2_ * 8);                          \
      const float ss_ = group_sum<G::N8>(cb_ss8(v_));                                                      \
      const float inv_ = rsqrtf(ss_ / (float)(C) + (eps));                                                 \
      bf16x8 o8_;                                                                                          \
      _Pragma("unroll") for (int q_ = 0; q_ < 8; ++q_) o8_[q_] = cb_norm(v_[q_], inv_, (m).wn[q_]);        \
      if (t_ < (B)) {                                                                                      \
        *(bf16x8*)((ns) + (t_ - (L0) + 6) * G::XLD + c2_ * 8) = o8_;                                       \
        if ((append) && t_ >= (T) - 6)                                                                     \
          *(bf16x8*)((blk).mix + (slot) * (blk).mix_sB + (long long)(6 + t_) * (C) + c2_ * 8) = o8_;       \
      }                                                                                                    \
    }                                                                                                      \
  } while (0)
// M2: rows [lo, B): depthwise conv + gamma residual -> y at yd (xs itself: in place, item (t, c2)
// is read and written by this thread alone; or rows of its own); FFN norm -> fc1's input rows as
#define CB_TILE_MIX_CONV(G, C, m, eps, xs, ns, yd, as, L0, lo, B, c2_, rp_)                                \
  do {                                                                                                     \
    for (int p_ = (lo); p_ < (B); p_ += G::RPP) {                                                          \
      const int t_ = p_ + rp_, tc_ = min(t_, (B) - 1);                                                     \
      float acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0};                                                            \
      _Pragma("unroll") for (int k_ = 0; k_ < 7; ++k_)                                                     \
          cb_conv8(acc_, (m).wk, *(const bf16x8*)((ns) + (tc_ - (L0) + k_) * G::XLD + c2_ * 8), k_);       \
      const bf16x8 xv_ = *(const bf16x8*)((xs) + (tc_ - (L0)) * G::XLD + c2_ * 8);                         \
      bf16x8 y8_;                                                                                          \
      float ss_ = 0.f;                                                                                     \
      _Pragma("unroll") for (int q_ = 0; q_ < 8; ++q_) {                                                   \
        y8_[q_] = cb_y(xv_[q_], acc_[q_], (m).bb[q_], (m).gv[q_]);                                         \
        ss_ += bf(y8_[q_]) * bf(y8_[q_]);                                                                  \
      }                                                                                                    \
      ss_ = group_sum<G::N8>(ss_);                                                                         \
      const float inv_ = rsqrtf(ss_ / (float)(C) + (eps));                                                 \
      bf16x8 o8_;                                                                                          \
      _Pragma("unroll") for (int q_ = 0; q_ < 8; ++q_) o8_[q_] = cb_norm(y8_[q_], inv_, (m).wf[q_]);       \
      if (t_ < (B)) {                                                                                      \
        *(bf16x8*)((yd) + (t_ - (L0)) * G::XLD + c2_ * 8) = y8_;                                           \
        *(bf16x8*)((as) + (t_ - (L0)) * G::XLD + c2_ * 8) = o8_;                                           \
      }                                                                                                    \
    }                                                                                                      \
  } while (0)
