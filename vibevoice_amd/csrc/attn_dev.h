// The parts k_attn (attention.hip), k_lm_attn (lm_attn.hip) and o_proj's XF_ATTN_MERGE (gemm.hip)
// share, each written once: a row's key-split plan, the K / V fragment loads of one 32-key step,
// the step itself, and the merge of a few (m, l, O) partials.  Force-inlined pieces for the
// callers' own schedules (k_attn's two register sets, la_long_units' two K sets, the short
// forms' loads -> KVQ patch -> step), not a schedule of their own.
//
// A step is 32 keys [c0, c0 + 32) of one (row, kv head) on one wave, keys past w1 masked:
//   S[16 heads x 16 keys] = Q . K^T, 2 tiles x 4 MFMAs (lane: r = lane & 15, g = lane >> 4; Q
//       row = head r, zero past the kv head's query heads; K column = key c0 + 16 tt + r)
//   online softmax on the fp32 scores in registers (a head's row over 16 lanes), scaled after
//       the MFMA
//   P rounded to bf16 (as the reference's eager path rounds it) through the wave's LDS tile
//   O[heads x 128] (+)= P . V, 8 MFMAs (V^T blocks, common.h v_off; l stays fp32)
//
// Rules every form keeps (each cost a debugging round once):
//   Clamped loads.  Fragment loads are unconditional, from positions clamped into [0, w1): no
//     branch and no per-load wait.  (Guarded V loads followed by the tail mask compiled to a
//     branch + s_waitcnt vmcnt(0) after EACH of a step's 8 V loads -- eight serialized memory
//     round trips per step.)
//   Tail masking.  Keys past w1 are masked where their values are used: S to -inf (so P = 0)
//     and V to 0 on the tail step (the clamped rows hold other keys' values, and 0 x NaN
//     would not vanish).
//   FP8 scale placement.  The e4m3 cache (kernels.h KV8) loads a fragment's 8 codes with one
//     8-byte load and converts them to bf16 in registers (exact, cvt8) for the same MFMAs; the
//     rows' power-of-two scales go on the 16 x 16 score tile, not on the operands: the fp32
//     score of key j times 2^eK[j] after Q.K^T, its fp32 probability times 2^eV[j] before the
//     rounding to bf16 for P.V, l from the unscaled probabilities.  A power of two commutes
//     with both roundings, so the result is bit for bit that of the bf16 form over a cache
//     holding the dequantised values.
#pragma once
#include <type_traits>

#include "common.h"

// ---------------------------------------------------------------- split plan
// A row of `len` keys under a launch planned as `nsplit` splits of >= `chunk` keys: the row's
// own split size (>= chunk, a multiple of 32, all nsplit splits cover len), its active splits
// nact = ceil(len / chunk) (splits past the row's last key do nothing), and the partials its
// consumer merges: ceil(nact / group) group partials, or the nact splits' when group = 0.
// k_attn, k_attn_merge, k_attn_finish and XF_ATTN_MERGE all evaluate this.
struct AttnSplits {
  int chunk, nact, nparts;
};
__host__ __device__ inline AttnSplits attn_row_splits(int len, int nsplit, int chunk, int group) {
  const int c = ((len + nsplit - 1) / nsplit + 31) / 32 * 32;
  AttnSplits s;
  s.chunk = chunk > c ? chunk : c;
  s.nact = (len + s.chunk - 1) / s.chunk;
  s.nparts = group ? (s.nact + group - 1) / group : s.nact;
  return s;
}

// ---------------------------------------------------------------- fragment loads
// ST = the cache's storage type: bf16, or unsigned char for e4m3 codes
template <class ST>
struct KvFrag {   // one lane's MFMA operand piece of 8 cached values, as loaded
  typedef bf16x8 type;
};
template <>
struct KvFrag<unsigned char> {
  typedef u32x2 type;
};
// A load policy LD gives ld(const bf16*) -> bf16x8 and ld(const unsigned char*) -> u32x2.
// Plain loads (k_attn); k_lm_attn's is non-temporal (lm_attn.hip LaLdNT).
struct AttnLdPlain {
  static DEV bf16x8 ld(const bf16* p) { return *(const bf16x8*)p; }
  static DEV u32x2 ld(const unsigned char* p) { return *(const u32x2*)p; }
};

// The K fragments of keys c0 + 16 tt + r (B operand of S: column = key) of a step that ends at
// w1; codes: also the row exponents ek / ev [ctx] of those keys into xk / xv (bf16: untouched)
template <class LD, class ST>
DEV void attn_load_k(const ST* K, const signed char* ek, const signed char* ev, int c0, int w1, int r, int g,
                     typename KvFrag<ST>::type (&kf)[2][4], int (&xk)[2], int (&xv)[2]) {
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int key = min(c0 + 16 * tt + r, w1 - 1);
#pragma unroll
    for (int c = 0; c < 4; ++c) kf[tt][c] = LD::ld(K + (long long)key * 128 + 32 * c + 8 * g);
    if constexpr (!std::is_same<ST, bf16>::value) {
      xk[tt] = ek[key];
      xv[tt] = ev[key];
    }
  }
}
// The V fragments (B operand of O: k = keys kb .. kb + 7, column = dim 16 j + r)
template <class LD, class ST>
DEV void attn_load_v(const ST* VB, int c0, int w1, int r, int g, typename KvFrag<ST>::type (&vf)[8]) {
  const int kb = min(c0 + 8 * g, (w1 - 1) & ~7);
#pragma unroll
  for (int j = 0; j < 8; ++j) vf[j] = LD::ld(VB + v_off(16 * j + r, kb));
}
// A step's fragments as loaded from the e4m3 cache -> bf16 (exact)
DEV void attn_frags_bf16(const u32x2 (&kq)[2][4], const u32x2 (&vq)[8], bf16x8 (&kf)[2][4], bf16x8 (&vf)[8]) {
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int c = 0; c < 4; ++c) kf[tt][c] = cvt8(kq[tt][c][0], kq[tt][c][1]);
#pragma unroll
  for (int j = 0; j < 8; ++j) vf[j] = cvt8(vq[j][0], vq[j][1]);
}

// ---------------------------------------------------------------- the step
// One 32-key step, keys [c0, w1): the tail masking of V (in place), S = Q.K^T, the scale and mask,
// the row max and sum, the P tile through this wave's LDS tile ptw [16][32], the P.V MFMA.  KV8: the
// keys' row exponents xk / xv.  CARRY: (m, l, O) carried from earlier steps (from (-inf, 0, 0)): m =
// max(m, step max), alpha = e^{m_old - m} on l and on O (the P.V MFMA's C operand).  Otherwise they
// are this step's alone: no carried max, no alpha, a zero C operand.  From (-inf, 0, 0) the first
// carried step's alpha is 0 and its results are the uncarried step's, bit for bit.
template <bool KV8, bool CARRY>
DEV void attn_step(float scale, const bf16x8 (&qf)[4], const bf16x8 (&kf)[2][4], bf16x8 (&vf)[8], const int (&xk)[2],
                   const int (&xv)[2], int c0, int w1, bf16* ptw, int r16, int g4, float (&mv)[4], float (&lv)[4],
                   f32x4 (&o)[8]) {
  if (c0 + 32 > w1) {   // the tail step (wave-uniform): keys kb + e >= w1 contribute nothing
    const int kb2 = c0 + 8 * g4;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) vf[j][e] = kb2 + e < w1 ? vf[j][e] : (bf16)0.f;
  }
  f32x4 sacc[2];   // lane: S[head 4 g + i][key c0 + 16 tt + r]
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    sacc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) sacc[tt] = mfma16(qf[c], kf[tt][c], sacc[tt]);
  }
  float pp[2][4], al[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {   // (the step holds a valid key, so its max is finite)
    if constexpr (KV8) {   // the key's 2^eK on the fp32 score
      sacc[0][i] = ldexpf(sacc[0][i], xk[0]);
      sacc[1][i] = ldexpf(sacc[1][i], xk[1]);
    }
    const float s0 = c0 + r16 < w1 ? sacc[0][i] * scale : -INFINITY;
    const float s1 = c0 + 16 + r16 < w1 ? sacc[1][i] * scale : -INFINITY;
    float mx = row16_max(fmaxf(s0, s1));
    if constexpr (CARRY) {
      mx = fmaxf(mv[i], mx);
      al[i] = __expf(mv[i] - mx);
    }
    pp[0][i] = __expf(s0 - mx);
    pp[1][i] = __expf(s1 - mx);
    const float ps = row16_sum(pp[0][i] + pp[1][i]);
    if constexpr (CARRY) lv[i] = lv[i] * al[i] + ps;
    else lv[i] = ps;
    mv[i] = mx;
  }
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (KV8)   // ... and the key's 2^eV on the fp32 probability before its rounding (l: unscaled)
        ptw[(4 * g4 + i) * 32 + 16 * tt + r16] = (bf16)ldexpf(pp[tt][i], xv[tt]);
      else
        ptw[(4 * g4 + i) * 32 + 16 * tt + r16] = (bf16)pp[tt][i];
    }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const bf16x8 pa = *(const bf16x8*)(ptw + r16 * 32 + 8 * g4);   // A operand: row = head r, k = keys 8 g .. 8 g + 7
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    f32x4 oc = (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (CARRY) {
#pragma unroll
      for (int i = 0; i < 4; ++i) oc[i] = o[j][i] * al[i];
    }
    o[j] = mfma16(pa, vf[j], oc);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the P tile read before the next step writes it
}

// ---------------------------------------------------------------- merge of <= NMAX partials
// M = max m_s, w_s = e^{m_s - M}, num = sum w_s o_s, den = sum w_s l_s over partials s = 0 .. n - 1
// in order (n <= NMAX), ND dims per thread.  load(s, m, l, o) fetches partial s's (m, l) and this
// thread's ND values of O: agent-scope relaxed atomics in k_attn (the partials were written through
// in this launch), plain loads after a kernel boundary.  All of a thread's loads are issued before
// the first is used: one memory round trip.  The multiply-adds are written fused, so the bits do
// not depend on where this is inlined (the in-kernel merge and XF_ATTN_MERGE must agree bit for bit).
template <int NMAX, int ND, class LOAD>
DEV void attn_merge_parts(int n, LOAD load, float& M, float (&num)[ND], float& den) {
  float mv[NMAX], lv[NMAX], ov[NMAX][ND];
#pragma unroll
  for (int s = 0; s < NMAX; ++s)
    if (s < n) load(s, mv[s], lv[s], ov[s]);
  M = -INFINITY;
#pragma unroll
  for (int s = 0; s < NMAX; ++s)
    if (s < n) M = fmaxf(M, mv[s]);
#pragma unroll
  for (int k = 0; k < ND; ++k) num[k] = 0.f;
  den = 0.f;
#pragma unroll
  for (int s = 0; s < NMAX; ++s) {
    if (s < n) {
      const float w = __expf(mv[s] - M);
#pragma unroll
      for (int k = 0; k < ND; ++k) num[k] = __builtin_fmaf(w, ov[s][k], num[k]);
      den = __builtin_fmaf(w, lv[s], den);
    }
  }
}
