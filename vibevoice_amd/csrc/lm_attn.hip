// The LM attention half at decode in ONE launch (k_lm_attn): input_layernorm ->
// q|k|v projection (+bias) -> RoPE -> KV append -> GQA attention over the
// compacted per-row cache -> o_proj -> residual, for R <= 16 query rows (17 .. 32: the
// second row class, MT below) of the 1.5B shapes (H 1,536, 12 q / 2 kv heads of 128).
// Reference: transformers Qwen2Attention (modeling_qwen2.py:99-134, 150-173,
// 195-247) as VibeVoiceModel.forward calls it per layer
// (vibevoice/modular/modeling_vibevoice.py:169-209) inside the generate loop
// (modeling_vibevoice_inference.py:483-486, 591-604).
//
// Per op this was three launches (k_gemv1 q|k|v with the RoPE / cache epilogue,
// k_attn with key splits, k_gemv1 o_proj merging the splits' partials): 7.5 +
// 6.5 + 7.4 us per layer at B = 1, ~11 MB of weights -- latency, not bytes.  Here
// 256 workgroups (one per CU) run four phases with three grid-wide waits:
//   1. workgroups 0..127 each own one 16-column q|k|v tile over all of K (48 KB
//      of weights in registers; the R A rows by LDS DMA, RMSNorm'd in place),
//      MFMA, the 8 waves' K slices summed in order, epi_rope's epilogue written
//      through (q rows; K rows and V columns into the cache).  Workgroups
//      128..223 meanwhile load their o_proj tile (48 KB) into registers, where it
//      stays until phase 4.
//   2. attention in units of (row, kv head, 32 keys), one wave each, dealt
//      round-robin over the 256 workgroups: S = Q.K^T and P.V on MFMA (attn_dev.h
//      attn_step, the kv head's 6 query heads padded to 16 rows), the unit's
//      (m, l, O) partial written through.
//   3. one wave per (row, query head) merges its units' partials in unit order
//      (attn_dev.h's merge formula, online) into the attention row, written through.
//   4. the o_proj workgroups DMA the attention rows, MFMA with the resident
//      weights, residual epilogue.
// Hand-offs: write-through (sc1) stores, each storing wave's vmcnt(0), a
// workgroup barrier, lane 0's arrival (persist_dev.h hl_grid_wait); readers
// use sc1 / nt loads (L1-bypassing; MI355X_MICROARCH.md's hand-off table, first
// row).  Arithmetic: epi_rope's and attn_dev.h's (scores scaled after the MFMA, P
// rounded to bf16 for P.V, l in fp32; the units merged by its split-merge formula).
//
// The kernel is one template, k_lm_attn<W8, KVQ, LONG, MT>, eleven instantiations (la_form below), its body
// four phases and three la_wait()s over force-inlined pieces, each written once:
//   la_load_tile / la_tile_mfma   a wave's six k-blocks of one 16-row weight tile: the loads (q|k|v, and
//                                 o_proj at entry or after wait 1) and the MFMAs + `red` store (phases 1, 4)
//   la_rope_append                phase 1's epilogue: the K slices summed, bias, RoPE, q rows / KV append
//   la_unit_begin / la_zero_pad_rows / la_store_partial
//                                 an attention unit: its (row, kv head), cache base and Q fragments; the
//                                 unit's partial.  Its 32-key K / V fragment loads and its 32-key step
//                                 are attn_dev.h's (attn_load_k / attn_load_v with LaLdNT, attn_step)
//   la_kvq_rows                   the KVQ forms' rows appended by this pass
//   la_merge                      phase 3
//
// W8 (GemmArgs::w8 / w8e of LmAttnArgs::qkv, LmAttnArgs::ow8 / owe): the two weight tiles are e4m3
// codes in mfma_pack8 order (gemv_w8.hip: 1 KB pair blocks of 16 rows x 64 columns = two k-blocks, a
// lane's 16 bytes = its two fragments) + one int8 exponent per packed row.  Same workgroup roles, same
// 6 k-blocks per wave (3 whole pairs), same MFMA order per accumulator, same LDS sums, epilogues,
// phases 2-3, waits and stamps; only la_load_tile and la_tile_mfma branch on it: a lane holds 3 u32x4
// per matrix instead of 6 bf16x8 and converts a fragment to code * 2^e[row] (cvt8s: the bf16 value
// k_dequant_w8 stores, exactly) where the bf16 form reads the register -- bit for bit the bf16 kernel
// on the dequantised matrices (tests/test_gpu_w8_lm_attn.py, tests/test_gpu_lm_attn_long.py).
//
// KVQ (the KV format; LmAttnArgs::kvq): 0 = the rows appended raw to a bf16 cache, as above.  1 = the
// FP8 (e4m3) cache of kv_fp8.hip (KV8: codes in the bf16 geometry + one int8 exponent per row; the
// per-engine option vv_set_lm_attn_kv8): phase 1 writes the K rows and V columns to the context's bf16
// staging cache (slot 0, position = the row index; cos / sin of the real position), as the GEMV
// epilogues do under FP8 KV.  Phase 2 never uses a cache entry this launch writes: la_kvq_rows takes
// them from the staged rows through the row quantiser (kv_quant_dev.h).  The K / V fragments load as
// codes (8 bytes where bf16 loads 16), convert with cvt8 (exact), and the scales go where attn_dev.h
// puts them (attn_step<KV8>): 2^eK[j] on the fp32 score of key j, 2^eV[j] on its fp32
// probability before the bf16 rounding, l from the unscaled probabilities.  No k_kv_stage_prep /
// k_kv_quant launch, no added wait.  2 = diagnostic (vv_lm_attn_kvround): KVQ = 1's data flow and
// quantiser on a bf16 cache -- the appended rows stored dequantised, the fragments read as bf16, the
// step KVQ = 0's -- the only other producer of the bits KVQ = 1 must produce
// (tests/test_gpu_lm_attn_kv8.py).
//
// LONG (bf16 KV only; a pass planned past LA_MAX_KEYS keys, which an engine allows with
// vv_set_lm_attn_max_keys): a unit covers 32 s keys, s = la_unit_steps(len) = ceil(len / 4,096) per
// row, computed in the kernel from the pass's position table, so a captured graph replays as rows
// grow across the s edges.  Its wave runs attn_step<., CARRY> s times, carrying (m, l, O): m = max(m,
// step max), alpha = e^{m_old - m} on l and on O (the P.V MFMA's C operand).  The short form's step is
// the same text with CARRY = false: no carried max, no alpha, a zero C operand.  From (-inf, 0, 0) the
// first carried step's alpha is 0 and its results are the uncarried step's, bit for bit, so a unit of
// one step (every row of <= 4,096 keys) writes the partial the short form writes.  One partial per
// unit, at most 128 units per (row, kv head): phases 1, 3 and 4, the waits, the stamps and the
// partials' workspace do not depend on LONG.
//
// MT (row tiles of 16 A rows; 2 = a pass of 17 .. 32 rows, which an engine allows with
// vv_set_lm_attn_max_rows; KVQ = 0 only): the row class.  MT = 1 is the kernel above.  At MT = 2 a q|k|v or
// o_proj workgroup still loads its one weight tile once (the same six k-blocks per wave, the same loads, the
// same vmcnt wait) and runs each fragment's MFMA over both row tiles, one accumulator per tile with the
// k-blocks in MT = 1's order, each tile into its own `red` area; the epilogues (la_rope_append, the residual
// store) run on one wave per row tile, waves 0 and 1, over their tile's 8 slices in MT = 1's order.  xs holds
// 32 rows, the unit prefix 2 x 32 + 1 entries, inv_s 32: 124 KB of LDS (la::Lds<2>) against 82, still one
// workgroup per CU.  Phases 2 and 3, the waits, the stamps and the partial layout are per (row, kv head,
// unit) and per (row, query head): the same text.  Every value of a row depends on that row's A row, the
// weights and its own KV entries only, so a row computes the bits it computes in a pass of <= 16 rows
// (tests/test_gpu_lm_attn_rows.py).  The KVQ forms are not built at MT = 2 (their tables and staged rows are
// the 16-row class's): an FP8-KV engine keeps its launches above 16 rows.
#include <type_traits>

#include "attn_dev.h"
#include "kv_quant_dev.h"
#include "persist_dev.h"

namespace la {
constexpr int H = 1536, NH = 12, NKV = 2, G = 6, D = 128, NQKV = (NH + 2 * NKV) * D;
constexpr int GRID = pk::G, NW = 8, NT = NW * 64, RMAX = 16;
constexpr int KC = H / 32, KPW = KC / NW;        // 48 k-blocks, 6 per wave
constexpr int PC = KC / 2, PPW = KPW / 2;        // W8: 24 pair blocks per tile, 3 per wave
constexpr int TQ = NQKV / 16, TO = H / 16;       // 128 q|k|v tiles, 96 o_proj tiles
constexpr int O0 = TQ;                           // o_proj workgroups [O0, O0 + TO)
constexpr int XST = H + 8;                       // padded LDS row (elements)
constexpr int MTMAX = 2;                         // row tiles of 16: the row classes 1..16 (MT = 1) and 17..32 (MT = 2)
// the LDS carve-up of a row class: MT tiles of 16 A rows
template <int MT>
struct Lds {
  static constexpr int ROWS = 16 * MT;
  static constexpr int XS = 0, XS_B = ROWS * XST * 2;
  static constexpr int RED = XS + XS_B, RED_B = MT * NW * 256 * 4;   // one [8 waves][256] area per row tile
  static constexpr int PT = RED + RED_B, PT_B = NW * 16 * 32 * 2;
  static constexpr int NWS = PT + PT_B, NWS_B = H * 2;              // input_layernorm weight
  static constexpr int INV_B = 4 * ROWS;                            // inverse RMS per row
  static constexpr int SM = NWS + NWS_B, SM_B = INV_B + 4 * (2 * ROWS + 1) + 12;
  // the KVQ forms' tables: the pass's slots [16], positions [16], and per row the first position this
  // pass appends to the row's slot [16]
  static constexpr int KT = SM + SM_B, KT_B = 3 * ROWS * 4;
  // MT = 1, 82 KB: one workgroup per CU (two would share a CU while another idles).  MT = 2: 124 KB as carved
  static constexpr int FLOOR = MT == 1 ? 82 * 1024 : 0;
  static constexpr int TOTAL = (KT + KT_B) > FLOOR ? (KT + KT_B) : FLOOR;
  static_assert(KT + KT_B <= 160 * 1024 && KT % 16 == 0 && 2 * TOTAL > 160 * 1024, "lm attn LDS");
};
constexpr int PART = G * D + 2 * G;              // floats per unit partial: O[6][128], then (m, l) x 6
static_assert(Lds<1>::TOTAL == 82 * 1024 && Lds<1>::ROWS == RMAX && Lds<1>::INV_B == 64, "lm attn LDS: the 16-row class");
static_assert(RMAX == LA_ROWS && 16 * MTMAX == LA_MAX_ROWS, "the row classes of kernels.h");
static_assert(NW * G * D * 4 <= Lds<1>::XS_B, "phase 2's partials pass through xs");
static_assert(GRID == pk::G, "grid waits: 256 arrivals per wait");
static_assert(KPW * NW == KC && KPW % 2 == 0 && PPW * 2 == KPW, "lm attn W8: a wave's k-blocks are whole pairs");
// a lane's registers of one weight tile: one 16-byte load each (W8: the 16 code bytes of a pair block)
template <bool W8>
using WF = std::conditional_t<W8, u32x4, bf16x8>;
template <bool W8>
constexpr int NWL = W8 ? PPW : KPW;   // weight loads per wave and matrix: one per register
static_assert(NWL<true> * 64 == KPW * 32 && NWL<false> * 32 == KPW * 32 && NWL<false> <= 63,
              "one 16-byte load per weight register, together the wave's 6 k-blocks; the count fits vmcnt");
}  // namespace la

DEV void la_stamp(const LmAttnArgs& a, int k) { hl_stamp(a.stamps, blockIdx.x, k, 0); }

// Grid wait n (1 .. 3), stamps 2 n and 2 n + 1 around it: the workgroup's stores are drained by their
// waves (vmcnt(0), at the callers), a barrier, lane 0's arrival and wait, a barrier.  False: the wait gave up.
DEV bool la_wait(const LmAttnArgs& a, unsigned g0, int n, unsigned* ok_s, int w) {
  la_stamp(a, 2 * n);
  __syncthreads();
  if (threadIdx.x == 0) ok_s[0] = hl_grid_wait(a.sync, pk::GEN_LM_ATTN, g0, n, w, a.err) ? 1u : 0u;
  __syncthreads();
  la_stamp(a, 2 * n + 1);
  return ok_s[0] != 0;
}

// This wave's 6 k-blocks of 16-row tile `tile` of a packed matrix (W8: pairs [3 wave, + 3) of its codes):
// NWL 16-byte non-temporal loads, lane `ln`
template <bool W8>
DEV void la_load_tile(la::WF<W8> (&wf)[la::NWL<W8>], const bf16* w_bf16, const unsigned char* w_codes, int tile,
                      int wave, int ln) {
  using namespace la;
  if constexpr (W8) {
    const unsigned char* wp = hl_opaque(w_codes) + ((long long)tile * PC + wave * PPW) * 1024 + ln * 16;
#pragma unroll
    for (int pp = 0; pp < PPW; ++pp) wf[pp] = hl_ldnt8(wp + (long long)pp * 1024);
  } else {
    const bf16* wp = hl_opaque(w_bf16) + ((long long)tile * KC + wave * KPW) * 512 + ln * 8;
#pragma unroll
    for (int kk = 0; kk < KPW; ++kk) wf[kk] = hl_ldnt(wp + (long long)kk * 512);
  }
}

// D[n][m] over this wave's k-blocks into red[wave]: A = the weight tile (row n = lane & 15; W8: code *
// sc, sc = 2^e of that row), B = the LDS rows xs (column m).  MT row tiles: the one weight fragment runs
// over rows 16 t + m of every tile t, each tile its own accumulator (k-blocks in the same order) and its
// own `red` area [t][wave][256]
template <bool W8, int MT>
DEV void la_tile_mfma(const la::WF<W8> (&wf)[la::NWL<W8>], float sc, const bf16* xs, float* red, int wave, int lane) {
  using namespace la;
  const int r16 = lane & 15, g4 = lane >> 4;
  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < KPW; ++kk) {
    const int kc = wave * KPW + kk;   // W8: k-block kc = half kk & 1 of pair kc >> 1
    bf16x8 wk;
    if constexpr (W8)
      wk = hl_frag8(wf[kk >> 1], kk & 1, sc);
    else
      wk = wf[kk];
#pragma unroll
    for (int t = 0; t < MT; ++t)
      acc[t] = mfma16(wk, *(const bf16x8*)(xs + (16 * t + r16) * XST + kc * 32 + 8 * g4), acc[t]);
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) *(f32x4*)(red + (t * NW + wave) * 256 + lane * 4) = acc[t];
}

// Phase 1's epilogue, one wave per row tile of q|k|v tile w: the 8 K slices of the row tile's `red` in order
// (lane: row m = m0 + (lane & 15), m0 = 16 x the row tile; columns 16 w + 4 g + i), then epi_rope's arithmetic on the prefetched operands (rp / rs: the row's
// position and slot, rb4 the bias, cs4 / sn4 the cos / sin row), written through.  KVQ != 0: the K rows
// and V columns go to the staging cache (slot 0, position = the row index).
template <int KVQ>
DEV void la_rope_append(const LmAttnArgs& a, const float* red, int w, int lane, int m0, int R, int rp, int rs,
                        bf16x4 rb4, bf16x4 cs4, bf16x4 sn4) {
  using namespace la;
  const RopeEpi& RP = a.qkv.rope;
  const int r16 = lane & 15, g4 = lane >> 4;
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float s = 0.f;
#pragma unroll
    for (int wv = 0; wv < NW; ++wv) s += red[wv * 256 + lane * 4 + i];
    v[i] = s;
  }
  const int n0 = 16 * w, hh = n0 / D, tt = (n0 % D) >> 4, m = m0 + r16;
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = rb(v[i] + bf(rb4[i]));   // q/k/v_proj output (bf16)
  if (hh < NH + NKV) {
    float u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = xor32(v[i]);
    if (g4 < 2 && m < R) {
      const int j = 8 * tt + 4 * g4;
      float cs[4], sn[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (RP.cs_tab) {
          cs[i] = bf(cs4[i]);
          sn[i] = bf(sn4[i]);
        } else {
          const float f = (float)rp * RP.inv_freq[j + i];
          cs[i] = rb(cosf(f));
          sn[i] = rb(sinf(f));
        }
      }
      bf16x4 o1, o2;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o1[i] = tobf(rb(v[i] * cs[i]) + rb(-u[i] * sn[i]));
        o2[i] = tobf(rb(u[i] * cs[i]) + rb(v[i] * sn[i]));
      }
      bf16* dst;
      if constexpr (KVQ != 0)   // K rows to the staging cache: slot 0, position = the row index
        dst = hh < NH ? RP.q_out + (long long)m * NH * D + hh * D
                      : a.stg.k + (long long)(hh - NH) * a.stg.s_head + (long long)m * D;
      else
        dst = hh < NH ? RP.q_out + (long long)m * NH * D + hh * D
                      : RP.kv.k + (long long)RP.layer * RP.kv.s_layer + (long long)rs * RP.kv.s_slot +
                            (long long)(hh - NH) * RP.kv.s_head + (long long)rp * D;
      MemWT::st8(dst + j, o1);
      MemWT::st8(dst + j + 64, o2);
    }
  } else if (m < R) {   // V cache in 32-position blocks of [dim][position] (common.h v_off)
    bf16* hb;
    if constexpr (KVQ != 0)
      hb = a.stg.v + (long long)(hh - NH - NKV) * a.stg.s_head;
    else
      hb = RP.kv.v + (long long)RP.layer * RP.kv.s_layer + (long long)rs * RP.kv.s_slot +
           (long long)(hh - NH - NKV) * RP.kv.s_head;
    const int dim0 = (n0 % D) + 4 * g4;
    const int vp = KVQ != 0 ? m : rp;
#pragma unroll
    for (int i = 0; i < 4; ++i) MemWT::st2(hb + v_off(dim0 + i, vp), tobf(v[i]));
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Attention unit u: its pair p = (row qi, kv head kh), its index ui among the pair's units, the row's
// length, the (layer, slot, kv head) cache base, and the Q fragments of the kv head's 6 query heads (loads
// issued; rows >= G of the 16 repeat row G - 1 until la_zero_pad_rows)
struct LaUnit {
  int qi, kh, ui, len;
  long long cbase;
};
DEV LaUnit la_unit_begin(const LmAttnArgs& a, const int* pre, int u, int r16, int g4, bf16x8 (&qf)[4]) {
  using namespace la;
  const RopeEpi& RP = a.qkv.rope;
  int p = 0;
  while (pre[p + 1] <= u) ++p;
  LaUnit t;
  t.qi = p / NKV;
  t.kh = p - t.qi * NKV;
  t.ui = u - pre[p];
  t.len = RP.pos[t.qi] + 1;
  t.cbase = (long long)RP.layer * RP.kv.s_layer + (long long)RP.slots[t.qi] * RP.kv.s_slot + (long long)t.kh * RP.kv.s_head;
  const bf16* qrow = RP.q_out + (long long)t.qi * NH * D + (t.kh * G + min(r16, G - 1)) * D + 8 * g4;
#pragma unroll
  for (int c = 0; c < 4; ++c) qf[c] = MemWT::ld16(qrow + 32 * c);
  return t;
}
// ... rows >= G of the 16 zeroed.  Apart from la_unit_begin: this waits for the Q loads, so the short forms
// call it after the unit's K and V loads are issued (one memory round trip per unit, not two); the long form
// calls it ahead of its first K set, as it always did.
DEV void la_zero_pad_rows(bf16x8 (&qf)[4], int r16) {
  if (r16 >= la::G) {
#pragma unroll
    for (int c = 0; c < 4; ++c) qf[c] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
  }
}

// k_lm_attn's K / V fragment loads (attn_dev.h attn_load_k / attn_load_v): global and non-temporal, a
// fragment's 8 codes as one 8-byte load
struct LaLdNT {
  static DEV bf16x8 ld(const bf16* p) { return hl_ldnt(p); }
  static DEV u32x2 ld(const unsigned char* p) { return hl_ldnt8h(p); }
};

// Unit u's partial: O[head][dim], then (m, l) per head.  O goes through this wave's 3 KB of LDS (xs is
// free in phase 2) so that each lane stores whole 16-byte pieces (as 8-byte write-through halves:
// narrower sc1 stores cost several times more per byte)
DEV void la_store_partial(const LmAttnArgs& a, int u, bf16* xs, int wave, int lane, const float (&mv)[4],
                          const float (&lv)[4], const f32x4 (&o)[8]) {
  using namespace la;
  const int r16 = lane & 15, g4 = lane >> 4;
  float* pu = a.part + (long long)u * PART;
  float* ow = (float*)xs + wave * (G * D);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int h = 4 * g4 + i;
    if (h < G) {
#pragma unroll
      for (int j = 0; j < 8; ++j) ow[h * D + 16 * j + r16] = o[j][i];
      if (r16 == 0) {
        const float2 mlv = make_float2(mv[i], lv[i]);
        __hip_atomic_store((gu64*)(pu + G * D + 2 * h), __builtin_bit_cast(unsigned long long, mlv), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int q = 0; q < G * D / 256; ++q) {
    const f32x4 v4 = *(const f32x4*)(ow + (q * 64 + lane) * 4);
    const u64x2 uv = __builtin_bit_cast(u64x2, v4);
    __hip_atomic_store((gu64*)(pu + (q * 64 + lane) * 4), uv[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((gu64*)(pu + (q * 64 + lane) * 4 + 2), uv[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the LDS reads done before the next unit's writes
}

// The KVQ forms' appended rows, for the unit t over keys [c0, w1) whose fragments the caller has loaded
// (KVQ = 1: codes kq / vq and the exponents xk / xv of this lane's score columns; KVQ = 2: bf16 kf / vf).
// The keys this pass appends (row m2 of the pass: the unit's slot, a position in [c0, w1)) are not
// in the cache: what the loads returned at their positions is replaced here and never used.  A pass may
// carry several rows of one slot (a short prompt is one pass below the prefill threshold), so "appended"
// is decided per key against the pass's tables tslot / tpos / tmin (LDS), not per tail unit.
// Every unit that holds such a key takes row m2's staged K row and V row (written through by phase
// 1's workgroups before wait 1; nt loads bypass L1), runs them through the row quantiser -- a pure
// function, so every reader derives the same values -- and uses code * 2^e (KVQ = 1: the codes and
// the exponent).  The unit of query row m2 itself also stores the result at the real (slot,
// position); nothing reads that entry in this launch.  All lanes load the row: K in the fragment
// layout (dims 32 c + 8 g ..), V as dims 16 j + r; a row's amax is then the wave's.  KVQ = 1 ends with
// codes -> bf16 (exact) into kf / vf, for the bf16 step.
template <int KVQ>
DEV void la_kvq_rows(const LmAttnArgs& a, const int* tslot, const LaUnit& t, int c0, int w1, int R, int lane,
                     bf16x8 (&kf)[2][4], bf16x8 (&vf)[8], u32x2 (&kq)[2][4], u32x2 (&vq)[8], int (&xk)[2], int (&xv)[2]) {
  using namespace la;
  const RopeEpi& RP = a.qkv.rope;
  const int *tpos = tslot + RMAX, *tmin = tpos + RMAX;
  const int r16 = lane & 15, g4 = lane >> 4;
  const int qi = t.qi, kh = t.kh;
  const long long cbase = t.cbase;
  if (w1 > __builtin_amdgcn_readfirstlane(tmin[qi])) {
    const int uslot = __builtin_amdgcn_readfirstlane(tslot[qi]);
    for (int m2 = 0; m2 < R; ++m2) {
      const int ps = __builtin_amdgcn_readfirstlane(tpos[m2]);
      if (__builtin_amdgcn_readfirstlane(tslot[m2]) != uslot || ps < c0 || ps >= w1) continue;
      const bf16* SK = a.stg.k + (long long)kh * a.stg.s_head + (long long)m2 * D;
      const bf16* SV = a.stg.v + (long long)kh * a.stg.s_head;
      bf16x8 sk[4];
      bf16 sv[8];
#pragma unroll
      for (int c = 0; c < 4; ++c) sk[c] = hl_ldnt(SK + 32 * c + 8 * g4);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        sv[j] = __builtin_bit_cast(bf16, __builtin_nontemporal_load((const gu16*)(SV + v_off(16 * j + r16, m2))));
      float ak = 0.f, av = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 8; ++i) ak = fmaxf(ak, fabsf(bf(sk[c][i])));
#pragma unroll
      for (int j = 0; j < 8; ++j) av = fmaxf(av, fabsf(bf(sv[j])));
      const int eK = row_exp(wave_max(ak)), eV = row_exp(wave_max(av));
      u32x2 pk[4];      // K codes, fragment order
      unsigned cv[8];   // V codes of dims 16 j + r
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        unsigned cc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) cc[i] = enc_e4m3(ldexpf(bf(sk[c][i]), -eK));
        pk[c][0] = cc[0] | (cc[1] << 8) | (cc[2] << 16) | (cc[3] << 24);
        pk[c][1] = cc[4] | (cc[5] << 8) | (cc[6] << 16) | (cc[7] << 24);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) cv[j] = enc_e4m3(ldexpf(bf(sv[j]), -eV));
      const int ee = ps - (c0 + 8 * g4);   // this lane's V fragments hold key ps at element ee (0 .. 7)
      const bool own = m2 == qi;
      if constexpr (KVQ == 1) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          const bool hit = c0 + 16 * tt + r16 == ps;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            kq[tt][c][0] = hit ? pk[c][0] : kq[tt][c][0];
            kq[tt][c][1] = hit ? pk[c][1] : kq[tt][c][1];
          }
          xk[tt] = hit ? eK : xk[tt];
          xv[tt] = hit ? eV : xv[tt];
        }
        const unsigned sh = 8u * (unsigned)(ee & 3);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const unsigned lo = (vq[j][0] & ~(0xffu << sh)) | (cv[j] << sh);
          const unsigned hi = (vq[j][1] & ~(0xffu << sh)) | (cv[j] << sh);
          vq[j][0] = (ee >= 0 && ee < 4) ? lo : vq[j][0];
          vq[j][1] = (ee >= 4 && ee < 8) ? hi : vq[j][1];
        }
        if (own) {
          if (r16 == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) *(u32x2*)(a.kv8.k + cbase + (long long)ps * D + 32 * c + 8 * g4) = pk[c];
          }
          if (g4 == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) a.kv8.v[cbase + v_off(16 * j + r16, ps)] = (unsigned char)cv[j];
          }
          if (lane == 0) {
            a.kv8.ek[cbase / D + ps] = (signed char)eK;
            a.kv8.ev[cbase / D + ps] = (signed char)eV;
          }
        }
      } else {   // KVQ = 2: the dequantised rows (k_kv_rows' read expression), bf16 throughout
        bf16x8 dk[4];
        bf16 dv[8];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int i = 0; i < 8; ++i) dk[c][i] = tobf(ldexpf(dec_e4m3((pk[c][i >> 2] >> (8 * (i & 3))) & 0xffu), eK));
#pragma unroll
        for (int j = 0; j < 8; ++j) dv[j] = tobf(ldexpf(dec_e4m3(cv[j]), eV));
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
          const bool hit = c0 + 16 * tt + r16 == ps;
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int i = 0; i < 8; ++i) kf[tt][c][i] = hit ? dk[c][i] : kf[tt][c][i];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
          for (int e = 0; e < 8; ++e) vf[j][e] = ee == e ? dv[j] : vf[j][e];
        if (own) {
          if (r16 == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) *(bf16x8*)(RP.kv.k + cbase + (long long)ps * D + 32 * c + 8 * g4) = dk[c];
          }
          if (g4 == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) RP.kv.v[cbase + v_off(16 * j + r16, ps)] = dv[j];
          }
        }
      }
    }
  }
  if constexpr (KVQ == 1) attn_frags_bf16(kq, vq, kf, vf);   // codes -> bf16 (exact), then the bf16 step
}

// Phase 2, short forms: the attention units (row, kv head, 32 keys) of workgroup w's wave.  The unit's K and
// V loads (KVQ = 1: as e4m3 codes, 8 bytes where bf16 loads 16, and the row exponents of this lane's
// score columns), the KVQ patch, one uncarried step, the partial.
template <int KVQ>
DEV void la_short_units(const LmAttnArgs& a, const int* pre, const int* tslot, bf16* xs, bf16* pt, int R, int w, int wave,
                        int lane) {
  using namespace la;
  const RopeEpi& RP = a.qkv.rope;
  const int r16 = lane & 15, g4 = lane >> 4;
  const int U = pre[2 * R];
  for (int u = w + GRID * wave; u < U; u += GRID * NW) {
    bf16x8 qf[4], kf[2][4], vf[8];
    const LaUnit t = la_unit_begin(a, pre, u, r16, g4, qf);
    const int c0 = t.ui * 32, w1 = min(t.len, c0 + 32);
    u32x2 kq[2][4], vq[8];
    int xk[2] = {0, 0}, xv[2] = {0, 0};
    if constexpr (KVQ == 1) {
      attn_load_k<LaLdNT>(a.kv8.k + t.cbase, a.kv8.ek + t.cbase / D, a.kv8.ev + t.cbase / D, c0, w1, r16, g4, kq, xk, xv);
      attn_load_v<LaLdNT>(a.kv8.v + t.cbase, c0, w1, r16, g4, vq);
    } else {
      attn_load_k<LaLdNT>(RP.kv.k + t.cbase, nullptr, nullptr, c0, w1, r16, g4, kf, xk, xv);
      attn_load_v<LaLdNT>(RP.kv.v + t.cbase, c0, w1, r16, g4, vf);
    }
    if constexpr (KVQ != 0) la_kvq_rows<KVQ>(a, tslot, t, c0, w1, R, lane, kf, vf, kq, vq, xk, xv);
    la_zero_pad_rows(qf, r16);
    float mv[4], lv[4];
    f32x4 o[8];   // lane: O[head 4 g + i][dim 16 j + r]
    attn_step<KVQ == 1, false>(a.scale, qf, kf, vf, xk, xv, c0, w1, pt + wave * 512, r16, g4, mv, lv, o);
    la_store_partial(a, u, xs, wave, lane, mv, lv, o);
  }
}

// Phase 2, long form: unit u of a pair covers keys [cu, ue) = 32 s keys, s = la_unit_steps(len) from the
// row's own length; the wave runs the carried step over them.  The next step's K fragments load under
// this step's MFMAs (two K sets in turn); V loads at the step's start.
DEV void la_long_units(const LmAttnArgs& a, const int* pre, bf16* xs, bf16* pt, int R, int w, int wave, int lane) {
  using namespace la;
  const RopeEpi& RP = a.qkv.rope;
  const int r16 = lane & 15, g4 = lane >> 4;
  const int U = pre[2 * R];
  int x0[2] = {0, 0};   // bf16 KV: no row exponents
  for (int u = w + GRID * wave; u < U; u += GRID * NW) {
    bf16x8 qf[4];
    const LaUnit t = la_unit_begin(a, pre, u, r16, g4, qf);
    la_zero_pad_rows(qf, r16);
    const int len = t.len, s = la_unit_steps(len);
    const int cu = __builtin_amdgcn_readfirstlane(t.ui * 32 * s);
    const int ue = __builtin_amdgcn_readfirstlane(min(len, cu + 32 * s));
    const bf16* K = RP.kv.k + t.cbase;
    const bf16* VB = RP.kv.v + t.cbase;
    float mv[4], lv[4];
    f32x4 o[8];   // lane: O[head 4 g + i][dim 16 j + r]
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      mv[i] = -INFINITY;
      lv[i] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16* ptw = pt + wave * 512;
    // one step on the K set `kf`; `kn` takes the next step's K when there is one
    auto step = [&](int c0, bf16x8(&kf)[2][4], bf16x8(&kn)[2][4]) __attribute__((always_inline)) {
      const int w1 = min(len, c0 + 32);
      bf16x8 vf[8];
      attn_load_v<LaLdNT>(VB, c0, w1, r16, g4, vf);
      if (c0 + 32 < ue) attn_load_k<LaLdNT>(K, nullptr, nullptr, c0 + 32, min(len, c0 + 64), r16, g4, kn, x0, x0);
      attn_step<false, true>(a.scale, qf, kf, vf, x0, x0, c0, w1, ptw, r16, g4, mv, lv, o);
    };
    bf16x8 ka[2][4], kb[2][4];
    attn_load_k<LaLdNT>(K, nullptr, nullptr, cu, min(len, cu + 32), r16, g4, ka, x0, x0);
    for (int c0 = cu; c0 < ue; c0 += 64) {
      step(c0, ka, kb);
      if (c0 + 32 >= ue) break;
      step(c0 + 32, kb, ka);
    }
    la_store_partial(a, u, xs, wave, lane, mv, lv, o);
  }
}

// Phase 3: the merge, one wave per (row, query head); lane: dims 2 l, 2 l + 1.
// One round of loads for <= 32 units: lane u's (m, l) of units u and u + 64, and
// every lane's O pairs of units 0..31, issued together; the weights
// e_u = e^{m_u - M} then reach every lane by readlane, summed in unit order.
DEV void la_merge(const LmAttnArgs& a, const int* pre, int R, int w, int wave, int lane) {
  using namespace la;
  for (int x = w + GRID * wave; x < R * NH; x += GRID * NW) {
    const int qi = x / NH, hq = x - qi * NH, kh = hq / G, h = hq - kh * G;
    const int u0 = pre[qi * NKV + kh], nu = pre[qi * NKV + kh + 1] - u0;   // 1 .. LA_MAX_KEYS / 32
    const float* pb = a.part + (long long)u0 * PART;
    const unsigned long long ml0 = MemWT::l64(pb + (long long)min(lane, nu - 1) * PART + G * D + 2 * h);
    const unsigned long long ml1 = MemWT::l64(pb + (long long)min(lane + 64, nu - 1) * PART + G * D + 2 * h);
    unsigned long long ov[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) ov[q] = MemWT::l64(pb + (long long)min(q, nu - 1) * PART + h * D + 2 * lane);
    const float m0 = lane < nu ? __uint_as_float((unsigned)ml0) : -INFINITY;
    const float m1 = lane + 64 < nu ? __uint_as_float((unsigned)ml1) : -INFINITY;
    const float M = wave_max(fmaxf(m0, m1));
    const float e0 = lane < nu ? __expf(m0 - M) : 0.f, e1 = lane + 64 < nu ? __expf(m1 - M) : 0.f;
    const float el0 = e0 * __uint_as_float((unsigned)(ml0 >> 32)), el1 = e1 * __uint_as_float((unsigned)(ml1 >> 32));
    float n0 = 0.f, n1 = 0.f, den = 0.f;
    for (int s0 = 0; s0 < nu; s0 += 32) {
      if (s0) {
#pragma unroll
        for (int q = 0; q < 32; ++q) ov[q] = MemWT::l64(pb + (long long)min(s0 + q, nu - 1) * PART + h * D + 2 * lane);
      }
#pragma unroll
      for (int q = 0; q < 32; ++q) {
        const int u = s0 + q;
        if (u < nu) {
          const float e = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(u < 64 ? e0 : e1), u & 63));
          const float el = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(u < 64 ? el0 : el1), u & 63));
          // (fused, both dims: written out so that the bits do not hang on the vectoriser's choice)
          n0 = __builtin_fmaf(e, __uint_as_float((unsigned)ov[q]), n0);
          n1 = __builtin_fmaf(e, __uint_as_float((unsigned)(ov[q] >> 32)), n1);
          den += el;
        }
      }
    }
    const bf16 b0 = tobf(n0 / den), b1 = tobf(n1 / den);
    const unsigned bits = (unsigned)__builtin_bit_cast(unsigned short, b0) |
                          ((unsigned)__builtin_bit_cast(unsigned short, b1) << 16);
    __hip_atomic_store((hl_gu32*)(a.att + (long long)qi * H + hq * D + 2 * lane), bits, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <bool W8, int KVQ, bool LONG, int MT>
__global__ void __launch_bounds__(la::NT) k_lm_attn(LmAttnArgs a) {
  using namespace la;
  using L = Lds<MT>;
  constexpr int ROWS = L::ROWS;
  static_assert(!LONG || KVQ == 0, "the long form reads a bf16 cache");
  static_assert(MT == 1 || (MT == 2 && KVQ == 0), "the KVQ forms' tables and staged rows are the 16-row class's");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bf16* xs = (bf16*)(smem + L::XS);        // phase 1: [16 MT][XST] A rows; phase 4: attention rows
  float* red = (float*)(smem + L::RED);    // [MT row tiles][8 waves][256] MFMA partials
  bf16* pt = (bf16*)(smem + L::PT);        // [8 waves][16][32] P tiles
  bf16* nw_s = (bf16*)(smem + L::NWS);
  float* inv_s = (float*)(smem + L::SM);   // [16 MT]
  int* pre = (int*)(smem + L::SM + L::INV_B);    // [2R + 1] unit prefix over (row, kv head) pairs
  unsigned* ok_s = (unsigned*)(smem + L::SM + L::INV_B + 4 * (2 * ROWS + 1));
  int* tslot = (int*)(smem + L::KT);       // KVQ: [16] the pass's slots, [16] positions, [16] first appended position
  int *tpos = tslot + RMAX, *tmin = tpos + RMAX;

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, w = blockIdx.x, R = a.R;
  const int r16 = lane & 15, g4 = lane >> 4;
  const RopeEpi& RP = a.qkv.rope;
  const bool qt = w < TQ, ot = w >= O0 && w < O0 + TO;
  // the epilogues of phases 1 and 4 run one wave per row tile: wave `et` rows 16 et + (lane & 15)
  const bool ew = MT == 1 ? wave == 0 : wave < MT;
  const int et = MT == 1 ? 0 : wave, em = 16 * et + r16;
  unsigned g0 = 0;
  if (threadIdx.x == 0)
    g0 = hl_base_gen(a.sync, pk::GEN_LM_ATTN);
  // the attention units: pair p = row * NKV + kv head holds ceil(len / 32) of
  // them (positions read first: a wait for them then leaves the streams in flight)
  int nunit = 0;
  if (threadIdx.x < 2 * ROWS) {
    const int qi = threadIdx.x / NKV;
    if constexpr (LONG)   // ceil(len / (32 s)) units of s = la_unit_steps(len) steps: the same units while len <= 4,096
      nunit = qi < R ? la_unit_count(RP.pos[qi] + 1) : 0;
    else
      nunit = qi < R ? (RP.pos[qi] + 1 + 31) / 32 : 0;
  }
  int ts = 0, tp = 0;   // KVQ: row threadIdx.x's slot and position (rows >= R repeat R - 1)
  if constexpr (KVQ != 0) {
    if (threadIdx.x < RMAX) {
      ts = RP.slots[min((int)threadIdx.x, R - 1)];
      tp = RP.pos[min((int)threadIdx.x, R - 1)];
    }
  }
  la_stamp(a, 0);
  bf16x4 rv_pre = (bf16x4){0, 0, 0, 0};   // o_proj's residual operand (variant 4: loaded at entry)
  if ((a.variant & 4) && ot && ew && em < R)
    rv_pre = *(const bf16x4*)(rm_bf(a.res, em) + 16 * (w - O0) + 4 * g4);

  // ================= phase 1: q|k|v tile (workgroups < 128) / o_proj weights (128..223)
  // W8: the exponent of this lane's row (lane & 15) of this workgroup's tile (q|k|v or o_proj) is loaded
  // here, ahead of the A side, so the vmcnt immediate below counts weight loads only
  WF<W8> wq[NWL<W8>], wo[NWL<W8>];
  int ex = 0;
  if constexpr (W8)   // (unconditional, clamped: no branch to wait in; read through hl_vopaque where first used)
    ex = ot ? a.owe[16 * (w - O0) + r16] : a.qkv.w8e[16 * min(w, TQ - 1) + r16];
  const int ln = hl_vopaque(lane);
  // the epilogue waves' RoPE operands (row m = 16 et + (lane & 15), columns 16 w + 4 g ..): position,
  // slot and bias first, the cos / sin row (dependent on the position) after the weights
  int rp = 0, rs = 0;
  bf16x4 rb4 = (bf16x4){0, 0, 0, 0}, cs4 = rb4, sn4 = rb4;
  if (qt && ew) {
    const int mm = min(em, R - 1);
    rp = RP.pos[mm];
    rs = RP.slots[mm];
    rb4 = *(const bf16x4*)(a.qkv.epi.bias + 16 * w + 4 * g4);
  }
  if (qt) {
    const int qn = (a.variant & 1) ? R * 3 : ROWS * 3;
    for (int q = wave; q < qn; q += NW) {   // row q / 3, 64-chunk piece q % 3 (rows >= R re-read R - 1)
      const int m = q / 3, i = q - m * 3;
      hl_dma16<false>(xs + m * XST + i * 512, rm_bf(a.qkv.a, min(m, R - 1)) + (i * 64 + ln) * 8);
    }
    if (wave < 3) hl_dma16<false>(nw_s + wave * 512, a.nw + (wave * 64 + ln) * 8);
    la_load_tile<W8>(wq, a.qkv.w, a.qkv.w8, w, wave, ln);
    // this wave's A-side DMA: the NWL weight loads (6; W8: 3 -- its exponent load is older) are younger
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NWL<W8>) : "memory");
    if (ew && RP.cs_tab) {
      const int j = 8 * (w & 7) + 4 * (g4 & 1);
      cs4 = *(const bf16x4*)(RP.cs_tab + (long long)rp * D + j);
      sn4 = *(const bf16x4*)(RP.cs_tab + (long long)rp * D + 64 + j);
    }
  } else if (ot && !(a.variant & 2)) {
    la_load_tile<W8>(wo, a.ow, a.ow8, w - O0, wave, ln);
  }
  if (threadIdx.x < 2 * ROWS) pre[threadIdx.x + 1] = nunit;
  if constexpr (KVQ != 0) {
    if (threadIdx.x < RMAX) {
      tslot[threadIdx.x] = ts;
      tpos[threadIdx.x] = tp;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    pre[0] = 0;
    for (int p = 1; p <= 2 * ROWS; ++p) pre[p] += pre[p - 1];
  }
  if constexpr (KVQ != 0) {   // (read in phase 2, after the barriers below)
    if (threadIdx.x < RMAX) {
      int mn = tp;
      for (int m2 = 0; m2 < R; ++m2) mn = tslot[m2] == ts ? min(mn, tpos[m2]) : mn;
      tmin[threadIdx.x] = mn;
    }
  }
  la_stamp(a, 1);
  if (qt) {
    const int mr = (a.variant & 1) ? R : ROWS;   // (rows >= R of the MFMA are never stored)
    for (int m = wave; m < mr; m += NW) {   // inverse RMS in k_rmsnorm's order
      float ss = 0.f;
      for (int c = ln; c < H / 8; c += 64) {
        const bf16x8 v = *(const bf16x8*)(xs + m * XST + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += bf(v[j]) * bf(v[j]);
      }
      ss = wave_sum(ss);
      if (ln == 0) inv_s[m] = rsqrtf(ss / (float)H + a.eps);
    }
    __syncthreads();
    hl_rows_norm<H, true, false>(xs, XST, mr, nw_s, nullptr, nullptr, 0, inv_s, hl_vopaque((int)threadIdx.x), NT);
    __syncthreads();
    la_tile_mfma<W8, MT>(wq, W8 ? w8_scale(hl_vopaque(ex)) : 0.f, xs, red, wave, lane);
    __syncthreads();
    if (ew) la_rope_append<KVQ>(a, red + et * (NW * 256), w, lane, 16 * et, R, rp, rs, rb4, cs4, sn4);
  }
  if (!la_wait(a, g0, 1, ok_s, w)) return;
  if (ot && (a.variant & 2)) la_load_tile<W8>(wo, a.ow, a.ow8, w - O0, wave, ln);

  // ================= phase 2: attention units (row, kv head, 32 keys; LONG: 32 s keys), one wave each
  if constexpr (LONG)
    la_long_units(a, pre, xs, pt, R, w, wave, lane);
  else
    la_short_units<KVQ>(a, pre, tslot, xs, pt, R, w, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (!la_wait(a, g0, 2, ok_s, w)) return;

  // ================= phase 3: merge, one wave per (row, query head)
  la_merge(a, pre, R, w, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (!la_wait(a, g0, 3, ok_s, w) || !ot) return;

  // ================= phase 4: o_proj tile w - O0 over the attention rows + residual
  for (int q = wave; q < ((a.variant & 1) ? R * 3 : ROWS * 3); q += NW) {
    const int m = q / 3, i = q - m * 3;
    hl_dma16<true>(xs + m * XST + i * 512, a.att + (long long)min(m, R - 1) * H + (i * 64 + ln) * 8);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  la_tile_mfma<W8, MT>(wo, W8 ? w8_scale(hl_vopaque(ex)) : 0.f, xs, red, wave, lane);
  __syncthreads();
  if (ew && em < R) {   // EPI_RES: out = bf16(res + bf16(acc)), row m = 16 et + (lane & 15)
    const int m = em, n = 16 * (w - O0) + 4 * g4;
    const float* redt = red + et * (NW * 256);
    const bf16x4 rv = (a.variant & 4) ? rv_pre : *(const bf16x4*)(rm_bf(a.res, m) + n);
    bf16x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s = 0.f;
#pragma unroll
      for (int wv = 0; wv < NW; ++wv) s += redt[wv * 256 + lane * 4 + i];
      o[i] = tobf(bf(rv[i]) + rb(s));
    }
    *(bf16x4*)(rm_bfw(a.out, m) + n) = o;
  }
  la_stamp(a, 8);
}

// ---- host side: the eleven forms, one table.  A form is (W8, KVQ, LONG, MT); LONG exactly when the pass is
// planned past LA_MAX_KEYS, MT = 2 exactly when the pass has more than 16 rows.  KVQ = 2 (the diagnostic)
// is built for bf16 weights only, the KVQ forms read their own cache formats only in the short step, and
// no KVQ form is built at MT = 2 (their tables and staged rows are the 16-row class's): an FP8-KV engine
// keeps its launches above 16 rows.
struct LaForm {
  bool w8;
  int kvq;
  bool lng;
  int mt;
};
struct LaKernel {
  LaForm form;
  void (*kernel)(LmAttnArgs);
  bool (*resident)();   // persist_resident_kernel of `kernel`, queried on first use
  int lds;              // the row class's carve-up (la::Lds<MT>::TOTAL)
};
template <bool W8, int KVQ, bool LONG, int MT>
static bool la_resident() {
  static const bool ok =
      persist_resident_kernel((const void*)k_lm_attn<W8, KVQ, LONG, MT>, la::NT, la::Lds<MT>::TOTAL, la::GRID);
  return ok;
}
template <bool W8, int KVQ, bool LONG, int MT = 1>
constexpr LaKernel la_kernel() {
  return {{W8, KVQ, LONG, MT}, k_lm_attn<W8, KVQ, LONG, MT>, la_resident<W8, KVQ, LONG, MT>, la::Lds<MT>::TOTAL};
}
static const LaKernel LA_KERNELS[] = {la_kernel<false, 0, false>(),    la_kernel<true, 0, false>(),    la_kernel<false, 1, false>(),
                                      la_kernel<true, 1, false>(),     la_kernel<false, 2, false>(),   la_kernel<false, 0, true>(),
                                      la_kernel<true, 0, true>(),      la_kernel<false, 0, false, 2>(), la_kernel<true, 0, false, 2>(),
                                      la_kernel<false, 0, true, 2>(),  la_kernel<true, 0, true, 2>()};
// the form of a pass of `rows` rows and `keys` keys, or nullptr: no such form
static const LaKernel* la_form(bool w8, int kvq, int keys, int rows) {
  if (keys < 1 || keys > LA_LONG_MAX_KEYS || rows < 1 || rows > 16 * la::MTMAX) return nullptr;
  const LaForm f{w8, kvq, keys > LA_MAX_KEYS, rows > la::RMAX ? 2 : 1};
  for (const LaKernel& e : LA_KERNELS)
    if (e.form.w8 == f.w8 && e.form.kvq == f.kvq && e.form.lng == f.lng && e.form.mt == f.mt) return &e;
  return nullptr;
}
extern "C" int vv_diag_lm_attn_form_rows(int w8, int kvq, int keys, int rows, int* out) {
  const LaKernel* e = out && (w8 == 0 || w8 == 1) ? la_form(w8 != 0, kvq, keys, rows) : nullptr;
  if (!e) return 1;
  out[0] = e->form.w8;
  out[1] = e->form.kvq;
  out[2] = e->form.lng;
  out[3] = e->form.mt;
  return 0;
}
// (the table of passes of <= 16 rows: out[0..2])
extern "C" int vv_diag_lm_attn_form(int w8, int kvq, int keys, int* out) {
  int f[4];
  if (!out || vv_diag_lm_attn_form_rows(w8, kvq, keys, la::RMAX, f)) return 1;
  out[0] = f[0];
  out[1] = f[1];
  out[2] = f[2];
  return 0;
}

bool lm_attn_fits(bool w8, int kvq, int H, int nh, int nkv, int d, int R, int keys) {
  if (H != la::H || nh != la::NH || nkv != la::NKV || d != la::D) return false;
  const LaKernel* e = la_form(w8, kvq, keys, R);
  return e && e->resident();
}

// (the most units of any row of <= keys keys: la_unit_count is not monotonic past LA_MAX_KEYS, where a
// row of LA_MAX_KEYS keys holds the maximum, LA_MAX_KEYS / 32)
size_t lm_attn_part_floats(int R, int keys) {
  return (size_t)R * la::NKV * (((keys < LA_MAX_KEYS ? keys : LA_MAX_KEYS) + 31) / 32) * la::PART;
}
extern "C" int vv_diag_lm_attn_plan(int len, int* out) {
  if (len < 1 || len > LA_LONG_MAX_KEYS || !out) return 1;
  out[0] = la_unit_steps(len);
  out[1] = la_unit_count(len);
  return 0;
}

// the W8 form when a code pointer is set (all four of q|k|v's and o_proj's codes and exponents, or it is an
// error); the KV form from a.kvq (1: the FP8 cache a.kv8; 2: the diagnostic round trip, bf16 weights only),
// which needs the staging cache and, for the bounds of phase 1's staged append, its 16 positions
int launch_lm_attn(const LmAttnArgs& a, int keys, hipStream_t st) {
  const bool w8 = a.qkv.w8 || a.qkv.w8e || a.ow8 || a.owe;
  if (w8 && (!a.qkv.w8 || !a.qkv.w8e || !a.ow8 || !a.owe)) return 1;
  const int kvq = a.kvq;
  if (kvq < 0 || kvq > 2 || (kvq == 2 && w8)) return 1;
  if (kvq && (!a.stg.k || !a.stg.v || a.stg.max_ctx < la::RMAX || a.stg.s_head < (long long)la::D * 32)) return 1;
  if (kvq == 1 && (!a.kv8.k || !a.kv8.v || !a.kv8.ek || !a.kv8.ev || a.qkv.rope.kv.s_layer % la::D ||
                   a.qkv.rope.kv.s_slot % la::D || a.qkv.rope.kv.s_head % la::D))
    return 1;
  if (kvq == 2 && (!a.qkv.rope.kv.k || !a.qkv.rope.kv.v)) return 1;
  if (!lm_attn_fits(w8, kvq, la::H, la::NH, la::NKV, la::D, a.R, keys) || a.qkv.M != a.R || a.qkv.N != la::NQKV ||
      a.qkv.K != la::H || !a.qkv.epi.bias || !a.part || !a.att || !a.sync || !a.err)
    return 3;
  const LaKernel* e = la_form(w8, kvq, keys, a.R);
  hipLaunchKernelGGL(e->kernel, dim3(la::GRID), dim3(la::NT), e->lds, st, a);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
