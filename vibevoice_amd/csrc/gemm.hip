// bf16 MFMA GEMMs for gfx950:  Y[m, n] = epi( sum_k xf(A)[m, k] * W[n, k] )
//
// W is a PyTorch Linear weight [N, K], or a conv weight that the loader
// re-packed to the same [N, K] form (see vibevoice_amd/weights.py), stored in
// MFMA-fragment order ("mfma_pack"): the 16 x 32 block (tile t, chunk c) is 1 KB
// contiguous at (t * K/32 + c) * 512 elements, lane l's 8 elements at l * 8 =
// W[16t + (l & 15)][32c + 8(l >> 4) .. +7] — every wave load is one coalesced
// 1 KB read instead of 16 row fragments of 64 B.
//   * causal conv k, stride s, channels-last input buffer with (k - s) history
//     rows in front:  A row t = buffer + t*s*C_in, K = k*C_in  (lda = s*C_in),
//   * 2-tap ConvTranspose (k = 2r, stride r): A row t = rows [t-1, t] of the
//     input buffer (1 history row), N = r*C_out and one output row = r
//     consecutive channels-last output rows.
// so every linear / conv layer on the hot path is this one kernel family.
//
// Fusions (the producer / consumer of each GEMM folded into it):
//   * A transform (XF_*): RMSNorm (+ weight, + adaLN modulate) of the A rows, or
//     SiLU(row + vec), applied to each A fragment as it is loaded.  The inverse
//     RMS of the block's rows is computed in a prologue (every workgroup redoes
//     it: at M <= 64 that is a few KB of L2 reads against MBs of weights).
//   * epilogues (EPI_*): bias, GELU, SiLU(gate)*up, gated / layer-scaled
//     residual, RoPE + KV-cache append, CFG + DPM-Solver++ update.
//
// Two shapes:
//   k_gemv : M <= 64 (LM decode rows, diffusion-head rows, codec stage at T=1).
//            HBM-bound weight stream.  MFMA 16x16x32 with W as the A operand
//            (16 weight rows = the MFMA M dim) and the <=16*MREP activation rows
//            as the B operand.  One workgroup per 16 weight rows; up to 16 waves
//            split K and each wave issues U chunks (U x 1 KB per wave) of weight
//            loads before its first MFMA, so a 16-wave workgroup keeps >100 KB in
//            flight (the "GEMV / M <= 16" row of cdna_hip_programming.md: no LDS
//            staging).  Waves reduce through LDS.  Cross-workgroup split-K (agent
//            release / ticket / acquire, Guideline 16) only for few-tile shapes.
//   k_gemm : M > 64 (codec stages at T >= 8, LM prefill).  64 x BN workgroup
//            tile, 4 waves of 32 x BN/2, operands straight from L2.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "attn_dev.h"
#include "codec_dev.h"
#include "kernels.h"
#include "gemv_dev.h"

// Diagnostic timestamps (tools/gemv_stamps.py): 100 MHz real-time clock, one
// lane per workgroup, to a buffer nothing else reads (a.stamps == nullptr in
// every product call).
DEV void stamp(const GemmArgs& a, int which) {
  if (a.stamps && threadIdx.x == 0) {
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
    a.stamps[((long long)blockIdx.y * gridDim.x + blockIdx.x) * 4 + which] = t;
  }
}

// ------------------------------------------------------------------ GEMV
// (the K-range index math and its "read blockDim first" rule: gemv_dev.h part_of, k_range)
// Split-K hand-off of the 16 x (16*MREP) fp32 tile between the workgroups of one
// tile column: every split stores its slab, takes a ticket, the last arriver
// sums the slabs in split order (deterministic) and runs the epilogue.
//   handoff 0: plain stores + agent release / acquire fences (Guideline 16 R1)
//   handoff 1: sc1 (write-through) 4-B stores, vmcnt(0) in every storing wave,
//              one agent atomic per workgroup, sc1 loads by the last arriver
//              (MI355X_MICROARCH.md "Valid forms", first table row)
// Returns true in the workgroup that must run the epilogue (red[] = sums).
DEV bool splitk_handoff(const GemmArgs& a, float* red, int TILE, unsigned* last_flag, int NT) {
  float* slab = a.ws + ((long long)blockIdx.x * a.ksplit + blockIdx.y) * TILE;
  const int t = threadIdx.x;
  if (a.handoff == 1) {
    for (int e = t; e < TILE; e += NT) __hip_atomic_store(slab + e, red[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    for (int e = t; e < TILE; e += NT) slab[e] = red[e];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (t == 0) {
    if (a.handoff != 1) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const unsigned tk = __hip_atomic_fetch_add(&a.counters[blockIdx.x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *last_flag = tk == (unsigned)(a.ksplit - 1) ? 1u : 0u;
    if (*last_flag) {
      if (a.handoff != 1) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __hip_atomic_store(&a.counters[blockIdx.x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  if (!*last_flag) return false;
  const float* slabs = a.ws + (long long)blockIdx.x * a.ksplit * TILE;
  for (int e = t; e < TILE; e += NT) {
    float s = 0.f;
    if (a.handoff == 1) {
      for (int k = 0; k < a.ksplit; ++k) s += __hip_atomic_load(slabs + k * TILE + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      for (int k = 0; k < a.ksplit; ++k) s += slabs[k * TILE + e];
    }
    red[e] = s;
  }
  __syncthreads();
  return true;
}

// M <= 16: the workgroup's A rows (its K range, transformed) are staged once in
// LDS; each wave streams its weight chunks with a two-deep register ping-pong
// (U chunks = U KB per wave in flight while the previous U are multiplied).
// RW instantiations: the fused RMSNorm prologue with whole rows per wave.  Wave
// w loads rows w*RPW .. w*RPW+RPW-1 (lane l: 8-column items l, l+64, ...), so a
// row's sum of squares is one in-register accumulation + wave_sum and the norm
// is applied before the A rows ever reach LDS: one barrier instead of three and
// no LDS round trip of partial sums.  Each row's summation order is the one the
// item-per-thread form used (per-item partials when that form was "fast", one
// running sum otherwise = k_rmsnorm's), so both forms are bit-identical.
// (Rejected variants -- weights issued twice as deep before the prologue, a
// one-round-trip M = 16 prologue, epilogue operands prefetched at kernel start --
// are recorded with their measurements in DESIGN.md and no longer built.)
// TPW = 5: the balanced many-tile form (gemm_decide): one workgroup per CU, 4 or
// 5 tiles each, 2 waves per tile (10 waves)
constexpr int gemv1_max_waves(int tpw) { return tpw == 5 ? 10 : 8; }
constexpr int GEMV1_Q = 4;   // A items per thread on the fast path
// ---- A staging into LDS (rows [0, M) x chunks [b0, b1), row stride padded
// 16 B), overlapped with the first weight chunks: six prologue forms, each
// given the workgroup's geometry and `first`, the callable that issues the
// wave's first weight batch.  vmcnt waits are in issue order, so every form
// that waits on A-side loads (row chunk + its transform operands) issues them
// BEFORE first(): the prologue then waits only for its own bytes and the
// weight stream stays in flight through the norm math.
struct Gemv1Geo {
  int NT, NW, lane, wave;
  int b0;            // first chunk of the workgroup's K range
  int n8, lds_ld;    // 8-element items staged per row; LDS row stride in elements
  bool fast;         // M * n8 <= GEMV1_Q * NT: the item form holds every item in registers (ss8's contract)
  bf16* xs;          // the staged rows
  float* part;       // LDS behind them: partial sums (XF_MIX: its conv rows, then the sums)
  float* inv_s;      // [16]
};
// One whole row in a wave's registers (lane l: items l, l + 64, ..): its sum of
// squares in the order the item form gives that row (ss8's contract), wave_sum,
// inverse RMS, and for a real row (store) the norm chain into its LDS row.
// (the uniform has_w / has_mod tests stay per element: hoisting them into
// specialised copies raised the kernel to 180 VGPRs, 3 -> 2 waves / SIMD)
template <int IPR, bool MOD>
DEV void rw_row_norm(const GemmArgs& a, const Gemv1Geo& g, const bf16x8* xv, const bf16x8* wv, const bf16x8* sc,
                     const bf16x8* sh, bool has_w, bool has_mod, bool store, bf16* xrow_l) {
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < IPR; ++i) {
    if (g.fast) ss += ss8(xv[i]);
    else ss = ss8_run(ss, xv[i]);
  }
  ss = wave_sum(ss);
  const float inv = rsqrtf(ss / (float)a.K + a.xf.eps);
  if (store) {
#pragma unroll
    for (int i = 0; i < IPR; ++i) {
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = norm_rt(xv[i][j], inv, has_w, wv[i][j], has_mod, sc[MOD ? i : 0][j], sh[MOD ? i : 0][j]);
      *(bf16x8*)(xrow_l + (g.lane + 64 * i) * 8) = o;
    }
  }
}
// RW = 1, row-per-wave norm: IPR items per lane per row x RPW rows per wave; MOD:
// adaLN operands possible (their registers reserved).  Loads (A, norm weight,
// adaLN shift / scale; all unconditional, clamped to valid rows, so no branch
// join waits on them), then the weight stream, then rw_row_norm per row.
template <int IPR, int RPW, bool MOD, class F>
DEV void gemv1_stage_rw(const GemmArgs& a, const Gemv1Geo& g, F first) {
  constexpr int QR = IPR * RPW;
  const int lane = g.lane, wave = g.wave;
  bf16x8 xv[QR], wv[QR], sh[MOD ? QR : 1], sc[MOD ? QR : 1];
  const bool has_w = a.xf.w != nullptr, has_mod = MOD && a.xf.mod != nullptr;
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int m = min(wave * RPW + r, a.M - 1);
    const bf16* xr = rm_bf(a.a, m);
    const bf16* wp = has_w ? a.xf.w : xr;
    const bf16* md = has_mod ? a.xf.mod + (long long)m * a.xf.mod_ld : xr;
    const int so = has_mod ? a.xf.shift_off : 0, co = has_mod ? a.xf.scale_off : 0;
#pragma unroll
    for (int i = 0; i < IPR; ++i) {
      const int k = (lane + 64 * i) * 8;
      xv[r * IPR + i] = *(const bf16x8*)(xr + k);
      wv[r * IPR + i] = *(const bf16x8*)(wp + k);
      if (has_mod) {
        sh[MOD ? r * IPR + i : 0] = *(const bf16x8*)(md + so + k);
        sc[MOD ? r * IPR + i : 0] = *(const bf16x8*)(md + co + k);
      }
    }
  }
  first();
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int m = wave * RPW + r;
    rw_row_norm<IPR, MOD>(a, g, xv + r * IPR, wv + r * IPR, sc + (MOD ? r * IPR : 0), sh + (MOD ? r * IPR : 0), has_w,
                          has_mod, m < a.M, g.xs + m * g.lds_ld);
  }
}
// RW = 2, K = 3,584 rows with adaLN operands (VibeVoice-Large head): the raw A row
// goes straight to its LDS row by 16-byte LDS DMA (lane l's item i lands at
// (l + 64 i) * 8, the row layout), so only the norm weight and shift / scale
// take registers; the row is read back by its own lanes after a counted vmcnt
// (the 21 operand loads and the U weight loads issued after it stay in flight).
// Then rw_row_norm, gemv1_stage_rw's row tail, the modulation unconditional.
template <int U, class F>
DEV void gemv1_stage_rw_dma(const GemmArgs& a, const Gemv1Geo& g, F first) {
  constexpr int IPR = 7;
  const int lane = g.lane, wave = g.wave;
  bf16x8 wv[IPR], sh[IPR], sc[IPR];
  const bool has_w = a.xf.w != nullptr;
  const int m = min(wave, a.M - 1);
  bf16* xrow_l = g.xs + m * g.lds_ld;
  if (wave < a.M) {
    const bf16* xr = rm_bf(a.a, m);
    const bf16* wp = has_w ? a.xf.w : xr;
    const bf16* md = a.xf.mod + (long long)m * a.xf.mod_ld;
#pragma unroll
    for (int i = 0; i < IPR; ++i)
      __builtin_amdgcn_global_load_lds((const void*)(xr + (lane + 64 * i) * 8),
                                       (__attribute__((address_space(3))) void*)(xrow_l + 64 * i * 8), 16, 0, 0);
    // the counted wait below needs exactly these loads younger than the DMA,
    // in this order: sched_barrier fences keep the scheduler from moving any
    // of them across
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < IPR; ++i) {
      const int k = (lane + 64 * i) * 8;
      wv[i] = *(const bf16x8*)(wp + k);
      sh[i] = *(const bf16x8*)(md + a.xf.shift_off + k);
      sc[i] = *(const bf16x8*)(md + a.xf.scale_off + k);
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  first();
  __builtin_amdgcn_sched_barrier(0);
  if (wave < a.M) {
    // the DMA is older than 3 * IPR operand loads and the weight loads
    constexpr int after = 3 * IPR + U;
    __builtin_amdgcn_s_waitcnt((after & 15) | ((after >> 4) << 14) | (7 << 4) | (15 << 8));
    bf16x8 xv[IPR];
#pragma unroll
    for (int i = 0; i < IPR; ++i) xv[i] = *(const bf16x8*)(xrow_l + (lane + 64 * i) * 8);
    rw_row_norm<IPR, true>(a, g, xv, wv, sc, sh, has_w, true, true, xrow_l);
  }
}
// XF_ATTN_MERGE: o_proj's A rows = the decode attention output, merged from the
// key splits' partials k_attn left (AttnArgs::defer, or its groups' partials): the
// attention kernel's own merge (attn_dev.h attn_merge_parts, so bit-identical),
// one round trip of partial loads here instead of a ticket + merge at the
// attention's tail.  Item (m, 8 dims of head hq).
template <class F>
DEV void gemv1_stage_merge(const GemmArgs& a, const Gemv1Geo& g, F first) {
  const int n8 = g.n8, nsp = a.xf.nsplit;
  // the weight stream first: the merge's two dependent round trips (query
  // length, then the partials) then overlap it instead of preceding it
  first();
#pragma unroll 1
  for (int e = threadIdx.x; e < a.M * n8; e += g.NT) {
    const int m = e / n8, k = (e - m * n8) * 8;
    const int hq = k >> 7, j0 = k & 127;
    const int np = attn_row_splits(a.xf.qpos[m] + 1, nsp, a.xf.chunk, 0).nact;
    const long long p0 = ((long long)m * (a.K >> 7) + hq) * nsp;
    float M, num[8], den;
    attn_merge_parts<8>(
        np,
        [&](int s, float& ms, float& ls, float(&os)[8]) __attribute__((always_inline)) {
          const float2 ml = *(const float2*)(a.xf.part_ml + (p0 + s) * 2);
          ms = ml.x;
          ls = ml.y;
          const f32x4 o0 = *(const f32x4*)(a.xf.part_o + (p0 + s) * 128 + j0);
          const f32x4 o1 = *(const f32x4*)(a.xf.part_o + (p0 + s) * 128 + j0 + 4);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            os[q] = o0[q];
            os[4 + q] = o1[q];
          }
        },
        M, num, den);
    bf16x8 o8;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) o8[jj] = tobf(num[jj] / den);
    *(bf16x8*)(g.xs + m * g.lds_ld + k) = o8;
  }
}
// XF_MIX: the codec Block1D front half for the M = ns * T rows (codec_dev.h's
// arithmetic, a row's chunk sums added in k_mix's order): every workgroup
// recomputes it (a few tens of KB of L2 reads next to its weight slice);
// workgroup 0 also stores the conv-buffer rows and y.  One dependent global
// round trip: operands, x rows and history rows are issued together ahead of
// the weight stream (the slot ids come through the scalar cache: sbase, read
// by the kernel before any store), the raw x rows stay in LDS (xs) and are
// overwritten by y, then by fc1's normalised input.
template <class F>
DEV void gemv1_stage_mix(const GemmArgs& a, const Gemv1Geo& g, long long sb0, long long sb1, long long sb2, long long sb3,
                         F first) {
  const long long sbase[4] = {sb0, sb1, sb2, sb3};   // by value: through a reference the selects below became a scratch array
  const int NT = g.NT, n8 = g.n8, lds_ld = g.lds_ld;
  bf16* xs = g.xs;
  float* inv_s = g.inv_s;
  const int C = a.K, T = a.xf.T, ctx = a.xf.ctx, ns = a.M / T;
  bf16* nrm = (bf16*)g.part;                               // [ns][ctx + T][C] conv input rows
  float* ssp = (float*)(nrm + (size_t)ns * (ctx + T) * C); // [M][n8] partial sums of squares
  const bool writer = blockIdx.x == 0;
  const int c2 = threadIdx.x % n8;                         // fixed: NT % n8 == 0
  bf16x8 wk[7], bb, gv, wf, wn;
#pragma unroll
  for (int k = 0; k < 7; ++k) wk[k] = *(const bf16x8*)(a.xf.dw_w + (size_t)c2 * 56 + k * 8);
  bb = *(const bf16x8*)(a.xf.dw_b + c2 * 8);
  gv = *(const bf16x8*)(a.xf.gamma + c2 * 8);
  wf = *(const bf16x8*)(a.xf.ffn_w + c2 * 8);
  wn = *(const bf16x8*)(a.xf.w + c2 * 8);
  // items [0, M*n8): x row m; [M*n8, (M + ns*ctx)*n8): history row h of sample s.
  // Every load is unconditional from an address chosen by selects (items past
  // the end re-read the last one): guarded loads, and rm_off's optional slot
  // lookup, compiled to a branch + s_waitcnt vmcnt(0) per item -- eight
  // serialized round trips per pass.  (x rows: host-checked plain map, no idx.)
  // Rows, not items: the n8 consecutive threads of a row share it, so thread t
  // takes rows t / n8 + j * (NT / n8) -- no per-item division (the item form
  // spent ~100 VALU per item on index math ahead of the weight stream).
  constexpr int CTX = 6;                                    // host-checked (k = 7)
  const int nrow = a.M + ns * CTX, rpt = NT / n8, rt = threadIdx.x / n8, nx = a.M * n8;
  const bf16* xbase = (const bf16*)a.a.base;
  for (int r0 = 0, it0 = 1; r0 < nrow; r0 += 8 * rpt, it0 = 0) {
    bf16x8 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int R = min(r0 + rt + q * rpt, nrow - 1);
      const int mx = min(R, a.M - 1), gx = mx / a.a.T;
      const bf16* px = xbase + gx * a.a.sB + (long long)(mx - gx * a.a.T) * a.a.sT;
      const int hr = max(R - a.M, 0), s_ = hr / CTX;
      long long sb = sbase[0];
#pragma unroll
      for (int q2 = 1; q2 < 4; ++q2) sb = s_ == q2 ? sbase[q2] : sb;
      const bf16* ph = a.xf.buf + sb + (long long)(hr - s_ * CTX) * C;
      v[q] = *(const bf16x8*)((R < a.M ? px : ph) + c2 * 8);
    }
    if (it0) first();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int R = r0 + rt + q * rpt;
      if (R < a.M) {
        *(bf16x8*)(xs + R * lds_ld + c2 * 8) = v[q];
        ssp[R * n8 + c2] = cb_ss8(v[q]);
      } else if (R < nrow) {
        const int hr = R - a.M, s_ = hr / CTX;
        *(bf16x8*)(nrm + ((size_t)s_ * (CTX + T) + (hr - s_ * CTX)) * C + c2 * 8) = v[q];
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  part_inv(ssp, n8, a.M, C, a.xf.eps, inv_s, g.wave, g.NW, g.lane);   // k_mix's row-sum order (64 lanes)
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  // mixer norm of the new rows -> conv input rows; workgroup 0 appends them to the buffer
  for (int e = threadIdx.x; e < nx; e += NT) {
    const int m = e / n8, s_ = m / T, t = m - s_ * T;
    const bf16x8 v = *(const bf16x8*)(xs + m * lds_ld + c2 * 8);
    const float rr = inv_s[m];
    bf16x8 o8;
#pragma unroll
    for (int j = 0; j < 8; ++j) o8[j] = cb_norm(v[j], rr, wn[j]);
    *(bf16x8*)(nrm + ((size_t)s_ * (ctx + T) + ctx + t) * C + c2 * 8) = o8;
    if (writer) {
      long long sb = sbase[0];
#pragma unroll
      for (int q2 = 1; q2 < 4; ++q2) sb = s_ == q2 ? sbase[q2] : sb;
      *(bf16x8*)(a.xf.buf + sb + (long long)(ctx + t) * C + c2 * 8) = o8;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  // depthwise conv + gamma residual: y over the raw x in xs (workgroup 0 stores y)
  for (int e = threadIdx.x; e < nx; e += NT) {
    const int m = e / n8, s_ = m / T, t = m - s_ * T;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 7; ++k)
      cb_conv8(acc, wk, *(const bf16x8*)(nrm + ((size_t)s_ * (ctx + T) + t + k) * C + c2 * 8), k);
    bf16x8* px = (bf16x8*)(xs + m * lds_ld + c2 * 8);
    const bf16x8 xv = *px;
    bf16x8 y8;
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      y8[j] = cb_y(xv[j], acc[j], bb[j], gv[j]);
      ss += bf(y8[j]) * bf(y8[j]);
    }
    if (writer) *(bf16x8*)(a.xf.y + (long long)m * C + c2 * 8) = y8;
    *px = y8;
    ssp[e] = ss;
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  part_inv(ssp, n8, a.M, C, a.xf.eps, inv_s, g.wave, g.NW, g.lane);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  for (int e = threadIdx.x; e < nx; e += NT) {             // FFN pre-norm, in place
    const int m = e / n8;
    bf16x8* px = (bf16x8*)(xs + m * lds_ld + c2 * 8);
    const bf16x8 y8 = *px;
    const float rr = inv_s[m];
    bf16x8 o8;
#pragma unroll
    for (int j = 0; j < 8; ++j) o8[j] = cb_norm(y8[j], rr, wf[j]);
    *px = o8;
  }
}
// The item-per-thread "fast" form (g.fast): every item (row m, 8 columns) of
// the block in one batch of GEMV1_Q registers per thread.  Every A-side load is
// unconditional (items past the end re-read the last; absent operands re-read
// the row) and, for a plain row map, has no slot lookup: a guarded load
// compiled to a branch + s_waitcnt vmcnt(0) at its join, so each item waited
// for the one before it and the weight stream behind them was issued several
// round trips late.
template <int XF, class F>
DEV void gemv1_stage_fast(const GemmArgs& a, const Gemv1Geo& g, F first) {
  constexpr int Q = GEMV1_Q;
  const int NT = g.NT, n8 = g.n8, b0 = g.b0;
  bf16x8 xv[Q], wv[Q], sh[Q], sc[Q];
  const int ne = a.M * n8;
  const bool has_w = XF == XF_NORM ? a.xf.w != nullptr : XF == XF_SILU_ADD;
  const bool has_mod = XF == XF_NORM && a.xf.mod != nullptr;
  auto fast_loads = [&](auto plain_c) {
    constexpr bool PLAIN = decltype(plain_c)::value;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int e = min(threadIdx.x + q * NT, ne - 1);
      const int m = e / n8, k = b0 * 32 + (e - m * n8) * 8;
      const bf16* xr = PLAIN ? rm_bf_plain(a.a, m) : rm_bf(a.a, m);
      xv[q] = *(const bf16x8*)(xr + k);
      if (XF == XF_NORM || XF == XF_SILU_ADD) {
        const bf16* wp = has_w ? (XF == XF_NORM ? a.xf.w : a.xf.vec) : xr;
        wv[q] = *(const bf16x8*)(wp + k);
      }
      if (XF == XF_NORM) {
        const bf16* md = has_mod ? a.xf.mod + (long long)m * a.xf.mod_ld : xr;
        sh[q] = *(const bf16x8*)(md + (has_mod ? a.xf.shift_off : 0) + k);
        sc[q] = *(const bf16x8*)(md + (has_mod ? a.xf.scale_off : 0) + k);
      }
    }
  };
  if (a.a.idx) fast_loads(std::false_type());
  else fast_loads(std::true_type());
  first();
  if (XF == XF_NORM) {
    // per-item sums of squares -> LDS, rows reduced in a fixed order
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int e = threadIdx.x + q * NT;
      if (e < a.M * n8) g.part[e] = ss8(xv[q]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (a.ksplit == 1) part_inv(g.part, n8, a.M, a.K, a.xf.eps, g.inv_s, g.wave, g.NW, g.lane);
    else row_inv(a, 0, a.M, g.inv_s, g.wave, g.NW, g.lane);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int e = threadIdx.x + q * NT;
    if (e < a.M * n8) {
      const int m = e / n8, k8 = (e - m * n8) * 8;
      bf16x8 o = xv[q];
      if (XF == XF_NORM) {
        const float inv = g.inv_s[m];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          o[j] = norm_rt(xv[q][j], inv, a.xf.w != nullptr, wv[q][j], a.xf.mod != nullptr, sc[q][j], sh[q][j]);
      } else if (XF == XF_SILU_ADD) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = tobf(silu_f(rb(bf(xv[q][j]) + bf(wv[q][j]))));
      }
      *(bf16x8*)(g.xs + m * g.lds_ld + k8) = o;
    }
  }
}
// The many-rows "staged" form (B >= 8 batches): weights first, then the A rows
// through registers to LDS in batches of 4 items per thread; the transform runs
// on the LDS rows (a row's sum of squares: ss8_run over its lanes' items).
template <int XF, class F>
DEV void gemv1_stage_rows(const GemmArgs& a, const Gemv1Geo& g, F first) {
  const int NT = g.NT, NW = g.NW, lane = g.lane, wave = g.wave, n8 = g.n8, lds_ld = g.lds_ld, b0 = g.b0;
  bf16* xs = g.xs;
  float* inv_s = g.inv_s;
  first();
  const int ne = a.M * n8;
  const bool plain = !a.a.idx;
  for (int e0 = threadIdx.x; e0 < ne; e0 += 4 * NT) {
    bf16x8 xv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {   // unconditional loads (see the fast form)
      const int e = min(e0 + q * NT, ne - 1);
      const int m = e / n8, k8 = (e - m * n8) * 8;
      xv[q] = *(const bf16x8*)((plain ? rm_bf_plain(a.a, m) : rm_bf(a.a, m)) + b0 * 32 + k8);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = e0 + q * NT;
      if (e < a.M * n8) {
        const int m = e / n8, k8 = (e - m * n8) * 8;
        *(bf16x8*)(xs + m * lds_ld + k8) = xv[q];
      }
    }
  }
  if (XF != XF_NONE) {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (XF == XF_NORM) {
      if (a.ksplit == 1) {
        for (int m = wave; m < a.M; m += NW) {
          float ss = 0.f;
          for (int c = lane; c < n8; c += 64) ss = ss8_run(ss, *(const bf16x8*)(xs + m * lds_ld + c * 8));
          ss = wave_sum(ss);
          if (lane == 0) inv_s[m] = rsqrtf(ss / (float)a.K + a.xf.eps);
        }
      } else {
        row_inv(a, 0, a.M, inv_s, wave, NW, lane);
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    for (int e = threadIdx.x; e < a.M * n8; e += NT) {
      const int m = e / n8, k8 = (e - m * n8) * 8;
      bf16x8* px = (bf16x8*)(xs + m * lds_ld + k8);
      *px = xform<XF>(a, *px, m, b0 * 32 + k8, XF == XF_NORM ? inv_s[m] : 0.f);
    }
  }
}

// k_gemv1: geometry; stage A while the first weight batch is in flight; barrier;
// stream; reduce; epilogue.
template <int U, int XF, bool KEEP = false, int TPW = 1, int RW = 0>
__global__ void __launch_bounds__(64 * gemv1_max_waves(TPW)) k_gemv1(GemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float inv_s[16];
  __shared__ float red[gemv1_max_waves(TPW) * 256];
  __shared__ unsigned last_flag;
  const int NT = blockDim.x, NW = NT >> 6;   // first: a scalar load (see part_of)
  // XF_MIX: the (<= 4) samples' conv-buffer slot bases, read before any store
  // so they are scalar loads issued together (as guarded per-slot vector loads
  // each took a round trip of its own)
  long long sbase[4] = {0, 0, 0, 0};
  if constexpr (XF == XF_MIX) {
    const int nsl = a.M / a.xf.T;
#pragma unroll
    for (int q = 0; q < 4; ++q) sbase[q] = (long long)a.xf.slots[min(q, nsl - 1)] * a.xf.buf_sB;
  }
  stamp(a, 0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  // The workgroup owns TPW consecutive 16-row weight tiles and stages the A
  // rows once for all of them (at M = 16 one tile per workgroup re-read the
  // whole A block per 16 weight rows: as many L2 bytes as weight bytes, and the
  // LDS it needed capped residency at 2 workgroups per CU).  Waves are
  // tile-major: wave = tile_in_group * KW + k-slice.
  const int KW = TPW == 1 ? NW : NW / TPW;
  const int tw = TPW == 1 ? 0 : wave / KW, kwv = TPW == 1 ? wave : wave - tw * KW;
  const int ntile = a.N >> 4;
  // tiles [T0, T0 + ntl) of this workgroup: an even share of the grid's (<= TPW
  // each; = TPW * blockIdx.x .. when the grid is ntile / TPW workgroups)
  const int T0 = TPW == 1 ? blockIdx.x : part_of(ntile, blockIdx.x, gridDim.x);
  const int ntl = TPW == 1 ? 1 : part_of(ntile, blockIdx.x + 1, gridDim.x) - T0;
  const int tile = T0 + tw;
  const bool tile_ok = TPW == 1 || tw < ntl;
  // this workgroup's chunk range [b0, b1), then the wave's [c0, c1)
  const KRange kr = k_range(a.K >> 5, a.ksplit, kwv, KW);
  const int b0 = kr.b0, b1 = kr.b1, c0 = kr.c0, c1 = tile_ok ? kr.c1 : c0;
  // MFMA-packed W (a wave past the last tile streams nothing; its clamped
  // prologue loads read tile 0)
  const bf16* wrow = a.w + (long long)(tile_ok ? tile : 0) * a.K * 16 + lane * 8;
  const bf16x8 zero8 = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 wa[U], wb[U];
  auto load = [&](bf16x8 (&wf)[U], int c) {
#pragma unroll
    for (int u = 0; u < U; ++u) wf[u] = ldw<KEEP>(wrow + min(c + u, max(c1 - 1, 0)) * 512);
  };
  auto first = [&]() { load(wa, c0); };

  // ---- A staging (the gemv1_stage_* forms above), the first weight batch issued inside it
  const int kw = (b1 - b0) * 32;         // elements staged per row
  Gemv1Geo geo;
  geo.NT = NT, geo.NW = NW, geo.lane = lane, geo.wave = wave, geo.b0 = b0;
  geo.n8 = kw >> 3, geo.lds_ld = kw + 8;
  geo.fast = a.M * geo.n8 <= GEMV1_Q * NT;
  geo.xs = (bf16*)smem;
  geo.part = (float*)(smem + (((size_t)a.M * geo.lds_ld * 2 + 15) & ~(size_t)15));
  geo.inv_s = inv_s;
  const int lds_ld = geo.lds_ld;
  const bf16* xs = geo.xs;
  if constexpr (RW == 2) {   // its own instantiation: its registers would cost the others occupancy
    gemv1_stage_rw_dma<U>(a, geo, first);
  } else if constexpr (RW == 1) {
    // items per lane per row x rows per wave (the host picks RW for eligible shapes, gemm_decide)
    const int ipr = geo.n8 >> 6, rpw = (a.M + NW - 1) / NW;
    if (ipr == 3 && rpw == 1) gemv1_stage_rw<3, 1, true>(a, geo, first);
    else if (ipr == 3) gemv1_stage_rw<3, 2, true>(a, geo, first);
    else gemv1_stage_rw<7, 1, false>(a, geo, first);
  } else if constexpr (XF == XF_ATTN_MERGE) {
    gemv1_stage_merge(a, geo, first);
  } else if constexpr (XF == XF_MIX) {
    gemv1_stage_mix(a, geo, sbase[0], sbase[1], sbase[2], sbase[3], first);
  } else if (geo.fast) {
    gemv1_stage_fast<XF>(a, geo, first);
  } else {
    gemv1_stage_rows<XF>(a, geo, first);
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  stamp(a, 1);

  f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
  // A fragment reads are unconditional (a guarded LDS read compiled to an
  // exec-masked ds_read + lgkmcnt(0) per chunk): lanes of rows >= M read row
  // M - 1 -- they only feed output columns the epilogue drops -- and chunks past
  // the wave's range re-read its last chunk against a zeroed weight fragment
  const bf16* xrow = xs + min(r, a.M - 1) * lds_ld + 8 * g - b0 * 32;
  auto compute = [&](bf16x8 (&wf)[U], int c) {
    bf16x8 x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = *(const bf16x8*)(xrow + min(c + u, c1 - 1) * 32);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bf16x8 w = c + u < c1 ? wf[u] : zero8;
      acc = mfma(w, x[u], acc);
    }
  };
  for (int c = c0; c < c1; c += 2 * U) {
    load(wb, c + U);
    compute(wa, c);
    load(wa, c + 2 * U);
    compute(wb, c + U);
  }
  stamp(a, 2);

  // ---- reduce each tile's K-slice waves (tile t's sum lands in slab t * KW)
#pragma unroll
  for (int i = 0; i < 4; ++i) red[(wave * 4 + i) * 64 + lane] = acc[i];
  __syncthreads();
  slices_sum<TPW, 256>(red, KW, NT);
  if (a.ksplit > 1 && !splitk_handoff(a, red, 256, &last_flag, NT)) return;   // host: ksplit > 1 => TPW == 1
  if (wave < TPW && (TPW == 1 || wave < ntl)) {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = red[wave * KW * 256 + i * 64 + lane];
    epi_tile(a, r, (T0 + wave) * 16, lane, v);
    if (a.stamps) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      stamp(a, 3);
    }
  }
}

// 16 < M <= 64: A fragments loaded straight from global / L2, transform per
// chunk; weights ping-ponged as in k_gemv1.
// W8 (all three tiled families below): the weight operand is GemmArgs::w8 / w8e
// (e4m3 codes in mfma_pack8 order + one exponent per weight row, gemv_w8.hip).
// Only the weight-fragment loads differ: a lane loads its code bytes and
// converts them in registers to code * 2^e[n] (cvt8s) -- the bf16 values
// k_dequant_w8 would have stored -- ahead of the same MFMA sequence: chunk order,
// wave / K-split partition, reductions and epilogue are the bf16 instantiation's,
// so the result is that kernel's on the dequantised matrix, bit for bit.
template <int MREP, int U, int XF, bool W8 = false>
__global__ void __launch_bounds__(512) k_gemv(GemmArgs a) {
  __shared__ float red[8 * MREP * 256];
  __shared__ float inv_s[64];
  __shared__ unsigned last_flag;
  const int NT = blockDim.x, NW = NT >> 6;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const KRange kr = k_range(a.K >> 5, a.ksplit, wave, NW);
  const int c0 = kr.c0, c1 = kr.c1;
  const bf16* wrow = a.w + (long long)(n0 >> 4) * a.K * 16 + lane * 8;  // MFMA-packed W
  const unsigned char* wrow8 = a.w8 + (long long)(n0 >> 4) * a.K * 16 + lane * 16;   // W8: its codes
  const float wsc = W8 ? w8_scale(a.w8e[n0 + r]) : 0.f;
  using WF = std::conditional_t<W8, u32x2, bf16x8>;   // one chunk's weight fragment as loaded
  const bf16x8 zero8 = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
  if (XF == XF_NORM) {
    row_inv(a, 0, 16 * MREP, inv_s, wave, NW, lane);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  const bf16* xrow[MREP];
  bool xok[MREP];
  float inv[MREP];
#pragma unroll
  for (int mr = 0; mr < MREP; ++mr) {
    const int m = r + 16 * mr;
    xok[mr] = m < a.M;
    xrow[mr] = rm_bf(a.a, min(m, a.M - 1)) + 8 * g;   // rows >= M: a valid row, results dropped
    inv[mr] = XF == XF_NORM ? inv_s[m] : 0.f;
  }
  f32x4 acc[MREP];
#pragma unroll
  for (int mr = 0; mr < MREP; ++mr) acc[mr] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // each chunk's A fragments travel with its weight chunk (vmcnt waits are in
  // issue order: loading A inside compute would wait for the next batch too)
  WF wa[U], wb[U];
  bf16x8 xa[U][MREP], xb[U][MREP];
  // (odd_c, W8 only: the wave's range starts on an odd chunk, ldw8_chunks)
  auto load = [&](WF (&wf)[U], bf16x8 (&xf)[U][MREP], int c, auto odd_c) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int cc = min(c + u, max(c1 - 1, 0));
#pragma unroll
      for (int mr = 0; mr < MREP; ++mr) xf[u][mr] = *(const bf16x8*)(xrow[mr] + cc * 32);
      if constexpr (!W8) wf[u] = ldw(wrow + cc * 512);
    }
    if constexpr (W8) ldw8_chunks<U, decltype(odd_c)::value>(wf, wrow8, c, max(c1 - 1, 0));
  };
  auto compute = [&](WF (&wf)[U], bf16x8 (&xf)[U][MREP], int c) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = c + u < c1;
      const int cc = min(c + u, max(c1 - 1, 0));
      bf16x8 w;
      if constexpr (W8) w = ok ? cvt8s(wf[u][0], wf[u][1], wsc) : zero8;
      else w = ok ? wf[u] : zero8;
#pragma unroll
      for (int mr = 0; mr < MREP; ++mr) {
        bf16x8 x = (xok[mr] && ok) ? xf[u][mr] : zero8;
        if (XF != XF_NONE && xok[mr] && ok) x = xform<XF>(a, x, r + 16 * mr, cc * 32 + 8 * g, inv[mr]);
        acc[mr] = mfma(w, x, acc[mr]);
      }
    }
  };
  auto stream = [&](auto odd_c) __attribute__((always_inline)) {
    load(wa, xa, c0, odd_c);
    for (int c = c0; c < c1; c += 2 * U) {
      load(wb, xb, c + U, odd_c);
      compute(wa, xa, c);
      load(wa, xa, c + 2 * U, odd_c);
      compute(wb, xb, c + U);
    }
  };
  // W8: one copy of the loop per parity (wave-uniform) -- a parity test inside
  // it would put the weight loads behind a branch -- each inlined like the one
  // bf16 copy (out of line, the fragment arrays would live in scratch)
  if constexpr (W8) {
    if (c0 & 1) stream(std::true_type());
    else stream(std::false_type());
  } else {
    stream(std::false_type());
  }
  const int TILE = MREP * 256;
#pragma unroll
  for (int mr = 0; mr < MREP; ++mr)
#pragma unroll
    for (int i = 0; i < 4; ++i) red[(wave * MREP * 4 + mr * 4 + i) * 64 + lane] = acc[mr][i];
  __syncthreads();
  slices_sum<1, TILE>(red, NW, NT);
  if (a.ksplit > 1 && !splitk_handoff(a, red, TILE, &last_flag, NT)) return;
  for (int mr = wave; mr < MREP; mr += NW) {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = red[(mr * 4 + i) * 64 + lane];
    epi_tile(a, r + 16 * mr, n0, lane, v);
  }
}

// 16 < M <= 64 with many weight tiles (B >= 9 decode rows, the batched head
// adaLN, 64-row codec stages).  k_gemv re-reads the A fragments from L2 for
// every 16 weight rows -- at M = 64 four times the weight bytes (B = 32: LM
// gate|up 51 us for 55 MB).  Here each of the 8 waves holds the A fragments of
// its K slice (GW_NCH chunks per K block) in registers and applies them to the
// workgroup's TPW weight tiles, streaming those tiles' chunks of the slice with
// a ping-pong over tiles; the 8 slices reduce in LDS per tile, in wave order,
// before the epilogue.  A crosses L2 once per workgroup.
constexpr int GW_NCH = 6;   // 32-column chunks per wave per K block (8 waves: 1,536 columns)

template <int MREP, int TPW, bool KEEP, bool W8 = false>
__global__ void __launch_bounds__(512) k_gemvw(GemmArgs a) {
  __shared__ float red[8][MREP * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int ntile = a.N >> 4, nchunk = a.K >> 5;
  const int t0 = blockIdx.x * TPW;
  const bf16x8 zero8 = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
  f32x4 acc[TPW][MREP];
#pragma unroll
  for (int i = 0; i < TPW; ++i)
#pragma unroll
    for (int mr = 0; mr < MREP; ++mr) acc[i][mr] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // rows >= M read row M - 1 (their output columns are dropped): no guarded loads
  const bf16* arow[MREP];
#pragma unroll
  for (int mr = 0; mr < MREP; ++mr) arow[mr] = rm_bf(a.a, min(16 * mr + r, a.M - 1)) + 8 * g;
  // W8: a wave's GW_NCH chunks of a tile are GW_NCH / 2 whole chunk pairs (its
  // first chunk is even and K % 64 == 0), 16 bytes per lane each
  using WB = std::conditional_t<W8, u32x4[GW_NCH / 2], bf16x8[GW_NCH]>;
  float wsc[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) wsc[i] = W8 ? w8_scale(a.w8e[min(t0 + i, ntile - 1) * 16 + r]) : 0.f;
  for (int kb = 0; kb < nchunk; kb += 8 * GW_NCH) {
    const int cw = kb + wave * GW_NCH;        // this wave's first chunk of the block (wave-uniform)
    if (cw >= nchunk) continue;
    bf16x8 xf[GW_NCH][MREP];
#pragma unroll
    for (int c = 0; c < GW_NCH; ++c)
#pragma unroll
      for (int mr = 0; mr < MREP; ++mr) xf[c][mr] = *(const bf16x8*)(arow[mr] + min(cw + c, nchunk - 1) * 32);
    WB wa, wb;
    auto wload = [&](WB& w, int i) {
      const int t = min(t0 + i, ntile - 1);
      if constexpr (W8) {
        const unsigned char* wr = a.w8 + (long long)t * a.K * 16 + lane * 16;
#pragma unroll
        for (int p = 0; p < GW_NCH / 2; ++p) w[p] = ldw8<KEEP>(wr + (long long)(min(cw + 2 * p, nchunk - 1) >> 1) * 1024);
      } else {
        const bf16* wr = a.w + (long long)t * a.K * 16 + lane * 8;
#pragma unroll
        for (int c = 0; c < GW_NCH; ++c) w[c] = ldw<KEEP>(wr + min(cw + c, nchunk - 1) * 512);
      }
    };
    auto mac = [&](WB& w, int i) {
#pragma unroll
      for (int c = 0; c < GW_NCH; ++c) {
        bf16x8 wc;   // chunks past K: zero weights
        if constexpr (W8) wc = cw + c < nchunk ? cvt8s(w[c >> 1][2 * (c & 1)], w[c >> 1][2 * (c & 1) + 1], wsc[i]) : zero8;
        else wc = cw + c < nchunk ? w[c] : zero8;
#pragma unroll
        for (int mr = 0; mr < MREP; ++mr) acc[i][mr] = mfma(wc, xf[c][mr], acc[i][mr]);
      }
    };
    wload(wa, 0);
#pragma unroll
    for (int i = 0; i < TPW; i += 2) {
      if (i + 1 < TPW) wload(wb, i + 1);
      mac(wa, i);
      if (i + 2 < TPW) wload(wa, i + 2);
      if (i + 1 < TPW) mac(wb, i + 1);
    }
  }
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
#pragma unroll
    for (int mr = 0; mr < MREP; ++mr)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[wave][mr * 256 + j * 64 + lane] = acc[i][mr][j];
    __syncthreads();
    for (int e = threadIdx.x; e < MREP * 256; e += 512) {
      float sum = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) sum += red[w][e];
      red[0][e] = sum;
    }
    __syncthreads();
    const int t = t0 + i;
    if (t < ntile) {
      for (int mr = wave; mr < MREP; mr += 8) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = red[0][mr * 256 + j * 64 + lane];
        epi_tile(a, 16 * mr + r, t * 16, lane, v);
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ tiled GEMM (M > 64)
template <int BN, int XF, bool W8 = false>
__global__ void __launch_bounds__(256) k_gemm(GemmArgs a) {
  constexpr int NT = BN / 32;  // 16-wide n tiles per wave (wave covers BN/2 columns)
  __shared__ float inv_s[64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int m_blk = blockIdx.x * 64;
  const int m_base = m_blk + wm * 32;
  const int n_base = blockIdx.y * BN + wn * (BN / 2);
  if (XF == XF_NORM) {
    row_inv(a, m_blk, 64, inv_s, wave, 4, lane);
    __syncthreads();
  }
  const bf16* wrow[NT];
  const unsigned char* wrow8[NT];   // W8: the codes, and each weight row's scale
  float wsc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    wrow[nt] = a.w + (long long)((n_base >> 4) + nt) * a.K * 16 + lane * 8;
    wrow8[nt] = a.w8 + (long long)((n_base >> 4) + nt) * a.K * 16 + lane * 16;
    wsc[nt] = W8 ? w8_scale(a.w8e[n_base + nt * 16 + r]) : 0.f;
  }
  // rows past M read row M - 1 (unconditional loads: a guarded load compiles to a
  // branch + a vmcnt(0) wait); their products land in rows the epilogue drops
  const bf16* xrow[2];
  bool xok[2];
  float inv[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int m = m_base + mt * 16 + r;
    xok[mt] = m < a.M;
    xrow[mt] = rm_bf(a.a, min(m, a.M - 1)) + 8 * g;
    inv[mt] = XF == XF_NORM ? inv_s[min(m, a.M - 1) - m_blk] : 0.f;
  }
  f32x4 acc[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const bf16x8 zero8 = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
  const int nk = a.K >> 5;
  // two register sets of 2 chunks each: the loads of chunks c + 4 .. go out while
  // chunks c .. compute (one set in flight per round trip left the loop
  // latency-bound: the 320-row codec fc2 at C = 512, K 2,048, took 24 us)
  // W8: a set's 2 chunks are one chunk pair (c even, K % 64 == 0: never past K), 16 code bytes per lane
  using WS = std::conditional_t<W8, u32x4[1][NT], bf16x8[2][NT]>;
  WS wfA, wfB;
  bf16x8 xfA[2][2], xfB[2][2];
  auto load = [&](int c, WS& wf, bf16x8 (&xf)[2][2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int cc = min(c + u, nk - 1);
      if constexpr (!W8) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wf[u][nt] = *(const bf16x8*)(wrow[nt] + cc * 512);   // re-read across row tiles: default policy
      } else if (u == 0) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wf[0][nt] = ldw8<true>(wrow8[nt] + (long long)(cc >> 1) * 1024);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) xf[u][mt] = *(const bf16x8*)(xrow[mt] + cc * 32);
    }
  };
  auto comp = [&](int c, WS& wf, bf16x8 (&xf)[2][2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      bf16x8 wv[W8 ? NT : 1];   // W8: this chunk's fragments, converted once for both row tiles
      if constexpr (W8) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wv[nt] = cvt8s(wf[0][nt][2 * u], wf[0][nt][2 * u + 1], wsc[nt]);
      } else if (c + u >= nk) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wf[u][nt] = zero8;
      }
      if (XF != XF_NONE) {
        const int k = min(c + u, nk - 1) * 32 + 8 * g;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
          if (xok[mt]) xf[u][mt] = xform<XF>(a, xf[u][mt], m_base + mt * 16 + r, k, inv[mt]);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          if constexpr (W8) acc[mt][nt] = mfma(wv[nt], xf[u][mt], acc[mt][nt]);
          else acc[mt][nt] = mfma(wf[u][nt], xf[u][mt], acc[mt][nt]);
        }
    }
  };
  load(0, wfA, xfA);
  if (2 < nk) load(2, wfB, xfB);
  for (int c = 0; c < nk; c += 4) {
    comp(c, wfA, xfA);
    if (c + 4 < nk) load(c + 4, wfA, xfA);
    if (c + 2 < nk) {
      comp(c + 2, wfB, xfB);
      if (c + 6 < nk) load(c + 6, wfB, xfB);
    }
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      float v[4] = {acc[mt][nt][0], acc[mt][nt][1], acc[mt][nt][2], acc[mt][nt][3]};
      epi_tile(a, m_base + mt * 16 + r, n_base + nt * 16, lane, v);
    }
}

// ------------------------------------------------------------------ LDS-staged GEMM (prefill-sized M)
// M >= GEMM_BIG_M rows (a prompt's prefill: thousands of tokens through every
// projection).  k_gemm's operands come straight from L2
// per wave (4 fragments per 4 MFMAs); here a 128 x 128 tile of 4 waves (each
// 64 x 64: 4 weight tiles x 4 row tiles, 16 accumulators) stages each 64-deep
// K step in LDS with 16-byte global_load_lds: the packed weight blocks are
// already 1 KB MFMA fragments (one wave instruction each), and the A rows are
// gathered per lane into the same fragment order (lane l <- row l & 15,
// k 8(l >> 4)), so every LDS read is a conflict-free lane-linear ds_read_b128.
// One __shared__ array (a second LDS object makes hipcc wait vmcnt(0) early,
// cdna_hip_programming.md §5 trap 4a), two barriers per K step, ~3 workgroups
// per CU overlap each other's staging.  Workgroups are remapped XCD-major so
// each XCD's L2 holds a compact block of (row tile, weight tile) pairs.
constexpr int GB_M = 128, GB_N = 128, GB_K = 64;
constexpr int GEMM_BIG_M = 256;
constexpr int GEMM_BIG_TILES = 256;

template <int NS>
__global__ void __launch_bounds__(256) k_gemm_big(GemmArgs a) {
  constexpr int STAGE = 2 * 16 * 512;   // [W blocks 16][A blocks 16] x 1 KB
  __shared__ __attribute__((aligned(16))) bf16 sm[NS * STAGE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int ntm = (a.M + GB_M - 1) / GB_M, ntn = a.N / GB_N, total = ntm * ntn;
  // XCD-major remap: consecutive ids go round-robin over the 8 XCDs; give XCD x
  // the contiguous range [x * per, (x + 1) * per) of tiles
  const int per = (total + 7) >> 3;
  const int t = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  if (t >= total) return;
  // grouped order inside the range: 4 row tiles sweep the weight tiles together
  constexpr int GM = 4;
  const int grp = t / (GM * ntn), gm = min(GM, ntm - grp * GM), tin = t - grp * GM * ntn;
  const int tm = grp * GM + tin % gm, tn = tin / gm;
  const int nchunk = a.K >> 5, nks = a.K >> 6;
  // staging: wave w fills W blocks 4w..4w+3 and A blocks 4w..4w+3 (block j = (tile j >> 1, chunk j & 1))
  const bf16* wsrc[4];
  const bf16* asrc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = 4 * wave + i;
    wsrc[i] = a.w + ((long long)(tn * 8 + (j >> 1)) * nchunk + (j & 1)) * 512 + lane * 8;
    const int m = min(tm * GB_M + (j >> 1) * 16 + r, a.M - 1);
    asrc[i] = rm_bf(a.a, m) + (j & 1) * 32 + 8 * g;
  }
  auto issue = [&](int ks) {
    bf16* st = sm + (ks % NS) * STAGE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 4 * wave + i;
      __builtin_amdgcn_global_load_lds((const void*)(wsrc[i] + (long long)ks * 1024),
                                       (__attribute__((address_space(3))) void*)(st + j * 512), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const void*)(asrc[i] + ks * GB_K),
                                       (__attribute__((address_space(3))) void*)(st + 16 * 512 + j * 512), 16, 0, 0);
    }
  };
  f32x4 acc[4][4];   // [weight tile nt][row tile mt]
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (NS > 1) issue(0);
  for (int ks = 0; ks < nks; ++ks) {
    if (NS == 1) {
      issue(ks);
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    } else if (ks + 1 < nks) {
      // step ks + 1 streams into the other stage (released by the previous
      // step's closing barrier) while this one computes; raw barriers so the
      // prefetch stays in flight (cdna_hip_programming.md "Pipelining across barriers")
      issue(ks + 1);
      asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }
    const bf16* wl = sm + (ks % NS) * STAGE;
    const bf16* al = wl + 16 * 512;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      bf16x8 wf[4], xf[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) wf[nt] = *(const bf16x8*)(wl + ((wn * 4 + nt) * 2 + c) * 512 + lane * 8);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) xf[mt] = *(const bf16x8*)(al + ((wm * 4 + mt) * 2 + c) * 512 + lane * 8);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[nt][mt] = mfma(wf[nt], xf[mt], acc[nt][mt]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  // epilogue: one epi_tile body in a rolled loop, the accumulators rotated
  // through acc[0][0] (16 unrolled copies of epi_tile's RoPE / DPM forms
  // spilled the accumulators to scratch)
#pragma unroll 1
  for (int i = 0; i < 16; ++i) {
    float v[4] = {acc[0][0][0], acc[0][0][1], acc[0][0][2], acc[0][0][3]};
    epi_tile(a, tm * GB_M + (wm * 4 + (i & 3)) * 16 + r, tn * GB_N + (wn * 4 + (i >> 2)) * 16, lane, v);
#pragma unroll
    for (int k = 0; k < 15; ++k) acc[k >> 2][k & 3] = acc[(k + 1) >> 2][(k + 1) & 3];
  }
}

// ------------------------------------------------------------------ 256 x 256 tile (prefill, large batches)
// cdna_hip_programming.md §5: the 128² two-barrier structure (k_gemm_big) tops
// out near 900 TF; a 256 x 256 tile at one 8-wave workgroup per CU halves the
// operand bytes per FLOP and keeps a 3-stage-deep LDS-DMA ring in flight across
// raw barriers.  Here:
//   * 8 waves as 2 (rows m) x 4 (weight rows n): wave (wr, wc) owns 128 m x 64 n
//     = 8 x 4 accumulator tiles (128 VGPRs);
//   * K in 32-wide stages, a ring of 4 stages in LDS (4 x 32 KB: 16 A + 16 W one-KB
//     fragment blocks).  Step s computes stage s from registers while the wave
//     reads stage s + 1's fragments into its second register set; stage s + 4 is
//     issued into stage s's buffer right after the barrier that ends every wave's
//     reads of it, so three stages are in flight; each step waits with a counted
//     vmcnt (never 0 in the loop) and ONE raw s_barrier (a __syncthreads() would
//     drain the ring);
//   * the packed weight blocks are MFMA fragments already (one 1 KB glds per wave
//     instruction, lane-linear) and A rows are gathered per lane into the same
//     order, so every ds_read_b128 is lane-linear and conflict-free (no swizzle);
//   * one __shared__ array (a second LDS object makes hipcc drain vmcnt(0) before
//     every k-step, §5 item 4a); loads hand-interleaved between the MFMAs.
// K order of accumulation per output is k_gemm's (chunk by chunk): bit-identical.
// s_waitcnt immediates (gfx9 encoding: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] |
// vmcnt[5:4] << 14; a field at its maximum does not wait).  The builtin, unlike an
// asm wait, is seen by hipcc's waitcnt pass, which then does not re-wait (with
// lgkmcnt(0)) for fragments this wait already retired
constexpr unsigned WC_VM12 = 0x0F7C, WC_VM8_LGKM0 = 0x0078, WC_LGKM0 = 0xC07F, WC_VM0 = 0x0F70;
// (Measured and rejected, DESIGN.md "Prefill": the wave tile on
// v_mfma_f32_32x32x16_bf16 -- 0.305 vs 0.443 of peak on gate|up -- and the
// ablation builds that located the ceiling; neither is built any more.)
constexpr int GX_M = 256, GX_N = 256, GX_NS = 4;
// fewest 256 x 256 tiles that take k_gemm_xl: 3/4 of the 256 CUs.  One round of
// 192 tiles (the diffusion head's down projection at M = 8,192: 32 x 6) runs
// at the per-tile rate of k_gemm_xl's multi-round launches (~1,000 TF/s at
// 384 tiles, DESIGN.md "MFMA utilisation") where k_gemm_big's 768 128² tiles
// reached 665 TF/s
constexpr int GX_MIN_TILES = 192;
constexpr int GX_STAGE = 32 * 512;                       // elements per stage
constexpr size_t GX_LDS = (size_t)GX_NS * GX_STAGE * 2;   // 128 KB

__global__ void __launch_bounds__(512) k_gemm_xl(GemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) bf16 smx[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // scalar: the glds LDS bases (M0) too
  const int r = lane & 15, g = lane >> 4;
  const int wr = wave >> 2, wc = wave & 3;
  const int ntm = (a.M + GX_M - 1) / GX_M, ntn = a.N / GX_N, total = ntm * ntn;
  // XCD-major remap (bijective for any total), then groups of 4 row tiles sweep the weight tiles
  const int nb = gridDim.x, xcd = (int)(blockIdx.x & 7), q8 = nb >> 3, r8 = nb & 7;
  const int t = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (int)(blockIdx.x >> 3);
  if (t >= total) return;
  constexpr int GM = 4;
  const int grp = t / (GM * ntn), gm = min(GM, ntm - grp * GM), tin = t - grp * GM * ntn;
  const int tm = grp * GM + tin % gm, tn = tin / gm;
  const int nch = a.K >> 5;
  // staging: wave w fills A blocks 2w, 2w + 1 (row tiles) and W blocks 2w, 2w + 1 (weight tiles)
  const bf16* asrc[2];
  const bf16* wsrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int j = 2 * wave + i;
    if (a.apack) {   // packed rows: one contiguous 1 KB block per (row tile, chunk), like W
      asrc[i] = (const bf16*)a.a.base + (long long)min(tm * 16 + j, (a.M - 1) >> 4) * nch * 512 + lane * 8;
    } else {
      const int m = min(tm * GX_M + j * 16 + r, a.M - 1);
      asrc[i] = rm_bf(a.a, m) + 8 * g;
    }
    wsrc[i] = a.w + (long long)(tn * 16 + j) * nch * 512 + lane * 8;
  }
  auto issue = [&](int s) {
    bf16* st = smx + (s & (GX_NS - 1)) * GX_STAGE;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int j = 2 * wave + i;
      __builtin_amdgcn_global_load_lds((const void*)(asrc[i] + (a.apack ? (long long)s * 512 : (long long)s * 32)),
                                       (__attribute__((address_space(3))) void*)(st + j * 512), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const void*)(wsrc[i] + (long long)s * 512),
                                       (__attribute__((address_space(3))) void*)(st + (16 + j) * 512), 16, 0, 0);
    }
  };
  // one of a stage's 4 glds pieces per wave (q: block i = q >> 1, A (even) or W (odd))
  auto issue_piece = [&](int s, int q) {
    bf16* st = smx + (s & (GX_NS - 1)) * GX_STAGE;
    const int i = q >> 1, j = 2 * wave + i;
    if (q & 1)
      __builtin_amdgcn_global_load_lds((const void*)(wsrc[i] + (long long)s * 512),
                                       (__attribute__((address_space(3))) void*)(st + (16 + j) * 512), 16, 0, 0);
    else
      __builtin_amdgcn_global_load_lds((const void*)(asrc[i] + (a.apack ? (long long)s * 512 : (long long)s * 32)),
                                       (__attribute__((address_space(3))) void*)(st + j * 512), 16, 0, 0);
  };
  f32x4 acc[4][8];   // [weight tile nt][row tile mt]
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) acc[nt][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // fragments of stage s are read into registers during step s - 1 (two register
  // sets), so each wave's LDS reads of the next stage overlap its MFMAs
  auto frags = [&](int s, bf16x8 (&wf)[4], bf16x8 (&xf)[8]) {
    const bf16* st = smx + (s & (GX_NS - 1)) * GX_STAGE;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) wf[nt] = *(const bf16x8*)(st + (16 + wc * 4 + nt) * 512 + lane * 8);
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) xf[mt] = *(const bf16x8*)(st + (wr * 8 + mt) * 512 + lane * 8);
  };
  auto macs = [&](const bf16x8 (&wf)[4], const bf16x8 (&xf)[8]) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int mt = 0; mt < 8; ++mt) acc[nt][mt] = mfma(wf[nt], xf[mt], acc[nt][mt]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read (glds)
      __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);   // DS read
      __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);   // MFMA
    }
    // keep the MFMAs above the next step's asm waits ("memory" does not order
    // register-only instructions, cdna_hip_programming.md §5.7 rule 18)
    __builtin_amdgcn_sched_barrier(0);
  };
  // ring: stages s + 1 .. s + 3 in flight while stage s computes; exactly 4 glds
  // per wave per step (stages past the end re-load the last one into a buffer
  // nothing reads again), so vmcnt(8) retires stage s + 1 at every step and each
  // half-step below is one basic block the scheduler can interleave
  const int last = nch - 1;
  issue(0);
  issue(min(1, last));
  issue(min(2, last));
  issue(min(3, last));
  __builtin_amdgcn_s_waitcnt(WC_VM12);
  __builtin_amdgcn_s_barrier();
  bf16x8 wa[4], xa[8], wb[4], xb[8];
  frags(0, wa, xa);
  int s = 0;
  // A step in 4 pinned groups (sched_barrier fences): 1 glds piece of stage
  // s + 4, 3 fragment reads of stage s + 1, then the 8 MFMAs of weight tile nt = q
  // on stage s -- the loads' issue cost (M0 set-up, ~60+ cycles per LDS-DMA
  // piece) sits between MFMAs instead of in front of all 32 with the matrix pipe
  // idle.  Hand-placed: sched_group_barrier did not move the glds, and
  // s_setprio is a scheduling boundary (with it around the MFMAs every load
  // issued ahead of all 32).
  auto step = [&](int sis, int srd, const bf16x8 (&wf)[4], const bf16x8 (&xf)[8], bf16x8 (&wn)[4],
                  bf16x8 (&xn)[8]) {
    const bf16* st = smx + (srd & (GX_NS - 1)) * GX_STAGE;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      issue_piece(sis, q);
#pragma unroll
      for (int f = 3 * q; f < 3 * q + 3; ++f) {
        if (f < 4) wn[f] = *(const bf16x8*)(st + (16 + wc * 4 + f) * 512 + lane * 8);
        else xn[f - 4] = *(const bf16x8*)(st + (wr * 8 + f - 4) * 512 + lane * 8);
      }
#pragma unroll
      for (int mt = 0; mt < 8; ++mt) acc[q][mt] = mfma(wf[q], xf[mt], acc[q][mt]);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  for (; s + 1 < nch; s += 2) {
    __builtin_amdgcn_s_waitcnt(WC_VM8_LGKM0);
    __builtin_amdgcn_s_barrier();
    step(min(s + 4, last), s + 1, wa, xa, wb, xb);
    __builtin_amdgcn_s_waitcnt(WC_VM8_LGKM0);
    __builtin_amdgcn_s_barrier();
    step(min(s + 5, last), min(s + 2, last), wb, xb, wa, xa);
  }
  if (s < nch) {   // odd stage count: the last stage is in set a
    __builtin_amdgcn_s_waitcnt(WC_LGKM0);
    macs(wa, xa);
  }
  __builtin_amdgcn_s_waitcnt(WC_VM0);   // the past-the-end re-loads land before the workgroup ends
  // epilogue: the accumulators go through the (now idle) LDS ring, 16 tiles per
  // wave at a time, so ONE epi_tile body runs in a rolled loop that indexes
  // memory (unrolled copies of the RoPE / DPM forms spill; rotating 32
  // accumulators through one register tile cost ~4,000 moves per wave -- 30 % of
  // a K = 1536 tile)
  __syncthreads();   // every wave is past its reads of the last stage
  // pass p (row tiles 64 p .. 64 p + 63 of the wave's 128) -> this wave's LDS
  // region as [64 rows][64 cols] f32, odd rows' float4 slots XOR-shifted by one
  auto stage_ep = [&](float* ep, int p) {
    auto sw = [](int row, int col) { return row * 64 + (col ^ ((row & 1) << 2)); };
#pragma unroll
    for (int mq = 0; mq < 4; ++mq)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) *(f32x4*)(ep + sw(mq * 16 + r, nt * 16 + 4 * g)) = acc[nt][4 * p + mq];
  };
  if (rope_row8_ok(a)) {
    // q|k|v + RoPE + KV append in the same row-contiguous staging: a q / k lane
    // takes one row's 16-column tile (its two RoPE halves), a V lane one column
    // over 8 consecutive rows (one 16-byte store into the [dim][32 pos] block)
    float* ep = (float*)smx + wave * (64 * 64);
    auto sw = [](int row, int col) { return row * 64 + (col ^ ((row & 1) << 2)); };
    const int mb = tm * GX_M + wr * 128, nb = tn * GX_N + wc * 64;
    const bool vhead = (nb >> 7) >= a.rope.nh + a.rope.nkv;   // a wave's 64 columns lie in one head
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      stage_ep(ep, p);
      if (!vhead) {
#pragma unroll 1
        for (int it = 0; it < 4; ++it) {
          const int row = it * 16 + (lane >> 2), tq = lane & 3, m = mb + 64 * p + row;
          float lo[8], hi[8];
          *(f32x4*)lo = *(const f32x4*)(ep + sw(row, 16 * tq));
          *(f32x4*)(lo + 4) = *(const f32x4*)(ep + sw(row, 16 * tq + 4));
          *(f32x4*)hi = *(const f32x4*)(ep + sw(row, 16 * tq + 8));
          *(f32x4*)(hi + 4) = *(const f32x4*)(ep + sw(row, 16 * tq + 12));
          if (m < a.M) rope_qk8(a, m, nb + 16 * tq, lo, hi);
        }
      } else {
#pragma unroll 1
        for (int it = 0; it < 8; ++it) {
          const int r0 = it * 8, m0 = mb + 64 * p + r0;
          float vv[8];
#pragma unroll
          for (int k2 = 0; k2 < 8; ++k2) vv[k2] = ep[sw(r0 + k2, lane)];
          if (m0 < a.M) rope_v8(a, m0, nb + lane, vv);
        }
      }
    }
    return;
  }
  if (epi_row8_ok(a)) {
    // row-contiguous form: per wave and pass, 4 m-tiles x its 4 n-tiles -> LDS
    // [64 rows][64 cols] f32 (16 KB per wave, the whole ring for 8 waves; odd rows'
    // float4 slots XOR-shifted by one so the b128 reads below are conflict-free),
    // then every lane takes 8 consecutive columns of a row: 16-byte stores, 8 rows
    // x 128 bytes per instruction (SiLU*up: 16 rows x 64 bytes).  A wave reads
    // only its own region and its LDS ops run in order: no barrier between passes.
    float* ep = (float*)smx + wave * (64 * 64);
    auto sw = [](int row, int col) { return row * 64 + (col ^ ((row & 1) << 2)); };
    const int mb = tm * GX_M + wr * 128, nb = tn * GX_N + wc * 64;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      stage_ep(ep, p);
      if (a.epi.kind == EPI_SILU_MUL) {
#pragma unroll 1
        for (int it = 0; it < 4; ++it) {
          const int row = it * 16 + (lane >> 2), a4 = lane & 3, m = mb + 64 * p + row;
          float gt[8], up[8];
          *(f32x4*)gt = *(const f32x4*)(ep + sw(row, 16 * a4));
          *(f32x4*)(gt + 4) = *(const f32x4*)(ep + sw(row, 16 * a4 + 4));
          *(f32x4*)up = *(const f32x4*)(ep + sw(row, 16 * a4 + 8));
          *(f32x4*)(up + 4) = *(const f32x4*)(ep + sw(row, 16 * a4 + 12));
          if (m < a.M) epi_silu8(a, m, (nb >> 1) + 8 * a4, gt, up);
        }
      } else {
#pragma unroll 1
        for (int it = 0; it < 8; ++it) {
          const int row = it * 8 + (lane >> 3), c8 = lane & 7, m = mb + 64 * p + row;
          float v[8];
          *(f32x4*)v = *(const f32x4*)(ep + sw(row, 8 * c8));
          *(f32x4*)(v + 4) = *(const f32x4*)(ep + sw(row, 8 * c8 + 4));
          if (m < a.M) epi_row8(a, m, nb + 8 * c8, v);
        }
      }
    }
    return;
  }
  float* ep = (float*)smx + wave * (16 * 256);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int t = 0; t < 16; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) ep[t * 256 + j * 64 + lane] = acc[2 * h + (t >> 3)][t & 7][j];
#pragma unroll 1
    for (int t = 0; t < 16; ++t) {
      const int i = 16 * h + t;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = ep[t * 256 + j * 64 + lane];
      epi_tile(a, tm * GX_M + (wr * 8 + (i & 7)) * 16 + r, tn * GX_N + (wc * 4 + (i >> 3)) * 16, lane, v);
    }
  }
}

// ------------------------------------------------------------------ host launch
// Diagnostic state (process-wide; include/vibevoice_hip_diag.h documents each
// setter).  g_tune holds the words, gemm_decide reads one GemmTune snapshot.
constexpr size_t GEMV1_LDS_MAX = 151552, GEMV1_LDS_DEFAULT = 65536;   // k_gemv1's dynamic LDS (gemv1_lds below)
struct ShapeTune { int N, K, mmax, nw, ks, u, tpw; };
template <class I>
struct GemmTuneT {
  I nw{0}, ks{0}, handoff{-1}, waves{0}, u{0}, tpw{0};   // vv_gemv_tune / _tpw: 0 (-1) = the plan's
  I bal{1};                       // vv_gemv_tune_bal: 0 = ntile / 8 workgroups at M >= 8
  I max_m{64};                    // vv_gemv_tune_maxm: more rows than this take the tiled k_gemm
  I wide{1};                      // vv_gemv_tune_wide: 0 = k_gemv for every 16 < M <= 64
  I lds_max{GEMV1_LDS_DEFAULT};   // vv_gemv_tune_lds
  I rw_min_m{1}, rw_dma{1};       // vv_gemv_tune_rw
  // vv_gemm_tune_big: 0 keeps every M > 64 GEMM on k_gemm; 1 / 2 LDS stages of the
  // 128² tile (k_gemm_big); 3 (built-in) = the 256² tile (k_gemm_xl) where it
  // applies, else k_gemm_big<2>; + 4 (big_any) ignores the tile-count thresholds
  I big{3}, big_any{0};
  // vv_gemv_tune_shape: plan overrides for one (N, K) at M <= m_max, for same-box
  // A/Bs of a single shape inside the loop (tools/ab_bench.py)
  I nshape{0};
  ShapeTune shape[8];
};
using GemmTune = GemmTuneT<int>;
static GemmTuneT<std::atomic<int>> g_tune;
static GemmTune tune_snapshot() {
  const auto& g = g_tune;
  GemmTune t{g.nw, g.ks, g.handoff, g.waves, g.u, g.tpw, g.bal, g.max_m, g.wide, g.lds_max, g.rw_min_m, g.rw_dma,
             g.big, g.big_any, g.nshape};
  for (int i = 0; i < t.nshape; ++i) t.shape[i] = g.shape[i];
  return t;
}
extern "C" int vv_gemv_tune(int nw, int ks, int handoff, int target_waves, int u) {
  g_tune.nw = nw;
  g_tune.ks = ks;
  g_tune.handoff = handoff;
  g_tune.waves = target_waves;
  g_tune.u = u;
  return 0;
}
extern "C" int vv_gemv_tune_tpw(int tpw) { return g_tune.tpw = tpw, 0; }
extern "C" int vv_gemv_tune_bal(int on) { return g_tune.bal = on ? 1 : 0, 0; }
extern "C" int vv_gemv_tune_maxm(int m) { return g_tune.max_m = m > 0 ? m : 64, 0; }
extern "C" int vv_gemv_tune_wide(int on) { return g_tune.wide = on, 0; }
extern "C" int vv_gemv_tune_lds(int bytes) {
  return g_tune.lds_max = bytes > 0 && (size_t)bytes <= GEMV1_LDS_MAX ? bytes : (int)GEMV1_LDS_DEFAULT, 0;
}
extern "C" int vv_gemv_tune_rw(int min_m) {
  g_tune.rw_min_m = min_m > 0 ? min_m : 1;
  g_tune.rw_dma = min_m >= 0;
  return 0;
}
extern "C" int vv_gemm_tune_big(int mode) {
  g_tune.big_any = mode >= 0 && (mode & 4) ? 1 : 0;
  g_tune.big = mode < 0 ? 3 : mode & 3;
  return 0;
}
extern "C" int vv_gemv_tune_shape(int N, int K, int mmax, int nw, int ks, int u, int tpw) {
  if (N <= 0) return g_tune.nshape = 0, 0;
  const int n = g_tune.nshape;
  if (n >= 8) return 1;
  g_tune.shape[n] = {N, K, mmax, nw, ks, u, tpw};
  g_tune.nshape = n + 1;   // published after the entry (seq_cst store)
  return 0;
}

// diagnostic: GEMV launches record per-workgroup timestamps into buf (nullptr: off)
static std::atomic<unsigned long long*> g_stamps{nullptr};
extern "C" int vv_gemv_stamps(void* buf) { return g_stamps = (unsigned long long*)buf, 0; }
static const bool g_shape_log = getenv("VV_GEMM_LOG") != nullptr;

// ------------------------------------------------------------------ the launch decision (gemm_decide)
// Measured on MI355X (tools/gemv_sweep.py two-pass min, profiles/r01_gemv_sweep*.txt).
// Cross-workgroup split-K only for few-tile, long-row shapes (the M >= 8 down
// projections and codec fc2, and the M < 8 LM down projection, listed below):
// a hand-off costs >= 2 us in the sc1 form and up to 30 us with fences, which
// only those shapes win back in extra CUs.  Waves per workgroup (nw) and weight
// chunks in flight per wave (u):
//   * >= 1024 tiles (LM gate|up, head adaLN): 2 waves — every workgroup resident
//     in the first round (4-wave groups left a second-round tail: 16.7 -> 14.0 us)
//   * few tiles, long rows (LM / head down): 8 waves x 4; 128 tiles x K >= 8192
//     (codec fc2): 4 x 8; at M >= 8 two workgroups split K (the shapes
//     where the hand-off pays, profiles/r01_gemv_sweep_ks.txt: B = 8 LM down
//     18.7 -> 15.5 us, head down 13.0 -> 12.3, B = 8 codec fc2 13.1 -> 12.0),
//     and at M < 8 for < 128 tiles x K >= 8192 (LM down: 96 tiles reach only 96
//     CUs; same-box interleaved A/B, 5 pairs: B = 1 step 3.749 -> 3.725 ms,
//     B = 2 4.41 -> 4.30 ms)
//   * 16 < M <= 64 (k_gemv): 4 waves, 1 for >= 1024 tiles (the batched head
//     adaLN, M = 2 x 10 steps: 35 -> 20.5 us)
//   * few tiles, short rows (qkv, o_proj): 4 x 8, all chunks in flight at once
//   * 8 <= M <= 16 otherwise: 8 x 2; with many tiles the workgroup owns tpw
//     tiles that share one staging of the A rows (tools/gemv_sweep.py --tpw,
//     profiles/r01_gemv_sweep_tpw.txt: B = 8 LM gate|up 30.5 -> 20.0 us, head
//     gate|up 4 tiles per group 15.6 us)
struct GemvPlan { int nw, ksplit, u, tpw; };
static GemvPlan gemv_plan(int N, int K, int M, const GemmTune& t) {
  for (int i = 0; i < t.nshape; ++i) {
    const ShapeTune& s = t.shape[i];
    if (s.N == N && s.K == K && M <= s.mmax) return {s.nw, s.ks, s.u, s.tpw};
  }
  const int chunks = K / 32, tiles = N / 16;
  int nw = 4, ks = 1, u = 4, tpw = 1;
  if (tiles <= 128 && chunks >= 128) {
    if (M >= 8) {   // batched rows: 2-way split-K (sc1 hand-off) reaches 2x the CUs
      ks = 2;
      if (chunks == 256 && tiles == 128) nw = 8;   // codec fc2, C = 2,048: 8 x 4 (B = 8 in-loop A/B: -53 us per step)
      else if (chunks >= 256 && M <= 16) {
        // long rows: split K until the workgroup's A slice fits k_gemv1's 64 KB of
        // LDS (staged once) instead of k_gemv's per-wave A fragment reads from L2
        // (LM down at B = 8, M 16 x K 8,960: 5 ways; B = 8 step 5.15 -> 5.05 ms in
        // interleaved in-loop runs, profiles/r03_gemv_rw_ab.txt; the same rule for
        // the codec fc2 above cost +20 us); 8 waves x 4 chunks
        while (ks < 8 && (size_t)M * ((chunks + ks - 1) / ks * 32 + 8) * 2 > 65536) ++ks;
        nw = 8;
      } else if (chunks >= 256) u = 8;
      else {
        nw = 8;
        // 4 splits at M > 16 (the codec fc2 at C = 1,024, B = 8: 64 rows x N 1,024 x
        // K 4,096 on 64 tiles; interleaved in-loop pairs, B = 8 step 3.921 / 3.923 ->
        // 3.893 / 3.896 ms; 8 splits x 2 chunks 3.935)
        if (M > 16) ks = 4;
      }
    } else if (tiles < 128 && chunks >= 256) {   // M < 8 LM down: 2-way split-K, 8 waves x 4
      ks = 2;
      nw = 8;
    } else if (tiles == 128 && chunks >= 256) {
      if (chunks == 256) nw = 8;   // codec fc2 at C = 2,048 (K 8,192): 8 x 4 (in-loop A/Bs below)
      else u = 8;
    } else {
      nw = 8;
    }
  } else if (M > 16) {
    nw = tiles >= 1024 ? 1 : 4;   // k_gemv (A from L2 per chunk): batched head adaLN 35 -> 20.5 us
  } else if (M >= 8 && tiles <= 8 && chunks >= 32) {
    // the head's final layer (N 64, K 1,536: 4 tiles) at B = 8: 8-way split-K so 32
    // workgroups share the 16-row RMSNorm prologue and the stream (interleaved
    // in-loop pairs: B = 8 step -20..-40 us; at M = 2 the hand-off costs more
    // than it saves, +20..+50 us)
    nw = 8;
    u = 2;
    ks = 8;
  } else if (M >= 8) {
    nw = 8;
    u = 2;
    if (tiles >= 1024) {  // many tiles: 8 tiles per workgroup (one wave each) share one A staging
      tpw = 8;
      u = M > 8 ? 4 : 8;
    } else if (tiles >= 512) {
      // 2 tiles per workgroup (256 workgroups: the codec fc1 at C = 2,048, N 8,192 x
      // K 2,048, B = 8) -- 4 reached only 128 CUs; interleaved in-loop pairs, B = 8
      // step 3.953 / 3.948 -> 3.927 / 3.920 ms (tools/ab_bench.py gemv_tune_shape)
      tpw = 2;
      u = 4;
    }
  } else if (tiles >= 1024) {
    // (VibeVoice-Large's K 3,584 rows too: 4 waves x 2 chunks won the bare-GEMV
    // sweep, 46.1 -> 43.8 us, but lost in the loop, 7.07 -> 7.15 ms per step)
    nw = 2;
  } else if (tiles <= 128) {
    // LM q|k|v (128 tiles x K 1,536) with codec fc2 above: 8 waves x 4 chunks
    // instead of 4 x 8, interleaved in-loop pairs -5 .. -26 us per B = 1 step
    if (tiles == 128 && chunks <= 64) nw = 8;
    else u = 8;
  } else if (tiles >= 512 && chunks <= 64) {
    u = 2;   // head gate|up (576 tiles x K 1,536): 6 interleaved in-loop pairs, B = 1 step -13 us vs u = 4
  }
  if (t.waves > 0) {
    int wpt = (t.waves + tiles - 1) / tiles;
    const int maxw = (chunks + 3) / 4;
    if (wpt > maxw) wpt = maxw;
    if (wpt < 1) wpt = 1;
    nw = wpt < 4 ? wpt : 4;
    ks = (wpt + nw - 1) / nw;
  }
  if (t.nw > 0) nw = t.nw;
  if (t.ks > 0) ks = t.ks;
  if (t.u > 0) u = t.u;
  if (t.tpw > 0) tpw = t.tpw;
  if (ks > chunks) ks = chunks;
  return {nw, ks, u, tpw};
}

// k_gemv1's dynamic LDS: the staged A slice (+ per-item sums of squares for
// the fused RMSNorm).  Built-in limit 64 KB.  Up to GEMV1_LDS_MAX is possible
// with the per-kernel opt-in (one workgroup may hold 160 KiB; k_gemv1's static
// arrays take ~8.3 KB) so the B = 8 down projections (M = 16 rows of 4,480 /
// 2,304 columns per K split) stage A once per workgroup instead of k_gemv's
// per-wave fragment loads -- measured slower (B = 8 step 5.51 -> 5.83 ms: one
// workgroup per CU leaves too few weight loads in flight), so it stays a hook.
static size_t gemv1_lds(int M, int K, int ksplit, bool norm) {
  const size_t kw = ((K / 32 + ksplit - 1) / ksplit) * 32;
  const size_t xs = ((size_t)M * (kw + 8) * sizeof(bf16) + 15) & ~(size_t)15;
  return xs + (norm ? (size_t)M * (kw / 8) * sizeof(float) : 0);
}

// LDS of the XF_MIX GEMV (A rows + history/new rows + partial sums), 0 when
// the fused form does not apply (rows > 16, rows not whole samples, C outside
// [512, 2048] — k_mix's summation order needs >= 64 chunks — or > 64 KB)
size_t gemv_mix_lds(int M, int T, int C) {
  if (M <= 0 || M > 16 || T <= 0 || M % T || M / T > 4 || C < 512 || C > 2048 || C % 256) return 0;
  const int rows = (M / T) * (6 + T), n8 = C / 8;
  const size_t xs = ((size_t)M * (C + 8) * 2 + 15) & ~(size_t)15;
  const size_t lds = xs + (size_t)rows * C * 2 + (size_t)M * n8 * 4;
  return lds <= 98304 ? lds : 0;
}

// The GEMV family (M <= 64): k_gemvw, else the plan resolved against the
// arguments -- split-to-fit, the tiles-per-workgroup gate, the balanced form --
// and the form that runs it: k_gemv1 (special forms, RW) or k_gemv.
static GemmLaunch gemv_decide(const GemmArgs& a, int cus, const GemmTune& t) {
  const int tiles = a.N / 16, mrep = (a.M + 15) / 16, xk = a.xf.kind;
  GemmLaunch d;
  d.mrep = mrep;
  d.keep = a.keep != 0;
  d.handoff = t.handoff >= 0 ? t.handoff : 1;
  // k_gemvw: 16 < M <= 64, >= 256 tiles, plain A (no transform), one K split
  if (t.wide && a.M > 16 && tiles >= 256 && xk == XF_NONE && a.epi.kind != EPI_CFG_DPM) {
    d.kind = GemmKind::GEMVW;
    d.tpw = tiles >= 1024 ? 4 : tiles >= 512 ? 2 : 1;   // ~256-340 workgroups
    d.grid_x = (tiles + d.tpw - 1) / d.tpw;
    d.block = 512;
    return d;
  }
  GemvPlan p = gemv_plan(a.N, a.K, a.M, t);
  if (p.nw > 8) p.nw = 8;   // no plan asks for more waves (the balanced form below sets its own 10)
  const bool can_split = a.ws && a.counters && tiles <= 65536, norm = xk == XF_NORM;
  auto fits = [&](int ks) { return gemv1_lds(a.M, a.K, ks, norm) <= (size_t)t.lds_max; };
  int ks = p.ksplit > 1 && !can_split ? 1 : p.ksplit;
  // Rows too long for one workgroup to stage in k_gemv1's LDS at one K split
  // (VibeVoice-Large's LM down projection, M = 2 x K 18,944 = 76 KB): split K
  // until the slice fits, 8 waves x 4 chunks (tools/gemv_sweep.py --large: 48.4 ->
  // 27.1 us), instead of k_gemv re-loading A fragments from L2 per chunk.
  if (mrep == 1 && a.M < 8 && xk == XF_NONE && !t.ks && can_split && !fits(ks)) {
    int s = ks;
    while (!fits(s) && s < 4) s *= 2;
    if (fits(s)) {
      ks = s;
      if (!t.nw) p.nw = 8;
      if (!t.u) p.u = 4;
    }
  }
  int nw = p.nw, tpw = 1;
  if (mrep == 1 && ks == 1 && xk != XF_MIX && (p.tpw == 2 || p.tpw == 4 || p.tpw == 8) && nw % p.tpw == 0 && fits(1))
    tpw = p.tpw;
  // Many tiles at M >= 8 (B = 8 LM gate|up: 1,120 tiles): ntile / 8 = 140
  // workgroups streamed from 140 of the 256 CUs (tools/gemv_stamps.py: 8.2 us of
  // stream per workgroup).  Balanced form: one workgroup per CU, an even share of
  // 4 or 5 tiles each, 2 waves per tile (k_gemv1<.., 5, ..>).
  const bool bal = t.bal && tpw == 8 && a.M >= 8 && xk != XF_ATTN_MERGE && cus > 0 && (tiles + cus - 1) / cus == 5;
  if (bal) {
    tpw = 5;
    nw = 10;
  }
  d.u = p.u;
  if (xk == XF_MIX) {
    d.lds = gemv_mix_lds(a.M, a.xf.T, a.K);
    if (mrep != 1 || ks != 1 || !d.lds || (64 * nw) % (a.K / 8) || a.xf.ctx != 6 || a.a.idx) return GemmLaunch{};
    // tiles per workgroup (diagnostic plans only so far): the Block1D front half is
    // recomputed once per workgroup, so fewer, wider workgroups recompute it less
    tpw = (p.tpw == 2 || p.tpw == 4) && nw % p.tpw == 0 ? p.tpw : 1;
    d.u = 4;
    d.keep = 0;
    d.lds_optin = true;   // up to 96 KB (one workgroup may hold 160 KiB)
  } else if (xk == XF_ATTN_MERGE) {   // o_proj on the attention's split partials: one plan form
    if (mrep != 1 || a.xf.nsplit < 1 || a.xf.nsplit > 8 || a.K % 128 || !a.xf.part_o || !a.xf.part_ml || !a.xf.qpos)
      return GemmLaunch{};
    ks = tpw = 1;
    d.u = 8;
    d.keep = 0;
    d.lds = gemv1_lds(a.M, a.K, 1, false);
  } else if (mrep == 1 && fits(ks)) {
    d.lds = gemv1_lds(a.M, a.K, ks, norm);
    d.lds_optin = d.lds > 65536;
    // Row-per-wave norm prologue (k_gemv1's RW form) for this launch?  Whole rows
    // of K = 1,536 (3 items per lane) at up to 2 rows per wave, or K = 3,584 (7
    // items) at one row per wave without adaLN operands (their registers would cost
    // occupancy).  A separate instantiation: compiled into the item-per-thread
    // kernels it cost them registers / SGPR spills (B = 1 step 3.57 -> 3.66 ms).
    // Interleaved same-box runs (profiles/r03_gemv_rw_ab.txt): B = 8 step 5.45-5.47
    // -> 5.14-5.16 ms (M = 16 LM gate|up 19.98 -> 17.11 us, q|k|v 11.20 -> 8.63,
    // head gate|up 15.62 -> 12.45 in tools/gemv_variants.py), VibeVoice-Large B = 1
    // 7.14 -> 6.85 ms (K = 3,584 rows), 1.5B B = 1 3.597 -> 3.588 ms.
    // The K = 3,584 adaLN rows (VibeVoice-Large head) take the LDS-DMA form (RW 2),
    // built at one tile per workgroup only.
    // Diagnostic: vv_gemv_tune_rw(min rows; 99 = off; -1 = built-in without RW 2).
    if (norm && ks == 1 && a.M >= t.rw_min_m && a.K % 512 == 0) {
      const int ipr = a.K / 512, rpw = (a.M + nw - 1) / nw;
      if (ipr == 3 && rpw <= 2) d.rw = 1;
      else if (ipr == 7 && rpw == 1) d.rw = !a.xf.mod ? 1 : t.rw_dma && tpw == 1 ? 2 : 0;
    }
  }
  // k_gemv1 (d.lds set), else k_gemv: mrep > 1, or the A slice does not fit
  d.kind = d.lds ? GemmKind::GEMV1 : GemmKind::GEMV;
  d.xf = xk;
  d.ksplit = ks;
  d.tpw = tpw;
  d.grid_x = bal ? cus : (tiles + tpw - 1) / tpw;
  d.grid_y = ks;
  d.block = 64 * nw;
  return d;
}

// The tiled kernels (M > 64, or above vv_gemv_tune_maxm's rows)
constexpr int GEMM_BN32 = 128;   // fewer 64-wide-tile workgroups than this: 32-wide tiles
static GemmLaunch gemm_tiled_decide(const GemmArgs& a, const GemmTune& t) {
  GemmLaunch d;
  d.xf = a.xf.kind == XF_NORM || a.xf.kind == XF_SILU_ADD ? a.xf.kind : XF_NONE;
  d.block = 256;
  // k_gemm_big only with >= one 128 x 128 tile per CU or >= 2^30 MACs: the
  // decode loop's codec GEMMs (B = 8: 320 - 1,600 rows x 256 - 1,024 columns
  // x K <= 1,024: 24 - 104 such tiles) are faster as k_gemm's 4x more 64 x 64
  // workgroups (B = 8 step 5.53 ms vs 5.83), a 1K-token prompt's o / down /
  // q|k|v projections (108 - 144 tiles, K >= 1,536) on k_gemm_big (14.5 -> 13.4 ms)
  // k_gemm_xl with >= GX_MIN_TILES 256 x 256 tiles (16K-token prefill: 384 - 4,480 tiles)
  const bool big_rows = d.xf == XF_NONE && a.M >= GEMM_BIG_M;
  const int total_xl = ((a.M + GX_M - 1) / GX_M) * (a.N / GX_N), total = ((a.M + GB_M - 1) / GB_M) * (a.N / GB_N);
  // 64-wide tiles unless that leaves fewer than GEMM_BN32 workgroups (the
  // codec's 200-row stage: fc2 N = 256 is 16 workgroups of K = 1,024)
  const int wg64 = ((a.M + 63) / 64) * (a.N / 64);
  if (big_rows && t.big == 3 && a.N % GX_N == 0 && a.K % 32 == 0 && (total_xl >= GX_MIN_TILES || t.big_any)) {
    d.kind = GemmKind::GEMM_XL;
    d.grid_x = total_xl;
    d.block = 512;
    d.lds = GX_LDS;
    d.lds_optin = true;
  } else if (big_rows && t.big && a.N % GB_N == 0 && a.K % GB_K == 0 &&
             (total >= GEMM_BIG_TILES || (long long)a.M * a.N * a.K >= (1LL << 30) || t.big_any)) {
    d.kind = t.big == 1 ? GemmKind::GEMM_BIG1 : GemmKind::GEMM_BIG2;
    d.grid_x = ((total + 7) >> 3) * 8;
  } else if (a.N % 32 == 0) {
    const bool bn64 = a.N % 64 == 0 && wg64 >= GEMM_BN32;
    d.kind = bn64 ? GemmKind::GEMM64 : GemmKind::GEMM32;
    d.grid_x = (a.M + 63) / 64;
    d.grid_y = a.N / (bn64 ? 64 : 32);
  }
  return d;
}

GemmLaunch gemm_decide(const GemmArgs& a, int cus) {
  const GemmTune t = tune_snapshot();
  GemmLaunch d;
  if (a.M <= 0 || a.K % 32 || a.N % 16 || (a.epi.kind == EPI_CFG_DPM && a.M > 16)) return d;
  if (a.w8 && gemv_w8_serves(a)) {   // FP8 weight-only storage: its own GEMV, or dequantise and go on in bf16
    d.kind = GemmKind::GEMV_W8;
    return d;
  }
  const bool gemv = a.M <= 64 && (a.M <= 16 || a.M <= t.max_m || a.epi.kind == EPI_CFG_DPM);
  d = gemv ? gemv_decide(a, cus, t) : gemm_tiled_decide(a, t);
  if (a.w8) {
    // FP8 weights above 16 rows: the chosen bf16 kernel's W8 instantiation reads the
    // codes itself where one is built -- k_gemv<2..4>, k_gemvw and k_gemm<64 / 32>,
    // every transform they take, K % 64 == 0 (whole chunk pairs per row).  The rest
    // dequantises first: k_gemv1's forms gemv_w8_serves declines and k_gemv<1> (at
    // most 16 rows), k_gemm_big / k_gemm_xl (>= 256 rows amortise one dequantise
    // pass), and everything under vv_gemv_w8(0).
    const bool built = (d.kind == GemmKind::GEMV && d.mrep >= 2) || d.kind == GemmKind::GEMVW ||
                       d.kind == GemmKind::GEMM64 || d.kind == GemmKind::GEMM32;
    d.w8_native = built && a.w8e && a.K % 64 == 0 && gemv_w8_enabled();
    d.dequant_w8 = !d.w8_native;
  }
  return d;
}

bool gemm_uses_xl(const GemmArgs& a) { return gemm_decide(a, 0).kind == GemmKind::GEMM_XL; }

// Host-only plan queries (no device work; tests and tools): gemm_decide's answer
// for a shape, with placeholder operands (the decision only tests them for null).
static GemmArgs plan_args(int M, int N, int K, int xf, int has_w, int has_mod, int epi, int keep) {
  static const bf16 dummy[8] = {};
  static float dummy_f[1];
  static unsigned dummy_ctr[1];
  static const int dummy_i[1] = {};
  GemmArgs a{};
  a.M = M;
  a.N = N;
  a.K = K;
  a.epi.kind = epi;
  a.keep = keep;
  a.xf.kind = xf;
  a.xf.w = has_w ? dummy : nullptr;
  a.xf.mod = has_mod ? dummy : nullptr;
  a.xf.T = 1;   // XF_MIX: M samples of one step
  a.xf.ctx = 6;
  a.xf.part_o = a.xf.part_ml = dummy_f;   // XF_ATTN_MERGE: one split
  a.xf.qpos = dummy_i;
  a.xf.nsplit = 1;
  a.ws = dummy_f;
  a.counters = dummy_ctr;
  return a;
}
static bool plan_bad(int M, int N, int K, int xf, int epi, const int* out) {
  return M <= 0 || K <= 0 || K % 32 || N <= 0 || N % 16 || !out || xf < XF_NONE || xf > XF_ATTN_MERGE ||
         epi < EPI_STORE || epi > EPI_CFG_DPM;
}
static void plan_words(const GemmLaunch& d, int* o) {
  const int w[11] = {(int)d.kind, d.mrep, (int)d.block / 64, d.ksplit, d.u, d.tpw, d.rw, (int)d.grid_x, (int)d.grid_y,
                     (int)d.block, (int)d.lds};
  std::copy(w, w + 11, o);
}

// CUs of the current device (cached per device)
static int device_cus() {
  static std::atomic<int> cache[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 0;
  int v = cache[dev].load();
  if (!v) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    cache[dev] = v;
  }
  return v;
}
// Any M, every kind, on a device of `cus` CUs: out[11] = {GemmKind, mrep, waves, K splits, u, tpw, rw,
// grid x, grid y, workgroup size, dynamic LDS bytes}; n = the caller's capacity in words.
extern "C" int vv_gemm_plan(int M, int N, int K, int xf, int has_w, int has_mod, int epi, int keep, int cus, int* out,
                            int n) {
  if (n < 11 || plan_bad(M, N, K, xf, epi, out)) return 1;
  plan_words(gemm_decide(plan_args(M, N, K, xf, has_w, has_mod, epi, keep), cus), out);
  return 0;
}
// The same for a quantised operand (GemmArgs::w8): out[0..10] = the bf16 decision's words (what runs after a
// dequantise, and the geometry of the W8 instantiation), out[11] = where the codes go: 0 k_gemv_w8, 1 the bf16
// kernel's W8 instantiation, 2 dequantise into the scratch first.
extern "C" int vv_gemm_plan_w8(int M, int N, int K, int xf, int has_w, int has_mod, int epi, int keep, int cus, int* out,
                               int n) {
  if (n < 12 || plan_bad(M, N, K, xf, epi, out)) return 1;
  GemmArgs a = plan_args(M, N, K, xf, has_w, has_mod, epi, keep);
  plan_words(gemm_decide(a, cus), out);
  static const unsigned char dummy8[1] = {};
  a.w8 = dummy8;
  a.w8e = (const signed char*)dummy8;
  const GemmLaunch q = gemm_decide(a, cus);
  out[11] = q.kind == GemmKind::GEMV_W8 ? 0 : q.w8_native ? 1 : 2;
  return 0;
}
// An M <= 16 GEMV on the current device: out[7] = {kernel (0 k_gemv1, 1 k_gemv: A fragments from L2), waves,
// K splits, u, tpw, rw (0 item per thread, 1 row per wave, 2 row per wave with LDS-DMA rows), LDS bytes}.
extern "C" int vv_gemv_plan(int M, int N, int K, int xf, int has_w, int has_mod, int* out) {
  int o[11];
  if (M > 16 || xf > XF_SILU_ADD || !out || vv_gemm_plan(M, N, K, xf, has_w, has_mod, EPI_STORE, 0, device_cus(), o, 11))
    return 1;
  const int g[7] = {o[0] != (int)GemmKind::GEMV1, o[2], o[3], o[4], o[5], o[6], o[10]};
  std::copy(g, g + 7, out);
  return 0;
}

// ------------------------------------------------------------------ the launcher
// A runtime value as a template argument: f(std::integral_constant<int, V>) for
// the V among Vs that equals v; 1 (as launch_gemm's "not served") when none does.
template <int... Vs, class F>
static int pick(int v, F f) {
  int rc = 1;
  (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
  return rc;
}
#define V(x) decltype(x)::value

// The k_gemv1 builds: U x KEEP x TPW for the three plain transforms, the RW
// forms for XF_NORM (RW 2 at one tile per workgroup), and the two special forms.
// TPW is a template argument so the one-tile form (every M < 8 launch) keeps
// its straight-line index math (a runtime tiles-per-group cost 1 us per launch)
constexpr bool gemv1_built(int xf, int u, int keep, int tpw, int rw) {
  if (xf == XF_MIX) return u == 4 && !keep && rw == 0 && (tpw == 1 || tpw == 2 || tpw == 4);
  if (xf == XF_ATTN_MERGE) return u == 8 && !keep && rw == 0 && tpw == 1;
  return rw == 0 || (xf == XF_NORM && (rw == 1 || tpw == 1));
}
static int go_gemv1(const GemmLaunch& d, const GemmArgs& a, hipStream_t st) {
  return pick<XF_NONE, XF_NORM, XF_SILU_ADD, XF_MIX, XF_ATTN_MERGE>(d.xf, [&](auto XF) {
    return pick<2, 4, 8>(d.u == 2 || d.u == 4 ? d.u : 8, [&](auto U) {
      return pick<0, 1>(d.keep, [&](auto KEEP) {
        return pick<1, 2, 4, 5, 8>(d.tpw, [&](auto TPW) {
          return pick<0, 1, 2>(d.rw, [&](auto RW) {
            if constexpr (gemv1_built(V(XF), V(U), V(KEEP), V(TPW), V(RW))) {
              constexpr auto k = k_gemv1<V(U), V(XF), V(KEEP) != 0, V(TPW), V(RW)>;
              if (d.lds_optin) {   // > 64 KB of dynamic LDS needs the opt-in, once per instantiation
                static const bool attr = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                             V(XF) == XF_MIX ? 98304 : (int)GEMV1_LDS_MAX) == hipSuccess;
                if (!attr) return 2;
              }
              hipLaunchKernelGGL(k, dim3(d.grid_x, d.grid_y), dim3(d.block), d.lds, st, a);
              return 0;
            } else {
              return 1;
            }
          });
        });
      });
    });
  });
}
static int go_gemvw(const GemmLaunch& d, const GemmArgs& a, hipStream_t st) {
  return pick<2, 3, 4>(d.mrep, [&](auto MREP) {
    return pick<1, 2, 4>(d.tpw, [&](auto TPW) {
      return pick<0, 1>(d.keep, [&](auto KEEP) {
        return pick<0, 1>(d.w8_native, [&](auto W8) {
          hipLaunchKernelGGL((k_gemvw<V(MREP), V(TPW), V(KEEP) != 0, V(W8) != 0>), dim3(d.grid_x), dim3(d.block), 0, st,
                             a);
          return 0;
        });
      });
    });
  });
}

// returns 0 ok, else an error code (see engine.cpp)
int launch_gemm(GemmArgs a, hipStream_t st) {
  if (a.M <= 0) return 0;
  if (a.K % 32 != 0 || a.N % 16 != 0) return 1;
  if (a.apack && (a.xf.kind != XF_NONE || !gemm_uses_xl(a))) return 1;   // only k_gemm_xl reads packed A rows
  if (a.epi.pack && (a.epi.kind != EPI_SILU_MUL || a.xf.kind != XF_NONE || !gemm_uses_xl(a) || (a.N >> 1) % 32 ||
                     ((unsigned long long)a.epi.out.base & 15)))
    return 1;   // ... and only its row-contiguous SiLU*up epilogue writes them
  if (a.xf.kind == XF_NORM && a.K % 8 != 0) return 1;
  if (a.epi.kind == EPI_ROPE && (a.rope.kv.d != 128 || !a.rope.pos || !a.rope.slots)) return 1;
  if (a.epi.kind == EPI_CFG_DPM && (a.M > 16 || 2 * a.dpm.n != a.M)) return 1;
  // (only the balanced form, M >= 8, reads the CU count: the M < 8 decode launches skip the runtime's query)
  const GemmLaunch d = gemm_decide(a, a.M >= 8 ? device_cus() : 0);
  if (d.kind == GemmKind::REJECT) return 1;
  if (d.kind == GemmKind::GEMV_W8) return launch_gemv_w8(a, st);
  if (d.dequant_w8) {
    if (!a.w8e || !a.w8_scratch || a.K % 64) return 1;
    if (int rc = launch_dequant_w8(a.w8, a.w8e, a.w8_scratch, a.N, a.K, st)) return rc;
    a.w = a.w8_scratch;
    a.w8 = nullptr;
  }
  a.stamps = g_stamps;
  if (g_shape_log) {   // VV_GEMM_LOG=1: one line per launch (shape census for profiles/)
    fprintf(stderr, "vv_gemm M=%d N=%d K=%d xf=%d epi=%d\n", a.M, a.N, a.K, a.xf.kind, a.epi.kind);
  }
  a.ksplit = d.ksplit;
  a.handoff = d.handoff;
  a.tpw = d.tpw;
  const dim3 grid(d.grid_x, d.grid_y), block(d.block);
  // (XF, W8): the transform and the weight operand (W8 = d.w8_native) as template arguments
  auto xf3 = [&](auto f) {
    return pick<XF_NONE, XF_NORM, XF_SILU_ADD>(d.xf, [&](auto XF) {
      return pick<0, 1>(d.w8_native, [&](auto W8) { return f(XF, std::bool_constant<V(W8) != 0>{}); });
    });
  };
  int rc = 0;
  switch (d.kind) {
    case GemmKind::GEMV1: rc = go_gemv1(d, a, st); break;
    case GemmKind::GEMVW: rc = go_gemvw(d, a, st); break;
    case GemmKind::GEMV:   // chunks in flight per mrep: 8 / 4 / 2 / 2
      rc = xf3([&](auto XF, auto W8) {
        if (d.mrep == 1) {
          if constexpr (V(W8)) return 1;   // not built (gemm_decide)
          else hipLaunchKernelGGL((k_gemv<1, 8, V(XF)>), grid, block, 0, st, a);
        } else if (d.mrep == 2) hipLaunchKernelGGL((k_gemv<2, 4, V(XF), V(W8)>), grid, block, 0, st, a);
        else if (d.mrep == 3) hipLaunchKernelGGL((k_gemv<3, 2, V(XF), V(W8)>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_gemv<4, 2, V(XF), V(W8)>), grid, block, 0, st, a);
        return 0;
      });
      break;
    case GemmKind::GEMM64:
    case GemmKind::GEMM32:
      rc = xf3([&](auto XF, auto W8) {
        if (d.kind == GemmKind::GEMM64) hipLaunchKernelGGL((k_gemm<64, V(XF), V(W8)>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_gemm<32, V(XF), V(W8)>), grid, block, 0, st, a);
        return 0;
      });
      break;
    case GemmKind::GEMM_BIG1: hipLaunchKernelGGL(k_gemm_big<1>, grid, block, 0, st, a); break;
    case GemmKind::GEMM_BIG2: hipLaunchKernelGGL(k_gemm_big<2>, grid, block, 0, st, a); break;
    default: {   // GEMM_XL
      static const bool attr = hipFuncSetAttribute((const void*)k_gemm_xl, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)GX_LDS) == hipSuccess;   // once (thread-safe static init)
      if (!attr) return 2;
      hipLaunchKernelGGL(k_gemm_xl, grid, block, d.lds, st, a);
    }
  }
  if (rc) return rc;
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
#undef V
