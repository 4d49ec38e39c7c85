// FP8 (OCP e4m3) KV cache for the LM: the quantiser that appends to it, its
// entry copy and the diagnostic row access.  (The attention kernels that read
// it are the one-byte instantiations of k_attn / k_attn_pf in attention.hip;
// k_lm_attn's FP8-KV form in lm_attn.hip appends and reads in one launch.  The
// row quantiser itself is kv_quant_dev.h, shared with it.)
//
// Format (vibevoice_amd/weights.py: quantize_rows_e4m3 / fake_quantize_kv): a
// row is the 128 bf16 values of one (layer, slot, kv head, position), K after
// RoPE and V separately.  e = the smallest integer with amax / 2^e <= 448 (an
// all-zero row: 0; clamped to [-100, 127]); codes = round-to-nearest-even e4m3
// of x * 2^-e, so no code saturates and no NaN code occurs; code * 2^e is exact
// in bf16.  Storage (kernels.h KV8): the codes in the bf16 cache's geometry at
// one byte per element -- K [layer][slot][kv_head][ctx][128], V in 32-position
// blocks of [128][32] (common.h v_off) -- and the exponents in side arrays
// [layer][slot][kv_head][ctx].
//
// Append: the q|k|v projection's EPI_ROPE epilogues (GEMV, GEMM and FP8-GEMV
// families) are unchanged.  Under FP8 KV the engine points their KVLayout at a
// bf16 staging cache of one slot whose position is the pass's token index m
// (slot table all 0, position table 0, 1, 2, ...; the epilogue reads cos / sin
// at its position, so the pass also gets a table of the real positions' rows),
// and k_kv_quant then moves every staged row to the token's real (slot,
// position).  Attention runs after it, so every key and value it reads --
// the pass's own tokens included -- is a dequantised stored value.
#include <algorithm>

#include "kernels.h"
#include "kv_quant_dev.h"

namespace {

constexpr int KQ_WAVES = 4;

// wave w of the grid takes rows w, w + waves, ...: row = (K | V, kv head, token),
// tokens fastest (neighbouring waves read neighbouring staged rows / the same V block)
__global__ void __launch_bounds__(64 * KQ_WAVES) k_kv_quant(KVLayout stg, KVLayout kv, KV8 q, int layer, int nkv,
                                                            int nslots, int ntok, const int* slots, const int* pos) {
  constexpr int d = 128;
  const int lane = threadIdx.x & 63;
  const long long rows = 2ll * nkv * ntok;
  for (long long row = (long long)blockIdx.x * KQ_WAVES + (threadIdx.x >> 6); row < rows;
       row += (long long)gridDim.x * KQ_WAVES) {
    const int m = (int)(row % ntok), hv = (int)(row / ntok), h = hv % nkv, isv = hv / nkv;
    const int slot = slots[m], p = pos[m];
    if (slot < 0 || slot >= nslots || p < 0 || p >= kv.max_ctx) continue;   // wave-uniform
    const long long sb = (long long)h * stg.s_head;
    const long long cb = (long long)layer * kv.s_layer + (long long)slot * kv.s_slot + (long long)h * kv.s_head;
    float x0, x1;
    if (!isv) {
      const bf16* src = stg.k + sb + (long long)m * d + 2 * lane;
      x0 = bf(src[0]);
      x1 = bf(src[1]);
    } else {
      x0 = bf(stg.v[sb + v_off(2 * lane, m)]);
      x1 = bf(stg.v[sb + v_off(2 * lane + 1, m)]);
    }
    unsigned c0, c1;
    const int e = quant_row(x0, x1, c0, c1);
    if (!isv) {
      *(unsigned short*)(q.k + cb + (long long)p * d + 2 * lane) = (unsigned short)(c0 | (c1 << 8));
      if (lane == 0) q.ek[cb / d + p] = (signed char)e;
    } else {
      q.v[cb + v_off(2 * lane, p)] = (unsigned char)c0;
      q.v[cb + v_off(2 * lane + 1, p)] = (unsigned char)c1;
      if (lane == 0) q.ev[cb / d + p] = (signed char)e;
    }
  }
}

// the pass's tables for the staged append (one thread per 8 table elements + the index tables)
// (the index tables are written for all `cap` staging positions: the epilogue's run test reads up to 7 past a row)
__global__ void __launch_bounds__(256) k_kv_stage_prep(int ntok, int cap, const int* pos, int max_ctx,
                                                       const bf16* rope_tab, bf16* cs, int* stg_slot, int* stg_pos) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int m = i >> 4, j = (i & 15) * 8;
  if (m >= cap) return;
  if (j == 0) {
    stg_slot[m] = 0;
    stg_pos[m] = m;
  }
  if (m >= ntok) return;
  const int p = min(max(pos[m], 0), max_ctx - 1);
  *(bf16x8*)(cs + (long long)m * 128 + j) = *(const bf16x8*)(rope_tab + (long long)p * 128 + j);
}

// k_kv_copy for the FP8 cache: codes and exponents of entry src -> dst, every layer / kv head
__global__ void __launch_bounds__(256) k_kv_copy8(KVLayout kv, KV8 q, int n_layers, int nkv, const int* slots,
                                                  const int* src, const int* dst) {
  const int i = blockIdx.x;
  const int d = kv.d;
  const int per = n_layers * nkv * d;
  for (int e = threadIdx.x; e < per; e += blockDim.x) {
    const int l = e / (nkv * d), r = e - l * nkv * d, h = r / d, j = r - h * d;
    const long long hb = (long long)l * kv.s_layer + (long long)slots[i] * kv.s_slot + (long long)h * kv.s_head;
    q.k[hb + (long long)dst[i] * d + j] = q.k[hb + (long long)src[i] * d + j];
    q.v[hb + v_off(j, dst[i])] = q.v[hb + v_off(j, src[i])];
    if (j == 0) {
      q.ek[hb / d + dst[i]] = q.ek[hb / d + src[i]];
      q.ev[hb / d + dst[i]] = q.ev[hb / d + src[i]];
    }
  }
}

// diagnostics: one wave per (K | V, layer, kv head, position) row of one slot
template <bool F8, bool WRITE>
__global__ void __launch_bounds__(64 * KQ_WAVES) k_kv_rows(KVLayout kv, KV8 q, int n_layers, int nkv, int slot, int p0,
                                                           int p1, bf16* k_rows, bf16* v_rows) {
  constexpr int d = 128;
  const int lane = threadIdx.x & 63, span = p1 - p0;
  const long long rows = 2ll * n_layers * nkv * span;
  for (long long row = (long long)blockIdx.x * KQ_WAVES + (threadIdx.x >> 6); row < rows;
       row += (long long)gridDim.x * KQ_WAVES) {
    const int pi = (int)(row % span);
    const long long lh = row / span;
    const int h = (int)(lh % nkv), l = (int)(lh / nkv % n_layers), isv = (int)(lh / nkv / n_layers);
    const int p = p0 + pi;
    const long long cb = (long long)l * kv.s_layer + (long long)slot * kv.s_slot + (long long)h * kv.s_head;
    bf16* host = (isv ? v_rows : k_rows) + (((long long)l * nkv + h) * span + pi) * d + 2 * lane;
    const long long i0 = isv ? cb + v_off(2 * lane, p) : cb + (long long)p * d + 2 * lane;
    const long long i1 = isv ? cb + v_off(2 * lane + 1, p) : i0 + 1;
    signed char* ex = (isv ? q.ev : q.ek) + cb / d + p;
    if (WRITE) {
      const float x0 = bf(host[0]), x1 = bf(host[1]);
      if (F8) {
        unsigned c0, c1;
        const int e = quant_row(x0, x1, c0, c1);
        unsigned char* c = isv ? q.v : q.k;
        c[i0] = (unsigned char)c0;
        c[i1] = (unsigned char)c1;
        if (lane == 0) *ex = (signed char)e;
      } else {
        bf16* c = isv ? kv.v : kv.k;
        c[i0] = host[0];
        c[i1] = host[1];
      }
    } else {
      if (F8) {
        const unsigned char* c = isv ? q.v : q.k;
        const int e = *ex;
        host[0] = tobf(ldexpf(dec_e4m3(c[i0]), e));
        host[1] = tobf(ldexpf(dec_e4m3(c[i1]), e));
      } else {
        const bf16* c = isv ? kv.v : kv.k;
        host[0] = c[i0];
        host[1] = c[i1];
      }
    }
  }
}

int wave_grid(long long rows) { return (int)std::min<long long>((rows + KQ_WAVES - 1) / KQ_WAVES, 16384); }

}  // namespace

int launch_kv_stage_prep(int ntok, int cap, const int* pos, int max_ctx, const bf16* rope_tab, bf16* cs,
                         int* stg_slot, int* stg_pos, hipStream_t st) {
  if (ntok <= 0) return 0;
  if (!pos || !rope_tab || !cs || !stg_slot || !stg_pos || max_ctx < 1 || cap < ntok) return 1;
  hipLaunchKernelGGL(k_kv_stage_prep, dim3((cap * 16 + 255) / 256), dim3(256), 0, st, ntok, cap, pos, max_ctx,
                     rope_tab, cs, stg_slot, stg_pos);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

int launch_kv_quant(KVLayout stg, KVLayout kv, KV8 kv8, int layer, int nkv, int nslots, int ntok, const int* slots,
                    const int* pos, hipStream_t st) {
  if (ntok <= 0) return 0;
  if (kv.d != 128 || stg.d != 128 || ntok > stg.max_ctx || !stg.k || !stg.v || !kv8.k || !kv8.v || !kv8.ek ||
      !kv8.ev || layer < 0 || kv.s_layer % 128 || kv.s_slot % 128 || kv.s_head % 128)
    return 1;
  hipLaunchKernelGGL(k_kv_quant, dim3(wave_grid(2ll * nkv * ntok)), dim3(64 * KQ_WAVES), 0, st, stg, kv, kv8, layer,
                     nkv, nslots, ntok, slots, pos);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

int launch_kv_copy8(KVLayout kv, KV8 kv8, int n_layers, int nkv, int n, const int* slots, const int* src,
                    const int* dst, hipStream_t st) {
  if (n <= 0) return 0;
  if (!kv8.k || kv.d != 128) return 1;
  hipLaunchKernelGGL(k_kv_copy8, dim3(n), dim3(256), 0, st, kv, kv8, n_layers, nkv, slots, src, dst);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

int launch_kv_rows(KVLayout kv, KV8 kv8, int n_layers, int nkv, int slot, int p0, int p1, bf16* k_rows, bf16* v_rows,
                   int write, hipStream_t st) {
  if (p1 <= p0) return 0;
  if (kv.d != 128 || p0 < 0 || p1 > kv.max_ctx || slot < 0 || !k_rows || !v_rows) return 1;
  const dim3 grid(wave_grid(2ll * n_layers * nkv * (p1 - p0))), blk(64 * KQ_WAVES);
  if (kv8.k) {
    if (write) hipLaunchKernelGGL((k_kv_rows<true, true>), grid, blk, 0, st, kv, kv8, n_layers, nkv, slot, p0, p1, k_rows, v_rows);
    else hipLaunchKernelGGL((k_kv_rows<true, false>), grid, blk, 0, st, kv, kv8, n_layers, nkv, slot, p0, p1, k_rows, v_rows);
  } else {
    if (write) hipLaunchKernelGGL((k_kv_rows<false, true>), grid, blk, 0, st, kv, kv8, n_layers, nkv, slot, p0, p1, k_rows, v_rows);
    else hipLaunchKernelGGL((k_kv_rows<false, false>), grid, blk, 0, st, kv, kv8, n_layers, nkv, slot, p0, p1, k_rows, v_rows);
  }
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
