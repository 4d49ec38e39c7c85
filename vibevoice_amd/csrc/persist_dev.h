// Device helpers of the grid-waiting kernels (head_m16.hip, lm_ffn.hip,
// lm_attn.hip, codec_stage.hip, codec_wide.hip): one workgroup per CU (G = 256),
// a control wave doing the hand-offs, grid-wide waits on XCD-sharded counters
// (sync_layout.h: which counter lives where).
#pragma once
#include "gemv_dev.h"
#include "sync_layout.h"

#pragma clang diagnostic ignored "-Winline-asm"

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) const bf16x8 hl_gbf16x8;
typedef __attribute__((address_space(1))) unsigned hl_gu32;
DEV bf16x8 hl_ld(const bf16* p) { return *(hl_gbf16x8*)p; }
// a weight-stream load: global (a flat load would also count in lgkmcnt, so every
// LDS wait would drain the stream) and non-temporal (gemv_dev.h ldw)
DEV bf16x8 hl_ldnt(const bf16* p) { return __builtin_nontemporal_load((hl_gbf16x8*)p); }
// the FP8 weight stream (lm_ffn.hip, lm_attn.hip): global and non-temporal as hl_ldnt;
// 16 bytes = a lane's piece of a pair block, 8 bytes = one k-block's fragment of it
typedef __attribute__((address_space(1))) const u32x4 hl_gu32x4;
typedef __attribute__((address_space(1))) const u32x2 hl_gu32x2;
DEV u32x4 hl_ldnt8(const unsigned char* p) { return __builtin_nontemporal_load((hl_gu32x4*)p); }
DEV u32x2 hl_ldnt8h(const unsigned char* p) { return __builtin_nontemporal_load((hl_gu32x2*)p); }
// fragment `half` (0 / 1) of a lane's 16 code bytes, scaled by the lane's row scale
DEV bf16x8 hl_frag8(u32x4 v, int half, float sc) { return half ? cvt8s(v[2], v[3], sc) : cvt8s(v[0], v[1], sc); }

DEV float hl_dot8(bf16x8 w, bf16x8 x, float acc) {
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(w, w, 0, 1), __builtin_shufflevector(x, x, 0, 1), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(w, w, 2, 3), __builtin_shufflevector(x, x, 2, 3), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(w, w, 4, 5), __builtin_shufflevector(x, x, 4, 5), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(w, w, 6, 7), __builtin_shufflevector(x, x, 6, 7), acc, false);
  return acc;
}

// 16-byte LDS DMA (global_load_lds_dwordx4): lane l's 16 bytes from gptr land at
// lds_base + 16 l (lds_base wave-uniform).  Inline asm, so hipcc neither drains
// the queue before the first LDS access nor counts it: the issuing wave waits
// with an explicit s_waitcnt vmcnt.  SC1: the bytes were written in this launch
// (write-through stores, MI355X_MICROARCH.md's hand-off table: sc1 loads).
// NT: a weight stream read once per token (no reuse before eviction: the
// non-temporal policy keeps it from evicting what does stay in the caches).
template <bool SC1, bool NT = false>
DEV void hl_dma16(const void* lds_base, const void* gptr) {
  const unsigned lds = __builtin_amdgcn_readfirstlane(
      (unsigned)(unsigned long long)(__attribute__((address_space(3))) const unsigned char*)lds_base);
  if (NT)
    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off nt" ::"s"(lds), "v"(gptr) : "memory", "m0");
  else if (SC1)
    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off sc1" ::"s"(lds), "v"(gptr) : "memory", "m0");
  else
    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds), "v"(gptr) : "memory", "m0");
}

// A kernel-argument pointer re-read inside a loop: hipcc would otherwise hoist
// every per-lane address derived from it out of the step / layer loops and keep
// dozens of them live (VGPR spills); through this opaque copy they are recomputed
// where used (a few VALU each).
template <class T>
DEV T* hl_opaque(T* p) {
  asm volatile("" : "+s"(p));
  return p;
}
DEV int hl_vopaque(int v) {   // the same for a per-lane value
  asm volatile("" : "+v"(v));
  return v;
}

// element (row j, column k) of an MFMA-packed [N][K] weight (weights.py mfma_pack):
// the 16-byte chunk holding columns k .. k+7 (k % 8 == 0)
DEV const bf16* hl_packed(const bf16* w, int K, int j, int k) {
  return w + ((long long)((j >> 4) * (K >> 5) + (k >> 5)) * 64 + (j & 15) + 16 * ((k & 31) >> 3)) * 8;
}

// diagnostic time stamp k of workgroup `slot` (16 words each), by thread tid_sel
// (I: int or unsigned, as the kernel indexed before -- the extension of slot * 16 + k)
template <class I>
DEV void hl_stamp(unsigned long long* stamps, I slot, int k, int tid_sel) {
  if (stamps && threadIdx.x == tid_sel) stamps[slot * 16 + k] = __builtin_amdgcn_s_memrealtime();
}

// ------------------------------------------------------------------ shared arithmetic
// What the one-launch kernels (k_lm_ffn, k_lm_ffn16, k_head_m16, k_head_fin,
// k_lm_attn) must compute to the GEMV path's bits, written once.  What stays per
// kernel: the DMA issue order, the s_waitcnt counts, the LDS maps, and -- because
// a helper compiled to other instructions there -- the row inverse-RMS loop
// (gemv_dev.h row_inv's order), the D-tile index, the act store loop and the
// workgroup-to-tile maps.
//
// xform<XF_NORM> over `rows` rows of H bf16 in LDS at stride XST, in place
// (gemv_dev.h norm8): norm weight nw_s [H] (HAS_W), adaLN scale / shift rows sc_s /
// sh_s at stride mod_stride (HAS_MOD), inverse RMS inv_s[m].  ZERO_TAIL: rows
// [rows, 16) are zeroed (MFMA operand rows that are read).
template <int H, bool HAS_W, bool HAS_MOD, bool ZERO_TAIL = false>
DEV void hl_rows_norm(bf16* xs, int XST, int rows, const bf16* nw_s, const bf16* sc_s, const bf16* sh_s, int mod_stride,
                      const float* inv_s, int tid, int NT) {
  constexpr int NCH = H / 8;
  for (int e = tid; e < (ZERO_TAIL ? 16 : rows) * NCH; e += NT) {
    const int m = e / NCH, c = e - m * NCH;
    bf16x8 o;
    if (!ZERO_TAIL || m < rows) {
      const bf16x8 xv = *(const bf16x8*)(xs + m * XST + c * 8);
      const bf16x8 none = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};   // an absent operand (never read)
      const bf16x8 wv = HAS_W ? *(const bf16x8*)(nw_s + c * 8) : none;
      const bf16x8 shv = HAS_MOD ? *(const bf16x8*)(sh_s + m * mod_stride + c * 8) : none;
      const bf16x8 scv = HAS_MOD ? *(const bf16x8*)(sc_s + m * mod_stride + c * 8) : none;
      o = norm8<HAS_W, HAS_MOD>(xv, inv_s[m], wv, scv, shv);
    } else {
      o = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    }
    *(bf16x8*)(xs + m * XST + c * 8) = o;
  }
}
// (SiLU(gate) * up from the fp32 sums: gemv_dev.h silu_up)

// One grid-wide wait: arrival of this workgroup + poll until k waits of this
// launch have completed.  Lane 0 of the control wave (or of the wave that made
// the workgroup's last store), behind that wave's own s_waitcnt vmcnt(0).  The
// arrival adds to this workgroup's XCD shard counter (w % 8: 32 workgroups
// each); a shard's 32nd arrival of a wait bumps the kernel's generation word at
// `line` (sync_layout.h: only that kernel bumps it; the shard lines are shared),
// so one wait completes when the generation has advanced by 8.  Two chained
// device-scope atomics before the release.  Measured against (DESIGN.md
// "Persistent head"): polling all 256 per-workgroup flags (2x slower: 256
// pollers sweeping the same lines) and polling the 8 shard counters without the
// generation word (one atomic per wait, but 8 lines per poll: 755 -> 774 us per
// head sample).  Counters are monotonic across launches and compared wrap-safe.
//
// The launch's base generation, read at entry: the word moves 8 per wait, so it
// is a multiple of 8 between launches.  A workgroup reading it at entry may see
// up to 7 bumps of the first wait (other shards complete it; its own cannot):
// base = word rounded down to 8.
DEV unsigned hl_base_gen(unsigned* sync, int line) {
  return __hip_atomic_load((hl_gu32*)(sync + line * pk::LINE), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) &
         ~(unsigned)(pk::SHARDS - 1);
}
// arrival of workgroup w
DEV void hl_arrive(unsigned* sync, int line, int w) {
  using namespace pk;
  const unsigned v = __hip_atomic_fetch_add((hl_gu32*)(sync + (w & (SHARDS - 1)) * LINE), 1u, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
  if ((v + 1) % (G / SHARDS) == 0)
    __hip_atomic_fetch_add((hl_gu32*)(sync + line * LINE), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// poll word 0 of `line` until it has advanced by `adv` from g0 (k grid waits:
// adv = SHARDS * k); false: gave up after ~200 ms (error word set).  (A/B builds,
// tools/ab_lib.sh: two polls in flight half a round trip apart, or s_sleep 4
// between polls: B = 1 within +-0.01 ms of this one-at-a-time loop.  Polling by
// scalar loads that miss the scalar cache was tried: the hand-offs took 11-20 us
// instead of 1.4-3.)
DEV bool hl_poll(unsigned* sync, int line, unsigned g0, unsigned adv, unsigned* err) {
  hl_gu32* word = (hl_gu32*)(sync + line * pk::LINE);
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while ((unsigned)(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - g0) < adv) {
    __builtin_amdgcn_s_sleep(1);
    if (__builtin_amdgcn_s_memrealtime() - t0 > 20000000ull) {   // ~200 ms at 100 MHz
      __hip_atomic_store((hl_gu32*)err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
  }
  return true;
}
// arrive + poll until k waits of this launch (base generation g0) have completed
DEV bool hl_grid_wait(unsigned* sync, int line, unsigned g0, unsigned k, int w, unsigned* err) {
  hl_arrive(sync, line, w);
  return hl_poll(sync, line, g0, pk::SHARDS * k, err);
}
