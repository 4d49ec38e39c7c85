// FP8 (OCP e4m3fn) weight-only GEMV for gfx950, M <= 16 rows:
//   Y[m, n] = epi( 2^e[n] * sum_k xf(A)[m, k] * code[n, k] )
//
// Weight-only storage of the LM projections (vibevoice_amd/weights.py,
// quantize_rows_e4m3): one e4m3 code per element and one int8 exponent per
// output row, scale = 2^e[n].  Both the e4m3 -> bf16 conversion and the
// power-of-two scale are exact, so the products are those of a bf16 GEMV on the
// dequantised matrix; only the fp32 summation order differs.
//
// Layout ("mfma_pack8", weights.py): the codes [N, K] (K % 64 == 0) in the tile
// and lane mapping of mfma_pack (gemm.hip), two 32-column chunks per block so a
// lane's piece is 16 bytes: block (tile t, chunk pair p) of 16 rows x 64
// columns is 1 KB contiguous at (t * K/64 + p) * 1024 bytes, lane l's 16 bytes
// at l * 16 =
//   W[16t + (l & 15)][64p      + 8(l >> 4) .. +7]   (bytes 0..7,  chunk 2p)
//   W[16t + (l & 15)][64p + 32 + 8(l >> 4) .. +7]   (bytes 8..15, chunk 2p + 1)
// -- each half is exactly the lane's MFMA 16x16x32 A fragment of that chunk, and
// every wave load is one coalesced 1 KB read.
//
// Kernel form (the "GEMV / M <= 16" row the bf16 family follows): one workgroup
// per 16-row weight tile, up to 8 waves splitting K.  The A rows (transformed:
// XF_NONE or XF_NORM) are staged once in LDS; each wave streams its chunk pairs
// with 16-byte non-temporal loads, two batches of W8_U pairs ping-ponged (8 KB
// per wave in flight), converts e4m3 -> f32 -> bf16 in registers, runs two MFMA
// 16x16x32 bf16 per pair with W as the A operand, and the waves' partial tiles
// are summed through LDS in wave order.  The sum is multiplied by 2^e[n] before
// the bias and epilogue (gemv_dev.h epi_tile, unchanged).  Rows longer than the
// LDS budget (M x K bf16 > 96 KB, e.g. 16 rows of K = 18,944) are staged in K
// blocks, with a barrier between blocks.
//
// More than 16 rows: the bf16 kernels that serve them read the codes themselves
// (gemm.hip, their W8 instantiations; gemm_decide's w8_native) -- k_gemv<2..4>
// and k_gemvw (17 to 64 rows), k_gemm<64 / 32> (65 to 255 rows, and any row
// count with a transform), with every transform they are built for.  A lane
// loads its 16 code bytes of a chunk pair (8 where a wave's K range cuts a
// pair) and converts them in registers to code * 2^e[n] (cvt8s, common.h): the
// bf16 values the dequantise pass would store, fed to the same MFMA sequence,
// partition, reductions and epilogue -- bit for bit the bf16 kernel on the
// dequantised matrix, with no dequantise pass (vv_w8_dequant_launches stands
// still).  vv_gemm_plan_w8 answers where a shape goes.
//
// What is left takes the fallback: k_dequant_w8 writes the matrix as bf16 in
// mfma_pack order into a scratch buffer and the bf16 launch runs on it -- bit
// for bit a bf16 engine holding the dequantised weights.  That is: up to 16
// rows in a form k_gemv_w8 does not serve (adaLN operands, SiLU-add, the codec
// mixer, the attention merge, k_gemv<1>); the LDS-staged prefill tiles
// k_gemm_big / k_gemm_xl (>= 256 plain rows: one dequantise over hundreds of
// rows); K % 64 != 0; and every quantised GEMM under vv_gemv_w8(0).
#include <algorithm>
#include <atomic>

#include "kernels.h"
#include "gemv_dev.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int W8_U = 4;                  // chunk pairs (KB) per batch per wave; two batches in flight
constexpr int W8_MAX_WAVES = 8;
constexpr size_t W8_LDS_MAX = 98304;     // A rows staged per K block (dynamic LDS, opt-in above 64 KB)

// the code stream: ldw8; the K ranges: k_slice (gemv_dev.h); e4m3 -> bf16: cvt8 (common.h)

// kbp: chunk pairs per K block (host: M * (64 kbp + 8) * 2 bytes of dynamic LDS)
template <int XF>
__global__ void __launch_bounds__(64 * W8_MAX_WAVES) k_gemv_w8(GemmArgs a, int kbp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float inv_s[16];
  __shared__ float red[W8_MAX_WAVES * 256];
  const int NT = blockDim.x, NW = NT >> 6;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x;
  const int npair = a.K >> 6;
  const unsigned char* wrow = a.w8 + (long long)tile * a.K * 16 + lane * 16;
  bf16* xs = (bf16*)smem;
  const bool plain = !a.a.idx;
  if (XF == XF_NORM) {   // whole-row inverse RMS (k_rmsnorm's summation order), before any K block
    row_inv(a, 0, a.M, inv_s, wave, NW, lane);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
  const u32x4 zero4 = (u32x4){0u, 0u, 0u, 0u};
  for (int pb = 0; pb < npair; pb += kbp) {
    const int np = min(kbp, npair - pb);
    // this wave's chunk pairs [c0, c1) of the block
    const KRange kr = k_slice(pb, pb + np, wave, NW);
    const int c0 = kr.c0, c1 = kr.c1;
    const int kw = np * 64, lds_ld = kw + 8, n8 = kw >> 3, ne = a.M * n8;
    u32x4 wa[W8_U] = {zero4, zero4, zero4, zero4}, wb[W8_U] = {zero4, zero4, zero4, zero4};
    // loads past the wave's range are skipped (wave-uniform test): a repeated
    // non-temporal read would be a second trip to HBM
    auto load = [&](u32x4 (&wf)[W8_U], int c) {
#pragma unroll
      for (int u = 0; u < W8_U; ++u)
        if (c + u < c1) wf[u] = ldw8(wrow + (long long)(c + u) * 1024);
    };
    if (pb) __syncthreads();   // the previous block's fragment reads are done
    // ---- A staging (rows [0, M) x this block's columns, row stride padded 16 B):
    // the first batch of A loads is issued ahead of the first weight batch, so
    // the transform waits only for its own bytes (vmcnt counts in issue order)
    for (int e0 = threadIdx.x, it = 0; it == 0 || e0 < ne; e0 += 4 * NT, ++it) {
      bf16x8 xv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {   // unconditional loads, items past the end re-read the last
        const int e = min(e0 + q * NT, ne - 1);
        const int m = e / n8, k8 = (e - m * n8) * 8;
        xv[q] = *(const bf16x8*)((plain ? rm_bf_plain(a.a, m) : rm_bf(a.a, m)) + pb * 64 + k8);
      }
      if (it == 0) load(wa, c0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = e0 + q * NT;
        if (e < ne) {
          const int m = e / n8, k8 = (e - m * n8) * 8;
          *(bf16x8*)(xs + m * lds_ld + k8) = xform<XF>(a, xv[q], m, pb * 64 + k8, XF == XF_NORM ? inv_s[m] : 0.f);
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    // B fragments: lanes of rows >= M read row M - 1 (columns the epilogue drops)
    const bf16* xrow = xs + min(r, a.M - 1) * lds_ld + 8 * g - pb * 64;
    auto compute = [&](u32x4 (&wf)[W8_U], int c) {
      bf16x8 x0[W8_U], x1[W8_U];
#pragma unroll
      for (int u = 0; u < W8_U; ++u) {
        const int pc = min(c + u, c1 - 1);
        x0[u] = *(const bf16x8*)(xrow + pc * 64);
        x1[u] = *(const bf16x8*)(xrow + pc * 64 + 32);
      }
#pragma unroll
      for (int u = 0; u < W8_U; ++u) {
        const u32x4 w = c + u < c1 ? wf[u] : zero4;
        acc = mfma(cvt8(w[0], w[1]), x0[u], acc);
        acc = mfma(cvt8(w[2], w[3]), x1[u], acc);
      }
    };
    for (int c = c0; c < c1; c += 2 * W8_U) {
      load(wb, c + W8_U);
      compute(wa, c);
      load(wa, c + 2 * W8_U);
      compute(wb, c + W8_U);
    }
  }

  // ---- K-slice waves summed in wave order, then scale, bias and epilogue
#pragma unroll
  for (int i = 0; i < 4; ++i) red[(wave * 4 + i) * 64 + lane] = acc[i];
  __syncthreads();
  if (wave == 0) {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s = red[i * 64 + lane];
      for (int w = 1; w < NW; ++w) s += red[(w * 4 + i) * 64 + lane];
      v[i] = s;
    }
    // lane holds output columns n0 + 4g + i: their exponents are one aligned dword
    const int n0 = tile * 16;
    const unsigned ev = *(const unsigned*)(a.w8e + n0 + 4 * g);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = ldexpf(v[i], (int)(signed char)(ev >> (8 * i)));
    epi_tile(a, r, n0, lane, v);
  }
}

// codes (mfma_pack8) -> bf16 (mfma_pack): one thread per lane piece of 16 codes
__global__ void __launch_bounds__(256) k_dequant_w8(const unsigned char* codes, const signed char* ex, bf16* out,
                                                    int K, long long nitem) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nitem) return;
  const int lane = (int)(i & 63), npair = K >> 6;
  const long long blk = i >> 6;
  const long long t = blk / npair;
  const int p = (int)(blk - t * npair);
  const u32x4 v = *(const u32x4*)(codes + i * 16);
  const int e = ex[16 * t + (lane & 15)];
  bf16x8 w0 = cvt8(v[0], v[1]), w1 = cvt8(v[2], v[3]);
#pragma unroll
  for (int j = 0; j < 8; ++j) {   // a power-of-two scale of a 4-bit significand: exact in bf16
    w0[j] = tobf(ldexpf(bf(w0[j]), e));
    w1[j] = tobf(ldexpf(bf(w1[j]), e));
  }
  bf16* o = out + (t * (K >> 5) + 2 * p) * 512 + lane * 8;
  *(bf16x8*)o = w0;
  *(bf16x8*)(o + 512) = w1;
}

static std::atomic<int> g_gemv_w8{1};   // diagnostic (vv_gemv_w8): 0 = every quantised GEMM takes the fallback
extern "C" int vv_gemv_w8(int on) {
  g_gemv_w8 = on ? 1 : 0;
  return 0;
}
bool gemv_w8_enabled() { return g_gemv_w8 != 0; }
static std::atomic<unsigned> g_dequant_launches{0};   // diagnostic: k_dequant_w8 launches of this process
extern "C" int vv_w8_dequant_launches() { return (int)(g_dequant_launches.load(std::memory_order_relaxed) & 0x7fffffffu); }

bool gemv_w8_serves(const GemmArgs& a) {
  if (!g_gemv_w8 || !a.w8 || !a.w8e || a.M < 1 || a.M > 16 || a.K % 64 || a.N % 16 || a.apack || a.epi.pack) return false;
  if (a.xf.kind != XF_NONE && !(a.xf.kind == XF_NORM && !a.xf.mod)) return false;
  const int e = a.epi.kind;
  return e == EPI_STORE || e == EPI_GELU || e == EPI_SILU_MUL || e == EPI_RES || e == EPI_F32 || e == EPI_ROPE;
}

int launch_gemv_w8(const GemmArgs& a, hipStream_t st) {
  const int npair = a.K / 64;
  int kbp = npair;
  while ((size_t)a.M * (kbp * 64 + 8) * 2 > W8_LDS_MAX) kbp = (kbp + 1) / 2;
  const size_t lds = (size_t)a.M * (kbp * 64 + 8) * 2;
  const int nw = std::min(W8_MAX_WAVES, std::max(1, (kbp + 1) / 2));
  // > 64 KB of dynamic LDS needs the opt-in; once, thread-safe
  static const bool attr =
      hipFuncSetAttribute((const void*)k_gemv_w8<XF_NONE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)W8_LDS_MAX) ==
          hipSuccess &&
      hipFuncSetAttribute((const void*)k_gemv_w8<XF_NORM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)W8_LDS_MAX) ==
          hipSuccess;
  if (!attr) return 2;
  const dim3 grid(a.N / 16), block(64 * nw);
  if (a.xf.kind == XF_NORM) hipLaunchKernelGGL((k_gemv_w8<XF_NORM>), grid, block, lds, st, a, kbp);
  else hipLaunchKernelGGL((k_gemv_w8<XF_NONE>), grid, block, lds, st, a, kbp);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

int launch_dequant_w8(const unsigned char* codes, const signed char* ex, bf16* out, int N, int K, hipStream_t st) {
  if (N % 16 || K % 64 || !codes || !ex || !out) return 1;
  const long long nitem = (long long)N * K / 16;
  g_dequant_launches.fetch_add(1, std::memory_order_relaxed);
  hipLaunchKernelGGL(k_dequant_w8, dim3((unsigned)((nitem + 255) / 256)), dim3(256), 0, st, codes, ex, out, K, nitem);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
