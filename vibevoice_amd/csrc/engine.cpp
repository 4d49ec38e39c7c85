// libvibevoice_hip.so — native engine for VibeVoice's generate loop on MI355X.
//
// Owns: borrowed weight pointers, the compacted LM KV cache, per-slot streaming
// conv state of the acoustic decoder and semantic encoder, workspaces, and the
// diffusion schedule.  Every entry point only enqueues kernels on the caller's
// stream (no host sync, no allocation after vv_finalize except the grow-only
// prefill / voice-prompt workspaces).  C ABI: include/vibevoice_hip.h.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/vibevoice_hip_diag.h"
#include "kernels.h"
#include "sync_layout.h"

static thread_local std::string g_err;

#define FAIL(msg)        \
  do {                   \
    g_err = (msg);       \
    return -1;           \
  } while (0)
#define HIPCHK(x)                                                                 \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      g_err = std::string(#x) + ": " + hipGetErrorString(e_);                     \
      return -1;                                                                  \
    }                                                                             \
  } while (0)
#define KCHK(x)                                                                   \
  do {                                                                            \
    int r_ = (x);                                                                 \
    if (r_) {                                                                     \
      g_err = std::string("kernel launch rejected (") + std::to_string(r_) + "): " + #x; \
      return -1;                                                                  \
    }                                                                             \
  } while (0)
#define CHK(x)          \
  do {                  \
    if ((x) != 0) return -1; \
  } while (0)

namespace {

struct Weight {
  const void* p = nullptr;
  std::vector<int64_t> shape;
};

// Per-slot conv input buffer: [ctx history rows | rows of this step (+ zero pad)] x C
struct ConvBuf {
  bf16* base = nullptr;
  long long sB = 0;  // elements per slot
  int ctx = 0, T = 0, C = 0, rows = 0;
};

// Bumped whenever a workspace moves: a hipGraph captured earlier bakes the old
// pointers in, so the host drops its graphs when this changes (vv_ws_epoch).
static std::atomic<int> g_ws_epoch{0};
// Contexts per device that may run the one-launch kernels with grid-wide waits
// (k_lm_ffn, k_head_m16, k_codec_stage*: one workgroup per CU).  Two such
// launches from two contexts cannot be resident together, so they run only while
// ONE finalized context of the device is registered; a change of that count bumps
// the epoch, so hosts re-capture graphs that baked in the other path.  Contexts
// of OTHER processes are invisible here: a shared-GPU deployment turns the
// kernels off (VIBEVOICE_PERSISTENT=0 or vv_set_persistent).
static std::mutex g_hl_mu;
static std::map<int, int> g_hl_ctxs;
static void hl_register(int device, int delta) {
  std::lock_guard<std::mutex> lk(g_hl_mu);
  const int before = g_hl_ctxs[device];
  const int after = before + delta;
  g_hl_ctxs[device] = after;
  if ((before == 1) != (after == 1) || (before <= 2) != (after <= 2)) g_ws_epoch.fetch_add(1);
}
static int hl_count(int device) {
  std::lock_guard<std::mutex> lk(g_hl_mu);
  auto it = g_hl_ctxs.find(device);
  return it == g_hl_ctxs.end() ? 0 : it->second;
}

// Process default for new contexts: VIBEVOICE_PERSISTENT=0 in the environment
// turns the grid-waiting kernels off (e.g. several processes sharing one GPU).
static bool persist_env_default() {
  static const bool on = [] {
    const char* e = getenv("VIBEVOICE_PERSISTENT");
    return !(e && e[0] == '0');
  }();
  return on;
}

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int ensure(size_t b) {
    if (b <= bytes) return 0;
    if (p) g_ws_epoch.fetch_add(1);
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    if (hipMalloc(&p, b) != hipSuccess) {
      g_err = "hipMalloc failed (" + std::to_string(b) + " bytes)";
      return -1;
    }
    bytes = b;
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// One causal conv stack of the σ-VAE codec (acoustic decoder, or an encoder),
// laid out for `slots` sample slots and `T0` input rows per call.
struct ConvNet {
  bool decoder = true;
  std::string wp;             // weight-name prefix: "dec", "sem", "aenc"
  int nst = 0;
  int depth[VV_MAX_STAGES] = {}, chans[VV_MAX_STAGES] = {}, rat[VV_MAX_STAGES] = {}, T[VV_MAX_STAGES] = {};
  int in_ch = 0, out_ch = 0, T0 = 0, slots = 0, nmax = 0;
  int Tin[VV_MAX_STAGES] = {};  // rows entering the strided conv before stage i (encoder)
  ConvBuf stem, head;
  std::vector<std::vector<ConvBuf>> mix;
  ConvBuf tr[VV_MAX_STAGES];
  DevBuf state;               // all ConvBufs
  DevBuf work;                // X stages + A + F
  bf16* X[VV_MAX_STAGES] = {};
  bf16* Y[VV_MAX_STAGES] = {};   // residual ping-pong partner of X (k_mix output)
  bf16* A = nullptr;
  bf16* F = nullptr;
  std::vector<RollDesc> rolls;
  DevBuf d_rolls;
  // weights, resolved by convnet_check (vv_finalize); tr_w[i] / tr_b[i]: the transition before stage i
  const bf16 *stem_w = nullptr, *stem_b = nullptr, *head_w = nullptr, *head_b = nullptr;
  const bf16 *tr_w[VV_MAX_STAGES] = {}, *tr_b[VV_MAX_STAGES] = {};
  std::vector<std::vector<Block1D>> blk;   // [stage][block]: weights + the conv buffer mix[stage][block] (convnet_alloc)
};

// An LM projection's weight operand: the bf16 matrix, or the FP8 codes + row exponents
struct LmW {
  const bf16* w = nullptr;
  const unsigned char* w8 = nullptr;
  const signed char* w8e = nullptr;
};
// The resolved weight table (vv_ctx: lm, lmw, head, headw, conn_ac, conn_se, scaling;
// ConvNet: stem, head, tr, blk): vv_finalize fills each entry in the need() call that
// checks the name's presence and shape, and every later call reads the table only
struct LmLayerW {
  const bf16 *in_norm = nullptr, *qkv_b = nullptr, *post_norm = nullptr;
  LmW qkv, o, gu, down;
};
struct HeadLayerW { const bf16 *norm = nullptr, *gu = nullptr, *down = nullptr; };
struct ConnW { const bf16 *fc1_w = nullptr, *fc1_b = nullptr, *norm = nullptr, *fc2_w = nullptr, *fc2_b = nullptr; };

}  // namespace

// diagnostic: attention launches record per-workgroup timestamps (nullptr: off)
static std::atomic<unsigned long long*> g_attn_stamps{nullptr};
extern "C" int vv_attn_stamps(void* buf) {
  g_attn_stamps = (unsigned long long*)buf;
  return 0;
}

struct vv_ctx {
  vv_config cfg;
  int device = 0;
  std::unordered_map<std::string, Weight> w;   // vv_bind_weight -> vv_finalize only
  bool finalized = false;
  // the resolved weights (vv_finalize)
  struct {
    const bf16 *embed = nullptr, *lm_head = nullptr, *norm = nullptr;
    const float* inv_freq = nullptr;
  } lm;
  std::vector<LmLayerW> lmw;
  struct {
    const bf16 *noisy = nullptr, *cond = nullptr, *t0 = nullptr, *t2 = nullptr, *ada = nullptr, *final = nullptr;
  } head;
  std::vector<HeadLayerW> headw;
  ConnW conn_ac, conn_se;
  const bf16 *scaling = nullptr, *bias = nullptr;   // speech_scaling_factor, speech_bias_factor
  bool has_aenc = false;                            // the optional acoustic encoder (aenc.*) is bound
  // LM
  int qkv_n = 0, lm_slots = 0;
  DevBuf kv_k, kv_v;
  KVLayout kv;
  DevBuf lm_ws;  // h, a, qkv, q, att, act
  size_t lm_ws_tokens = 0;
  DevBuf attn_part, attn_cnt;
  DevBuf norm_ws;   // pre-normalised A rows of XF_NORM GEMMs with > 16 rows
  DevBuf valid_ids;
  int n_valid = 0;
  // split-K
  DevBuf splitk_ws, splitk_cnt;
  // diffusion
  int steps = 0;
  std::vector<DpmCoef> coef;
  DevBuf temb, tfreq_tmp;
  DevBuf head_ws;
  // codec
  ConvNet dec, sem, aenc;
  ConvNet senc;     // the semantic encoder laid out for one non-streaming call (vv_semantic_encode)
  DevBuf codec_ws;  // connectors
  DevBuf slot_scratch;
  DevBuf unit_sb;   // bf16 {1, 0}: identity scaling / bias for vv_codec_decode
  // tensor parallelism of the LM (Megatron split, configuration_vibevoice.py:175-183):
  // this engine holds rank tp_rank's shard; the residual stream is all-reduced
  // after o_proj and down_proj
  int tp_rank = 0, tp_size = 1;
  int head_tp = 0;      // 1: the diffusion head's FFN is sharded too (vv_tp_shard_head; head_ffn is local)
  ncclComm_t comm = nullptr;
  DevBuf zero_rows;     // [2 * max_batch][H] zeros: the residual of a sharded head's rank > 0
  DevBuf hf_sync;   // head_m16.hip's wait counters + every grid-waiting kernel's error word (layout: sync_layout.h)
  DevBuf lf_sync;   // lm_ffn.hip's wait counters (+ k_lm_ffn16's column-group tickets)
  DevBuf lf_slab;   // k_lm_ffn16's down partials [48][4][16][32] fp32
  DevBuf la_part;   // k_lm_attn's per-unit attention partials (lm_attn_part_floats)
  DevBuf m16_buf;   // head_m16.hip's distributed A side: row partial sums of squares [16][192] f32 + rows [16][H]
  DevBuf cs_sync;          // persistent codec stage (codec_stage.hip): its wait counters
  DevBuf cw_sync;          // wide codec stages (codec_wide.hip): one counter line per cluster, per C
  DevBuf cw_slab, cw_xbuf; // ... their partial slabs and block outputs
  bool persist_ok = true;       // this context may run one-launch (grid-waiting) kernels (vv_set_persistent)
  bool persist_capable = false; // some grid-waiting kernel fits this engine's shapes (vv_finalize)
  bool persist_follow = false;  // unregistered, runs them while exactly one context is registered (vv_set_persistent 2)
  bool hl_registered = false;   // counted in g_hl_ctxs (its device's grid-waiting contexts)
  bool head_gemv = true;        // the head FFN's GEMV layout is bound (head.<l>.gu_w / down_w)
  DevBuf rope_tab;   // [max_ctx][cos 64 | sin 64] bf16 (k_rope_table)
  // FP8 weight-only LM projections (gemv_w8.hip): bound as <name>8 (e4m3 codes,
  // mfma_pack8 order) + <name>e (int8 row exponents) instead of the bf16 <name>
  bool quantized = false;
  // the MLP projections (gu_w, down_w of every layer), decided once at vv_finalize: the
  // one-launch MLP kernels read one form throughout, a mixed binding keeps the GEMV pair
  enum { MLP_BF16 = 0, MLP_W8 = 1, MLP_MIXED = 2 };
  int mlp_form = MLP_BF16;
  // the attention projections (qkv_w, o_w of every layer), decided the same way: k_lm_attn reads
  // one form throughout (MLP_* values).  Its W8 form is this context's option
  // (vv_set_lm_attn_w8 before vv_finalize, default off: an FP8 engine runs the three launches)
  int attn_form = MLP_BF16;
  int lm_attn_w8 = 0;
  // ... and its FP8-KV form (k_lm_attn<., 1>: the rows quantised inside the launch) is this
  // context's option too (vv_set_lm_attn_kv8 before vv_finalize, default off: an FP8-KV engine
  // runs q|k|v, k_kv_quant, k_attn, o_proj)
  int lm_attn_kv8 = 0;
  // the longest pass (keys) the one-launch attention kernel is planned for (vv_set_lm_attn_max_keys before
  // vv_finalize; default LA_MAX_KEYS: the short form only, three launches past it)
  int lm_attn_max_keys = LA_MAX_KEYS;
  // the most rows of a decode pass the kernel is planned for (vv_set_lm_attn_max_rows before vv_finalize;
  // default LA_ROWS: the 16-row class only, three launches above it; bf16 KV above 16 rows)
  int lm_attn_max_rows = LA_ROWS;
  DevBuf w8_scratch; // one dequantised matrix (the largest), bf16: the fallback of launch_gemm
  // FP8 (e4m3) KV cache (kv_fp8.hip; vv_set_kv_dtype before vv_finalize): codes + row
  // exponents instead of kv_k / kv_v; kv keeps the strides (elements) and max_ctx
  int kv_dtype = 0;
  DevBuf kv8_k, kv8_v, kv8_ek, kv8_ev;
  KV8 kv8 = {nullptr, nullptr, nullptr, nullptr};
  // the staged append of a pass: a one-slot bf16 cache over the pass's token indices
  // (K | V), the cos / sin rows of the tokens' real positions, and the slot (all 0) /
  // position (0, 1, ...) tables the q|k|v epilogue indexes it with.  (Every engine has the
  // decode-pass-sized one: k_lm_attn's KVQ forms stage their rows in it, the diagnostic
  // round trip vv_lm_attn_kvround on a bf16 cache included; it is no part of vv_kv_bytes.)
  DevBuf kv_stage;
  size_t kv_stage_tokens = 0;
  KVLayout stg = {nullptr, nullptr, 0, 0, 0, 0, 0};
  bf16* stg_cs = nullptr;
  int *stg_slot = nullptr, *stg_pos = nullptr;
};

// ------------------------------------------------------------------ helpers
static std::vector<DevBuf*> sync_bufs(vv_ctx* c) { return {&c->hf_sync, &c->cs_sync, &c->lf_sync}; }   // sync_layout.h's layout
static unsigned* err_word(vv_ctx* c) { return (unsigned*)c->hf_sync.p + pk::ERR * pk::LINE; }

// vv_finalize's one lookup: weight `n` is bound with this shape ({}: any), and its
// pointer goes to the table entry *slot -- nothing is resolved unchecked
template <class T>
static int need(vv_ctx* c, const std::string& n, const std::vector<int64_t>& shape, const T** slot) {
  auto it = c->w.find(n);
  if (it == c->w.end()) FAIL("missing weight: " + n);
  if (!shape.empty() && it->second.shape != shape) {
    std::string s = "shape mismatch for " + n + ": got [";
    for (auto v : it->second.shape) s += std::to_string(v) + ",";
    s += "] want [";
    for (auto v : shape) s += std::to_string(v) + ",";
    FAIL(s + "]");
  }
  *slot = (const T*)it->second.p;
  return 0;
}

// vv_finalize: the projection is bound either as bf16 `n` [N][K] or as the pair `n`8 [N][K] + `n`e [N]
static int need_lm_w(vv_ctx* c, const std::string& n, int64_t N, int64_t K, LmW* slot) {
  const bool b = c->w.count(n) > 0, q = c->w.count(n + "8") > 0, e = c->w.count(n + "e") > 0;
  if (b && (q || e)) FAIL("weight " + n + " is bound both as bf16 and as FP8 (" + n + "8 / " + n + "e)");
  if (b) return need(c, n, {N, K}, &slot->w);
  if (!q && !e) FAIL("missing weight: " + n + " (bf16), or its FP8 pair " + n + "8 (codes) + " + n + "e (exponents)");
  if (!q) FAIL("missing weight: " + n + "8 (FP8 codes; only the exponents " + n + "e are bound)");
  if (!e) FAIL("missing weight: " + n + "e (FP8 row exponents; only the codes " + n + "8 are bound)");
  if (K % 64) FAIL("FP8 weight " + n + "8: K = " + std::to_string(K) + " is not a multiple of 64");
  if (c->tp_size > 1 || c->comm) FAIL("FP8 weights (" + n + "8) are not supported on a tensor-parallel engine");
  CHK(need(c, n + "8", {N, K}, &slot->w8));
  CHK(need(c, n + "e", {N}, &slot->w8e));
  c->quantized = true;
  return 0;
}

// The staging cache for passes of up to ntok tokens (FP8 KV; grown outside a hot
// call only: vv_finalize sizes it for a decode pass, a longer prefill grows it and
// bumps the workspace epoch through DevBuf::ensure)
static int kv_stage_ensure(vv_ctx* c, size_t ntok) {
  if (ntok <= c->kv_stage_tokens) return 0;
  const size_t cap = (ntok + 31) / 32 * 32, d = 128, nkv = c->cfg.n_kv_heads;
  const size_t kv_elems = nkv * cap * d;
  CHK(c->kv_stage.ensure((2 * kv_elems + cap * d) * sizeof(bf16) + 2 * cap * sizeof(int)));
  c->kv_stage_tokens = cap;
  c->stg.k = (bf16*)c->kv_stage.p;
  c->stg.v = c->stg.k + kv_elems;
  c->stg.d = (int)d;
  c->stg.max_ctx = (int)cap;
  c->stg.s_head = (long long)(cap * d);
  c->stg.s_slot = c->stg.s_head * (long long)nkv;
  c->stg.s_layer = 0;
  c->stg_cs = c->stg.v + kv_elems;
  c->stg_slot = (int*)(c->stg_cs + cap * d);
  c->stg_pos = c->stg_slot + cap;
  return 0;
}

static GemmArgs gemm_args(vv_ctx* c, int M, int N, int K, RowMap a, const bf16* w, int epi, RowMap out,
                          const bf16* bias = nullptr) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.M = M;
  g.N = N;
  g.K = K;
  g.ksplit = 1;
  g.a = a;
  g.w = w;
  g.ldw = K;
  g.epi.kind = epi;
  g.epi.bias = bias;
  g.epi.out = out;
  g.ws = (float*)c->splitk_ws.p;
  g.counters = (unsigned*)c->splitk_cnt.p;
  return g;
}
static GemmArgs gemm_args(vv_ctx* c, int M, int N, int K, RowMap a, const LmW& w, int epi, RowMap out,
                          const bf16* bias = nullptr) {
  GemmArgs g = gemm_args(c, M, N, K, a, w.w, epi, out, bias);
  g.w8 = w.w8;
  g.w8e = w.w8e;
  g.w8_scratch = (bf16*)c->w8_scratch.p;
  return g;
}

static ATransform xf_norm(const bf16* w, float eps, const bf16* mod = nullptr, long long mod_ld = 0, int shift_off = 0,
                          int scale_off = 0) {
  ATransform x;
  memset(&x, 0, sizeof(x));
  x.kind = XF_NORM;
  x.eps = eps;
  x.w = w;
  x.mod = mod;
  x.mod_ld = mod_ld;
  x.shift_off = shift_off;
  x.scale_off = scale_off;
  return x;
}

static int rmsnorm(int M, int C, RowMap in, RowMap out, const bf16* w, float eps, hipStream_t st,
                   const bf16* mod = nullptr, long long mod_ld = 0, int shift_off = 0, int scale_off = 0,
                   int pack = 0);

// test switch (vv_norm_pack): 1 = the normalised rows feeding a 256 x 256-tile
// GEMM are written MFMA-fragment-packed (16K-token gate|up 1055 -> 948 us, q|k|v
// 98 -> 92: one contiguous 1 KB load per A block instead of 16 row pieces)
static std::atomic<int> g_norm_pack{1};
extern "C" int vv_norm_pack(int on) {
  g_norm_pack = on;
  return 0;
}

static int gemm(vv_ctx* c, GemmArgs g, hipStream_t st) {
  if (!g.w && !g.w8) FAIL("gemm: null weight");
  if (g.xf.kind == XF_NORM && g.M > 16) {
    // more rows than one MFMA tile: the GEMV / GEMM kernels would re-normalise
    // the A block in every workgroup (B = 32: LM gate|up 334 us); normalise it
    // once (k_rmsnorm: the same arithmetic and summation order, bit-identical)
    GemmArgs probe = g;
    probe.xf.kind = XF_NONE;
    const int pack = g_norm_pack && g.K % 32 == 0 && gemm_uses_xl(probe) ? 1 : 0;
    CHK(c->norm_ws.ensure((size_t)(g.M + 15) / 16 * 16 * g.K * sizeof(bf16)));
    CHK(rmsnorm(g.M, g.K, g.a, rowmap(c->norm_ws.p, g.K), g.xf.w, g.xf.eps, st, g.xf.mod, g.xf.mod_ld,
                g.xf.shift_off, g.xf.scale_off, pack));
    g.a = rowmap(c->norm_ws.p, g.K);
    g.apack = pack;
    g.xf.kind = XF_NONE;
  }
  KCHK(launch_gemm(g, st));
  return 0;
}

static int rmsnorm(int M, int C, RowMap in, RowMap out, const bf16* w, float eps, hipStream_t st,
                   const bf16* mod, long long mod_ld, int shift_off, int scale_off, int pack) {
  NormArgs a;
  memset(&a, 0, sizeof(a));
  a.pack = pack;
  a.M = M;
  a.C = C;
  a.eps = eps;
  a.in = in;
  a.out = out;
  a.w = w;
  a.has_mod = mod != nullptr;
  a.mod = mod;
  a.mod_ld = mod_ld;
  a.shift_off = shift_off;
  a.scale_off = scale_off;
  KCHK(launch_rmsnorm(a, st));
  return 0;
}

// ------------------------------------------------------------------ grid-waiting kernels
// The context half of the decision every one-launch (grid-waiting) kernel takes
// before its launch; the kernel half is its *_fits (shape + persist_resident on
// the occupancy query).  Both halves are vv_persist_decision for the tests.
static bool persist_ctx_ok(int enabled, int contexts_on_device) { return enabled && contexts_on_device == 1; }
static bool persist_on(vv_ctx* c) {
  return persist_ctx_ok(c->persist_ok && (c->hl_registered || c->persist_follow) ? 1 : 0, hl_count(c->device));
}
extern "C" int vv_persist_decision(int blocks_per_cu, int cus, int scratch_bytes, int grid, int contexts_on_device,
                                   int enabled) {
  return persist_resident(blocks_per_cu, cus, scratch_bytes, grid) && persist_ctx_ok(enabled, contexts_on_device) ? 1
                                                                                                                   : 0;
}

// ------------------------------------------------------------------ codec layout
static void convnet_shape(vv_ctx* c, ConvNet& n, bool decoder, const std::string& wp, int nf, int in_ch, int out_ch,
                          int T0, int slots) {
  const vv_config& k = c->cfg;
  n.decoder = decoder;
  n.wp = wp;
  n.nst = k.n_stages;
  n.in_ch = in_ch;
  n.out_ch = out_ch;
  n.T0 = T0;
  n.slots = slots;
  n.nmax = slots;
  for (int i = 0; i < n.nst; ++i) {
    if (decoder) {
      n.depth[i] = k.dec_depths[i];
      n.chans[i] = nf << (n.nst - 1 - i);
      n.rat[i] = i == 0 ? 1 : k.ratios[i - 1];
      n.T[i] = i == 0 ? T0 : n.T[i - 1] * n.rat[i];
      n.Tin[i] = i == 0 ? T0 : n.T[i - 1];
    } else {
      n.depth[i] = k.enc_depths[i];
      n.chans[i] = nf << i;
      n.rat[i] = i == 0 ? 1 : k.ratios[n.nst - 1 - i];  // encoder ratios are reversed
      n.Tin[i] = i == 0 ? T0 : n.T[i - 1];
      n.T[i] = i == 0 ? T0 : (n.T[i - 1] + n.rat[i] - 1) / n.rat[i];
    }
  }
}

static int convnet_alloc(ConvNet& n, int kernel) {
  // layout the per-slot buffers
  std::vector<ConvBuf*> all;
  size_t total = 0;
  auto add = [&](ConvBuf& b, int ctx, int T, int rows_pad, int C) {
    b.ctx = ctx;
    b.T = T;
    b.C = C;
    b.rows = ctx + rows_pad;
    b.sB = (long long)b.rows * C;
    all.push_back(&b);
    total += (size_t)b.sB * n.slots;
  };
  add(n.stem, kernel - 1, n.T0, n.T0, n.in_ch);
  n.mix.assign(n.nst, {});
  for (int i = 0; i < n.nst; ++i) {
    if (i > 0) {
      if (n.decoder) {
        add(n.tr[i], 1, n.Tin[i], n.Tin[i], n.chans[i - 1]);
      } else {
        const int s = n.rat[i];
        add(n.tr[i], s, n.Tin[i], n.T[i] * s, n.chans[i - 1]);
      }
    }
    n.mix[i].resize(n.depth[i]);
    for (int j = 0; j < n.depth[i]; ++j) add(n.mix[i][j], kernel - 1, n.T[i], n.T[i], n.chans[i]);
  }
  add(n.head, kernel - 1, n.T[n.nst - 1], n.T[n.nst - 1], n.chans[n.nst - 1]);
  CHK(n.state.ensure(total * sizeof(bf16)));
  HIPCHK(hipMemset(n.state.p, 0, total * sizeof(bf16)));
  bf16* p = (bf16*)n.state.p;
  n.rolls.clear();
  for (ConvBuf* b : all) {
    b->base = p;
    p += (size_t)b->sB * n.slots;
    RollDesc r;
    r.base = b->base;
    r.sB = b->sB;
    r.ctx = b->ctx;
    r.T = b->T;
    r.C = b->C;
    r.pad_ = 0;
    n.rolls.push_back(r);
  }
  for (int i = 0; i < n.nst; ++i)
    for (int j = 0; j < n.depth[i]; ++j) {
      n.blk[i][j].mix = n.mix[i][j].base;
      n.blk[i][j].mix_sB = n.mix[i][j].sB;
    }
  CHK(n.d_rolls.ensure(n.rolls.size() * sizeof(RollDesc)));
  HIPCHK(hipMemcpy(n.d_rolls.p, n.rolls.data(), n.rolls.size() * sizeof(RollDesc), hipMemcpyHostToDevice));
  // transient work: X per stage + A (normed rows) + F (ffn hidden)
  size_t xw = 0, aw = 0, fw = 0;
  for (int i = 0; i < n.nst; ++i) {
    xw += (size_t)n.T[i] * n.chans[i];
    aw = std::max(aw, (size_t)n.T[i] * n.chans[i]);
    fw = std::max(fw, (size_t)n.T[i] * n.chans[i] * 4);
  }
  const size_t per = 2 * xw + aw + fw;
  CHK(n.work.ensure(per * n.nmax * sizeof(bf16)));
  bf16* q = (bf16*)n.work.p;
  for (int i = 0; i < n.nst; ++i) {
    n.X[i] = q;
    q += (size_t)n.T[i] * n.chans[i] * n.nmax;
    n.Y[i] = q;
    q += (size_t)n.T[i] * n.chans[i] * n.nmax;
  }
  n.A = q;
  q += aw * n.nmax;
  n.F = q;
  return 0;
}

// vv_finalize: the net's weights, checked and resolved (the shapes depend on the
// channels only, so the table holds when vv_*_encode lays the net out again)
static int convnet_check(vv_ctx* c, ConvNet& n) {
  const std::string& p = n.wp;
  const int k = 7;
  if (n.decoder) {
    CHK(need(c, p + ".stem_w", {n.chans[0], (int64_t)k * n.in_ch}, &n.stem_w));
  } else {
    CHK(need(c, p + ".stem_w", {n.chans[0], (int64_t)k}, &n.stem_w));
  }
  CHK(need(c, p + ".stem_b", {n.chans[0]}, &n.stem_b));
  n.blk.assign(n.nst, {});
  for (int i = 0; i < n.nst; ++i) {
    const int C = n.chans[i];
    if (i > 0) {
      const std::string t = p + ".tr" + std::to_string(i);
      const int Ci = n.chans[i - 1], r = n.rat[i];
      if (n.decoder) {
        CHK(need(c, t + "_w", {(int64_t)r * C, 2LL * Ci}, &n.tr_w[i]));
        CHK(need(c, t + "_b", {(int64_t)r * C}, &n.tr_b[i]));
      } else {
        CHK(need(c, t + "_w", {C, 2LL * r * Ci}, &n.tr_w[i]));
        CHK(need(c, t + "_b", {C}, &n.tr_b[i]));
      }
    }
    n.blk[i].assign(n.depth[i], Block1D{});
    for (int j = 0; j < n.depth[i]; ++j) {
      const std::string b = p + ".s" + std::to_string(i) + ".b" + std::to_string(j);
      Block1D& B = n.blk[i][j];
      CHK(need(c, b + ".norm", {C}, &B.norm));
      CHK(need(c, b + ".dw_w", {C, k}, &B.dw_w));
      CHK(need(c, b + ".dw_b", {C}, &B.dw_b));
      CHK(need(c, b + ".gamma", {C}, &B.gamma));
      CHK(need(c, b + ".ffn_norm", {C}, &B.ffn_norm));
      CHK(need(c, b + ".fc1_w", {4LL * C, C}, &B.fc1_w));
      CHK(need(c, b + ".fc1_b", {4LL * C}, &B.fc1_b));
      CHK(need(c, b + ".fc2_w", {C, 4LL * C}, &B.fc2_w));
      CHK(need(c, b + ".fc2_b", {C}, &B.fc2_b));
      CHK(need(c, b + ".ffn_gamma", {C}, &B.ffn_gamma));
    }
  }
  const int Cl = n.chans[n.nst - 1];
  if (n.decoder) {
    CHK(need(c, p + ".head_w", {k, Cl}, &n.head_w));
    CHK(need(c, p + ".head_b", {1}, &n.head_b));
  } else {
    CHK(need(c, p + ".head_w", {n.out_ch, (int64_t)k * Cl}, &n.head_w));
    CHK(need(c, p + ".head_b", {n.out_ch}, &n.head_b));
  }
  return 0;
}

// Rows of ConvBuf b, starting after its history, for the active samples (slot map).
static RowMap buf_in_rows(const ConvBuf& b, int T, const int* slots) {
  return rowmap(b.base + (long long)b.ctx * b.C, b.C, T, b.sB, slots);
}

// Codec Block1D front half folded into fc1's prologue where it fits (XF_MIX);
// off only for the bit-exactness test against the k_mix path.
static std::atomic<int> g_mix_fusion{3};   // bit 0: XF_MIX, bit 1: k_block
extern "C" int vv_codec_mix_fusion(int mask) {
  g_mix_fusion = mask & 3;
  return 0;
}

// A codec stage of Block1Ds of one sample (C = 2,048 at T = 1, C = 1,024 at
// T = 2 / 8) runs as ONE persistent launch (codec_stage.hip) while the context is the device's only one registered for
// persistent kernels (persist_on); 0 = the launch-per-GEMV path (A/B and tests).
static std::atomic<int> g_codec_stage{1};
// Bits 1..3 pick how the C = 2,048 form issues its weight stream (A/B only):
// 0 = the default, the split, paced stream (CodecStageArgs::pubfirst 5); v > 0 =
// pubfirst v - 1 (1: round 5's whole-block stream at each block's end).
extern "C" int vv_codec_stage(int on) {
  g_codec_stage = on & 15;
  return 0;
}
static std::atomic<unsigned long long*> g_codec_stage_stamps{nullptr};
static std::atomic<int> g_codec_stage_stamp_at{0};
// diagnostic: the acoustic decoder's stage `stage` records [256][64] per-workgroup phase stamps
extern "C" int vv_codec_stage_stamps(void* buf, int stage) {
  g_codec_stage_stamps = (unsigned long long*)buf;
  g_codec_stage_stamp_at = stage;
  return 0;
}
// The narrow stages (C <= 128) as ONE launch each (codec_tile.hip: transition
// conv + three Block1Ds [+ the decoder's head conv], halo recomputed per
// workgroup); 0 = k_block per Block1D + the transition GEMMs (A/B and tests).
static std::atomic<int> g_codec_tile{1};
extern "C" int vv_codec_tile(int on) {
  g_codec_tile = on ? 1 : 0;
  return 0;
}
// diagnostic: tile launches record [n][tiles][16] phase stamps at buf + 4096 x (3 x net + stage index among
// the tiled stages) (net 0 decoder, 1 encoders); nullptr: off
static std::atomic<unsigned long long*> g_codec_tile_stamps{nullptr};
extern "C" int vv_codec_tile_stamps(void* buf) {
  g_codec_tile_stamps = (unsigned long long*)buf;
  return 0;
}
// The wide stages (C = 256 / 512) as ONE launch each (codec_wide.hip: clusters of
// C / 32 workgroups per 16-row tile) under the grid-waiting kernels' rule
// (persist_on: the launch's workgroups must be co-resident); 0 = k_mix + fc1 /
// fc2 GEMMs per Block1D (A/B and tests).
static std::atomic<int> g_codec_wide{1};
extern "C" int vv_codec_wide(int on) {
  g_codec_wide = on ? 1 : 0;
  return 0;
}
extern "C" int vv_codec_wide_over(int on) {   // diagnostic: 1 = grids past one resident wave too (B = 8)
  codec_wide_oversubscribe(on);
  return 0;
}
static std::atomic<unsigned long long*> g_codec_wide_stamps{nullptr};
extern "C" int vv_codec_wide_stamps(void* buf) {   // diagnostic: [n][tiles x S][16] at buf + 8192 x (2 x net + (C == 512))
  g_codec_wide_stamps = (unsigned long long*)buf;
  return 0;
}
// ------------------------------------------------------------------ codec plan
// One StagePlan per stage of a convnet_run call; the routes in priority order (DESIGN.md "How a codec step picks its kernels")
enum { CR_TILE = 0, CR_WIDE = 1, CR_STAGE = 2, CR_BLOCKS = 3, CR_GEMMS = 4 };
struct CodecSw { int stage, wide, tile, fusion, persist; };                     // the four switches, persist_on
struct CodecShape { int decoder, i, nst, C, T, depth, ctx, rat, Cn, in_ch; };   // (Cn: stage i - 1's channels)
struct CodecFits { bool tile, wide, stage, block, mix; };
// pre / post: CT_PRE_* / CT_POST_* inside a tile launch; own_pre: the transition before the stage (stage 0: the stem) is
// a launch of its own; xf_mix (CR_GEMMS): the mixer in fc1's prologue, not k_mix; R (CR_BLOCKS / CR_GEMMS): rows per
// mixer workgroup (R * C / 8 = 256 conv items: one per thread)
struct StagePlan { int route, pre, post, own_pre, xf_mix, R; };
// a plan record of ints as the diag exports' words
template <class P>
static int* put_words(const P& p, int* out) {
  memcpy(out, &p, sizeof(P));
  return out + sizeof(P) / sizeof(int);
}
static int mixer_rows(int T, int C) { return std::max(1, std::min(T, 2048 / C)); }
// the transition and the head conv a tile launch of the stage would fuse
static void codec_tile_ends(const CodecShape& s, int& pre, int& post) {
  pre = CT_PRE_NONE;
  if (s.decoder && s.i > 0 && s.rat == 2 && s.Cn == 2 * s.C) pre = CT_PRE_CONVT;
  if (!s.decoder && s.i > 0 && s.rat == 2 && 2 * s.Cn == s.C) pre = CT_PRE_SCONV;
  if (!s.decoder && s.i == 0 && s.in_ch == 1) pre = CT_PRE_STEM;
  post = s.decoder && s.i == s.nst - 1 ? CT_POST_HEAD : CT_POST_NONE;
}
// The ordering, from plain values (vv_diag_codec_route); f: the five *_fits / *_lds answers at this call's n
static StagePlan codec_route(const CodecSw& w, const CodecShape& s, const CodecFits& f) {
  StagePlan p{CR_GEMMS, CT_PRE_NONE, CT_POST_NONE, 1, 0, 0};
  const bool tile = w.tile && !(s.decoder && s.i == 0) && f.tile;   // (the decoder's stem stage is the widest)
  p.route = tile ? CR_TILE : w.wide && w.persist && f.wide ? CR_WIDE : w.stage && w.persist && f.stage ? CR_STAGE
            : (w.fusion & 2) && f.block ? CR_BLOCKS : CR_GEMMS;
  if (tile) codec_tile_ends(s, p.pre, p.post);
  p.own_pre = s.i == 0 ? p.pre != CT_PRE_STEM : p.pre != CT_PRE_CONVT && p.pre != CT_PRE_SCONV;
  p.xf_mix = p.route == CR_GEMMS && (w.fusion & 1) && f.mix;
  if (p.route >= CR_BLOCKS) p.R = mixer_rows(s.T, s.C);
  return p;
}
extern "C" int vv_diag_codec_route(int stage, int wide, int tile, int fusion, int persist, int decoder, int i, int nst,
                                   int C, int T, int depth, int ctx, int rat, int Cn, int in_ch, int fit_tile,
                                   int fit_wide, int fit_stage, int fit_block, int fit_mix, int* out) {
  if (!out || C < 1) return 1;
  put_words(codec_route({stage, wide, tile, fusion, persist}, {decoder, i, nst, C, T, depth, ctx, rat, Cn, in_ch},
                        {fit_tile != 0, fit_wide != 0, fit_stage != 0, fit_block != 0, fit_mix != 0}), out);
  return 0;
}
struct CodecPlan {
  StagePlan st[VV_MAX_STAGES];
  int nst;
  bool own_head() const { return st[nst - 1].post != CT_POST_HEAD; }   // the head conv is a launch of its own
  bool any(int route) const { return std::any_of(st, st + nst, [&](const StagePlan& p) { return p.route == route; }); }
  bool grid_waiting() const { return any(CR_STAGE) || any(CR_WIDE); }   // (one sample, ever: vv_finalize's registry count)
};
// Per call, not at vv_finalize: the switches and persist_on change between calls (a captured graph replays its capture's
// plan).  ever: what could run at all -- every switch on, persist_on assumed.  The device-touching part is the five fit
// answers; the cluster kernel's one sync line per cluster (n x tiles <= pk::CW_LINES) is tested here and nowhere else.
static CodecPlan codec_plan(vv_ctx* c, const ConvNet& net, int n, bool ever = false) {
  const CodecSw w = ever ? CodecSw{1, 1, 1, 3, 1}
                         : CodecSw{g_codec_stage.load(), g_codec_wide.load(), g_codec_tile.load(), g_mix_fusion.load(), persist_on(c)};
  CodecPlan P{};
  P.nst = net.nst;
  for (int i = 0; i < net.nst; ++i) {
    const int C = net.chans[i], T = net.T[i], depth = net.depth[i], ctx = net.mix[i].empty() ? 0 : net.mix[i][0].ctx;
    const CodecShape s{net.decoder, i, net.nst, C, T, depth, ctx, net.rat[i], i > 0 ? net.chans[i - 1] : 0, net.in_ch};
    int pre, post;
    codec_tile_ends(s, pre, post);
    P.st[i] = codec_route(w, s, {codec_tile_fits(C, pre, post, depth, ctx),
                                 n * ((T + 15) / 16) <= pk::CW_LINES && codec_wide_fits(C, T, n, depth, ctx),
                                 codec_stage_fits(C, T, n, depth), block_lds(mixer_rows(T, C), C) != 0,
                                 gemv_mix_lds(n * T, T, C) != 0});
  }
  return P;
}
// test queries: a one-sample step runs the acoustic decoder's stage 0 persistent / an n-sample step some stage of it wide now
extern "C" int vv_codec_stage_active(vv_ctx* c) { return c && c->finalized && codec_plan(c, c->dec, 1).st[0].route == CR_STAGE; }
extern "C" int vv_codec_wide_active(vv_ctx* c, int n) { return c && c->finalized && codec_plan(c, c->dec, n).any(CR_WIDE); }
// diagnostic: the plan of a step of n samples now; out = {nst, own_head, then per stage vv_diag_codec_route's six}
extern "C" int vv_diag_codec_plan(vv_ctx* c, int net, int n, int* out, int cap) {
  if (!c || !c->finalized || !out || n < 1 || (net != 0 && net != 1)) FAIL("vv_diag_codec_plan: bad arguments");
  const CodecPlan P = codec_plan(c, net == 0 ? c->dec : c->sem, n);
  if (cap < 2 + 6 * P.nst) FAIL("vv_diag_codec_plan: out[] too short (" + std::to_string(2 + 6 * P.nst) + " words)");
  *out++ = P.nst;
  *out++ = P.own_head();
  for (int i = 0; i < P.nst; ++i) out = put_words(P.st[i], out);
  return 0;
}

// diffusion steps whose adaLN modulations are computed in one GEMM
static constexpr int HEAD_SC = 16;

// ------------------------------------------------------------------ codec run
// Stage i of one convnet_run call: n samples (slots[n]) of T rows x C channels
struct StageRun {
  ConvNet& net;
  int i, n, T, C;
  const int* slots;
  float eps;
  RowMap out;   // the last block's output rows: the next transition's input rows, or the head conv's
  hipStream_t st;
  StagePlan p;
};

// A Block1D record into the launch-per-block kernels' argument structs
static void set_block(MixArgs& m, const Block1D& b) {
  m.buf = b.mix;
  m.buf_sB = b.mix_sB;
  m.norm_w = b.norm;
  m.dw_w = b.dw_w;
  m.dw_b = b.dw_b;
  m.gamma = b.gamma;
  m.ffn_norm_w = b.ffn_norm;
}
static void set_block(ATransform& x, const Block1D& b) {
  x.buf = b.mix;
  x.buf_sB = b.mix_sB;
  x.w = b.norm;
  x.dw_w = b.dw_w;
  x.dw_b = b.dw_b;
  x.gamma = b.gamma;
  x.ffn_w = b.ffn_norm;
}
static void set_block(BlockArgs& a, const Block1D& b) {   // (a.mix: mix_args)
  a.w1 = b.fc1_w;
  a.b1 = b.fc1_b;
  a.w2 = b.fc2_w;
  a.b2 = b.fc2_b;
  a.g2 = b.ffn_gamma;
}
// block j's front half (k_mix, k_block) but for its x / y / a rows
static MixArgs mix_args(const StageRun& s, int j) {
  MixArgs mx;
  memset(&mx, 0, sizeof(mx));
  mx.n = s.n;
  mx.T = s.T;
  mx.C = s.C;
  mx.R = s.p.R;
  mx.eps = s.eps;
  mx.ctx = s.net.mix[s.i][j].ctx;
  mx.slots = s.slots;
  set_block(mx, s.net.blk[s.i][j]);
  return mx;
}

// the stem conv: stem rows -> X[0]
static int convnet_stem(vv_ctx* c, ConvNet& net, int n, const int* slots, hipStream_t st) {
  const int T = net.T[0], C = net.chans[0], k = 7;
  RowMap xo = rowmap(net.X[0], C, T, (long long)T * C);
  if (net.decoder) {
    RowMap a = rowmap(net.stem.base, net.stem.C, T, net.stem.sB, slots);
    return gemm(c, gemm_args(c, n * T, C, k * net.in_ch, a, net.stem_w, EPI_STORE, xo, net.stem_b), st);
  }
  ConvIn1Args a{n * T, C, k, rowmap(net.stem.base, 1, T, net.stem.sB, slots), net.stem_w, net.stem_b, xo};
  KCHK(launch_conv_cin1(a, st));
  return 0;
}

// the transition conv before stage i: tr[i] rows -> X[i]
static int convnet_transition(vv_ctx* c, ConvNet& net, int i, int n, const int* slots, hipStream_t st) {
  const ConvBuf& tb = net.tr[i];
  const int T = net.T[i], C = net.chans[i], Ci = net.chans[i - 1], r = net.rat[i];
  if (net.decoder) {
    // 2-tap ConvTranspose: input row t = buffer rows [t, t+1] (1 history row)
    RowMap a = rowmap(tb.base, Ci, net.Tin[i], tb.sB, slots);
    RowMap o = rowmap(net.X[i], (long long)r * C, net.Tin[i], (long long)T * C);
    return gemm(c, gemm_args(c, n * net.Tin[i], r * C, 2 * Ci, a, net.tr_w[i], EPI_STORE, o, net.tr_b[i]), st);
  }
  // strided causal conv, k = 2r, ctx = r: output row t = buffer rows [t*r, t*r + 2r)
  RowMap a = rowmap(tb.base, (long long)r * Ci, T, tb.sB, slots);
  RowMap X = rowmap(net.X[i], C, T, (long long)T * C);
  return gemm(c, gemm_args(c, n * T, C, 2 * r * Ci, a, net.tr_w[i], EPI_STORE, X, net.tr_b[i]), st);
}

// the head conv (disable_last_norm: no final norm, modular_vibevoice_tokenizer.py:908-911)
static int convnet_head(vv_ctx* c, ConvNet& net, int n, const int* slots, RowMap out, RowMap out2, hipStream_t st) {
  const int Tl = net.T[net.nst - 1], Cl = net.chans[net.nst - 1], k = 7;
  RowMap a = rowmap(net.head.base, Cl, Tl, net.head.sB, slots);
  if (!net.decoder) return gemm(c, gemm_args(c, n * Tl, net.out_ch, k * Cl, a, net.head_w, EPI_STORE, out, net.head_b), st);
  Conv1Args h{n * Tl, Cl, k, a, net.head_w, net.head_b, out, out2};
  KCHK(launch_conv_cout1(h, st));
  return 0;
}

// what the tile and the cluster launch's arguments share
template <class A>
static A stage_args(const StageRun& s) {
  A a;
  memset(&a, 0, sizeof(a));
  a.n = s.n;
  a.T = s.T;
  a.depth = s.net.depth[s.i];
  a.eps = s.eps;
  a.slots = s.slots;
  a.x = s.net.X[s.i];
  for (int j = 0; j < a.depth; ++j) a.b[j] = s.net.blk[s.i][j];
  return a;
}

// the whole narrow stage in one launch (codec_tile.hip): + the transition s.p.pre
// before it and, with CT_POST_HEAD, the decoder's head conv (-> audio, audio2)
static int stage_tile(const StageRun& s, RowMap audio, RowMap audio2) {
  ConvNet& net = s.net;
  const int pre = s.p.pre, post = s.p.post;
  CodecTileArgs A = stage_args<CodecTileArgs>(s);
  if (pre != CT_PRE_NONE) {
    const bool stem = pre == CT_PRE_STEM;
    const ConvBuf& pb = stem ? net.stem : net.tr[s.i];
    A.pre_buf = pb.base;
    A.pre_sB = pb.sB;
    A.pre_w = stem ? net.stem_w : net.tr_w[s.i];
    A.pre_b = stem ? net.stem_b : net.tr_b[s.i];
  }
  if (post == CT_POST_HEAD) {
    A.head_w = net.head_w;
    A.head_b = net.head_b;
    A.head_buf = net.head.base;
    A.head_sB = net.head.sB;
    A.audio = audio;
    A.audio2 = audio2;
  } else {
    A.out = s.out;
  }
  const int C = s.C;
  if (unsigned long long* sp = g_codec_tile_stamps.load())
    A.stamps = sp + 4096 * (3 * (net.decoder ? 0 : 1) + (C == 128 ? (net.decoder ? 0 : 2) : C == 64 ? 1 : (net.decoder ? 2 : 0)));
  KCHK(launch_codec_tile(A, C, pre, post, s.st));
  return 0;
}

// the whole wide stage in one launch of clusters (codec_wide.hip)
static int stage_wide(vv_ctx* c, const StageRun& s) {
  ConvNet& net = s.net;
  const int C = s.C;
  CodecWideArgs A = stage_args<CodecWideArgs>(s);
  A.out = s.out;
  CHK(c->cw_slab.ensure(codec_wide_slab_floats(C, s.T, s.n) * sizeof(float)));
  CHK(c->cw_xbuf.ensure(codec_wide_xbuf_elems(C, s.T, s.n) * sizeof(bf16)));
  A.sync = (unsigned*)c->cw_sync.p + (C == 512 ? pk::CW_HALF : 0);
  A.err = err_word(c);
  A.slab = (float*)c->cw_slab.p;
  A.xbuf = (bf16*)c->cw_xbuf.p;
  if (unsigned long long* sp = g_codec_wide_stamps.load()) A.stamps = sp + 8192 * (2 * (net.decoder ? 0 : 1) + (C == 512));
  const int rc = launch_codec_wide(A, C, s.st);
  if (rc) FAIL("wide codec stage: launch failed (" + std::to_string(rc) + ")");
  return 0;
}

// the whole stage (one sample) in one persistent launch (codec_stage.hip)
static int stage_persistent(vv_ctx* c, const StageRun& s) {
  ConvNet& net = s.net;
  CodecStageArgs A;
  memset(&A, 0, sizeof(A));
  A.depth = net.depth[s.i];
  A.ctx = net.mix[s.i][0].ctx;
  A.C = s.C;
  A.M = s.T;
  A.eps = s.eps;
  A.slots = s.slots;
  A.x = net.X[s.i];
  A.xe = net.Y[s.i];
  A.h = net.F;
  A.out = s.out;
  for (int j = 0; j < net.depth[s.i]; ++j) {
    A.b[j] = net.blk[s.i][j];
    if (net.mix[s.i][j].ctx != A.ctx) FAIL("codec stage: conv buffers of one stage differ in history length");
  }
  A.sync = (unsigned*)c->cs_sync.p;
  A.err = err_word(c);
  A.stamps = net.decoder && s.i == g_codec_stage_stamp_at ? g_codec_stage_stamps.load() : nullptr;
  const int v = (g_codec_stage.load() >> 1) & 7;
  A.pubfirst = v ? v - 1 : 5;
  const int rc = launch_codec_stage(A, s.st);
  if (rc) FAIL("persistent codec stage: launch failed (" + std::to_string(rc) + ": " +
               hipGetErrorString(hipGetLastError()) + ")");
  return 0;
}

// narrow stage: each Block1D is one k_block launch; the residual ping-pongs
// X -> Y -> X (a workgroup reads halo rows other workgroups own)
static int stage_blocks(const StageRun& s) {
  ConvNet& net = s.net;
  const int i = s.i;
  for (int j = 0; j < net.depth[i]; ++j) {
    BlockArgs ba;
    memset(&ba, 0, sizeof(ba));
    ba.mix = mix_args(s, j);
    ba.mix.x = (j & 1) ? net.Y[i] : net.X[i];
    set_block(ba, net.blk[i][j]);
    ba.out = j == net.depth[i] - 1 ? s.out : rowmap((j & 1) ? net.X[i] : net.Y[i], s.C, s.T, (long long)s.T * s.C);
    KCHK(launch_block(ba, s.st));
  }
  return 0;
}

// per Block1D: the front half (k_mix, or fc1's prologue), fc1 and fc2 GEMMs
static int stage_gemms(vv_ctx* c, const StageRun& s) {
  ConvNet& net = s.net;
  const int i = s.i, n = s.n, T = s.T, C = s.C;
  RowMap X = rowmap(net.X[i], C, T, (long long)T * C);
  RowMap Y = rowmap(net.Y[i], C, T, (long long)T * C);
  RowMap Fm = rowmap(net.F, 4LL * C);
  for (int j = 0; j < net.depth[i]; ++j) {
    const Block1D& B = net.blk[i][j];
    if (s.p.xf_mix) {
      // few rows (T = 1, 8 stages at small batch): the mix runs in fc1's prologue
      GemmArgs g = gemm_args(c, n * T, 4 * C, C, X, B.fc1_w, EPI_GELU, Fm, B.fc1_b);
      g.xf.kind = XF_MIX;
      g.xf.eps = s.eps;
      g.xf.T = T;
      g.xf.ctx = net.mix[i][j].ctx;
      g.xf.slots = s.slots;
      set_block(g.xf, B);
      g.xf.y = net.Y[i];
      CHK(gemm(c, g, s.st));
    } else {
      // mixer norm + depthwise conv + gamma residual (X -> Y) + ffn_norm (-> A), one launch
      MixArgs mx = mix_args(s, j);
      mx.x = net.X[i];
      mx.y = net.Y[i];
      mx.a = net.A;
      KCHK(launch_mix(mx, s.st));
      CHK(gemm(c, gemm_args(c, n * T, 4 * C, C, rowmap(net.A, C), B.fc1_w, EPI_GELU, Fm, B.fc1_b), s.st));
    }
    GemmArgs g = gemm_args(c, n * T, C, 4 * C, Fm, B.fc2_w, EPI_RES, j == net.depth[i] - 1 ? s.out : X, B.fc2_b);
    g.epi.res = Y;
    g.epi.gamma = B.ffn_gamma;
    CHK(gemm(c, g, s.st));
  }
  return 0;
}

// One block stack + transitions.  n active samples (slots[n]); input rows already
// in `stem` (rows [ctx, ctx+T0)).  Decoder: writes audio to out (+ out2).
// Encoder: writes [n, out_ch] features to out.
static int convnet_run(vv_ctx* c, ConvNet& net, int n, const int* slots, RowMap out, RowMap out2, hipStream_t st) {
  const CodecPlan P = codec_plan(c, net, n);
  for (int i = 0; i < net.nst; ++i) {
    const StagePlan& p = P.st[i];
    // (the encoders' stem and the 2x transitions are fused into the stage's tile launch where it applies)
    if (p.own_pre) CHK(i == 0 ? convnet_stem(c, net, n, slots, st) : convnet_transition(c, net, i, n, slots, st));
    const ConvBuf& nb = (i + 1 < net.nst) ? net.tr[i + 1] : net.head;
    const StageRun s{net, i, n, net.T[i], net.chans[i], slots, c->cfg.codec_eps, buf_in_rows(nb, net.T[i], slots), st, p};
    switch (p.route) {
      case CR_TILE: CHK(stage_tile(s, out, out2)); break;
      case CR_WIDE: CHK(stage_wide(c, s)); break;
      case CR_STAGE: CHK(stage_persistent(c, s)); break;
      case CR_BLOCKS: CHK(stage_blocks(s)); break;
      default: CHK(stage_gemms(c, s));
    }
  }
  if (P.own_head()) CHK(convnet_head(c, net, n, slots, out, out2, st));
  return 0;
}

static int convnet_roll(ConvNet& net, int n, const int* slots, int mode, hipStream_t st) {
  KCHK(launch_roll((const RollDesc*)net.d_rolls.p, (int)net.rolls.size(), slots, n, mode, st));
  return 0;
}

// ------------------------------------------------------------------ C ABI
extern "C" {

const char* vv_last_error(void) { return g_err.c_str(); }
int vv_ws_epoch(void) { return g_ws_epoch.load(); }

int vv_create(const vv_config* cfg, int device, vv_ctx** out) {
  if (!cfg || !out) FAIL("vv_create: null argument");
  if (cfg->head_dim != 128) FAIL("head_dim must be 128");
  if (cfg->n_stages < 1 || cfg->n_stages > VV_MAX_STAGES) FAIL("n_stages out of range");
  if (cfg->n_heads % cfg->n_kv_heads || cfg->n_heads / cfg->n_kv_heads > 8) FAIL("unsupported GQA ratio");
  if (cfg->max_batch < 1 || cfg->max_batch > 32) FAIL("max_batch must be in [1, 32]");
  HIPCHK(hipSetDevice(device));
  vv_ctx* c = new vv_ctx();
  c->cfg = *cfg;
  c->device = device;
  c->persist_ok = persist_env_default();
  *out = c;
  return 0;
}

void vv_destroy(vv_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  if (c->hl_registered) hl_register(c->device, -1);
  DevBuf* bufs[] = {&c->norm_ws, &c->kv_k, &c->kv_v, &c->lm_ws, &c->attn_part, &c->attn_cnt, &c->valid_ids, &c->splitk_ws, &c->splitk_cnt,
                    &c->temb, &c->tfreq_tmp, &c->head_ws, &c->codec_ws, &c->slot_scratch, &c->unit_sb,
                    &c->rope_tab, &c->zero_rows, &c->hf_sync, &c->cs_sync, &c->m16_buf, &c->lf_sync,
                    &c->cw_sync, &c->cw_slab, &c->cw_xbuf, &c->lf_slab, &c->la_part, &c->w8_scratch,
                    &c->kv8_k, &c->kv8_v, &c->kv8_ek, &c->kv8_ev, &c->kv_stage};
  for (DevBuf* b : bufs) b->release();
  ConvNet* nets[] = {&c->dec, &c->sem, &c->aenc, &c->senc};
  for (ConvNet* n : nets) {
    n->state.release();
    n->work.release();
    n->d_rolls.release();
  }
  if (c->comm) (void)ncclCommDestroy(c->comm);
  delete c;
}

int vv_bind_weight(vv_ctx* c, const char* name, const void* p, const int64_t* shape, int ndim) {
  if (!c || !name || !p) FAIL("vv_bind_weight: null argument");
  if (c->finalized)
    FAIL(std::string("vv_bind_weight(") + name + ") after vv_finalize: the weight table is resolved (and captured graphs hold its pointers)");
  Weight w;
  w.p = p;
  w.shape.assign(shape, shape + ndim);
  c->w[name] = w;
  return 0;
}

// What every option setter refuses first: a null context, a call after vv_finalize (`why`: what is settled by
// then) and, with no_tp, a tensor-parallel engine.
static int option_guard(vv_ctx* c, const std::string& fn, const char* why, bool no_tp) {
  if (!c) FAIL(fn + ": null context");
  if (c->finalized) FAIL(fn + " after vv_finalize: " + why);
  if (no_tp && (c->tp_size > 1 || c->comm)) FAIL(fn + " is not supported on a tensor-parallel engine");
  return 0;
}
static const char* const LA_CHOSEN = "the attention half's kernels are already chosen";
int vv_set_kv_dtype(vv_ctx* c, int dtype) {
  CHK(option_guard(c, "vv_set_kv_dtype", "the KV cache is already allocated", false));
  if (dtype != 0 && dtype != 1)
    FAIL("vv_set_kv_dtype: unsupported dtype " + std::to_string(dtype) + " (0 = bf16, 1 = fp8 e4m3)");
  if (dtype && (c->tp_size > 1 || c->comm)) FAIL("an FP8 KV cache is not supported on a tensor-parallel engine");
  c->kv_dtype = dtype;
  return 0;
}
int vv_kv_dtype(vv_ctx* c) { return c ? c->kv_dtype : 0; }
// (the two on / off options; they leave refusing a tensor-parallel engine to their callers)
static int set_lm_attn_flag(vv_ctx* c, const std::string& fn, int on, int vv_ctx::*opt) {
  if (on != 0 && on != 1) FAIL(fn + ": unsupported value " + std::to_string(on) + " (0 = off, 1 = on)");
  CHK(option_guard(c, fn, LA_CHOSEN, false));
  c->*opt = on;
  return 0;
}
int vv_set_lm_attn_w8(vv_ctx* c, int on) { return set_lm_attn_flag(c, "vv_set_lm_attn_w8", on, &vv_ctx::lm_attn_w8); }
int vv_lm_attn_w8(vv_ctx* c) { return c ? c->lm_attn_w8 : 0; }
int vv_set_lm_attn_kv8(vv_ctx* c, int on) { return set_lm_attn_flag(c, "vv_set_lm_attn_kv8", on, &vv_ctx::lm_attn_kv8); }
int vv_lm_attn_kv8(vv_ctx* c) { return c ? c->lm_attn_kv8 : 0; }
int vv_set_lm_attn_max_keys(vv_ctx* c, int keys) {
  CHK(option_guard(c, "vv_set_lm_attn_max_keys", LA_CHOSEN, true));
  const int hi = std::min(c->cfg.max_ctx, LA_LONG_MAX_KEYS);
  if (keys < LA_MAX_KEYS || keys > hi)
    FAIL("vv_set_lm_attn_max_keys: " + std::to_string(keys) + " is outside [" + std::to_string(LA_MAX_KEYS) + ", " +
         std::to_string(hi) + "] (4,096 .. the engine's max_ctx)");
  c->lm_attn_max_keys = keys;
  return 0;
}
int vv_lm_attn_max_keys(vv_ctx* c) { return c ? c->lm_attn_max_keys : 0; }
int vv_set_lm_attn_max_rows(vv_ctx* c, int rows) {
  CHK(option_guard(c, "vv_set_lm_attn_max_rows", LA_CHOSEN, true));
  if (rows < LA_ROWS || rows > LA_MAX_ROWS)
    FAIL("vv_set_lm_attn_max_rows: " + std::to_string(rows) + " is outside [" + std::to_string(LA_ROWS) + ", " +
         std::to_string(LA_MAX_ROWS) + "]");
  c->lm_attn_max_rows = rows;
  return 0;
}
int vv_lm_attn_max_rows(vv_ctx* c) { return c ? c->lm_attn_max_rows : 0; }
int vv_kv_bytes(vv_ctx* c, long long* bytes) {
  if (!c || !bytes) FAIL("vv_kv_bytes: null argument");
  if (!c->finalized) FAIL("vv_kv_bytes before vv_finalize: the KV cache is not allocated yet");
  *bytes = (long long)(c->kv_k.bytes + c->kv_v.bytes + c->kv8_k.bytes + c->kv8_v.bytes + c->kv8_ek.bytes +
                       c->kv8_ev.bytes);
  return 0;
}

int vv_set_valid_ids(vv_ctx* c, int n, const int* ids) {
  if (n < 1 || n > 4) FAIL("vv_set_valid_ids: 1..4 ids");
  CHK(c->valid_ids.ensure(4 * sizeof(int)));
  HIPCHK(hipMemcpy(c->valid_ids.p, ids, n * sizeof(int), hipMemcpyHostToDevice));
  c->n_valid = n;
  return 0;
}

// diagnostic: a bf16-weight, bf16-KV engine runs k_lm_attn<false, 2> where it would run <false, 0> -- the
// FP8-KV form's data flow and quantiser on a bf16 cache (the appended rows stored dequantised)
static std::atomic<int> g_lm_attn_kvround{0};
extern "C" int vv_lm_attn_kvround(int on) {
  g_lm_attn_kvround = on ? 1 : 0;
  return 0;
}
// The attention half's route for a pass of `rows` rows planned for `keys` keys, decided here only and from
// plain values (LmAttnOpts: how qkv_w / o_w are bound, the KV format, the context's four options, max_ctx,
// the round-trip switch, whether a staging cache exists).  `one` = false is the three launches (q|k|v,
// k_attn, o_proj).  w8: every layer's qkv_w and o_w bound as codes with the option on (bf16 throughout: the
// bf16 form; a mixed binding, or codes without the option: the three launches).  kvq: 0 raw rows into a bf16
// cache, 1 the FP8 cache with its option (without it: the three launches + k_kv_quant), 2 the diagnostic
// round trip.  Above LA_ROWS rows: with max_rows, raw rows into a bf16 cache only (no KVQ form is built
// there).  Which (w8, kvq, keys, rows) are built, and resident, is lm_attn_fits' to say.
struct LmAttnOpts { int attn_form, kv_dtype, w8, kv8, max_keys, max_rows, max_ctx, kvround, staged; };
struct LmAttnRoute { bool one, w8; int kvq; };
static LmAttnRoute lm_attn_route(const LmAttnOpts& o, int rows, int keys) {
  const bool w8 = o.attn_form == vv_ctx::MLP_W8 && o.w8;
  const int kvq = o.kv_dtype ? 1 : o.kvround && o.attn_form == vv_ctx::MLP_BF16 && o.staged ? 2 : 0;
  const bool one = (w8 || o.attn_form == vv_ctx::MLP_BF16) && (!o.kv_dtype || o.kv8) &&
                   keys <= std::min(o.max_ctx, o.max_keys) && (rows <= LA_ROWS || (rows <= o.max_rows && kvq == 0));
  return {one, w8, kvq};
}
// diagnostic: out = {one, w8, kvq} of lm_attn_route (attn_form: 0 bf16, 1 FP8, 2 mixed)
extern "C" int vv_diag_lm_attn_route(int attn_form, int kv_dtype, int w8, int kv8, int max_keys, int max_rows,
                                     int max_ctx, int kvround, int staged, int rows, int keys, int* out) {
  if (!out) return 1;
  const LmAttnRoute r = lm_attn_route({attn_form, kv_dtype, w8, kv8, max_keys, max_rows, max_ctx, kvround, staged}, rows, keys);
  const int v[3] = {r.one, r.w8, r.kvq};
  std::copy(v, v + 3, out);
  return 0;
}
static LmAttnOpts lm_attn_opts(const vv_ctx* c) {
  return {c->attn_form, c->kv_dtype, c->lm_attn_w8, c->lm_attn_kv8, c->lm_attn_max_keys, c->lm_attn_max_rows,
          c->cfg.max_ctx, g_lm_attn_kvround.load(), c->stg.k != nullptr};
}
static bool lm_attn_route_fits(const vv_ctx* c, const LmAttnRoute& r, int rows, int keys) {
  const vv_config& k = c->cfg;
  return r.one && lm_attn_fits(r.w8, r.kvq, k.hidden, k.n_heads, k.n_kv_heads, k.head_dim, rows, keys);
}

int vv_finalize(vv_ctx* c) {
  const vv_config& k = c->cfg;
  HIPCHK(hipSetDevice(c->device));
  const int H = k.hidden, d = k.head_dim;
  c->qkv_n = (k.n_heads + 2 * k.n_kv_heads) * d;
  // ---- LM weights
  CHK(need(c, "lm.embed", {}, &c->lm.embed));
  CHK(need(c, "lm.lm_head", {}, &c->lm.lm_head));
  CHK(need(c, "lm.inv_freq", {d / 2}, &c->lm.inv_freq));
  CHK(need(c, "lm.norm", {H}, &c->lm.norm));
  c->lmw.assign(k.n_layers, LmLayerW{});
  for (int l = 0; l < k.n_layers; ++l) {
    const std::string p = "lm." + std::to_string(l);
    LmLayerW& w = c->lmw[l];
    CHK(need(c, p + ".in_norm", {H}, &w.in_norm));
    CHK(need_lm_w(c, p + ".qkv_w", c->qkv_n, H, &w.qkv));
    CHK(need(c, p + ".qkv_b", {c->qkv_n}, &w.qkv_b));
    CHK(need_lm_w(c, p + ".o_w", H, (int64_t)k.n_heads * d, &w.o));
    CHK(need(c, p + ".post_norm", {H}, &w.post_norm));
    CHK(need_lm_w(c, p + ".gu_w", 2LL * k.intermediate, H, &w.gu));
    CHK(need_lm_w(c, p + ".down_w", H, k.intermediate, &w.down));
  }
  {
    int n8 = 0;
    for (const LmLayerW& w : c->lmw) n8 += (w.gu.w8 != nullptr) + (w.down.w8 != nullptr);
    c->mlp_form = n8 == 0 ? vv_ctx::MLP_BF16 : n8 == 2 * k.n_layers ? vv_ctx::MLP_W8 : vv_ctx::MLP_MIXED;
    int a8 = 0;
    for (const LmLayerW& w : c->lmw) a8 += (w.qkv.w8 != nullptr) + (w.o.w8 != nullptr);
    c->attn_form = a8 == 0 ? vv_ctx::MLP_BF16 : a8 == 2 * k.n_layers ? vv_ctx::MLP_W8 : vv_ctx::MLP_MIXED;
  }
  if (c->quantized) {
    // the fallback's scratch (launch_gemm: more than 16 rows, forms k_gemv_w8 does not
    // serve): sized once to the largest quantised matrix, never grown in a hot call
    const size_t nk = std::max({(size_t)c->qkv_n * H, (size_t)H * k.n_heads * d, 2 * (size_t)k.intermediate * H});
    CHK(c->w8_scratch.ensure(nk * sizeof(bf16)));
  }
  // ---- diffusion head
  const int L = k.head_layers, F = k.head_ffn, D = k.latent_dim;
  CHK(need(c, "head.noisy_w", {H, D}, &c->head.noisy));
  CHK(need(c, "head.cond_w", {H, H}, &c->head.cond));
  CHK(need(c, "head.t0_w", {H, 256}, &c->head.t0));
  CHK(need(c, "head.t2_w", {H, H}, &c->head.t2));
  CHK(need(c, "head.ada_w", {(3LL * L + 2) * H, H}, &c->head.ada));
  // the FFN in the GEMV layout (weights.py: 16-row gate|up tiles of 8 gate + 8 up rows)
  c->head_gemv = true;
  c->headw.assign(L, HeadLayerW{});
  for (int l = 0; l < L; ++l) {
    const std::string p = "head." + std::to_string(l);
    CHK(need(c, p + ".norm", {H}, &c->headw[l].norm));
    CHK(need(c, p + ".gu_w", {2LL * F, H}, &c->headw[l].gu));
    CHK(need(c, p + ".down_w", {H, F}, &c->headw[l].down));
  }
  CHK(need(c, "head.final_w", {D, H}, &c->head.final));
  // grid-wait counters + the error word (always present: vv_sync_error_async reads it)
  for (DevBuf* b : sync_bufs(c)) {
    CHK(b->ensure(pk::BYTES));
    HIPCHK(hipMemset(b->p, 0, pk::BYTES));
  }
  // ---- connectors + latent scaling
  for (int q = 0; q < 2; ++q) {
    const std::string s(q == 0 ? "conn.ac" : "conn.se");
    ConnW& w = q == 0 ? c->conn_ac : c->conn_se;
    CHK(need(c, s + ".fc1_w", {H, q == 0 ? D : k.semantic_dim}, &w.fc1_w));
    CHK(need(c, s + ".fc1_b", {H}, &w.fc1_b));
    CHK(need(c, s + ".norm", {H}, &w.norm));
    CHK(need(c, s + ".fc2_w", {H, H}, &w.fc2_w));
    CHK(need(c, s + ".fc2_b", {H}, &w.fc2_b));
  }
  CHK(need(c, "speech_scaling_factor", {}, &c->scaling));
  CHK(need(c, "speech_bias_factor", {}, &c->bias));
  // ---- codec nets
  const int hop = [&] {
    int h = 1;
    for (int i = 0; i + 1 < k.n_stages; ++i) h *= k.ratios[i];
    return h;
  }();
  convnet_shape(c, c->dec, true, "dec", k.dec_n_filters, D, 1, 1, k.max_batch);
  convnet_shape(c, c->sem, false, "sem", k.sem_n_filters, 1, k.semantic_dim, hop, k.max_batch);
  CHK(convnet_check(c, c->dec));
  CHK(convnet_check(c, c->sem));
  // the non-streaming encoders: weights now, buffers per call (encode_nonstreaming)
  convnet_shape(c, c->senc, false, "sem", k.sem_n_filters, 1, k.semantic_dim, 0, 0);
  CHK(convnet_check(c, c->senc));
  c->has_aenc = c->w.count("aenc.stem_w") > 0;   // optional: vv_acoustic_encode fails without it
  if (c->has_aenc) {
    convnet_shape(c, c->aenc, false, "aenc", k.ac_enc_n_filters, 1, D, 0, 0);
    CHK(convnet_check(c, c->aenc));
  }
  CHK(convnet_alloc(c->dec, 7));
  CHK(convnet_alloc(c->sem, 7));
  // a context that can run a grid-waiting kernel (the persistent codec stage, the
  // one-launch head layer at 16 rows, ...) counts in the device's registry (hl_register)
  // (the one-launch MLP kernels in the form the MLP weights are bound in; a mixed binding runs neither)
  const bool mlp_w8 = c->mlp_form == vv_ctx::MLP_W8, mlp_one = c->mlp_form != vv_ctx::MLP_MIXED;
  const bool lf_fits = mlp_one && lm_ffn_fits(mlp_w8, k.hidden, k.intermediate, 2);
  const bool lf16_fits = mlp_one && lm_ffn16_fits(mlp_w8, k.hidden, k.intermediate, 16);
  if (k.max_batch >= 2 && lf16_fits) CHK(c->lf_slab.ensure(48 * 4 * 16 * 32 * sizeof(float)));
  // k_lm_attn: the (row class, key class) corners this context can reach, each through a pass's own route and
  // lm_attn_fits, so every form it may run has its residency queried here, not in a hot call or a graph capture.
  // The base corner (<= LA_ROWS rows, <= LA_MAX_KEYS keys) decides la_fits; the wider ones count only then, a row
  // class's long corner only after its short one.  la_top: the most rows admitted; the partials are sized for them.
  const int la_keys = std::min(k.max_ctx, c->lm_attn_max_keys);
  const int la_rows[2] = {std::min(2 * k.max_batch, LA_ROWS), std::min(2 * k.max_batch, c->lm_attn_max_rows)};
  const int la_kcls[2] = {std::min(la_keys, LA_MAX_KEYS), la_keys};
  const LmAttnOpts la_o = lm_attn_opts(c);
  int la_top = 0;
  for (int ri = 0; ri < (la_top && la_rows[1] > LA_ROWS ? 2 : 1); ++ri)
    for (int ki = 0; ki < (la_keys > LA_MAX_KEYS ? 2 : 1); ++ki) {
      const bool fits = lm_attn_route_fits(c, lm_attn_route(la_o, la_rows[ri], la_kcls[ki]), la_rows[ri], la_kcls[ki]);
      if (ki == 0 && !fits) break;
      if (ki == 0) la_top = la_rows[ri];
    }
  const bool la_fits = la_top > 0;
  if (la_fits) CHK(c->la_part.ensure(lm_attn_part_floats(la_top, la_keys) * sizeof(float)));
  CHK(c->cw_sync.ensure(pk::CW_BYTES));
  HIPCHK(hipMemset(c->cw_sync.p, 0, pk::CW_BYTES));
  if (c->head_gemv && head_m16_fits(k.hidden, k.head_ffn, 16))
  {
    CHK(c->m16_buf.ensure(16 * 192 * sizeof(float) + 16 * (size_t)k.hidden * sizeof(bf16)));
    HIPCHK(hipMemset(c->m16_buf.p, 0, 16 * 192 * sizeof(float)));
  }
  c->persist_capable = codec_plan(c, c->dec, 1, true).grid_waiting() || codec_plan(c, c->sem, 1, true).grid_waiting() ||
                       (c->head_gemv && head_m16_fits(k.hidden, k.head_ffn, 16)) ||
                       lf_fits || lf16_fits || la_fits;
  if (c->persist_ok && !c->persist_follow && c->persist_capable && !c->hl_registered) {
    c->hl_registered = true;
    hl_register(c->device, +1);
  }
  // ---- LM KV cache: [layer][slot][kv_head][ctx][d]
  c->lm_slots = 2 * k.max_batch;
  c->kv.d = d;
  // position stride of the cache rounded up to 64 (128 B): V^T rows [dim][ctx]
  // are read 16 B at a time by the attention kernel, and an odd stride left
  // every other row misaligned
  c->kv.max_ctx = (k.max_ctx + 63) / 64 * 64;
  c->kv.s_head = (long long)c->kv.max_ctx * d;
  c->kv.s_slot = c->kv.s_head * k.n_kv_heads;
  c->kv.s_layer = c->kv.s_slot * c->lm_slots;
  const size_t kvb = (size_t)c->kv.s_layer * k.n_layers * sizeof(bf16);
  if (c->kv_dtype) {
    // FP8 e4m3: one byte per element in the same geometry + one int8 exponent per row
    if (c->tp_size > 1 || c->comm) FAIL("an FP8 KV cache is not supported on a tensor-parallel engine");
    if (d != 128) FAIL("an FP8 KV cache needs head_dim 128");
    const size_t codes = kvb / sizeof(bf16), exps = codes / d;
    CHK(c->kv8_k.ensure(codes));
    CHK(c->kv8_v.ensure(codes + 256));
    CHK(c->kv8_ek.ensure(exps));
    CHK(c->kv8_ev.ensure(exps));
    HIPCHK(hipMemset(c->kv8_k.p, 0, c->kv8_k.bytes));
    HIPCHK(hipMemset(c->kv8_v.p, 0, c->kv8_v.bytes));
    HIPCHK(hipMemset(c->kv8_ek.p, 0, exps));
    HIPCHK(hipMemset(c->kv8_ev.p, 0, exps));
    c->kv8.k = (unsigned char*)c->kv8_k.p;
    c->kv8.v = (unsigned char*)c->kv8_v.p;
    c->kv8.ek = (signed char*)c->kv8_ek.p;
    c->kv8.ev = (signed char*)c->kv8_ev.p;
  } else {
    CHK(c->kv_k.ensure(kvb));
    CHK(c->kv_v.ensure(kvb + 256));
  }
  if (d == 128) CHK(kv_stage_ensure(c, (size_t)c->lm_slots));   // a decode pass's staging (>= 32 positions)
  // RoPE cos / sin per position (the q|k|v epilogue reads it instead of cosf / sinf)
  if (d == 128) {
    CHK(c->rope_tab.ensure((size_t)c->kv.max_ctx * 128 * sizeof(bf16)));
    KCHK(launch_rope_table(c->kv.max_ctx, c->lm.inv_freq, (bf16*)c->rope_tab.p, nullptr));
    HIPCHK(hipDeviceSynchronize());
  }
  c->kv.k = (bf16*)c->kv_k.p;
  c->kv.v = (bf16*)c->kv_v.p;
  // ---- attention split partials for decode (2 * max_batch rows, <= 64 splits) + tickets
  CHK(c->attn_part.ensure(attn_part_bytes((size_t)2 * k.max_batch, k.n_heads, 256, 0)));
  CHK(c->attn_cnt.ensure(65536 * sizeof(unsigned)));
  HIPCHK(hipMemset(c->attn_cnt.p, 0, 65536 * sizeof(unsigned)));
  // ---- split-K slabs + tickets
  CHK(c->splitk_ws.ensure(64ull << 20));
  CHK(c->splitk_cnt.ensure(65536 * sizeof(unsigned)));
  HIPCHK(hipMemset(c->splitk_cnt.p, 0, 65536 * sizeof(unsigned)));
  // ---- diffusion workspace (rows = 2 * max_batch)
  {
    const size_t R = 2 * (size_t)k.max_batch;
    const size_t mod = (3 * (size_t)L + 2) * H;
    const size_t elems = R * H * 6 + HEAD_SC * R * (mod + H) + R * F + R * D * 3 + (size_t)k.max_batch * D * 2;
    CHK(c->head_ws.ensure(elems * sizeof(bf16)));
  }
  CHK(c->codec_ws.ensure((size_t)k.max_batch * (4 * H + 2 * 256) * sizeof(bf16) + 4096));
  CHK(c->zero_rows.ensure((size_t)2 * k.max_batch * H * sizeof(bf16)));
  HIPCHK(hipMemset(c->zero_rows.p, 0, (size_t)2 * k.max_batch * H * sizeof(bf16)));
  CHK(c->slot_scratch.ensure(4096));
  {
    const uint16_t one_zero[2] = {0x3F80, 0x0000};
    CHK(c->unit_sb.ensure(sizeof(one_zero)));
    HIPCHK(hipMemcpy(c->unit_sb.p, one_zero, sizeof(one_zero), hipMemcpyHostToDevice));
  }
  HIPCHK(hipDeviceSynchronize());
  c->finalized = true;
  return 0;
}

int vv_set_schedule(vv_ctx* c, int steps, const float* coef, const void* tfreq, vv_stream vst) {
  hipStream_t st = (hipStream_t)vst;
  if (!c->finalized) FAIL("vv_set_schedule before vv_finalize");
  if (steps < 1 || steps > 1000) FAIL("steps out of range");
  const int H = c->cfg.hidden;
  c->coef.resize(steps);
  for (int s = 0; s < steps; ++s) {
    const float* q = coef + 8 * s;
    DpmCoef& e = c->coef[s];
    e.alpha_s = q[0];
    e.sigma_s = q[1];
    e.c_x = q[2];
    e.c_d0 = q[3];
    e.c_d1 = q[4];
    e.inv_r0 = q[5];
    e.order = (int)q[6];
    e.c_n = q[7];
    e.cfg = 0.f;
  }
  // sized for the largest schedule once, so captured graphs keep valid pointers
  CHK(c->temb.ensure((size_t)1000 * H * sizeof(bf16)));
  CHK(c->tfreq_tmp.ensure((size_t)1000 * H * sizeof(bf16)));
  // t_emb = Linear2(SiLU(Linear0(t_freq)))  (TimestepEmbedder.forward, diffusion_head.py:90-93)
  bf16* t1 = (bf16*)c->tfreq_tmp.p;
  CHK(gemm(c, gemm_args(c, steps, H, 256, rowmap(tfreq, 256), c->head.t0, EPI_STORE, rowmap(t1, H)), st));
  KCHK(launch_silu(steps * H, t1, t1, st));
  CHK(gemm(c, gemm_args(c, steps, H, H, rowmap(t1, H), c->head.t2, EPI_STORE, rowmap(c->temb.p, H)), st));
  c->steps = steps;
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

int vv_kv_copy(vv_ctx* c, int n, const int* slots, const int* src, const int* dst, vv_stream vst) {
  if (!c->finalized) FAIL("vv_kv_copy before vv_finalize");
  if (c->kv_dtype) {
    KCHK(launch_kv_copy8(c->kv, c->kv8, c->cfg.n_layers, c->cfg.n_kv_heads, n, slots, src, dst, (hipStream_t)vst));
    return 0;
  }
  KCHK(launch_kv_copy(c->kv, c->cfg.n_layers, c->cfg.n_kv_heads, n, slots, src, dst, (hipStream_t)vst));
  return 0;
}

int vv_kv_synthetic(vv_ctx* c, int n, const int* slots, int p0, int p1, unsigned seed, vv_stream vst) {
  if (!c->finalized) FAIL("vv_kv_synthetic before vv_finalize");
  if (c->kv_dtype) FAIL("vv_kv_synthetic: the synthetic fill (k_kv_fill) writes a bf16 cache; this engine's KV cache is FP8 e4m3");
  if (p0 < 0 || p1 > c->cfg.max_ctx || p0 > p1) FAIL("vv_kv_synthetic: positions outside [0, max_ctx)");
  KCHK(launch_kv_fill(c->kv, c->cfg.n_layers, c->cfg.n_kv_heads, n, slots, p0, p1, seed, (hipStream_t)vst));
  return 0;
}

int vv_embed(vv_ctx* c, int n, const int* ids, void* out, vv_stream vst) {
  if (!c->finalized) FAIL("vv_embed before vv_finalize");
  const int H = c->cfg.hidden;
  KCHK(launch_gather_rows(n, H, c->lm.embed, H, ids, rowmap(out, H), (hipStream_t)vst));
  return 0;
}

// ------------------------------------------------------------------ LM pass
// test switch (vv_rope_table): 0 = the q|k|v epilogue computes cos / sin inline
static std::atomic<int> g_rope_tab{1};
extern "C" int vv_rope_table(int on) {
  g_rope_tab = on;
  return 0;
}
// One forward of ntok token rows, split so that a tensor-parallel group can
// interleave its ranks layer by layer (vv_lm_forward_group) or all-reduce over
// RCCL between the halves (vv_lm_forward).
// Decode attention with a deferred split merge (vv_attn_defer): contexts of 2..8
// chunks of g_defer_chunk keys run that many splits per (row, kv head), each
// leaves its (m, l, o) partial and o_proj merges them while staging its A rows
// (XF_ATTN_MERGE) -- the split parallelism without a ticket or a merge pass.
// Rows: B = 1 (2 rows) gains 1.5 % at K = 750; at B = 8 (16 rows) o_proj's
// staging of 16 rows' partials cost more than the splits saved (5.79 vs 5.67 ms),
// so by default only <= 4 rows defer.
static std::atomic<int> g_attn_defer{4}, g_defer_chunk{128};
// longest split of the deferred-merge plan (keys); longer contexts take the
// grouped plan's many splits (diagnostic vv_attn_defer_max)
static std::atomic<int> g_defer_max{1024};
extern "C" int vv_attn_defer_max(int keys) {
  g_defer_max = keys <= 0 ? 1024 : keys;
  return 0;
}
extern "C" int vv_attn_defer(int on, int chunk) {
  if (chunk % 32 || chunk < 32 || on < 0) return 1;
  g_attn_defer = on == 1 ? 4 : on;   // 1: the default row limit; n >= 2: up to n rows (<= 16)
  g_defer_chunk = chunk;
  return 0;
}
// Long contexts (> 8 splits of 1,024 keys, i.e. > 8,192 keys) with <= 16 rows:
// up to 120 splits of >= 256 keys (65K: 120 x 544, so the one long row's 2 kv
// heads fill 240 CUs where 1,024-key splits busied 128), merged in <= 8
// groups of <= 16 consecutive splits by each group's last-arriving workgroup;
// o_proj merges the group partials (XF_ATTN_MERGE) -- no k_attn_merge launch.
// 120, not 128: k_attn takes one CU per workgroup (234 VGPRs), and the
// dispatcher does not deal workgroups to the 8 XCDs strictly round-robin
// (tools/attn_long_stamps.py: 256 workgroups landed 30 / 34 on two XCDs), so
// with 256 keyed workgroups two CUs ran two in turn and the launch took twice
// as long as its median workgroup.
static std::atomic<int> g_attn_group{120};   // diagnostic (vv_attn_group): 0 = the 1,024-key plan + k_attn_merge
extern "C" int vv_attn_group(int on) {      // 1 = default; n >= 2: at most n splits (<= 128)
  g_attn_group = on == 1 ? 120 : on <= 0 ? 0 : std::min(on, 128);
  return 0;
}
// The decode attention's plan for a pass of ntok rows over max_pos_p1 keys
// (lm_plan; vv_attn_pass_plan reports it to the CPU tests): prefill kernel or
// not, key splits, deferred merge (o_proj merges), grouped merge.
struct AttnPassPlan {
  int prefill = 0, nsplit = 1, chunk = 64, defer = 0, group = 0, ngroups = 0;
};
static AttnPassPlan attn_pass_plan(int ntok, int lm_slots, int head_dim, int n_kv, int max_pos_p1) {
  AttnPassPlan P;
  P.prefill = attn_use_prefill(ntok, lm_slots) ? 1 : 0;
  P.nsplit = P.prefill ? 1 : attn_plan(ntok, n_kv, max_pos_p1, &P.chunk);
  if (!P.prefill && g_attn_defer && ntok <= g_attn_defer && ntok <= 16 && head_dim == 128) {
    // 2..8 splits of >= g_defer_chunk keys, up to 8 x 1,024 keys (longer contexts
    // keep attn_plan's many 1,024-key splits: the merge input grows with them)
    int ch = g_defer_chunk, ns = (max_pos_p1 + ch - 1) / ch;
    if (ns > 8) {
      ch = ((max_pos_p1 + 7) / 8 + 31) / 32 * 32;
      ns = (max_pos_p1 + ch - 1) / ch;
    }
    if (ns >= 2 && ns <= 8 && ch <= g_defer_max) {
      P.defer = 1;
      P.nsplit = ns;
      P.chunk = ch;
    }
  }
  if (!P.prefill && !P.defer && g_attn_group && P.nsplit > 8 && ntok <= 16 && head_dim == 128) {
    int ns = std::min((int)g_attn_group, (max_pos_p1 + 255) / 256);
    const int ch = ((max_pos_p1 + ns - 1) / ns + 31) / 32 * 32;
    ns = (max_pos_p1 + ch - 1) / ch;
    const int gs = (ns + 7) / 8, ng = (ns + gs - 1) / gs;
    // the two limits the kernels have: k_attn's group merge holds <= 16 split
    // partials (GMAX), o_proj's XF_ATTN_MERGE staging <= 8 group partials (with
    // gs = ceil(ns / 8) and ns <= 128 both hold by construction; checked, not
    // assumed -- tests/test_capi_cpu.py sweeps the plan against them)
    if (gs <= 16 && ng <= 8) {
      P.nsplit = ns;
      P.chunk = ch;
      P.group = gs;
      P.ngroups = ng;
    }
  }
  return P;
}
// diagnostic: out = {prefill, nsplit, chunk, defer, group, ngroups}
extern "C" int vv_attn_pass_plan(int ntok, int lm_slots, int head_dim, int n_kv, int max_pos_p1, int* out) {
  if (!out || ntok <= 0 || max_pos_p1 <= 0) return 1;
  const AttnPassPlan P = attn_pass_plan(ntok, lm_slots, head_dim, n_kv, max_pos_p1);
  const int v[6] = {P.prefill, P.nsplit, P.chunk, P.defer, P.group, P.ngroups};
  for (int i = 0; i < 6; ++i) out[i] = v[i];
  return 0;
}

// residual epilogue of a row-parallel projection: rank 0 adds the residual,
// the other ranks contribute their partial only (the all-reduce sums them)
static void tp_residual(vv_ctx* c, GemmArgs& g, const RowMap& res) {
  if (c->tp_rank == 0) {
    g.epi.kind = EPI_RES;
    g.epi.res = res;
  } else {
    g.epi.kind = EPI_STORE;
  }
}

// the LM attention half at decode in one launch (lm_attn.hip): <= 16 rows (the context's lm_attn_max_rows) of the
// 1.5B shapes, contexts <= the context's lm_attn_max_keys (default LA_MAX_KEYS), unsharded, while the context is the
// device's only registered one; 0 = the three launches (q|k|v, k_attn, o_proj)
static std::atomic<int> g_lm_attn{1};
static std::atomic<unsigned long long*> g_lm_attn_stamps{nullptr};
extern "C" int vv_lm_attn(int on) {
  g_lm_attn = on & 15;   // bits 1..3 (A/B): clear those LmAttnArgs::variant bits
  return 0;
}
extern "C" int vv_lm_attn_stamps(void* buf) {   // diagnostic: k_lm_attn launches record [256][16] phase stamps
  g_lm_attn_stamps = (unsigned long long*)buf;
  return 0;
}
// the LM MLP block in one launch (lm_ffn.hip) at decode with <= 2 rows, unsharded,
// while the context is the device's only registered one; 0 = two GEMV launches
static std::atomic<int> g_lm_ffn{1};
static std::atomic<unsigned long long*> g_lm_ffn_stamps{nullptr};
extern "C" int vv_lm_ffn_stamps(void* buf) {   // diagnostic: k_lm_ffn16 launches record [256][16] phase stamps
  g_lm_ffn_stamps = (unsigned long long*)buf;
  return 0;
}
extern "C" int vv_lm_ffn(int on) {   // bit 0: on; bit 1: not at 3..16 rows (k_lm_ffn16)
  g_lm_ffn = on & 3;
  return 0;
}
// FP8 MLP weights: the W8 forms of the two kernels (vv_lm_ffn_w8 bit 0: at <= 2 rows, bit 1:
// at 3..16 rows; 0 = an FP8 engine runs the k_gemv_w8 pair).  A bf16 engine does not read it.
// Bumps the workspace epoch: graphs captured with the other path are re-captured.
static std::atomic<int> g_lm_ffn_w8{3};
extern "C" int vv_lm_ffn_w8(int bits) {
  if (bits < 0 || bits > 3) FAIL("vv_lm_ffn_w8: bits 0..3 (bit 0: <= 2 rows, bit 1: 3..16 rows)");
  g_lm_ffn_w8 = bits;
  g_ws_epoch.fetch_add(1);
  return 0;
}

// Which kernels a pass of ntok rows planned for `keys` keys runs (DESIGN.md "How an LM pass picks its kernels"),
// decided once per pass, not at vv_finalize: persist_on follows the contexts registered at that moment and the
// diagnostic switches may flip between passes; each is read once here.  The layers' halves decide nothing.
enum FfnRoute { FFN_GEMMS = 0, FFN_ONE = 1, FFN_ONE16 = 2 };   // the GEMM pair, k_lm_ffn (<= 2 rows), k_lm_ffn16 (3..16)
struct LmPlan {
  AttnPassPlan attn;               // k_attn's launch plan (the three launches; `prefill` bars every one-launch kernel)
  LmAttnRoute la{false, false, 0}; // la.one: the attention half is one k_lm_attn launch, in the form (la.w8, la.kvq)
  int la_variant = 0;              // LmAttnArgs::variant (vv_lm_attn's A/B bits)
  bool stage_kv = false;           // three launches on an FP8-KV context: staging prep at layer 0, k_kv_quant per layer
  // the MLP half runs in chunks of mlp_rows rows: the whole pass, or LA_ROWS where the attention half took
  // k_lm_attn's second row class (the GEMMs of 17 .. 32 rows sum K in another order: every row keeps the bits
  // it has in a pass of <= 16 rows)
  int mlp_rows = 0;
  FfnRoute ffn_full = FFN_GEMMS, ffn_tail = FFN_GEMMS;   // a chunk of mlp_rows rows; the shorter last one
};
static LmPlan lm_plan(vv_ctx* c, int ntok, int keys) {
  const vv_config& k = c->cfg;
  const int sw_attn = g_lm_attn, sw_ffn = g_lm_ffn, sw_ffn_w8 = g_lm_ffn_w8;
  LmPlan p;
  // (keys < 1 -- vv_lm_mlp_replay, vv_lm_ffn_active: no attention half, no prefill; lm_attn_fits refuses it)
  if (keys > 0) p.attn = attn_pass_plan(ntok, c->lm_slots, k.head_dim, k.n_kv_heads, keys);
  // what every grid-waiting LM kernel asks of the pass and the context
  const bool grid = !p.attn.prefill && c->tp_size == 1 && !c->comm && persist_on(c);
  p.la = lm_attn_route(lm_attn_opts(c), ntok, keys);
  p.la.one = sw_attn && grid && c->la_part.p && lm_attn_route_fits(c, p.la, ntok, keys) &&
             lm_attn_part_floats(ntok, keys) * sizeof(float) <= c->la_part.bytes;
  p.la_variant = 7 ^ (sw_attn >> 1);
  p.stage_kv = c->kv_dtype && !p.la.one;
  p.mlp_rows = ntok > LA_ROWS && p.la.one ? LA_ROWS : ntok;
  const auto ffn = [&](int rows) {
    const bool w8 = c->mlp_form == vv_ctx::MLP_W8, small = rows <= 2;
    if (!sw_ffn || !grid || c->mlp_form == vv_ctx::MLP_MIXED || (w8 && !(sw_ffn_w8 & (small ? 1 : 2)))) return FFN_GEMMS;
    if (small) return lm_ffn_fits(w8, k.hidden, k.intermediate, rows) ? FFN_ONE : FFN_GEMMS;
    return !(sw_ffn & 2) && c->lf_slab.p && lm_ffn16_fits(w8, k.hidden, k.intermediate, rows) ? FFN_ONE16 : FFN_GEMMS;
  };
  p.ffn_full = ffn(p.mlp_rows);
  p.ffn_tail = ffn(ntok % std::max(1, p.mlp_rows));
  return p;
}
extern "C" int vv_lm_attn_active(vv_ctx* c, int ntok, int max_pos_p1) {
  return c && c->finalized && lm_plan(c, ntok, max_pos_p1).la.one ? 1 : 0;
}
extern "C" int vv_lm_ffn_active(vv_ctx* c, int ntok) {
  return c && c->finalized && lm_plan(c, ntok, 0).ffn_full != FFN_GEMMS ? 1 : 0;
}

struct LmPass {
  int ntok = 0;
  int maxp = 0;   // keys of the longest row (max position + 1)
  LmPlan plan;
  bf16 *h = nullptr, *q = nullptr, *att = nullptr, *act = nullptr;
  RowMap in_m, hm;
  const int *slot = nullptr, *pos = nullptr;
};

static int lm_begin(vv_ctx* c, LmPass& P, int ntok, const void* embeds, int embed_rows, const int* slot,
                    const int* pos, int max_pos_p1) {
  if (!c->finalized) FAIL("vv_lm_forward before vv_finalize");
  if (max_pos_p1 > c->cfg.max_ctx) FAIL("position beyond max_ctx");
  const vv_config& k = c->cfg;
  const int H = k.hidden, d = k.head_dim, I = k.intermediate, nhd = k.n_heads * d;
  const size_t per = (size_t)H * 3 + c->qkv_n + nhd * 2 + I;
  if (c->kv_dtype) CHK(kv_stage_ensure(c, (size_t)ntok));
  if ((size_t)ntok > c->lm_ws_tokens) {
    // + 16 act rows: a packed act block (vv_norm_pack) rounds the rows up to 16
    CHK(c->lm_ws.ensure((per * ntok + (size_t)16 * I) * sizeof(bf16) + 256));
    c->lm_ws_tokens = ntok;
  }
  P.ntok = ntok;
  P.maxp = max_pos_p1;
  P.h = (bf16*)c->lm_ws.p;
  bf16* a = P.h + (size_t)ntok * H;
  bf16* qkv = a + (size_t)ntok * H;
  P.q = qkv + (size_t)ntok * c->qkv_n;
  P.att = P.q + (size_t)ntok * nhd;
  P.act = P.att + (size_t)ntok * nhd;
  P.plan = lm_plan(c, ntok, max_pos_p1);
  const AttnPassPlan& ap = P.plan.attn;
  if (ap.nsplit > 1) {
    if ((size_t)ntok * k.n_kv_heads * std::max(1, ap.ngroups) > 65536) FAIL("attention split tickets exhausted");
    CHK(c->attn_part.ensure(attn_part_bytes(ntok, k.n_heads, ap.nsplit, ap.ngroups)));
  }
  // token row m reads embeds row m % embed_rows (the negative CFG rows consume the
  // positive rows' embeddings, :594-596); layer 0's attention residual writes h
  if (embed_rows <= 0 || embed_rows > ntok) embed_rows = ntok;
  P.in_m = rowmap(embeds, H, embed_rows, 0);
  P.hm = rowmap(P.h, H);   // (the one-launch kernels rely on it: dense rows of stride H, no index, every row of the pass)
  P.slot = slot;
  P.pos = pos;
  return 0;
}

// input_layernorm .. o_proj (+ residual on rank 0)
static int lm_attn_half(vv_ctx* c, LmPass& P, int l, hipStream_t st) {
  const vv_config& k = c->cfg;
  const int H = k.hidden, d = k.head_dim, nhd = k.n_heads * d;
  const LmLayerW& w = c->lmw[l];
  const LmPlan& plan = P.plan;
  {
    // input_layernorm -> q|k|v projection (+bias) -> RoPE -> q / KV cache, one launch
    GemmArgs g = gemm_args(c, P.ntok, c->qkv_n, H, l == 0 ? P.in_m : P.hm, w.qkv, EPI_ROPE, RowMap{},
                           w.qkv_b);
    g.xf = xf_norm(w.in_norm, k.rms_eps);
    g.rope.nh = k.n_heads;
    g.rope.nkv = k.n_kv_heads;
    g.rope.layer = l;
    g.rope.q_out = P.q;
    g.rope.slots = P.slot;
    g.rope.pos = P.pos;
    g.rope.inv_freq = c->lm.inv_freq;
    g.rope.cs_tab = g_rope_tab ? (const bf16*)c->rope_tab.p : nullptr;
    g.rope.kv = c->kv;
    // (k_lm_attn's KVQ forms stage and quantise inside the launch: the real tables, no prep, no k_kv_quant)
    if (plan.stage_kv) {
      // FP8 KV: the epilogue appends to the staging cache (token m at slot 0, position m; cos / sin
      // from the pass's rows of the real positions), k_kv_quant below moves the rows to the cache
      if (l == 0)
        KCHK(launch_kv_stage_prep(P.ntok, (int)c->kv_stage_tokens, P.pos, c->kv.max_ctx, (const bf16*)c->rope_tab.p, c->stg_cs, c->stg_slot,
                                  c->stg_pos, st));
      g.rope.slots = c->stg_slot;
      g.rope.pos = c->stg_pos;
      g.rope.cs_tab = c->stg_cs;
      g.rope.kv = c->stg;
    }
    if (plan.la.one) {
      LmAttnArgs a;
      memset(&a, 0, sizeof(a));
      a.qkv = g;
      a.kvq = plan.la.kvq;
      a.stg = c->stg;
      a.kv8 = c->kv8;
      a.nw = w.in_norm;
      a.eps = k.rms_eps;
      a.scale = 1.0f / sqrtf((float)d);
      a.R = P.ntok;
      a.ow = w.o.w;
      a.ow8 = w.o.w8;     // codes throughout: the launcher picks the W8 form (a.qkv carries q|k|v's)
      a.owe = w.o.w8e;
      a.res =l == 0 ? P.in_m : P.hm;
      a.out = P.hm;
      a.att = P.att;
      a.part = (float*)c->la_part.p;
      a.sync = (unsigned*)c->lf_sync.p;
      a.err = err_word(c);
      a.stamps = g_lm_attn_stamps.load();
      a.variant = plan.la_variant;
      KCHK(launch_lm_attn(a, P.maxp, st));
      return 0;
    }
    CHK(gemm(c, g, st));
    if (plan.stage_kv)
      KCHK(launch_kv_quant(c->stg, c->kv, c->kv8, l, k.n_kv_heads, c->lm_slots, P.ntok, P.slot, P.pos, st));
  }
  AttnArgs at;
  memset(&at, 0, sizeof(at));
  at.kv8 = c->kv8;
  at.stamps = g_attn_stamps;
  at.nq = P.ntok;
  at.nh = k.n_heads;
  at.nkv = k.n_kv_heads;
  at.layer = l;
  at.nsplit = plan.attn.nsplit;
  at.chunk = plan.attn.chunk;
  at.prefill = plan.attn.prefill;
  at.defer = plan.attn.defer;
  at.counters = (unsigned*)c->attn_cnt.p;
  at.scale = 1.0f / sqrtf((float)d);
  at.q = P.q;
  at.out = P.att;
  at.slots = P.slot;
  at.pos = P.pos;
  at.kv = c->kv;
  at.group = plan.attn.group;
  at.ngroups = plan.attn.ngroups;
  attn_part_carve(at, c->attn_part.p);
  KCHK(launch_attn(at, st));
  GemmArgs g = gemm_args(c, P.ntok, H, nhd, rowmap(P.att, nhd), w.o, EPI_RES, P.hm);
  if (at.defer || at.group) attn_merge_xf(g, at);
  tp_residual(c, g, l == 0 ? P.in_m : P.hm);
  CHK(gemm(c, g, st));
  return 0;
}

// post_attention_layernorm .. down_proj (+ residual on rank 0), chunk by chunk (LmPlan::mlp_rows)
static int lm_mlp_half(vv_ctx* c, LmPass& P, int l, hipStream_t st) {
  const vv_config& k = c->cfg;
  const int H = k.hidden, I = k.intermediate;
  const LmLayerW& w = c->lmw[l];
  for (int r0 = 0; r0 < P.ntok; r0 += P.plan.mlp_rows) {
    const int n = std::min(P.plan.mlp_rows, P.ntok - r0);
    const FfnRoute route = n == P.plan.mlp_rows ? P.plan.ffn_full : P.plan.ffn_tail;
    bf16* const h = (bf16*)P.hm.base + (size_t)r0 * H;
    bf16* const act = P.act + (size_t)r0 * I;
    if (route != FFN_GEMMS) {
      LmFfnArgs a;
      memset(&a, 0, sizeof(a));
      a.x = h;
      a.out = h;
      a.ldx = H;
      a.R = n;
      a.eps = k.rms_eps;
      a.nw = w.post_norm;
      a.gu = w.gu.w;
      a.dn = w.down.w;
      a.gu8 = w.gu.w8;     // MLP_W8: the code forms (the launchers pick the W8 kernels)
      a.gue = w.gu.w8e;
      a.dn8 = w.down.w8;
      a.dne = w.down.w8e;
      a.act = act;
      a.sync = (unsigned*)c->lf_sync.p;
      a.err = err_word(c);
      a.slab = (float*)c->lf_slab.p;
      a.stamps = g_lm_ffn_stamps.load();
      if (route == FFN_ONE) KCHK(launch_lm_ffn(a, st));
      else KCHK(launch_lm_ffn16(a, st));
      continue;
    }
    // post_attention_layernorm fused into gate|up's A load
    const RowMap hm = rowmap(h, H);
    GemmArgs g = gemm_args(c, n, 2 * I, H, hm, w.gu, EPI_SILU_MUL, rowmap(act, I));
    g.xf = xf_norm(w.post_norm, k.rms_eps);
    GemmArgs d = gemm_args(c, n, H, I, rowmap(act, I), w.down, EPI_RES, hm);
    tp_residual(c, d, hm);
    // prefill: SiLU*up written MFMA-fragment-packed for the down projection when
    // both take the 256 x 256 tile (16K rows: down 449 -> 388 us)
    GemmArgs gp = g;
    gp.xf.kind = XF_NONE;
    if (g_norm_pack && I % 32 == 0 && gemm_uses_xl(gp) && gemm_uses_xl(d)) {
      g.epi.pack = 1;
      d.apack = 1;
    }
    CHK(gemm(c, g, st));
    CHK(gemm(c, d, st));
  }
  return 0;
}

// Diagnostic (bench.py's roofline of the LM MLP block): `reps` passes over the
// LM layers' MLP blocks alone on `ntok` decode rows (hidden [ntok][H], act
// [ntok][I] scratch), as lm_mlp_half runs them (k_lm_ffn or the GEMV pair).
// The call has no key count, so its plan has no attention half: a pass of 17 .. 32
// rows runs whole, never as the 16-row chunks of k_lm_attn's second row class.
extern "C" int vv_lm_mlp_replay(vv_ctx* c, int ntok, void* hidden, void* act, int reps, vv_stream vst) {
  if (!c || !c->finalized || ntok < 1 || ntok > 2 * c->cfg.max_batch || !hidden || !act)
    FAIL("vv_lm_mlp_replay: bad arguments");
  LmPass P;
  P.ntok = ntok;
  P.plan = lm_plan(c, ntok, 0);
  P.h = (bf16*)hidden;
  P.hm = rowmap(hidden, c->cfg.hidden);
  P.act = (bf16*)act;
  for (int r = 0; r < reps; ++r)
    for (int l = 0; l < c->cfg.n_layers; ++l) CHK(lm_mlp_half(c, P, l, (hipStream_t)vst));
  return 0;
}

// Benchmarks only (bench.py --tp: the collective's share of an LM pass):
// skip the all-reduces of a communicator engine — the outputs are then wrong.
static std::atomic<int> g_tp_null{0};
extern "C" int vv_tp_null_collective(int on) {
  g_tp_null = on ? 1 : 0;
  return 0;
}

static int tp_allreduce(vv_ctx* c, LmPass& P, hipStream_t st) {
  if (!c->comm) {
    if (c->tp_size > 1) FAIL("tensor-parallel engine without a communicator (vv_tp_init)");
    return 0;
  }
  if (g_tp_null) return 0;
  const ncclResult_t r = ncclAllReduce(P.h, P.h, (size_t)P.ntok * c->cfg.hidden, ncclBfloat16, ncclSum, c->comm, st);
  if (r != ncclSuccess) FAIL(std::string("ncclAllReduce: ") + ncclGetErrorString(r));
  return 0;
}

static int lm_end(vv_ctx* c, LmPass& P, int nout, const int* out_idx, void* hidden_out, float* logits_out,
                  hipStream_t st) {
  if (nout <= 0) return 0;
  const vv_config& k = c->cfg;
  // gather the output rows + final norm + the valid-id lm_head rows, one launch
  KCHK(launch_final_head(nout, k.hidden, P.h, out_idx, c->lm.norm, k.rms_eps, (bf16*)hidden_out,
                         c->lm.lm_head, (const int*)c->valid_ids.p, logits_out ? c->n_valid : 0, logits_out,
                         st));
  return 0;
}

int vv_lm_forward(vv_ctx* c, int ntok, const void* embeds, int embed_rows, const int* slot, const int* pos,
                  int max_pos_p1, int nout, const int* out_idx, void* hidden_out, float* logits_out, vv_stream vst) {
  hipStream_t st = (hipStream_t)vst;
  if (ntok <= 0) return 0;
  LmPass P;
  CHK(lm_begin(c, P, ntok, embeds, embed_rows, slot, pos, max_pos_p1));
  for (int l = 0; l < c->cfg.n_layers; ++l) {
    CHK(lm_attn_half(c, P, l, st));
    CHK(tp_allreduce(c, P, st));
    CHK(lm_mlp_half(c, P, l, st));
    CHK(tp_allreduce(c, P, st));
  }
  return lm_end(c, P, nout, out_idx, hidden_out, logits_out, st);
}

// Diagnostic (bench.py's candidate roofline of the LM attention half): `reps`
// passes over the LM layers' attention halves alone on `ntok` decode rows
// (embeds [ntok][H] as layer 0's input; later layers read / write the pass's own
// hidden rows), as lm_attn_half runs them (k_lm_attn or the three launches).
extern "C" int vv_lm_attn_replay(vv_ctx* c, int ntok, const void* embeds, const int* slot, const int* pos,
                                 int max_pos_p1, int reps, vv_stream vst) {
  if (!c || !c->finalized || ntok < 1 || ntok > 2 * c->cfg.max_batch || !embeds || !slot || !pos)
    FAIL("vv_lm_attn_replay: bad arguments");
  LmPass P;
  CHK(lm_begin(c, P, ntok, embeds, ntok, slot, pos, max_pos_p1));
  for (int r = 0; r < reps; ++r)
    for (int l = 0; l < c->cfg.n_layers; ++l) CHK(lm_attn_half(c, P, l, (hipStream_t)vst));
  return 0;
}

int vv_lm_forward_group(int n, vv_ctx* const* ctxs, int ntok, const void* embeds, int embed_rows, const int* slot,
                        const int* pos, int max_pos_p1, int nout, const int* out_idx, void* hidden_out,
                        float* logits_out, vv_stream vst) {
  hipStream_t st = (hipStream_t)vst;
  if (n < 1 || n > 8) FAIL("vv_lm_forward_group: 1..8 ranks");
  if (ntok <= 0) return 0;
  std::vector<LmPass> P(n);
  SumRows sr;
  sr.n = n;
  for (int r = 0; r < n; ++r) {
    if (ctxs[r]->tp_rank != r || ctxs[r]->tp_size != n) FAIL("vv_lm_forward_group: engine r must be TP rank r of n");
    CHK(lm_begin(ctxs[r], P[r], ntok, embeds, embed_rows, slot, pos, max_pos_p1));
    sr.p[r] = P[r].h;
  }
  const long long count = (long long)ntok * ctxs[0]->cfg.hidden;
  for (int l = 0; l < ctxs[0]->cfg.n_layers; ++l) {
    for (int r = 0; r < n; ++r) CHK(lm_attn_half(ctxs[r], P[r], l, st));
    KCHK(launch_sum_rows(sr, count, st));
    for (int r = 0; r < n; ++r) CHK(lm_mlp_half(ctxs[r], P[r], l, st));
    KCHK(launch_sum_rows(sr, count, st));
  }
  return lm_end(ctxs[0], P[0], nout, out_idx, hidden_out, logits_out, st);
}

int vv_tp_unique_id(void* out, int nbytes) {
  if (nbytes < (int)sizeof(ncclUniqueId)) FAIL("vv_tp_unique_id: buffer smaller than ncclUniqueId");
  ncclUniqueId id;
  const ncclResult_t r = ncclGetUniqueId(&id);
  if (r != ncclSuccess) FAIL(std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
  memcpy(out, &id, sizeof(id));
  return (int)sizeof(id);
}

int vv_tp_init(vv_ctx* c, int rank, int size, const void* unique_id) {
  if (size < 1 || rank < 0 || rank >= size) FAIL("vv_tp_init: bad rank / size");
  if (size > 1 && c->kv_dtype) FAIL("vv_tp_init: an FP8 KV cache is not supported on a tensor-parallel engine");
  c->tp_rank = rank;
  c->tp_size = size;
  if (!unique_id) return 0;  // group emulation in one process: no communicator
  HIPCHK(hipSetDevice(c->device));
  ncclUniqueId id;
  memcpy(&id, unique_id, sizeof(id));
  const ncclResult_t r = ncclCommInitRank(&c->comm, size, id, rank);
  if (r != ncclSuccess) FAIL(std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  return 0;
}

// Every grid-wait counter of the context back to 0 and the error word cleared,
// with nothing in flight (the device is synchronised): after a wait gave up, the
// counters of that launch stay part-advanced, and a later launch's base
// generation (persist_dev.h) would let a wait release early.
int vv_sync_reset(vv_ctx* c) {
  if (!c->finalized) FAIL("vv_sync_reset before vv_finalize");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());
  for (DevBuf* b : sync_bufs(c)) HIPCHK(hipMemset(b->p, 0, pk::BYTES));   // (allocated by vv_finalize)
  HIPCHK(hipMemset(c->cw_sync.p, 0, pk::CW_BYTES));
  HIPCHK(hipDeviceSynchronize());
  return 0;
}
// A grid wait of a one-launch kernel gave up (workgroups not co-resident):
// every output since the last call is invalid.  Reset on read (with the wait
// counters: vv_sync_reset).
// (hipMemcpy on the null stream does not wait for non-blocking streams, where
// the host's generate() runs: synchronise the device first)
int vv_sync_error(vv_ctx* c) {
  unsigned v = 0;
  if (c->hf_sync.p) {
    HIPCHK(hipDeviceSynchronize());
    if (hipMemcpy(&v, err_word(c), 4, hipMemcpyDeviceToHost) != hipSuccess)
      FAIL("vv_sync_error: reading the error word failed (hipMemcpy)");
    if (v) CHK(vv_sync_reset(c));
  }
  return v ? 1 : 0;
}
// Stream-ordered form: enqueue on st a copy of the error word to dst (4 bytes of
// pinned host or device memory) and its reset, behind everything queued before.
// The host reads dst once an event recorded after this call has completed
// (GenerateSession: with each step's logits read-back, and before audio leaves
// for a streamer); when it reads 1 it calls vv_sync_reset before anything else.
int vv_sync_error_async(vv_ctx* c, void* dst, vv_stream vst) {
  hipStream_t st = (hipStream_t)vst;
  if (!dst) FAIL("vv_sync_error_async: dst is NULL");
  if (!c->finalized) FAIL("vv_sync_error_async before vv_finalize");
  unsigned* word = err_word(c);
  HIPCHK(hipMemcpyAsync(dst, word, 4, hipMemcpyDefault, st));
  HIPCHK(hipMemsetAsync(word, 0, 4, st));
  return 0;
}
// Per-context switch of the grid-waiting kernels (default: on unless
// VIBEVOICE_PERSISTENT=0).  Off: the context neither launches them nor counts in
// the device's registry, so it never demotes another context (the standalone
// tokenizer API's codec context) nor contends with it.  Bumps the workspace
// epoch: graphs captured with the other path are re-captured.
int vv_set_persistent(vv_ctx* c, int on) {
  if (!c) FAIL("vv_set_persistent: null context");
  if (on < 0 || on > 2) FAIL("vv_set_persistent: 0 (off), 1 (on) or 2 (follow)");
  c->persist_ok = on != 0;
  c->persist_follow = on == 2;
  if (on == 2) c->persist_ok = true;
  if (c->finalized) {
    if ((!c->persist_ok || c->persist_follow) && c->hl_registered) {
      c->hl_registered = false;
      hl_register(c->device, -1);
    } else if (c->persist_ok && !c->persist_follow && c->persist_capable && !c->hl_registered) {
      c->hl_registered = true;
      hl_register(c->device, +1);
    }
  }
  g_ws_epoch.fetch_add(1);
  return 0;
}
int vv_persistent_active(vv_ctx* c) { return c && c->finalized && persist_on(c) ? 1 : 0; }
// Diagnostic (tests): raise the error word as a grid wait that gave up would, and leave
// the counters part-advanced as such a launch does: per buffer shard 0 + 5, each
// generation line + 3, the last ticket + 1; cluster 0 of each cw_sync half + 3.
extern "C" int vv_diag_raise_sync_error(vv_ctx* c) {
  if (!c->finalized) FAIL("vv_diag_raise_sync_error before vv_finalize");
  HIPCHK(hipDeviceSynchronize());
  auto bump = [](void* buf, int word, unsigned by) -> int {
    unsigned v = 0, *p = (unsigned*)buf + word;
    HIPCHK(hipMemcpy(&v, p, 4, hipMemcpyDeviceToHost));
    v += by;
    HIPCHK(hipMemcpy(p, &v, 4, hipMemcpyHostToDevice));
    return 0;
  };
  CHK(bump(c->hf_sync.p, pk::ERR * pk::LINE, 1));
  for (DevBuf* b : sync_bufs(c)) {
    CHK(bump(b->p, 0, 5));
    for (int line : pk::GEN_LINES) CHK(bump(b->p, line * pk::LINE, 3));
    CHK(bump(b->p, pk::TICKET0 + pk::TICKETS - 1, 1));
  }
  for (int half = 0; half < 2; ++half) CHK(bump(c->cw_sync.p, half * pk::CW_HALF, 3));
  return 0;
}
// Diagnostic (tests): the counters between launches -> out[n >= pk::DIAG_WORDS] (vibevoice_hip_diag.h)
extern "C" int vv_diag_sync_words(vv_ctx* c, unsigned* out, int n) {
  if (!c->finalized || n < pk::DIAG_WORDS) FAIL("vv_diag_sync_words before vv_finalize, or out[] shorter than 53 words");
  HIPCHK(hipDeviceSynchronize());
  std::vector<unsigned> h(2 * pk::CW_HALF);
  auto max_mod = [&](int w0, int n, int stride, unsigned m) {   // the highest residue of n counters
    unsigned r = 0;
    for (int i = 0; i < n; ++i) r = std::max(r, h[w0 + i * stride] % m);
    return r;
  };
  for (DevBuf* b : sync_bufs(c)) {
    HIPCHK(hipMemcpy(h.data(), b->p, pk::BYTES, hipMemcpyDeviceToHost));
    for (int line = 0; line < pk::LINES; ++line) *out++ = h[line * pk::LINE];
    *out++ = max_mod(pk::TICKET0, pk::TICKETS, 1, pk::TICKET_STEP);
  }
  HIPCHK(hipMemcpy(h.data(), c->cw_sync.p, pk::CW_BYTES, hipMemcpyDeviceToHost));
  for (int half = 0; half < 2; ++half) *out++ = max_mod(half * pk::CW_HALF, pk::CW_LINES, pk::LINE, pk::CW_S[half]);
  return 0;
}

// ------------------------------------------------------------------ diffusion head
// 2n <= 16 rows in the GEMV layout: the layer as one launch (head_m16.hip) while the context is
// the device's only registered one; 0 = two GEMV launches (A/B and tests)
static std::atomic<int> g_head_m16{1};
extern "C" int vv_head_m16(int on) {
  g_head_m16 = on;   // A/B variants: bit 1 / bit 3 HeadM16Args::a_first on / off (default: > 8 rows),
                     // bit 2 the down weights' earlier issue point
  return 0;
}
// layers l >= 1 build the A side distributed (HeadM16Args::pre) from the previous
// layer's row partials; 0 = every workgroup transforms the whole A side
static std::atomic<int> g_head_m16_pre{1};
extern "C" int vv_head_m16_pre(int on) {
  g_head_m16_pre = on;
  return 0;
}
static std::atomic<unsigned long long*> g_head_m16_stamps{nullptr};
extern "C" int vv_head_m16_stamps(void* buf) {   // diagnostic: [256][16] per-workgroup phase stamps
  g_head_m16_stamps = (unsigned long long*)buf;
  return 0;
}
// step s's final layer + DPM and step s + 1's noisy projection as ONE launch
// (head_fin.hip) at 2n <= 16 rows with the head's weights cache-resident; 0 = the
// two launches (A/B and tests)
static std::atomic<int> g_head_fin{1};
extern "C" int vv_head_fin(int on) {
  g_head_fin = on ? 1 : 0;
  return 0;
}

// One record per vv_diffusion_sample call (DESIGN.md "How a diffusion sample picks its kernels"), all ints:
// vv_diag_head_route's words.  R: 2n rows.  keep: the per-step head weights (noisy, gate|up, down, final: 170 MB at
// 1.5B) are re-read by every diffusion step: default cache policy keeps them in the Infinity Cache (256 MB) across the
// S steps; VibeVoice-Large's (925 MB per step; 231 MB per rank at TP = 4) stream non-temporal like the LM's.
// sharded: x is summed over the ranks after every layer.  m16: a layer is one k_head_m16 launch, with pre (the A side
// built distributed above 4 rows, the noisy projection then k_head_noisy16: at 2 - 4 rows the whole A side is 18 - 36
// KB per CU and the extra grid wait costs more than it saves, n = 1 head sample 659 us whole vs 688 us distributed),
// a_first (the A side ahead of every weight load: at 16 rows a whole head sample 890 -> 860 us, at 2 rows 595 -> 603
// us; tools/head_m16_stamps.py) and late_down.  fin: k_head_fin fuses step s's final layer with step s + 1's noisy
// projection for an EVEN number nfused of steps [s0, S - 1), so that the latents, the DPM history and the state rows
// ping-pong back to x_io / m1 / xh for the last step's final layer.  epi_dpm: CFG + DPM is the final GEMM's epilogue.
struct HeadPlan { int R, keep, sharded, m16, pre, a_first, late_down, fin, nfused, s0, epi_dpm; };
// The rule, from plain values (vv_diag_head_route): the three switches (one snapshot each), wbytes the head layers'
// weight bytes, fit_* the answers of head_m16_fits and head_fin_fits at R rows.
static HeadPlan head_route(int head_tp, int head_gemv, int tp_size, int comm, int m16, int m16_pre, int fin, int persist,
                           int steps, int R, long long wbytes, bool fit_m16, bool fit_fin) {
  HeadPlan p{};
  p.R = R;
  p.keep = wbytes <= (192ll << 20) && !(head_tp && tp_size > 1);
  p.sharded = head_tp && (tp_size > 1 || comm);   // (a 1-rank communicator: tests)
  p.m16 = m16 && !head_tp && head_gemv && fit_m16 && persist;
  p.pre = m16_pre && R > 4 && p.m16;
  p.a_first = (m16 & 2) ? 1 : (m16 & 8) ? 0 : R > 8;
  p.late_down = !(m16 & 4);
  p.fin = fin && !head_tp && p.keep && fit_fin && steps >= 3;
  p.nfused = !p.fin ? 0 : (steps - 1) % 2 == 0 ? steps - 1 : steps - 2;
  p.s0 = steps - 1 - p.nfused;
  p.epi_dpm = R <= 16;
  return p;
}
extern "C" int vv_diag_head_route(int head_tp, int head_gemv, int tp_size, int comm, int m16, int m16_pre, int fin,
                                  int persist, int steps, int R, long long wbytes, int fit_m16, int fit_fin, int* out) {
  if (!out) return 1;
  put_words(head_route(head_tp, head_gemv, tp_size, comm, m16, m16_pre, fin, persist, steps, R, wbytes, fit_m16 != 0,
                       fit_fin != 0), out);
  return 0;
}
static HeadPlan head_plan(vv_ctx* c, int n) {
  const vv_config& k = c->cfg;
  return head_route(c->head_tp, c->head_gemv, c->tp_size, c->comm != nullptr, g_head_m16.load(), g_head_m16_pre.load(),
                    g_head_fin.load(), persist_on(c), c->steps, 2 * n,
                    (long long)k.head_layers * 3 * k.head_ffn * k.hidden * sizeof(bf16),
                    head_m16_fits(k.hidden, k.head_ffn, 2 * n), head_fin_fits(k.hidden, k.latent_dim, 2 * n));
}
// test queries: a sample of n rows on c would run k_head_m16 / k_head_fin now; diagnostic: head_plan's eleven words
extern "C" int vv_head_m16_active(vv_ctx* c, int n) { return c && c->finalized && head_plan(c, n).m16 ? 1 : 0; }
extern "C" int vv_head_fin_active(vv_ctx* c, int n) { return c && c->finalized && head_plan(c, n).fin ? 1 : 0; }
extern "C" int vv_diag_head_plan(vv_ctx* c, int n, int* out, int cap) {
  if (!c || !c->finalized || !out || n < 1 || cap < 11) FAIL("vv_diag_head_plan: bad arguments");
  put_words(head_plan(c, n), out);
  return 0;
}

// One rank's plan, buffers and operands of a vv_diffusion_sample call.
struct HeadRun {
  HeadPlan p{};
  int n = 0;
  long long MODW = 0;
  bf16 *cat = nullptr, *condp = nullptr, *xh = nullptr, *mods = nullptr, *sa = nullptr, *act = nullptr, *v = nullptr,
       *m1 = nullptr;
  bf16 *xh2 = nullptr, *lat2 = nullptr, *m12 = nullptr;   // k_head_fin's double buffers (state rows, latents, history)
  const bf16* cond = nullptr;
  RowMap xh_m;
};

// layout, condition rows and cond_proj (step-invariant: once per token)
static int head_begin(vv_ctx* c, int n, const void* pos_h, const void* neg_h, HeadRun& h, hipStream_t st) {
  const vv_config& k = c->cfg;
  const int H = k.hidden, F = k.head_ffn, D = k.latent_dim, L = k.head_layers;
  h.n = n;
  h.MODW = (3LL * L + 2) * H;
  const int R = h.p.R;
  h.cat = (bf16*)c->head_ws.p;
  h.condp = h.cat + (size_t)R * H;
  bf16* sc = h.condp + (size_t)R * H;
  h.xh = sc + (size_t)R * H;
  bf16* a = h.xh + (size_t)R * H;
  h.mods = a + (size_t)R * H;                             // [HEAD_SC steps][R][MODW]
  h.sa = h.mods + (size_t)HEAD_SC * R * h.MODW;           // [HEAD_SC steps][R][H] adaLN inputs
  h.act = h.sa + (size_t)HEAD_SC * R * H;
  h.v = h.act + (size_t)R * F;
  h.m1 = h.v + (size_t)R * D;
  h.lat2 = h.m1 + (size_t)R * D;        // (head_ws: R * D * 3 + max_batch * D * 2 after act)
  h.m12 = h.lat2 + (size_t)R * D;
  h.xh2 = a;                            // (head_ws: the spare [R][H] after xh)
  h.xh_m = rowmap(h.xh, H);
  // condition rows cat[pos_h, neg_h]: used in place when the caller's rows are adjacent
  h.cond = (const bf16*)pos_h;
  if ((const bf16*)neg_h != (const bf16*)pos_h + (size_t)n * H) {
    HIPCHK(hipMemcpyAsync(h.cat, pos_h, (size_t)n * H * sizeof(bf16), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(h.cat + (size_t)n * H, neg_h, (size_t)n * H * sizeof(bf16), hipMemcpyDeviceToDevice, st));
    h.cond = h.cat;
  }
  CHK(gemm(c, gemm_args(c, R, H, H, rowmap(h.cond, H), c->head.cond, EPI_STORE, rowmap(h.condp, H)), st));
  return 0;
}

static int head_gemm(vv_ctx* c, const HeadRun& h, GemmArgs g, hipStream_t st) {
  g.keep = h.p.keep;
  return gemm(c, g, st);
}

// all adaLN modulations ([shift|scale|gate] x L, [shift|scale] final) of up to
// HEAD_SC steps in ONE GEMM: the condition is step-invariant and the timesteps
// are the schedule's, so silu(cond_proj(c) + t_emb[s]) is known for every step
// up front -- the 3LH+2H x H adaLN matrix is read once per chunk, not per step
static int head_mods(vv_ctx* c, const HeadRun& h, int s, hipStream_t st) {
  if (s % HEAD_SC) return 0;
  const int H = c->cfg.hidden, sc = std::min(HEAD_SC, c->steps - s);
  KCHK(launch_head_cond(sc, h.p.R, H, h.condp, (const bf16*)c->temb.p + (size_t)s * H, h.sa, st));
  CHK(gemm(c, gemm_args(c, sc * h.p.R, (int)h.MODW, H, rowmap(h.sa, H), c->head.ada, EPI_STORE,
                        rowmap(h.mods, h.MODW)), st));
  return 0;
}

// x = noisy_images_proj(cat[x, x])  -- both halves read the same n latent rows
static int head_noisy(vv_ctx* c, const HeadRun& h, const void* x_io, hipStream_t st) {
  const int H = c->cfg.hidden, D = c->cfg.latent_dim;
  if (h.p.pre) {   // k_head_noisy16: + the row partials layer 0's distributed A side reads
    HeadNoisyArgs a;
    a.lat = (const bf16*)x_io;
    a.w = c->head.noisy;
    a.x = (bf16*)h.xh;
    a.ssp = (float*)c->m16_buf.p;
    a.n = h.n;
    a.R = h.p.R;
    a.D = D;
    a.ldx = H;
    KCHK(launch_head_noisy16(a, st));
    return 0;
  }
  return head_gemm(c, h, gemm_args(c, h.p.R, H, D, rowmap(x_io, D, h.n, 0), c->head.noisy, EPI_STORE, h.xh_m),
                   st);
}

// layer l of step s: modulate(norm(x)) -> gate|up -> SiLU*up -> down -> x += gate * (.)
// With the FFN sharded (vv_tp_shard_head) this rank holds head_ffn / tp_size of
// the hidden columns: gate|up column-parallel, down row-parallel; rank 0 adds
// the residual, the others contribute gate * partial only (onto zero rows), and
// the caller sums x over the ranks (all-reduce).
static int head_layer(vv_ctx* c, const HeadRun& h, int s, int l, hipStream_t st) {
  const vv_config& k = c->cfg;
  const int H = k.hidden, F = k.head_ffn;
  const HeadLayerW& w = c->headw[l];
  const bf16* mod = h.mods + (size_t)(s % HEAD_SC) * h.p.R * h.MODW;
  const int o = 3 * H * l;
  // modulate(norm(x), shift, scale) fused into gate|up's A load
  GemmArgs g = gemm_args(c, h.p.R, 2 * F, H, h.xh_m, w.gu, EPI_SILU_MUL, rowmap(h.act, F));
  g.xf = xf_norm(w.norm, k.head_eps, mod, h.MODW, o, o + H);
  const bool partial = c->head_tp && c->tp_size > 1 && c->tp_rank > 0;
  if (h.p.m16) {
    // 2n <= 16 rows, GEMV layout: one launch with two grid-wide waits (head_m16.hip)
    HeadM16Args a;
    memset(&a, 0, sizeof(a));
    a.x = h.xh;
    a.out = h.xh;
    a.ldx = H;
    a.mod = mod;
    a.ldmod = h.MODW;
    a.shift_off = o;
    a.scale_off = o + H;
    a.gate_off = o + 2 * H;
    a.R = h.p.R;
    a.eps = k.head_eps;
    a.nw = w.norm;
    a.gu = w.gu;
    a.dn = w.down;
    a.act = h.act;
    a.sync = (unsigned*)c->hf_sync.p;
    a.err = err_word(c);
    a.stamps = g_head_m16_stamps;
    a.a_first = h.p.a_first;
    a.late_down = h.p.late_down;
    a.ssp = (float*)c->m16_buf.p;
    a.xt = (bf16*)((char*)c->m16_buf.p + 16 * 192 * sizeof(float));
    a.pre = h.p.pre;   // (layer 0: the partials of k_head_noisy16)
    KCHK(launch_head_m16(a, st));
    return 0;
  }
  if (!c->head_gemv)
    FAIL("diffusion head: " + std::to_string(h.p.R) + " rows need the GEMV layout (head.<l>.gu_w / down_w), which this "
         "engine did not bind");
  CHK(head_gemm(c, h, g, st));
  g = gemm_args(c, h.p.R, H, F, rowmap(h.act, F), w.down, EPI_RES, h.xh_m);
  g.epi.res = partial ? rowmap(c->zero_rows.p, H) : h.xh_m;
  g.epi.gate = rowmap(mod + o + 2 * H, h.MODW);
  return head_gemm(c, h, g, st);
}

// final layer: modulate(norm_final(x)) -> linear -> CFG + DPM-Solver++ step on x
static int head_final(vv_ctx* c, const HeadRun& h, int s, void* x_io, float cfg_scale, const float* sde_noise,
                      hipStream_t st) {
  const vv_config& k = c->cfg;
  const int H = k.hidden, D = k.latent_dim, L = k.head_layers;
  const bf16* mod = h.mods + (size_t)(s % HEAD_SC) * h.p.R * h.MODW;
  DpmCoef e = c->coef[s];
  e.cfg = cfg_scale;
  // sde-dpmsolver++: this step's [2n, D] fp32 draw; rows [0, n) update the live latents
  const float* zs = sde_noise ? sde_noise + (size_t)s * h.p.R * D : nullptr;
  GemmArgs g = gemm_args(c, h.p.R, D, H, h.xh_m, c->head.final, EPI_STORE, rowmap(h.v, D));
  g.xf = xf_norm(nullptr, k.head_eps, mod, h.MODW, 3 * H * L, 3 * H * L + H);
  if (h.p.epi_dpm) {
    g.epi.kind = EPI_CFG_DPM;
    g.dpm.n = h.n;
    g.dpm.k = e;
    g.dpm.x = (bf16*)x_io;
    g.dpm.m1 = h.m1;
    g.dpm.noise = zs;
    CHK(head_gemm(c, h, g, st));
  } else {
    CHK(head_gemm(c, h, g, st));
    KCHK(launch_cfg_dpm(h.n, D, e, h.v, (bf16*)x_io, h.m1, zs, st));
  }
  return 0;
}

// Diagnostic (bench.py's roofline of the head FFN layer): the condition rows
// and step 0's modulations as vv_diffusion_sample sets them up, then `reps`
// passes over the head_layers FFN layers alone (the kernels the loop launches
// for them at this n: the fused layer, or gate|up + down), on stream st.
extern "C" int vv_head_layers_replay(vv_ctx* c, int n, const void* pos_h, const void* neg_h, int reps,
                                     vv_stream vst) {
  hipStream_t st = (hipStream_t)vst;
  if (!c->finalized || c->steps == 0) FAIL("vv_head_layers_replay: engine not finalized or no schedule");
  if (n <= 0 || n > c->cfg.max_batch) FAIL("vv_head_layers_replay: bad n");
  HeadRun h;
  h.p = head_plan(c, n);
  if (h.p.sharded) FAIL("vv_head_layers_replay: sharded head");
  CHK(head_begin(c, n, pos_h, neg_h, h, st));
  CHK(head_mods(c, h, 0, st));
  for (int r = 0; r < reps; ++r)
    for (int l = 0; l < c->cfg.head_layers; ++l) CHK(head_layer(c, h, 0, l, st));
  return 0;
}

int vv_tp_shard_head(vv_ctx* c, int on) {
  if (on && c->tp_size > 1 && c->cfg.head_ffn % 32) FAIL("vv_tp_shard_head: the local head FFN width must be a multiple of 32");
  c->head_tp = on ? 1 : 0;
  return 0;
}

// lat / m1 read, lat_out / m1_out written; the state rows h.xh read, xo written
static int head_fin(vv_ctx* c, const HeadRun& h, int s, const bf16* lat, bf16* lat_out, const bf16* m1, bf16* m1_out,
                    bf16* xo, float cfg_scale, const float* sde_noise, hipStream_t st) {
  const vv_config& k = c->cfg;
  const int H = k.hidden, D = k.latent_dim, L = k.head_layers;
  HeadFinArgs a;
  memset(&a, 0, sizeof(a));
  a.n = h.n;
  a.R = h.p.R;
  a.eps = k.head_eps;
  a.shift_off = 3 * H * L;
  a.scale_off = 3 * H * L + H;
  a.ldmod = h.MODW;
  a.x = h.xh;
  a.mod = h.mods + (size_t)(s % HEAD_SC) * h.p.R * h.MODW;
  a.fw = c->head.final;
  a.k = c->coef[s];
  a.k.cfg = cfg_scale;
  a.lat = lat;
  a.lat_out = lat_out;
  a.m1 = m1;
  a.m1_out = m1_out;
  a.noise = sde_noise ? sde_noise + (size_t)s * h.p.R * D : nullptr;
  a.nw = c->head.noisy;
  a.xo = xo;
  a.ssp = h.p.pre ? (float*)c->m16_buf.p : nullptr;   // (layer 0's distributed A side at > 4 rows)
  KCHK(launch_head_fin(a, st));
  return 0;
}

int vv_diffusion_sample(vv_ctx* c, int n, const void* pos_h, const void* neg_h, void* x_io, float cfg_scale,
                        const float* sde_noise, vv_stream vst) {
  hipStream_t st = (hipStream_t)vst;
  if (!c->finalized || c->steps == 0) FAIL("vv_diffusion_sample: engine not finalized or no schedule");
  if (n <= 0) return 0;
  const vv_config& k = c->cfg;
  if (n > k.max_batch) FAIL("vv_diffusion_sample: n > max_batch");
  const int H = k.hidden, L = k.head_layers;
  HeadRun h;
  h.p = head_plan(c, n);
  const bool sharded = h.p.sharded;
  if (sharded && !c->comm)
    FAIL("sharded diffusion head without a communicator (vv_tp_init; one process: vv_diffusion_sample_group)");
  CHK(head_begin(c, n, pos_h, neg_h, h, st));
  const int R = h.p.R, nfused = h.p.nfused, s0 = h.p.s0;
  bf16* lat[2] = {(bf16*)x_io, h.lat2};
  bf16* hist[2] = {h.m1, h.m12};
  bf16* xs[2] = {h.xh, h.xh2};
  int cur = 0;
  for (int s = 0; s < c->steps; ++s) {
    h.xh = xs[cur];
    h.xh_m = rowmap(h.xh, H);
    h.m1 = hist[cur];
    CHK(head_mods(c, h, s, st));
    if (!(nfused && s > s0)) CHK(head_noisy(c, h, lat[cur], st));   // (else: the previous k_head_fin)
    for (int l = 0; l < L; ++l) {
      CHK(head_layer(c, h, s, l, st));
      if (sharded && !g_tp_null) {   // x = sum over the ranks (rank 0 carried the residual)
        const ncclResult_t r = ncclAllReduce(h.xh, h.xh, (size_t)R * H, ncclBfloat16, ncclSum, c->comm, st);
        if (r != ncclSuccess) FAIL(std::string("ncclAllReduce (head): ") + ncclGetErrorString(r));
      }
    }
    if (nfused && s >= s0 && s + 1 < c->steps) {
      CHK(head_fin(c, h, s, lat[cur], lat[cur ^ 1], hist[cur], hist[cur ^ 1], xs[cur ^ 1], cfg_scale, sde_noise, st));
      cur ^= 1;
    } else {
      CHK(head_final(c, h, s, lat[cur], cfg_scale, sde_noise, st));
    }
  }
  if (cur != 0) FAIL("vv_diffusion_sample: internal (latent buffers did not return)");
  return 0;
}

int vv_diffusion_sample_group(int nr, vv_ctx* const* ctxs, int n, const void* pos_h, const void* neg_h, void* x_io,
                              float cfg_scale, const float* sde_noise, vv_stream vst) {
  hipStream_t st = (hipStream_t)vst;
  if (nr < 1 || nr > 8) FAIL("vv_diffusion_sample_group: 1..8 ranks");
  if (n <= 0) return 0;
  HeadRun h[8];
  SumRows sr;
  sr.n = nr;
  for (int r = 0; r < nr; ++r) {
    vv_ctx* c = ctxs[r];
    if (c->tp_rank != r || c->tp_size != nr || !c->head_tp)
      FAIL("vv_diffusion_sample_group: engine r must be TP rank r of n with a sharded head (vv_tp_shard_head)");
    if (!c->finalized || c->steps != ctxs[0]->steps) FAIL("vv_diffusion_sample_group: engines not finalized alike");
    if (n > c->cfg.max_batch) FAIL("vv_diffusion_sample_group: n > max_batch");
    h[r].p = head_plan(c, n);
    CHK(head_begin(c, n, pos_h, neg_h, h[r], st));
    sr.p[r] = h[r].xh;
  }
  const vv_config& k = ctxs[0]->cfg;
  const long long count = (long long)h[0].p.R * k.hidden;
  for (int s = 0; s < ctxs[0]->steps; ++s) {
    for (int r = 0; r < nr; ++r) {
      CHK(head_mods(ctxs[r], h[r], s, st));
      CHK(head_noisy(ctxs[r], h[r], x_io, st));
    }
    for (int l = 0; l < k.head_layers; ++l) {
      for (int r = 0; r < nr; ++r) CHK(head_layer(ctxs[r], h[r], s, l, st));
      KCHK(launch_sum_rows(sr, count, st));
    }
    // the latent update once (every rank would compute the same; rank 0's x is the sum)
    CHK(head_final(ctxs[0], h[0], s, x_io, cfg_scale, sde_noise, st));
  }
  return 0;
}

static int connector(vv_ctx* c, const ConnW& w, int n, int din, RowMap x, RowMap out, const RowMap* res,
                     hipStream_t st) {
  const int H = c->cfg.hidden;
  bf16* t1 = (bf16*)c->codec_ws.p;
  bf16* t2 = t1 + (size_t)c->cfg.max_batch * H;
  RowMap t1m = rowmap(t1, H), t2m = rowmap(t2, H);
  CHK(gemm(c, gemm_args(c, n, H, din, x, w.fc1_w, EPI_STORE, t1m, w.fc1_b), st));
  // LlamaRMSNorm(eps=1e-6) (modeling_vibevoice.py:62) fused into fc2's A load
  GemmArgs g = gemm_args(c, n, H, H, t1m, w.fc2_w, res ? EPI_RES : EPI_STORE, out, w.fc2_b);
  g.xf = xf_norm(w.norm, 1e-6f);
  if (res) g.epi.res = *res;
  CHK(gemm(c, g, st));
  return 0;
}

int vv_connector(vv_ctx* c, int which, int n, const void* x, void* out, vv_stream vst) {
  hipStream_t st = (hipStream_t)vst;
  if (!c->finalized) FAIL("vv_connector before vv_finalize");
  const int H = c->cfg.hidden;
  const int din = which == 0 ? c->cfg.latent_dim : c->cfg.semantic_dim;
  // chunk rows through the max_batch-sized connector workspace
  for (int r0 = 0; r0 < n; r0 += c->cfg.max_batch) {
    const int m = std::min(c->cfg.max_batch, n - r0);
    CHK(connector(c, which == 0 ? c->conn_ac : c->conn_se, m, din, rowmap((const bf16*)x + (size_t)r0 * din, din),
                  rowmap((bf16*)out + (size_t)r0 * H, H), nullptr, st));
  }
  return 0;
}

int vv_codec_step(vv_ctx* c, int n, const int* slots, const void* latent, void* audio_out, void* sem_out,
                  void* embeds_out, const int* embed_rows, vv_stream vst) {
  hipStream_t st = (hipStream_t)vst;
  if (!c->finalized) FAIL("vv_codec_step before vv_finalize");
  if (n <= 0) return 0;
  if (n > c->cfg.max_batch) FAIL("vv_codec_step: n > max_batch");
  const int H = c->cfg.hidden, D = c->cfg.latent_dim, S = c->cfg.semantic_dim;
  ConvNet& dn = c->dec;
  ConvNet& sn = c->sem;
  const int hop = dn.T[dn.nst - 1];
  // decoder input: latent / scaling - bias  (modeling_vibevoice_inference.py:651)
  KCHK(launch_latent_to_dec(n, D, (const bf16*)latent, c->scaling, c->bias,
                            buf_in_rows(dn.stem, 1, slots), st));
  // decoder -> audio chunk (also written as the semantic encoder's input rows)
  CHK(convnet_run(c, dn, n, slots, rowmap(audio_out, 1, hop, hop), buf_in_rows(sn.stem, hop, slots), st));
  CHK(convnet_roll(dn, n, slots, 0, st));
  // semantic encoder -> [n, S]
  bf16* sem = sem_out ? (bf16*)sem_out : (bf16*)c->codec_ws.p + (size_t)c->cfg.max_batch * 2 * H;
  CHK(convnet_run(c, sn, n, slots, rowmap(sem, S, 1, S), RowMap{}, st));
  CHK(convnet_roll(sn, n, slots, 0, st));
  // next input embedding = acoustic_connector(latent) + semantic_connector(sem)  (:682-687)
  if (embeds_out) {
    bf16* ac = (bf16*)c->codec_ws.p + (size_t)c->cfg.max_batch * 3 * H;
    RowMap acm = rowmap(ac, H);
    CHK(connector(c, c->conn_ac, n, D, rowmap(latent, D), acm, nullptr, st));
    RowMap outm = rowmap(embeds_out, H, 1, H, embed_rows);
    CHK(connector(c, c->conn_se, n, S, rowmap(sem, S), outm, &acm, st));
  }
  return 0;
}

int vv_codec_reset(vv_ctx* c, int n, const int* slots, vv_stream vst) {
  hipStream_t st = (hipStream_t)vst;
  if (n <= 0) return 0;
  CHK(convnet_roll(c->dec, n, slots, 1, st));
  CHK(convnet_roll(c->sem, n, slots, 1, st));
  return 0;
}

// The two halves of vv_codec_step as separate calls: the reference's standalone
// tokenizer API (acoustic_tokenizer.decode / semantic_tokenizer.encode with a
// VibeVoiceTokenizerStreamingCache, modular_vibevoice_tokenizer.py:1081-1108,
// 193-256), one frame per call.  Slot state is the same per-slot ConvBuf
// history vv_codec_step keeps.
int vv_codec_decode(vv_ctx* c, int n, const int* slots, const void* z, void* audio_out, vv_stream vst) {
  hipStream_t st = (hipStream_t)vst;
  if (!c->finalized) FAIL("vv_codec_decode before vv_finalize");
  if (n <= 0) return 0;
  if (n > c->cfg.max_batch) FAIL("vv_codec_decode: n > max_batch");
  ConvNet& dn = c->dec;
  const int hop = dn.T[dn.nst - 1];
  // z is already the decoder input (latent / scaling - bias, done by the caller):
  // identity scale / bias keep the copy bit-exact
  const bf16* one = (const bf16*)c->unit_sb.p;
  KCHK(launch_latent_to_dec(n, c->cfg.latent_dim, (const bf16*)z, one, one + 1, buf_in_rows(dn.stem, 1, slots), st));
  CHK(convnet_run(c, dn, n, slots, rowmap(audio_out, 1, hop, hop), RowMap{}, st));
  CHK(convnet_roll(dn, n, slots, 0, st));
  return 0;
}

int vv_codec_encode(vv_ctx* c, int n, const int* slots, const void* audio, void* sem_out, vv_stream vst) {
  hipStream_t st = (hipStream_t)vst;
  if (!c->finalized) FAIL("vv_codec_encode before vv_finalize");
  if (n <= 0) return 0;
  if (n > c->cfg.max_batch) FAIL("vv_codec_encode: n > max_batch");
  ConvNet& sn = c->sem;
  const int hop = c->dec.T[c->dec.nst - 1];
  // audio rows [n, hop] -> the encoder stem's input rows of each slot (one row of
  // hop channels-last samples per slot)
  RowMap in = rowmap(sn.stem.base + (long long)sn.stem.ctx * sn.stem.C, hop, 1, sn.stem.sB, slots);
  KCHK(launch_copy_rows1(n, hop, (const bf16*)audio, hop, in, st));
  const int S = c->cfg.semantic_dim;
  CHK(convnet_run(c, sn, n, slots, rowmap(sem_out, S, 1, S), RowMap{}, st));
  CHK(convnet_roll(sn, n, slots, 0, st));
  return 0;
}

int vv_codec_reset_net(vv_ctx* c, int net, int n, const int* slots, vv_stream vst) {
  hipStream_t st = (hipStream_t)vst;
  if (n <= 0) return 0;
  if (net != 0 && net != 1) FAIL("vv_codec_reset_net: net must be 0 (acoustic decoder) or 1 (semantic encoder)");
  CHK(convnet_roll(net == 0 ? c->dec : c->sem, n, slots, 1, st));
  return 0;
}

// Non-streaming encode of nv clips of L samples (zero-padded to a common L) by
// one of the σ-VAE encoders, laid out for this call: nv slots, T0 = L.  The
// per-layer right zero padding of the strided-conv inputs (ConvBuf rows past
// the input, zeroed per call) is the reference's non-streaming extra padding
// (modular_vibevoice_tokenizer.py:127-133, :393-408), so a clip that ends in a
// partial frame gives ceil(L / hop) frames as the reference does.
static int encode_nonstreaming(vv_ctx* c, ConvNet& net, int nf, int out_ch, int nv, int L, const void* audio, void* out,
                               hipStream_t st) {
  if (net.slots != nv || net.T0 != L) {
    convnet_shape(c, net, false, net.wp, nf, 1, out_ch, L, nv);   // (the channels, so the weights, as vv_finalize's)
    CHK(convnet_alloc(net, 7));
  } else {
    HIPCHK(hipMemsetAsync(net.state.p, 0, net.state.bytes, st));
  }
  CHK(c->slot_scratch.ensure(sizeof(int) * (size_t)std::max(nv, 1024)));
  std::vector<int> ids(nv);
  for (int i = 0; i < nv; ++i) ids[i] = i;
  int* d_ids = (int*)c->slot_scratch.p;
  HIPCHK(hipMemcpyAsync(d_ids, ids.data(), nv * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpy2DAsync(net.stem.base + net.stem.ctx, net.stem.sB * sizeof(bf16), audio, (size_t)L * sizeof(bf16),
                          (size_t)L * sizeof(bf16), nv, hipMemcpyDeviceToDevice, st));
  const int Tl = net.T[net.nst - 1];
  CHK(convnet_run(c, net, nv, d_ids, rowmap(out, out_ch, Tl, (long long)Tl * out_ch), RowMap{}, st));
  HIPCHK(hipStreamSynchronize(st));  // d_ids scratch is reused by the next call
  return 0;
}

int vv_acoustic_encode(vv_ctx* c, int nv, int L, const void* audio, void* mean_out, vv_stream vst) {
  if (!c->finalized) FAIL("vv_acoustic_encode before vv_finalize");
  if (!c->has_aenc) FAIL("acoustic encoder weights not bound");
  if (nv <= 0 || L <= 0) return 0;
  return encode_nonstreaming(c, c->aenc, c->cfg.ac_enc_n_filters, c->cfg.latent_dim, nv, L, audio, mean_out,
                             (hipStream_t)vst);
}

int vv_semantic_encode(vv_ctx* c, int nv, int L, const void* audio, void* mean_out, vv_stream vst) {
  if (!c->finalized) FAIL("vv_semantic_encode before vv_finalize");
  if (nv <= 0 || L <= 0) return 0;
  return encode_nonstreaming(c, c->senc, c->cfg.sem_n_filters, c->cfg.semantic_dim, nv, L, audio, mean_out,
                             (hipStream_t)vst);
}

int vv_vae_features(vv_ctx* c, int nv, int frames, const void* mean, const void* stdv, const void* noise, void* feat,
                    vv_stream vst) {
  if (!c->finalized) FAIL("vv_vae_features before vv_finalize");
  KCHK(launch_vae_features(nv * frames, c->cfg.latent_dim, frames, (const bf16*)mean, (const bf16*)stdv,
                           (const bf16*)noise, c->scaling, c->bias, (bf16*)feat, (hipStream_t)vst));
  return 0;
}

int vv_scatter_rows(vv_ctx* c, int n, int C, const void* src, int64_t lds, const int* idx, void* dst, int64_t ldd,
                    vv_stream vst) {
  (void)c;
  // dst[idx[i]] = src[i]: a gather with the roles of the maps swapped
  RowMap dm = rowmap(dst, ldd, 1, ldd, idx);
  KCHK(launch_gather_rows(n, C, (const bf16*)src, lds, nullptr, dm, (hipStream_t)vst));
  return 0;
}

// diagnostic (vv_gemm_tune_apack): vv_gemm_bf16's A is MFMA-fragment packed (k_gemm_xl only)
static std::atomic<int> g_gemm_apack{0};
extern "C" int vv_gemm_tune_apack(int on) {
  g_gemm_apack = on;
  return 0;
}

int vv_gemm_bf16(int M, int N, int K, const void* A, int64_t lda, const void* Wt, const void* bias, int epi, void* Y,
                 int64_t ldy, const void* res, const void* gamma, vv_ctx* c, vv_stream vst) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.M = M;
  g.N = N;
  g.K = K;
  g.ksplit = 1;
  g.a = rowmap(A, lda);
  g.w = (const bf16*)Wt;
  g.ldw = K;
  g.epi.kind = epi;
  g.epi.bias = (const bf16*)bias;
  g.epi.out = rowmap(Y, ldy);
  g.epi.res = rowmap(res, ldy);
  g.epi.gamma = (const bf16*)gamma;
  g.apack = g_gemm_apack;
  if (c) {
    g.ws = (float*)c->splitk_ws.p;
    g.counters = (unsigned*)c->splitk_cnt.p;
  } else {
    // standalone calls (tests): a process-wide split-K workspace
    static DevBuf ws, cnt;
    if (!cnt.p) {
      CHK(ws.ensure(64ull << 20));
      CHK(cnt.ensure(65536 * sizeof(unsigned)));
      HIPCHK(hipMemset(cnt.p, 0, 65536 * sizeof(unsigned)));
    }
    g.ws = (float*)ws.p;
    g.counters = (unsigned*)cnt.p;
  }
  KCHK(launch_gemm(g, (hipStream_t)vst));
  return 0;
}

int vv_gemm_bf16_norm(int M, int N, int K, const void* A, int64_t lda, const void* norm_w, float eps, const void* Wt,
                      int epi, void* Y, int64_t ldy, vv_ctx* c, vv_stream vst) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.M = M;
  g.N = N;
  g.K = K;
  g.ksplit = 1;
  g.a = rowmap(A, lda);
  g.w = (const bf16*)Wt;
  g.ldw = K;
  g.epi.kind = epi;
  g.epi.out = rowmap(Y, ldy);
  g.xf = xf_norm((const bf16*)norm_w, eps);
  if (c) {   // the engine's own dispatch (M > 16: k_rmsnorm once, then the GEMV on normalised rows)
    g.ws = (float*)c->splitk_ws.p;
    g.counters = (unsigned*)c->splitk_cnt.p;
    CHK(gemm(c, g, (hipStream_t)vst));
    return 0;
  }
  KCHK(launch_gemm(g, (hipStream_t)vst));
  return 0;
}

// vv_gemm_bf16 / vv_gemm_bf16_norm on FP8 weight-only storage: codes [N][K] in
// mfma_pack8 order + int8 row exponents; xf 0 = none, 1 = RMSNorm of the A rows
// (norm_w optional); a quantised GemmArgs as the engine builds it (k_gemv_w8, or
// the dequantise-and-bf16 fallback into the context's / a process-wide scratch)
int vv_gemm_w8(int M, int N, int K, const void* A, int64_t lda, const void* codes, const void* exps, int xf,
               const void* norm_w, float eps, const void* bias, int epi, void* Y, int64_t ldy, const void* res,
               vv_ctx* c, vv_stream vst) {
  if (!codes || !exps) FAIL("vv_gemm_w8: null codes / exponents");
  if (xf != XF_NONE && xf != XF_NORM) FAIL("vv_gemm_w8: xf must be 0 (none) or 1 (RMSNorm)");
  if (K % 64 || N % 16) FAIL("vv_gemm_w8: needs K % 64 == 0 and N % 16 == 0");
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.M = M;
  g.N = N;
  g.K = K;
  g.ksplit = 1;
  g.a = rowmap(A, lda);
  g.ldw = K;
  g.w8 = (const unsigned char*)codes;
  g.w8e = (const signed char*)exps;
  g.epi.kind = epi;
  g.epi.bias = (const bf16*)bias;
  g.epi.out = rowmap(Y, ldy);
  g.epi.res = rowmap(res, ldy);
  if (xf == XF_NORM) g.xf = xf_norm((const bf16*)norm_w, eps);
  static DevBuf ws, cnt, scratch;   // standalone calls (tests): process-wide workspaces
  if (c) {
    g.ws = (float*)c->splitk_ws.p;
    g.counters = (unsigned*)c->splitk_cnt.p;
  } else {
    if (!cnt.p) {
      CHK(ws.ensure(64ull << 20));
      CHK(cnt.ensure(65536 * sizeof(unsigned)));
      HIPCHK(hipMemset(cnt.p, 0, 65536 * sizeof(unsigned)));
    }
    g.ws = (float*)ws.p;
    g.counters = (unsigned*)cnt.p;
  }
  if (c && c->w8_scratch.bytes >= (size_t)N * K * sizeof(bf16)) {
    g.w8_scratch = (bf16*)c->w8_scratch.p;
  } else if (!gemv_w8_serves(g)) {
    CHK(scratch.ensure((size_t)N * K * sizeof(bf16)));
    g.w8_scratch = (bf16*)scratch.p;
  }
  if (c) {
    CHK(gemm(c, g, (hipStream_t)vst));
    return 0;
  }
  KCHK(launch_gemm(g, (hipStream_t)vst));
  return 0;
}

// Test hook: after a vv_lm_forward of ntok rows (synchronises the device), the q rows of
// the last layer that ran ([ntok][n_heads * 128], RoPE applied) and, for row i, the K / V
// cache entries of `layer` at (slots[i], pos[i]) ([ntok][n_kv_heads][128] each)
int vv_diag_lm_qkv(vv_ctx* c, int ntok, int layer, const int* slots, const int* pos, void* q_out, void* k_out,
                   void* v_out) {
  if (!c || !c->finalized || !slots || !pos || !q_out || !k_out || !v_out) FAIL("vv_diag_lm_qkv: bad arguments");
  const vv_config& k = c->cfg;
  if (ntok < 1 || (size_t)ntok > c->lm_ws_tokens) FAIL("vv_diag_lm_qkv: no such pass");
  if (layer < 0 || layer >= k.n_layers) FAIL("vv_diag_lm_qkv: bad layer");
  if (c->kv_dtype) FAIL("vv_diag_lm_qkv reads a bf16 KV cache; this engine's is FP8 e4m3 (vv_diag_kv_read)");
  HIPCHK(hipDeviceSynchronize());
  const int H = k.hidden, d = k.head_dim, nhd = k.n_heads * d;
  const bf16* q = (const bf16*)c->lm_ws.p + (size_t)ntok * (2 * (size_t)H + c->qkv_n);
  HIPCHK(hipMemcpy(q_out, q, (size_t)ntok * nhd * sizeof(bf16), hipMemcpyDeviceToDevice));
  for (int i = 0; i < ntok; ++i) {
    if (slots[i] < 0 || slots[i] >= c->lm_slots || pos[i] < 0 || pos[i] >= c->kv.max_ctx) FAIL("vv_diag_lm_qkv: bad slot / position");
    for (int h = 0; h < k.n_kv_heads; ++h) {
      const long long base = (long long)layer * c->kv.s_layer + (long long)slots[i] * c->kv.s_slot + (long long)h * c->kv.s_head;
      bf16* ko = (bf16*)k_out + ((size_t)i * k.n_kv_heads + h) * d;
      bf16* vo = (bf16*)v_out + ((size_t)i * k.n_kv_heads + h) * d;
      HIPCHK(hipMemcpy(ko, c->kv.k + base + (long long)pos[i] * d, d * sizeof(bf16), hipMemcpyDeviceToDevice));
      // V: blocks of 32 positions, [dim][position] (common.h v_off): dim i at stride 32 elements
      const long long v0 = base + (long long)(pos[i] >> 5) * (128 * 32) + (pos[i] & 31);
      HIPCHK(hipMemcpy2D(vo, sizeof(bf16), c->kv.v + v0, 32 * sizeof(bf16), sizeof(bf16), d, hipMemcpyDeviceToDevice));
    }
  }
  return 0;
}

// Diagnostics: positions [p0, p1) of `slot` as bf16 rows [layer][kv_head][p][128] (device
// memory), K and V: read returns the cached values (dequantised under FP8 KV), write stores
// rows (quantised under FP8 KV).  Synchronous.
static int diag_kv_rows(vv_ctx* c, int slot, int p0, int p1, void* k_rows, void* v_rows, int write, const char* who) {
  if (!c || !c->finalized || !k_rows || !v_rows) FAIL(std::string(who) + ": bad arguments");
  if (slot < 0 || slot >= c->lm_slots || p0 < 0 || p1 > c->cfg.max_ctx || p0 > p1)
    FAIL(std::string(who) + ": slot / positions out of range");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());
  KCHK(launch_kv_rows(c->kv, c->kv8, c->cfg.n_layers, c->cfg.n_kv_heads, slot, p0, p1, (bf16*)k_rows, (bf16*)v_rows,
                      write, nullptr));
  HIPCHK(hipDeviceSynchronize());
  return 0;
}
int vv_diag_kv_read(vv_ctx* c, int slot, int p0, int p1, void* k_out, void* v_out) {
  return diag_kv_rows(c, slot, p0, p1, k_out, v_out, 0, "vv_diag_kv_read");
}
int vv_diag_kv_write(vv_ctx* c, int slot, int p0, int p1, const void* k_in, const void* v_in) {
  return diag_kv_rows(c, slot, p0, p1, const_cast<void*>(k_in), const_cast<void*>(v_in), 1, "vv_diag_kv_write");
}

// Diagnostics: the streaming codec's per-slot conv buffers (net 0 = acoustic decoder, 1 =
// semantic encoder) in convnet_alloc's order: stem, per stage tr[i] (i > 0) and mix[i][0..depth),
// head.  Layout: host only, out = {count, then {kind (0 stem, 1 transition, 2 mixer, 3 head),
// stage, block, ctx, T, rows, C} per buffer}.  State: the slot's [rows][C] slice of every buffer,
// back to back in that order, into a device bf16 buffer (synchronous; plain copies).
struct CodecBufRef {
  const ConvBuf* b;
  int kind, stage, block;
};
static std::vector<CodecBufRef> codec_bufs(const ConvNet& n) {
  std::vector<CodecBufRef> v;
  v.push_back({&n.stem, 0, 0, 0});
  for (int i = 0; i < n.nst; ++i) {
    if (i > 0) v.push_back({&n.tr[i], 1, i, 0});
    for (int j = 0; j < n.depth[i]; ++j) v.push_back({&n.mix[i][j], 2, i, j});
  }
  v.push_back({&n.head, 3, n.nst - 1, 0});
  return v;
}
int vv_diag_codec_layout(vv_ctx* c, int net, int* out, int n) {
  if (!c || !c->finalized || !out) FAIL("vv_diag_codec_layout: bad arguments");
  if (net != 0 && net != 1) FAIL("vv_diag_codec_layout: net must be 0 (acoustic decoder) or 1 (semantic encoder)");
  const std::vector<CodecBufRef> v = codec_bufs(net == 0 ? c->dec : c->sem);
  if (n < 1 + 7 * (int)v.size()) FAIL("vv_diag_codec_layout: out[] too short (" + std::to_string(1 + 7 * v.size()) + " words)");
  out[0] = (int)v.size();
  int* o = out + 1;
  for (const CodecBufRef& r : v) {
    const int w[7] = {r.kind, r.stage, r.block, r.b->ctx, r.b->T, r.b->rows, r.b->C};
    for (int k = 0; k < 7; ++k) *o++ = w[k];
  }
  return 0;
}
int vv_diag_codec_state(vv_ctx* c, int net, int slot, void* out, int64_t capacity_elems) {
  if (!c || !c->finalized || !out) FAIL("vv_diag_codec_state: bad arguments");
  if (net != 0 && net != 1) FAIL("vv_diag_codec_state: net must be 0 (acoustic decoder) or 1 (semantic encoder)");
  const ConvNet& cn = net == 0 ? c->dec : c->sem;
  if (slot < 0 || slot >= cn.slots) FAIL("vv_diag_codec_state: slot out of range");
  const std::vector<CodecBufRef> v = codec_bufs(cn);
  long long total = 0;
  for (const CodecBufRef& r : v) total += r.b->sB;
  if (capacity_elems < total) FAIL("vv_diag_codec_state: capacity short (" + std::to_string(total) + " elements)");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());
  bf16* o = (bf16*)out;
  for (const CodecBufRef& r : v) {
    HIPCHK(hipMemcpy(o, r.b->base + (long long)slot * r.b->sB, (size_t)r.b->sB * sizeof(bf16), hipMemcpyDeviceToDevice));
    o += r.b->sB;
  }
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

// Diagnostic: only the attention launch of `layer` over the context's own cache, no append:
// nq query rows q [nq][n_heads * 128] (device) at (slots[i], pos[i]) (device tables; row i
// attends keys [0, pos[i]]) -> out [nq][n_heads * 128].  form: 0 = the decode kernel as
// launch_attn plans it (splits by vv_attn_tune; in-kernel merge or k_attn_merge), 1 = the
// prefill kernel, 2 = decode with the deferred merge (<= 8 splits), 3 = decode with the
// grouped merge (groups of 2 splits, <= 8 groups); 2 and 3 leave partials that o_proj merges
// in a pass -- here a diagnostic kernel merges them (launch_attn_finish).
int vv_diag_attn_ctx(vv_ctx* c, int layer, int nq, const void* q, const int* slots, const int* pos, int form,
                     void* out, vv_stream vst) {
  if (!c || !c->finalized || !q || !slots || !pos || !out || nq < 1) FAIL("vv_diag_attn_ctx: bad arguments");
  const vv_config& k = c->cfg;
  if (layer < 0 || layer >= k.n_layers) FAIL("vv_diag_attn_ctx: bad layer");
  if (form < 0 || form > 3) FAIL("vv_diag_attn_ctx: form must be 0..3");
  hipStream_t st = (hipStream_t)vst;
  std::vector<int> hp(nq), hs(nq);
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipMemcpy(hp.data(), pos, nq * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hs.data(), slots, nq * sizeof(int), hipMemcpyDeviceToHost));
  int maxp = 0;
  for (int i = 0; i < nq; ++i) {
    if (hs[i] < 0 || hs[i] >= c->lm_slots || hp[i] < 0 || hp[i] >= k.max_ctx) FAIL("vv_diag_attn_ctx: bad slot / position");
    maxp = std::max(maxp, hp[i] + 1);
  }
  const int d = k.head_dim;
  AttnArgs at;
  memset(&at, 0, sizeof(at));
  at.kv8 = c->kv8;
  at.kv = c->kv;
  at.nq = nq;
  at.nh = k.n_heads;
  at.nkv = k.n_kv_heads;
  at.layer = layer;
  at.prefill = form == 1;
  at.nsplit = at.prefill ? 1 : attn_plan(nq, k.n_kv_heads, maxp, &at.chunk);
  if (at.prefill) at.chunk = 64;
  at.defer = form == 2;
  if (form == 2 && (at.nsplit < 2 || at.nsplit > 8)) FAIL("vv_diag_attn_ctx: the deferred merge takes 2..8 splits");
  if (form == 3) {
    at.group = 2;
    at.ngroups = (at.nsplit + 1) / 2;
    if (at.nsplit < 2 || at.ngroups > 8) FAIL("vv_diag_attn_ctx: the grouped merge takes 2..16 splits");
  }
  if ((size_t)nq * k.n_kv_heads * std::max(1, at.ngroups) > 65536) FAIL("attention split tickets exhausted");
  CHK(c->attn_part.ensure(attn_part_bytes(nq, k.n_heads, at.nsplit, at.ngroups)));
  at.counters = (unsigned*)c->attn_cnt.p;
  at.scale = 1.0f / sqrtf((float)d);
  at.q = (const bf16*)q;
  at.out = (bf16*)out;
  at.slots = slots;
  at.pos = pos;
  attn_part_carve(at, c->attn_part.p);
  KCHK(launch_attn(at, st));
  if (at.defer || at.group) KCHK(launch_attn_finish(at, st));
  return 0;
}

int vv_weights_quantized(vv_ctx* c) { return c && c->finalized && c->quantized ? 1 : 0; }

int vv_attention_bf16(int nq, int nh, int nkv, const void* q, const void* k_cache, const void* v_cache,
                      int64_t s_slot, int64_t s_head, const int* slots, const int* pos, int max_pos_p1, void* out,
                      vv_ctx* c, vv_stream vst) {
  if (!c) FAIL("vv_attention_bf16: needs an engine for split workspaces");
  KVLayout kv;
  kv.k = (bf16*)k_cache;
  kv.v = (bf16*)v_cache;
  kv.s_layer = 0;
  kv.s_slot = s_slot;
  kv.s_head = s_head;
  kv.d = 128;
  kv.max_ctx = (int)(s_head / 128);
  if (s_head % (128 * 32)) FAIL("vv_attention_bf16: the V cache is blocked by 32 positions (s_head % 4096 != 0)");
  AttnArgs at;
  memset(&at, 0, sizeof(at));
  int chunk = 0;
  // the slot count is unknown here: auto keeps k_attn (vv_attn_prefill(1) forces k_attn_pf)
  at.prefill = attn_use_prefill(nq, nq) ? 1 : 0;
  if (at.prefill && s_head % (128 * 64))
    FAIL("vv_attention_bf16: the prefill kernel stages 64 keys at a time (s_head % 8192 != 0)");
  at.nsplit = at.prefill ? 1 : attn_plan(nq, nkv, max_pos_p1, &chunk);
  if (at.nsplit > 1) {
    if ((size_t)nq * nkv > 65536) FAIL("attention split tickets exhausted");
    CHK(c->attn_part.ensure(attn_part_bytes(nq, nh, at.nsplit, 0)));
  }
  at.nq = nq;
  at.nh = nh;
  at.nkv = nkv;
  at.layer = 0;
  at.chunk = chunk;
  at.scale = 1.0f / sqrtf(128.f);
  at.q = (const bf16*)q;
  at.out = (bf16*)out;
  at.slots = slots;
  at.pos = pos;
  at.kv = kv;
  at.counters = (unsigned*)c->attn_cnt.p;
  attn_part_carve(at, c->attn_part.p);
  at.stamps = g_attn_stamps;
  KCHK(launch_attn(at, (hipStream_t)vst));
  return 0;
}

int vv_rmsnorm_bf16(int M, int C, const void* x, int64_t ldx, const void* w, float eps, void* y, int64_t ldy,
                    vv_stream vst) {
  return rmsnorm(M, C, rowmap(x, ldx), rowmap(y, ldy), (const bf16*)w, eps, (hipStream_t)vst);
}

}  // extern "C"
