/*
 * vibevoice_hip_diag.h — diagnostics of libvibevoice_hip.so: kernel-level entry
 * points (parity tests, benchmarks), launch-plan tuning hooks, per-workgroup
 * timing stamps and benchmark-only switches.  NOT the product interface
 * (include/vibevoice_hip.h is): nothing in vibevoice_amd/ calls these, and the
 * reference has nothing they replace.
 *
 * The hooks set PROCESS-WIDE state (std::atomic words read by every launch of
 * every context): set them only while no other thread is launching work, and
 * restore the built-in value (0 / -1 as documented) afterwards.  Tests use them
 * to pin alternative forms bit-identical to the default; tools/ uses them for
 * same-box A/B runs.
 */
#ifndef VIBEVOICE_HIP_DIAG_H
#define VIBEVOICE_HIP_DIAG_H
#include <stdint.h>

#include "vibevoice_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Switch (benchmarks only): 1 = skip the RCCL all-reduces of communicator
 * engines (outputs wrong), so bench.py --tp can time an LM pass with and
 * without its 2 x n_layers collectives and report their share. */
int vv_tp_null_collective(int on);

/* Benchmarks only: fill the KV cache of `slots` at
 * positions [p0, p1) with deterministic pseudo-random values, so decode can be
 * timed at a long context without a long prefill.  Not a reference operation. */
int vv_kv_synthetic(vv_ctx* c, int n, const int* slots, int p0, int p1, unsigned seed, vv_stream stream);

/* Low-level kernel entry points (used by the parity tests).  W is [N, K] in the
 * MFMA-packed order of vibevoice_amd/weights.py:mfma_pack (csrc/gemm.hip). */
int vv_gemm_bf16(int M, int N, int K, const void* A, int64_t lda, const void* W, const void* bias, int epi,
                 void* Y, int64_t ldy, const void* res, const void* gamma, vv_ctx* ws_ctx, vv_stream st);
int vv_rmsnorm_bf16(int M, int C, const void* x, int64_t ldx, const void* w, float eps, void* y, int64_t ldy,
                    vv_stream st);
/* The same with the A operand RMS-normalised on load (x * rsqrt(mean(x^2) + eps),
 * bf16, times norm_w when not NULL): the fused input_layernorm / ConvRMSNorm
 * producer of the loop's GEMMs (no bias / residual epilogues). */
int vv_gemm_bf16_norm(int M, int N, int K, const void* A, int64_t lda, const void* norm_w, float eps, const void* W,
                      int epi, void* Y, int64_t ldy, vv_ctx* ws_ctx, vv_stream st);
/* vv_gemm_bf16 / vv_gemm_bf16_norm on FP8 weight-only storage: `codes` is the
 * [N, K] e4m3fn matrix in the byte order of weights.py:mfma_pack8
 * (csrc/gemv_w8.hip), `exps` one int8 exponent per output row (scale 2^e).
 * xf: 0 = A as is, 1 = A RMS-normalised on load (norm_w may be NULL).  epi as
 * vv_gemm_bf16 (bias, res optional).  M <= 16 rows run the FP8 GEMV; more rows
 * run the bf16 kernel's instantiation that reads the codes itself (k_gemv,
 * k_gemvw, k_gemm: 17 to 255 rows, and k_gemm's RMSNorm form above that); the
 * LDS-staged prefill tiles, and every call under vv_gemv_w8(0), dequantise the
 * matrix and run the bf16 kernels.  vv_gemm_plan_w8 answers which. */
int vv_gemm_w8(int M, int N, int K, const void* A, int64_t lda, const void* codes, const void* exps, int xf,
               const void* norm_w, float eps, const void* bias, int epi, void* Y, int64_t ldy, const void* res,
               vv_ctx* ws_ctx, vv_stream st);
/* Test / A-B switch: 1 (default) = quantised GEMMs read their codes in the
 * kernel (the FP8 GEMV of gemv_w8.hip up to 16 rows, the bf16 kernels' W8
 * instantiations above); 0 = every quantised GEMM, at every row count,
 * dequantises its matrix into the scratch and runs the bf16 kernels (bit for
 * bit a bf16 engine on the dequantised weights). */
int vv_gemv_w8(int on);
/* Process-wide count of dequantise passes (k_dequant_w8 launches) so far: it
 * stands still while every quantised GEMM reads its codes in the kernel. */
int vv_w8_dequant_launches(void);
/* Test hook: after a vv_lm_forward of ntok rows on ctx (synchronises the
 * device): the q rows the last layer's q|k|v epilogue wrote ([ntok][n_heads x
 * 128], RoPE applied) and the K / V cache entries of `layer` at (slots[i],
 * pos[i]) for each row ([ntok][n_kv_heads][128] each; host slots / pos, device
 * outputs).  ntok must be the row count of that pass. */
int vv_diag_lm_qkv(vv_ctx* ctx, int ntok, int layer, const int* slots, const int* pos, void* q_out, void* k_out,
                   void* v_out);
/* Test hooks on the context's own KV cache, either format (synchronous; device
 * buffers of bf16 rows [layer][kv_head][p1 - p0][128], K and V):
 *   vv_diag_kv_read: positions [p0, p1) of `slot` as cached (dequantised under FP8 KV)
 *   vv_diag_kv_write: store rows there (quantised under FP8 KV)
 *   vv_diag_attn_ctx: only the attention launch of `layer`, no append: nq query
 *     rows q [nq][n_heads x 128] (RoPE applied) at device tables slots / pos (row
 *     i attends keys [0, pos[i]]) -> out [nq][n_heads x 128].  form: 0 = decode
 *     kernel as planned (splits by vv_attn_tune; in-kernel merge or k_attn_merge),
 *     1 = prefill kernel, 2 = decode with the deferred merge (2..8 splits), 3 =
 *     decode with the grouped merge (groups of 2 splits); the partials of 2 and 3,
 *     which o_proj merges in a pass, are merged by a diagnostic kernel. */
int vv_diag_kv_read(vv_ctx* ctx, int slot, int p0, int p1, void* k_out, void* v_out);
int vv_diag_kv_write(vv_ctx* ctx, int slot, int p0, int p1, const void* k_in, const void* v_in);
int vv_diag_attn_ctx(vv_ctx* ctx, int layer, int nq, const void* q, const int* slots, const int* pos, int form,
                     void* out, vv_stream st);
/* Test hooks on the streaming codec's state: the per-slot conv buffers of one net
 * (0 = acoustic decoder, 1 = semantic encoder, as vv_codec_reset_net), each
 * [ctx history rows | rows of the last step][C], in allocation order: the stem,
 * then per stage the transition before it (stages >= 1) and its Block1Ds' mixer
 * buffers, then the head.
 *   vv_diag_codec_layout: host only.  out[0] = the number of buffers, then per
 *     buffer {kind (0 stem, 1 transition, 2 mixer, 3 head), stage, block, ctx, T,
 *     rows, C}; n is the caller's capacity in words (fails, writing nothing, when
 *     it is short).
 *   vv_diag_codec_state: synchronises the device, then copies `slot`'s [rows][C]
 *     slice of every buffer, back to back in layout order, into the device bf16
 *     buffer out (fails, writing nothing, when capacity_elems is short).  Read
 *     only: no kernel, no launch changes.
 * After a vv_codec_step, in every stage form: rows [0, ctx) hold the history the
 * next frame reads; a transition's (and the head's) rows [ctx, ctx + T) hold the
 * previous stage's complete output; a mixer's rows [ctx + T - 6, ctx + T) its
 * block's last normalised rows (the one-launch stage forms store no others). */
int vv_diag_codec_layout(vv_ctx* ctx, int net, int* out, int n);
int vv_diag_codec_state(vv_ctx* ctx, int net, int slot, void* out, int64_t capacity_elems);
/* GQA attention of nq query rows (q [nq, nh*128] bf16, RoPE applied) over a
 * caller-owned cache in the engine layout ([slot][kv_head][ctx][128], strides
 * in elements): row i attends keys [0, pos[i]] of slot slots[i] -> out
 * [nq, nh*128].  max_pos_p1 bounds pos + 1 (launch plan); ws_ctx supplies the
 * split-merge workspace.  (Kernel entry for tests / benchmarks.) */
int vv_attention_bf16(int nq, int nh, int nkv, const void* q, const void* k_cache, const void* v_cache,
                      int64_t s_slot, int64_t s_head, const int* slots, const int* pos, int max_pos_p1, void* out,
                      vv_ctx* ws_ctx, vv_stream st);
/* Tuning hook (benchmarks only): override the GEMV launch plan — waves per
 * workgroup, split-K workgroups, split-K hand-off form (0 fences, 1 sc1),
 * target waves per launch, weight chunks in flight per wave (2/4/8).
 * 0 / -1 restore the built-in plan. */
int vv_gemv_tune(int nw, int ks, int handoff, int target_waves, int u);
/* Tuning hook (benchmarks only): 16-row weight tiles per workgroup of the
 * M <= 16 GEMV (the waves split into tpw groups that share one staging of the
 * A rows); 0 restores the built-in plan. */
int vv_gemv_tune_tpw(int tpw);
/* Tuning hook (benchmarks only): GEMMs with more than m rows (m >= 16) use the
 * tiled MFMA kernel instead of the GEMV family; 0 restores the built-in 64. */
int vv_gemv_tune_maxm(int m);
/* Tuning hook (benchmarks only): 0 = the 16 < M <= 64 GEMVs with >= 256 tiles
 * use k_gemv (A fragments per tile) instead of k_gemvw (A held per K slice
 * across several tiles); 1 = built-in. */
int vv_gemv_tune_wide(int on);
/* Tuning hook (benchmarks only): the largest dynamic LDS (bytes) the M <= 16
 * GEMV may stage its A slice in before it falls back to per-wave A fragment
 * loads, up to 148 KiB (per-kernel opt-in above 64 KB); 0 = built-in (64 KB). */
int vv_gemv_tune_lds(int bytes);
/* Tuning hook (benchmarks only): fused-RMSNorm GEMVs with at least min_m rows
 * (and an eligible shape) stage whole A rows per wave (k_gemv1's RW form: the
 * norm applied in registers, one barrier); 0 restores the built-in 1; -1 = the
 * built-in without the LDS-DMA form for K = 3,584 adaLN rows; 99 = off. */
int vv_gemv_tune_rw(int min_m);
/* Host-only plan query (no device work; tests and tools): the kernel form and
 * launch plan the library uses for an M <= 16 GEMV (xf: 0 none, 1 RMSNorm, 2
 * SiLU-add; has_w / has_mod: norm weight, adaLN shift / scale present).
 * out[7] = {kernel (0 = A staged in LDS, 1 = A fragments from L2), waves, K
 * splits, weight chunks in flight, tiles per workgroup, norm prologue form
 * (0 item per thread, 1 row per wave, 2 row per wave + LDS-DMA rows), dynamic
 * LDS bytes}. Replaces nothing in the reference (the plan is this engine's). */
int vv_gemv_plan(int M, int N, int K, int xf, int has_w, int has_mod, int* out);
/* Host-only query of the same launch decision (csrc/gemm.hip: gemm_decide) for
 * any M and every kernel form, on a device of `cus` compute units (0: none
 * known).  xf as above, 3 = the codec mixer prologue (M samples of one step),
 * 4 = the attention split merge (one split); epi: the epilogue (0 store .. 6
 * CFG + DPM step); keep: the default cache policy for the weights.
 * out[11] = {kind (0 k_gemv1, 1 k_gemv, 2 k_gemvw, 3 FP8 GEMV, 4 k_gemm<64>,
 * 5 k_gemm<32>, 6 k_gemm_big<1>, 7 k_gemm_big<2>, 8 k_gemm_xl, 9 rejected),
 * 16-row A tiles, waves, K splits, weight chunks in flight, tiles per workgroup,
 * norm prologue form, grid x, grid y, workgroup size, dynamic LDS bytes}; n is
 * the caller's capacity in words (fails, writing nothing, when n < 11). */
int vv_gemm_plan(int M, int N, int K, int xf, int has_w, int has_mod, int epi, int keep, int cus, int* out, int n);
/* vv_gemm_plan for an FP8 weight-only operand (vv_gemm_w8's): out[0..10] as
 * above for the same shape in bf16 -- the kernel that runs, on the codes or
 * after the dequantise -- and out[11] = where the codes go: 0 the FP8 GEMV
 * (k_gemv_w8), 1 that kernel's own W8 instantiation, 2 a dequantise pass into
 * the scratch first.  Fails, writing nothing, when n < 12.  Host only. */
int vv_gemm_plan_w8(int M, int N, int K, int xf, int has_w, int has_mod, int epi, int keep, int cus, int* out, int n);
/* Tuning hook (benchmarks / tests): XF-free GEMMs with >= 256 rows,
 * N % 128 == 0, K % 64 == 0 and >= 256 such tiles (or >= 2^30 MACs) take the
 * LDS-staged 128 x 128 tile (k_gemm_big, the prefill projections) with 2 LDS
 * stages (2) or 1 stage (1); 0 = they stay on k_gemm; -1 / 3 = built-in: the
 * 256 x 256 tile (k_gemm_xl) where N % 256 == 0, K % 32 == 0 and there are
 * >= 192 such tiles, else as 2; + 4 = any tile count (tests). */
int vv_gemm_tune_big(int mode);
/* Diagnostic (benchmarks only): M <= 16 GEMV launches write 4 s_memrealtime
 * stamps per workgroup (start, A staged, weights streamed, epilogue stored) to
 * buf (uint64[grid * 4]); NULL turns it off. */
int vv_gemv_stamps(void* buf);
/* Diagnostic (benchmarks only): vv_attention_bf16 launches write 4 stamps per
 * workgroup (start, K/V/Q landed, keys done, output stored); NULL: off. */
int vv_attn_stamps(void* buf);
/* Tuning hook (benchmarks only): attention keys per split (multiple of 32;
 * 0 = built-in) and the largest split count merged inside the attention
 * kernel (more splits go to the separate merge pass; -1 = built-in). */
int vv_attn_tune(int chunk, int merge_in);
/* Tuning hook (benchmarks / tests): the attention kernel for many query rows
 * per slot (prompt prefill): -1 = built-in choice (>= 256 rows and >= 32 rows
 * per slot of the engine -> the 32-row-tile prefill kernel), 0 = always the
 * per-row decode kernel, 1 = always the prefill kernel. */
int vv_attn_prefill(int mode);
/* Diagnostic (benchmarks only): vv_gemm_bf16 reads A in MFMA-fragment order
 * (as the packed weights; the 256 x 256 tile only). */
int vv_gemm_tune_apack(int on);
/* Test / A-B switch: 1 (default) = at 4 < 2n <= 16 rows each head FFN layer
 * is one launch with one grid-wide hand-off (head_m16.hip; within bf16 of the
 * GEMV pair, not bitwise) while ctx is the device's only registered context;
 * 0 = gate|up + down GEMV launches. */
int vv_head_m16(int on);
/* Test query: the m16 word of vv_diag_head_plan: 1 when a head layer of n
 * samples on ctx would run head_m16 now. */
int vv_head_m16_active(vv_ctx* ctx, int n);
/* Diagnostic: per-workgroup s_memrealtime stamps of every head_m16 launch into
 * buf ([256][16] u64, overwritten per launch; NULL = off). */
int vv_head_m16_stamps(void* buf);
/* Diagnostic switch: the LM MLP block at decode with <= 2 rows as one launch
 * (lm_ffn.hip; 1, default) or the gate|up + down GEMV pair (0); and whether
 * the one-launch block applies to this context at ntok rows. */
int vv_lm_ffn(int on);
int vv_lm_ffn_active(vv_ctx* ctx, int ntok);
/* Diagnostic switch for contexts whose MLP projections (gu_w, down_w of every
 * layer) are all bound as FP8: the one-launch block then runs in its W8 form
 * (the same kernels reading the codes; bit for bit the bf16 form on the
 * dequantised weights).  bits: bit 0 = at <= 2 rows (k_lm_ffn), bit 1 = at
 * 3..16 rows (k_lm_ffn16); default 3; 0 = such a context runs the FP8 GEMV pair.
 * Other values are an error.  vv_lm_ffn still gates both forms, a bf16 context
 * is unaffected, and a context with some MLP projections bf16 and some FP8
 * always runs the GEMV pair.  Bumps the workspace epoch (vv_ws_epoch), so
 * captured graphs are re-captured. */
int vv_lm_ffn_w8(int bits);
/* Diagnostic: k_lm_ffn16 launches write per-workgroup phase stamps ([256][16]
 * u64, overwritten per launch; NULL = off). */
int vv_lm_ffn_stamps(void* buf);
/* Diagnostic switch: the diffusion head's step boundary (final layer + DPM of
 * step s, noisy projection of step s + 1) as one launch at 2n <= 16 rows
 * (head_fin.hip; 1, default) or the two GEMV launches (0); and the fin word of
 * vv_diag_head_plan: whether it applies to this context at n samples now. */
int vv_head_fin(int on);
int vv_head_fin_active(vv_ctx* ctx, int n);
/* Diagnostic switch: the LM attention half at decode (input_layernorm .. o_proj
 * + residual, <= 16 rows, contexts <= 4,096 keys or the context's
 * vv_set_lm_attn_max_keys) as one launch (lm_attn.hip;
 * 1, default) or the q|k|v, attention and o_proj launches (0); whether it applies
 * to this context at ntok rows over max_pos_p1 keys; and per-workgroup phase
 * stamps of its launches ([256][16] u64, overwritten per launch; NULL = off). */
int vv_lm_attn(int on);
int vv_lm_attn_active(vv_ctx* ctx, int ntok, int max_pos_p1);
int vv_lm_attn_stamps(void* buf);
/* Diagnostic switch: a bf16-weight, bf16-KV context runs the one-launch LM
 * attention kernel's round-trip form (k_lm_attn<false, 2>: the FP8-KV form's data
 * flow and e4m3 row quantiser, the appended rows stored dequantised in the bf16
 * cache and read as bf16) where it would run the plain form (1), or the plain
 * form (0, default) -- the bits the FP8-KV form must produce. */
int vv_lm_attn_kvround(int on);
/* Diagnostic: the one-launch kernel's attention units for a row of `len` keys
 * (1 .. 2^20): out[0] = steps of 32 keys per unit (1 while len <= 4,096),
 * out[1] = units per (row, kv head) (<= 128); the function the kernel itself
 * evaluates per row (kernels.h la_unit_steps / la_unit_count). */
int vv_diag_lm_attn_plan(int len, int* out);
/* Diagnostic: the key splits of a row of `len` keys (1 .. 2^20) under a decode
 * attention launch planned as `nsplit` splits (1 .. 256) of >= `chunk` keys (a
 * multiple of 32), merged in groups of `group` splits (0: no groups): out[0] =
 * the row's keys per split, out[1] = its active splits, out[2] = the partials
 * its consumer merges (ceil(active / group); the active splits when group = 0);
 * the function the attention, merge and o_proj kernels themselves evaluate per
 * row (attn_dev.h attn_row_splits). */
int vv_diag_attn_row_splits(int len, int nsplit, int chunk, int group, int* out);
/* Diagnostic: the one-launch kernel's form for FP8 weights (w8 0 / 1), the KV form
 * kvq (0 raw bf16 rows, 1 the FP8 cache, 2 the round-trip diagnostic) and a pass
 * planned for `keys` keys (1 .. 2^20): 0 and out[0..2] = (w8, kvq, long) when that
 * form is built (seven are: kvq = 2 with bf16 weights only, kvq != 0 at <= 4,096
 * keys only), nonzero when it is not; the table the launcher itself looks up. */
int vv_diag_lm_attn_form(int w8, int kvq, int keys, int* out);
/* ... and for a pass of `rows` rows (1 .. 32): 0 and out[0..3] = (w8, kvq, long,
 * row tiles) when that form is built.  Eleven are: the seven above at 1 .. 16 rows
 * (row tiles = 1, vv_diag_lm_attn_form's answers) and, at 17 .. 32 rows (row tiles
 * = 2; the per-engine option vv_set_lm_attn_max_rows), kvq = 0 with bf16 or FP8
 * weights, short or long.  Nonzero: kvq != 0 above 16 rows, rows outside 1 .. 32,
 * a null out. */
int vv_diag_lm_attn_form_rows(int w8, int kvq, int keys, int rows, int* out);
/* Diagnostic: the attention half's route for a pass of `rows` rows planned for
 * `keys` keys, as a function of plain values -- how qkv_w / o_w are bound
 * (attn_form: 0 all bf16, 1 all FP8 pairs, 2 a mix), the KV format (0 / 1), the
 * four per-context options (vv_set_lm_attn_w8 / _kv8 / _max_keys / _max_rows),
 * max_ctx, vv_lm_attn_kvround and whether the context has a staging cache.
 * out[0..2] = (one, w8, kvq): one = 0 is the q|k|v, attention and o_proj
 * launches; w8 / kvq name the k_lm_attn form asked for (vv_diag_lm_attn_form_rows
 * says whether it is built).  The function every pass and vv_finalize evaluate;
 * residency, buffers, switches and tensor parallelism are the pass plan's. */
int vv_diag_lm_attn_route(int attn_form, int kv_dtype, int w8, int kv8, int max_keys, int max_rows, int max_ctx,
                          int kvround, int staged, int rows, int keys, int* out);
/* Diagnostic (bench.py): `reps` passes over the LM layers' attention halves alone
 * on ntok decode rows (embeds [ntok][H] as layer 0's input, slots / positions as
 * for vv_lm_forward). */
int vv_lm_attn_replay(vv_ctx* ctx, int ntok, const void* embeds, const int* slot, const int* pos, int max_pos_p1,
                      int reps, vv_stream stream);
/* Diagnostic (bench.py): `reps` passes over the LM layers' MLP blocks alone on
 * ntok decode rows (hidden [ntok][H] in place, act [ntok][I] scratch). */
int vv_lm_mlp_replay(vv_ctx* ctx, int ntok, void* hidden, void* act, int reps, vv_stream stream);
/* Diagnostic switch: head layers l >= 1 at 4 < 2n <= 16 rows build their A side
 * distributed from the previous layer's row partials (1, default) or transform
 * it whole in every workgroup (0). */
int vv_head_m16_pre(int on);
/* Diagnostic (bench.py): the head's condition rows and step-0 modulations for
 * n samples, then `reps` passes over its FFN layers alone (the kernels the loop
 * runs for them at this n), asynchronously on st. */
int vv_head_layers_replay(vv_ctx* ctx, int n, const void* pos_h, const void* neg_h, int reps, vv_stream st);
/* Diagnostic: how a diffusion sample of R = 2n rows picks its kernels,
 * as a function of plain values -- vv_tp_shard_head, whether the head is bound in
 * the GEMV layout, the TP size and whether a communicator exists; the values
 * given to vv_head_m16 / vv_head_m16_pre / vv_head_fin; whether the grid-waiting
 * kernels run on the context now (vv_persistent_active); the schedule's steps;
 * the bytes of the head layers' weights; what head_m16.hip and head_fin.hip
 * answer for the shape at R rows.  out[0..10] = (R, keep, sharded, m16, pre,
 * a_first, late_down, fin, nfused, s0, epi_dpm): keep = the weights stay cache
 * resident; m16 = a layer is one k_head_m16 launch, with pre (the distributed A
 * side: the noisy projection is then k_head_noisy16), a_first and late_down as
 * its arguments; fin = the steps [s0, s0 + nfused) end in k_head_fin; epi_dpm =
 * CFG + DPM is the final GEMM's epilogue, not k_cfg_dpm.  The function every
 * sample, vv_head_layers_replay and the two _active queries evaluate.
 * vv_diag_head_plan: the same words for n samples on a finalized ctx now (cap:
 * the caller's capacity in words, >= 11). */
int vv_diag_head_route(int head_tp, int head_gemv, int tp_size, int comm, int m16, int m16_pre, int fin, int persist,
                       int steps, int R, long long wbytes, int fit_m16, int fit_fin, int* out);
int vv_diag_head_plan(vv_ctx* ctx, int n, int* out, int cap);
/* Test hook: raise the engine's grid-wait error word as a wait that gave up
 * would, and leave its wait counters part-advanced as such a launch does
 * (synchronises the device first): in each of the three counter buffers shard 0,
 * every generation line and one ticket word of csrc/sync_layout.h's table; in
 * the wide codec stages' buffer the first cluster counter of each C. */
int vv_diag_raise_sync_error(vv_ctx* ctx);
/* Test hook: the wait counters (csrc/sync_layout.h) into out[53]; n is the
 * caller's capacity in words (fails, writing nothing, when n < 53).  Per buffer
 * (head, codec stage, LM: 17 words each): word 0 of each of the 16 lines, then
 * max(ticket % 4) over the 48 ticket words.  Then, for the wide codec stages'
 * buffer, max(counter % S) over the 256 cluster counters of C = 256 (S = 8) and
 * of C = 512 (S = 16).  Consistent between launches: every shard line (0-7) a
 * multiple of 32, every generation line (11, 12, 15) a multiple of 8, the three
 * residues 0. */
int vv_diag_sync_words(vv_ctx* ctx, unsigned* out, int n);
/* The rule every grid-waiting launch applies (kernels.h persist_resident + the
 * context half): 1 when a grid of `grid` one-per-CU workgroups with the
 * occupancy query's blocks_per_cu on `cus` CUs and `scratch_bytes` of scratch
 * is resident, the context has the kernels enabled and it is the device's only
 * registered context.  Pure function (no device work). */
int vv_persist_decision(int blocks_per_cu, int cus, int scratch_bytes, int grid, int contexts_on_device, int enabled);
/* A/B / test switch: 1 (default) = each narrow codec stage (C <= 128) as ONE
 * launch (codec_tile.hip: transition conv + 3 Block1Ds [+ head conv], halo
 * recomputed per workgroup); 0 = one k_block launch per Block1D + the
 * transition GEMMs. */
int vv_codec_tile(int on);
/* Diagnostic: the tile launches record per-workgroup s_memrealtime phase stamps
 * ([n][tiles][16] u64 at buf + 4096 x (3 x net + stage), net 0 = decoder, 1 =
 * encoder; stage 0..2 in run order); NULL = off. */
int vv_codec_tile_stamps(void* buf);
/* A/B / test switch: 1 (default) = each wide codec stage (C = 256 / 512) as ONE
 * launch of workgroup clusters (codec_wide.hip) where the grid-waiting kernels
 * run; 0 = k_mix + fc1 / fc2 GEMMs per Block1D.  _active: whether some
 * acoustic-decoder stage of a codec step of n samples on ctx runs as such a
 * launch now (the wide route of vv_diag_codec_plan, below).  _stamps:
 * per-workgroup phase stamps ([n][tiles x S][16] u64 at buf + 8192 x (2 x net +
 * (C == 512))); NULL = off. */
int vv_codec_wide(int on);
/* Diagnostic: wide-stage grids past one resident wave (1: clusters complete in
 * dispatch order; slower at B = 8 than the GEMM path) or only grids resident at
 * once (0, default). */
int vv_codec_wide_over(int on);
int vv_codec_wide_active(vv_ctx* ctx, int n);
int vv_codec_wide_stamps(void* buf);
/* A/B switch: 1 (default) = the balanced many-tile GEMV plan at M >= 8 (one
 * workgroup per CU, 4-5 weight tiles each); 0 = ntile / 8 workgroups. */
int vv_gemv_tune_bal(int on);
/* Tuning hook (benchmarks only): override the GEMV plan (waves, K splits, chunks
 * in flight, tiles per workgroup) for one weight shape N x K at M <= mmax rows;
 * up to 8 overrides; N <= 0 clears them. */
int vv_gemv_tune_shape(int N, int K, int mmax, int nw, int ks, int u, int tpw);
/* Test switch: 1 (default) = the q|k|v RoPE epilogue reads the engine's
 * per-position bf16 cos / sin table; 0 = computes cosf / sinf inline
 * (bit-identical by construction). */
int vv_rope_table(int on);
/* Test switch: on = 1 (default, chunk 128): decode passes of <= 4 rows over up
 * to 8,192 keys run 2..8 key splits of >= `chunk` keys (multiple of 32) and
 * leave their partials to o_proj, which merges them while staging its A rows
 * (bit-identical to the same splits merged in the attention kernel); on = n >= 2:
 * passes of <= n rows (n <= 16); 0 = the attn_plan splits everywhere. */
int vv_attn_defer(int on, int chunk);
/* Test / A-B switch: the longest key split (keys) of the deferred-merge plan
 * above; a context needing longer splits takes the grouped plan below.
 * <= 0 restores the built-in 1,024. */
int vv_attn_defer_max(int keys);
/* Test switch: 1 (default) = decode passes of <= 16 rows over more than 8,192
 * keys run up to 120 splits of >= 256 keys merged in <= 8 groups by each
 * group's last-arriving workgroup, o_proj merging the groups; n >= 2: at most
 * n (<= 128) such splits; 0 = 1,024-key splits merged by k_attn_merge. */
int vv_attn_group(int on);
/* The decode attention's plan for a pass of ntok rows over max_pos_p1 keys,
 * host logic only (CPU tests): out = {prefill, nsplit, chunk, defer, group,
 * ngroups}. */
int vv_attn_pass_plan(int ntok, int lm_slots, int head_dim, int n_kv, int max_pos_p1, int* out);
/* Test switch: 1 (default) = the A rows of the prefill's 256 x 256-tile GEMMs
 * are written MFMA-fragment-packed by their producers (RMSNorm rows for q|k|v
 * and gate|up, gate|up's SiLU*up rows for down); 0 = row-major.  Both give the
 * same bits. */
int vv_norm_pack(int on);
/* Test switch (bit mask, default 3): bit 0 folds each codec Block1D's mixer
 * (norm, depthwise conv, gamma residual, FFN norm) into its fc1 GEMV where
 * <= 16 rows fit (XF_MIX); bit 1 runs whole narrow-stage blocks (C <= 128) as
 * one k_block launch.  0 = separate k_mix + GEMM launches everywhere.  Every
 * mask gives the same bits. */
int vv_codec_mix_fusion(int mask);
/* Test / A-B switch: 1 (default) = a codec stage of Block1Ds at T = 1 and one
 * sample (the acoustic decoder's first, the semantic encoder's last) runs as
 * one persistent launch (codec_stage.hip) while ctx is the device's only
 * context registered for persistent kernels; 0 = one launch per GEMV. */
int vv_codec_stage(int on);
/* Test query: 1 when a one-sample codec step on ctx would run the acoustic
 * decoder's first stage as the persistent launch now (stage 0 of
 * vv_diag_codec_plan(ctx, 0, 1), below, takes the persistent route). */
int vv_codec_stage_active(vv_ctx* ctx);
/* Diagnostic: how one codec stage picks its kernels, as a function of
 * plain values -- the values given to vv_codec_stage / _wide / _tile /
 * _mix_fusion; whether the grid-waiting kernels run on the context now (the
 * two kernels' sync buffers exist in every finalized context); the stage (net,
 * index i of nst, channels C, rows T, blocks, mixer history ctx, ratio rat and
 * channels Cn of the transition before it, the stem's in_ch); and what
 * codec_tile_fits, codec_wide_fits (with the one sync line per cluster),
 * codec_stage_fits, block_lds and gemv_mix_lds answer for it (vv_codec_wide_over
 * acts through the second).  out[0..5] = (route, pre, post, own_pre, xf_mix, R):
 * route 0 one tile launch, 1 one launch of clusters, 2 one persistent launch, 3
 * one k_block per Block1D, 4 fc1 / fc2 GEMMs per Block1D; pre / post = the
 * CT_PRE_* transition and CT_POST_* head conv inside a tile launch; own_pre = the
 * transition before the stage (stage 0: the stem) is a launch of its own; xf_mix
 * (route 4) = the mixer runs in fc1's prologue, not as k_mix; R (routes 3, 4) =
 * rows per mixer workgroup.  The function every codec run and vv_finalize evaluate.
 * vv_diag_codec_plan: a step of n samples on a finalized ctx now, net 0 = the
 * acoustic decoder, 1 = the semantic encoder: out = (stages, own_head, then the
 * six words per stage); own_head = the head conv is a launch of its own; cap:
 * the caller's capacity in words (fails, writing nothing, when short). */
int vv_diag_codec_route(int stage, int wide, int tile, int fusion, int persist, int decoder, int i, int nst, int C,
                        int T, int depth, int ctx, int rat, int Cn, int in_ch, int fit_tile, int fit_wide,
                        int fit_stage, int fit_block, int fit_mix, int* out);
int vv_diag_codec_plan(vv_ctx* ctx, int net, int n, int* out, int cap);
/* Diagnostic: the acoustic decoder's persistent launch of stage `stage`
 * records per-workgroup s_memrealtime stamps into buf ([256][64] u64;
 * nullptr: off). */
int vv_codec_stage_stamps(void* buf, int stage);

#ifdef __cplusplus
}
#endif
#endif
