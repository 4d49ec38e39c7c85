// Layout of the grid-wait counter buffers, for the kernels (persist_dev.h) and
// the engine (allocation, reset, error word, diagnostics).  Host-safe: constants only.
//
// hf_sync, cs_sync and lf_sync share ONE layout of LINES lines of LINE words; a
// buffer leaves unused the lines of kernels that wait on another buffer.
//
//   line    words                                  waits on it (buffer)
//   0-7     shard counters, word 0 of each         every kernel below, in its buffer
//   10      error word (hf_sync's only; every      set by any wait that gave up,
//           kernel's err points at it)             k_codec_wide's included
//   11      generation                             k_codec_stage, k_codec_stage_s<2|8> (cs_sync)
//                                                  k_lm_ffn (lf_sync)
//   12      generation                             k_head_m16 (hf_sync)
//                                                  k_lm_ffn16 (lf_sync)
//   13-14   TICKETS words from TICKET0: one per    k_lm_ffn16 (lf_sync)
//           down column group, + TICKET_STEP
//           arrivals per launch
//   15      generation                             k_lm_attn (lf_sync)
//
// The shard lines of one buffer are shared by every kernel that waits on that
// buffer.  That is sound only because each of them makes G = 256 arrivals per
// wait (G / SHARDS per shard), so between launches every shard counter is a
// multiple of G / SHARDS whichever kernel ran; each kernel static_asserts its
// grid == G.  A generation word is bumped by its one kernel only, SHARDS per wait.
//
// cw_sync is k_codec_wide's own: one line per cluster (word 0 counts the
// cluster's arrivals, S = C / 32 per wait), CW_LINES lines for C = 256 and then
// CW_LINES for C = 512.
#pragma once

namespace pk {
constexpr int G = 256;              // workgroups of a persistent launch (one per CU)
constexpr int LINE = 32;            // words per counter line
constexpr int SHARDS = 8;           // shard lines 0 .. 7 (workgroup w: XCD w % 8)
constexpr int LINES = 16;
constexpr int BYTES = LINES * LINE * 4;
constexpr int ERR = 10;
constexpr int GEN_CODEC_STAGE = 11, GEN_LM_FFN = 11;
constexpr int GEN_HEAD_M16 = 12, GEN_LM_FFN16 = 12;
constexpr int GEN_LM_ATTN = 15;
constexpr int GEN_LINES[] = {GEN_LM_FFN, GEN_LM_FFN16, GEN_LM_ATTN};   // the distinct ones (lf_sync uses all)
constexpr int TICKET0 = 13 * LINE, TICKETS = 48;   // words, not lines
constexpr int TICKET_STEP = 4;      // a group's arrivals per launch (its hidden ranges)

constexpr int CW_LINES = 256;       // wide codec stage clusters per C (n x tiles <= 256 by residency)
constexpr int CW_HALF = CW_LINES * LINE;            // word offset of the C = 512 half
constexpr int CW_BYTES = 2 * CW_HALF * 4;
constexpr unsigned CW_S[2] = {8, 16};               // cluster members at C = 256 / 512
// vv_diag_sync_words: per buffer word 0 of every line + max(ticket % TICKET_STEP); then per cw_sync half max(counter % S)
constexpr int DIAG_WORDS = 3 * (LINES + 1) + 2;

constexpr bool is_gen(int line) { return line == GEN_LINES[0] || line == GEN_LINES[1] || line == GEN_LINES[2]; }
// a counter line of its own: past the shards, inside the buffer, clear of the tickets
constexpr bool line_free(int line) {
  return line >= SHARDS && line < LINES && ((line + 1) * LINE <= TICKET0 || line * LINE >= TICKET0 + TICKETS);
}
static_assert(G % SHARDS == 0 && (SHARDS & (SHARDS - 1)) == 0, "G / SHARDS arrivals per shard, w & (SHARDS - 1)");
static_assert(GEN_LINES[0] != GEN_LINES[1] && GEN_LINES[0] != GEN_LINES[2] && GEN_LINES[1] != GEN_LINES[2] &&
                  !is_gen(ERR),
              "no two named lines coincide");
static_assert(is_gen(GEN_CODEC_STAGE) && is_gen(GEN_HEAD_M16), "every generation line is in GEN_LINES");
static_assert(line_free(ERR) && line_free(GEN_LINES[0]) && line_free(GEN_LINES[1]) && line_free(GEN_LINES[2]),
              "named lines: past the shards, inside the buffer, clear of the tickets");
static_assert(TICKET0 >= (GEN_LM_FFN16 + 1) * LINE && TICKET0 >= (ERR + 1) * LINE, "tickets start after the lines below them");
static_assert(TICKET0 + TICKETS <= GEN_LM_ATTN * LINE, "tickets end before the next used line");
static_assert(TICKET0 + TICKETS <= LINES * LINE, "tickets inside the buffer");
}  // namespace pk
