/*
 * tiler_slider_mixed.h — C-ABI of the mixed rollouts (lib/libtiler_slider_mixed.so).
 *
 * K steps in one launch in which a network and a table expert SHARE the play, decided per board and per step - DAgger's
 * behaviour policy, the expert with probability beta and the learner otherwise -, with the table's answer on every board visited
 * logged by the same launch.  A twentieth library: it shares the data layout, ts_dims, ts_state, ts_status and the flag / mode
 * bits of tiler_slider.h (every pointer a DEVICE pointer owned by the caller, `stream` a hipStream_t as void*, every call
 * asynchronous, no allocation, no retained pointers), the network, the select rules and the outputs of tiler_slider_policy.h, the
 * dense table and its lookup of tiler_slider_table.h, the reach table, its format and its lookup of tiler_slider_rtable.h - both
 * formats are fixed there, and this library restates the lookups from them -, and has an ABI version of its own.
 *
 * THE DEFINITION.  For every board n and k = 0 .. steps - 1, the names are those of tiler_slider_policy.h, tiler_slider_table.h
 * and tiler_slider_rtable.h:
 *
 *     r     = mix64(key_k + (board_offset + n) * kDrawMul)        -- the draw of the action stream, as in ts_policy_rollout
 *     rnd   = r >> 62
 *     z     = the logits of the board as it stands                 -- ts_mlp, computed whether or not the board is done
 *     e     = TS_POLICY_GREEDY / TS_POLICY_SAMPLE on (z, r)        -- exactly ts_policy_rollout's e
 *     (m, bits, x) = moves, best, action of the lookup on the board as it stands (its current cells, done or not):
 *                    TS_MIXED_DENSE: ts_table_lookup(table, n_rows, rows)
 *                    TS_MIXED_REACH: ts_rtable_lookup(table, slots, count, n_rows, rows)
 *     g     = mix64(r ^ TS_MIXED_SALT),  TS_MIXED_SALT = 0x6a09e667f3bcc909
 *     teach   = (g & 0xffffffff) < beta_threshold                   -- beta * 2^32, 0 .. 2^32
 *     explore = (r & 0xffffffff) < explore_threshold
 *     a     = explore ? rnd : (teach && x != 255) ? x : e
 *     who   = explore ? 2 : (teach && x != 255) ? 1 : 0             -- TS_MIXED_WHO_RANDOM / _EXPERT / _NETWORK
 *     the step of tiler_slider.h on (dims, st, a, mode)
 *
 * Where the expert has no move the NETWORK plays, not the random draw: a won board, TS_SOLVE_NONE / TS_SOLVE_DEPTH, a FULL row,
 * TS_RTABLE_ABSENT, a row outside the table, an invalid placement.
 *
 * Everything after `a` is ts_policy_rollout's: the nine outputs and logits_log, write_state, strict and auto-reset modes, and the
 * strict tail - in which the standing board's lookup, like its logits, is constant.
 *
 * Four more optional logs, each [K][N]: expert_log uint8 (x), moves_log int16 (m), best_log uint8 (bits), who_log uint8.  Row k
 * is the answer on the board step k was chosen on, so expert_log, moves_log and best_log are byte for byte what ts_traj_labels /
 * ts_rexpert_labels give on the same rollout's start and pos_log.
 *
 * THE TABLE IS READ when beta_threshold != 0 or one of expert_log, moves_log, best_log is asked for.  Otherwise no byte of it is
 * read - `dense`, `table` and `count` may then be NULL -, and who_log is filled without a lookup.  The table is read only and
 * must not change while the launch runs.  The probe's promises hold as in tiler_slider_rexpert.h: at most `slots` reads per
 * probe, each masked into the board's row, and nothing of table or count is read for a row index outside 0 .. n_rows - 1; a
 * dense lookup reads five bytes of the board's row.  No atomics are used: a call gives the same bits on every run.
 *
 * Supported shapes: TS_MIXED_DENSE - ts_policy_supported(dims, hidden) and ts_table_states(dims) > 0;
 *                   TS_MIXED_REACH - ts_policy_supported(dims, hidden) and ts_rtable_supported(dims).
 */
#ifndef TILER_SLIDER_MIXED_H
#define TILER_SLIDER_MIXED_H

#include "tiler_slider_policy.h"
#include "tiler_slider_rtable.h"
#include "tiler_slider_table.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_MIXED_ABI_VERSION 1
#define TS_MIXED_SALT 0x6a09e667f3bcc909ull

/* ts_mixed_cfg.kind */
#define TS_MIXED_DENSE 0
#define TS_MIXED_REACH 1

/* who_log */
#define TS_MIXED_WHO_NETWORK 0
#define TS_MIXED_WHO_EXPERT 1
#define TS_MIXED_WHO_RANDOM 2

/* ts_policy_cfg's fields with their meaning, and the expert */
typedef struct ts_mixed_cfg {
  int32_t steps;       /* K, 0 .. TS_ROLLOUT_MAX_STEPS */
  uint32_t mode;       /* TS_MODE_STRICT or TS_MODE_AUTORESET */
  int32_t select;      /* TS_POLICY_* */
  int32_t write_state; /* 1: pos / step_count / done are stored back; 0: a playout, no state byte is touched */
  uint64_t seed;
  int64_t step_index;
  int64_t board_offset;
  uint64_t explore_threshold; /* 0 .. 2^32, epsilon * 2^32 */
  uint64_t beta_threshold;    /* 0 .. 2^32, beta * 2^32 */
  int32_t kind;               /* TS_MIXED_* */
  int32_t reserved;
  const uint8_t *dense;  /* TS_MIXED_DENSE: uint8 [n_rows][ts_table_states(dims)] of ts_table_build */
  const uint64_t *table; /* TS_MIXED_REACH: uint64 [n_rows][slots] of ts_rtable_build */
  int64_t slots;         /* TS_MIXED_REACH: a power of two, 2 .. 2^31 */
  const int32_t *count;  /* TS_MIXED_REACH: int32 [n_rows] of ts_rtable_build */
  int64_t n_rows;
  const int32_t *rows;   /* int32 [N] or NULL (board n reads row n) */
} ts_mixed_cfg;

/* ts_policy_out's ten fields with their meaning, and the four logs.  Each is optional (NULL); the call needs at least one, or
 * write_state. */
typedef struct ts_mixed_out {
  int32_t *wins;
  int32_t *finished;
  int32_t *first_win;
  int32_t *win_moves;
  int32_t *reward_sum;
  uint8_t *flags;
  uint8_t *act_log;
  uint8_t *flags_log;
  void *pos_log;
  float *logits_log;   /* [K][N][4], 16-byte aligned */
  uint8_t *expert_log; /* [K][N] x */
  int16_t *moves_log;  /* [K][N] m, 2-byte aligned */
  uint8_t *best_log;   /* [K][N] bits */
  uint8_t *who_log;    /* [K][N] TS_MIXED_WHO_* */
} ts_mixed_out;

/* out_mask of the describe call: the TS_ROLLOUT_OUT_* bits, TS_POLICY_OUT_LOGITS_LOG, and */
#define TS_MIXED_OUT_EXPERT_LOG 0x400u
#define TS_MIXED_OUT_MOVES_LOG 0x800u
#define TS_MIXED_OUT_BEST_LOG 0x1000u
#define TS_MIXED_OUT_WHO_LOG 0x2000u

int32_t ts_mixed_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_mixed_last_hip_error(void);

/* 1 where ts_mixed_rollout takes these dims, this width and this kind (above: Supported shapes), 0 where it does not, a negative
 * ts_status for invalid dims (TS_ERR_NULL, TS_ERR_DIMS); an unknown kind is judged by the policy shape alone - 0 where that is
 * unsupported - and then gives TS_ERR_ARG.  Host only. */
int32_t ts_mixed_supported(const ts_dims *dims, int32_t hidden, int32_t kind);

/* One launch: k_mixed_rollout<S, select, kind>, one board per lane.  Checked in this order, before any HIP call:
 *   1. dims: the dims check every library shares (TS_ERR_NULL, TS_ERR_DIMS, and TS_ERR_LIMIT for a size above 32 or more than 255
 *      tiles or targets - BEFORE the NULL checks: a 33x33 call with a NULL cfg is TS_ERR_LIMIT);
 *   2. cfg or mlp NULL (TS_ERR_NULL);
 *   3. an unsupported shape or width (TS_ERR_LIMIT); an unknown kind is judged by the policy shape alone and then gives TS_ERR_ARG;
 *   4. a bad argument (TS_ERR_ARG): mode bits, select, steps outside 0 .. TS_ROLLOUT_MAX_STEPS, explore_threshold or
 *      beta_threshold above 2^32, n_rows < 0, and for TS_MIXED_REACH slots no power of two in 2 .. 2^31;
 *   5. n_boards = 0 and steps = 0 are TS_OK without a launch: nothing is written and no further pointer is looked at;
 *   6. a missing pointer (TS_ERR_NULL): st, out, a state row (blk, step_count, done, pos with tiles, init with tiles in
 *      TS_MODE_AUTORESET, tgt with targets), a parameter of the network, neither an output nor write_state, and - only where THE
 *      TABLE IS READ (above) and n_rows > 0 - dense (TS_MIXED_DENSE), table or count (TS_MIXED_REACH);
 *   7. a logits_log that is not 16-byte aligned or a moves_log that is not 2-byte aligned (TS_ERR_ARG).
 * Asynchronous on `stream`. */
int32_t ts_mixed_rollout(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_mixed_cfg *cfg, const ts_mixed_out *out,
                         void *stream);

/* What a call would launch, computed by the code it runs before it launches; touches no device. */
typedef struct ts_mixed_desc {
  int32_t threads_per_block;
  int32_t lds_bytes;      /* dynamic LDS of a block, as ts_policy_desc's: the second layer, the staged tile-plane weights, hs */
  int32_t weights_in_lds; /* 1: the tile-plane weights are staged in LDS; 0: gathered from global memory (or there are none) */
  int32_t table_read;     /* 1: THE TABLE IS READ (above) - a uniform branch of the kernel, not another kernel */
  int64_t blocks;         /* grid size; 0 where nothing is launched (name is empty) */
  int64_t logged_bytes;   /* bytes of the eight logs that out_mask asks for */
  char name[64];          /* as rocprofv3 prints it, e.g. "k_mixed_rollout<5, 1, 1>" */
} ts_mixed_desc;
/* dims, cfg or desc NULL is TS_ERR_NULL; then checks 1, 3, 4 and 5 of ts_mixed_rollout, in its order. */
int32_t ts_describe_mixed_rollout(const ts_dims *dims, int32_t hidden, const ts_mixed_cfg *cfg, uint32_t out_mask, ts_mixed_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_MIXED_H */
