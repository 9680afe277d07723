/*
 * tiler_slider_targets.h — C-ABI of the trajectory targets (lib/libtiler_slider_targets.so).
 *
 * A seventh library beside the step, search, table, rollout, policy and train libraries: it shares the data layout, ts_dims,
 * ts_state and ts_status of tiler_slider.h (every pointer a DEVICE pointer owned by the caller, `stream` a hipStream_t as void*,
 * every call asynchronous, no allocation, no retained pointers, no state written), the samples of tiler_slider_train.h and the
 * tables of tiler_slider_table.h, and has an ABI version of its own.  It computes what a loss over a logged trajectory is
 * computed AGAINST: per-step rewards, generalised advantage estimates and returns (ts_traj_returns), and the expert's answer on
 * every visited board (ts_traj_labels).  One launch each, one pass over the log per board.
 *
 * THE SAMPLES are those of tiler_slider_train.h: sample (k, n) is board n's level with the cells c[k], where c[0] is `first`
 * (cell_t [T][N]) and c[k] is pos_log[k - 1] for k >= 1.  The cells AFTER step k are pos_log[k]: unlike the train calls,
 * ts_traj_returns reads the last row of pos_log too.  flags_log[k][n] are the TS_FLAG_* of step k, as a rollout logs them.
 *
 * TS_TRAJ_RETURNS.  From the flags of step k
 *
 *     void_k = flags_k & (STEPPED_DONE | AUTORESET | BAD_ACTION)      no transition was played
 *     end_k  = flags_k & (SUCCESS | TIMEOUT)                          the episode ends with this step
 *     m(c)   = the build-defined Manhattan reward of ts_reward on the cells c (an integer <= 0)
 *
 * the reward of a step that is not void is, in real arithmetic,
 *
 *     r_k = w_step + w_win [SUCCESS] + w_timeout [TIMEOUT] + w_invalid [INVALID_MOVE]
 *         + w_dist m(pos_log[k]) + w_progress (m(pos_log[k]) - m(c[k]))
 *
 * and the recursion runs backwards, k = K - 1 .. 0, with a carry A+ that starts at 0.  V_k = values[k][n]; V+_k is 0 where
 * end_k holds, else last_value[n] for k = K - 1 and values[k + 1][n] for an earlier k; every V is 0 where `values` (or
 * `last_value`) is NULL.
 *
 *     void_k:  reward = adv = ret = 0, mask = 0; the carry is left as it is
 *     else:    delta = r_k + gamma V+_k - V_k
 *              A_k   = delta + (end_k ? 0 : gamma lambda A+);   A+ <- A_k
 *              reward = r_k, adv = A_k, ret = A_k + V_k, mask = 1
 *
 * This is GAE(gamma, lambda); with values = NULL and lambda = 1, `ret` is the discounted return-to-go.  BOTH SUCCESS AND TIMEOUT
 * CUT THE BOOTSTRAP: a timeout is treated as the end of the episode, not as a truncation whose value is bootstrapped - that
 * variant is NOT BUILT.  w_progress weighs a PLAIN DIFFERENCE of m; it is NOT gamma-corrected potential-based shaping.
 * Arithmetic is float32; the order of the sum inside r_k and the use of fused multiply-adds are NOT PART OF THE CONTRACT.  The
 * recursion is sequential per board, without atomics, so results are reproducible bit for bit from run to run.
 *
 * Board n of row k of `values` is values[(k * N + n) * value_stride], value_stride 1 or 4 (in elements): with 4, column 0 of
 * a [K][N][4] logits tensor is read in place.  `first` may be NULL when w_progress == 0; pos_log, st->tgt and st->blk (and st
 * itself) may be NULL when w_dist == w_progress == 0 - the cells are then not read at all.  (m() does not look at the
 * obstacles: st->blk is never read by this call.)  Cell ids >= S*S are clamped as everywhere else.  Supported shapes: exactly
 * those of ts_rollout_supported(dims, TS_ROLLOUT_RANDOM).
 *
 * TS_TRAJ_LABELS.  For every sample (k, n): exactly what ts_table_lookup(table, n_rows, rows) writes for a board that stands on
 * c[k] - moves int16, best uint8, action uint8, each [K][N] - with ts_table_lookup's contract for rows outside the table,
 * entries that are no placement, and clamping.  The last row of pos_log is not read; pos_log may be NULL when steps == 1.
 * Supported where ts_table_states(dims) > 0.
 */
#ifndef TILER_SLIDER_TARGETS_H
#define TILER_SLIDER_TARGETS_H

#include "tiler_slider_train.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_TARGETS_ABI_VERSION 1

/* `which` of ts_targets_supported */
#define TS_TARGETS_RETURNS 0
#define TS_TARGETS_LABELS 1

/* `what` of the describe calls: the outputs asked for ... */
#define TS_RETURNS_OUT_REWARD 0x01u
#define TS_RETURNS_OUT_ADV 0x02u
#define TS_RETURNS_OUT_RET 0x04u
#define TS_RETURNS_OUT_MASK 0x08u
/* ... and what a ts_traj_returns call would read beside the flags */
#define TS_RETURNS_IN_CELLS 0x10u      /* w_dist or w_progress is not 0: pos_log and the targets */
#define TS_RETURNS_IN_FIRST 0x20u      /* w_progress is not 0 */
#define TS_RETURNS_IN_VALUES 0x40u     /* values is given */
#define TS_RETURNS_IN_LAST_VALUE 0x80u /* last_value is given */
#define TS_LABELS_OUT_MOVES 0x01u
#define TS_LABELS_OUT_BEST 0x02u
#define TS_LABELS_OUT_ACTION 0x04u

typedef struct ts_returns_in {
  const void *first;        /* cell_t [T][N]: c[0]; may be NULL when w_progress == 0 */
  const void *pos_log;      /* cell_t [K][T][N]; may be NULL when w_dist == w_progress == 0 */
  const uint8_t *flags_log; /* [K][N] */
  const float *values;      /* board n of row k at values[(k * N + n) * value_stride]; may be NULL: every V_k is 0 */
  const float *last_value;  /* [N]; may be NULL: 0 */
  int32_t steps;            /* K, 1 .. TS_ROLLOUT_MAX_STEPS */
  int32_t value_stride;     /* 1 or 4 (checked with or without values) */
  float gamma, lam;         /* each in [0, 1] */
  float w_step, w_win, w_timeout, w_invalid, w_dist, w_progress;
} ts_returns_in;

/* each may be NULL, not all four */
typedef struct ts_returns_out {
  float *reward; /* [K][N] */
  float *adv;    /* [K][N] */
  float *ret;    /* [K][N] */
  uint8_t *mask; /* [K][N]: 1 where a transition was played */
} ts_returns_out;

typedef struct ts_labels_in {
  const void *first;    /* cell_t [T][N]: c[0] */
  const void *pos_log;  /* cell_t [K][T][N]: c[k] = pos_log[k - 1]; may be NULL when steps == 1 */
  const uint8_t *table; /* [n_rows][ts_table_states(dims)], as ts_table_build wrote it; may be NULL when n_rows == 0 */
  const int32_t *rows;  /* [N]: board n reads row rows[n]; NULL: row n */
  int64_t n_rows;
  int32_t steps; /* K, 1 .. TS_ROLLOUT_MAX_STEPS */
  int32_t reserved;
} ts_labels_in;

/* each may be NULL, not all three */
typedef struct ts_labels_out {
  int16_t *moves;  /* [K][N] */
  uint8_t *best;   /* [K][N] */
  uint8_t *action; /* [K][N] */
} ts_labels_out;

int32_t ts_targets_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_targets_last_hip_error(void);

/* 1 / 0: TS_TARGETS_RETURNS exactly ts_rollout_supported(dims, TS_ROLLOUT_RANDOM), TS_TARGETS_LABELS ts_table_states(dims) > 0;
 * a negative status for invalid dims (TS_ERR_LIMIT counts as 0) or another `which` (TS_ERR_ARG).  Host only. */
int32_t ts_targets_supported(const ts_dims *dims, int32_t which);

/* Both calls check, in this order and before any HIP call: dims (the check every library shares: TS_ERR_NULL, TS_ERR_DIMS, and
 * TS_ERR_LIMIT for a size above 32 or more than 255 tiles or targets - BEFORE the NULL check of in / out), in and out
 * (TS_ERR_NULL), an unsupported shape (TS_ERR_LIMIT), a bad argument (TS_ERR_ARG: steps outside 1 .. TS_ROLLOUT_MAX_STEPS;
 * gamma or lam outside [0, 1] or NaN; a value_stride other than 1 or 4; n_rows < 0); then n_boards = 0 is TS_OK without a
 * launch; then a missing pointer (TS_ERR_NULL.  ts_traj_returns: flags_log; where the cells are read and there are tiles
 * pos_log, first if w_progress != 0, and st and st->tgt where there are targets.  ts_traj_labels: st, st->blk, first where
 * there are tiles, pos_log where there are tiles and steps > 1, table where n_rows > 0.  Both: no output at all), then a float
 * pointer - values, last_value, reward, adv, ret - that is not 4-byte aligned (TS_ERR_ARG).
 *
 * One launch, k_traj_returns<S>, one board per lane. */
int32_t ts_traj_returns(const ts_dims *dims, const ts_state *st, const ts_returns_in *in, const ts_returns_out *out, void *stream);

/* One launch, k_traj_labels<S>, one board per lane. */
int32_t ts_traj_labels(const ts_dims *dims, const ts_state *st, const ts_labels_in *in, const ts_labels_out *out, void *stream);

/* What a call would launch, computed by the code it runs before it launches; touches no device. */
typedef struct ts_targets_desc {
  int32_t threads_per_block;
  int32_t lds_bytes;     /* dynamic LDS of a block: 0, neither kernel uses any */
  int32_t chunk_steps;   /* steps of a board whose loads are issued together and held in registers */
  int32_t reserved;
  int64_t blocks;        /* grid size; 0 where nothing is launched (name is empty) */
  int64_t samples;       /* steps * n_boards */
  int64_t bytes_read;    /* algorithmic: the log, the values, the table entries and the level, for `what` */
  int64_t bytes_written; /* the outputs of `what` */
  char name[64];         /* as rocprofv3 prints it, e.g. "k_traj_returns<4>" */
} ts_targets_desc;
/* `what`: TS_RETURNS_OUT_* | TS_RETURNS_IN_*, TS_LABELS_OUT_*; bits beyond those, or no output bit, give TS_ERR_ARG */
int32_t ts_describe_traj_returns(const ts_dims *dims, int32_t steps, uint32_t what, ts_targets_desc *desc);
int32_t ts_describe_traj_labels(const ts_dims *dims, int32_t steps, uint32_t what, ts_targets_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_TARGETS_H */
