/*
 * tiler_slider_rollout.h — C-ABI of the fused on-device rollouts (lib/libtiler_slider_rollout.so).
 *
 * A fourth library beside libtiler_slider_hip.so, libtiler_slider_search.so and libtiler_slider_table.so: it shares the data
 * layout, ts_dims, ts_state, ts_status and the flag / mode bits of tiler_slider.h (every pointer a DEVICE pointer owned by the
 * caller, `stream` a hipStream_t as void*, every call asynchronous, no allocation, no retained pointers), the table format of
 * tiler_slider_table.h, and has an ABI version of its own.
 *
 * ts_rollout plays `steps` steps of every board in ONE launch: a board is loaded once, lives in its lane's registers while
 * the steps are played, draws or looks up each action itself, and is stored once.  THE DEFINITION: for every board n,
 * ts_rollout leaves exactly what this loop over the entry points of the other libraries leaves (k = 0 .. steps - 1):
 *
 *     r[n]   = mix64(key_k + (board_offset + n) * kDrawMul),  key_k = mix64(seed ^ ((step_index + k) * kBoardMul))
 *     rnd[n] = r[n] >> 62                      -- exactly ts_fill_actions(n_boards, seed, board_offset, step_index + k)
 *     a[n]   = TS_ROLLOUT_GIVEN : actions[k][n]
 *              TS_ROLLOUT_RANDOM: rnd[n]
 *              TS_ROLLOUT_TABLE : e = the action output of ts_table_lookup(table, n_rows, rows) on the board as it stands;
 *                                 explore = (r[n] & 0xffffffff) < explore_threshold;
 *                                 a = (explore or e == 255) ? rnd[n] : e
 *     ts_step(dims, st, a, mode, {flags_k, reward_k})
 *
 * (mix64, kDrawMul, kBoardMul: the counter-based stream of ts_fill_actions.)  Where the expert has no move (e == 255: a won or
 * unwinnable board, a row outside the table) the random draw plays: action 255 would leave the board untouched and uncounted,
 * and a board the expert cannot win would never time out.
 *
 * Supported shapes: S <= 8 with n_tiles <= 8 and n_targets <= 8 (a board's dynamic and static state stays in registers);
 * TS_ROLLOUT_TABLE also needs (S*S)^n_tiles <= 65536, the tables' own limit.  Cell ids >= S*S are clamped as the step
 * kernels clamp them.
 */
#ifndef TILER_SLIDER_ROLLOUT_H
#define TILER_SLIDER_ROLLOUT_H

#include "tiler_slider_table.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_ROLLOUT_ABI_VERSION 1
#define TS_ROLLOUT_MAX_STEPS 65535 /* no counter can overflow: |reward| <= 8 * 14 per step */
#define TS_ROLLOUT_MAX_SIZE 8      /* S */
#define TS_ROLLOUT_MAX_TILES 8     /* n_tiles and n_targets */

/* ts_rollout_cfg.policy */
#define TS_ROLLOUT_GIVEN 0  /* actions[k][n] */
#define TS_ROLLOUT_RANDOM 1 /* the stream of ts_fill_actions */
#define TS_ROLLOUT_TABLE 2  /* epsilon-greedy on a distance table */

typedef struct ts_rollout_cfg {
  int32_t steps;              /* K, 0 .. TS_ROLLOUT_MAX_STEPS */
  uint32_t mode;              /* TS_MODE_STRICT or TS_MODE_AUTORESET: ts_step's, unchanged */
  int32_t policy;             /* TS_ROLLOUT_* */
  int32_t write_state;        /* 1: pos / step_count / done are stored back; 0: a playout from where the boards stand, no state
                                 byte is touched */
  const uint8_t *actions;     /* GIVEN: uint8 [K][N]; else unused */
  uint64_t seed;              /* RANDOM and TABLE: the stream (seed, step_index + k, board_offset + n) */
  int64_t step_index;
  int64_t board_offset;
  uint64_t explore_threshold; /* TABLE: 0 .. 2^32, epsilon * 2^32 */
  const uint8_t *table;       /* TABLE: uint8 [n_rows][states] of ts_table_build; may be NULL when n_rows is 0 */
  int64_t n_rows;
  const int32_t *rows;        /* TABLE: int32 [N] or NULL (board n reads row n): ts_table_lookup's contract - a row outside
                                 0 .. n_rows - 1 gives no expert move, and nothing outside the table is read */
} ts_rollout_cfg;

/* Reductions over the loop; each is optional (NULL).  The call needs at least one, or write_state. */
typedef struct ts_rollout_out {
  int32_t *wins;       /* [N] steps with flags_k & TS_FLAG_SUCCESS */
  int32_t *finished;   /* [N] steps with flags_k & (TS_FLAG_SUCCESS | TS_FLAG_TIMEOUT) */
  int32_t *first_win;  /* [N] 1-based k of the first SUCCESS step, 0 if none */
  int32_t *win_moves;  /* [N] sum of step_count after the step, over SUCCESS steps */
  int32_t *reward_sum; /* [N] sum of reward_k, the build-defined Manhattan reward of ts_step_out.reward */
  uint8_t *flags;      /* [N] flags_{K-1} */
  uint8_t *act_log;    /* [K][N] a as played */
  uint8_t *flags_log;  /* [K][N] flags_k */
  void *pos_log;       /* cell_t [K][T][N] pos after step k: the compact form a learner re-encodes with ts_encode */
} ts_rollout_out;

/* bits of ts_describe_rollout's out_mask, one per pointer of ts_rollout_out */
#define TS_ROLLOUT_OUT_WINS 0x001u
#define TS_ROLLOUT_OUT_FINISHED 0x002u
#define TS_ROLLOUT_OUT_FIRST_WIN 0x004u
#define TS_ROLLOUT_OUT_WIN_MOVES 0x008u
#define TS_ROLLOUT_OUT_REWARD_SUM 0x010u
#define TS_ROLLOUT_OUT_FLAGS 0x020u
#define TS_ROLLOUT_OUT_ACT_LOG 0x040u
#define TS_ROLLOUT_OUT_FLAGS_LOG 0x080u
#define TS_ROLLOUT_OUT_POS_LOG 0x100u

int32_t ts_rollout_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_rollout_last_hip_error(void);

/* 1 if ts_rollout plays these dims under this policy, 0 if the shape is beyond it (ts_rollout: TS_ERR_LIMIT), a negative
 * ts_status for invalid dims (TS_ERR_NULL, TS_ERR_DIMS) or an unknown policy (TS_ERR_ARG).  Host only. */
int32_t ts_rollout_supported(const ts_dims *dims, int32_t policy);

/* One launch: k_rollout<S, policy>, one board per lane, no LDS.  Checked in this order, before any HIP call: dims (TS_ERR_NULL,
 * TS_ERR_DIMS), an unsupported shape (TS_ERR_LIMIT), a bad argument (TS_ERR_ARG: mode bits, policy, steps outside
 * 0 .. TS_ROLLOUT_MAX_STEPS, explore_threshold above 2^32, n_rows < 0), then a missing pointer (TS_ERR_NULL: st, out, a state
 * row, actions for GIVEN, table for TABLE with n_rows > 0, or neither an output nor write_state).  cfg itself is needed to know
 * the policy: a NULL cfg is TS_ERR_NULL right after dims.  n_boards = 0 and steps = 0 are TS_OK without a launch: nothing is
 * written and no pointer is looked at.  st->init is read in TS_MODE_AUTORESET only.  Asynchronous on `stream`. */
int32_t ts_rollout(const ts_dims *dims, const ts_state *st, const ts_rollout_cfg *cfg, const ts_rollout_out *out, void *stream);

/* What ts_rollout would launch, computed by the code it runs before it launches; touches no device. */
typedef struct ts_rollout_desc {
  int32_t threads_per_block;
  int32_t lds_bytes;    /* 0: the board lives in registers */
  int64_t blocks;       /* grid size; 0 for an empty batch or steps = 0 (nothing is launched, name is empty) */
  int64_t logged_bytes; /* bytes of act_log + flags_log + pos_log that out_mask asks for */
  char name[64];        /* as rocprofv3 prints it, e.g. "k_rollout<4, 2>" */
} ts_rollout_desc;
int32_t ts_describe_rollout(const ts_dims *dims, const ts_rollout_cfg *cfg, uint32_t out_mask, ts_rollout_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_ROLLOUT_H */
