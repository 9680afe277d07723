/*
 * tiler_slider_search.h — C-ABI of the on-device breadth-first solver (lib/libtiler_slider_search.so).
 *
 * A second library beside libtiler_slider_hip.so: it shares the data layout, ts_dims, ts_state and ts_status of
 * tiler_slider.h (every pointer a DEVICE pointer owned by the caller, `stream` a hipStream_t as void*, every call
 * asynchronous, no allocation, no retained pointers) and has an ABI version of its own.
 *
 * The reference has no solver.  What is searched is defined by the reference alone:
 *   a move  = TilerSliderEnv.step / GameState.move    ref: explainrl/environment/environment.py:100-143,
 *                                                          explainrl/environment/state.py:120-170
 *   won     = GameState.is_won                        ref: explainrl/environment/state.py:172-186
 * i.e. exactly what ts_step and ts_is_won of tiler_slider.h compute - in both colour modes, with repeated targets,
 * with n_tiles != n_targets (multi-colour: never won; single colour: the SETS of cells are compared) and with zero
 * tiles.  Cell ids >= S*S are clamped to S*S - 1 as the step kernels clamp them.
 *
 * The search runs over the index space  idx = sum_t cell_t * (S*S)^t  of all placements of the T tiles, kept as
 * bitmaps in LDS; it supports S <= 8 and (S*S)^T <= 65536 (ts_solve_states).  Larger boards need a hash set in global
 * memory - a different kernel, not part of this library.
 */
#ifndef TILER_SLIDER_SEARCH_H
#define TILER_SLIDER_SEARCH_H

#include "tiler_slider.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_SEARCH_ABI_VERSION 1
#define TS_SOLVE_MAX_SIZE 8
#define TS_SOLVE_MAX_STATES 65536
#define TS_SOLVE_MAX_DEPTH 32767

#define TS_SOLVE_NONE (-1)  /* the reachable set was exhausted: no sequence of moves solves the board */
#define TS_SOLVE_DEPTH (-2) /* not solved within max_depth moves, and unexpanded states remain */

int32_t ts_search_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_search_last_hip_error(void);

/* (S*S)^T, the size of the index space the search runs over, if ts_solve supports these dims; 0 if it does not
 * (S > 8, or (S*S)^T > 65536); a negative ts_status for invalid dims (NULL, negative counts, more tiles than
 * cells, a size or a count above TS_MAX_*).  Host only. */
int64_t ts_solve_states(const ts_dims *dims);

/* For every board, from its CURRENT cells st->pos (not from init): breadth-first search over the moves of ts_step.
 *   moves[n]  int16: 0 if ts_is_won holds as the board stands; else the least d in 1..max_depth such that some
 *             sequence of d moves reaches a won board; else TS_SOLVE_NONE / TS_SOLVE_DEPTH.  Precisely, with F(d) the
 *             set of states first reached after d moves (F(0) = the board as it stands): the search stops at the first d
 *             with F(d) empty (TS_SOLVE_NONE), else at d = max_depth with F(d) not empty (TS_SOLVE_DEPTH: the states of
 *             F(max_depth) were never expanded - also when expanding them would have reached nothing new).
 *   best[n]   uint8 (optional, may be NULL): bit a set <=> moves[n] >= 1 and the board after Move a is
 *             moves[n] - 1 moves from won (so: every first move of every shortest solution).  0 otherwise.
 * Reads pos, tgt, blk only.  Ignores done, step_count and max_steps (as ts_valid_moves does) and writes no state.
 * An illegal move (nothing slides) leads to the same state and is never on a shortest path.
 * TS_ERR_NULL for a missing pointer; TS_ERR_LIMIT where ts_solve_states is 0; TS_ERR_ARG for max_depth < 0 or
 * > TS_SOLVE_MAX_DEPTH; n_boards = 0 is TS_OK without a launch
 * (no pointer is looked at); asynchronous on `stream`. */
int32_t ts_solve(const ts_dims *dims, const ts_state *st, int32_t max_depth, int16_t *moves, uint8_t *best, void *stream);

/* What ts_solve would launch for these dims, computed by the code ts_solve runs before it launches; touches no device.
 * Two forms:
 *   TS_SOLVE_FORM_WAVE   k_solve_wave<S>: one-wave blocks without block barriers; a board is searched by
 *                        lanes_per_board = 1 .. 64 lanes, 64 / lanes_per_board boards per block
 *   TS_SOLVE_FORM_BLOCK  k_solve_block<S>: one board per block of four waves */
#define TS_SOLVE_FORM_NONE 0 /* empty batch: nothing is launched */
#define TS_SOLVE_FORM_WAVE 1
#define TS_SOLVE_FORM_BLOCK 2
typedef struct ts_solve_desc {
  int32_t form;             /* TS_SOLVE_FORM_* */
  int32_t lanes_per_board;  /* threads that search one board */
  int32_t boards_per_block;
  int32_t threads_per_block;
  int32_t bitmap_words;     /* uint32 words of one bitmap = ceil(states / 32) */
  int32_t lds_bytes_board;  /* seven bitmaps and three control words */
  int32_t lds_bytes_block;  /* dynamic LDS requested per block */
  int32_t reserved;
  int64_t states;           /* ts_solve_states(dims) */
  int64_t blocks;           /* grid size */
  char name[64];            /* as rocprofv3 prints it, e.g. "k_solve_wave<4>" */
} ts_solve_desc;
int32_t ts_describe_solve(const ts_dims *dims, ts_solve_desc *desc);

/* Process-wide launch-policy knobs of this library (speed only: both forms run the same search and are under the same
 * tests).  value >= 0 sets, value < 0 only queries; returns the value before the call, -1 for an unknown key.
 *   TS_SOLVE_TUNE_WAVE_MAX_STATES  index spaces up to this size take the wave form, larger ones the block form where
 *       one is compiled (boards 3x3 .. 6x6; any other takes the wave form regardless).  Default 8192 (measured:
 *       DESIGN.md section 11).
 *   TS_SOLVE_TUNE_WORDS_PER_LANE   bitmap words a lane of the wave form scans per pass (1, 2, 4, ...): lanes per board =
 *       ceil(words / value) rounded up to a power of two, at most 64.  Default 1. */
#define TS_SOLVE_TUNE_WAVE_MAX_STATES 0
#define TS_SOLVE_TUNE_WORDS_PER_LANE 1
int64_t ts_search_tuning(int32_t key, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_SEARCH_H */
