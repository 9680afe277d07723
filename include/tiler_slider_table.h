/*
 * tiler_slider_table.h — C-ABI of the distance-to-win tables (lib/libtiler_slider_table.so).
 *
 * A third library beside libtiler_slider_hip.so and libtiler_slider_search.so: it shares the data layout, ts_dims,
 * ts_state and ts_status of tiler_slider.h (every pointer a DEVICE pointer owned by the caller, `stream` a hipStream_t
 * as void*, every call asynchronous, no allocation, no retained pointers), the answers TS_SOLVE_NONE / TS_SOLVE_DEPTH
 * and the limits of tiler_slider_search.h, and has an ABI version of its own.
 *
 * A board's level - its obstacles `blk` and its targets `tgt` - never changes for the life of an environment: ts_reset
 * and the auto-reset of ts_step only put the tiles back.  So the optimal cost-to-go of EVERY placement of the tiles is
 * computed once per level (ts_table_build) and then read wherever the board stands (ts_table_lookup), instead of one
 * breadth-first search per board and step (ts_solve).  Slides cannot be undone, so the table is not a search from the
 * goal: every placement looks at its four successors, round after round.
 *
 * A move and a won board are what ts_step and ts_is_won of tiler_slider.h compute (tiler_slider_search.h names the
 * reference lines); cell ids >= S*S are clamped to S*S - 1 as the step kernels clamp them.  Supported shapes are those of
 * ts_solve: S <= 8 and (S*S)^T <= 65536.
 */
#ifndef TILER_SLIDER_TABLE_H
#define TILER_SLIDER_TABLE_H

#include "tiler_slider_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_TABLE_ABI_VERSION 1
#define TS_TABLE_MAX_DEPTH 252 /* the largest distance an entry can hold, and the largest max_depth */
#define TS_TABLE_INVALID 253   /* not a placement: a tile on a blocked cell, or two tiles on one cell */
#define TS_TABLE_DEEP 254      /* not resolved when the rounds were cut at max_depth */
#define TS_TABLE_NONE 255      /* no sequence of moves wins from there */

int32_t ts_table_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_table_last_hip_error(void);

/* Entries of one board's row = (S*S)^T if these dims are supported, 0 if they are not, a negative ts_status for invalid
 * dims: the values of ts_solve_states.  Host only. */
int64_t ts_table_states(const ts_dims *dims);

/* table: uint8 [n_boards, states], row-major, states = ts_table_states(dims); entry idx = sum_t cell_t * (S*S)^t of row n
 * is, for board n's level (blk, tgt) and the tiles on cells cell_0 .. cell_{T-1}:
 *     TS_TABLE_INVALID  a tile on a blocked cell or two tiles on one cell.  Decided before the win test and never
 *                       computed: no move leads from a valid placement to an invalid one.
 *     0                 ts_is_won holds on that placement
 *     d = 1 .. 252      the least number of ts_step moves from that placement to a won one
 *     TS_TABLE_NONE / TS_TABLE_DEEP   with R(d) the valid placements at distance exactly d: the board stops at the first d
 *                       with R(d) empty, and everything unresolved becomes TS_TABLE_NONE; else it stops at d = max_depth
 *                       with R(d) not empty, and everything unresolved becomes TS_TABLE_DEEP (also placements that no
 *                       number of further rounds would have resolved).
 * Reads blk and tgt only (st->pos may be NULL), writes no state and every entry of the table exactly once.
 * TS_ERR_NULL for a missing pointer; TS_ERR_LIMIT where ts_table_states is 0; TS_ERR_ARG for max_depth < 0 or
 * > TS_TABLE_MAX_DEPTH; n_boards = 0 is TS_OK without a launch (no pointer is looked at); asynchronous on `stream`. */
int32_t ts_table_build(const ts_dims *dims, const ts_state *st, int32_t max_depth, uint8_t *table, void *stream);

/* For every board, from its CURRENT cells st->pos: its own entry and the entries of its four successors, five byte reads
 * of one row of `table` (uint8 [n_rows, states]).  One board per lane, no LDS.  Each output is optional (NULL), at least
 * one is required:
 *   moves[n]   int16: the entry d = 0 .. 252 as it is; TS_TABLE_NONE and TS_TABLE_INVALID -> TS_SOLVE_NONE;
 *              TS_TABLE_DEEP -> TS_SOLVE_DEPTH
 *   best[n]    uint8: bit a set <=> moves[n] >= 1 and the entry of the board after Move a is moves[n] - 1
 *   action[n]  uint8: the lowest set bit of best[n], 255 if there is none (ts_step treats 255 as a bad action and
 *              leaves the board untouched)
 * With a complete table (no TS_TABLE_DEEP in the row) moves and best are exactly ts_solve's outputs.
 * rows: int32 [n_boards] or NULL.  Board n reads row rows[n]; NULL means row n.  A table of L levels serves any number
 * of boards that replicate them.  THE CALLER'S CONTRACT: the row was built for the board's level (same blk, same tgt, same
 * dims but n_boards); the kernel cannot know.  A row index outside 0 .. n_rows - 1 yields TS_SOLVE_NONE, 0 and 255, and
 * nothing outside the table is read.  A board standing on an invalid placement is out of contract: it reports
 * TS_SOLVE_NONE, 0 and 255 and reads nothing outside its row.
 * Reads pos and blk only, writes no state.  TS_ERR_NULL for a missing pointer (table may be NULL when n_rows is 0) or no
 * output at all; TS_ERR_LIMIT where ts_table_states is 0; TS_ERR_ARG for n_rows < 0; n_boards = 0 is TS_OK without a
 * launch (no pointer is looked at); asynchronous on `stream`. */
int32_t ts_table_lookup(const ts_dims *dims, const ts_state *st, const uint8_t *table, int64_t n_rows, const int32_t *rows,
                        int16_t *moves, uint8_t *best, uint8_t *action, void *stream);

/* What ts_table_build would launch for these dims, computed by the code ts_table_build runs before it launches; touches no
 * device.  Two forms of one body:
 *   TS_TABLE_FORM_WAVE   k_table_wave<S>: one-wave blocks without block barriers; a board is worked by
 *                        lanes_per_board = 1 .. 64 lanes, 64 / lanes_per_board boards per block
 *   TS_TABLE_FORM_BLOCK  k_table_block<S>: one board per block of four waves */
#define TS_TABLE_FORM_NONE 0 /* empty batch: nothing is launched */
#define TS_TABLE_FORM_WAVE 1
#define TS_TABLE_FORM_BLOCK 2
typedef struct ts_table_desc {
  int32_t form;             /* TS_TABLE_FORM_* */
  int32_t lanes_per_board;  /* threads that work on one board */
  int32_t boards_per_block;
  int32_t threads_per_block;
  int32_t bitmap_words;     /* uint32 words of one bitmap = ceil(states / 32) */
  int32_t lds_bytes_board;  /* three bitmaps and two control words */
  int32_t lds_bytes_block;  /* dynamic LDS requested per block */
  int32_t lds_bytes_max;    /* the bound every launch of this library stays within: 64 KiB, the default limit of a block */
  int64_t states;           /* ts_table_states(dims) */
  int64_t blocks;           /* grid size */
  int64_t table_bytes;      /* n_boards * states */
  char name[64];            /* as rocprofv3 prints it, e.g. "k_table_wave<4>" */
} ts_table_desc;
int32_t ts_describe_table_build(const ts_dims *dims, ts_table_desc *desc);

/* Process-wide launch-policy knobs of this library (speed only: both forms compute the same table and are under the same
 * tests).  value >= 0 sets, value < 0 only queries; returns the value before the call, -1 for an unknown key.
 *   TS_TABLE_TUNE_WAVE_MAX_STATES    index spaces up to this size take the wave form, larger ones the block form where one
 *       is compiled (boards 2x2 .. 8x8; a 1x1 board takes the wave form regardless).  Default 1024 (measured: DESIGN.md
 *       section 12).
 *   TS_TABLE_TUNE_BLOCK_BELOW_BOARDS batches of fewer boards than this take the block form whatever the index space, if
 *       it has at least 256 placements (one per thread of the block): one wave per board does not fill the GPU there.
 *       0 switches the rule off.  Default 32768 (measured: DESIGN.md section 12).
 *   TS_TABLE_TUNE_STATES_PER_LANE    placements a lane of the wave form visits per round: lanes per board =
 *       ceil(states / value) rounded up to a power of two, at most 64 (0 counts as 1).  Default 1. */
#define TS_TABLE_TUNE_WAVE_MAX_STATES 0
#define TS_TABLE_TUNE_STATES_PER_LANE 1
#define TS_TABLE_TUNE_BLOCK_BELOW_BOARDS 2
int64_t ts_table_tuning(int32_t key, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_TABLE_H */
