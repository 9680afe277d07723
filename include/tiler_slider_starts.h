/*
 * tiler_slider_starts.h — C-ABI of the curriculum starts (lib/libtiler_slider_starts.so).
 *
 * A twelfth library beside the step, search, table, rollout, policy, train, targets, actor-critic, in-place-step, loss and
 * optimiser libraries: it shares the data layout, ts_dims, ts_state and ts_status of tiler_slider.h (every pointer a DEVICE
 * pointer owned by the caller, `stream` a hipStream_t as void*, every call asynchronous, no allocation, no retained
 * pointers), the entry values and limits of tiler_slider_table.h, and has an ABI version of its own.
 *
 * A board starts where its level's `init` cells say, and most random levels cannot be won from there.  A distance table
 * (ts_table_build) holds, for every level, the exact distance to the win of EVERY placement of its tiles; ts_starts_place
 * reads each board's row once and puts the board on a uniformly drawn placement whose distance lies in a requested band of
 * moves: reverse curricula (one move from the win, then wider), per-board difficulty, fresh starts for finished boards.
 *
 * Supported shapes are exactly those of ts_table_states: S <= 8 and (S*S)^T <= 65536.
 */
#ifndef TILER_SLIDER_STARTS_H
#define TILER_SLIDER_STARTS_H

#include "tiler_slider_table.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_STARTS_ABI_VERSION 1
#define TS_STARTS_ALL 0        /* ts_starts_cfg.where: every board is selected */
#define TS_STARTS_DONE 1       /* boards with st->done[n] != 0 are selected */
#define TS_STARTS_PIECE_BYTES 16 /* what a lane reads of a row per pass */

int32_t ts_starts_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_starts_last_hip_error(void);
/* 1 where ts_table_states(dims) > 0, 0 where it is 0, a negative ts_status for invalid dims.  Host only. */
int32_t ts_starts_supported(const ts_dims *dims);

typedef struct ts_starts_cfg {
  int32_t lo, hi;          /* the band of distances, 0 .. TS_TABLE_MAX_DEPTH each; lo > hi is an empty band, not an error */
  const uint8_t *band;     /* optional uint8 [2][N]: row 0 = lo of board n, row 1 = hi; overrides lo / hi; any byte values */
  int32_t where;           /* TS_STARTS_ALL 0: every board is selected; TS_STARTS_DONE 1: boards with st->done[n] != 0 */
  int32_t write_pos;       /* 1: st->pos, st->step_count (= 0) and st->done (= 0) of a placed board are written */
  int32_t write_init;      /* 1: st->init of a placed board is written too (reset and auto-reset return there) */
  int32_t reserved;
  uint64_t seed;
  int64_t step_index;
  int64_t board_offset;
} ts_starts_cfg;

/* Each output is optional (NULL): count int32 [N], dist uint8 [N], deepest uint8 [N]. */
typedef struct ts_starts_out {
  int32_t *count;
  uint8_t *dist;
  uint8_t *deepest;
} ts_starts_out;

/* THE DEFINITION.  For board n, with row r = rows ? rows[n] : n of `table` (uint8 [n_rows][states], states =
 * ts_table_states(dims), C = S * S), e the bytes of that row, and the band (lo_n, hi_n) = band ? (band[n], band[N + n]) :
 * (lo, hi):
 *     match(i)    <=>  lo_n <= e[i] <= min(hi_n, 252).  TS_TABLE_INVALID, TS_TABLE_DEEP and TS_TABLE_NONE never match.
 *     count[n]    =    the number of matching i
 *     deepest[n]  =    the largest e[i] <= 252 of the row, 255 where the row has none
 * Both are properties of the row and are reported for every board, selected or not.  A row index outside 0 .. n_rows - 1
 * gives 0 and 255, and nothing outside the table is read.
 * A board is PLACED <=> it is selected by `where`, its row exists, and count[n] > 0.  For a placed board
 *     R    = the action stream's 64-bit draw at (seed, board_offset + n, step_index):
 *            mix64(mix64(seed ^ step_index * 0xd1b54a32d192ed03) + (board_offset + n) * 0x9e3779b97f4a7c15), mix64 the
 *            splitmix64 finaliser, everything modulo 2^64 - the draw whose top two bits are ts_fill_actions' action
 *     j    = ((R >> 32) * count[n]) >> 32
 *     idx  = the j-th matching index in ascending order (j = 0: the lowest)
 *     cell_t = (idx / C^t) % C  for t = 0 .. T - 1
 * and the cells are written to pos[t][n] where write_pos - together with step_count[n] = 0 and done[n] = 0 - and to
 * init[t][n] where write_init (ts_state declares init const for the libraries that only read it; this call writes through
 * it); dist[n] = e[idx].  A board that is not placed keeps every state byte and reports
 * dist[n] = 255.
 * THE CALLER'S CONTRACT, as for ts_table_lookup: the row was built for the board's level.  Over arbitrary bytes the call
 * still reads and writes nothing outside its buffers and still writes cells < C.  Everything is integer arithmetic: the
 * result is the same bits on every run.
 *
 * REFUSALS, in this order and before any HIP call:
 *   1. dims: TS_ERR_NULL, TS_ERR_DIMS or TS_ERR_LIMIT of the shared check
 *   2. cfg or out NULL: TS_ERR_NULL
 *   3. a shape where ts_table_states is 0 (or more blocks than a grid holds): TS_ERR_LIMIT
 *   4. lo or hi outside 0 .. 252, `where` outside {0, 1}, write_pos or write_init outside {0, 1}, n_rows < 0: TS_ERR_ARG
 *   5. n_boards = 0: TS_OK without a launch, no pointer is looked at
 *   6. TS_ERR_NULL for a missing pointer: st; table where n_rows > 0; pos, step_count and done where write_pos (pos only
 *      where n_tiles > 0); init where write_init and n_tiles > 0; done where TS_STARTS_DONE; and a call with no output and
 *      no write at all
 *   7. `band` overlapping anything that is written (pos, step_count, done, init, count, dist, deepest): TS_ERR_ARG
 * Then n_rows = 0 is TS_OK without a launch too, and NOTHING is written: no board has a row.
 * One launch, asynchronous on `stream`.  Reads table, rows, band and, with TS_STARTS_DONE, done. */
int32_t ts_starts_place(const ts_dims *dims, const ts_state *st, const uint8_t *table, int64_t n_rows, const int32_t *rows,
                        const ts_starts_cfg *cfg, const ts_starts_out *out, void *stream);

/* What ts_starts_place would launch for these dims, computed by the code it runs before it launches; touches no device.
 * k_starts_place<S>: blocks of ONE wave, cut into groups of lanes_per_board = 1 .. 64 lanes, a board per group.  A group's
 * lanes read consecutive ALIGNED 16-byte pieces of the row, one coalesced request per group and pass; a row that fits one
 * piece per lane stays in registers between counting and selecting, a longer one is walked twice and the second walk stops
 * at the piece that holds j.  lanes_per_board = ceil(states / 16) rounded up to a power of two, at most 64; passes =
 * ceil(ceil(states / 16) / lanes_per_board), for a row that starts on a 16-byte boundary (one that does not can span one
 * piece more, and where that is one more than the lanes, one pass more: the kernel counts the pieces of each row itself). */
#define TS_STARTS_FORM_NONE 0 /* empty batch: nothing is launched */
#define TS_STARTS_FORM_WAVE 1
typedef struct ts_starts_desc {
  int32_t form;              /* TS_STARTS_FORM_* */
  int32_t lanes_per_board;
  int32_t boards_per_block;
  int32_t threads_per_block; /* 64 */
  int32_t bytes_per_lane;    /* of a row, per lane and pass: TS_STARTS_PIECE_BYTES */
  int32_t passes;            /* walks of lanes_per_board pieces that cover an aligned row */
  int64_t states;            /* ts_table_states(dims) */
  int64_t blocks;            /* grid size */
  char name[64];             /* as rocprofv3 prints it, e.g. "k_starts_place<4>" */
} ts_starts_desc;
int32_t ts_describe_starts_place(const ts_dims *dims, ts_starts_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_STARTS_H */
