/*
 * tiler_slider_rstarts.h — C-ABI of the reach-table curricula (lib/libtiler_slider_rstarts.so).
 *
 * ts_starts_place (tiler_slider_starts.h) puts boards a chosen distance from the win by reading a dense distance table, so it
 * stops at index spaces of 65,536 placements.  This library does the same from a reachable distance table
 * (tiler_slider_rtable.h).  A hash row cannot be scanned per board - it is pow2ceil(2 * capacity) 64-bit slots, and which slot a
 * state lies in differs from build to build -, so each level's states are sorted ONCE into a band index (ts_rstarts_index), and
 * boards are placed from the index with a handful of reads each (ts_rstarts_place).  It shares the data layout, ts_dims,
 * ts_state and ts_status of tiler_slider.h (every pointer a DEVICE pointer owned by the caller, `stream` a hipStream_t as void*,
 * every call asynchronous, no allocation, no retained pointers), the slot format of tiler_slider_rtable.h, the structs
 * ts_starts_cfg and ts_starts_out, TS_STARTS_ALL and TS_STARTS_DONE of tiler_slider_starts.h, and has an ABI version of its own.
 *
 * Supported shapes are exactly those of ts_rtable_supported: S <= 8, n_tiles <= 8, any valid n_targets.
 */
#ifndef TILER_SLIDER_RSTARTS_H
#define TILER_SLIDER_RSTARTS_H

#include "tiler_slider_rtable.h"
#include "tiler_slider_starts.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_RSTARTS_ABI_VERSION 1
#define TS_RSTARTS_FIRST 256      /* int32 words of one level's `first` row */
#define TS_RSTARTS_FORM_NONE 0    /* no level: nothing is launched */
#define TS_RSTARTS_FORM_LDS 1     /* every level of the width is sorted in LDS */
#define TS_RSTARTS_FORM_GLOBAL 2  /* levels above lds_states are sorted in their own `sorted` row */

int32_t ts_rstarts_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_rstarts_last_hip_error(void);
/* What ts_rtable_supported(dims) answers: 1, 0, or a negative ts_status for invalid dims.  Host only. */
int32_t ts_rstarts_supported(const ts_dims *dims);

/* THE BAND INDEX.  For every level l of `table` (uint64 [n_levels][slots]) and `count` (int32 [n_levels]), as ts_rtable_build
 * wrote them, and a width W (the table's capacity):
 *     sorted[l]  uint64 [W]: the occupied slot words of row l (bit 63 set) in ascending unsigned order, then zeros.  By the slot
 *                format (bit 63 | the entry in bits 48 .. 55 | the key in bits 0 .. 47) that is ascending (entry, key):
 *                distances 1 .. 252 first, each bucket in key order, then TS_TABLE_DEEP, then TS_TABLE_NONE.
 *     first[l]   int32 [256]: first[d] = the number of kept words w with (w & ~bit63) < ((uint64)d << 48) - a lower bound in the
 *                sorted row.  first[0] = first[1] = 0; first[253] is the number of states with a finite distance.
 * A level with count < 0 (FULL) or count > W has an EMPTY index: first all zero, sorted all zero.
 * Both outputs are caller-owned and every word of them is written: neither needs zeroing first.
 * The result is a function of the row's SET of (key, entry) pairs only: two builds of the same table differ in the bits of a row
 * (which slot a state took) and give the same bits here.
 * Over a row of arbitrary bytes (and any count) the call ends, reads nothing outside the row and count[l], writes nothing outside
 * its two output rows, and keeps at most W words (at most lds_states where count[l] <= lds_states); which words it keeps is
 * unspecified there, the kept words are sorted and `first` is their lower bounds all the same.
 *
 * REFUSALS, in this order and before any HIP call:
 *   1. n_levels < 0, slots no power of two in 2 .. 2^31, W outside 1 .. TS_REACH_MAX_CAPACITY: TS_ERR_ARG
 *   2. n_levels = 0: TS_OK without a launch, no pointer is looked at
 *   3. table, count, sorted or first NULL: TS_ERR_NULL
 *   4. `sorted` or `first` overlapping `table` or `count`, or each other: TS_ERR_ARG
 * One launch, asynchronous on `stream`: k_rstarts_index<GLOBAL>, min(n_levels, 1024) blocks of four waves; block b indexes levels
 * b, b + blocks, ...  Integer arithmetic only. */
int32_t ts_rstarts_index(const uint64_t *table, int64_t slots, const int32_t *count, int64_t n_levels, int64_t W, uint64_t *sorted,
                         int32_t *first, void *stream);

/* THE PLACEMENT: ts_starts_place with the index in place of the dense row.  For board n, with row r = rows ? rows[n] : n of
 * `sorted` (uint64 [n_rows][W]) and `first` (int32 [n_rows][256]), the band (lo_n, hi_n) = band ? (band[n], band[N + n]) :
 * (lo, hi), C = S * S, and clamp(x) = min(max(x, 0), W):
 *     a = clamp(first[r][lo_n]),  b = clamp(first[r][min(hi_n, 252) + 1])
 *     count[n]    =  max(b - a, 0): the states of the level whose entry lies in lo_n .. min(hi_n, 252).  UNLIKE the dense call,
 *                    distance 0 never matches: won placements are not stored in a reach table (first[0] = first[1])
 *     deepest[n]  =  the entry of sorted[r][clamp(first[r][253]) - 1], or 255 where clamp(first[r][253]) is 0; read only when
 *                    the output is asked for
 * Both are properties of the row and are reported for every board, selected or not.  A row index outside 0 .. n_rows - 1 gives
 * 0 and 255, and nothing of the index is read.
 * A board is PLACED <=> it is selected by `where`, its row exists, and count[n] > 0.  For a placed board, with R the draw of
 * tiler_slider_starts.h at (seed, board_offset + n, step_index):
 *     j      = ((R >> 32) * count[n]) >> 32
 *     w      = sorted[r][a + j]
 *     cell_t = ((w & (2^48 - 1)) / C^t) % C  for t = 0 .. T - 1: always below C
 *     dist[n] = bits 48 .. 55 of w
 * and the writes are ts_starts_place's: pos[t][n] where write_pos - together with step_count[n] = 0 and done[n] = 0 -, init[t][n]
 * where write_init.  A board that is not placed keeps every state byte and reports dist[n] = 255.
 * THE CALLER'S CONTRACT: the index was built by ts_rstarts_index, at this W, from a table of the board's levels.  Over an index
 * nobody built - `first` values above W, negative or decreasing, arbitrary words - the call still reads and writes nothing
 * outside its buffers (every position read is below W) and still writes cells below C.  Everything is integer arithmetic: the
 * same bits on every run.
 *
 * REFUSALS, in this order and before any HIP call:
 *   1. dims: TS_ERR_NULL, TS_ERR_DIMS or TS_ERR_LIMIT of the shared check
 *   2. cfg or out NULL: TS_ERR_NULL
 *   3. a shape ts_rstarts_supported refuses (or more blocks than a grid holds): TS_ERR_LIMIT
 *   4. lo or hi outside 0 .. 252, `where` outside {0, 1}, write_pos or write_init outside {0, 1}, n_rows < 0, W outside
 *      1 .. TS_REACH_MAX_CAPACITY: TS_ERR_ARG
 *   5. n_boards = 0: TS_OK without a launch, no pointer is looked at
 *   6. TS_ERR_NULL for a missing pointer: st; sorted and first where n_rows > 0; pos, step_count and done where write_pos (pos
 *      only where n_tiles > 0); init where write_init and n_tiles > 0; done where TS_STARTS_DONE; and a call with no output and
 *      no write at all
 *   7. `band` overlapping anything that is written (pos, step_count, done, init, count, dist, deepest): TS_ERR_ARG
 * Then n_rows = 0 is TS_OK without a launch too, and NOTHING is written: no board has a row.
 * One launch, asynchronous on `stream`: k_rstarts_place<S>, one board per lane, blocks of four waves; no LDS, no atomics, no
 * barrier.  Reads sorted, first, rows, band and, with TS_STARTS_DONE, done. */
int32_t ts_rstarts_place(const ts_dims *dims, const ts_state *st, const uint64_t *sorted, const int32_t *first, int64_t W,
                         int64_t n_rows, const int32_t *rows, const ts_starts_cfg *cfg, const ts_starts_out *out, void *stream);

/* What a call would launch, computed by the code it runs before it launches; touches no device. */
typedef struct ts_rstarts_desc {
  int32_t form;              /* index: TS_RSTARTS_FORM_*; place: 0 */
  int32_t threads_per_block; /* 256 */
  int32_t lds_bytes;         /* of a block: index 8 * lds_states + 16, place 0 */
  int32_t lds_states;        /* index: a level of at most so many states is sorted in LDS (the threshold); place 0 */
  int64_t blocks;            /* grid size; 0 where nothing is launched (name is empty) */
  int64_t bytes;             /* index: what one level's outputs take, 8 * W + 1024; place: 0 */
  char name[64];             /* as rocprofv3 prints it: "k_rstarts_index<false>", "k_rstarts_index<true>", "k_rstarts_place<5>" */
} ts_rstarts_desc;
/* desc NULL: TS_ERR_NULL; then refusal 1 of ts_rstarts_index.  W <= lds_states takes TS_RSTARTS_FORM_LDS (k_rstarts_index<false>),
 * a larger one TS_RSTARTS_FORM_GLOBAL (k_rstarts_index<true>: each level takes the LDS sort or the sort in its row by its count). */
int32_t ts_describe_rstarts_index(int64_t n_levels, int64_t slots, int64_t W, ts_rstarts_desc *desc);
/* dims or desc NULL: TS_ERR_NULL; then refusals 1 and 3 of ts_rstarts_place. */
int32_t ts_describe_rstarts_place(const ts_dims *dims, ts_rstarts_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_RSTARTS_H */
