/*
 * tiler_slider_rtable.h — C-ABI of the reachable distance tables (lib/libtiler_slider_rtable.so).
 *
 * ts_table_build (tiler_slider_table.h) holds the distance to the win of EVERY placement of a level and stops at index spaces of
 * 65,536 placements.  ts_reach_solve (tiler_slider_reach.h) covers the shapes beyond that with a whole breadth-first search per
 * board and call.  This library solves such a level once: the distance of every placement that play can REACH from the level's
 * root, in a hash table in caller-owned memory (ts_rtable_build), read wherever the board stands by a probe per board and one per
 * successor (ts_rtable_lookup).  It shares the data layout, ts_dims, ts_state and ts_status of tiler_slider.h (every pointer a
 * DEVICE pointer owned by the caller, `stream` a hipStream_t as void*, every call asynchronous, no allocation, no retained
 * pointers), the entry codes of tiler_slider_table.h, TS_REACH_FULL and the limits of tiler_slider_reach.h, and has an ABI version
 * of its own.
 *
 * Definition.  Moves, win test, the clamping of cell ids (>= S*S reads as S*S - 1) and the ordered key
 * idx = sum_t cell_t * (S*S)^t  (below 2^48) are ts_reach_solve's; single-colour boards are NOT canonicalised.
 *   Root.  One placement per level: the cells of st->init (TS_RTABLE_ROOT_INIT: the table stays right through ts_reset and the
 *     auto-reset of ts_step) or of st->pos (TS_RTABLE_ROOT_POS).
 *   R.  The least set that holds the root if it is not won and, with every s in R, each of the four successors of s that is not
 *     won.  Won placements are never stored and never expanded: play ends there.  count = |R| (0 for a won root).  A level with
 *     |R| > capacity is FULL: its count is TS_REACH_FULL, its row holds nothing a lookup may use, and every lookup into it
 *     answers TS_REACH_FULL.
 *   Distance.  D(s) = 0 on a won placement, else 1 + the least D over the four successors of s, computed over R by rounds
 *     d = 1, 2, ...: round d resolves the unresolved states of R that have a successor at distance d - 1 (for d = 1: a won
 *     successor).  With R(d) the states of R at distance exactly d, d >= 1: the level stops at the first d <= max_depth with R(d)
 *     empty, and everything unresolved becomes TS_TABLE_NONE; otherwise it stops behind round max_depth, and everything
 *     unresolved becomes TS_TABLE_DEEP (with max_depth = 0 no round runs: every state of R is TS_TABLE_DEEP).
 *   An entry is 1 .. 252, TS_TABLE_DEEP or TS_TABLE_NONE; 0 and TS_TABLE_INVALID are never stored.
 *
 * The table.  uint64 [n_levels, slots], row-major, slots = ts_rtable_slots(capacity) = pow2ceil(2 * capacity), at least 2.  A
 * slot is 0 (empty) or
 *     bit 63 set | bits 56 .. 62 zero | bits 48 .. 55 the entry | bits 0 .. 47 the key.
 * A state lies in the first free slot of its probe sequence: linear probing, slot + 1 modulo slots, from
 *     home(key) = (uint32)((key * 0x9e3779b97f4a7c15) >> 32) >> (32 - log2(slots)).
 * Which of two states takes a contested slot depends on how the lanes race: the BITS of a row are not reproducible from run to
 * run, its SET of (key, entry) pairs is, and so is everything a lookup answers.  count, root_moves and deepest are sizes and
 * extrema of sets: the same bits on every run.
 */
#ifndef TILER_SLIDER_RTABLE_H
#define TILER_SLIDER_RTABLE_H

#include "tiler_slider_reach.h"
#include "tiler_slider_table.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_RTABLE_ABI_VERSION 1
#define TS_RTABLE_ROOT_INIT 0 /* the level's initial cells st->init */
#define TS_RTABLE_ROOT_POS 1  /* the cells as they stand, st->pos */
#define TS_RTABLE_ABSENT (-4) /* ts_rtable_lookup: the row does not hold the board's placement - play from the root never gets there */

int32_t ts_rtable_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_rtable_last_hip_error(void);

/* 1 if these dims are taken (those of ts_reach_supported: S <= 8, n_tiles <= 8, any valid n_targets), 0 if not, a negative
 * ts_status for invalid dims.  Host only. */
int32_t ts_rtable_supported(const ts_dims *dims);

/* 64-bit slots of one level's row: pow2ceil(2 * capacity), 2 .. 2^31.  TS_ERR_ARG for a capacity outside
 * 1 .. TS_REACH_MAX_CAPACITY.  Host only. */
int64_t ts_rtable_slots(int32_t capacity);

typedef struct ts_rtable_cfg {
  int32_t max_depth;       /* 0 .. TS_TABLE_MAX_DEPTH */
  int32_t capacity;        /* 1 .. TS_REACH_MAX_CAPACITY: states a level may hold before it is FULL */
  int32_t root;            /* TS_RTABLE_ROOT_INIT or TS_RTABLE_ROOT_POS */
  void *workspace;         /* device memory, 8-byte aligned, any contents: every word is written before it is read */
  int64_t workspace_bytes; /* at least ts_rtable_workspace_bytes(dims, capacity, 1) */
} ts_rtable_cfg;

typedef struct ts_rtable_out {
  uint64_t *table;     /* [N, slots], required; any contents: every slot of every row is written */
  int32_t *count;      /* [N], required: |R|, or TS_REACH_FULL.  ts_rtable_lookup reads it */
  int16_t *root_moves; /* [N], may be NULL: 0 for a won root, TS_REACH_FULL for a FULL level, else the root's entry as
                          ts_table_lookup maps entries (1 .. 252, TS_SOLVE_NONE, TS_SOLVE_DEPTH) */
  int32_t *deepest;    /* [N], may be NULL: the largest entry 1 .. 252 of the row; 0 if there is none or the level is FULL */
} ts_rtable_out;

/* Bytes of workspace that let `levels_in_flight` levels be built at once (one block each): levels_in_flight times the
 * workspace_bytes of ts_describe_rtable_build.  A call with fewer levels in flight than n_boards builds the rest through the same
 * slices, one after another.  A negative ts_status for invalid dims, TS_ERR_LIMIT for an unsupported shape, TS_ERR_ARG for a
 * capacity outside 1 .. TS_REACH_MAX_CAPACITY or levels_in_flight < 1.  Host only. */
int64_t ts_rtable_workspace_bytes(const ts_dims *dims, int32_t capacity, int64_t levels_in_flight);

/* The table defined above, one row per board of the batch.  Reads blk, tgt and the root cells only and writes no state.
 * Refusals, in this order and before any HIP call: dims NULL (TS_ERR_NULL) or invalid (TS_ERR_DIMS); a shape ts_rtable_supported
 * refuses (TS_ERR_LIMIT); cfg NULL (TS_ERR_NULL); cfg->max_depth, cfg->capacity or cfg->root out of range, or a workspace too
 * small for ONE level (TS_ERR_ARG); a missing pointer - out, st, out->table, out->count, cfg->workspace, st->blk, the root cells
 * with tiles, st->tgt with targets (TS_ERR_NULL).  n_boards = 0 is TS_OK without a launch once max_depth, capacity and root have
 * passed. */
int32_t ts_rtable_build(const ts_dims *dims, const ts_state *st, const ts_rtable_cfg *cfg, const ts_rtable_out *out, void *stream);

/* For every board, from its CURRENT cells st->pos, read from row rows[n] (rows NULL: row n) of `table` (uint64 [n_rows, slots])
 * and `count` (int32 [n_rows]).  One board per lane, no LDS, at most `slots` steps per probe.  Each output is optional (NULL), at
 * least one is required.  In this order:
 *     a row index outside 0 .. n_rows - 1     TS_SOLVE_NONE, 0, 255 (ts_table_lookup's rule; nothing of table or count is read)
 *     a won board                             0, 0, 255
 *     a FULL row (count == TS_REACH_FULL)     TS_REACH_FULL, 0, 255
 *     a placement the row does not hold       TS_RTABLE_ABSENT, 0, 255
 *     else                                    the entry as ts_table_lookup maps it: 1 .. 252 as it is, TS_TABLE_NONE (and
 *                                             TS_TABLE_INVALID, 0: never stored by a build) -> TS_SOLVE_NONE, TS_TABLE_DEEP ->
 *                                             TS_SOLVE_DEPTH
 *   best[n]    uint8: bit a set <=> moves[n] >= 1 and the board after Move a is moves[n] - 1 from the win: it is won (and
 *              moves[n] is 1), or the row holds it with that entry
 *   action[n]  uint8: the lowest set bit of best[n], 255 if there is none
 * THE CALLER'S CONTRACT is ts_table_lookup's: the row was built for the board's level.  Whatever bytes a row holds, a lookup
 * ends after at most 5 * slots reads and reads nothing outside that row.
 * Reads pos, blk and tgt only, writes no state.  Refusals, in this order: dims NULL (TS_ERR_NULL) or invalid (TS_ERR_DIMS); an
 * unsupported shape (TS_ERR_LIMIT); n_rows < 0, or slots no power of two in 2 .. 2^31 (TS_ERR_ARG); a missing pointer - st,
 * st->blk, st->pos with tiles, st->tgt with targets, table or count with n_rows > 0, no output at all (TS_ERR_NULL).
 * n_boards = 0 is TS_OK without a launch once n_rows and slots have passed; asynchronous on `stream`. */
int32_t ts_rtable_lookup(const ts_dims *dims, const ts_state *st, const uint64_t *table, int64_t slots, const int32_t *count,
                         int64_t n_rows, const int32_t *rows, int16_t *moves, uint8_t *best, uint8_t *action, void *stream);

/* What ts_rtable_build would launch, computed by the code it runs before it launches; touches no device (cfg->workspace is not
 * looked at).  One launch of k_rtable_build<S> for any N: levels_in_flight = min(n_boards, cfg->workspace_bytes /
 * workspace_bytes, 1024) blocks of four waves; block b builds levels b, b + blocks, ... through slice b of the workspace. */
typedef struct ts_rtable_desc {
  int32_t threads_per_block;
  int32_t reserved;
  int64_t blocks;           /* grid size = levels_in_flight; 0 for an empty batch */
  int64_t levels_in_flight;
  int64_t slots;            /* ts_rtable_slots(capacity) */
  int64_t table_bytes;      /* of one level's row: 8 * slots */
  int64_t workspace_bytes;  /* of one level's slice: the log of claimed slots (uint32 per state, rounded up to 8 bytes) and the
                               four successor slots of every state (uint32 x 4) */
  char name[64];            /* as rocprofv3 prints it, e.g. "k_rtable_build<5>"; "" for an empty batch */
} ts_rtable_desc;
int32_t ts_describe_rtable_build(const ts_dims *dims, const ts_rtable_cfg *cfg, ts_rtable_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_RTABLE_H */
