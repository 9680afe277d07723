/*
 * tiler_slider_reach.h — C-ABI of the hashed breadth-first solver (lib/libtiler_slider_reach.so).
 *
 * ts_solve (tiler_slider_search.h) keeps bitmaps over the whole index space (S*S)^T in LDS and stops at 65,536 placements.
 * This library searches the same moves with a hash set in global memory: it costs memory by what a board REACHES, not by its
 * index space, and covers every board of S <= 8 with up to 8 tiles.  It shares the data layout, ts_dims, ts_state and ts_status
 * of tiler_slider.h (every pointer a DEVICE pointer owned by the caller, `stream` a hipStream_t as void*, every call
 * asynchronous, no allocation, no retained pointers) and has an ABI version of its own.
 *
 * Definition.  Moves, win test and the clamping of cell ids (>= S*S reads as S*S - 1) are ts_solve's; a state is the ordered
 * index  idx = sum_t cell_t * (S*S)^t  (below 2^48).  Single-colour boards are NOT canonicalised: two orders of the same cells
 * are two states, so that `states` below has one meaning.
 *   F(0) = the board as it stands.  F(d) = the set of non-won states first reached after d moves.  V(d) = |F(0) u .. u F(d)|.
 * A won board gives moves = 0.  Otherwise, for d = 1, 2, ...: every state of F(d-1) is expanded by all four moves - the depth
 * always runs to its end - and then, in this order:
 *   1. a successor was won              moves = d
 *   2. V(d) > capacity                  moves = TS_REACH_FULL
 *   3. F(d) is empty                    moves = TS_SOLVE_NONE
 *   4. d == max_depth                   moves = TS_SOLVE_DEPTH
 * With max_depth = 0 a board that is not won gives TS_SOLVE_DEPTH.
 *   moves[n]   int16, as above.
 *   best[n]    uint8 (optional): exactly ts_solve's meaning - bit a set <=> moves[n] >= 1 and the board after Move a is
 *              moves[n] - 1 moves from won: every first move of every shortest solution.  0 unless moves[n] >= 1.
 *   states[n]  int32 (optional): the number of states EXPANDED, V(D - 1) with D the depth at which the search stopped; 0 for a
 *              won board and for max_depth = 0.
 * All three are sizes of sets: the same bits on every run, however the lanes race.  TS_REACH_FULL follows from the count V(d)
 * alone: the table of a board has more slots than `capacity`, so it can run out only once the count is above `capacity`.
 */
#ifndef TILER_SLIDER_REACH_H
#define TILER_SLIDER_REACH_H

#include "tiler_slider_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_REACH_ABI_VERSION 1
#define TS_REACH_MAX_SIZE 8
#define TS_REACH_MAX_TILES 8
#define TS_REACH_MAX_DEPTH 32767
/* the log of claimed slots holds uint32 slot numbers and a board has pow2ceil(2 * capacity) slots: 2^31 at most */
#define TS_REACH_MAX_CAPACITY 1073741824

#define TS_REACH_FULL (-3) /* more than `capacity` states were reached before the search ended: budget exhausted */

int32_t ts_reach_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_reach_last_hip_error(void);

/* 1 if ts_reach_solve takes these dims (S <= 8, n_tiles <= 8, any valid n_targets), 0 if not, a negative ts_status for invalid
 * dims (NULL, negative counts, more tiles than cells, a size or a count above TS_MAX_*).  Host only. */
int32_t ts_reach_supported(const ts_dims *dims);

typedef struct ts_reach_cfg {
  int32_t max_depth;       /* 0 .. TS_REACH_MAX_DEPTH */
  int32_t capacity;        /* 1 .. TS_REACH_MAX_CAPACITY: states a board may reach before TS_REACH_FULL */
  void *workspace;         /* device memory, 8-byte aligned, any contents: the kernel clears what it uses */
  int64_t workspace_bytes; /* at least ts_reach_workspace_bytes(dims, capacity, 1) */
} ts_reach_cfg;

typedef struct ts_reach_out {
  int16_t *moves;  /* [N], required */
  uint8_t *best;   /* [N], may be NULL */
  int32_t *states; /* [N], may be NULL */
} ts_reach_out;

/* Bytes of workspace that let `boards_in_flight` boards be searched at once (one block each): boards_in_flight times the
 * bytes_per_board of ts_describe_reach.  A call with fewer boards in flight than n_boards plays the rest through the same
 * slices, one after another.  A negative ts_status for invalid dims, TS_ERR_LIMIT for an unsupported shape, TS_ERR_ARG for a
 * capacity outside 1 .. TS_REACH_MAX_CAPACITY or boards_in_flight < 1.  Host only. */
int64_t ts_reach_workspace_bytes(const ts_dims *dims, int32_t capacity, int64_t boards_in_flight);

/* The search defined above, for every board from its CURRENT cells st->pos.  Reads pos, tgt, blk only and writes no state.
 * Refusals, in this order and before any HIP call: dims NULL (TS_ERR_NULL) or invalid (TS_ERR_DIMS); a shape
 * ts_reach_supported refuses (TS_ERR_LIMIT); cfg->max_depth or cfg->capacity out of range, or a workspace too small for ONE
 * board (TS_ERR_ARG); a missing pointer - cfg, out, st, out->moves, cfg->workspace, st->blk, st->pos with tiles, st->tgt with
 * targets (TS_ERR_NULL).  n_boards = 0 is TS_OK without a launch once max_depth and capacity have passed. */
int32_t ts_reach_solve(const ts_dims *dims, const ts_state *st, const ts_reach_cfg *cfg, const ts_reach_out *out, void *stream);

/* What ts_reach_solve would launch, computed by the code it runs before it launches; touches no device (cfg->workspace is not
 * looked at).  One launch of k_reach<S> for any N: boards_in_flight = min(n_boards, workspace_bytes / bytes_per_board, 1024)
 * blocks of four waves; block b plays boards b, b + blocks, ... through slice b of the workspace. */
typedef struct ts_reach_desc {
  int32_t threads_per_block;
  int32_t reserved;
  int64_t blocks;           /* grid size = boards_in_flight; 0 for an empty batch */
  int64_t boards_in_flight;
  int64_t slots_per_board;  /* 64-bit entries of a board's hash set: pow2ceil(2 * capacity) */
  int64_t table_bytes;      /* 8 * slots_per_board */
  int64_t frontier_bytes;   /* 8 * capacity: the compacted frontier, key and first-move bits of every state to expand */
  int64_t log_bytes;        /* 4 * capacity: the slot of every state in the order it was claimed; its tail is the next frontier */
  int64_t bytes_per_board;  /* table_bytes + frontier_bytes + log_bytes */
  char name[64];            /* as rocprofv3 prints it, e.g. "k_reach<5>"; "" for an empty batch */
} ts_reach_desc;
int32_t ts_describe_reach(const ts_dims *dims, const ts_reach_cfg *cfg, ts_reach_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_REACH_H */
