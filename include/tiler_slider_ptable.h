/*
 * tiler_slider_ptable.h — C-ABI of the policy tables (lib/libtiler_slider_ptable.so).
 *
 * A library of its own beside the twelve others: it shares the data layout, ts_dims, ts_state and ts_status of tiler_slider.h
 * (every pointer a DEVICE pointer owned by the caller, `stream` a hipStream_t as void*, every call asynchronous, no allocation,
 * no retained pointers), the index space and the codes of tiler_slider_table.h, the network ts_mlp and TS_POLICY_GREEDY of
 * tiler_slider_policy.h, and has an ABI version of its own.
 *
 * A level's placements are a finite space, idx = sum_t cell_t * (S*S)^t, states = (S*S)^T <= 65536 of them, and
 * ts_table_build holds the optimal distance to the win of every one.  A DETERMINISTIC policy on that space is a successor
 * function, so its outcome from every placement is exact - no sampling, no horizon, no start distribution: it wins in d moves,
 * or it never wins (greedy play runs into a cycle or a fixed point), or it does not win within the cut.  A POLICY TABLE is that
 * outcome in the distance table's own format, uint8 [L][states] with the same codes
 *
 *     TS_TABLE_INVALID (253)  a tile on an obstacle or two tiles on one cell
 *     TS_TABLE_DEEP    (254)  not resolved when the rounds were cut at max_depth
 *     TS_TABLE_NONE    (255)  the policy never wins from there
 *     0 .. TS_TABLE_MAX_DEPTH (252)  the moves the policy takes to the win
 *
 * so ts_table_lookup and ts_starts_place read it unchanged.  Three calls: the network's greedy action on every placement
 * (ts_ptable_actions), the walk of an action table (ts_ptable_walk), and a fixed-size integer score of a policy table against
 * the optimal one (ts_ptable_score).
 *
 * L = dims->n_boards is the number of levels; a level is board n's obstacles `blk` and targets `tgt`.  No call reads pos, init,
 * step_count or done (they may be NULL), and none writes any state.  A move and a won board are what ts_step and ts_is_won of
 * tiler_slider.h compute; cell ids >= S*S in tgt are clamped to S*S - 1 as the step kernels clamp them.
 *
 * SUPPORTED exactly where ts_table_states(dims) > 0 and ts_policy_supported(dims, hidden) both hold (ts_ptable_supported); the
 * walk and the score, which have no network, take hidden = 1.
 */
#ifndef TILER_SLIDER_PTABLE_H
#define TILER_SLIDER_PTABLE_H

#include "tiler_slider_policy.h"
#include "tiler_slider_table.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_PTABLE_ABI_VERSION 1
#define TS_PTABLE_NO_ACTION 255 /* act of an invalid placement */
#define TS_PTABLE_SCORE_COLUMNS 8

int32_t ts_ptable_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_ptable_last_hip_error(void);

/* 1 where ts_table_states(dims) > 0 and ts_policy_supported(dims, hidden) == 1, 0 otherwise, a negative ts_status for invalid
 * dims (TS_ERR_NULL, TS_ERR_DIMS).  Host only. */
int32_t ts_ptable_supported(const ts_dims *dims, int32_t hidden);

/* 1. THE ACTIONS.  act uint8 [L][states]; logits float32 [L][states][4], 16-byte aligned, or NULL.  For every valid placement i
 * of level n: z is exactly what ts_policy_logits gives on a board of that level standing on that placement - the same sequence
 * of float operations, so it is bit-equal - and act[n][i] is TS_POLICY_GREEDY's choice on z, the lowest action among the
 * largest logits (on the float32 values that are stored).  Won placements get their action too.  An invalid placement gets
 * act = TS_PTABLE_NO_ACTION and four 0.0f.  Reads blk and tgt only; writes every byte of both outputs exactly once.
 * Non-finite weights are the caller's business: whatever they are, no access leaves its buffer and act of a valid placement is <= 3.
 * One launch: k_ptable_actions<S>, one placement per lane.
 * Checked in this order, before any HIP call: dims (TS_ERR_NULL, TS_ERR_DIMS, TS_ERR_LIMIT beyond the step library's own
 * limits), mlp (TS_ERR_NULL), an unsupported shape or width (TS_ERR_LIMIT); then n_boards = 0 is TS_OK without a launch (no
 * further pointer is looked at); then a missing pointer (TS_ERR_NULL: st, act, a parameter of the network, blk, tgt where there
 * are targets); then a logits pointer that is not 16-byte aligned (TS_ERR_ARG). */
int32_t ts_ptable_actions(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, uint8_t *act, float *logits, void *stream);

/* 2. THE WALK.  act uint8 [L][states] may hold ANY bytes: a tabular policy need not come from a network.  With
 *     succ(i) = the placement after ts_step's move act[i] where act[i] <= 3, and i itself otherwise,
 * dist uint8 [L][states] is, per level:
 *     TS_TABLE_INVALID  where i is invalid (act[i] is not read)
 *     0                 where ts_is_won holds on i
 *     d = 1 .. 252      the least d >= 1 with succ^d(i) won
 *     TS_TABLE_NONE / TS_TABLE_DEEP   the stopping rule of ts_table_build, word for word: with R(d) the valid placements at
 *                       distance exactly d, the level stops at the first d with R(d) empty, and everything unresolved becomes
 *                       TS_TABLE_NONE; else it stops at d = max_depth with R(d) not empty, and everything unresolved becomes
 *                       TS_TABLE_DEEP (also placements that no number of further rounds would have resolved).
 * Writes every entry exactly once.  act must be complete before the call starts on `stream` (a kernel boundary: behind
 * ts_ptable_actions on the same stream it is).  The body is ts_table_build's round loop with one successor in place of four,
 * the frontier in LDS bitmaps; two forms, k_ptable_walk_wave<S> and k_ptable_walk_block<S>, chosen as ts_table_build chooses.
 * Checked in this order: dims, an unsupported shape (TS_ERR_LIMIT), max_depth < 0 or > TS_TABLE_MAX_DEPTH (TS_ERR_ARG); then
 * n_boards = 0 is TS_OK without a launch; then a missing pointer (TS_ERR_NULL: st, act, dist, blk, tgt where there are
 * targets); then act and dist sharing a byte (TS_ERR_ARG). */
int32_t ts_ptable_walk(const ts_dims *dims, const ts_state *st, const uint8_t *act, int32_t max_depth, uint8_t *dist, void *stream);

/* 3. THE SCORE.  score int32 [L][8].  All counts are over the placements i that the level itself makes valid (decided from blk,
 * not from the bytes of the tables).  With p = ptable[n][i] and o = table[n][i]:
 *     column 0  valid placements
 *     column 1  solvable:  1 <= o <= 252
 *     column 2  solved:    1 <= p <= 252
 *     column 3  optimal:   solved and p = o
 *     column 4  agree:     solvable, act[n][i] <= 3, and table[n][succ(i)] = o - 1: the policy's move is one of the expert's
 *     column 5  excess:    the sum of p - o over the placements that are both solved and solvable, signed
 *     column 6  p = TS_TABLE_DEEP
 *     column 7  p = 0
 * Integers only and no atomics - a group of lanes per level, reduced by shuffles: the same bits on every run.  Over tables
 * nobody built (any bytes) it still reads nothing outside its three rows.  One launch: k_ptable_score<S>.
 * Checked in this order: dims, an unsupported shape (TS_ERR_LIMIT); then n_boards = 0 is TS_OK without a launch; then a missing
 * pointer (TS_ERR_NULL: st, ptable, act, table, score, blk); then a score pointer that is not 4-byte aligned (TS_ERR_ARG). */
int32_t ts_ptable_score(const ts_dims *dims, const ts_state *st, const uint8_t *ptable, const uint8_t *act, const uint8_t *table,
                        int32_t *score, void *stream);

/* What a call would launch, computed by the code it runs before it launches; touches no device. */
#define TS_PTABLE_FORM_NONE 0  /* empty batch: nothing is launched (name is empty) */
#define TS_PTABLE_FORM_WAVE 1  /* one-wave blocks, a level worked by lanes_per_level = 1 .. 64 lanes */
#define TS_PTABLE_FORM_BLOCK 2 /* one level per block of four waves */
#define TS_PTABLE_FORM_FLAT 3  /* the actions: placements of all levels dealt over the lanes in order, one each */
typedef struct ts_ptable_desc {
  int32_t form;              /* TS_PTABLE_FORM_* */
  int32_t lanes_per_level;   /* threads that work on one level; FLAT: min(states, threads_per_block) */
  int32_t threads_per_block;
  int32_t lds_bytes;         /* dynamic LDS of a block, at most 64 KiB */
  int32_t weights_in_lds;    /* the actions: 1 where the tile-plane weights are staged in LDS, 0 where gathered through L2 */
  int32_t passes;            /* placements a lane visits (per round, in the walk) */
  int64_t states;            /* ts_table_states(dims) */
  int64_t blocks;            /* grid size; 0 where nothing is launched */
  char name[64];             /* as rocprofv3 prints it, e.g. "k_ptable_walk_wave<4>" */
} ts_ptable_desc;
int32_t ts_describe_ptable_actions(const ts_dims *dims, int32_t hidden, ts_ptable_desc *desc);
int32_t ts_describe_ptable_walk(const ts_dims *dims, ts_ptable_desc *desc);
int32_t ts_describe_ptable_score(const ts_dims *dims, ts_ptable_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_PTABLE_H */
