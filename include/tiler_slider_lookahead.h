/*
 * tiler_slider_lookahead.h — C-ABI of the lookahead: a network's values backed up through exact search
 * (lib/libtiler_slider_lookahead.so).
 *
 * A nineteenth library: it shares the data layout, ts_dims, ts_state and ts_status of tiler_slider.h (every pointer a DEVICE
 * pointer owned by the caller, `stream` a hipStream_t as void*, every call asynchronous, no allocation, no retained pointers),
 * the network ts_mlp and the limits of tiler_slider_policy.h, the samples ts_train_in of tiler_slider_train.h, the value head
 * ts_value_head of tiler_slider_ac.h - all included, none redefined - and has an ABI version of its own.
 *
 * The environment is deterministic and a transition is a few dozen integer instructions on cells in a lane's registers, so a
 * full-width search of depth d is 4 + ... + 4^d slides and 4^d evaluations of the network's tile-dependent part: the part of the
 * first layer the tiles cannot change is folded once per board, as in every other kernel that plays this network.
 *
 * THE SAMPLES are tiler_slider_train.h's, word for word: a call works on steps * n_boards samples.  Sample (k, n) is board n's
 * level - blk and tgt of ts_state - with the T tile cells c[k][t][n], where c[0] is `first` (cell_t [T][N]) and c[k] is
 * pos_log[k - 1] for k >= 1.  pos_log is exactly the [K][T][N] log a rollout writes, so its last row is never read; it may be NULL
 * when steps == 1.  Cell ids >= S*S are clamped as everywhere else.  st->pos, init, step_count and done are never read, and no
 * state is written.
 *
 * PER NODE, for tile cells c and an action a in 0 .. 3 (UP, DOWN, LEFT, RIGHT):
 *
 *     c'     = the slide of ts_step                      moved = (c' != c)
 *     won'   = the win test of ts_step on c'
 *     r(c,a) = w_step + w_win [won'] + w_invalid [!moved]
 *
 * THE BACKUP, with depth d = cfg->depth in 1 .. TS_LOOKAHEAD_MAX_DEPTH:
 *
 *     Q_1(c,a) = r(c,a) + gamma (won' ? 0 : L(c'))
 *     Q_d(c,a) = r(c,a) + gamma (won' ? 0 : max_a' Q_{d-1}(c',a'))          d >= 2
 *     L(c')    = 0                  TS_LOOKAHEAD_LEAF_ZERO    no network is read: mlp and head may be NULL
 *              = v(c')              TS_LOOKAHEAD_LEAF_VALUE   tiler_slider_ac.h's value head on ts_mlp's hidden layer
 *              = max_a z_a(c')      TS_LOOKAHEAD_LEAF_QMAX    ts_mlp's logits read as Q-values; head is not read and may be NULL
 *
 * THE OUTPUTS, each of which may be NULL but not all four:
 *
 *     q      float32 [K][N][4]   Q_d(c[k][n], a), one 16-byte store per sample
 *     value  float32 [K][N]      max_a q
 *     best   uint8   [K][N]      the lowest action among the largest q
 *     win_in uint8   [K][N]      the least number of plies <= d after which some action sequence has won, 0 if none has
 *
 * A sample whose board is ALREADY WON gets q = 0, 0, 0, 0, value = 0, best = TS_LOOKAHEAD_NO_ACTION (255: the byte ts_step
 * leaves a board alone for, and the label a cross-entropy over trajectory labels reads as "no sample") and win_in = 0.
 *
 * STATED PLAINLY.  An invalid move is a child like any other: c' = c, and it costs a ply.  There is no transposition table and
 * no pruning: every one of the 4^d action sequences is walked.  TIMEOUT is not modelled - the search does not know step_count.
 * The Manhattan terms w_dist / w_progress of ts_traj_returns are NOT BUILT here.  Arithmetic is float32; the order of operations
 * inside r and the use of fused multiply-adds are free, and z and v are tiler_slider_policy.h's and tiler_slider_ac.h's with the
 * freedoms those headers state.  `value` and `best` are functions of the q the kernel stores, bit for bit.  win_in is integer and
 * exact.  There are no atomics: a call gives the same bits on every run.  Non-finite inputs are the caller's business: whatever
 * they are, no read or write leaves its buffer.
 *
 * Supported shapes and widths: with a network leaf exactly those of tiler_slider_policy.h; with TS_LOOKAHEAD_LEAF_ZERO the same
 * shapes, the width ignored.  Every supported shape is searched to every depth 1 .. TS_LOOKAHEAD_MAX_DEPTH.
 */
#ifndef TILER_SLIDER_LOOKAHEAD_H
#define TILER_SLIDER_LOOKAHEAD_H

#include "tiler_slider_ac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_LOOKAHEAD_ABI_VERSION 1

#define TS_LOOKAHEAD_MAX_DEPTH 4
#define TS_LOOKAHEAD_NO_ACTION 255

#define TS_LOOKAHEAD_LEAF_ZERO 0
#define TS_LOOKAHEAD_LEAF_VALUE 1
#define TS_LOOKAHEAD_LEAF_QMAX 2

typedef struct ts_lookahead_cfg {
  int32_t depth;   /* 1 .. TS_LOOKAHEAD_MAX_DEPTH */
  int32_t leaf;    /* TS_LOOKAHEAD_LEAF_* */
  float gamma;     /* 0 .. 1 */
  float w_step;    /* every transition */
  float w_win;     /* a transition into a won board */
  float w_invalid; /* a transition that moves no tile */
  int32_t reserved[2];
} ts_lookahead_cfg;

typedef struct ts_lookahead_out {
  float *q;        /* [K][N][4], 16-byte aligned, or NULL */
  float *value;    /* [K][N], or NULL */
  uint8_t *best;   /* [K][N], or NULL */
  uint8_t *win_in; /* [K][N], or NULL */
} ts_lookahead_out;

int32_t ts_lookahead_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_lookahead_last_hip_error(void);

/* 1 / 0, or a negative status for invalid dims (TS_ERR_NULL, TS_ERR_DIMS) or an unknown leaf (TS_ERR_ARG, after the dims).  For
 * the two network leaves exactly ts_policy_supported(dims, hidden); for TS_LOOKAHEAD_LEAF_ZERO `hidden` is ignored.  Host only. */
int32_t ts_lookahead_supported(const ts_dims *dims, int32_t hidden, int32_t leaf);

/* Checks, in this order and before any HIP call: dims (the check every library shares: TS_ERR_NULL, TS_ERR_DIMS, and
 * TS_ERR_LIMIT for a size above 32 or more than 255 tiles or targets - BEFORE the NULL checks); in, cfg and out, and mlp where
 * cfg->leaf is a network leaf, for its width (TS_ERR_NULL); an unsupported shape or width (TS_ERR_LIMIT; an unknown leaf is
 * judged by the shape alone); then TS_ERR_ARG for steps outside 1 .. TS_ROLLOUT_MAX_STEPS, depth outside
 * 1 .. TS_LOOKAHEAD_MAX_DEPTH, an unknown leaf, gamma outside [0, 1] or NaN; then n_boards = 0 is TS_OK without a launch; then a
 * missing pointer (TS_ERR_NULL: st, blk, tgt where there are targets, first where there are tiles, pos_log where there are tiles
 * and steps > 1, a parameter of the network with a network leaf, head or one of its two parameters with TS_LOOKAHEAD_LEAF_VALUE,
 * all four outputs); then a q pointer that is not 16-byte aligned or a value pointer that is not 4-byte aligned (TS_ERR_ARG).
 *
 * One launch, k_lookahead<S, D>, one sample per lane and step: between the load of a sample's cells and the store of its outputs
 * nothing goes to memory.  Every lane of a wave walks the same 4^D action sequences in the same order; the leaf kind is a
 * uniform branch of the kernel, not a template parameter. */
int32_t ts_lookahead(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_value_head *head, const ts_train_in *in,
                     const ts_lookahead_cfg *cfg, const ts_lookahead_out *out, void *stream);

/* What a call would launch, computed by the code it runs before it launches; touches no device. */
typedef struct ts_lookahead_desc {
  int32_t threads_per_block;
  int32_t lds_bytes;        /* dynamic LDS of a block, all of it; 0 with TS_LOOKAHEAD_LEAF_ZERO */
  int32_t weights_in_lds;   /* 1: the tile-plane weights are staged in LDS; 0: gathered from global memory (or none are read) */
  int32_t leaf_is_template; /* 0: the leaf kind is a uniform branch of k_lookahead<S, D> */
  int32_t depth;
  int32_t reserved;
  int64_t blocks;           /* grid size; 0 where nothing is launched (name is empty) */
  int64_t samples;          /* steps * n_boards */
  int64_t leaves;           /* samples * 4^depth: the leaf evaluations of the call */
  char name[64];            /* as rocprofv3 prints it, e.g. "k_lookahead<4, 2>" */
} ts_lookahead_desc;
int32_t ts_describe_lookahead(const ts_dims *dims, int32_t hidden, int32_t steps, int32_t depth, int32_t leaf, ts_lookahead_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_LOOKAHEAD_H */
