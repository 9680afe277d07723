/*
 * tiler_slider_policy.h — C-ABI of the neural-policy rollouts (lib/libtiler_slider_policy.so).
 *
 * A fifth library beside libtiler_slider_hip.so, libtiler_slider_search.so, libtiler_slider_table.so and
 * libtiler_slider_rollout.so: it shares the data layout, ts_dims, ts_state, ts_status and the flag / mode bits of tiler_slider.h
 * (every pointer a DEVICE pointer owned by the caller, `stream` a hipStream_t as void*, every call asynchronous, no allocation,
 * no retained pointers), the output fields and limits of tiler_slider_rollout.h, and has an ABI version of its own.
 *
 * THE NETWORK (ts_mlp): one hidden layer with ReLU, float32, shared by all boards.  Its input x is exactly what ts_encode_onehot
 * writes for the board as it stands, flattened plane-major: feature f = plane * S*S + cell, D = ts_onehot_channels(dims) * S*S
 * (plane 0 the obstacles; multi colour: plane 1 + t tile t, plane 1 + T + j target j; single colour: plane 1 the set of tile
 * cells, plane 2 the set of target cells - two targets on one cell give one 1).  Cell ids >= S*S are clamped as the step kernels
 * clamp them.  In real arithmetic the logits are
 *
 *     z = b2 + w2^T relu(b1 + w1^T x),      w1 float32 [D][H], b1 [H], w2 [H][4], b2 [4]
 *
 * The kernels compute them in float32; summation order and the use of fused multiply-adds are not part of the contract.
 *
 * THE DEFINITION of the rollout: for every board n, and k = 0 .. steps - 1,
 *
 *     r    = mix64(key_k + (board_offset + n) * kDrawMul),  key_k = mix64(seed ^ ((step_index + k) * kBoardMul))
 *                                              -- the 64-bit draw of the action stream of tiler_slider.h at (seed, board, step)
 *     rnd  = r >> 62
 *     z    = the logits of the board as it stands (before the step; computed whether or not the board is done)
 *     e    = TS_POLICY_GREEDY: the lowest a with z[a] == max(z)         (on the float32 values the kernel holds and logs)
 *            TS_POLICY_SAMPLE: w[a] = exp(z[a] - max z); c[a] = w[0] + .. + w[a]; u = ((r >> 32) & 0xffffff) * 2^-24;
 *                              the lowest a with u * c[3] < c[a], else 3
 *     a    = ((r & 0xffffffff) < explore_threshold) ? rnd : e
 *     the step of tiler_slider.h on (dims, st, a, mode)
 *
 * Bits 32 .. 55 of r are used by neither the explore test nor rnd.  Everything after `a` is the fused rollout's of
 * tiler_slider_rollout.h: done on entry, auto-reset, the nine outputs, the logs, and in strict mode the early exit once every
 * board of a wave is done - the tail still logs what the loop would log, from the constant logits of a standing board.
 *
 * Non-finite weights are the caller's business: whatever they are, no read or write leaves its buffer and the action played
 * is <= 3.
 *
 * Supported shapes: those of the random policy of tiler_slider_rollout.h (S <= 8, n_tiles <= 8, n_targets <= 8), for every
 * hidden width 1 .. TS_POLICY_MAX_HIDDEN.  Whether the tile-plane weights are staged in LDS or gathered through L2 is a decision
 * of the launch plan, not a limit.
 */
#ifndef TILER_SLIDER_POLICY_H
#define TILER_SLIDER_POLICY_H

#include "tiler_slider_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_POLICY_ABI_VERSION 1
#define TS_POLICY_MAX_HIDDEN 64

/* ts_policy_cfg.select */
#define TS_POLICY_GREEDY 0
#define TS_POLICY_SAMPLE 1

typedef struct ts_mlp {
  const float *w1; /* [D][hidden] */
  const float *b1; /* [hidden] */
  const float *w2; /* [hidden][4] */
  const float *b2; /* [4] */
  int32_t hidden;  /* H, 1 .. TS_POLICY_MAX_HIDDEN */
  int32_t reserved;
} ts_mlp;

typedef struct ts_policy_cfg {
  int32_t steps;       /* K, 0 .. TS_ROLLOUT_MAX_STEPS */
  uint32_t mode;       /* TS_MODE_STRICT or TS_MODE_AUTORESET */
  int32_t select;      /* TS_POLICY_* */
  int32_t write_state; /* 1: pos / step_count / done are stored back; 0: a playout, no state byte is touched */
  uint64_t seed;
  int64_t step_index;
  int64_t board_offset;
  uint64_t explore_threshold; /* 0 .. 2^32, epsilon * 2^32 */
} ts_policy_cfg;

/* The nine fields of ts_rollout_out with the same meaning, and the logits of every step.  Each is optional (NULL); the call
 * needs at least one, or write_state. */
typedef struct ts_policy_out {
  int32_t *wins;
  int32_t *finished;
  int32_t *first_win;
  int32_t *win_moves;
  int32_t *reward_sum;
  uint8_t *flags;
  uint8_t *act_log;
  uint8_t *flags_log;
  void *pos_log;
  float *logits_log; /* [K][N][4] z of step k, the values e was chosen from; 16-byte aligned */
} ts_policy_out;

/* out_mask of the describe call: the TS_ROLLOUT_OUT_* bits, and */
#define TS_POLICY_OUT_LOGITS_LOG 0x200u

int32_t ts_policy_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_policy_last_hip_error(void);

/* 1 where the random policy of tiler_slider_rollout.h plays these dims and 1 <= hidden <= TS_POLICY_MAX_HIDDEN, 0 otherwise, a
 * negative ts_status for invalid dims (TS_ERR_NULL, TS_ERR_DIMS).  Host only. */
int32_t ts_policy_supported(const ts_dims *dims, int32_t hidden);

/* In both calls below "dims" is the dims check every library shares: it also answers TS_ERR_LIMIT for a size above 32 or more
 * than 255 tiles or targets, and does so BEFORE the NULL check of cfg / mlp - a 33x33 call with a NULL cfg is TS_ERR_LIMIT.
 *
 * One forward pass on the boards as they stand: logits float32 [N][4], one 16-byte store per lane.  Checked in this order, before
 * any HIP call: dims (TS_ERR_NULL, TS_ERR_DIMS, TS_ERR_LIMIT beyond the step library's own limits), mlp (TS_ERR_NULL), an
 * unsupported shape or width (TS_ERR_LIMIT); then n_boards = 0 is TS_OK without a launch; then a missing pointer (TS_ERR_NULL: st, logits, a parameter of the network, blk, pos
 * or tgt where there are tiles or targets), then a logits pointer that is not 16-byte aligned (TS_ERR_ARG).  No state is
 * written; step_count and done are not read. */
int32_t ts_policy_logits(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, float *logits, void *stream);

/* One launch: k_policy_rollout<S, select>, one board per lane.  Checked in this order, before any HIP call: dims (TS_ERR_NULL,
 * TS_ERR_DIMS, TS_ERR_LIMIT beyond the step library's own limits), cfg and mlp (TS_ERR_NULL), an unsupported shape or width
 * (TS_ERR_LIMIT), a bad argument (TS_ERR_ARG: mode bits, select, steps outside 0 .. TS_ROLLOUT_MAX_STEPS, explore_threshold above 2^32); then n_boards = 0 and steps = 0 are TS_OK
 * without a launch (nothing is written and no further pointer is looked at); then a missing pointer (TS_ERR_NULL: st, out, a
 * state row, a parameter of the network, or neither an output nor write_state), then a logits_log that is not 16-byte aligned
 * (TS_ERR_ARG).  st->init is read in TS_MODE_AUTORESET only.  Asynchronous on `stream`. */
int32_t ts_policy_rollout(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_policy_cfg *cfg, const ts_policy_out *out,
                          void *stream);

/* What a call would launch, computed by the code it runs before it launches; touches no device. */
typedef struct ts_policy_desc {
  int32_t threads_per_block;
  int32_t lds_bytes;      /* dynamic LDS of a block: the second layer (w2 and b2, 16 * hidden + 16 bytes), the staged tile-plane
                             weights [hidden][slots] and the static pre-activations [hidden][threads_per_block] */
  int32_t weights_in_lds; /* 1: the tile-plane weights are staged in LDS; 0: gathered from global memory (or there are none) */
  int32_t reserved;
  int64_t blocks;         /* grid size; 0 where nothing is launched (name is empty) */
  int64_t logged_bytes;   /* bytes of act_log + flags_log + pos_log + logits_log that out_mask asks for; the logits call: its output */
  char name[64];          /* as rocprofv3 prints it, e.g. "k_policy_rollout<4, 1>" */
} ts_policy_desc;
int32_t ts_describe_policy_rollout(const ts_dims *dims, int32_t hidden, const ts_policy_cfg *cfg, uint32_t out_mask, ts_policy_desc *desc);
int32_t ts_describe_policy_logits(const ts_dims *dims, int32_t hidden, ts_policy_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_POLICY_H */
