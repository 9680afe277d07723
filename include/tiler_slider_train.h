/*
 * tiler_slider_train.h — C-ABI of the trainable policies (lib/libtiler_slider_train.so).
 *
 * A sixth library beside the step, search, table, rollout and policy libraries: it shares the data layout, ts_dims, ts_state and
 * ts_status of tiler_slider.h (every pointer a DEVICE pointer owned by the caller, `stream` a hipStream_t as void*, every call
 * asynchronous, no allocation, no retained pointers), the network ts_mlp and the limits of tiler_slider_policy.h, and has an ABI
 * version of its own.  It makes the logits of a logged trajectory a differentiable function of the network's parameters: one
 * forward launch over all steps * n_boards logged board-steps, one backward launch that takes dL/dlogits and ADDS dL/dparameter
 * into four gradient buffers.  The loss stays the caller's.
 *
 * THE SAMPLES.  A call works on steps * n_boards samples.  Sample (k, n) is board n's level - blk and tgt of ts_state - with the
 * T tile cells c[k][t][n], where c[0] is `first` (cell_t [T][N]) and c[k] is pos_log[k - 1] for k >= 1.  pos_log is exactly the
 * [K][T][N] log a rollout writes (the cells AFTER step k), so its last row is never read; it may be NULL when steps == 1.  c[k] is
 * the board the logits of step k of ts_policy_rollout were computed on, in strict and in auto-reset mode.  With steps = 1 and
 * first = st->pos the call is "the boards as they stand".  Cell ids >= S*S are clamped as everywhere else.  Neither call reads
 * st->pos, st->init, step_count or done, and neither writes any state.
 *
 * THE FORWARD: every sample gets the z of tiler_slider_policy.h on that sample's board: the same features, the same set semantics
 * in single colour, the same freedom of summation order and fused multiply-adds.
 *
 * THE BACKWARD, in real arithmetic, for every sample with dz = dlogits[k][n][.]:
 *
 *     pre_j = b1_j + sum_f x_f w1[f][j]        h_j  = max(pre_j, 0)
 *     dh_j  = sum_a w2[j][a] dz_a              dp_j = pre_j > 0 ? dh_j : 0        (the derivative at 0 is 0)
 *
 * and the call ADDS into grad
 *
 *     b2[a] += sum dz_a     w2[j][a] += sum h_j dz_a     b1[j] += sum dp_j     w1[f][j] += sum x_f dp_j
 *
 * the sums over all samples.  The caller zeroes grad or accumulates into it.  Rows of w1 whose feature no sample has are not
 * written.  x has set semantics in single colour: a cell two tiles share, or two targets share, contributes once.  Everything is
 * computed in float32; the sums across boards are float atomic adds.  THE ORDER OF THE SUMS IS NOT PART OF THE CONTRACT, and
 * results are NOT reproducible bit for bit from run to run, except where every partial sum is exactly representable (then every
 * order gives the same bits).  Non-finite inputs are the caller's business: whatever they are, no read or write leaves its buffer.
 * Lanes past the batch add nothing.
 *
 * Supported shapes and widths: exactly those of tiler_slider_policy.h.  Where the weights and the gradient accumulators of a
 * block live (LDS or global memory) is a decision of the launch plan reported by the describe calls, not a limit.
 */
#ifndef TILER_SLIDER_TRAIN_H
#define TILER_SLIDER_TRAIN_H

#include "tiler_slider_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_TRAIN_ABI_VERSION 1

typedef struct ts_train_in {
  const void *first;   /* cell_t [T][N]: c[0] */
  const void *pos_log; /* cell_t [K][T][N]: c[k] = pos_log[k - 1]; may be NULL when steps == 1 */
  int32_t steps;       /* K, 1 .. TS_ROLLOUT_MAX_STEPS */
  int32_t reserved;
} ts_train_in;

/* the layouts of ts_mlp: [D][H], [H], [H][4], [4] */
typedef struct ts_mlp_grad {
  float *w1;
  float *b1;
  float *w2;
  float *b2;
} ts_mlp_grad;

int32_t ts_train_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_train_last_hip_error(void);

/* Exactly ts_policy_supported.  Host only. */
int32_t ts_train_supported(const ts_dims *dims, int32_t hidden);

/* Both calls check, in this order and before any HIP call: dims (the check every library shares: TS_ERR_NULL, TS_ERR_DIMS, and
 * TS_ERR_LIMIT for a size above 32 or more than 255 tiles or targets - BEFORE the NULL check of mlp / in), mlp and in
 * (TS_ERR_NULL), an unsupported shape or width (TS_ERR_LIMIT), steps outside 1 .. TS_ROLLOUT_MAX_STEPS (TS_ERR_ARG); then
 * n_boards = 0 is TS_OK without a launch; then a missing pointer (TS_ERR_NULL: st, blk, tgt where there are targets, first where
 * there are tiles, pos_log where there are tiles and steps > 1, a parameter of the network, grad or one of its four buffers,
 * logits / dlogits), then a logits / dlogits pointer that is not 16-byte aligned (TS_ERR_ARG).
 *
 * One launch, k_train_forward<S>, one board per lane: logits float32 [K][N][4], one 16-byte store per sample. */
int32_t ts_train_forward(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_train_in *in, float *logits, void *stream);

/* One launch, k_train_backward<S>: dlogits float32 [K][N][4]; adds into the four buffers of grad. */
int32_t ts_train_backward(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_train_in *in, const float *dlogits,
                          const ts_mlp_grad *grad, void *stream);

/* What a call would launch, computed by the code it runs before it launches; touches no device. */
typedef struct ts_train_desc {
  int32_t threads_per_block;
  int32_t lds_bytes;      /* dynamic LDS of a block, all of it */
  int32_t weights_in_lds; /* 1: the tile-plane weights are staged in LDS; 0: gathered from global memory (or there are none) */
  int32_t grads_in_lds;   /* backward: 2 the whole gradient of w1 is accumulated in LDS and flushed once per block, 1 its tile
                             planes only (obstacle and target rows by global atomics, once per board and unit), 0 none of it
                             (every add to w1's gradient is a global atomic); the gradients of b1, w2 and b2 always are.
                             forward: 0 */
  int32_t chunk_steps;    /* backward: steps of a board held in registers while the hidden units are walked; forward: 0 */
  int32_t reserved;
  int64_t blocks;         /* grid size; 0 where nothing is launched (name is empty).  The backward grid is bounded: a block
                             strides over groups of threads_per_block boards */
  int64_t samples;        /* steps * n_boards */
  int64_t flush_bytes;    /* backward: bytes of float atomic adds of the end-of-block flushes of the whole grid at the most (zero
                             entries are skipped); the forward: the bytes of its output */
  char name[64];          /* as rocprofv3 prints it, e.g. "k_train_backward<4>" */
} ts_train_desc;
int32_t ts_describe_train_forward(const ts_dims *dims, int32_t hidden, int32_t steps, ts_train_desc *desc);
int32_t ts_describe_train_backward(const ts_dims *dims, int32_t hidden, int32_t steps, ts_train_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_TRAIN_H */
