/*
 * tiler_slider_ac.h — C-ABI of the actor-critic network (lib/libtiler_slider_ac.so).
 *
 * An eighth library beside the step, search, table, rollout, policy, train and targets libraries: it shares the data layout,
 * ts_dims, ts_state and ts_status of tiler_slider.h (every pointer a DEVICE pointer owned by the caller, `stream` a hipStream_t as
 * void*, every call asynchronous, no allocation, no retained pointers), the network ts_mlp and the limits of
 * tiler_slider_policy.h, the samples ts_train_in, the gradient buffers ts_mlp_grad and the description ts_train_desc of
 * tiler_slider_train.h, and has an ABI version of its own.
 *
 * THE NETWORK.  With ts_mlp of tiler_slider_policy.h unchanged - h = relu(b1 + w1^T x), z = b2 + w2^T h - a value head of two
 * parameters of its own reads the same hidden layer:
 *
 *     v = bv + sum_j wv[j] h_j        wv float32 [H], bv float32 [1]
 *
 * It is not a fifth column of w2: the actor part is exactly a ts_mlp in the kernels' layout, so the tensors a rollout plays and
 * ts_train_forward reads are the ones this library trains.  One forward launch gives the logits and the value of every logged
 * board-step, one backward launch takes both cotangents and ADDS dL/dparameter into six gradient buffers.
 *
 * THE SAMPLES are tiler_slider_train.h's, word for word: a call works on steps * n_boards samples.  Sample (k, n) is board n's
 * level - blk and tgt of ts_state - with the T tile cells c[k][t][n], where c[0] is `first` (cell_t [T][N]) and c[k] is
 * pos_log[k - 1] for k >= 1.  pos_log is exactly the [K][T][N] log a rollout writes (the cells AFTER step k), so its last row is
 * never read; it may be NULL when steps == 1.  Cell ids >= S*S are clamped as everywhere else.  x has set semantics in single
 * colour: a cell two tiles share, or two targets share, contributes once.  Neither call reads st->pos, st->init, step_count or
 * done, and neither writes any state.
 *
 * THE FORWARD: every sample gets the z of tiler_slider_policy.h on that sample's board - out of the same sequence of float
 * operations as the rollout's own logits_log - and v beside it, with the same freedom of summation order and fused multiply-adds.
 *
 * THE BACKWARD, in real arithmetic, for every sample with dz = dlogits[k][n][.] and dv = dvalues[k][n]:
 *
 *     pre_j = b1_j + sum_f x_f w1[f][j]                h_j  = max(pre_j, 0)
 *     dh_j  = sum_a w2[j][a] dz_a + wv[j] dv           dp_j = pre_j > 0 ? dh_j : 0        (the derivative at 0 is 0)
 *
 * and the call ADDS into grad and head_grad
 *
 *     b2[a] += sum dz_a     w2[j][a] += sum h_j dz_a     b1[j] += sum dp_j     w1[f][j] += sum x_f dp_j
 *     bv    += sum dv       wv[j]    += sum h_j dv
 *
 * the sums over all samples.  The caller zeroes the buffers or accumulates into them.  Rows of w1 whose feature no sample has are
 * not written.  Everything is computed in float32; the sums across boards are float atomic adds.  THE ORDER OF THE SUMS IS NOT
 * PART OF THE CONTRACT, and results are NOT reproducible bit for bit from run to run, except where every partial sum is exactly
 * representable (then every order gives the same bits).  Non-finite inputs are the caller's business: whatever they are, no read
 * or write leaves its buffer.  Lanes past the batch add nothing.
 *
 * Supported shapes and widths: exactly those of tiler_slider_policy.h.  Where the weights and the gradient accumulators of a
 * block live (LDS or global memory) is a decision of the launch plan reported by the describe calls, not a limit.
 */
#ifndef TILER_SLIDER_AC_H
#define TILER_SLIDER_AC_H

#include "tiler_slider_train.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_AC_ABI_VERSION 1

/* the value head: v = bv[0] + sum_j wv[j] h_j */
typedef struct ts_value_head {
  const float *wv; /* [H] */
  const float *bv; /* [1] */
} ts_value_head;

/* the layouts of ts_value_head, added into */
typedef struct ts_value_head_grad {
  float *wv;
  float *bv;
} ts_value_head_grad;

int32_t ts_ac_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_ac_last_hip_error(void);

/* Exactly ts_policy_supported.  Host only. */
int32_t ts_ac_supported(const ts_dims *dims, int32_t hidden);

/* Both calls check, in this order and before any HIP call: dims (the check every library shares: TS_ERR_NULL, TS_ERR_DIMS, and
 * TS_ERR_LIMIT for a size above 32 or more than 255 tiles or targets - BEFORE the NULL check of mlp / in), mlp and in
 * (TS_ERR_NULL), an unsupported shape or width (TS_ERR_LIMIT), steps outside 1 .. TS_ROLLOUT_MAX_STEPS (TS_ERR_ARG); then
 * n_boards = 0 is TS_OK without a launch; then a missing pointer (TS_ERR_NULL: st, blk, tgt where there are targets, first where
 * there are tiles, pos_log where there are tiles and steps > 1, a parameter of the network, head or one of its two parameters,
 * grad or one of its four buffers, head_grad or one of its two buffers, logits / dlogits, values / dvalues - both cotangents are
 * required: a caller without one passes zeros), then a logits / dlogits pointer that is not 16-byte aligned or a values / dvalues
 * pointer that is not 4-byte aligned (TS_ERR_ARG).
 *
 * One launch, k_ac_forward<S>, one board per lane: logits float32 [K][N][4], one 16-byte store per sample; values float32 [K][N],
 * one 4-byte store per sample; both contiguous across lanes. */
int32_t ts_ac_forward(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_value_head *head, const ts_train_in *in,
                      float *logits, float *values, void *stream);

/* One launch, k_ac_backward<S>: dlogits float32 [K][N][4], dvalues float32 [K][N]; adds into the four buffers of grad and the two
 * of head_grad. */
int32_t ts_ac_backward(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_value_head *head, const ts_train_in *in,
                       const float *dlogits, const float *dvalues, const ts_mlp_grad *grad, const ts_value_head_grad *head_grad,
                       void *stream);

/* What a call would launch, computed by the code it runs before it launches; touches no device.  The fields are ts_train_desc's:
 * grads_in_lds speaks of the gradient of w1 (those of b1, w2, b2, wv and bv always are in LDS), flush_bytes of the forward is the
 * bytes of both outputs. */
int32_t ts_describe_ac_forward(const ts_dims *dims, int32_t hidden, int32_t steps, ts_train_desc *desc);
int32_t ts_describe_ac_backward(const ts_dims *dims, int32_t hidden, int32_t steps, ts_train_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_AC_H */
