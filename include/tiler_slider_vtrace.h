/*
 * tiler_slider_vtrace.h — C-ABI of the V-trace targets (lib/libtiler_slider_vtrace.so).
 *
 * Off-policy returns for a logged trajectory whose actions were NOT drawn from the network that is being trained: a mixed or
 * epsilon-greedy rollout (tiler_slider_mixed.h, tiler_slider_policy.h), or a log replayed after the weights have moved.  V-trace
 * (Espeholt et al. 2018, "IMPALA"): truncated importance weights min(bar, pi / mu) inside the backward recursion that
 * ts_traj_returns runs, one launch, one pass over the log per board.  A twenty-first library: it shares the data layout, ts_dims,
 * ts_state and ts_status of tiler_slider.h (every pointer a DEVICE pointer owned by the caller, `stream` a hipStream_t as void*,
 * every call asynchronous, no allocation, no retained pointers, no state written), the samples, flags, reward and values of
 * tiler_slider_targets.h, the select rules of tiler_slider_policy.h and the thresholds of tiler_slider_mixed.h, and has an ABI
 * version of its own.  The reward rule and the flag rules are restated from tiler_slider_targets.h.
 *
 * THE DEFINITION.  The samples, void_k, end_k, m(), r_k, V_k, V+_k, value_stride and the clamping are exactly those of
 * ts_traj_returns (tiler_slider_targets.h).  A TIMEOUT cuts the bootstrap there, and it cuts it here.  For sample (k, n):
 *
 *     a     = min(act_log[k][n], 3)
 *     x     = expert_log ? expert_log[k][n] : 255
 *     eps   = explore_threshold * 2^-32,  beta = beta_threshold * 2^-32     (the thresholds of ts_mixed_cfg, 0 .. 2^32)
 *     p_e   = TS_POLICY_SAMPLE: softmax(mu_logits[k][n])
 *             TS_POLICY_GREEDY: 1 at the lowest argmax of mu_logits[k][n], 0 elsewhere
 *     inner = (beta_threshold != 0 && x != 255) ? beta [a == x] + (1 - beta) p_e[a] : p_e[a]
 *     mu    = eps / 4 + (1 - eps) inner
 *     pi    = softmax(pi_logits ? pi_logits[k][n] : mu_logits[k][n])[a]
 *     w     = mu > 0 ? pi / mu : +infinity       (mu == 0: the logs contradict the parameters; the clipped weights are then the bars)
 *     rho   = min(rho_bar, w),   c = lam * min(c_bar, w)
 *
 * mu is the probability with which ts_policy_rollout / ts_mixed_rollout play `a` from these logits, this expert's move and these
 * two thresholds.  THE SOFTMAX IS THE MODEL: the 24-bit uniform of the sampler quantises its probabilities by at most 2^-24, and
 * that is not modelled.  Backwards, k = K - 1 .. 0, with a carry D+ that starts at 0:
 *
 *     void_k:  every output 0, mask 0; the carry is left as it is
 *     else:    delta = rho (r_k + gamma V+_k - V_k)
 *              D_k   = delta + (end_k ? 0 : gamma c D+)
 *              ret   = V_k + D_k                                  (the V-trace target v_s)
 *              adv   = rho (r_k + gamma (end_k ? 0 : V+_k + D+) - V_k)   (the policy-gradient advantage, weight included)
 *              weight = w,  log_mu = log(mu)  (-infinity where mu == 0),  reward = r_k,  mask = 1;   D+ <- D_k
 *
 * Arithmetic is float32; the order of sums and the use of fused multiply-adds are NOT PART OF THE CONTRACT.  The exponentials and
 * the logarithm are the hardware's (__expf, __logf, as in ts_loss.hip), the softmax goes through the maximum, p = e / s, and
 * EVERY DIVISION - e / s of either softmax and pi / mu - IS THE CORRECTLY ROUNDED IEEE DIVISION (no reciprocal approximation):
 * x / x is exactly 1.  eps and beta reach the kernel as float32 (the threshold times 2^-32, rounded once).  No atomics are used: a
 * call gives the same bits on every run.
 *
 * TWO IDENTITIES are part of the contract.
 *   1. With pi_logits == NULL, both thresholds 0 and TS_POLICY_SAMPLE, w is exactly 1.0 on every live sample: pi and p_e[a] are then
 *      ONE value, computed once by one expression, mu is that value, and the division is exact.
 *   2. With rho_bar, c_bar >= 1, `ret` is then ts_traj_returns' ret for every lam, and `adv` is its adv at lam = 1.
 *
 * first, pos_log, st->tgt and st may be NULL exactly where ts_traj_returns allows it; the cells are read only where w_dist or
 * w_progress is not 0.  Supported shapes: exactly those of ts_targets_supported(dims, TS_TARGETS_RETURNS).
 *
 * NOT BUILT: timeouts as truncation, a separate clip for the policy-gradient weight, Retrace / Q(lambda), who_log-conditioned
 * probabilities, bf16.
 */
#ifndef TILER_SLIDER_VTRACE_H
#define TILER_SLIDER_VTRACE_H

#include "tiler_slider_policy.h"
#include "tiler_slider_targets.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_VTRACE_ABI_VERSION 1

/* `what` of the describe call: the outputs asked for ... */
#define TS_VTRACE_OUT_REWARD 0x01u
#define TS_VTRACE_OUT_ADV 0x02u
#define TS_VTRACE_OUT_RET 0x04u
#define TS_VTRACE_OUT_MASK 0x08u
#define TS_VTRACE_OUT_WEIGHT 0x10u
#define TS_VTRACE_OUT_LOG_MU 0x20u
/* ... and what a ts_traj_vtrace call would read beside flags_log, act_log and mu_logits */
#define TS_VTRACE_IN_CELLS 0x40u       /* w_dist or w_progress is not 0: pos_log and the targets */
#define TS_VTRACE_IN_FIRST 0x80u       /* w_progress is not 0 */
#define TS_VTRACE_IN_VALUES 0x100u     /* values is given */
#define TS_VTRACE_IN_LAST_VALUE 0x200u /* last_value is given */
#define TS_VTRACE_IN_EXPERT 0x400u     /* expert_log is given */
#define TS_VTRACE_IN_PI 0x800u         /* pi_logits is given */

/* the fields of ts_returns_in with their meaning, and the behaviour policy */
typedef struct ts_vtrace_in {
  const void *first;        /* cell_t [T][N]: c[0]; may be NULL when w_progress == 0 */
  const void *pos_log;      /* cell_t [K][T][N]; may be NULL when w_dist == w_progress == 0 */
  const uint8_t *flags_log; /* [K][N] */
  const float *values;      /* board n of row k at values[(k * N + n) * value_stride]; may be NULL: every V_k is 0 */
  const float *last_value;  /* [N]; may be NULL: 0 */
  int32_t steps;            /* K, 1 .. TS_ROLLOUT_MAX_STEPS */
  int32_t value_stride;     /* 1 or 4 (checked with or without values) */
  float gamma, lam;         /* each in [0, 1] */
  float w_step, w_win, w_timeout, w_invalid, w_dist, w_progress;
  const uint8_t *act_log;    /* [K][N]: the action played */
  const uint8_t *expert_log; /* [K][N]: the expert's move, 255 where it had none; may be NULL: 255 everywhere */
  const float *mu_logits;    /* [K][N][4]: the logits each action was selected from (logits_log); 16-byte aligned */
  const float *pi_logits;    /* [K][N][4]: the target policy's logits; may be NULL: mu_logits; 16-byte aligned */
  int32_t select;            /* TS_POLICY_*: how the rollout selected */
  int32_t reserved;
  uint64_t explore_threshold; /* 0 .. 2^32, epsilon * 2^32: the rollout's */
  uint64_t beta_threshold;    /* 0 .. 2^32, beta * 2^32: the rollout's */
  float rho_bar, c_bar;       /* each >= 0; +infinity: no clipping */
} ts_vtrace_in;

/* each may be NULL, not all six */
typedef struct ts_vtrace_out {
  float *reward; /* [K][N] */
  float *adv;    /* [K][N] */
  float *ret;    /* [K][N] */
  float *weight; /* [K][N]: w, unclipped */
  float *log_mu; /* [K][N] */
  uint8_t *mask; /* [K][N]: 1 where a transition was played */
} ts_vtrace_out;

int32_t ts_vtrace_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_vtrace_last_hip_error(void);

/* Exactly ts_targets_supported(dims, TS_TARGETS_RETURNS): 1 / 0, a negative status for invalid dims (TS_ERR_LIMIT counts as 0).
 * Host only. */
int32_t ts_vtrace_supported(const ts_dims *dims);

/* One launch, one board per lane: k_traj_vtrace<S> where the cells are read (w_dist or w_progress is not 0 and there are tiles),
 * k_traj_vtrace<0>, one kernel for every size, where they are not - A TEMPLATE PARAMETER, NOT A BRANCH: ts_vtrace_desc.cells_kernel
 * says which.  Checked in this order, before any HIP call:
 *   1. dims: the dims check every library shares (TS_ERR_NULL, TS_ERR_DIMS, and TS_ERR_LIMIT for a size above 32 or more than 255
 *      tiles or targets - BEFORE the NULL checks);
 *   2. in or out NULL (TS_ERR_NULL);
 *   3. an unsupported shape (TS_ERR_LIMIT);
 *   4. a bad argument (TS_ERR_ARG): steps outside 1 .. TS_ROLLOUT_MAX_STEPS, an unknown select, explore_threshold or beta_threshold
 *      above 2^32, gamma or lam outside [0, 1] or NaN, a rho_bar or c_bar that is negative or NaN (+infinity is allowed: no
 *      clipping), a value_stride other than 1 or 4;
 *   5. n_boards = 0 is TS_OK without a launch: no pointer is looked at;
 *   6. a missing pointer (TS_ERR_NULL): ts_traj_returns' rules - flags_log; where the cells are read and there are tiles pos_log,
 *      first if w_progress != 0, and st and st->tgt where there are targets; no output at all - and act_log and mu_logits;
 *   7. alignment (TS_ERR_ARG): mu_logits and pi_logits at 16 bytes, every other float pointer - values, last_value, reward, adv,
 *      ret, weight, log_mu - at 4.
 * Asynchronous on `stream`. */
int32_t ts_traj_vtrace(const ts_dims *dims, const ts_state *st, const ts_vtrace_in *in, const ts_vtrace_out *out, void *stream);

/* What a call would launch, computed by the code it runs before it launches; touches no device.  The fields of ts_targets_desc. */
typedef struct ts_vtrace_desc {
  int32_t threads_per_block;
  int32_t lds_bytes;     /* dynamic LDS of a block: 0, no kernel uses any */
  int32_t chunk_steps;   /* steps of a board whose loads are issued together and whose weights are computed before the recursion */
  int32_t cells_kernel;  /* 1: k_traj_vtrace<S>, the kernel that reads the cells; 0: k_traj_vtrace<0>, which holds no such code */
  int64_t blocks;        /* grid size; 0 where nothing is launched (name is empty) */
  int64_t samples;       /* steps * n_boards */
  int64_t bytes_read;    /* algorithmic: flags, actions, mu_logits and what `what` names, and the level */
  int64_t bytes_written; /* the outputs of `what` */
  char name[64];         /* as rocprofv3 prints it, e.g. "k_traj_vtrace<4>" */
} ts_vtrace_desc;
/* dims or desc NULL is TS_ERR_NULL; then checks 1 and 3 of ts_traj_vtrace, steps as in 4, and `what`: TS_VTRACE_OUT_* |
 * TS_VTRACE_IN_*; bits beyond those, or no output bit, give TS_ERR_ARG.  TS_VTRACE_IN_FIRST implies TS_VTRACE_IN_CELLS. */
int32_t ts_describe_traj_vtrace(const ts_dims *dims, int32_t steps, uint32_t what, ts_vtrace_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_VTRACE_H */
