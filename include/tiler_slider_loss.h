/*
 * tiler_slider_loss.h — C-ABI of the fused actor-critic loss (lib/libtiler_slider_loss.so).
 *
 * A tenth library beside the step, search, table, rollout, policy, train, targets, actor-critic and in-place-step libraries,
 * with an ABI version of its own.  It shares ts_status with tiler_slider.h and the conventions of every other call: every
 * pointer a DEVICE pointer owned by the caller, `stream` a hipStream_t as void*, every call asynchronous, no host
 * synchronisation, no allocation, no retained pointers.  It knows no board: it works on M = n_samples samples (M = K * N for a
 * logged trajectory) and takes no ts_dims.
 *
 * It computes, in one pass over the samples, the loss between the network's outputs (tiler_slider_ac.h: logits [M][4], values
 * [M]) and the trajectory targets (tiler_slider_targets.h: adv, ret, mask, or the expert's labels) TOGETHER WITH ITS GRADIENT
 * with respect to the logits and the values: an advantage-weighted log-likelihood (A2C), its clipped-ratio form (PPO), or a
 * cross-entropy against labels (adv == NULL), each with an entropy bonus and a squared-error value term.
 *
 * DEFINITION (real arithmetic).  Sample i is LIVE when act[i] <= 3 and (mask == NULL or mask[i] != 0).  count is the number of
 * live samples and c = 1 / max(count, 1).  With z = logits[i]:
 *
 *     lp = log_softmax(z), taken through the max;  p = exp(lp);  a = act[i]
 *     A  = 1 where adv == NULL, otherwise adv[i];
 *          with normalize_adv, A = (adv[i] - mu) / (sigma + 1e-8): mu the mean of adv over the live samples, sigma their
 *          population standard deviation
 *
 * and per live sample
 *
 *     policy, old_logits == NULL (A2C, cross-entropy):   l_pi = -A lp[a]                        g = -A
 *     policy, old_logits given and clip > 0 (PPO):       r    = exp(lp[a] - log_softmax(old_logits[i])[a])
 *                                                        l_pi = -min(r A, clamp(r, 1 - clip, 1 + clip) A)
 *                                                        g    = -r A where the unclipped term is the minimum
 *                                                               (r A <= clamp(r) A), otherwise 0
 *     entropy:                                           H    = -sum_j p_j lp_j
 *     value, where values and ret are given:             l_v  = (values[i] - ret[i])^2
 *     total:                                             l    = l_pi + value_coef l_v - entropy_coef H
 *
 *     L = c sum_live l
 *     dlogits[i][j] = c (g (delta_aj - p_j) + entropy_coef p_j (lp_j + H))
 *     dvalues[i]    = 2 c value_coef (values[i] - ret[i])
 *
 * dlogits and dvalues are the gradient of L.  Both are EXACTLY 0 on a sample that is not live, whatever that sample's inputs
 * hold, NaN included.  Both are always written (dvalues where there is a value term); the call does not accumulate.
 *
 *     scalars float32 [8]:  [0] L   [1] c sum l_pi   [2] c sum l_v   [3] c sum H
 *                           [4] the approximate KL c sum ((r - 1) - log r)  (0 without old_logits)
 *                           [5] the share of live samples whose g was cut to 0 (0 without old_logits)
 *                           [6] count   [7] mu (0 without adv)
 *
 * Non-finite live logits are the caller's business.  Finite live logits of any spread give finite lp, p, H and A2C outputs: the
 * max is subtracted before the exponential.  (The ratio r is a float32: policies more than e^88 apart overflow it.)
 *
 * NOT BUILT: value clipping; an epsilon-mixed behaviour policy in the ratio; per-sample weights; bf16.
 *
 * ARITHMETIC.  Float32 throughout (the three sums of the advantage statistics - count, sum adv, sum adv^2 - are held as an
 * integer and two float64, so that sigma does not suffer the cancellation of a float32 sum of squares).  exp and log are the
 * hardware's (__expf, __logf).  The order of the operations inside one sample and the use of fused multiply-adds are NOT PART
 * OF THE CONTRACT.  NO FLOAT ATOMICS ANYWHERE: every sum over samples is taken over lanes, then the wave, then the block through
 * LDS, then ONE PARTIAL PER BLOCK in `workspace`, then by a one-block kernel that adds the partials in a fixed order.  Results
 * are therefore reproducible bit for bit from run to run.
 *
 * LAUNCHES, in stream order: k_loss_stats (count, mu, sigma: a pass over act, mask and adv, 2 or 6 bytes a sample),
 * k_loss_finish, k_loss_main (one sample per lane: everything else), k_loss_finish.  The grid of the two passes is bounded at
 * TS_LOSS_MAX_BLOCKS blocks of TS_LOSS_THREADS threads, grid-stride beyond.
 */
#ifndef TILER_SLIDER_LOSS_H
#define TILER_SLIDER_LOSS_H

#include "tiler_slider.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_LOSS_ABI_VERSION 1

#define TS_LOSS_THREADS 256
#define TS_LOSS_MAX_BLOCKS 2048
#define TS_LOSS_SCALARS 8

/* `what` of ts_describe_loss: the optional inputs a call would read */
#define TS_LOSS_OLD_LOGITS 0x01u
#define TS_LOSS_VALUES 0x02u /* values, ret and dvalues */
#define TS_LOSS_ADV 0x04u
#define TS_LOSS_MASK 0x08u

typedef struct ts_loss_in {
  const float *logits;     /* [M][4], 16-byte aligned */
  const float *old_logits; /* [M][4], 16-byte aligned; NULL: no ratio (A2C, cross-entropy) */
  const uint8_t *act;      /* [M]: the action played, or the label; a byte above 3 (255) is a sample that is not live */
  const uint8_t *mask;     /* [M]; NULL: every sample with act <= 3 is live */
  const float *adv;        /* [M]; NULL: 1 (cross-entropy) */
  const float *values;     /* [M]; NULL (with ret): no value term */
  const float *ret;        /* [M] */
  int64_t n_samples;       /* M >= 0 */
  float clip;              /* >= 0; > 0 where old_logits is given; checked, then unused, without old_logits */
  float value_coef;
  float entropy_coef;
  int32_t normalize_adv;   /* 0 or not 0; needs adv */
} ts_loss_in;

typedef struct ts_loss_out {
  float *dlogits;  /* [M][4], 16-byte aligned */
  float *dvalues;  /* [M]; NULL exactly where values is */
  float *scalars;  /* [TS_LOSS_SCALARS] */
  void *workspace; /* ts_loss_workspace_bytes(M) bytes, 4-byte aligned: the partials; contents undefined afterwards */
} ts_loss_out;

int32_t ts_loss_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_loss_last_hip_error(void);

/* Bytes of workspace a call on n_samples needs (0 for n_samples = 0); TS_ERR_ARG for n_samples < 0.  Host only. */
int64_t ts_loss_workspace_bytes(int64_t n_samples);

/* Checks, in this order and before any HIP call:
 *   1. in, out                                                                                   TS_ERR_NULL
 *   2. n_samples < 0; clip < 0 or NaN; old_logits given with clip == 0; exactly one of values and ret given; dvalues given
 *      without values; normalize_adv without adv; a coefficient that is NaN                      TS_ERR_ARG
 *   3. n_samples == 0: TS_OK without a launch; the eight scalars, where `scalars` is given, are written as 0 by a memset
 *      on the stream
 *   4. logits, act, dlogits, scalars, workspace, and dvalues where there is a value term         TS_ERR_NULL
 *   5. logits, old_logits, dlogits not 16-byte aligned; adv, values, ret, dvalues, scalars, workspace not 4-byte aligned
 *                                                                                                TS_ERR_ARG
 *   6. an output range (dlogits, dvalues, scalars, workspace) that overlaps an input or another output   TS_ERR_ARG
 * Four launches: k_loss_stats, k_loss_finish, k_loss_main, k_loss_finish. */
int32_t ts_actor_critic_loss(const ts_loss_in *in, const ts_loss_out *out, void *stream);

/* What a call would launch, computed by the code it runs before it launches; touches no device. */
typedef struct ts_loss_desc {
  int32_t threads_per_block; /* of all three kernels */
  int32_t lds_bytes;         /* static LDS of a block of k_loss_main; the other two use no more than 256 bytes */
  int32_t launches;          /* 4; 0 where nothing is launched */
  int32_t reserved;
  int64_t blocks;            /* grid of k_loss_stats and of k_loss_main (k_loss_finish: one block); 0: nothing is launched */
  int64_t partials;          /* partial sums per reduced quantity: one per block */
  int64_t samples;
  int64_t workspace_bytes;
  int64_t bytes_read;        /* algorithmic, both passes, for `what`; the partials are not counted */
  int64_t bytes_written;
  char name[64];             /* as rocprofv3 prints it: "k_loss_main" */
  char stats_name[32];       /* "k_loss_stats" */
  char finish_name[32];      /* "k_loss_finish" */
} ts_loss_desc;
/* `what`: TS_LOSS_*; bits beyond those, or n_samples < 0, give TS_ERR_ARG; a NULL desc TS_ERR_NULL */
int32_t ts_describe_loss(int64_t n_samples, uint32_t what, ts_loss_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_LOSS_H */
