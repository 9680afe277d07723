/*
 * tiler_slider_optim.h — C-ABI of the fused optimiser (lib/libtiler_slider_optim.so): the global-norm clip, AdamW and the
 * zeroing of the gradients in one launch.
 *
 * An eleventh library beside the step, search, table, rollout, policy, train, targets, actor-critic, in-place-step and loss
 * libraries, with an ABI version of its own.  It shares ts_status with tiler_slider.h and the conventions of every other call:
 * every pointer a DEVICE pointer owned by the caller, `stream` a hipStream_t as void*, every call asynchronous, no host
 * synchronisation, no allocation, no retained pointers.  Like the loss library it knows no board and takes no ts_dims.
 *
 * A call works on n <= TS_OPTIM_MAX_TENSORS tensors.  Tensor i has numel[i] >= 0 contiguous float32 elements in four arrays:
 * param[i], grad[i], m[i], v[i].  4-byte alignment is required; where all four pointers of a tensor are 16-byte aligned the
 * kernel moves 16 bytes at a time - a uniform decision per tensor, which changes no result.
 *
 * The device state is int64_t counters[2] (8-byte aligned): [0] is t, the updates applied so far; [1] the updates skipped.
 *
 * DEFINITION (real arithmetic), over all elements of all tensors:
 *
 *     gn  = sqrt(sum g^2)                                  -- the global gradient norm, before clipping
 *     c   = max_grad_norm > 0 ? min(1, max_grad_norm / (gn + 1e-6)) : 1      (clip_grad_norm_'s rule)
 *     if skip_nonfinite and gn is not finite:
 *         nothing changes but counters[1] += 1; grads are still zeroed where zero_grad is set
 *     else, with g^ = c g and t' = counters[0] + 1:
 *         m' = beta1 m + (1 - beta1) g^          v' = beta2 v + (1 - beta2) g^2
 *         p' = p (1 - lr weight_decay) - lr (m' / (1 - beta1^t')) / (sqrt(v' / (1 - beta2^t')) + eps)
 *         counters[0] = t'
 *     grad = 0 where zero_grad is set;  grad_norm[0] = gn where grad_norm is given (float32)
 *
 * (v' takes g^ too: g^2 above is the square of the clipped gradient.)  Weight decay is decoupled (AdamW's).
 *
 * NOT BUILT: amsgrad; L2 (coupled) decay; several parameter groups; bf16 or 8-bit state; other rules.
 *
 * ARITHMETIC, part of the contract.
 *   - THE SUM OF SQUARES IS ACCUMULATED IN FLOAT64: lanes, then the wave, then the block through LDS, then ONE PARTIAL PER BLOCK
 *     in `workspace`, then the partials added in a fixed order (partial j belongs to thread j mod 256 of the adding block, which
 *     takes its own in index order; then the wave, then the four waves in order).  NO FLOAT ATOMICS ANYWHERE.  gn is therefore
 *     right to within one float32 rounding, cannot overflow for finite float32 gradients (a float32 sum of squares reports a
 *     false non-finite norm from |g| ~ 1.8e19 on), and results are reproducible bit for bit from run to run.
 *   - beta1 and beta2 are doubles.  1 - beta^t' (beta^t' by repeated squaring in float64) and 1 - beta are evaluated in double
 *     and rounded to float32 once; c is evaluated in double from gn and rounded to float32 once.
 *   - Everything else is float32.  The order of the operations inside one element and the use of fused multiply-adds are NOT
 *     PART OF THE CONTRACT.  Division and square root are the correctly rounded ones.
 *   - lr is taken by value, or read from lr_dev (one float32 on the device) where that is not NULL: a schedule then works
 *     inside a captured graph.
 *
 * LAUNCHES.  The norm pass is needed when max_grad_norm > 0, skip_nonfinite is set or grad_norm is given.
 *   TS_OPTIM_FORM_ONE    total <= the one-block constant (ts_optim_tuning): ONE launch of ONE block of TS_OPTIM_ONE_THREADS
 *                        threads, k_optim_one: pass 1 for the norm (left out where no norm is needed), a barrier, pass 2 for
 *                        the update, a barrier, then one thread writes the counters.
 *   TS_OPTIM_FORM_MULTI  total above it, norm needed: k_optim_norm on min(chunks, TS_OPTIM_MAX_BLOCKS) blocks of
 *                        TS_OPTIM_THREADS threads, grid-stride beyond, one float64 partial per block into `workspace`; then
 *                        k_optim_apply on the same grid, in which every block adds the partials in the fixed order; then
 *                        k_optim_finish, one block.  Three launches.
 *   TS_OPTIM_FORM_APPLY  total above it, no norm needed: k_optim_apply, then k_optim_finish.  Two launches.
 * Every block reads counters[0] and the call writes it once: in the multi-block forms the write is k_optim_finish's, a launch
 * that stream order puts after every block's read; the one-block form writes after its last barrier.
 * A chunk is TS_OPTIM_CHUNK consecutive elements of ONE tensor (four per thread of a block); a tensor's last chunk is ragged,
 * and a chunk never straddles two tensors.  Chunks are numbered through the tensors in order and dealt to the blocks round-robin.
 * In the one block a chunk is TS_OPTIM_ONE_CHUNK elements, four per lane of one wave, dealt to its sixteen waves round-robin.
 */
#ifndef TILER_SLIDER_OPTIM_H
#define TILER_SLIDER_OPTIM_H

#include "tiler_slider.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TS_OPTIM_ABI_VERSION 1

#define TS_OPTIM_MAX_TENSORS 32
#define TS_OPTIM_THREADS 256
#define TS_OPTIM_ONE_THREADS 1024
#define TS_OPTIM_CHUNK 1024    /* elements of a chunk of the multi-block forms: four a thread of a block */
#define TS_OPTIM_ONE_CHUNK 256 /* elements of a chunk of the one block: four a lane of ONE WAVE, sixteen chunks in flight */
#define TS_OPTIM_MAX_BLOCKS 1024

#define TS_OPTIM_FORM_NONE 0
#define TS_OPTIM_FORM_ONE 1
#define TS_OPTIM_FORM_MULTI 2
#define TS_OPTIM_FORM_APPLY 3

/* `what` of ts_describe_adam_step */
#define TS_OPTIM_NORM 0x01u      /* the norm pass: a clip, skip_nonfinite or grad_norm */
#define TS_OPTIM_ZERO_GRAD 0x02u

typedef struct ts_optim_tensors {
  int32_t n_tensors; /* 0 .. TS_OPTIM_MAX_TENSORS */
  int32_t reserved;
  int64_t numel[TS_OPTIM_MAX_TENSORS];
  float *param[TS_OPTIM_MAX_TENSORS];
  float *grad[TS_OPTIM_MAX_TENSORS]; /* read; written (0) only with zero_grad */
  float *m[TS_OPTIM_MAX_TENSORS];
  float *v[TS_OPTIM_MAX_TENSORS];
} ts_optim_tensors;

typedef struct ts_adam_cfg {
  double beta1, beta2;   /* in [0, 1) */
  const float *lr_dev;   /* NULL: `lr`; otherwise one float32 on the device, read by the launch */
  float lr;              /* >= 0 */
  float eps;             /* >= 0 */
  float weight_decay;    /* >= 0, decoupled */
  float max_grad_norm;   /* >= 0; 0: no clip */
  int32_t skip_nonfinite; /* 0 or not 0 */
  int32_t zero_grad;      /* 0 or not 0 */
} ts_adam_cfg;

typedef struct ts_optim_out {
  int64_t *counters; /* [2], 8-byte aligned: updates applied, updates skipped */
  float *grad_norm;  /* [1]; NULL: not wanted */
  void *workspace;   /* ts_optim_workspace_bytes(total) bytes, 8-byte aligned: the partials; NULL is fine where the form is
                        not TS_OPTIM_FORM_MULTI; contents undefined afterwards */
} ts_optim_out;

int32_t ts_optim_abi_version(void);
/* hipError_t of the last failed launch of THIS library on the calling thread (0 if none). */
int32_t ts_optim_last_hip_error(void);

/* Process-wide launch-policy knob (speed only: the forms compute the same update and are under the same tests).
 * value >= 0 sets, value < 0 only queries; returns the value before the call, -1 for an unknown key.
 *   TS_OPTIM_TUNE_ONE_BLOCK_MAX   calls of at most this many elements in all take the one-block form; 0: never. */
#define TS_OPTIM_TUNE_ONE_BLOCK_MAX 0
int64_t ts_optim_tuning(int32_t key, int64_t value);

/* Bytes of workspace that a call on total_numel elements can need whatever the knob holds (0 for 0 elements; the grid is
 * bounded, so it is 8 * TS_OPTIM_MAX_BLOCKS otherwise); TS_ERR_ARG for a negative total.  Host only. */
int64_t ts_optim_workspace_bytes(int64_t total_numel);

/* Checks, in this order and before any HIP call:
 *   1. tensors, cfg, out                                                                         TS_ERR_NULL
 *   2. n_tensors outside 0 .. TS_OPTIM_MAX_TENSORS; a negative numel                              TS_ERR_ARG
 *   3. lr, eps or weight_decay negative or NaN; a beta outside [0, 1) or NaN; max_grad_norm negative or NaN   TS_ERR_ARG
 *   4. a total of 0 elements: TS_OK without a launch; grad_norm, where given, is set to 0 by a memset on the stream
 *   5. counters; param, grad, m or v of a tensor with numel > 0; workspace where the form is TS_OPTIM_FORM_MULTI   TS_ERR_NULL
 *   6. an array of a tensor with numel > 0, grad_norm or lr_dev not 4-byte aligned; counters or workspace not 8-byte aligned
 *                                                                                                TS_ERR_ARG
 *   7. two ranges that overlap, at least one of them written.  Written: param, m, v, grad with zero_grad, counters, grad_norm,
 *      the workspace where the form uses it.  Read: grad, lr_dev.                                 TS_ERR_ARG */
int32_t ts_adam_step(const ts_optim_tensors *tensors, const ts_adam_cfg *cfg, const ts_optim_out *out, void *stream);

/* What a call would launch, computed by the code it runs before it launches; touches no device. */
typedef struct ts_optim_desc {
  int32_t form;              /* TS_OPTIM_FORM_* */
  int32_t launches;          /* 1, 3 or 2; 0 where nothing is launched */
  int32_t threads_per_block; /* of the kernel(s) that touch the tensors */
  int32_t lds_bytes;         /* static LDS of such a block */
  int64_t blocks;            /* grid of k_optim_one (1), or of k_optim_norm and k_optim_apply */
  int64_t chunks;            /* pieces of TS_OPTIM_CHUNK (one block: TS_OPTIM_ONE_CHUNK) elements, none across two tensors */
  int64_t total_numel;
  int64_t workspace_bytes;   /* what this form uses: 8 * blocks in TS_OPTIM_FORM_MULTI, else 0 */
  int64_t bytes_read;        /* algorithmic: 4 (grad, norm pass) + 16 (param, grad, m, v) a element; the partials are not counted */
  int64_t bytes_written;     /* 12 (param, m, v) + 4 with zero_grad a element, + 16 (counters) + 4 (grad_norm, with the norm) */
  char name[32];             /* as rocprofv3 prints it: "k_optim_one" or "k_optim_apply" */
  char norm_name[32];        /* "k_optim_norm" in TS_OPTIM_FORM_MULTI, else "" */
  char finish_name[32];      /* "k_optim_finish" in the multi-block forms, else "" */
} ts_optim_desc;
/* `what`: TS_OPTIM_*; bits beyond those, a negative numel or n_tensors outside 0 .. 32 give TS_ERR_ARG, a NULL desc (or a
 * NULL numel with n_tensors > 0) TS_ERR_NULL */
int32_t ts_describe_adam_step(int32_t n_tensors, const int64_t *numel, uint32_t what, ts_optim_desc *desc);

#ifdef __cplusplus
}
#endif
#endif /* TILER_SLIDER_OPTIM_H */
