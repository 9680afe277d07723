// ts_ac.hip — the actor-critic network: the logits and the value of a logged trajectory and their gradient
// (include/tiler_slider_ac.h).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_ac.so).  The network and the host's plans are
// ts_mlp.h's, shared with ts_policy.hip and ts_train.hip; TArgs::kValue switches the value head on in them - wv and bv staged
// behind b2, a fifth accumulator beside z, one more column in the backward.  z still comes out of the same sequence of float
// operations: tests/test_gpu_ac.py holds it to the rollout's own logits_log bit for bit.
//
// k_ac_forward<S>: ONE BOARD PER LANE.  The hs prologue once per board, then K evaluations of logits_of on the cells of
// `first` / `pos_log` (one byte per lane and tile, contiguous across lanes); one 16-byte and one 4-byte store per sample.
//
// k_ac_backward<S>: k_train_backward's design (ts_train.hip's file comment) with one more column: the
// chunk holds dv beside dz (8 registers per step), a lane's running sums for a unit j are six (sum_k h_j dv joins them) and are
// reduced across the wave once per (j, chunk), and the gradients of wv and bv join those of b1, w2 and b2 in LDS, flushed once
// per block.  Gradient accumulators are given LDS before the staged tile-plane weights are, as in ts_train.hip.
#include "../../include/tiler_slider_ac.h"
#include "ts_mlp.h"

namespace {

struct TArgs {
  static constexpr bool kValue = true;  // the value head
  const uint8_t *first, *pos_log, *tgt;  // cell_t = uint8 (S <= 8)
  const uint32_t *blk;
  const float *w1, *b1, *w2, *b2, *wv, *bv;
  float *logits, *values;
  const float *dz, *dv;
  float *gw1, *gb1, *gw2, *gb2, *gwv, *gbv;
  int64_t N;
  int32_t T, Tt, mc, steps;
  int32_t H, slots, staged, wt_floats;  // slots: T' * S*S; wt_floats: LDS floats of the staged tile-plane weights
  int32_t D, mode, acc_stride;          // backward: features, grads_in_lds, the odd row stride of the w1 accumulator
};

template <int S>
__global__ __launch_bounds__(kMaxThreads) void k_ac_forward(const TArgs a) {
  constexpr int C = S * S, MT = max_tiles<S>();
  stage_weights(a, C);
  const int64_t N = a.N;
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n - (int64_t)(threadIdx.x & (kWave - 1)) >= N) return;  // wave-uniform
  const bool live = n < N;
  const int64_t nl = live ? n : N - 1;
  Level<S> b;
  load_level<S>(a, nl, b);
  Hs hs(g_lds + head_floats<TArgs::kValue>(a.H) + a.wt_floats + threadIdx.x, (int)blockDim.x);
  static_preact<S>(a, hs, b.blk, b.tgm, b.tg);
  for (int k = 0; k < a.steps; ++k) {
    uint32_t pc[MT];  // written out, as in backward_body: a shared function changed these kernels by 2 to 9 instructions
#pragma unroll
    for (int t = 0; t < MT; ++t) pc[t] = 0;
    if (a.T > 0) {
      const uint8_t *src = cells_of(a, k);
#pragma unroll
      for (int t = 0; t < MT; ++t) pc[t] = src[(int64_t)min(t, a.T - 1) * N + nl];
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) pc[t] = min(pc[t], (uint32_t)(C - 1));
    float z[4], v;
    logits_of<S, MT>(a, hs, pc, z, v);
    if (live) {
      reinterpret_cast<float4 *>(a.logits)[(int64_t)k * N + n] = make_float4(z[0], z[1], z[2], z[3]);
      a.values[(int64_t)k * N + n] = v;
    }
  }
}

template <int S>
__global__ __launch_bounds__(kWave, 2) void k_ac_backward(const TArgs a) {
  if (a.staged) {
    if (a.mode == 2) backward_body<S, true, 2>(a);
    else if (a.mode == 1) backward_body<S, true, 1>(a);
    else backward_body<S, true, 0>(a);
  } else {
    if (a.mode == 2) backward_body<S, false, 2>(a);
    else if (a.mode == 1) backward_body<S, false, 1>(a);
    else backward_body<S, false, 0>(a);
  }
}

using Kernel = void (*)(const TArgs);
using TrainPlan = Plan<TArgs, ts_train_desc>;

Kernel forward_kernel(int S) {
  return ts::by_size<Kernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> Kernel { return k_ac_forward<s>; });
}
Kernel backward_kernel(int S) {
  return ts::by_size<Kernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> Kernel { return k_ac_backward<s>; });
}
constexpr TrainKernels<TArgs> kKernels{"k_ac_forward", "k_ac_backward", forward_kernel, backward_kernel, 20};

bool inputs_complete(const ts_dims *d, const ts_state *st, const ts_mlp *mlp, const ts_value_head *head, const ts_train_in *in) {
  return st && mlp_complete(mlp) && head && head->wv && head->bv && st->blk && (d->n_targets == 0 || st->tgt) &&
         (d->n_tiles == 0 || in->first) && (d->n_tiles == 0 || in->steps == 1 || in->pos_log);
}

void fill_common(TArgs &a, const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_value_head *head, const ts_train_in *in,
                 const TrainPlan &p) {
  a.first = static_cast<const uint8_t *>(in->first), a.pos_log = static_cast<const uint8_t *>(in->pos_log);
  a.tgt = static_cast<const uint8_t *>(st->tgt), a.blk = st->blk;
  a.w1 = mlp->w1, a.b1 = mlp->b1, a.w2 = mlp->w2, a.b2 = mlp->b2, a.wv = head->wv, a.bv = head->bv;
  a.N = dims->n_boards;
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color, a.steps = in->steps;
  a.H = mlp->hidden, a.slots = p.slots, a.staged = p.staged, a.wt_floats = p.wt_floats;
  a.D = p.D, a.mode = p.mode, a.acc_stride = p.acc_stride;
}

}  // namespace

extern "C" {

int32_t ts_ac_abi_version(void) { return TS_AC_ABI_VERSION; }
int32_t ts_ac_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_ac_supported(const ts_dims *dims, int32_t hidden) { return supported(dims, hidden); }

int32_t ts_describe_ac_forward(const ts_dims *dims, int32_t hidden, int32_t steps, ts_train_desc *desc) {
  return describe_train(dims, hidden, steps, false, kKernels, desc);
}
int32_t ts_describe_ac_backward(const ts_dims *dims, int32_t hidden, int32_t steps, ts_train_desc *desc) {
  return describe_train(dims, hidden, steps, true, kKernels, desc);
}

int32_t ts_ac_forward(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_value_head *head, const ts_train_in *in,
                      float *logits, float *values, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!mlp || !in) return TS_ERR_NULL;
  TrainPlan p;
  if (const int32_t rc = plan_train(dims, mlp->hidden, in->steps, false, kKernels, p); rc != TS_OK) return rc;
  if (!p.kernel) return TS_OK;  // an empty batch
  if (!inputs_complete(dims, st, mlp, head, in) || !logits || !values) return TS_ERR_NULL;
  if (((uintptr_t)logits & 15u) || ((uintptr_t)values & 3u)) return TS_ERR_ARG;
  TArgs a{};
  fill_common(a, dims, st, mlp, head, in, p);
  a.logits = logits, a.values = values;
  hipLaunchKernelGGL(p.kernel, dim3(p.blocks), dim3(p.threads), p.lds, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

int32_t ts_ac_backward(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_value_head *head, const ts_train_in *in,
                       const float *dlogits, const float *dvalues, const ts_mlp_grad *grad, const ts_value_head_grad *head_grad,
                       void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!mlp || !in) return TS_ERR_NULL;
  TrainPlan p;
  if (const int32_t rc = plan_train(dims, mlp->hidden, in->steps, true, kKernels, p); rc != TS_OK) return rc;
  if (!p.kernel) return TS_OK;  // an empty batch
  if (!inputs_complete(dims, st, mlp, head, in) || !dlogits || !dvalues || !grad || !grad->w1 || !grad->b1 || !grad->w2 || !grad->b2 ||
      !head_grad || !head_grad->wv || !head_grad->bv)
    return TS_ERR_NULL;
  if (((uintptr_t)dlogits & 15u) || ((uintptr_t)dvalues & 3u)) return TS_ERR_ARG;
  TArgs a{};
  fill_common(a, dims, st, mlp, head, in, p);
  a.dz = dlogits, a.dv = dvalues;
  a.gw1 = grad->w1, a.gb1 = grad->b1, a.gw2 = grad->w2, a.gb2 = grad->b2, a.gwv = head_grad->wv, a.gbv = head_grad->bv;
  hipLaunchKernelGGL(p.kernel, dim3(p.blocks), dim3(p.threads), p.lds, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

}  // extern "C"
