// ts_train.hip — trainable policies: the logits of a logged trajectory and their gradient (include/tiler_slider_train.h).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_train.so).  The network - stage_weights, static_preact,
// logits_of, the level and cell loads, backward_body - and the host's plans are ts_mlp.h's, shared with ts_policy.hip and
// ts_ac.hip; this file keeps the argument struct, the kernels and the entry points.  tests/test_gpu_train.py holds the forward to
// the rollout's own logits_log bit for bit.
//
// k_train_forward<S>: ONE BOARD PER LANE.  The hs prologue once per board, then K evaluations of logits_of on the cells of
// `first` / `pos_log` (one byte per lane and tile, contiguous across lanes); one 16-byte store per sample.
//
// k_train_backward<S>: ONE WAVE PER BLOCK, a bounded grid, each block striding over groups of 64 boards.  Its cost is the sums
// across boards, so everything that shares a destination is summed on chip first:
//   * a chunk of kChunk steps of the wave's boards (cells, set-semantics mask and dz: 7 registers per step) is held in
//     REGISTERS, the hidden units are walked outside and the chunk's steps inside: for a fixed unit j a lane's running sums are
//     five registers (sum_k h_j dz_a, sum_k dp_j).  The four sums of w2's row are reduced across the wave once per (j, chunk),
//     not once per step, and added to the block's accumulator in LDS by lane 0.
//   * sum_k dp_j of a board is kept in LDS as the lane's column sd[j][lane] across the chunks: it is exactly what every CONSTANT
//     feature of that board (obstacles, targets) and b1 receive.  It is scattered once per board and unit, the mirror of
//     static_preact's walk over the mask bits.
//   * tile features get dp_j per step at acc[j][slot] by LDS atomic adds (ds_add_f32; a cell counts once, as in logits_of;
//     exact zeros - half the units of a ReLU layer - are skipped).
//   * the block's accumulators live in LDS where they fit: the whole gradient of w1 as [j][feature] (feature-contiguous, so
//     that lanes on different cells hit different banks; the row stride is made odd so that the flush, which reads along j, is
//     conflict-free too), else its tile planes only, else nothing - then every add to w1's gradient is a global atomic.  The
//     gradients of b1, w2, b2 always are in LDS.  Everything in LDS is flushed once per block by atomic wave instructions over
//     contiguous 256-byte rows, skipping exact zeros (rows no sample has are never written).
// Gradient accumulators are given LDS before the staged tile-plane weights are: a gathered weight is a cached read, a gradient
// that is not in LDS is a global atomic per lane.
#include "../../include/tiler_slider_train.h"
#include "ts_mlp.h"

namespace {

struct TArgs {
  static constexpr bool kValue = false;  // no value head
  const uint8_t *first, *pos_log, *tgt;  // cell_t = uint8 (S <= 8)
  const uint32_t *blk;
  const float *w1, *b1, *w2, *b2;
  float *logits;
  const float *dz;
  float *gw1, *gb1, *gw2, *gb2;
  int64_t N;
  int32_t T, Tt, mc, steps;
  int32_t H, slots, staged, wt_floats;  // slots: T' * S*S; wt_floats: LDS floats of the staged tile-plane weights
  int32_t D, mode, acc_stride;          // backward: features, grads_in_lds, the odd row stride of the w1 accumulator
};

template <int S>
__global__ __launch_bounds__(kMaxThreads) void k_train_forward(const TArgs a) {
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
    float z[4];
    logits_of<S, MT>(a, hs, pc, z);
    if (live) reinterpret_cast<float4 *>(a.logits)[(int64_t)k * N + n] = make_float4(z[0], z[1], z[2], z[3]);
  }
}

template <int S>
__global__ __launch_bounds__(kWave, 2) void k_train_backward(const TArgs a) {
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
  return ts::by_size<Kernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> Kernel { return k_train_forward<s>; });
}
Kernel backward_kernel(int S) {
  return ts::by_size<Kernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> Kernel { return k_train_backward<s>; });
}
constexpr TrainKernels<TArgs> kKernels{"k_train_forward", "k_train_backward", forward_kernel, backward_kernel, 16};

bool inputs_complete(const ts_dims *d, const ts_state *st, const ts_mlp *mlp, const ts_train_in *in) {
  return st && mlp_complete(mlp) && st->blk && (d->n_targets == 0 || st->tgt) && (d->n_tiles == 0 || in->first) &&
         (d->n_tiles == 0 || in->steps == 1 || in->pos_log);
}

void fill_common(TArgs &a, const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_train_in *in, const TrainPlan &p) {
  a.first = static_cast<const uint8_t *>(in->first), a.pos_log = static_cast<const uint8_t *>(in->pos_log);
  a.tgt = static_cast<const uint8_t *>(st->tgt), a.blk = st->blk;
  a.w1 = mlp->w1, a.b1 = mlp->b1, a.w2 = mlp->w2, a.b2 = mlp->b2;
  a.N = dims->n_boards;
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color, a.steps = in->steps;
  a.H = mlp->hidden, a.slots = p.slots, a.staged = p.staged, a.wt_floats = p.wt_floats;
  a.D = p.D, a.mode = p.mode, a.acc_stride = p.acc_stride;
}

}  // namespace

extern "C" {

int32_t ts_train_abi_version(void) { return TS_TRAIN_ABI_VERSION; }
int32_t ts_train_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_train_supported(const ts_dims *dims, int32_t hidden) { return supported(dims, hidden); }

int32_t ts_describe_train_forward(const ts_dims *dims, int32_t hidden, int32_t steps, ts_train_desc *desc) {
  return describe_train(dims, hidden, steps, false, kKernels, desc);
}
int32_t ts_describe_train_backward(const ts_dims *dims, int32_t hidden, int32_t steps, ts_train_desc *desc) {
  return describe_train(dims, hidden, steps, true, kKernels, desc);
}

int32_t ts_train_forward(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_train_in *in, float *logits, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!mlp || !in) return TS_ERR_NULL;
  TrainPlan p;
  if (const int32_t rc = plan_train(dims, mlp->hidden, in->steps, false, kKernels, p); rc != TS_OK) return rc;
  if (!p.kernel) return TS_OK;  // an empty batch
  if (!inputs_complete(dims, st, mlp, in) || !logits) return TS_ERR_NULL;
  if ((uintptr_t)logits & 15u) return TS_ERR_ARG;
  TArgs a{};
  fill_common(a, dims, st, mlp, in, p);
  a.logits = logits;
  hipLaunchKernelGGL(p.kernel, dim3(p.blocks), dim3(p.threads), p.lds, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

int32_t ts_train_backward(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_train_in *in, const float *dlogits,
                          const ts_mlp_grad *grad, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!mlp || !in) return TS_ERR_NULL;
  TrainPlan p;
  if (const int32_t rc = plan_train(dims, mlp->hidden, in->steps, true, kKernels, p); rc != TS_OK) return rc;
  if (!p.kernel) return TS_OK;  // an empty batch
  if (!inputs_complete(dims, st, mlp, in) || !dlogits || !grad || !grad->w1 || !grad->b1 || !grad->w2 || !grad->b2) return TS_ERR_NULL;
  if ((uintptr_t)dlogits & 15u) return TS_ERR_ARG;
  TArgs a{};
  fill_common(a, dims, st, mlp, in, p);
  a.dz = dlogits;
  a.gw1 = grad->w1, a.gb1 = grad->b1, a.gw2 = grad->w2, a.gb2 = grad->b2;
  hipLaunchKernelGGL(p.kernel, dim3(p.blocks), dim3(p.threads), p.lds, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

}  // extern "C"
