// ts_lookahead.hip — lookahead: a network's values backed up through a full-width search of the exact environment
// (include/tiler_slider_lookahead.h).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_lookahead.so).  The network and the host's block plan
// are ts_mlp.h's, unchanged, with the value head on (LArgs::kValue): stage_weights and static_preact once per board, then 4^D
// calls of logits_of per sample on cells that never leave registers.
//
// k_lookahead<S, D>: ONE SAMPLE PER LANE AND STEP, as k_ac_forward.  D is a template parameter because the ply stack - the cells,
// the running maximum and the running win distance of each ply - must be named registers: search_node<S, P> calls
// search_node<S, P - 1> from inside its loop over the four actions, every instance force-inlined with locals of its own, so the
// kernel is D nested loops with the leaf evaluation once, innermost.  The loops are kept rolled (the action is a scalar of the
// wave), so the code of D = 4 is four slides and one network, not 340 and 256.  Control flow is uniform: every lane walks the
// same 4^D action sequences in the same order, and a lane whose node has won walks the subtree below it all the same and drops
// its value in a select.  The four root values are kept by selects on the scalar action, never in an indexed array.
//
// The leaf kind is a uniform branch (a.leaf), not a template parameter: 32 kernels.  QMAX evaluates the network with the value
// head too and drops v; the host points wv and bv at w2 and b2 then (H and 1 readable floats), so no head is needed.
#include "../../include/tiler_slider_lookahead.h"
#include "ts_mlp.h"

namespace {

struct LArgs {
  static constexpr bool kValue = true;   // the value head
  const uint8_t *first, *pos_log, *tgt;  // cell_t = uint8 (S <= 8)
  const uint32_t *blk;
  const float *w1, *b1, *w2, *b2, *wv, *bv;
  float *q, *value;
  uint8_t *best, *win_in;
  int64_t N;
  int32_t T, Tt, mc, steps;
  int32_t H, slots, staged, wt_floats;
  int32_t leaf;
  float gamma, w_step, w_win, w_invalid;
};

// the win test of ts_step on the cells c[] (ts_policy.hip: state.py:172-186)
template <int S, int MT>
__device__ __forceinline__ bool won_on(const LArgs &a, const Level<S> &b, const uint32_t (&c)[MT]) {
  using M = typename Level<S>::M;
  bool ordered = a.T == a.Tt;
  M occ = 0;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (t < a.T) {
      ordered &= c[t] == b.tg[t];
      occ |= M(1) << c[t];
    }
  }
  return a.mc ? ordered : (occ == b.tgm);
}

// L(c) of the header
template <int S, int MT>
__device__ __forceinline__ float leaf_of(const LArgs &a, Hs &hs, const uint32_t (&c)[MT]) {
  if (a.leaf == TS_LOOKAHEAD_LEAF_ZERO) return 0.0f;  // uniform
  float z[4], v;
  logits_of<S, MT>(a, hs, c, z, v);
  return a.leaf == TS_LOOKAHEAD_LEAF_VALUE ? v : fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
}

template <int S, int P>
__device__ __forceinline__ void search_node(const LArgs &a, Hs &hs, const Level<S> &b, uint64_t cells, float &best_q, uint32_t &win);

// Q_P(c, dir) and the plies to the nearest win through that action (0: none within P).  A ply's cells travel packed, a byte per
// tile, and are unpacked behind an empty asm: without it the compiler hoists everything a slide derives from the cells alone -
// rows, columns, line masks, eight tiles' worth per ply - out of the loops over the actions, and the kernels of depth 3 and 4
// need more than 256 registers.
template <int S, int P>
__device__ __forceinline__ void search_child(const LArgs &a, Hs &hs, const Level<S> &b, uint64_t cells, int dir, float &q, uint32_t &win) {
  using M = typename Level<S>::M;
  constexpr int MT = max_tiles<S>();
  asm volatile("" : "+v"(cells));
  uint32_t c[MT];
  M occ = 0;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    c[t] = (uint32_t)(cells >> (8 * t)) & 0xffu;
    if (t < a.T) occ |= M(1) << c[t];
  }
  uint32_t n[MT];
  uint64_t next = 0;
  bool same = true;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    n[t] = c[t];
    if (t < a.T) n[t] = (uint32_t)ts::slide_cell<S>((int)c[t], occ, b.blk, dir);
    same &= n[t] == c[t];
    next |= (uint64_t)n[t] << (8 * t);
  }
  const bool won = won_on<S, MT>(a, b, n);
  const float r = a.w_step + (won ? a.w_win : 0.0f) + (same ? a.w_invalid : 0.0f);
  float x;
  uint32_t below = 0;
  if constexpr (P == 1)
    x = leaf_of<S, MT>(a, hs, n);
  else
    search_node<S, P - 1>(a, hs, b, next, x, below);
  q = fmaf(a.gamma, won ? 0.0f : x, r);
  win = won ? 1u : below ? below + 1u : 0u;
}

// max_a Q_P(c, a) and the plies to the nearest win below c
template <int S, int P>
__device__ __forceinline__ void search_node(const LArgs &a, Hs &hs, const Level<S> &b, uint64_t cells, float &best_q, uint32_t &win) {
  float m = -INFINITY;
  uint32_t w = 0;
#pragma unroll 1
  for (int dir = 0; dir < 4; ++dir) {
    float q;
    uint32_t wa;
    search_child<S, P>(a, hs, b, cells, dir, q, wa);
    m = fmaxf(m, q);
    w = wa && (!w || wa < w) ? wa : w;
  }
  best_q = m, win = w;
}

template <int S, int D>
__global__ __launch_bounds__(kMaxThreads) void k_lookahead(const LArgs a) {
  constexpr int C = S * S, MT = max_tiles<S>();
  const bool net = a.leaf != TS_LOOKAHEAD_LEAF_ZERO;  // uniform
  if (net) stage_weights(a, C);
  const int64_t N = a.N;
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n - (int64_t)(threadIdx.x & (kWave - 1)) >= N) return;  // wave-uniform
  const bool live = n < N;
  const int64_t nl = live ? n : N - 1;
  Level<S> b;
  load_level<S>(a, nl, b);
  Hs hs(g_lds + head_floats<LArgs::kValue>(a.H) + a.wt_floats + threadIdx.x, (int)blockDim.x);
  if (net) static_preact<S>(a, hs, b.blk, b.tgm, b.tg);
  for (int k = 0; k < a.steps; ++k) {
    uint32_t pc[MT];  // written out, as in k_ac_forward
#pragma unroll
    for (int t = 0; t < MT; ++t) pc[t] = 0;
    if (a.T > 0) {
      const uint8_t *src = cells_of(a, k);
#pragma unroll
      for (int t = 0; t < MT; ++t) pc[t] = src[(int64_t)min(t, a.T - 1) * N + nl];
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) pc[t] = min(pc[t], (uint32_t)(C - 1));
    const bool won = won_on<S, MT>(a, b, pc);
    uint64_t cells = 0;
#pragma unroll
    for (int t = 0; t < MT; ++t) cells |= (uint64_t)pc[t] << (8 * t);
    float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, q3 = 0.0f;
    uint32_t win = 0;
#pragma unroll 1
    for (int dir = 0; dir < 4; ++dir) {  // the root keeps all four: selects on the scalar action
      float q;
      uint32_t wa;
      search_child<S, D>(a, hs, b, cells, dir, q, wa);
      q0 = dir == 0 ? q : q0, q1 = dir == 1 ? q : q1, q2 = dir == 2 ? q : q2, q3 = dir == 3 ? q : q3;
      win = wa && (!win || wa < win) ? wa : win;
    }
    if (won) q0 = q1 = q2 = q3 = 0.0f, win = 0;
    uint32_t best = 0;
    float v = q0;
    if (q1 > v) v = q1, best = 1;
    if (q2 > v) v = q2, best = 2;
    if (q3 > v) v = q3, best = 3;
    if (won) best = TS_LOOKAHEAD_NO_ACTION;
    if (live) {
      const int64_t i = (int64_t)k * N + n;
      if (a.q) reinterpret_cast<float4 *>(a.q)[i] = make_float4(q0, q1, q2, q3);
      if (a.value) a.value[i] = v;
      if (a.best) a.best[i] = (uint8_t)best;
      if (a.win_in) a.win_in[i] = (uint8_t)win;
    }
  }
}

using Kernel = void (*)(const LArgs);
using LookPlan = Plan<LArgs, ts_lookahead_desc>;

template <int S>
Kernel kernel_of_depth(int D) {
  return ts::by_size<Kernel, 1, 2, 3, 4>(D, [](auto d) -> Kernel { return k_lookahead<S, d>; });
}
Kernel kernel_of(int S, int D) {
  return ts::by_size<Kernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [D](auto s) -> Kernel { return kernel_of_depth<s>(D); });
}
static_assert(TS_LOOKAHEAD_MAX_DEPTH == 4, "kernel_of_depth lists the depths");

inline bool leaf_known(int32_t leaf) { return leaf == TS_LOOKAHEAD_LEAF_ZERO || leaf == TS_LOOKAHEAD_LEAF_VALUE || leaf == TS_LOOKAHEAD_LEAF_QMAX; }
inline bool leaf_reads_network(int32_t leaf) { return leaf == TS_LOOKAHEAD_LEAF_VALUE || leaf == TS_LOOKAHEAD_LEAF_QMAX; }

// Every check that needs no pointer, and the launch the call would make.  `hidden` is read with a network leaf only.
int32_t plan_lookahead(const ts_dims *d, int32_t hidden, int32_t steps, int32_t depth, int32_t leaf, float gamma, LookPlan &p) {
  if (const int32_t rc = ts::check_dims(d); rc != TS_OK) return rc;
  const bool net = leaf_reads_network(leaf);
  if (!shape_supported(d, net ? hidden : 1)) return TS_ERR_LIMIT;
  if (steps < 1 || steps > TS_ROLLOUT_MAX_STEPS || depth < 1 || depth > TS_LOOKAHEAD_MAX_DEPTH || !leaf_known(leaf) || !(gamma >= 0.0f && gamma <= 1.0f))
    return TS_ERR_ARG;
  if (net)
    plan_forward_block(d, hidden, p);
  else
    p.threads = kMaxThreads, p.lds = 0, p.staged = 0, p.wt_floats = 0, p.slots = 0;
  p.desc.threads_per_block = (int32_t)p.threads;
  p.desc.lds_bytes = (int32_t)p.lds;
  p.desc.weights_in_lds = p.staged;
  p.desc.leaf_is_template = 0;
  p.desc.depth = depth;
  p.desc.samples = (int64_t)steps * d->n_boards;
  p.desc.leaves = p.desc.samples << (2 * depth);
  if (d->n_boards == 0) return TS_OK;  // nothing is launched
  const int64_t blocks = (d->n_boards + p.threads - 1) / p.threads;
  p.kernel = kernel_of(d->size, depth);
  if (!p.kernel || blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  p.blocks = (uint32_t)blocks;
  p.desc.blocks = blocks;
  snprintf(p.desc.name, sizeof p.desc.name, "k_lookahead<%d, %d>", d->size, depth);
  return TS_OK;
}

}  // namespace

extern "C" {

int32_t ts_lookahead_abi_version(void) { return TS_LOOKAHEAD_ABI_VERSION; }
int32_t ts_lookahead_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_lookahead_supported(const ts_dims *dims, int32_t hidden, int32_t leaf) {
  const int32_t rc = supported(dims, leaf_reads_network(leaf) ? hidden : 1);
  if (rc < 0) return rc;
  return leaf_known(leaf) ? rc : TS_ERR_ARG;
}

int32_t ts_describe_lookahead(const ts_dims *dims, int32_t hidden, int32_t steps, int32_t depth, int32_t leaf, ts_lookahead_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  LookPlan p;
  if (const int32_t rc = plan_lookahead(dims, hidden, steps, depth, leaf, 0.0f, p); rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_lookahead(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_value_head *head, const ts_train_in *in,
                     const ts_lookahead_cfg *cfg, const ts_lookahead_out *out, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!in || !cfg || !out) return TS_ERR_NULL;
  const bool net = leaf_reads_network(cfg->leaf);
  if (net && !mlp) return TS_ERR_NULL;
  LookPlan p;
  if (const int32_t rc = plan_lookahead(dims, net ? mlp->hidden : 1, in->steps, cfg->depth, cfg->leaf, cfg->gamma, p); rc != TS_OK) return rc;
  if (!p.kernel) return TS_OK;  // an empty batch
  const bool value_leaf = cfg->leaf == TS_LOOKAHEAD_LEAF_VALUE;
  if (!st || !st->blk || (dims->n_targets > 0 && !st->tgt) || (dims->n_tiles > 0 && !in->first) ||
      (dims->n_tiles > 0 && in->steps > 1 && !in->pos_log) || (net && !mlp_complete(mlp)) || (value_leaf && (!head || !head->wv || !head->bv)) ||
      (!out->q && !out->value && !out->best && !out->win_in))
    return TS_ERR_NULL;
  if (((uintptr_t)out->q & 15u) || ((uintptr_t)out->value & 3u)) return TS_ERR_ARG;
  LArgs a{};
  a.first = static_cast<const uint8_t *>(in->first), a.pos_log = static_cast<const uint8_t *>(in->pos_log);
  a.tgt = static_cast<const uint8_t *>(st->tgt), a.blk = st->blk;
  if (net) {
    a.w1 = mlp->w1, a.b1 = mlp->b1, a.w2 = mlp->w2, a.b2 = mlp->b2, a.H = mlp->hidden;
    // QMAX drops v: the head's H + 1 floats are read from the second layer's own 4 H + 4
    a.wv = value_leaf ? head->wv : mlp->w2, a.bv = value_leaf ? head->bv : mlp->b2;
  }
  a.q = out->q, a.value = out->value, a.best = out->best, a.win_in = out->win_in;
  a.N = dims->n_boards;
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color, a.steps = in->steps;
  a.slots = p.slots, a.staged = p.staged, a.wt_floats = p.wt_floats;
  a.leaf = cfg->leaf;
  a.gamma = cfg->gamma, a.w_step = cfg->w_step, a.w_win = cfg->w_win, a.w_invalid = cfg->w_invalid;
  hipLaunchKernelGGL(p.kernel, dim3(p.blocks), dim3(p.threads), p.lds, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

}  // extern "C"
