// ts_policy.hip — neural-policy rollouts: K steps, an MLP picks every action, one launch (include/tiler_slider_policy.h).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_policy.so): the step, search, table and rollout
// libraries are pinned symbol by symbol and kernel by kernel, and nothing here touches any of them.
//
// k_policy_rollout<S, SELECT>: ONE BOARD PER LANE, as k_rollout (ts_rollout.hip).  The step body below - clamp, slide, win test,
// done / auto-reset, reductions, logs, the strict-mode early exit and its tail - is a COPY of k_rollout's RANDOM path, not a
// shared header: lifting the reward and the done / slide / flags block into functions both files call was tried, and it changed
// all 24 k_rollout kernels (a VGPR or two more in 17 of them, instruction counts by -33 to +11 %: DESIGN.md section 14), which the
// rule for this library forbids.  The exact-rollout tests of tests/test_gpu_policy.py hold this copy to the same oracle loop
// byte for byte.
//
// What is new is the network.  Its input, the one-hot planes of a board, is sparse and mostly constant:
//   * prologue, once per board: hs[j] = b1[j] + sum over obstacle cells p of w1[p][j] + sum over target features f of w1[f][j]
//     (single colour: over the bits of the target mask - set semantics).  w1 is read through L2; hs lives in LDS as
//     [j][thread], a lane's own column - no barrier, no bank conflict (consecutive lanes, consecutive banks).
//     (hs in up to 64 registers was measured and dropped: it spilled and ran slower)
//   * per step, for every hidden unit j (a uniform loop): h = relu(hs[j] + sum over tiles of w1t[j][slot]); z[a] += h * w2[j][a].
//     The w2 rows and b2 are uniform; they are staged once per block at the front of LDS and read as one broadcast 16-byte
//     read per hidden unit.  (Read from global memory the compiler would not use scalar loads - the kernel also stores to global
//     memory, so the rows are not provably invariant - and every j paid an exposed L2 round trip: DESIGN.md section 15.)  slot = the tile's cell (single colour; a cell two tiles share counts once), or
//     t * S*S + cell (multi colour).
//   * the tile-plane weights w1t, H * T' * S*S floats (T' = T multi colour, 1 single colour), are staged once per block in LDS,
//     laid out [j][slot]: lanes on different cells read different banks, lanes on equal cells are a broadcast.  Where they do not
//     fit beside hs in the 64 KiB a block may ask for (ts_launch.h), they are gathered from global memory instead - a decision
//     of plan(), not a limit.
//
// The network - stage_weights, static_preact, logits_of - and the block plan are ts_mlp.h's, shared with ts_train.hip and
// ts_ac.hip.
#include "../../include/tiler_slider_policy.h"
#include "ts_mlp.h"

namespace {

struct PArgs {
  static constexpr bool kValue = false;  // no value head
  uint8_t *pos;  // cell_t = uint8 (S <= 8)
  const uint8_t *init, *tgt;
  const uint32_t *blk;
  int32_t *step_count;
  uint8_t *done;
  const float *w1, *b1, *w2, *b2;
  int32_t *wins, *finished, *first_win, *win_moves, *reward_sum;  // each output may be NULL
  uint8_t *flags, *act_log, *flags_log, *pos_log;
  float *logits_log, *logits;
  int64_t N, step_index, board_offset;
  uint64_t seed, threshold;
  int32_t T, Tt, mc, max_steps, steps, autoreset, write_state;
  int32_t H, slots, staged, wt_floats;  // slots: T' * S*S; wt_floats: LDS floats of the staged tile-plane weights
};

// e of the definition; <= 3 whatever z holds
template <int SELECT>
__device__ __forceinline__ uint32_t select_action(const float (&z)[4], uint64_t r) {
  const float m = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
  if constexpr (SELECT == TS_POLICY_GREEDY) {
    return z[0] == m ? 0u : z[1] == m ? 1u : z[2] == m ? 2u : 3u;
  } else {
    const float c0 = __expf(z[0] - m), c1 = c0 + __expf(z[1] - m), c2 = c1 + __expf(z[2] - m), c3 = c2 + __expf(z[3] - m);
    const float u = (float)(uint32_t)((r >> 32) & 0xffffffu) * 0x1p-24f;
    const float x = u * c3;
    return x < c0 ? 0u : x < c1 ? 1u : x < c2 ? 2u : 3u;
  }
}

template <int S>
struct Board {
  using M = typename ts::Bitboard<S>::mask_t;
  static constexpr int MT = max_tiles<S>();
  M blk, tgm;
  uint32_t p[MT], in[MT], tg[kMaxTargets];
};

// the board of lane nl: obstacles, targets, cells as they lie in memory, and (auto-reset) the clamped initial cells
// (the obstacle and target part is ts_mlp.h's load_level, written out: calling it changed 23 of the 24 kernels here)
template <int S>
__device__ __forceinline__ void load_board(const PArgs &a, int64_t nl, bool want_init, Board<S> &b) {
  using M = typename Board<S>::M;
  constexpr int C = S * S, MT = Board<S>::MT;
  constexpr M kFull = C == 64 ? ~M(0) : (M(1) << (C & 63)) - 1;
  const int64_t N = a.N;
  b.blk = ts::load_obstacles<S>(a.blk, N, nl) & kFull;
#pragma unroll
  for (int t = 0; t < MT; ++t) b.p[t] = 0, b.in[t] = 0;
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) b.tg[j] = 0;
  // loads go out unconditionally, all before the first one is consumed: rows past the count read the last row, results unused
  if (a.T > 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t) b.p[t] = a.pos[(int64_t)min(t, a.T - 1) * N + nl];
    if (want_init) {
#pragma unroll
      for (int t = 0; t < MT; ++t) b.in[t] = a.init[(int64_t)min(t, a.T - 1) * N + nl];
    }
  }
  if (a.Tt > 0) {
#pragma unroll
    for (int j = 0; j < kMaxTargets; ++j) b.tg[j] = a.tgt[(int64_t)min(j, a.Tt - 1) * N + nl];
  }
  b.tgm = 0;
#pragma unroll
  for (int t = 0; t < MT; ++t) b.in[t] = min(b.in[t], (uint32_t)(C - 1));
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) {
    b.tg[j] = min(b.tg[j], (uint32_t)(C - 1));
    if (j < a.Tt) b.tgm |= M(1) << b.tg[j];
  }
}

template <int S>
__global__ __launch_bounds__(kMaxThreads) void k_policy_logits(const PArgs a) {
  constexpr int C = S * S, MT = Board<S>::MT;
  stage_weights(a, C);
  const int64_t N = a.N;
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n - (int64_t)(threadIdx.x & (kWave - 1)) >= N) return;  // wave-uniform
  const bool live = n < N;
  const int64_t nl = live ? n : N - 1;
  Board<S> b;
  load_board<S>(a, nl, false, b);
  Hs hs(g_lds + head_floats<PArgs::kValue>(a.H) + a.wt_floats + threadIdx.x, (int)blockDim.x);
  static_preact<S>(a, hs, b.blk, b.tgm, b.tg);
  uint32_t pc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) pc[t] = min(b.p[t], (uint32_t)(C - 1));
  float z[4];
  logits_of<S, MT>(a, hs, pc, z);
  if (live) reinterpret_cast<float4 *>(a.logits)[n] = make_float4(z[0], z[1], z[2], z[3]);
}

template <int S, int SELECT>
__global__ __launch_bounds__(kMaxThreads) void k_policy_rollout(const PArgs a) {
  using M = typename Board<S>::M;
  constexpr int C = S * S, MT = Board<S>::MT;

  stage_weights(a, C);
  const int64_t N = a.N;
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n - (int64_t)(threadIdx.x & (kWave - 1)) >= N) return;  // wave-uniform
  // lanes past the batch play a copy of the LAST board and write nothing
  const bool live = n < N;
  const int64_t nl = live ? n : N - 1;
  const int T = a.T, Tt = a.Tt, K = a.steps;
  const bool mc = a.mc != 0, autoreset = a.autoreset != 0;

  // ---- the board, once ----
  Board<S> b;
  load_board<S>(a, nl, autoreset, b);
  uint32_t(&p)[MT] = b.p;
  const uint32_t(&in)[MT] = b.in;
  const uint32_t(&tg)[kMaxTargets] = b.tg;
  const M blk = b.blk, tgm = b.tgm;
  int32_t sc = a.step_count[nl];
  uint32_t done = a.done[nl];
  const uint64_t draw = (uint64_t)(a.board_offset + nl) * ts::kDrawMul;

  // ---- the network's constant part, once ----
  Hs hs(g_lds + head_floats<PArgs::kValue>(a.H) + a.wt_floats + threadIdx.x, (int)blockDim.x);
  static_preact<S>(a, hs, blk, tgm, tg);

  // build-defined Manhattan reward of the cells c[] (include/tiler_slider.h: ts_reward)
  auto manhattan = [](uint32_t x, uint32_t y) -> int {
    return abs((int)(x / S) - (int)(y / S)) + abs((int)(x % S) - (int)(y % S));
  };
  auto reward_of = [&](const uint32_t(&c)[MT]) -> int32_t {
    int sum = 0;
    if (mc) {
      const int m = T < Tt ? T : Tt;
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (t < m) sum += manhattan(c[t], tg[t]);
    } else if (Tt > 0) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        if (t < T) {
          int best = 1 << 30;
#pragma unroll
          for (int j = 0; j < kMaxTargets; ++j)
            if (j < Tt) best = min(best, manhattan(c[t], tg[j]));
          sum += best;
        }
      }
    }
    return -sum;
  };
  // the 64-bit draw of (step, board): its top two bits are ts_fill_actions' action
  auto draw_of = [&](int k) -> uint64_t {
    const uint64_t key = ts::mix64(a.seed ^ ((uint64_t)(a.step_index + k) * ts::kBoardMul));  // uniform: a scalar per step
    return ts::mix64(key + draw);
  };
  auto choose = [&](const float(&z)[4], uint64_t r) -> uint32_t {
    const uint32_t e = select_action<SELECT>(z, r);
    const bool explore = (r & 0xffffffffull) < a.threshold;
    return explore ? (uint32_t)(r >> 62) : e;
  };
  const bool want_reward = a.reward_sum != nullptr;  // uniform
  const bool want_logs = a.act_log || a.flags_log || a.pos_log || a.logits_log;
  auto write_logs = [&](int k, uint32_t act, uint32_t flags, const float(&z)[4]) {
    if (!live) return;
    if (a.act_log) a.act_log[(int64_t)k * N + n] = (uint8_t)act;
    if (a.flags_log) a.flags_log[(int64_t)k * N + n] = (uint8_t)flags;
    if (a.pos_log) {
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (t < T) a.pos_log[((int64_t)k * T + t) * N + n] = (uint8_t)p[t];
    }
    if (a.logits_log) reinterpret_cast<float4 *>(a.logits_log)[(int64_t)k * N + n] = make_float4(z[0], z[1], z[2], z[3]);
  };

  int32_t wins = 0, finished = 0, first_win = 0, win_moves = 0, reward_sum = 0;
  uint32_t flags = 0;

  int k = 0;
  for (; k < K; ++k) {
    // strict mode: once every board of the wave is done nothing moves any more - the rest is written by the tail below
    if (!autoreset && __builtin_amdgcn_ballot_w64(done == 0u) == 0) break;

    uint32_t pc[MT];
    M occ = 0;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      pc[t] = min(p[t], (uint32_t)(C - 1));  // clamp: malformed ids stay in-board
      if (t < T) occ |= M(1) << pc[t];
    }

    float z[4];
    logits_of<S, MT>(a, hs, pc, z);
    const uint32_t act = choose(z, draw_of(k));  // <= 3
    const int dir = (int)(act & 3u);
    uint32_t q[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      q[t] = pc[t];
      if (t < T) q[t] = (uint32_t)ts::slide_cell<S>((int)pc[t], occ, blk, dir);
    }

    // ---- ts_step (environment.py:100-143), the order of k_rollout: done on entry, slide ----
    bool same = true, ordered = T == Tt;
    M occ2 = 0;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      if (t < T) {
        same &= q[t] == pc[t];
        ordered &= q[t] == tg[t];
        occ2 |= M(1) << q[t];
      }
    }
    const bool won = mc ? ordered : (occ2 == tgm);  // state.py:172-186
    if (done) {                                     // environment.py:113-114
      flags = autoreset ? TS_FLAG_AUTORESET : TS_FLAG_STEPPED_DONE;
      if (autoreset) {
#pragma unroll
        for (int t = 0; t < MT; ++t) p[t] = in[t];
        sc = 0;
        done = 0;
      }
    } else {
      flags = (won ? (TS_FLAG_IS_WON | TS_FLAG_SUCCESS) : 0u) | (same ? TS_FLAG_INVALID_MOVE : 0u);
      sc += 1;
      done = won ? 1u : 0u;
      if (sc >= a.max_steps) {
        done = 1u;
        flags |= TS_FLAG_TIMEOUT;
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) p[t] = q[t];
    }

    // ---- the reductions ----
    const bool success = (flags & TS_FLAG_SUCCESS) != 0;
    wins += success ? 1 : 0;
    finished += (flags & (TS_FLAG_SUCCESS | TS_FLAG_TIMEOUT)) ? 1 : 0;
    first_win = (success && first_win == 0) ? k + 1 : first_win;
    win_moves += success ? sc : 0;
    if (want_reward) {
      uint32_t c[MT];
#pragma unroll
      for (int t = 0; t < MT; ++t) c[t] = min(p[t], (uint32_t)(C - 1));
      reward_sum += reward_of(c);
    }
    if (want_logs) write_logs(k, act, flags, z);
  }

  // ---- strict mode, every board of the wave done: what the loop would still write, without sliding ----
  if (k < K) {
    flags = TS_FLAG_STEPPED_DONE;
    uint32_t c[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) c[t] = min(p[t], (uint32_t)(C - 1));
    if (want_reward) reward_sum += (K - k) * reward_of(c);
    if (want_logs) {
      float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (a.act_log || a.logits_log) logits_of<S, MT>(a, hs, c, z);  // the board stands still, and so do its logits
      for (; k < K; ++k) write_logs(k, a.act_log ? choose(z, draw_of(k)) : 0u, flags, z);
    }
  }

  if (!live) return;
  if (a.write_state) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
      if (t < T) a.pos[(int64_t)t * N + n] = (uint8_t)p[t];
    a.step_count[n] = sc;
    a.done[n] = (uint8_t)done;
  }
  if (a.wins) a.wins[n] = wins;
  if (a.finished) a.finished[n] = finished;
  if (a.first_win) a.first_win[n] = first_win;
  if (a.win_moves) a.win_moves[n] = win_moves;
  if (a.reward_sum) a.reward_sum[n] = reward_sum;
  if (a.flags) a.flags[n] = (uint8_t)flags;
}

using Kernel = void (*)(const PArgs);

template <int SELECT>
Kernel select_kernel(int S) {
  return ts::by_size<Kernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> Kernel { return k_policy_rollout<s, SELECT>; });
}
Kernel rollout_kernel(int S, int select) {
  return select == TS_POLICY_GREEDY ? select_kernel<TS_POLICY_GREEDY>(S) : select_kernel<TS_POLICY_SAMPLE>(S);
}
Kernel logits_kernel(int S) {
  return ts::by_size<Kernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> Kernel { return k_policy_logits<s>; });
}

bool valid_select(int32_t s) { return s == TS_POLICY_GREEDY || s == TS_POLICY_SAMPLE; }

// valid dims: the random rollout's shapes (a board's dynamic and static state stays in registers), every allowed width
using PolicyPlan = Plan<PArgs, ts_policy_desc>;

void plan_block(const ts_dims *d, int32_t H, PolicyPlan &p) {
  plan_forward_block(d, H, p);
  p.desc.threads_per_block = (int32_t)p.threads;
  p.desc.lds_bytes = (int32_t)p.lds;
  p.desc.weights_in_lds = p.staged;
}

int32_t plan_grid(const ts_dims *d, PolicyPlan &p) {
  const int64_t blocks = (d->n_boards + p.threads - 1) / p.threads;
  if (!p.kernel || blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  p.blocks = (uint32_t)blocks;
  p.desc.blocks = blocks;
  return TS_OK;
}

// Every check of ts_policy_rollout that needs no pointer of st / mlp's parameters / out, and the launch it would make
int32_t plan_rollout(const ts_dims *d, int32_t hidden, const ts_policy_cfg *cfg, uint32_t out_mask, PolicyPlan &p) {
  if (const int32_t rc = ts::check_dims(d); rc != TS_OK) return rc;
  if (!cfg) return TS_ERR_NULL;
  if (!shape_supported(d, hidden)) return TS_ERR_LIMIT;
  if ((cfg->mode & ~TS_MODE_AUTORESET) || !valid_select(cfg->select) || cfg->steps < 0 || cfg->steps > TS_ROLLOUT_MAX_STEPS ||
      cfg->explore_threshold > (1ull << 32))
    return TS_ERR_ARG;
  plan_block(d, hidden, p);
  if (d->n_boards == 0 || cfg->steps == 0) return TS_OK;  // nothing is launched
  const int64_t per_step = ((out_mask & TS_ROLLOUT_OUT_ACT_LOG) ? 1 : 0) + ((out_mask & TS_ROLLOUT_OUT_FLAGS_LOG) ? 1 : 0) +
                           ((out_mask & TS_ROLLOUT_OUT_POS_LOG) ? d->n_tiles : 0) + ((out_mask & TS_POLICY_OUT_LOGITS_LOG) ? 16 : 0);
  p.desc.logged_bytes = per_step * cfg->steps * d->n_boards;
  p.kernel = rollout_kernel(d->size, cfg->select);
  if (const int32_t rc = plan_grid(d, p); rc != TS_OK) return rc;
  snprintf(p.desc.name, sizeof p.desc.name, "k_policy_rollout<%d, %d>", d->size, cfg->select);
  return TS_OK;
}

int32_t plan_logits(const ts_dims *d, int32_t hidden, PolicyPlan &p) {
  if (const int32_t rc = ts::check_dims(d); rc != TS_OK) return rc;
  if (!shape_supported(d, hidden)) return TS_ERR_LIMIT;
  plan_block(d, hidden, p);
  if (d->n_boards == 0) return TS_OK;
  p.desc.logged_bytes = 16 * d->n_boards;
  p.kernel = logits_kernel(d->size);
  if (const int32_t rc = plan_grid(d, p); rc != TS_OK) return rc;
  snprintf(p.desc.name, sizeof p.desc.name, "k_policy_logits<%d>", d->size);
  return TS_OK;
}

void fill_common(PArgs &a, const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const PolicyPlan &p) {
  a.pos = static_cast<uint8_t *>(st->pos), a.init = static_cast<const uint8_t *>(st->init), a.tgt = static_cast<const uint8_t *>(st->tgt);
  a.blk = st->blk, a.step_count = st->step_count, a.done = st->done;
  a.w1 = mlp->w1, a.b1 = mlp->b1, a.w2 = mlp->w2, a.b2 = mlp->b2;
  a.N = dims->n_boards;
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color, a.max_steps = dims->max_steps;
  a.H = mlp->hidden, a.slots = p.slots, a.staged = p.staged, a.wt_floats = p.wt_floats;
}


}  // namespace

extern "C" {

int32_t ts_policy_abi_version(void) { return TS_POLICY_ABI_VERSION; }
int32_t ts_policy_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_policy_supported(const ts_dims *dims, int32_t hidden) { return supported(dims, hidden); }

int32_t ts_describe_policy_rollout(const ts_dims *dims, int32_t hidden, const ts_policy_cfg *cfg, uint32_t out_mask, ts_policy_desc *desc) {
  if (!dims || !cfg || !desc) return TS_ERR_NULL;
  PolicyPlan p;
  const int32_t rc = plan_rollout(dims, hidden, cfg, out_mask, p);
  if (rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_describe_policy_logits(const ts_dims *dims, int32_t hidden, ts_policy_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  PolicyPlan p;
  const int32_t rc = plan_logits(dims, hidden, p);
  if (rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_policy_logits(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, float *logits, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!mlp) return TS_ERR_NULL;
  PolicyPlan p;
  if (const int32_t rc = plan_logits(dims, mlp->hidden, p); rc != TS_OK) return rc;
  if (!p.kernel) return TS_OK;  // an empty batch
  if (!st || !logits || !mlp_complete(mlp) || !st->blk || (dims->n_tiles > 0 && !st->pos) || (dims->n_targets > 0 && !st->tgt)) return TS_ERR_NULL;
  if ((uintptr_t)logits & 15u) return TS_ERR_ARG;
  PArgs a{};
  fill_common(a, dims, st, mlp, p);
  a.logits = logits;
  hipLaunchKernelGGL(p.kernel, dim3(p.blocks), dim3(p.threads), p.lds, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

int32_t ts_policy_rollout(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_policy_cfg *cfg, const ts_policy_out *out,
                          void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!cfg || !mlp) return TS_ERR_NULL;
  const uint32_t mask = !out ? 0u
                             : (out->wins ? TS_ROLLOUT_OUT_WINS : 0u) | (out->finished ? TS_ROLLOUT_OUT_FINISHED : 0u) |
                                   (out->first_win ? TS_ROLLOUT_OUT_FIRST_WIN : 0u) | (out->win_moves ? TS_ROLLOUT_OUT_WIN_MOVES : 0u) |
                                   (out->reward_sum ? TS_ROLLOUT_OUT_REWARD_SUM : 0u) | (out->flags ? TS_ROLLOUT_OUT_FLAGS : 0u) |
                                   (out->act_log ? TS_ROLLOUT_OUT_ACT_LOG : 0u) | (out->flags_log ? TS_ROLLOUT_OUT_FLAGS_LOG : 0u) |
                                   (out->pos_log ? TS_ROLLOUT_OUT_POS_LOG : 0u) | (out->logits_log ? TS_POLICY_OUT_LOGITS_LOG : 0u);
  PolicyPlan p;
  if (const int32_t rc = plan_rollout(dims, mlp->hidden, cfg, mask, p); rc != TS_OK) return rc;
  if (!p.kernel) return TS_OK;  // an empty batch or no step: nothing to launch, no pointer is looked at
  const bool autoreset = (cfg->mode & TS_MODE_AUTORESET) != 0;
  if (!st || !out || !mlp_complete(mlp) || !st->blk || !st->step_count || !st->done || (dims->n_tiles > 0 && !st->pos) ||
      (dims->n_tiles > 0 && autoreset && !st->init) || (dims->n_targets > 0 && !st->tgt) || (mask == 0u && !cfg->write_state))
    return TS_ERR_NULL;
  if ((uintptr_t)out->logits_log & 15u) return TS_ERR_ARG;
  PArgs a{};
  fill_common(a, dims, st, mlp, p);
  a.wins = out->wins, a.finished = out->finished, a.first_win = out->first_win, a.win_moves = out->win_moves, a.reward_sum = out->reward_sum;
  a.flags = out->flags, a.act_log = out->act_log, a.flags_log = out->flags_log, a.pos_log = static_cast<uint8_t *>(out->pos_log);
  a.logits_log = out->logits_log;
  a.step_index = cfg->step_index, a.board_offset = cfg->board_offset;
  a.seed = cfg->seed, a.threshold = cfg->explore_threshold;
  a.steps = cfg->steps, a.autoreset = autoreset ? 1 : 0, a.write_state = cfg->write_state ? 1 : 0;
  hipLaunchKernelGGL(p.kernel, dim3(p.blocks), dim3(p.threads), p.lds, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

}  // extern "C"
